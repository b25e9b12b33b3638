#!/usr/bin/env python3
"""What judging the twin towers on a held-out set costs from the model API on one MI355X, per way of running it.

siamese.py's model (siamese.py:44): 30 layers of dilations 1..512, 32 / 128 channels, D = 2, clips of 5120 samples, bf16.  A
set of N labelled clips is swept once per region; milliseconds per sweep, best of --reps regions with the spread, each path
in regions of its own, each region closed by a device synchronisation, after warm-up sweeps of that path (which include the
capture):

  (a) host loop   get_embedding(x) per batch of host arrays, then NumPy over all pairs: the distance matrix, per record the
                  nearest record and the rank of the nearest record of its label (one argsort per record), the two
                  histograms, and PairEvalResult's metrics from them
  (b) evaluate    model.evaluate(embed_sampler) on a DeviceDataset of the same clips: replays of one graph {draw, forward
                  pass, srwn_embed_collect}, srwn_pair_sweep, one host wait, the same metrics

Both give the same nearest-neighbour accuracy and the same histogram totals; the tool checks that before it times anything.
The pair launch is also timed alone (device events around --pair-iters launches, best of --reps) on planted embeddings.
usage: python tools/pair_eval_bench.py [--sizes 256,1024] [--batches 1,8,32] [--reps 3] [--pair 1024x2,1024x256,4096x2,4096x256]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
T, DIM, CLASSES, BINS = 5120, 2, 4, 512


def make_set(n):
    rng = np.random.default_rng(0)
    t = np.arange(T, dtype=np.float32)[None, :]
    clips = (0.5 * np.sin(t * rng.uniform(0.01, 0.3, (n, 1))) + 0.05 * rng.standard_normal((n, T))).astype(np.float32)
    return clips, rng.integers(0, CLASSES, n)


def regions(run, reps):
    """ms per call of `reps` regions of one call: (best, spread)."""
    import torch
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return min(v), max(v) - min(v)


def host_pairs(D, emb, labels, d_max):
    """The all-pairs pass in NumPy: a PairEvalResult from host embeddings."""
    n = emb.shape[0]
    e = emb.astype(np.float32)
    dist = np.sqrt(np.float32(1e-8) + ((e[:, None, :] - e[None, :, :]) ** 2).sum(-1, dtype=np.float32))
    j = np.arange(n)
    nearest, same_nearest, rank_same = (np.full(n, -1, np.int32) for _ in range(3))
    nearest_dist, same_dist = (np.full(n, np.inf, np.float32) for _ in range(2))
    for i in range(n):
        order = np.lexsort((j, dist[i]))
        order = order[order != i]
        if order.size:
            nearest[i], nearest_dist[i] = order[0], dist[i, order[0]]
        same = np.nonzero(labels[order] == labels[i])[0]
        if same.size:
            same_nearest[i], same_dist[i] = order[same[0]], dist[i, order[same[0]]]
            rank_same[i] = same[0]                                # (everything in front of it has another label)
    iu, ju = np.triu_indices(n, 1)
    b = np.minimum(BINS - 1, (dist[iu, ju] * np.float32(BINS / d_max)).astype(np.int64))
    eq = labels[iu] == labels[ju]
    hs, hd = np.bincount(b[eq], minlength=BINS), np.bincount(b[~eq], minlength=BINS)
    return D.PairEvalResult(e, nearest, nearest_dist, same_nearest, same_dist, rank_same, hs, hd, n, labels, BINS, d_max)


def pair_alone(D, K, n, dim, reps, iters):
    """ms per srwn_pair_sweep launch on planted embeddings: (best, spread) of `reps` event-timed runs of `iters` launches."""
    import torch
    rng = np.random.default_rng(1)
    ds = D.DeviceDataset(np.zeros((n, 8), np.float32), rng.integers(0, CLASSES, n), CLASSES)
    es = ds.embed_sampler(min(n, 64), 8, bins=BINS, d_max=4.0 * np.sqrt(dim), sweep_capacity=1)
    es.bind(dim, 1.0)
    es.emb.copy_(torch.as_tensor(rng.standard_normal((1, n, dim)).astype(np.float32)))
    es.state[2] = 1
    for _ in range(3):
        es.pair_sweep()
    v = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(iters):
            es.pair_sweep()
        t1.record()
        torch.cuda.synchronize()
        v.append(t0.elapsed_time(t1) / iters)
    assert int(es.hist_same.sum() + es.hist_diff.sum()) == n * (n - 1) // 2
    return min(v), max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024", help="clips of 5120 floats in the held-out set")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pair", default="1024x2,1024x256,4096x2,4096x256", help="N x D of the pair launch timed alone")
    ap.add_argument("--pair-iters", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    M = importlib.import_module("sr-wavenet_amd.model")
    D = importlib.import_module("sr-wavenet_amd.dataset")
    K = importlib.import_module("sr-wavenet_amd.kernels")
    m = M.SiameseWaveNet(T, DIM, DIL, skip_channels=128, learning_rate=1e-4)
    d_max = 2.0 * m.margin
    print("== twin towers, 30 layers, 32 / 128 channels, D = %d, bf16; clips of %d samples: ms per sweep, best of %d (spread)"
          % (DIM, T, a.reps), flush=True)
    for n in [int(s) for s in a.sizes.split(",")]:
        clips, labels = make_set(n)
        data = D.DeviceDataset(clips, labels, CLASSES)
        for B in [int(b) for b in a.batches.split(",")]:
            out = {}

            def host():
                emb = np.concatenate([m.get_embedding(None, clips[i:i + B])[:, 0, :] for i in range(0, n, B)])
                out["host"] = host_pairs(D, emb, labels, d_max)

            es = data.embed_sampler(B, T, bins=BINS)

            def device():
                out["device"] = m.evaluate(es)

            host()
            device()
            device()                   # (two eager steps, the capture: a sweep of one step captures in the second call)
            device()
            h, d = out["host"], out["device"]
            if h.hist_same.sum() != d.hist_same.sum() or h.hist_diff.sum() != d.hist_diff.sum():
                sys.exit("N %d batch %d: the two paths count different pairs" % (n, B))
            print("   N %4d batch %2d   1-NN accuracy %.4f / %.4f   EER %.4f / %.4f (host / device)"
                  % (n, B, h.nn_accuracy, d.nn_accuracy, h.eer, d.eer), flush=True)
            th, td = regions(host, a.reps), regions(device, a.reps)
            print("   N %4d batch %2d   (a) host loop %10.3f (%.3f)   (b) evaluate %10.3f (%.3f)   (a) / (b) = %.2f"
                  % (n, B, th[0], th[1], td[0], td[1], th[0] / td[0]), flush=True)
    print("== srwn_pair_sweep alone, %d bins: ms per launch, best of %d (spread)" % (BINS, a.reps), flush=True)
    for spec in a.pair.split(","):
        n, dim = (int(v) for v in spec.split("x"))
        best, spread = pair_alone(D, K, n, dim, a.reps, a.pair_iters)
        print("   N %4d D %3d   %8.3f (%.3f)   %.1f M pairs/s" % (n, dim, best, spread, n * (n - 1) / 2 / best / 1e3), flush=True)


if __name__ == "__main__":
    main()
