#!/usr/bin/env python3
"""What one sweep of a held-out set costs from the model API on one MI355X, per way of running it.

The reference driver's classifier shape (train.py:35-39): two blocks of dilations 1..512, 32 / 128 channels, clips of 16 384
samples, --classes classes, bf16.  A set of --records labelled clips is swept once per region; milliseconds per sweep, best
of --reps regions with the spread, each path in regions of its own, each region closed by a device synchronisation, after a
warm-up sweep of that path (which includes the capture):

  (a) host loop   the loop train.py --test runs (train.py:94-115), per batch of host arrays: predict(x), np.argmax, counting
                  the correct and wrong ones per class.  Batch 1 is train.py's own.
  (b) evaluate    model.evaluate(eval_sampler) on a DeviceDataset of the same clips: replays of one graph {draw, forward pass,
                  srwn_eval_classes} and one host wait per sweep

Both count the same predictions; the tool checks that before it times anything.
usage: python tools/eval_bench.py [--records 64] [--classes 30] [--reps 3] [--batches 1,8,32]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 2
T = 16384


def make_set(n, classes):
    rng = np.random.default_rng(0)
    t = np.arange(T, dtype=np.float32)[None, :]
    clips = (0.5 * np.sin(t * rng.uniform(0.01, 0.3, (n, 1))) + 0.05 * rng.standard_normal((n, T))).astype(np.float32)
    return clips, rng.integers(0, classes, n)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=64, help="clips of 16384 floats in the held-out set")
    ap.add_argument("--classes", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,8,32")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    M = importlib.import_module("sr-wavenet_amd.model")
    D = importlib.import_module("sr-wavenet_amd.dataset")
    clips, labels = make_set(a.records, a.classes)
    m = M.WaveNet(T, a.classes, DIL, dilation_channels=32, skip_channels=128, output_channels=a.classes, learning_rate=0.001)
    data = D.DeviceDataset(clips, labels, a.classes)
    print("== classifier, 20 layers, 32 / 128 channels, %d classes, bf16; %d clips of %d samples: ms per sweep, best of %d "
          "(spread)" % (a.classes, a.records, T, a.reps), flush=True)
    for B in [int(b) for b in a.batches.split(",")]:
        counts = {}

        def host():
            correct, total = np.zeros(a.classes, np.int64), np.zeros(a.classes, np.int64)
            for i in range(0, a.records, B):
                x, y = clips[i:i + B], labels[i:i + B]
                pred = np.argmax(m.predict(x)[:, 0, :], axis=1)
                np.add.at(total, y, 1)
                np.add.at(correct, y[pred == y], 1)
            counts["host"] = (correct, total)

        ev = data.eval_sampler(B, T)

        def device():
            counts["device"] = m.evaluate(ev).per_class

        host()
        device()
        device()                   # (two eager steps, the capture: a sweep of one step captures in the second call)
        if not (np.array_equal(counts["device"][:, 0], counts["host"][0]) and
                np.array_equal(counts["device"][:, 1], counts["host"][1])):
            sys.exit("batch %d: the two paths count differently: %r against %r" % (B, counts["device"].tolist(),
                                                                              [c.tolist() for c in counts["host"]]))
        h, d = regions(host, a.reps), regions(device, a.reps)
        print("   batch %2d   (a) host loop %9.3f (%.3f)   (b) evaluate %9.3f (%.3f)   (a) / (b) = %.2f   per clip: %.3f -> "
              "%.3f ms" % (B, h[0], h[1], d[0], d[1], h[0] / d[0], h[0] / a.records, d[0] / a.records), flush=True)


if __name__ == "__main__":
    main()
