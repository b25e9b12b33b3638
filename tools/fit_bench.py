#!/usr/bin/env python3
"""What a training step costs from the model API on one MI355X, per way of feeding it.

Two shapes: the config-2 teacher (30 layers, R = 64, S = 256, softmax, bf16, batch 8 x 16000) and examples/teacher.py's
auto-encoder (30 layers, S = 128, 5 mixtures, bf16, batch 4 x 4096).  Milliseconds per step, best of --reps regions of
--steps steps with the spread, each region closed by a device synchronisation, after a warm-up that includes the capture:

  (a) host arrays   model.train(x) on NumPy batches that already sit in host memory (a pool of 16, cycled)
  (b) TFRecord      model.train(x) on NsynthDataReader.next() over a generated file of --records clips of 16000 floats
  (c) fit           model.fit(sampler, steps) on a DeviceDataset of the same clips: one host wait per region
  (d) staged engine the engine's captured step replayed on inputs staged once (bench.py's path), this build against another
                    build of the library (--parent-lib, with --parent-root the package it belongs to: the parent commit's),
                    alternating fresh processes, --rounds each

(c) - (d) is what the draw and the log launch cost; (a) and (b) show what the host loop around the step costs.

Three more legs, for the models whose host loops do the most per step (--only student | twins_small | twins_wide; none of
them runs by default): the student at bench.py's student shape (4 flows x 30 layers, R = 64, a 30-layer MoL-10
auto-encoder teacher, bf16, batch 8 x 16000) and the twins at tools/siamese_bench.py's two shapes.  For each:

  (a) host loop     the example driver's loop on host arrays (a pool of 16, cycled): examples/student.py's encode, NumPy
                    logistic noise, train_fast; examples/siamese.py's train on pairs
  (b) fit           model.fit(sampler, steps) with a DistillSampler / PairSampler on a DeviceDataset
  (c) staged engine the captured step of the same engine replayed on the inputs of the last host step
  (e) student only: the teacher encoder's forward pass alone, as a graph -- (b) runs it inside the step, (c) does not

(a) - (c) is what the host loop costs above the step itself; (b) - (c) what the launches of the samplers (and, for the
student, the teacher's encoder inside the step) cost.
usage: python tools/fit_bench.py [--steps 200] [--reps 3] [--records 64]
                                 [--only teacher|autoencoder|student|twins_small|twins_wide]
                                 [--parent-lib ab/libsrwn_parent.so --parent-root ab/parent]"""
import argparse
import importlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
CLIP = 16000
SHAPES = {"teacher": (8, 16000), "autoencoder": (4, 4096)}
EXTRA = {"student": (8, 16000), "twins_small": (1, 5120), "twins_wide": (8, 16000)}     # batch (pairs) x samples


def make_model(M, shape):
    if shape == "teacher":
        return M.WaveNetTeacher(16000, 0, DIL, dilation_channels=64, skip_channels=256, quantization_channels=256)
    return M.WaveNetAutoEncoder(input_size=4096, condition_size=0, num_mixtures=5, dilations=DIL, latent_channels=16,
                                skip_channels=128, pool_stride=512, learning_rate=1e-4)        # examples/teacher.py


def make_clips(n):
    rng = np.random.default_rng(0)
    t = np.arange(CLIP, dtype=np.float32)[None, :]
    return (0.5 * np.sin(t * rng.uniform(0.01, 0.3, (n, 1))) + 0.05 * rng.standard_normal((n, CLIP))).astype(np.float32)


# ---- a TFRecord file of tf.train.Example{audio: float_list, pitch: int64_list}; the CRC fields are left zero and the reader
# is opened with verify_crc=False (a CRC-32C in Python over 64 KB records would dominate the tool's run time)
def _varint(v):
    out = b""
    while v >= 0x80:
        out += bytes([(v & 0x7F) | 0x80]); v >>= 7
    return out + bytes([v])


def _ld(field, payload):
    return _varint(field << 3 | 2) + _varint(len(payload)) + payload


def write_tfrecord(path, clips):
    with open(path, "wb") as f:
        for i, a in enumerate(clips):
            audio = _ld(2, _ld(1, a.astype("<f4").tobytes()))                    # Feature.float_list, packed
            pitch = _ld(3, _ld(1, _varint(21 + i % 88)))                         # Feature.int64_list, packed
            feats = b"".join(_ld(1, _ld(1, k) + _ld(2, v)) for k, v in ((b"audio", audio), (b"pitch", pitch)))
            payload = _ld(1, feats)
            f.write(struct.pack("<QI", len(payload), 0) + payload + struct.pack("<I", 0))


def regions(run, steps, reps):
    """ms per step of `reps` regions of `steps` steps: (best, spread)."""
    import torch
    v = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) / steps * 1e3)
    return min(v), max(v) - min(v)


def model_paths(a, shape):
    import torch
    M = importlib.import_module("sr-wavenet_amd.model")
    D = importlib.import_module("sr-wavenet_amd.dataset")
    NS = importlib.import_module("sr-wavenet_amd.nsynth")
    B, T = SHAPES[shape]
    clips = make_clips(a.records)
    out = {}
    # (a) host-resident batches
    m = make_model(M, shape)
    rng = np.random.default_rng(1)
    pool = [np.ascontiguousarray(clips[rng.integers(0, a.records, B), :T]) for _ in range(16)]

    def host(n):
        for i in range(n):
            m.train(pool[i % 16])
    host(a.warmup)
    out["a"] = regions(host, a.steps, a.reps)
    # (b) the TFRecord reader
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clips.tfrecord")
        write_tfrecord(path, clips)
        reader = NS.NsynthDataReader(path, B, T, audio_max_length=CLIP, seed=0, verify_crc=False)

        def tfr(n):
            for _ in range(n):
                m.train(reader.next()[0])
        tfr(a.warmup)
        out["b"] = regions(tfr, a.steps, a.reps)
        del reader
    # (c) fit on the device-resident clips (a fresh model: its own two eager steps and capture in the warm-up)
    del m
    m = make_model(M, shape)
    s = D.DeviceDataset(clips).sampler(B, T, seed=0)
    m.fit(s, a.warmup)
    out["c"] = regions(lambda n: m.fit(s, n), a.steps, a.reps)
    return out


def make_student(M):
    """bench.py's student shape on the model API: the frozen teacher is an auto-encoder, so that it can encode."""
    t = M.WaveNetAutoEncoder(16000, 0, 10, DIL, dilation_channels=64, skip_channels=256, latent_channels=16, pool_stride=125)
    return M.ParallelWaveNet(16000, 0, DIL, t, num_flows=4, dilation_channels=64, skip_channels=256, latent_channels=16,
                             pool_stride=125, alpha=1.0, beta=1.0, gamma=1e-3, learning_rate=1e-4)


def make_twins(M, shape):
    R, S = (32, 128) if shape == "twins_small" else (64, 256)
    return M.SiameseWaveNet(EXTRA[shape][1], 2, DIL, dilation_channels=R, skip_channels=S, learning_rate=1e-4)


def extra_paths(a, shape):
    """(a), (b), (c) of the student and the twins: {key: (best, spread)}."""
    import gc
    import torch
    M = importlib.import_module("sr-wavenet_amd.model")
    D = importlib.import_module("sr-wavenet_amd.dataset")
    SA = importlib.import_module("sr-wavenet_amd.simple_audio")
    B, T = EXTRA[shape]
    rng = np.random.default_rng(1)
    out = {}
    if shape == "student":
        clips = make_clips(a.records)
        labels = None
        m = make_student(M)
        pool = [np.ascontiguousarray(clips[rng.integers(0, a.records, B), :T]) for _ in range(16)]

        def host(n):
            for i in range(n):
                x = pool[i % 16]
                enc = m.encode(None, x, None)
                noise = rng.logistic(0, 1, (B, T)).astype(np.float32)
                m.train_fast(None, noise, x, enc, None)
        eng = lambda: m._engine(B, T)
    else:
        gen = np.random.RandomState(0)
        waves = [SA.generate_random_wave(T, rng=gen) for _ in range(a.records)]
        clips = np.array([w for w, _ in waves], dtype=np.float32)
        labels = np.array([int(np.argmax(y)) for _, y in waves])
        m = make_twins(M, shape)
        pool = []
        for _ in range(16):
            l, r = rng.integers(0, a.records, B), rng.integers(0, a.records, B)
            pool.append((clips[l], clips[r], (labels[l] == labels[r]).astype(np.float32)))

        def host(n):
            for i in range(n):
                m.train(None, *pool[i % 16])
        eng = lambda: m._engine(2 * B, T)
    host(a.warmup)
    out["a"] = regions(host, a.steps, a.reps)
    e = eng()

    def staged(n):
        for _ in range(n):
            e.train_step_graphed()
    staged(a.warmup)
    out["c"] = regions(staged, a.steps, a.reps)
    if shape == "student":      # what (b) runs inside the step and (c) does not: the teacher encoder's forward pass, as a graph
        enc = m._teacher._engine(B, T).enc
        enc.forward()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            enc.forward()

        def encode(n):
            for _ in range(n):
                g.replay()
        encode(a.warmup)
        out["e"] = regions(encode, a.steps, a.reps)
        del g, enc
    del m, e
    gc.collect()
    torch.cuda.empty_cache()
    if shape == "student":
        m = make_student(M)
        s = D.DeviceDataset(clips).distill_sampler(B, T, seed=0)
    else:
        m = make_twins(M, shape)
        s = D.DeviceDataset(clips, labels, 4).pair_sampler(B, T, seed=0)
    m.fit(s, a.warmup)
    out["b"] = regions(lambda n: m.fit(s, n), a.steps, a.reps)
    return out


def staged_child(a):
    """(d) in this process: bench.py's path on the package under --pkg-root."""
    sys.path.insert(0, a.pkg_root)
    import torch
    EG = importlib.import_module("sr-wavenet_amd.engine")
    KN = importlib.import_module("sr-wavenet_amd.kernels")
    B, T = SHAPES[a.only_shape]
    x = torch.tensor(make_clips(B)[:, :T], device="cuda")
    if a.only_shape == "teacher":
        cfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, output_channels=256, shift_input=True,
                             dtype=torch.bfloat16, learning_rate=1e-3)
        eng = EG.WaveNetEngine(cfg, B, T, "cuda", seed=0)
        eng.set_inputs(x, KN.mu_law_encode(x, 256))
    else:
        EN = importlib.import_module("sr-wavenet_amd.encoder")
        cfg = EG.StackConfig(dilations=DIL, dilation_channels=32, skip_channels=128, output_channels=20, cond_channels=16,
                             pool_stride=512, shift_input=True, head_mode="mol", dtype=torch.bfloat16, learning_rate=1e-4)
        eng = EN.AutoEncoderEngine(cfg, B, T, 128, 16, 0, "cuda", seed=0)
        eng.set_inputs(x)
    eng.train_step(); eng.train_step()
    eng.capture_graphs()

    def run(n):
        for _ in range(n):
            eng.train_step_graphed()
    run(a.warmup)
    print("ABRESULT " + json.dumps(regions(run, a.steps, a.reps)))


def staged(a, shape):
    builds = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so"), ROOT)]
    if a.parent_lib:
        builds.append(("parent", os.path.join(ROOT, a.parent_lib), os.path.join(ROOT, a.parent_root)))
    got = {k: [] for k, _, _ in builds}
    for r in range(a.rounds):
        for name, lib, root in builds:
            env = dict(os.environ, SRWN_LIB_PATH=lib)          # (both through the ctypes binding)
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--pkg-root", root, "--steps",
                                 str(a.steps), "--reps", str(a.reps), "--warmup", str(a.warmup)], env=env, cwd=root,
                                capture_output=True, text=True, timeout=600)
            line = [l for l in pr.stdout.splitlines() if l.startswith("ABRESULT ")]
            if pr.returncode or not line:
                sys.exit("FAILED %s build (exit %d): %s" % (name, pr.returncode, pr.stderr[-2000:]))    # nothing more on the GPU
            best, spread = json.loads(line[0][9:])
            got[name].append(best)
            print("   (d) round %d %-6s best %.4f ms (spread %.4f)" % (r, name, best, spread), flush=True)
    return {k: (min(v), max(v) - min(v)) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--records", type=int, default=64, help="clips of 16000 floats in the data set and the generated file")
    ap.add_argument("--only", default=None, choices=list(SHAPES) + list(EXTRA))
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for (d)")
    ap.add_argument("--parent-root", default=None, help="the package that library belongs to (relative to the repository)")
    ap.add_argument("--child", dest="only_shape", default=None, choices=list(SHAPES), help=argparse.SUPPRESS)
    ap.add_argument("--pkg-root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.only_shape:
        return staged_child(a)
    if bool(a.parent_lib) != bool(a.parent_root):
        sys.exit("--parent-lib and --parent-root go together")
    sys.path.insert(0, ROOT)
    if a.only in EXTRA:
        B, T = EXTRA[a.only]
        print("== %s, %d x %d, bf16: ms per step, best of %d regions of %d steps (spread)" % (a.only, B, T, a.reps, a.steps),
              flush=True)
        res = extra_paths(a, a.only)
        for key, name in (("a", "(a) the example's host loop"), ("b", "(b) fit"), ("c", "(c) staged engine replays")):
            print("   %-32s %.4f (%.4f)" % (name, *res[key]), flush=True)
        if "e" in res:
            print("   %-32s %.4f (%.4f)" % ("(e) teacher encoder forward alone", *res["e"]), flush=True)
        print("   (a) - (c) = %+.4f ms   (b) - (c) = %+.4f ms" % (res["a"][0] - res["c"][0], res["b"][0] - res["c"][0]),
              flush=True)
        return
    for shape in ([a.only] if a.only else list(SHAPES)):
        B, T = SHAPES[shape]
        print("== %s, batch %d x %d, bf16: ms per step, best of %d regions of %d steps (spread)" % (shape, B, T, a.reps, a.steps),
              flush=True)
        res = model_paths(a, shape)
        for key, name in (("a", "(a) train(x), host arrays"), ("b", "(b) train(x), NsynthDataReader"), ("c", "(c) fit")):
            print("   %-32s %.4f (%.4f)" % (name, *res[key]), flush=True)
        d = staged(a, shape)
        if d:
            for k, (best, spread) in d.items():
                print("   %-32s %.4f (%.4f over %d processes)" % ("(d) staged engine, %s build" % k, best, spread, a.rounds))
            print("   (c) - (d, this build) = %+.4f ms" % (res["c"][0] - d["this"][0]), flush=True)


if __name__ == "__main__":
    main()
