#!/usr/bin/env python3
"""Live slots in generation pools on one MI355X: the conditioned MoL-10 decoder at BASELINE config 5's shape (bf16, 30 layers
3 x [1..512], 64 residual / 256 skip channels, 16 latent channels; tools/live_decode_bench.py's decoder), conditioning
rings of 32 frames, chunks of 160.

  (a) step      us per pool step (one launch of 160 steps / 160) of a LIVE pool with every slot fed, against a plain
                generation_pool at the same capacity, 1 / 32 / 256 slots; the two alternate in one process
  (b) rotate    one srwn_generate_ring_rotate_slots launch for 1 and 32 lagging slots, and one GenerationPool.feed of one
                frame per slot (copy, projection, one scatter launch) for 1 and 32 slots: us per call
  (c) rounds    TeacherResynthesisPool: ms per round of one frame's audio per stream (push + step, NumPy in, NumPy out) in
                the steady state at B = 1 / 8 / 32, against one push of the lockstep TeacherResynthesizer.stream
  (d) old paths a plain pool's step and generate_chunk over a whole table (chunks of 160, 1 and 32 streams): this build
                against another build (--parent-lib, with --parent-root the package it belongs to: the parent commit's),
                alternating fresh processes through SRWN_LIB_PATH

Every measurement runs in a fresh child process under a time limit of its own, one after the other; the first that fails
ends the run.  Every timed region is device-synchronised and holds >= --seconds of work after a warm-up; best of --reps
with the spread.
usage: python tools/live_pool_bench.py [--seconds 0.5] [--reps 3] [--parent-lib ab/libsrwn_parent.so --parent-root ab/parent]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENC_LAYERS, R, S, LAT, MIX, RATE = 30, 64, 256, 16, 10, 16000
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
POOL, FRAMES, CHUNK = 125, 32, 160
STEP_LIMIT = 300          # seconds a child may take


def spread(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def timed(fn, seconds):
    """ms per call over a region of >= `seconds` (after two warm-up calls)."""
    import torch
    fn(); fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    reps = max(3, int(seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def decoder(pool=POOL):
    import torch
    EG = importlib.import_module("sr-wavenet_amd.engine")
    cfg = EG.StackConfig(dilations=DIL, dilation_channels=R, skip_channels=S, output_channels=4 * MIX, cond_channels=LAT,
                         pool_stride=pool, shift_input=True, head_mode="mol", dtype=torch.bfloat16)
    return EG.WaveNetEngine(cfg, 1, pool, "cuda")


class PoolSteps:
    """pool.step(n) for ever: every slot goes back to step 0 when it would pass its end (timing only: the rings keep what
    they hold).  A live pool's slots are fed a full ring and never pause, so no rotation runs."""

    def __init__(self, pool, n):
        self.pool, self.n = pool, n

    def __call__(self):
        p = self.pool
        if (p._t + self.n > p._end).any():
            p._t[:] = 0
            p._upload()
        p.step(self.n, mode="sample")


def full_pool(eng, cap, live):
    import torch
    pool = eng.generation_pool(cap, FRAMES, live=True) if live else eng.generation_pool(cap, FRAMES)
    enc = [torch.randn((FRAMES, LAT), device="cuda") for _ in range(cap)]
    if live:
        pool.join(list(range(cap)), cond=enc, live=True)
    else:
        pool.join(list(range(cap)), cond=enc)
    return pool


class Chunks:
    def __init__(self, eng, st, n):
        self.eng, self.st, self.n = eng, st, n

    def __call__(self):
        if self.st.t + self.n > self.st.limit:
            self.st.t = 0
        self.eng.generate_chunk(self.st, self.n, mode="sample")


def step_child(a):
    eng, cap = decoder(), a.batch
    live, plain = PoolSteps(full_pool(eng, cap, True), CHUNK), PoolSteps(full_pool(eng, cap, False), CHUNK)
    lv, pl = [], []
    for _ in range(a.reps):
        lv.append(timed(live, a.seconds) / CHUNK * 1e3)
        pl.append(timed(plain, a.seconds) / CHUNK * 1e3)
    print("RESULT " + json.dumps(dict(live=lv, plain=pl)))


def rotate_child(a):
    import torch
    K = importlib.import_module("sr-wavenet_amd.kernels")
    eng = decoder()
    pool = eng.generation_pool(32, FRAMES, live=True)
    pool.join(list(range(32)), cond=[None] * 32, live=True)
    out = {}
    for n in (1, 32):
        ids = torch.arange(n, dtype=torch.int32, device="cuda")
        sh = torch.full((n,), 160, dtype=torch.int32, device="cuda")
        dil = eng._gen_dilations()
        out["rotate%d" % n] = [timed(lambda: K.ring_rotate_slots(pool.ring, dil, eng.L, 32, eng.R, ids, sh), a.seconds) * 1e3
                               for _ in range(a.reps)]
        frames = [torch.zeros((1, LAT), device="cuda") for _ in range(n)]
        us = list(range(n))

        def feed():
            pool._t[:n] = pool._end[:n]        # (the steady state: every sample of the fed frames is made, the rings have room)
            pool.feed(us, frames)

        out["feed%d" % n] = [timed(feed, a.seconds) * 1e3 for _ in range(a.reps)]
    print("RESULT " + json.dumps(out))


def rounds_child(a):
    """(c) for one batch: the pool's round and the lockstep stream's push alternate in one process."""
    import torch
    M = importlib.import_module("sr-wavenet_amd.model")
    P, B, dt = 128, a.batch, torch.bfloat16
    enc = M.AudioEncoder(ENC_LAYERS, skip_channels=S, latent_channels=LAT, pool_stride=P, dtype=dt, max_batch=B,
                         max_frames=FRAMES)
    ae = M.WaveNetAutoEncoder(P * FRAMES, 0, MIX, DIL, dilation_channels=R, skip_channels=S, latent_channels=LAT,
                              pool_stride=P, dtype=dt)
    rng = np.random.default_rng(0)
    block = rng.uniform(-1, 1, (B, P)).astype(np.float32)
    head = rng.uniform(-1, 1, (B, P + ENC_LAYERS + 1)).astype(np.float32)
    rs = M.TeacherResynthesizer(enc, ae, max_frames=FRAMES)
    rp = rs.pool(chunk_size=P)
    us = rp.join(seed=1, n=B)
    rp.push(us, list(head))
    assert all(len(y) == P for y in rp.step().values())

    def round_():
        rp.push(us, list(block))
        out = rp.step()
        assert len(out) == B and len(out[0]) == P

    tp, ts = [], []
    for _ in range(a.reps):
        tp.append(timed(round_, a.seconds))
    del rp
    enc2 = M.AudioEncoder(ENC_LAYERS, skip_channels=S, latent_channels=LAT, pool_stride=P, dtype=dt, max_batch=B,
                          max_frames=FRAMES)      # (an encoder of its own: the pool above holds the first one's rows)
    s = M.TeacherResynthesizer(enc2, ae, max_frames=FRAMES).stream(batch=B, seed=1, chunk_size=P)
    assert s.push(head).shape == (B, P)

    def push():
        assert s.push(block).shape[1] == P

    for _ in range(a.reps):
        ts.append(timed(push, a.seconds))
    print("RESULT " + json.dumps(dict(pool=tp, stream=ts)))


def old_path_child(a):
    import torch
    eng = decoder()
    out = {}
    for B in (1, 32):
        st = eng.generation_state(B, torch.randn((B, FRAMES, LAT), device="cuda"), 1)
        out["chunk%d" % B] = [timed(Chunks(eng, st, CHUNK), a.seconds) / CHUNK * 1e3 for _ in range(a.reps)]
        out["pool%d" % B] = [timed(PoolSteps(full_pool(eng, B, False), CHUNK), a.seconds) / CHUNK * 1e3 for _ in range(a.reps)]
    print("RESULT " + json.dumps(out))


def child(args, a, env=None, root=ROOT):
    """A measurement in a fresh process under its own time limit -> the dict it reports, or None when it failed."""
    cmd = [sys.executable, os.path.abspath(__file__), "--seconds", str(a.seconds), "--reps", str(a.reps), "--root", root] + args
    try:
        pr = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        print("FAILED (time limit of %d s): %s" % (STEP_LIMIT, " ".join(args)), flush=True)
        return None
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if pr.returncode or not line:
        print("FAILED (exit %d): %s\n%s" % (pr.returncode, " ".join(args), pr.stderr[-2000:]), flush=True)
        return None
    return json.loads(line[0][7:])


def old_paths(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so"), ROOT),
            ("parent", os.path.join(ROOT, a.parent_lib), os.path.join(ROOT, a.parent_root))]
    print("== (d) the paths that existed before, chunks of %d: us per step, this build against %s, alternating fresh "
          "processes" % (CHUNK, a.parent_lib))
    keys = ("pool1", "pool32", "chunk1", "chunk32")
    got = {k: {q: [] for q in keys} for k, _, _ in libs}
    for r in range(a.rounds):
        for name, path, root in libs:
            d = child(["--only", "old-path-child"], a, dict(os.environ, SRWN_LIB_PATH=path), root)
            if d is None:
                sys.exit(1)
            for k in d:
                got[name][k] += d[k]
            print("round %d %-6s %s" % (r, name, "  ".join("%s: %s" % (k, " ".join("%.3f" % m for m in d[k])) for k in keys)),
                  flush=True)
    for k in keys:
        t, p = got["this"][k], got["parent"][k]
        print("%-8s this build best %.3f us (spread %.3f), parent best %.3f us (spread %.3f): difference %+.3f us"
              % (k, min(t), max(t) - min(t), min(p), max(p) - min(p), min(t) - min(p)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for (d)")
    ap.add_argument("--parent-root", default=None, help="the tree whose package goes with --parent-lib (relative)")
    ap.add_argument("--only", default=None, choices=["step-child", "rotate-child", "rounds-child", "old-path-child"])
    ap.add_argument("--root", default=ROOT, help="(children) the tree to import the package from")
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    if a.only:
        sys.path.insert(0, a.root)
        return {"step-child": step_child, "rotate-child": rotate_child, "rounds-child": rounds_child,
                "old-path-child": old_path_child}[a.only](a)

    print("== (a) a live pool with every slot fed against a plain pool: us per pool step, chunks of %d, best of %d (spread)"
          % (CHUNK, a.reps))
    for cap in (1, 32, 256):
        r = child(["--only", "step-child", "--batch", str(cap)], a)
        if r is None:
            sys.exit(1)
        print("%3d slots: live %s   plain %s   difference %+.3f us" %
              (cap, spread(r["live"]), spread(r["plain"]), min(r["live"]) - min(r["plain"])), flush=True)
    print("== (b) one rotation launch (30 layers) and one feed of one frame per slot: us per call, best of %d (spread)" % a.reps)
    r = child(["--only", "rotate-child"], a)
    if r is None:
        sys.exit(1)
    for n in (1, 32):
        print("%2d slot%s: rotation %s   feed %s" % (n, " " if n == 1 else "s", spread(r["rotate%d" % n]),
                                                    spread(r["feed%d" % n])), flush=True)
    print("== (c) TeacherResynthesisPool, one frame (128 samples) of audio per stream and round: ms per round, best of %d "
          "(spread); beside it one push of the lockstep stream" % a.reps)
    for B in (1, 8, 32):
        r = child(["--only", "rounds-child", "--batch", str(B)], a)
        if r is None:
            sys.exit(1)
        print("B = %2d: pool round %s   lockstep push %s   RTF pool %.3f" %
              (B, spread(r["pool"]), spread(r["stream"]), min(r["pool"]) / (128 / RATE * 1e3)), flush=True)
    if a.parent_lib:
        if not a.parent_root:
            sys.exit("--parent-lib needs --parent-root, the tree its package comes from")
        old_paths(a)


if __name__ == "__main__":
    main()
