#!/usr/bin/env python3
"""Live autoregressive decoding on one MI355X: the conditioned MoL-10 decoder at BASELINE config 5's shape (bf16, 30 layers
3 x [1..512], 64 residual / 256 skip channels, 16 latent channels; tools/stream_bench.py's decoder) fed while it runs.

  (a) old path  generate_chunk over a whole table, chunks of 160, B = 1 and 32, us per sample: this build against another
                build (--parent-lib, with --parent-root the package it belongs to: the parent commit's), alternating fresh
                processes through SRWN_LIB_PATH
  (b) live      us per sample of a live run's step (LiveDecoding._step_device: generate_chunk on a ring, outputs left on
                the device) in chunks of 160 and of one frame, against generate_chunk on a whole table at the same shapes,
                B = 1 / 8 / 32, pool 125; the two alternate in one process
  (c) feed      WaveNetEngine.feed of one frame alone (copy, projection, one scatter launch), for 1 and 32 streams
  (d) push      ms per TeacherResynthesizer push of exactly one frame's audio (NumPy in, NumPy out) in the steady state, B = 1,
                pool 128 and 512; beside it the encoder's push of one frame and the decoder's step of pool_stride samples
                measured apart, their sum, and the real-time factor at 16 kHz
  latency       the algorithmic latency in samples: pool_stride + encoder layers + 1 of look-ahead, plus the chunk

Every measurement runs in a fresh child process under a time limit of its own, one after the other; the first that fails
ends the run.  Every timed region is device-synchronised and holds >= --seconds of work after a warm-up.
usage: python tools/live_decode_bench.py [--seconds 0.5] [--reps 3] [--parent-lib ab/libsrwn_parent.so --parent-root ab/parent]"""
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
POOL, FRAMES = 125, 32
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


class Chunks:
    """generate_chunk(n) for ever on one state: at the end of what the table (or the full ring) covers the step goes back
    to 0 (timing only: the rings keep what they hold)."""

    def __init__(self, eng, st, n):
        self.eng, self.st, self.n = eng, st, n

    def __call__(self):
        if self.st.t + self.n > self.st.limit:
            self.st.t = 0
        self.eng.generate_chunk(self.st, self.n, mode="sample")


def old_path_child(a):
    import torch
    eng = decoder()
    out = {}
    for B in (1, 32):
        st = eng.generation_state(B, torch.randn((B, FRAMES, LAT), device="cuda"), 1)
        out[str(B)] = [timed(Chunks(eng, st, 160), a.seconds) / 160 * 1e3 for _ in range(a.reps)]
    print("RESULT " + json.dumps(out))


def live_child(a):
    import torch
    eng, B = decoder(), a.batch
    cond = torch.randn((B, FRAMES, LAT), device="cuda")
    whole = eng.generation_state(B, cond, 1)
    live = eng.live_generation_state(B, FRAMES, 1)
    eng.feed(live, cond)                       # a full ring: the steps alone are timed
    out = {}
    for n in (160, POOL):
        lv, wh = [], []
        for _ in range(a.reps):
            lv.append(timed(Chunks(eng, live, n), a.seconds) / n * 1e3)
            wh.append(timed(Chunks(eng, whole, n), a.seconds) / n * 1e3)
        out[str(n)] = dict(live=lv, whole=wh)
    print("RESULT " + json.dumps(out))


def feed_child(a):
    import torch
    eng = decoder()
    out = {}
    for B in (1, 32):
        st = eng.live_generation_state(B, FRAMES, 1)
        frame = torch.zeros((B, 1, LAT), device="cuda")

        def feed():
            st.t = st.limit                    # (the steady state: every sample of the fed frames is made, the ring has room)
            eng.feed(st, frame)

        out[str(B)] = [timed(feed, a.seconds) for _ in range(a.reps)]
    print("RESULT " + json.dumps(out))


def push_child(a):
    """(d) for one pool: the three measurements alternate in one process."""
    import torch
    M = importlib.import_module("sr-wavenet_amd.model")
    P, B, dt = a.pool, 1, torch.bfloat16
    enc = M.AudioEncoder(ENC_LAYERS, skip_channels=S, latent_channels=LAT, pool_stride=P, dtype=dt, max_batch=B,
                         max_frames=FRAMES)
    ae = M.WaveNetAutoEncoder(P * FRAMES, 0, MIX, DIL, dilation_channels=R, skip_channels=S, latent_channels=LAT,
                              pool_stride=P, dtype=dt)
    rng = np.random.default_rng(0)
    block = rng.uniform(-1, 1, (B, P)).astype(np.float32)
    head = rng.uniform(-1, 1, (B, P + ENC_LAYERS + 1)).astype(np.float32)
    rs = M.TeacherResynthesizer(enc, ae, max_frames=FRAMES)
    s = rs.stream(batch=B, seed=1, chunk_size=P)
    assert s.push(head).shape == (B, P)

    def push():
        assert s.push(block).shape[1] == P

    fe = enc._eng
    est = fe.start(B)
    dblock = torch.as_tensor(block).to("cuda")
    fe.push(est, torch.as_tensor(head).to("cuda"))

    def enc_push():
        assert fe.push(est, dblock).shape[1] == 1

    dec = ae._eng.dec
    st = dec.live_generation_state(B, FRAMES, 1)
    dec.feed(st, torch.zeros((B, FRAMES, LAT), device="cuda"))
    dec_step = Chunks(dec, st, P)
    tp, te, td = [], [], []
    for _ in range(a.reps):
        tp.append(timed(push, a.seconds))
        te.append(timed(enc_push, a.seconds))
        td.append(timed(dec_step, a.seconds))
    assert s.t > FRAMES * P, "the ring did not wrap during the measurement"
    print("RESULT " + json.dumps(dict(pool=P, push=tp, enc=te, dec=td)))


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


def old_path(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so"), ROOT),
            ("parent", os.path.join(ROOT, a.parent_lib), os.path.join(ROOT, a.parent_root))]
    print("== (a) generate_chunk over a whole table, chunks of 160: us per sample, this build against %s, alternating "
          "fresh processes" % a.parent_lib)
    got = {k: {"1": [], "32": []} for k, _, _ in libs}
    for r in range(a.rounds):
        for name, path, root in libs:
            d = child(["--only", "old-path-child"], a, dict(os.environ, SRWN_LIB_PATH=path), root)
            if d is None:
                sys.exit(1)
            for k in d:
                got[name][k] += d[k]
            print("round %d %-6s %s" % (r, name, "  ".join("B = %s: %s" % (k, " ".join("%.3f" % m for m in d[k])) for k in d)),
                  flush=True)
    for k in ("1", "32"):
        t, p = got["this"][k], got["parent"][k]
        print("B = %2s: this build best %.3f us (spread %.3f), parent best %.3f us (spread %.3f): difference %+.3f us"
              % (k, min(t), max(t) - min(t), min(p), max(p) - min(p), min(t) - min(p)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for (a)")
    ap.add_argument("--parent-root", default=None, help="the tree whose package goes with --parent-lib (relative)")
    ap.add_argument("--only", default=None, choices=["old-path-child", "live-child", "feed-child", "push-child"])
    ap.add_argument("--root", default=ROOT, help="(children) the tree to import the package from")
    ap.add_argument("--pool", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    if a.only:
        sys.path.insert(0, a.root)
        return {"old-path-child": old_path_child, "live-child": live_child, "feed-child": feed_child,
                "push-child": push_child}[a.only](a)

    if a.parent_lib:
        if not a.parent_root:
            sys.exit("--parent-lib needs --parent-root, the tree its package comes from")
        old_path(a)
    print("== (b) a live run's step against generate_chunk over a whole table: us per sample, best of %d (spread)" % a.reps)
    for B in (1, 8, 32):
        r = child(["--only", "live-child", "--batch", str(B)], a)
        if r is None:
            sys.exit(1)
        for n in ("160", str(POOL)):
            print("B = %2d chunks of %3s: live %s   whole table %s   RTF live %.3f" %
                  (B, n, spread(r[n]["live"]), spread(r[n]["whole"]), min(r[n]["live"]) * 1e-6 * RATE), flush=True)
    print("== (c) WaveNetEngine.feed of one frame: ms per feed, best of %d (spread)" % a.reps)
    r = child(["--only", "feed-child"], a)
    if r is None:
        sys.exit(1)
    for B in ("1", "32"):
        print("%2s stream%s: %s" % (B, " " if B == "1" else "s", spread(r[B])), flush=True)
    print("== (d) one frame per push, B = 1: ms per push, best of %d (spread); encoder push + decoder step measured apart" % a.reps)
    print("%4s %22s %22s %22s %9s %6s %s" % ("P", "TeacherResynth. push", "encoder push", "decoder step", "enc+dec", "RTF",
                                             "latency (samples)"))
    for P in (128, 512):
        r = child(["--only", "push-child", "--pool", str(P)], a)
        if r is None:
            sys.exit(1)
        print("%4d %22s %22s %22s %9.3f %6.3f %d + chunk %d = %d" %
              (P, spread(r["push"]), spread(r["enc"]), spread(r["dec"]), min(r["enc"]) + min(r["dec"]),
               min(r["push"]) / (P / RATE * 1e3), P + ENC_LAYERS + 1, P, 2 * P + ENC_LAYERS + 1), flush=True)


if __name__ == "__main__":
    main()
