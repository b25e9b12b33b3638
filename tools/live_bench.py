#!/usr/bin/env python3
"""Live synthesis on one MI355X: model.Resynthesizer over tools/encode_bench.py's encoder (30 layers, 128 channels, 256
skip channels, 16 latent channels) and bench.py's student_leg flows (4 x 30 layers, R = 64), both bf16.

  (a) push      ms per Resynthesizer push of exactly one frame's worth of audio (NumPy in, NumPy out) in the steady state,
                B = 1, 8, 32 for pool 128 and 512; beside it the separately measured encoder push of one frame and
                synthesizer step of pool_stride samples, and their sum
  (b) feed      FlowSynthesizer.feed of one frame alone, for 1 and 32 streams (one srwn_cond_ring_feed per flow)
  (c) old path  FlowSynthesizer.step of this build against another build of the library (--parent-lib: the parent
                commit's), B = 8, n = 160 and 1600, alternating fresh processes through SRWN_LIB_PATH
                (tools/synth_pool_bench.py's measurement)
  latency       the algorithmic latency in samples: pool_stride + encoder layers + 1 of look-ahead, plus the chunk

Every measurement runs in a fresh child process under a time limit of its own, one after the other; the first that fails
ends the run.  Every timed region is device-synchronised and holds >= --seconds of work after a warm-up.
usage: python tools/live_bench.py [--seconds 0.3] [--reps 3] [--parent-lib ab/libsrwn_parent.so] [--quick]"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ENC_LAYERS, S, LAT, RATE = 30, 256, 16, 16000
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
FLOWS, FRAMES = 4, 32
STEP_LIMIT = 300          # seconds a child may take


def spread(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def push_child(a):
    """(a) for one (pool, B): the three measurements alternate in one process."""
    import torch
    from synth_pool_bench import timed
    M = importlib.import_module("sr-wavenet_amd.model")
    P, B = a.pool, a.batch
    dt = torch.bfloat16
    enc = M.AudioEncoder(ENC_LAYERS, skip_channels=S, latent_channels=LAT, pool_stride=P, dtype=dt, max_batch=B,
                         max_frames=FRAMES)
    syn = M.StudentSynthesizer(DIL, FLOWS, dilation_channels=64, latent_channels=LAT, pool_stride=P, dtype=dt, max_batch=B,
                               max_chunk=P, max_frames=FRAMES)
    alone = M.StudentSynthesizer(DIL, FLOWS, dilation_channels=64, latent_channels=LAT, pool_stride=P, dtype=dt,
                                 max_batch=B, max_chunk=P, max_frames=FRAMES)
    rng = np.random.default_rng(0)
    block = rng.uniform(-1, 1, (B, P)).astype(np.float32)
    head = rng.uniform(-1, 1, (B, P + ENC_LAYERS + 1)).astype(np.float32)
    rs = M.Resynthesizer(enc, syn)
    s = rs.stream(batch=B, seed=1, chunk_size=P)
    assert s.push(head).shape == (B, P, 1)

    def push():
        assert s.push(block).shape[1] == P

    fe = enc._eng
    est = fe.start(B)
    dblock = torch.as_tensor(block).to("cuda")
    fe.push(est, torch.as_tensor(head).to("cuda"))

    def enc_push():
        assert fe.push(est, dblock).shape[1] == 1

    eng = alone._eng
    st = eng.start(torch.zeros((B, FRAMES, LAT)), seeds=1)

    def syn_step():
        if st.t + P > st.limit:
            eng.clock.fill_(P)
            st.t = P
        eng.step(st, P)

    tp, te, ts = [], [], []
    for _ in range(a.reps):
        tp.append(timed(push, a.seconds))
        te.append(timed(enc_push, a.seconds))
        ts.append(timed(syn_step, a.seconds))
    assert s.t > FRAMES * P, "the ring wrapped during the measurement"
    print("RESULT " + json.dumps(dict(pool=P, B=B, push=tp, enc=te, syn=ts)))


def feed_child(a):
    """(b): one frame into the rings of every flow, the state put back on the host when the ring is full."""
    import torch
    from synth_pool_bench import timed
    EG = importlib.import_module("sr-wavenet_amd.engine")
    ST = importlib.import_module("sr-wavenet_amd.student")
    fcfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, cond_channels=LAT, pool_stride=128,
                          dtype=torch.bfloat16)
    out = {}
    for B in (1, 32):
        syn = ST.FlowSynthesizer(fcfg, FLOWS, max_batch=B, max_chunk=128, max_frames=FRAMES)
        st = syn.start(None, 1, 1.0, live=True, batch=B)
        frame = torch.zeros((B, 1, LAT), device="cuda")

        def feed():
            if syn.room(st) == 0:
                st.fed, st.limit = 0, 0
            syn.feed(st, frame)

        out[str(B)] = [timed(feed, a.seconds) for _ in range(a.reps)]
    print("RESULT " + json.dumps(out))


def child(args, a, env=None):
    """A measurement in a fresh process under its own time limit -> the dict it reports, or None when it failed."""
    cmd = [sys.executable, os.path.abspath(__file__), "--seconds", str(a.seconds), "--reps", str(a.reps)] + args
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="B = 1 and 8 only")
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for (c)")
    ap.add_argument("--only", default=None, choices=["push-child", "feed-child"])
    ap.add_argument("--pool", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    if a.only == "push-child":
        return push_child(a)
    if a.only == "feed-child":
        return feed_child(a)

    print("== (a) one frame per push: ms per push, best of %d (spread); encoder push + synthesizer step measured apart" % a.reps)
    print("%4s %3s %22s %22s %22s %9s %10s %s" % ("P", "B", "Resynthesizer.push", "encoder push", "synthesizer step", "enc+syn",
                                                  "x realtime", "latency (samples)"))
    for P in (128, 512):
        for B in ((1, 8) if a.quick else (1, 8, 32)):
            r = child(["--only", "push-child", "--pool", str(P), "--batch", str(B)], a)
            if r is None:
                sys.exit(1)
            print("%4d %3d %22s %22s %22s %9.3f %10.1f %d + chunk %d = %d" %
                  (P, B, spread(r["push"]), spread(r["enc"]), spread(r["syn"]), min(r["enc"]) + min(r["syn"]),
                   (P / RATE * 1e3) / min(r["push"]), P + ENC_LAYERS + 1, P, 2 * P + ENC_LAYERS + 1), flush=True)
    print("== (b) FlowSynthesizer.feed of one frame (pool 128, %d flows): ms per feed, best of %d (spread)" % (FLOWS, a.reps))
    r = child(["--only", "feed-child"], a)
    if r is None:
        sys.exit(1)
    for B in ("1", "32"):
        print("%2s stream%s: %s" % (B, " " if B == "1" else "s", spread(r[B])), flush=True)
    if a.parent_lib:
        print("== (c) the path that was there before, against the parent commit's library")
        import synth_pool_bench
        a.seconds = max(a.seconds, 0.5)
        synth_pool_bench.old_path(a)


if __name__ == "__main__":
    main()
