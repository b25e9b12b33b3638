#!/usr/bin/env python3
"""Encoder and resynthesis pools on one MI355X, at tools/live_bench.py's shapes: encoder 30 layers x 128 channels (256 skip,
16 latent channels), student 4 flows x 30 layers, R = 64, rings of 32 frames, both bf16, pool_stride 128 and 512.

  (i)   pool vs stream   ms per round of one frame's worth of audio per stream (NumPy in, NumPy out), steady state, B = 1, 8,
                         32: an all-active ResynthesisPool (push + step) against Resynthesizer.stream(batch=B).push,
                         alternating in one process
  (ii)  encoder          EncoderPool push + step with B one-frame items against FrameEncoder.push at batch B, and against B
                         separate batch-one push calls (what ragged callers had to do before), host audio in all three
  (iii) churn            capacity 32, clips of 0.1-1 s, a new stream joins when one leaves, push sizes drawn per stream:
                         useful slot-steps and aggregate x real time (16 kHz)
  (iv)  old paths        FrameEncoder.push (B = 8, pool 128) and FlowSynthesizer.step (B = 8) of this build against another
                         build of the library (--parent-lib: the parent commit's), alternating fresh processes through
                         SRWN_LIB_PATH

Every measurement runs in a fresh child process under a time limit of its own, one after the other; the first that fails
ends the run.  Every timed region is device-synchronised and holds >= --seconds of work after a warm-up; best of --reps,
with the spread.
usage: python tools/resynth_pool_bench.py [--seconds 0.3] [--reps 3] [--parent-lib ab/libsrwn_parent.so] [--quick]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

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


def _models(P, B, nsyn):
    import torch
    M = importlib.import_module("sr-wavenet_amd.model")
    dt = torch.bfloat16
    enc = M.AudioEncoder(ENC_LAYERS, skip_channels=S, latent_channels=LAT, pool_stride=P, dtype=dt, max_batch=B,
                         max_frames=FRAMES)
    syns = [M.StudentSynthesizer(DIL, FLOWS, dilation_channels=64, latent_channels=LAT, pool_stride=P, dtype=dt, max_batch=B,
                                 max_chunk=P, max_frames=FRAMES) for _ in range(nsyn)]
    return M, enc, syns


def pool_child(a):
    """(i) for one (pool, B)."""
    from synth_pool_bench import timed
    P, B = a.pool, a.batch
    M, enc, (syn_s, syn_p) = _models(P, B, 2)
    rng = np.random.default_rng(0)
    block = rng.uniform(-1, 1, (B, P)).astype(np.float32)
    head = rng.uniform(-1, 1, (B, P + ENC_LAYERS + 1)).astype(np.float32)
    s = M.Resynthesizer(enc, syn_s).stream(batch=B, seed=1, chunk_size=P)
    assert s.push(head).shape == (B, P, 1)
    rp = M.Resynthesizer(enc, syn_p).pool(chunk_size=P)
    slots = rp.join(seed=1, n=B)
    rp.push(slots, list(head))
    assert sorted(rp.step()) == slots
    rows = list(block)

    def stream_push():
        assert s.push(block).shape[1] == P

    def pool_round():
        rp.push(slots, rows)
        out = rp.step()
        assert len(out) == B and len(out[slots[0]]) == P

    ts, tp = [], []
    for _ in range(a.reps):
        ts.append(timed(stream_push, a.seconds))
        tp.append(timed(pool_round, a.seconds))
    assert s.t > FRAMES * P and rp.t[0] > FRAMES * P, "the rings wrapped during the measurement"
    print("RESULT " + json.dumps(dict(pool=P, B=B, stream=ts, resynth_pool=tp)))


def enc_child(a):
    """(ii) for one (pool, B)."""
    import torch
    from synth_pool_bench import timed
    P, B = a.pool, a.batch
    _, enc, _ = _models(P, B, 0)
    fe = enc._eng
    rng = np.random.default_rng(0)
    block = rng.uniform(-1, 1, (B, P)).astype(np.float32)
    head = rng.uniform(-1, 1, (B, P + ENC_LAYERS + 1)).astype(np.float32)
    hblock, rows = torch.as_tensor(block), list(block)
    ep = fe.pool()
    slots = ep.join(B)
    ep.push(slots, list(head))
    assert len(ep.step()) == B
    st = fe.start(B)
    fe.push(st, torch.as_tensor(head))
    ones = [fe.start(1) for _ in range(B)]
    for i, o in enumerate(ones):
        fe.push(o, torch.as_tensor(head[i:i + 1]))

    def pool_round():
        ep.push(slots, rows)
        out = ep.step()
        assert len(out) == B and out[slots[0]].shape[0] == 1

    def lockstep():
        assert fe.push(st, hblock).shape[1] == 1

    def one_by_one():
        for i, o in enumerate(ones):
            assert fe.push(o, hblock[i:i + 1]).shape[1] == 1

    t = {"epool": [], "lockstep": [], "separate": []}
    for _ in range(a.reps):
        t["epool"].append(timed(pool_round, a.seconds))
        t["lockstep"].append(timed(lockstep, a.seconds))
        t["separate"].append(timed(one_by_one, a.seconds))
    print("RESULT " + json.dumps(dict(pool=P, B=B, **t)))


def churn_child(a):
    """(iii): requests of 0.1-1 s keep a pool of 32 slots full; every round pushes a drawn piece per stream and steps."""
    import torch
    P, cap = a.pool, 32
    M, enc, (syn,) = _models(P, cap, 1)
    rp = M.Resynthesizer(enc, syn).pool(chunk_size=P)
    rng = np.random.default_rng(2)
    left, runs = {}, []

    def refill():
        for u in rp.join(seed=int(rng.integers(1 << 30)), n=len(rp.free)) if rp.free else []:
            left[u] = int(rng.integers(RATE // 10, RATE + 1))

    for rep in range(a.reps + 1):        # (the first region is the warm-up)
        rounds = useful = made = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < max(a.seconds, 1.0):
            refill()
            us, xs, fin = [], [], []
            for u in rp.active:
                k = min(int(rng.integers(0, 2 * P + 1)), left.get(u, 0), rp.audio_room(u))
                if k:
                    us.append(u); xs.append(rng.uniform(-1, 1, k).astype(np.float32))
                    left[u] -= k
                if left.get(u) == 0:
                    fin.append(u); del left[u]
            if us:
                rp.push(us, xs)
            if fin:
                rp.finish(fin)
            out = rp.step()
            rounds += 1
            useful += len(out)
            made += sum(len(y) for y in out.values())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep:
            runs.append(dict(ms_per_round=dt / rounds * 1e3, useful=useful / (rounds * cap), xrt=made / RATE / dt))
    print("RESULT " + json.dumps(dict(pool=P, runs=runs)))


def enc_old_child(a):
    """(iv): FrameEncoder.push, B = 8, pool 128, one frame per push from the device, on whatever library SRWN_LIB_PATH names."""
    import torch
    from synth_pool_bench import modules, timed
    modules()
    E = importlib.import_module("sr-wavenet_amd.encoder")
    w = E.EncoderWeights(ENC_LAYERS, 128, S, LAT, 2, torch.bfloat16)
    fe = E.FrameEncoder(w, 128, max_batch=8, max_frames=FRAMES)
    rng = np.random.default_rng(0)
    st = fe.start(8)
    fe.push(st, torch.as_tensor(rng.uniform(-1, 1, (8, 128 + ENC_LAYERS + 1)).astype(np.float32)).to("cuda"))
    block = torch.as_tensor(rng.uniform(-1, 1, (8, 128)).astype(np.float32)).to("cuda")

    def push():
        assert fe.push(st, block).shape[1] == 1

    print("ABRESULT " + json.dumps({"push": [timed(push, a.seconds) for _ in range(a.reps)]}))


def child(args, a, env=None, tag="RESULT "):
    """A measurement in a fresh process under its own time limit -> the dict it reports, or None when it failed."""
    cmd = [sys.executable, os.path.abspath(__file__), "--seconds", str(a.seconds), "--reps", str(a.reps)] + args
    try:
        pr = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=STEP_LIMIT)
    except subprocess.TimeoutExpired:
        print("FAILED (time limit of %d s): %s" % (STEP_LIMIT, " ".join(args)), flush=True)
        return None
    line = [l for l in pr.stdout.splitlines() if l.startswith(tag)]
    if pr.returncode or not line:
        print("FAILED (exit %d): %s\n%s" % (pr.returncode, " ".join(args), pr.stderr[-2000:]), flush=True)
        return None
    return json.loads(line[0][len(tag):])


def old_paths(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so")), ("parent", os.path.join(ROOT, a.parent_lib))]
    print("== (iv) FrameEncoder.push, B = 8, pool 128: this build against %s, alternating fresh processes" % a.parent_lib)
    got = {k: [] for k, _ in libs}
    for r in range(a.rounds):
        for name, path in libs:
            d = child(["--only", "enc-old-child"], a, env=dict(os.environ, SRWN_LIB_PATH=path), tag="ABRESULT ")
            if d is None:
                sys.exit(1)
            got[name] += d["push"]
            print("round %d %-6s %s" % (r, name, " ".join("%.4f" % m for m in d["push"])), flush=True)
    t, p = got["this"], got["parent"]
    print("push: this build best %.4f ms (spread %.4f), parent best %.4f ms (spread %.4f): difference %+.4f ms"
          % (min(t), max(t) - min(t), min(p), max(p) - min(p), min(t) - min(p)), flush=True)
    import synth_pool_bench
    synth_pool_bench.old_path(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="B = 1 and 8 only")
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for (iv)")
    ap.add_argument("--only", default=None, choices=["pool-child", "enc-child", "churn-child", "enc-old-child", "old-paths"])
    ap.add_argument("--pool", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    if a.only in ("pool-child", "enc-child", "churn-child", "enc-old-child"):
        return {"pool-child": pool_child, "enc-child": enc_child, "churn-child": churn_child,
                "enc-old-child": enc_old_child}[a.only](a)
    if a.only == "old-paths":
        if not a.parent_lib:
            sys.exit("--only old-paths needs --parent-lib")
        a.seconds = max(a.seconds, 0.5)
        return old_paths(a)
    Bs = (1, 8) if a.quick else (1, 8, 32)
    print("== (i) one frame's worth of audio per stream and round: ms per round, best of %d (spread)" % a.reps)
    print("%4s %3s %24s %24s %10s %12s" % ("P", "B", "Resynthesizer.stream", "ResynthesisPool", "pool - str", "pool x rt"))
    for P in (128, 512):
        for B in Bs:
            r = child(["--only", "pool-child", "--pool", str(P), "--batch", str(B)], a)
            if r is None:
                sys.exit(1)
            print("%4d %3d %24s %24s %+10.3f %12.1f" % (P, B, spread(r["stream"]), spread(r["resynth_pool"]),
                                                        min(r["resynth_pool"]) - min(r["stream"]),
                                                        B * (P / RATE * 1e3) / min(r["resynth_pool"])), flush=True)
    print("== (ii) the encoder alone, one frame per stream from host audio: ms per round, best of %d (spread)" % a.reps)
    print("%4s %3s %24s %24s %24s" % ("P", "B", "EncoderPool push+step", "FrameEncoder.push [B]", "B x FrameEncoder.push [1]"))
    for P in (128, 512):
        for B in Bs:
            r = child(["--only", "enc-child", "--pool", str(P), "--batch", str(B)], a)
            if r is None:
                sys.exit(1)
            print("%4d %3d %24s %24s %24s" % (P, B, spread(r["epool"]), spread(r["lockstep"]), spread(r["separate"])), flush=True)
    print("== (iii) churn: 32 slots, clips of 0.1-1 s, a new stream joins when one leaves, pieces of 0..2 P samples")
    for P in (128, 512):
        r = child(["--only", "churn-child", "--pool", str(P)], a)
        if r is None:
            sys.exit(1)
        for k, name in (("ms_per_round", "ms per round"), ("useful", "useful slot-steps"), ("xrt", "aggregate x real time")):
            v = [run[k] for run in r["runs"]]
            print("P = %3d %-22s best %.3f (spread %.3f)" % (P, name, min(v) if k == "ms_per_round" else max(v), max(v) - min(v)),
                  flush=True)
    if a.parent_lib:
        a.seconds = max(a.seconds, 0.5)
        old_paths(a)


if __name__ == "__main__":
    main()
