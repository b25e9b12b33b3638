#!/usr/bin/env python3
"""Scorer pools on one MI355X: scorer.ScorerPool in bf16 at the shape of tools/score_bench.py (BASELINE config 5's stack: 3 x
[1..512] dilations, 64 residual and 256 skip channels, 256 mu-law classes), max_chunk 1600, 160 samples per slot per round in
the steady state (every stream has its whole history behind it), graph replay.

  overhead    a round of 160 samples per stream: the all-active pool (one push of B host pieces + one step) against lockstep
              StreamScorer.push of a [B, 160] host array and of a device tensor, B = 1, 8, 32, alternating in one process;
              and the pool's parts alone: the push (upload + srwn_audio_ring_put) and the step
  ragged      B batch-one scorers pushed one after the other against one pool round, B = 1, 8, 32
  occupancy   capacity 32 with 1, 8 and 32 slots holding audio: ms per round and per step
  memory      buffer_bytes() of a capacity-32 pool beside the lockstep scorer's and beside 32 batch-one scorers'
  old path    with --parent-lib: StreamScorer.push and StreamClassifier.push at B = 8 of this build against another build
              of the library (the parent commit's), alternating fresh processes

Every timed region is device-synchronised and holds >= --seconds of work after a warm-up; best of --reps with the spread.
Each section runs in a process of its own (--only).
usage: python tools/score_pool_bench.py [--seconds 0.3] [--reps 3] [--only SECTION] [--parent-lib ab/libsrwn_parent.so]"""
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

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
R, S, CLASSES, MAX_CHUNK, N, WARM = 64, 256, 256, 1600, 160, 3200


def fmt(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def weights():
    import torch
    import synth_pool_bench
    synth_pool_bench.modules()      # (an older library under SRWN_LIB_PATH: its missing symbols leave the table)
    SC = importlib.import_module("sr-wavenet_amd.scorer")
    w = SC.ScorerWeights(DIL, R, S, CLASSES, 2, torch.bfloat16)
    rng = np.random.default_rng(0)
    w.params.copy_(torch.tensor(rng.normal(0, 0.05, w.nparams), dtype=torch.float32))
    w.repack()
    return SC, w


class Lockstep:
    """StreamScorer.push of 160 samples per stream for ever (host: the audio comes as a NumPy array)."""

    def __init__(self, SC, w, B, host):
        import torch
        self.c = SC.StreamScorer(w, max_batch=B, max_chunk=MAX_CHUNK)
        self.st = self.c.start(B)
        rng = np.random.default_rng(1)
        self.c.push(self.st, rng.uniform(-1, 1, (B, WARM)).astype(np.float32))
        x = rng.uniform(-1, 1, (B, N)).astype(np.float32)
        self.x = x if host else torch.tensor(x, device="cuda")

    def __call__(self):
        assert self.c.push(self.st, self.x).shape[1] == N


class PoolRound:
    """One pool round for ever: `live` of the capacity's slots get 160 samples each in one push, then one step."""

    def __init__(self, SC, w, capacity, live):
        c = SC.StreamScorer(w, max_batch=capacity, max_chunk=MAX_CHUNK)
        self.P = P = c.pool()
        self.us = P.join(live)
        rng = np.random.default_rng(1)
        for at in range(0, WARM, MAX_CHUNK):
            P.push(self.us, [rng.uniform(-1, 1, MAX_CHUNK).astype(np.float32) for _ in self.us])
            P.step()
        assert all(P.scored[u] == WARM for u in self.us)
        self.x = [rng.uniform(-1, 1, N).astype(np.float32) for _ in self.us]

    def __call__(self):
        self.P.push(self.us, self.x)
        out = self.P.step()
        assert len(out) == len(self.us)

    # the round's parts alone (the clocks are moved by hand: only the time is of interest)
    def push_only(self):
        self.P.push(self.us, self.x)
        self.P._scored[self.us] = self.P._received[self.us]

    def step_only(self):
        self.P._received[self.us] += N
        assert len(self.P.step()) == len(self.us)


def overhead(a):
    from synth_pool_bench import timed
    SC, w = weights()
    print("== a round of %d samples per stream, ms, best of %d (spread)" % (N, a.reps))
    for B in (1, 8, 32):
        ls_h, ls_d, pool = Lockstep(SC, w, B, True), Lockstep(SC, w, B, False), PoolRound(SC, w, B, B)
        t = {k: [] for k in ("lockstep host", "lockstep device", "pool", "pool push", "pool step")}
        for _ in range(a.reps):
            t["lockstep host"].append(timed(ls_h, a.seconds))
            t["lockstep device"].append(timed(ls_d, a.seconds))
            t["pool"].append(timed(pool, a.seconds))
        for _ in range(a.reps):
            t["pool push"].append(timed(pool.push_only, a.seconds))
            t["pool step"].append(timed(pool.step_only, a.seconds))
        print("B = %2d: " % B + "; ".join("%s %s" % (k, fmt(v)) for k, v in t.items()), flush=True)
        print("        pool round - lockstep host push: %+.3f ms; launches per step: %d lockstep (+ mu-law and the staging copies "
              "outside the graph), %d pool" % (min(t["pool"]) - min(t["lockstep host"]), ls_h.c.launches_per_step,
                                              pool.P.launches_per_step), flush=True)


def ragged(a):
    from synth_pool_bench import timed
    SC, w = weights()
    print("== ragged callers: B batch-one pushes against one pool round, ms, best of %d (spread)" % a.reps)
    for B in (1, 8, 32):
        ones = [Lockstep(SC, w, 1, True) for _ in range(B)]
        pool = PoolRound(SC, w, B, B)

        def each():
            for o in ones:
                o()
        te, tp = [], []
        for _ in range(a.reps):
            te.append(timed(each, a.seconds))
            tp.append(timed(pool, a.seconds))
        print("B = %2d: %d x batch-one push %s; one pool round %s: %.1f x" % (B, B, fmt(te), fmt(tp), min(te) / min(tp)), flush=True)


def occupancy(a):
    from synth_pool_bench import timed
    SC, w = weights()
    print("== capacity 32, ms per round by slots holding audio, best of %d (spread)" % a.reps)
    for live in (1, 8, 32):
        pool = PoolRound(SC, w, 32, live)
        print("live %2d of 32: round %s; step alone %s" % (live, fmt([timed(pool, a.seconds) for _ in range(a.reps)]),
                                                          fmt([timed(pool.step_only, a.seconds) for _ in range(a.reps)])), flush=True)


def memory(a):
    SC, w = weights()
    c = SC.StreamScorer(w, max_batch=32, max_chunk=MAX_CHUNK)
    lock = c.buffer_bytes()
    pool = c.pool().buffer_bytes()
    one = SC.StreamScorer(w, max_batch=1, max_chunk=MAX_CHUNK).buffer_bytes()
    print("== device bytes, capacity / batch 32, max_chunk %d" % MAX_CHUNK)
    print("lockstep: total %d  %s" % (sum(lock.values()), json.dumps(lock)))
    print("pool:     total %d  %s" % (sum(pool.values()), json.dumps(pool)))
    print("batch 1:  total %d (x 32 callers = %d; the images %d are shared)  %s"
          % (sum(one.values()), 32 * (sum(one.values()) - one["images"]) + one["images"], one["images"], json.dumps(one)))
    print("launches per step: %d either way" % c.launches_per_step)


def old_path_child(a):
    from synth_pool_bench import timed
    SC, w = weights()
    ls = Lockstep(SC, w, 8, False)
    print("ABRESULT " + json.dumps({"push": [timed(ls, a.seconds) for _ in range(a.reps)]}))


def old_path(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so")), ("parent", os.path.join(ROOT, a.parent_lib))]
    print("== StreamScorer.push, B = 8, %d samples: this build against %s, alternating fresh processes" % (N, a.parent_lib))
    got = {k: [] for k, _ in libs}
    for r in range(a.rounds):
        for name, path in libs:
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "old-path-child", "--seconds",
                                 str(max(a.seconds, 0.5)), "--reps", str(a.reps)], env=dict(os.environ, SRWN_LIB_PATH=path),
                                cwd=ROOT, capture_output=True, text=True, timeout=300)
            line = [l for l in pr.stdout.splitlines() if l.startswith("ABRESULT ")]
            if pr.returncode or not line:
                print("FAILED", name, pr.stderr[-2000:], flush=True)
                return
            d = json.loads(line[0][9:])["push"]
            got[name] += d
            print("round %d %-6s %s" % (r, name, " ".join("%.4f" % m for m in d)), flush=True)
    t, p = got["this"], got["parent"]
    print("push: this build best %.4f ms (spread %.4f), parent best %.4f ms (spread %.4f): difference %+.4f ms"
          % (min(t), max(t) - min(t), min(p), max(p) - min(p), min(t) - min(p)), flush=True)
    import score_bench
    score_bench.old_path(a)      # StreamClassifier.push at B = 8, the same way


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for the old path")
    sections = {"overhead": overhead, "ragged": ragged, "occupancy": occupancy, "memory": memory, "old-path": old_path,
                "old-path-child": old_path_child}
    ap.add_argument("--only", default=None, choices=sorted(sections))
    a = ap.parse_args()
    if a.only == "old-path" and not a.parent_lib:
        sys.exit("--only old-path needs --parent-lib")
    if a.only:
        return sections[a.only](a)
    for name in ("overhead", "ragged", "occupancy", "memory"):      # one process per section
        subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name, "--seconds", str(a.seconds), "--reps",
                        str(a.reps)], cwd=ROOT, check=True)
    if a.parent_lib:
        old_path(a)


if __name__ == "__main__":
    main()
