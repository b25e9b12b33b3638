#!/usr/bin/env python3
"""Classifier pools on one MI355X: recognizer.ClassifierPool in bf16 at the shape of tools/recognize_bench.py (the
reference's classifier: 2 x [1..512] dilations, 32 residual and 128 skip channels, 12 classes), hop 160, window 16000,
max_hops 8.  Every stream is past its first full window, so every hop emits.

  overhead    a round of one hop per stream: the all-active pool (one push of B host pieces + one step) against lockstep
              StreamClassifier.push of a [B, hop] host array and of a device tensor, B = 1, 8, 32, alternating in one
              process; and the pool's parts alone: the push (upload + srwn_audio_ring_put), the table upload, the step
  ragged      B batch-one classifiers pushed one after the other against one pool round, B = 8, 32
  occupancy   capacity 32 with 1, 8 and 32 slots holding audio: ms per round
  memory      buffer_bytes() of a capacity-32 pool beside the lockstep classifier's
  old path    with --parent-lib: StreamClassifier.push at B = 8 and FlowSynthesizer.step at B = 8 (n = 160, 1600) of this
              build against another build of the library (the parent commit's), alternating fresh processes

Every timed region is device-synchronised and holds >= --seconds of work after a warm-up; best of --reps with the spread.
Run each section in a process of its own (--only).
usage: python tools/recognize_pool_bench.py [--seconds 0.3] [--reps 3] [--only SECTION] [--parent-lib ab/libsrwn_parent.so]"""
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

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 2
R, S, CLASSES, WINDOW, HOP, MAX_HOPS = 32, 128, 12, 16000, 160, 8


def fmt(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def weights():
    import torch
    import synth_pool_bench
    synth_pool_bench.modules()      # (an older library under SRWN_LIB_PATH: its missing symbols leave the table)
    RC = importlib.import_module("sr-wavenet_amd.recognizer")
    w = RC.ClassifierWeights(DIL, R, S, CLASSES, 2, torch.bfloat16)
    rng = np.random.default_rng(0)
    w.params.copy_(torch.tensor(rng.normal(0, 0.05, w.nparams), dtype=torch.float32))
    w.repack()
    return RC, w


class Lockstep:
    """StreamClassifier.push of one hop per stream for ever (host: the audio comes as a NumPy array)."""

    def __init__(self, RC, w, B, host):
        import torch
        self.c = RC.StreamClassifier(w, max_batch=B, hop=HOP, window=WINDOW, max_hops=MAX_HOPS)
        self.st = self.c.start(B)
        rng = np.random.default_rng(1)
        assert self.c.push(self.st, rng.uniform(-1, 1, (B, WINDOW)).astype(np.float32)).shape[1] == 1
        x = rng.uniform(-1, 1, (B, HOP)).astype(np.float32)
        self.x = x if host else torch.tensor(x, device="cuda")

    def __call__(self):
        assert self.c.push(self.st, self.x).shape[1] == 1


class PoolRound:
    """One pool round for ever: `live` of the capacity's slots get one hop each in one push, then one step."""

    def __init__(self, RC, w, capacity, live):
        c = RC.StreamClassifier(w, max_batch=capacity, hop=HOP, window=WINDOW, max_hops=MAX_HOPS)
        self.P = P = c.pool()
        self.us = P.join(live)
        rng = np.random.default_rng(1)
        for at in range(0, WINDOW, MAX_HOPS * HOP):
            n = min(MAX_HOPS * HOP, WINDOW - at)
            P.push(self.us, [rng.uniform(-1, 1, n).astype(np.float32) for _ in self.us])
            P.step()
        assert all(P.emitted[u] == 1 for u in self.us)
        self.x = [rng.uniform(-1, 1, HOP).astype(np.float32) for _ in self.us]

    def __call__(self):
        self.P.push(self.us, self.x)
        out = self.P.step()
        assert len(out) == len(self.us)

    # the round's parts alone (the clocks are moved by hand: only the time is of interest)
    def push_only(self):
        self.P.push(self.us, self.x)
        self.P._consumed[self.us] = self.P._received[self.us]

    def upload_only(self):
        import torch
        P = self.P
        P.table.copy_(torch.from_numpy(np.stack([P._consumed, P._consumed + HOP], 1)))

    def step_only(self):
        self.P._received[self.us] += HOP
        assert len(self.P.step()) == len(self.us)


def overhead(a):
    from synth_pool_bench import timed
    RC, w = weights()
    print("== a round of one hop per stream, ms, best of %d (spread)" % a.reps)
    for B in (1, 8, 32):
        ls_h, ls_d, pool = Lockstep(RC, w, B, True), Lockstep(RC, w, B, False), PoolRound(RC, w, B, B)
        t = {k: [] for k in ("lockstep host", "lockstep device", "pool", "pool push", "pool table", "pool step")}
        for _ in range(a.reps):
            t["lockstep host"].append(timed(ls_h, a.seconds))
            t["lockstep device"].append(timed(ls_d, a.seconds))
            t["pool"].append(timed(pool, a.seconds))
        for _ in range(a.reps):
            t["pool push"].append(timed(pool.push_only, a.seconds))
            t["pool table"].append(timed(pool.upload_only, a.seconds))
            t["pool step"].append(timed(pool.step_only, a.seconds))
        print("B = %2d: " % B + "; ".join("%s %s" % (k, fmt(v)) for k, v in t.items()), flush=True)


def ragged(a):
    from synth_pool_bench import timed
    RC, w = weights()
    print("== ragged callers: B batch-one pushes against one pool round, ms, best of %d (spread)" % a.reps)
    for B in (8, 32):
        ones = [Lockstep(RC, w, 1, True) for _ in range(B)]
        pool = PoolRound(RC, w, B, B)

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
    RC, w = weights()
    print("== capacity 32, ms per round by slots holding audio, best of %d (spread)" % a.reps)
    for live in (1, 8, 32):
        pool = PoolRound(RC, w, 32, live)
        print("live %2d of 32: round %s; step alone %s" % (live, fmt([timed(pool, a.seconds) for _ in range(a.reps)]),
                                                          fmt([timed(pool.step_only, a.seconds) for _ in range(a.reps)])), flush=True)


def memory(a):
    RC, w = weights()
    c = RC.StreamClassifier(w, max_batch=32, hop=HOP, window=WINDOW, max_hops=MAX_HOPS)
    lock = c.buffer_bytes()
    pool = c.pool().buffer_bytes()
    print("== device bytes, capacity / batch 32")
    print("lockstep: total %d  %s" % (sum(lock.values()), json.dumps(lock)))
    print("pool:     total %d  %s" % (sum(pool.values()), json.dumps(pool)))
    print("launches per step: %d either way" % c.launches_per_step)


def old_path_child(a):
    from synth_pool_bench import timed
    RC, w = weights()
    ls = Lockstep(RC, w, 8, False)
    print("ABRESULT " + json.dumps({"push": [timed(ls, a.seconds) for _ in range(a.reps)]}))


def old_path(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so")), ("parent", os.path.join(ROOT, a.parent_lib))]
    print("== StreamClassifier.push, B = 8, one hop: this build against %s, alternating fresh processes" % a.parent_lib)
    got = {k: [] for k, _ in libs}
    for r in range(a.rounds):
        for name, path in libs:
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "old-path-child", "--seconds", str(a.seconds),
                                 "--reps", str(a.reps)], env=dict(os.environ, SRWN_LIB_PATH=path), cwd=ROOT, capture_output=True,
                                text=True, timeout=300)
            line = [l for l in pr.stdout.splitlines() if l.startswith("ABRESULT ")]
            if pr.returncode or not line:
                print("FAILED", name, pr.stderr[-2000:], flush=True)
                return
            d = json.loads(line[0][9:])["push"]
            got[name] += d
            print("round %d %-6s %s" % (r, name, " ".join("%.4f" % m for m in d)), flush=True)
    t, p = got["this"], got["parent"]
    print("push: this build best %.4f ms (spread %.4f), parent best %.4f ms (spread %.4f): difference %+.4f ms"
          % (min(t), max(t) - min(t), min(p), max(p) - min(p), min(t) - min(p)))
    import synth_pool_bench
    a.seconds = max(a.seconds, 0.5)
    synth_pool_bench.old_path(a)


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
    for name in ("overhead", "ragged", "occupancy", "memory"):      # (one process per section is the cleaner measurement)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name, "--seconds", str(a.seconds), "--reps",
                        str(a.reps)], cwd=ROOT, check=True)
    if a.parent_lib:
        old_path(a)


if __name__ == "__main__":
    main()
