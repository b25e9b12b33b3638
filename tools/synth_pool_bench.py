#!/usr/bin/env python3
"""Student synthesis pools on one MI355X: student.SynthPool at bench.py's student_leg flows (4 x 30 layers, R = 64, bf16).

  overhead    all-active pool against FlowSynthesizer.step at the same B (1, 8, 32) and n (160, 1600), alternating in one
              process under graph replay, best of --reps each and the spread of each
  old path    FlowSynthesizer.step of this build against another build of the library (--parent-lib: the parent
              commit's), B = 8, n = 160 and 1600, alternating fresh processes (both through the ctypes binding)
  occupancy   ms per chunk at capacity 32 with 1, 8 and 32 live slots
  churn       capacity 32 fed with requests of 0.1 - 1 s of audio, a new one joining at the next chunk boundary: the share
              of slot-steps that were useful, aggregate x real time against a static batch of 32, and what a join of 1
              and of 8 streams costs (conditioning rows + reset + table upload, device-synchronised)

Every timed region is device-synchronised and holds >= --seconds of work after a warm-up.
usage: python tools/synth_pool_bench.py [--seconds 0.5] [--reps 3] [--parent-lib ab/libsrwn_parent.so] [--only SECTION]"""
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

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
POOL, LAT, FLOWS, RATE = 125, 16, 4, 16000


def modules():
    """The package, after dropping from the signature table what an older library (SRWN_LIB_PATH) does not export: the old
    path needs none of it."""
    import ctypes
    L = importlib.import_module("sr-wavenet_amd._lib")
    if os.environ.get("SRWN_LIB_PATH"):
        lib = ctypes.CDLL(L.LIB_PATH)
        for name in [n for n in L.SIGNATURES if not hasattr(lib, n)]:
            del L.SIGNATURES[name]
    return importlib.import_module("sr-wavenet_amd.engine"), importlib.import_module("sr-wavenet_amd.student")


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


class Stepper:
    """FlowSynthesizer.step(n) for ever (tools/synth_bench.py): at the encoding's end the clock goes back to n."""

    def __init__(self, syn, B, n, frames):
        import torch
        self.syn, self.n = syn, n
        rng = np.random.default_rng(1)
        self.st = syn.start(torch.tensor(rng.standard_normal((B, frames, LAT)), dtype=torch.float32), seeds=7)

    def __call__(self):
        if self.st.t + self.n > self.st.limit:
            self.syn.clock.fill_(self.n)
            self.st.t = self.n
        self.syn.step(self.st, self.n)


class PoolStepper:
    """SynthPool.step(n) for ever with `live` of the slots holding a stream: at the encodings' end every live slot's clock
    goes back to n through the pool's own table upload.  A re-join would not do: it zeroes the histories, and the regions
    measure the steady state with the whole history behind every chunk, as Stepper does for the synthesizer."""

    def __init__(self, syn, live, n, frames):
        self.P, self.n, self.limit = syn.pool(), n, frames * POOL
        rng = np.random.default_rng(1)
        self.us = self.P.join([rng.standard_normal((frames, LAT)).astype(np.float32) for _ in range(live)], 7)

    def __call__(self):
        P = self.P
        if P._t[self.us[0]] + self.n > self.limit:
            P._t[self.us] = self.n
            P._upload()
        P.step(self.n)


def spread(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def overhead(a, fcfg, ST):
    import torch
    print("== pool against synthesizer, all slots live, graph replay; ms per chunk, best of %d (spread)" % a.reps)
    static = {}
    for B in (1, 8, 32):
        frames = 512
        syn = ST.FlowSynthesizer(fcfg, FLOWS, max_batch=B, max_chunk=1600, max_frames=frames)
        for n in (160, 1600):
            s, p = [], []
            for _ in range(a.reps):
                s.append(timed(Stepper(syn, B, n, frames), a.seconds))
                p.append(timed(PoolStepper(syn, B, n, frames), a.seconds))
            static[(B, n)] = min(s)
            print("B = %2d n = %4d: FlowSynthesizer.step %s, SynthPool.step %s: %+.1f %%"
                  % (B, n, spread(s), spread(p), (min(p) / min(s) - 1) * 100), flush=True)
        del syn
        torch.cuda.empty_cache()
    return static


def occupancy(a, fcfg, ST):
    import torch
    print("== occupancy: capacity 32, ms per chunk by live slots, best of %d (spread)" % a.reps)
    syn = ST.FlowSynthesizer(fcfg, FLOWS, max_batch=32, max_chunk=1600, max_frames=512)
    for n in (160, 1600):
        for live in (1, 8, 32):
            v = [timed(PoolStepper(syn, live, n, 512), a.seconds) for _ in range(a.reps)]
            print("n = %4d live %2d of 32: %s" % (n, live, spread(v)), flush=True)
    del syn
    torch.cuda.empty_cache()


def churn(a, fcfg, ST, static_ms):
    import torch
    n, cap, frames = 160, 32, RATE // POOL
    print("== churn: capacity %d, n = %d, requests of 0.1 - 1 s, a new one at the next chunk boundary" % (cap, n))
    syn = ST.FlowSynthesizer(fcfg, FLOWS, max_batch=cap, max_chunk=n, max_frames=frames)
    rng = np.random.default_rng(3)
    enc = rng.standard_normal((frames, LAT)).astype(np.float32)

    def request():
        ln = int(rng.integers(RATE // 10, RATE + 1))
        return enc[:-(-ln // POOL)], ln

    res = []
    P = syn.pool()                                     # one pool for all rounds: its graph is captured in the first
    joins = 0
    for rep in range(a.reps + 1):                      # (the first round warms the kernels and captures the graph: not kept)
        P.leave(P.active)                              # drained between rounds
        useful = steps = 0
        j0 = joins
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < max(a.seconds, 1.0):
            free = P.free
            if free:
                rq = [request() for _ in free]
                P.join([r[0] for r in rq], 11 + joins, None, [r[1] for r in rq])
                joins += len(rq)
            _, ran = P.step(n)
            useful += int(ran.sum())
            steps += 1
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if rep:
            res.append((useful / (cap * n * steps), useful / RATE / wall, wall / steps * 1e3, joins - j0))
    best = max(res, key=lambda r: r[1])
    line = "useful slot-steps %.1f %%, aggregate %.0fx real time (best of %d; %.3f ms per pool step with its joins, %d joins)" \
        % (best[0] * 100, best[1], a.reps, best[2], best[3])
    if static_ms:
        line += "; static batch of 32: %.0fx" % (cap * n / RATE * 1e3 / static_ms)
    print(line)
    for k in (1, 8):
        cost = []
        for _ in range(10):
            P = syn.pool()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.join([enc] * k, 5)
            torch.cuda.synchronize()
            cost.append((time.perf_counter() - t0) * 1e3)
        print("join of %d stream%s: %.3f ms (best of 10, median %.3f)" % (k, "" if k == 1 else "s", min(cost), float(np.median(cost))))
    del syn
    torch.cuda.empty_cache()


def old_path_child(a, fcfg, ST):
    out = {}
    syn = ST.FlowSynthesizer(fcfg, FLOWS, max_batch=8, max_chunk=1600, max_frames=512)
    for n in (160, 1600):
        out[str(n)] = [timed(Stepper(syn, 8, n, 512), a.seconds) for _ in range(a.reps)]
    print("ABRESULT " + json.dumps(out))


def old_path(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so")), ("parent", os.path.join(ROOT, a.parent_lib))]
    print("== FlowSynthesizer.step, B = 8: this build against %s, alternating fresh processes" % a.parent_lib)
    got = {k: {"160": [], "1600": []} for k, _ in libs}
    for r in range(a.rounds):
        for name, path in libs:
            env = dict(os.environ, SRWN_LIB_PATH=path)
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "old-path-child", "--seconds", str(a.seconds),
                                 "--reps", str(a.reps)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
            line = [l for l in pr.stdout.splitlines() if l.startswith("ABRESULT ")]
            if pr.returncode or not line:
                print("FAILED", name, pr.stderr[-2000:], flush=True)
                return
            d = json.loads(line[0][9:])
            for k in d:
                got[name][k] += d[k]
            print("round %d %-6s %s" % (r, name, "  ".join("n = %s: %s" % (k, " ".join("%.4f" % m for m in d[k])) for k in d)), flush=True)
    for k in ("160", "1600"):
        t, p = got["this"][k], got["parent"][k]
        print("n = %4s: this build best %.4f ms (spread %.4f), parent best %.4f ms (spread %.4f): difference %+.4f ms"
              % (k, min(t), max(t) - min(t), min(p), max(p) - min(p), min(t) - min(p)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for the old-path A/B")
    ap.add_argument("--only", default=None, choices=["overhead", "old-path", "old-path-child", "occupancy", "churn"])
    a = ap.parse_args()
    if a.only == "old-path" or (a.only is None and a.parent_lib):
        if not a.parent_lib:
            sys.exit("--only old-path needs --parent-lib")
        old_path(a)
        if a.only:
            return
    import torch
    EG, ST = modules()
    fcfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, cond_channels=LAT, pool_stride=POOL,
                          dtype=torch.bfloat16)
    if a.only == "old-path-child":
        return old_path_child(a, fcfg, ST)
    static = overhead(a, fcfg, ST) if a.only in (None, "overhead") else {}
    if a.only in (None, "occupancy"):
        occupancy(a, fcfg, ST)
    if a.only in (None, "churn"):
        churn(a, fcfg, ST, static.get((32, 160)))


if __name__ == "__main__":
    main()
