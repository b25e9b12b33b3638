#!/usr/bin/env python3
"""Student synthesis on one MI355X: student.FlowSynthesizer at bench.py's student_leg flows (4 x 30 layers, R = 64, bf16).

  one-shot   synthesize 8 x 16000 in one chunk against StudentEngine.forward_flows() at the same shape and weights,
             alternating in one process, best of --reps each and the spread of each
  chunks     n = 160 / 1600 / 16000 at B = 1, 8, 32: ms per chunk, x real time at 16 kHz, cost per sample relative to
             n = 16000 at the same B, beside the recompute factor (n/st + 31) / (n/st) of both group kinds;
             eager launches against graph replay at n = 160
  launches per chunk (counted) and the time from start() to the first 160 samples

Every timed region is device-synchronised and holds >= --seconds of work after a warm-up.
usage: python tools/synth_bench.py [--seconds 0.5] [--reps 3] [--quick]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EG = importlib.import_module("sr-wavenet_amd.engine")
ST = importlib.import_module("sr-wavenet_amd.student")

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
POOL, LAT, FLOWS, RATE = 125, 16, 4, 16000


def timed(fn, seconds):
    """ms per call over a region of >= `seconds` (after two warm-up calls)."""
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
    """step(n) for ever: when the encoding runs out the clock goes back to n (not 0: the steady state, whole history)."""

    def __init__(self, syn, B, n, frames):
        self.syn, self.n = syn, n
        rng = np.random.default_rng(1)
        self.st = syn.start(torch.tensor(rng.standard_normal((B, frames, LAT)), dtype=torch.float32), seeds=7)

    def __call__(self):
        if self.st.t + self.n > self.st.limit:
            self.syn.clock.fill_(self.n)
            self.st.t = self.n
        self.syn.step(self.st, self.n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="B = 1 and 8 only")
    a = ap.parse_args()
    dt = torch.bfloat16
    fcfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, cond_channels=LAT, pool_stride=POOL, dtype=dt)

    # ---- one-shot against the training engine's forward pass
    B, T = 8, 16000
    tcfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, output_channels=40, cond_channels=LAT,
                          pool_stride=POOL, shift_input=True, dtype=dt, head_mode="mol")
    teacher = EG.WaveNetEngine(tcfg, B, T, "cuda", frozen=True)
    stu = ST.StudentEngine(teacher, fcfg, FLOWS)
    rng = np.random.default_rng(0)
    dev = lambda x: torch.tensor(x, dtype=torch.float32, device="cuda")
    cond = rng.standard_normal((B, T // POOL, LAT))
    stu.set_inputs(dev(rng.logistic(0, 1, (B, T))), None, dev(cond))
    syn = ST.FlowSynthesizer(fcfg, FLOWS, max_batch=B, max_chunk=T, max_frames=8 * T // POOL)
    for w, f in zip(syn.weights, stu.flows):
        w.params.copy_(f.params)
    syn.repack()
    step = Stepper(syn, B, T, 8 * T // POOL)
    par, new = [], []
    for _ in range(a.reps):
        par.append(timed(stu.forward_flows, a.seconds))
        new.append(timed(step, a.seconds))
    print("one-shot %d x %d: StudentEngine.forward_flows best %.3f ms (spread %.3f), FlowSynthesizer.step best %.3f ms "
          "(spread %.3f): %.2fx" % (B, T, min(par), max(par) - min(par), min(new), max(new) - min(new), min(par) / min(new)))
    print("launches per chunk: %d (1 noise + %d flows x (entry + %d groups + exit))" % (syn.launches_per_chunk, FLOWS, len(syn.groups)))
    del stu, teacher, syn, step
    torch.cuda.empty_cache()

    # ---- chunk sizes and batch sizes
    print("%4s %6s %10s %10s %12s %14s   recompute {1..16} / {32..512}" % ("B", "n", "ms/chunk", "x realtime", "vs n=16000", "eager ms"))
    for B in ((1, 8) if a.quick else (1, 8, 32)):
        frames = 4 * T // POOL
        syn = ST.FlowSynthesizer(fcfg, FLOWS, max_batch=B, max_chunk=T, max_frames=frames)
        t0 = time.perf_counter()
        st = syn.start(torch.zeros(B, frames, LAT), seeds=3)
        syn.step(st, 160)
        torch.cuda.synchronize()
        first = (time.perf_counter() - t0) * 1e3
        rows = {}
        for n in (16000, 1600, 160):
            syn.use_graphs = True
            rows[n] = timed(Stepper(syn, B, n, frames), a.seconds)
            eager = ""
            if n == 160:
                syn.use_graphs = False
                syn._graphs.clear()
                eager = "%.3f" % timed(Stepper(syn, B, n, frames), a.seconds)
            fac = lambda st_: (n / st_ + 31) / (n / st_)
            print("%4d %6d %10.3f %10.1f %12.2f %14s   %.3f / %.2f" % (B, n, rows[n], (n / RATE * 1e3) / rows[n],
                                                                       (rows[n] / n) / (rows[16000] / 16000), eager, fac(1), fac(32)))
        print("B = %d: start() to the first 160 samples %.2f ms (eager launches, first use of the kernels excluded: %s)"
              % (B, first, "no" if B == 1 else "yes"))
        del syn
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
