#!/usr/bin/env python3
"""Student flow inversion on one MI355X: student.FlowInverter over bench.py's student_leg flows (4 x 30 layers, R = 64,
bf16), audio -> noise + log scale.

Per batch B = 1 / 32 / 256 and cut (chunks of 160, chunks of 1600, one shot) the wall time of inverting --samples samples
of every stream (device-synchronised, inputs on the device; after a warm-up run of the same cut): microseconds per sample
of a stream, and the real-time factor of a stream at 16 kHz (all B streams run at that factor at once).  Best of --reps
with the spread.  A step is one pass of every flow's 30 layers, so the expectation is the generators' per-step cost times
the number of flows, whatever B <= 32 is; each further group of 32 streams is one more workgroup on a CU of its own.
usage: python tools/invert_bench.py [--samples 3200] [--reps 3] [--batches 1,32,256]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
FLOWS, LAT, POOL, RATE = 4, 16, 160, 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3200, help="samples per stream and run (a multiple of %d)" % POOL)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,32,256")
    a = ap.parse_args()
    import torch
    EG = importlib.import_module("sr-wavenet_amd.engine")
    ST = importlib.import_module("sr-wavenet_amd.student")
    T = a.samples
    if T < POOL or T % POOL:
        sys.exit("--samples must be a positive multiple of %d" % POOL)
    cfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, cond_channels=LAT, pool_stride=POOL,
                         dtype=torch.bfloat16)
    rng = np.random.default_rng(0)
    print("%d flows x %d layers, R = 64, bf16; %d samples per stream; best of %d (spread)" % (FLOWS, len(DIL), T, a.reps))
    print("%4s %9s %24s %12s" % ("B", "cut", "us per sample", "x realtime"))
    for B in [int(b) for b in a.batches.split(",")]:
        inv = ST.FlowInverter(cfg, FLOWS, max_batch=B)
        cond = torch.tensor(rng.standard_normal((B, T // POOL, LAT)), dtype=torch.float32)
        audio = torch.tensor(rng.uniform(-1, 1, (B, T)), dtype=torch.float32, device="cuda")

        def run(chunk):
            st = inv.start(cond)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(0, T, chunk):
                inv.step(st, audio[:, t:t + chunk])
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for name, chunk in (("160", 160), ("1600", 1600), ("one shot", T)):
            run(chunk)
            v = [run(chunk) / T * 1e6 for _ in range(a.reps)]
            print("%4d %9s %24s %12.3f" % (B, name, "%.2f (spread %.2f)" % (min(v), max(v) - min(v)),
                                           1e6 / RATE / min(v)), flush=True)


if __name__ == "__main__":
    main()
