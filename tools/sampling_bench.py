#!/usr/bin/env python3
"""Generation with sampling controls at BASELINE config 5's shape (bf16, 30 layers 3 x [1..512], 64 residual / 256 skip
channels, mu-law softmax, 16 kHz) and for the conditioned MoL-10 decoder: us per step of a one-shot `generate` and of a
pool stepped in chunks of 160, at B = 1, 32 and 2048, with the controls given (none: the calls without controls).

One process, one library: for A/B against another build of libsrwn.so start fresh alternating processes with
SRWN_LIB_PATH set (as tools/ab_step.py does for training) and compare the JSON lines; a library that predates the
*_sampled entry points is loaded without them (controls off only).
usage: python tools/sampling_bench.py [--temperature T] [--top-k K] [--top-p P] [--half] [--batches 1,32,2048] [--tag NAME]
  --half: only every second utterance / slot gets the controls (the others stay at the defaults)."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
CHUNK, POOL, LAT, MIX = 160, 125, 16, 10


def sync_time(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--half", action="store_true")
    ap.add_argument("--batches", default="1,32,2048")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    L = importlib.import_module("sr-wavenet_amd._lib")
    if os.environ.get("SRWN_LIB_PATH"):      # an older build for A/B: bind what it exports
        import ctypes
        probe = ctypes.CDLL(L.LIB_PATH)
        for n in [n for n in L.SIGNATURES if not hasattr(probe, n)]:
            del L.SIGNATURES[n]
    EG = importlib.import_module("sr-wavenet_amd.engine")
    on = (args.temperature, args.top_k, args.top_p) != (1.0, 0, 1.0)

    def controls(B, mol):
        if not on:
            return {}
        pick = lambda v, d: [v if (not args.half or u % 2 == 0) else d for u in range(B)]
        c = dict(temperature=pick(args.temperature, 1.0))
        if not mol:
            c.update(top_k=pick(args.top_k, 0), top_p=pick(args.top_p, 1.0))
        return c

    def run(head, eng, B, mol):
        T = 800 if B <= 32 else 320
        frames = T // POOL + 1
        cond = torch.randn((B, frames, LAT), device="cuda") if mol else None
        ctl = controls(B, mol)
        one = lambda: eng.generate(T, mode="sample", seed=1, batch=B, cond=cond, **ctl)
        one()
        t1 = min(sync_time(one) for _ in range(3))
        nch = 5 if B <= 32 else 2
        pframes = (nch * CHUNK) // POOL + 1
        pool = eng.generation_pool(B, pframes if mol else None)
        pcond = list(torch.randn((B, pframes, LAT), device="cuda")) if mol else None
        pool.join(list(range(B)), cond=pcond, **ctl)

        def steps():
            for _ in range(nch):
                pool.step(CHUNK, mode="sample")
        ts = []
        for r in range(4):                                  # (the first round warms up)
            pool.clock = 0
            pool._t[:] = 0
            pool._upload()
            t = sync_time(steps)
            if r:
                ts.append(t)
        for kind, us in (("oneshot", t1 / T * 1e6), ("pool160", min(ts) / (nch * CHUNK) * 1e6)):
            print(json.dumps(dict(tag=args.tag, head=head, B=B, kind=kind, us_per_step=round(us, 3),
                                  temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, half=args.half)),
                  flush=True)

    batches = [int(b) for b in args.batches.split(",")]
    cfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, output_channels=256, shift_input=True,
                         dtype=torch.bfloat16)
    eng = EG.WaveNetEngine(cfg, 1, 64, "cuda")
    for B in batches:
        run("softmax", eng, B, False)
    if (args.top_k, args.top_p) == (0, 1.0):                # (a mixture head takes the temperature only)
        cfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, output_channels=4 * MIX,
                             cond_channels=LAT, pool_stride=POOL, shift_input=True, head_mode="mol", dtype=torch.bfloat16)
        eng = EG.WaveNetEngine(cfg, 1, POOL, "cuda")
        for B in batches:
            run("mol%d" % MIX, eng, B, True)


if __name__ == "__main__":
    main()
