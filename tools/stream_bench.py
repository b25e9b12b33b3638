#!/usr/bin/env python3
"""Cost of streaming (resumable) generation at BASELINE config 5's shape (bf16, 30 layers 3 x [1..512], 64 residual / 256
skip channels, mu-law softmax) and for the conditioned MoL-10 decoder, B = 1 and 32, 16 kHz:
  * us per sample and real-time factor of 16 000 samples made in chunks of 1, 16, 160 and 1 600 (generate_chunk), next to
    one-shot generate() of the same 16 000 -- the difference is the cost of each resume (one launch per chunk);
  * time to the first chunk (160 samples) after a 16 000-sample prompt: the parallel prime (one forward pass of the stack +
    srwn_generate_ring_fill) and a stepped prime (the prompt as one teacher-forced chunk).
Timings are best of 3 after a warm-up run of the same call (the prime's forward-only view is allocated there)."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

EG = importlib.import_module("sr-wavenet_amd.engine")
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
N, SR, FIRST = 16000, 16000, 160
POOL, LAT, MIX = 125, 16, 10


def best(fn, reps=3):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def run(name, eng, B, cond_fn):
    cond = cond_fn(B, 2 * N)
    t = best(lambda: eng.generate(N, mode="sample", seed=1, batch=B, cond=None if cond is None else cond[:, :N // POOL]))
    print("%s B=%2d  one-shot generate  %.1f us/sample  RTF %.3f" % (name, B, t / N * 1e6, t / N * SR), flush=True)
    for chunk in (1, 16, 160, 1600):
        def chunks():
            st = eng.generation_state(B, cond, 1)
            for _ in range(N // chunk):
                eng.generate_chunk(st, chunk, mode="sample")
        tc = best(chunks, reps=1 if chunk == 1 else 3)
        print("%s B=%2d  chunks of %4d      %.1f us/sample  RTF %.3f  (%+.1f us per resume)"
              % (name, B, chunk, tc / N * 1e6, tc / N * SR, (tc - t) / (N // chunk) * 1e6), flush=True)
    prompt = torch.rand((B, N), device="cuda") * 0.2 - 0.1

    def parallel():
        st = eng.generation_state(B, cond, 1)
        eng.prime(st, prompt)
        eng.generate_chunk(st, FIRST, mode="sample")

    def stepped():
        st = eng.generation_state(B, cond, 1)
        eng.generate_chunk(st, N, mode="sample", forced=prompt)
        eng.generate_chunk(st, FIRST, mode="sample")
    tp, ts = best(parallel), best(stepped, reps=1)
    print("%s B=%2d  first %d samples after a %d-sample prompt: parallel prime %.2f ms, stepped prime %.1f ms"
          % (name, B, FIRST, N, tp * 1e3, ts * 1e3), flush=True)


def main():
    cfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, output_channels=256, shift_input=True,
                         dtype=torch.bfloat16)
    eng = EG.WaveNetEngine(cfg, 1, 64, "cuda")
    for B in (1, 32):
        run("config 5 softmax", eng, B, lambda b, n: None)
    cfg = EG.StackConfig(dilations=DIL, dilation_channels=64, skip_channels=256, output_channels=4 * MIX,
                         cond_channels=LAT, pool_stride=POOL, shift_input=True, head_mode="mol", dtype=torch.bfloat16)
    eng = EG.WaveNetEngine(cfg, 1, POOL, "cuda")
    for B in (1, 32):
        run("MoL-%d conditioned" % MIX, eng, B, lambda b, n: torch.randn((b, n // POOL, LAT), device="cuda"))


if __name__ == "__main__":
    main()
