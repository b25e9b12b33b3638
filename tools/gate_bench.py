#!/usr/bin/env python3
"""Training step of the canonical WaveNet gate (StackConfig gate_mode "wavenet") against its reference-gate twin.

Shape: BASELINE config 2 -- 30 layers 3 x [1..512], 64 residual / 256 skip channels, 256-way mu-law softmax, batch
8 x 16000 samples, bf16, graph-replayed.  Two legs, each in a fresh child process, alternated --rounds times on the same
box:

  wavenet     gate_mode "wavenet" (one launch per layer, csrc/srwn_wngate.hip: it has no multi-layer kernels)
  reference   gate_mode "reference" with SRWN_FUSE=0: the same one-launch-per-layer structure, the reference gate

Prints one JSON line per child run and a summary line: the median ms per step of each leg, and for the wavenet leg its
FLOP rate at the canonical unit's own count, 7 422 720 flop per sample forward + backward (the reference
gate's figure is a different one and is not mixed in here).  Not the driver's bench (that is bench.py)."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAVENET_FLOP_PER_SAMPLE = 7_422_720      # canonical gate, fwd + bwd, config 2
B, T = 8, 16000


def child(leg, steps, warmup):
    import numpy as np
    import torch
    EG = importlib.import_module("sr-wavenet_amd.engine")
    K = importlib.import_module("sr-wavenet_amd.kernels")
    from oracle import wavenet_np as O
    cfg = EG.StackConfig(dilations=[1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3, dilation_channels=64, skip_channels=256,
                         output_channels=256, shift_input=True, dtype=torch.bfloat16, learning_rate=1e-4,
                         gate_mode="wavenet" if leg == "wavenet" else "reference")
    eng = EG.WaveNetEngine(cfg, B, T, "cuda")
    audio = torch.tensor(O.synthetic_audio(B, T, seed=1), dtype=torch.float32, device="cuda")
    eng.set_inputs(audio, K.mu_law_encode(audio, 256))
    for _ in range(max(2, warmup)):
        eng.train_step()
    eng.capture_graphs()
    for _ in range(warmup):
        eng.train_step_graphed()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        eng.train_step_graphed()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    loss = float(eng.loss.item())
    if not np.isfinite(loss):
        raise RuntimeError("%s leg: loss %r" % (leg, loss))
    return dict(leg=leg, fuse=os.environ.get("SRWN_FUSE", "1"), steps=steps, ms_per_step=round(ms, 4), loss=loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two legs (fresh processes each)")
    ap.add_argument("--child", choices=["wavenet", "reference"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.steps, a.warmup)), flush=True)
        return
    res = {"wavenet": [], "reference": []}
    for _ in range(a.rounds):
        for leg in ("wavenet", "reference"):
            env = dict(os.environ)
            if leg == "reference":
                env["SRWN_FUSE"] = "0"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit("%s leg failed (exit %d):\n%s" % (leg, r.returncode, r.stderr[-2000:]))
            line = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(line), flush=True)
            res[leg].append(line["ms_per_step"])
    wn, ref = statistics.median(res["wavenet"]), statistics.median(res["reference"])
    print(json.dumps(dict(summary=True, batch=B, length=T, dtype="bf16", graphed=True, rounds=a.rounds,
                          wavenet_ms_per_step=wn, wavenet_ms_all=res["wavenet"],
                          reference_fuse0_ms_per_step=ref, reference_fuse0_ms_all=res["reference"],
                          wavenet_over_reference=round(wn / ref, 3),
                          wavenet_tflops=round(WAVENET_FLOP_PER_SAMPLE * B * T / (wn * 1e-3) / 1e12, 2))), flush=True)


if __name__ == "__main__":
    main()
