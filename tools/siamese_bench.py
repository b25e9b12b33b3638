#!/usr/bin/env python3
"""SiameseWaveNet training step (engine head_mode "contrastive", both towers as one batch of 2P clips) on one MI355X,
graph-replayed, at two shapes:

  small  siamese.py's: 1 pair x 5120 samples, 30 layers, 32/128 channels, D = 2
  wide   8 pairs x 16000 samples, 30 layers, 64/256 channels, D = 2

Prints one JSON line per shape: ms per step and clip samples per second (2P*T per step).  --profile re-runs each shape
in a child under `rocprofv3 --kernel-trace --stats` and adds the summed kernel time per step (its ratio to the wall
time says how much of the step the GPU is busy) and the shares of the head's launches: time_sum_kernel (first half of
srwn_time_mean; its slab reduction is a srwn_reduce_partials launch like the others), contrastive_head_kernel and
bcast_mask_kernel.  Not the driver's bench (that is bench.py)."""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"small": dict(pairs=1, length=5120, R=32, S=128), "wide": dict(pairs=8, length=16000, R=64, S=256)}
HEAD_KERNELS = ("time_sum_kernel", "contrastive_head_kernel", "bcast_mask_kernel")


def run(shape, steps, warmup, dtype):
    import numpy as np
    import torch
    EG = importlib.import_module("sr-wavenet_amd.engine")
    SA = importlib.import_module("sr-wavenet_amd.simple_audio")
    sh = SHAPES[shape]
    P, T = sh["pairs"], sh["length"]
    cfg = EG.StackConfig(dilations=[1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3, dilation_channels=sh["R"],
                         skip_channels=sh["S"], output_channels=2, head_mode="contrastive", margin=5.0,
                         dtype=torch.bfloat16 if dtype == "bf16" else torch.float32, learning_rate=1e-4)
    eng = EG.WaveNetEngine(cfg, 2 * P, T, "cuda")
    rng = np.random.RandomState(0)
    waves = [SA.generate_random_wave(T, rng=rng) for _ in range(2 * P)]
    x = torch.tensor(np.array([w for w, _ in waves]), dtype=torch.float32, device="cuda")
    y = torch.tensor([float((waves[p][1] == waves[P + p][1]).all()) for p in range(P)], device="cuda")
    eng.set_inputs(x, y)
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
    return dict(shape=shape, pairs=P, length=T, R=sh["R"], S=sh["S"], D=2, dtype=dtype, steps=steps,
                ms_per_step=round(ms, 4), clip_samples_per_s=round(2 * P * T / (ms * 1e-3), 1),
                loss=float(eng.loss.item()))


def profile(shape, steps, warmup, dtype):
    """One rocprofv3 --kernel-trace --stats run of this script on one shape; kernel time per step and head shares."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return {"profile_error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="siamese_prof_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--shape", shape, "--steps", str(steps), "--warmup",
               str(warmup), "--dtype", dtype]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"profile_error": "rocprofv3 exit %d: %s" % (r.returncode, r.stderr[-500:])}
        stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            return {"profile_error": "no kernel_stats.csv under the rocprofv3 output"}
        rows = list(csv.DictReader(open(stats[0])))
        total = sum(float(row["TotalDurationNs"]) for row in rows)
        # every step runs the same launches: warm-up eager steps, warm-up replays and timed replays alike
        nsteps = max(2, warmup) + warmup + steps
        shares = {}
        for k in HEAD_KERNELS:
            ns = sum(float(row["TotalDurationNs"]) for row in rows if k in row["Name"])
            shares[k] = dict(pct=round(100 * ns / total, 3), us_per_step=round(ns / 1e3 / nsteps, 2))
        return dict(kernel_ms_per_step=round(total / 1e6 / nsteps, 4), kernels_per_step=round(
            sum(int(row["Calls"]) for row in rows) / nsteps, 1), head_pct=round(sum(v["pct"] for v in shares.values()), 3),
            head=shares)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["small", "wide", "both"], default="both")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--profile", action="store_true", help="add one rocprofv3 --kernel-trace --stats run per shape")
    a = ap.parse_args()
    for shape in (["small", "wide"] if a.shape == "both" else [a.shape]):
        res = run(shape, a.steps, a.warmup, a.dtype)
        if a.profile:
            res.update(profile(shape, a.steps, a.warmup, a.dtype))
            if "kernel_ms_per_step" in res:
                res["gpu_busy_pct"] = round(100 * res["kernel_ms_per_step"] / res["ms_per_step"], 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
