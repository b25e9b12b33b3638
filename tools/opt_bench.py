#!/usr/bin/env python
"""Times the optimizer's update launch alone, at the parameter counts of bench.py's teacher (BASELINE config 2) and of
examples/teacher.py's auto-encoder (decoder and encoder buffers).

Legs:
  adam          srwn_adam_step                                     (what a step without controls runs)
  ctl           srwn_adam_step_ctl, no EMA, no clip                (schedule only: should equal `adam`)
  ctl+ema       srwn_adam_step_ctl with the shadow                 (seven streams of 4n bytes become nine)
  adam;ema3     srwn_adam_step, then the EMA as three torch ops    (the separate-launch alternative)
  adam;lerp     srwn_adam_step, then torch.lerp_                   (the same alternative as one launch: three more streams)
  clip+ctl+ema  srwn_sumsq, srwn_clip_scale, then ctl+ema          (everything on)

Each leg: device events around a region of --launches launches (default 200), --regions regions (default 3); the best
region and all of them (the spread) are printed as microseconds per launch, and one JSON line at the end.  --cold times
every launch with events of its own behind a fill of a buffer larger than the 256 MiB Infinity Cache, so that the
parameter buffers come from HBM as they do inside a training step.

    python tools/opt_bench.py [--launches 200] [--regions 3] [--cold]
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def param_counts():
    """name -> parameter count, read from engines built at a token (batch, length)."""
    EG = importlib.import_module("sr-wavenet_amd.engine")
    EN = importlib.import_module("sr-wavenet_amd.encoder")
    dil = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
    teacher = EG.WaveNetEngine(EG.StackConfig(dilations=dil, dilation_channels=64, skip_channels=256, output_channels=256,
                                              shift_input=True), 1, 1024)
    ae = EN.AutoEncoderEngine(EG.StackConfig(dilations=dil, dilation_channels=32, skip_channels=128, output_channels=20,
                                             cond_channels=16, pool_stride=512, shift_input=True, head_mode="mol"),
                              1, 1024, 128, 16, 0)
    return {"teacher (config 2)": teacher.nparams, "auto-encoder decoder": ae.dec.nparams, "auto-encoder encoder": ae.enc.nparams}


def legs(K, n, dev):
    z = lambda: torch.zeros(n, dtype=torch.float32, device=dev)
    theta, g, m, v, ema = torch.randn(n, device=dev), torch.randn(n, device=dev) * 1e-2, z(), z(), torch.randn(n, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    ctl = torch.tensor([[1e-4, 0.999]] * 8, dtype=torch.float32, device=dev)
    ctl_len = torch.full((1,), 8, dtype=torch.int32, device=dev)
    parts = torch.zeros(K.sumsq_partials(n), dtype=torch.float32, device=dev)
    clip = torch.zeros(2, dtype=torch.float32, device=dev)
    one_minus = torch.tensor(1.0 - 0.999, dtype=torch.float32, device=dev)

    def adam():
        K.adam_step(theta, g, m, v, step, 1e-4)

    def ema3():
        diff = ema - theta
        diff.mul_(one_minus)
        ema.sub_(diff)

    def clip_ctl_ema():
        K.sumsq(g, parts)
        K.clip_scale(parts, 1.0, 1.0, clip)
        K.adam_step_ctl(theta, g, m, v, step, ctl, ctl_len, ema=ema, scale_dev=clip)

    return [("adam", adam),
            ("ctl", lambda: K.adam_step_ctl(theta, g, m, v, step, ctl, ctl_len)),
            ("ctl+ema", lambda: K.adam_step_ctl(theta, g, m, v, step, ctl, ctl_len, ema=ema)),
            ("adam;ema3", lambda: (adam(), ema3())),
            ("adam;lerp", lambda: (adam(), ema.lerp_(theta, one_minus))),
            ("clip+ctl+ema", clip_ctl_ema)]


def time_region(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def time_cold(fn, launches, flush):
    total = 0.0
    for _ in range(launches):
        flush.add_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b) * 1e3
    return total / launches


def fit_times(steps, regions):
    """--fit: milliseconds per ``fit`` step of bench.py's teacher (B = 8, T = 16000, bf16) with no controls, with a
    schedule and clipping, and with the EMA too; then per validation sweep of examples/classifier.py's network with and
    without validate_ema (host clock around calls that end in a host wait; graphs captured before the timed calls)."""
    import time
    import numpy as np
    M = importlib.import_module("sr-wavenet_amd.model")
    D = importlib.import_module("sr-wavenet_amd.dataset")
    O = importlib.import_module("sr-wavenet_amd.optim")
    rng = np.random.default_rng(0)
    dil = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
    out = {}

    def timed(call):
        ts = []
        for _ in range(regions):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    clips = D.DeviceDataset((0.5 * rng.standard_normal((64, 16000))).astype(np.float32).clip(-1, 1))
    for name, kw in (("no controls", None), ("schedule+clip", dict(clip_norm=1.0)),
                     ("schedule+clip+ema", dict(clip_norm=1.0, ema_decay=0.999))):
        m = M.WaveNetTeacher(16000, 0, dil * 3, dilation_channels=64, skip_channels=256, dtype=torch.bfloat16)
        if kw is not None:
            m.set_training_controls(schedule=O.cosine(1e-3, 10 * steps), horizon=10 * steps, **kw)
        s = clips.sampler(8, 16000, seed=0)
        m.fit(s, 5)
        ts = [t / steps for t in timed(lambda: m.fit(s, steps))]
        out["fit step: " + name] = ts
        print("  fit step, %-18s best %8.3f ms   regions %s" % (name, min(ts), " ".join("%.3f" % t for t in ts)))
        del m
    labels = np.arange(64) % 4
    held = D.DeviceDataset((0.5 * rng.standard_normal((64, 16384))).astype(np.float32).clip(-1, 1), labels, 4)
    for name, vema in (("validation sweep", False), ("validation sweep, validate_ema", True)):
        m = M.WaveNet(16384, 4, (dil * 2)[:20], dilation_channels=32, skip_channels=128, output_channels=4,
                      dtype=torch.bfloat16)
        m.set_training_controls(schedule=1e-3, ema_decay=0.999, validate_ema=vema)
        s = held.sampler(1, 16384, seed=0)
        ev = held.eval_sampler(8, 16384, sweep_capacity=16)
        m.fit(s, 4, validate=(ev, 1))
        with_sweeps = timed(lambda: m.fit(s, 16, validate=(ev, 1)))
        without = timed(lambda: m.fit(s, 16))
        ts = [(a - min(without)) / 16 for a in with_sweeps]
        out[name] = ts
        print("  %-32s best %8.3f ms per sweep of 8 steps   regions %s" % (name, min(ts), " ".join("%.3f" % t for t in ts)))
        del m
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--cold", action="store_true", help="per-launch events behind a cache-sized fill")
    ap.add_argument("--fit", type=int, default=0, metavar="STEPS",
                    help="instead: time STEPS fit steps of bench.py's teacher per region, and validation sweeps")
    a = ap.parse_args(argv)
    if a.launches < 200:
        ap.error("--launches: at least 200 per region")
    if not torch.cuda.is_available():
        sys.exit("opt_bench: no GPU (there is no CPU timing of a device launch)")
    if a.fit:
        out = {"fit_steps": a.fit, "regions": a.regions, "ms": fit_times(a.fit, a.regions)}
        print(json.dumps(out))
        return out
    K = importlib.import_module("sr-wavenet_amd.kernels")
    dev = torch.device("cuda")
    flush = torch.zeros(96 << 20, dtype=torch.float32, device=dev) if a.cold else None      # 384 MiB
    out = {"launches": a.launches, "regions": a.regions, "cold": bool(a.cold), "us_per_launch": {}}
    for name, n in param_counts().items():
        print("%s: n = %d (%.1f MB per stream)" % (name, n, 4e-6 * n))
        res = {}
        for leg, fn in legs(K, n, dev):
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            ts = [time_cold(fn, a.launches, flush) if a.cold else time_region(fn, a.launches) for _ in range(a.regions)]
            res[leg] = ts
            print("  %-13s best %8.2f us   regions %s" % (leg, min(ts), " ".join("%.2f" % t for t in ts)))
        base = min(res["adam"])
        print("  ctl+ema / adam = %.3f (9/7 = 1.286);  adam;lerp / adam = %.3f;  ctl / adam = %.3f"
              % (min(res["ctl+ema"]) / base, min(res["adam;lerp"]) / base, min(res["ctl"]) / base))
        out["us_per_launch"][name] = {"n": n, **res}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
