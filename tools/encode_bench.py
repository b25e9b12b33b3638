#!/usr/bin/env python3
"""The standalone streaming encoder on one MI355X: encoder.FrameEncoder in bf16 at tools/ae_bench.py --config scale's
encoder (30 layers, 128 channels, 256 skip channels, 16 latent channels).

  (a) one-shot   encode 8 x 16000 (pool 125, launches of 32 frames) against EncoderStack.forward at the same shape and
                 weights
  (b) one frame  push of exactly one frame in the steady state at B = 1, 8, 32 for pool 128 and 512: ms per push and
                 x real time at 16 kHz, the one-launch chain (srwn_nc_encode_frames, the bf16 default) against the
                 layer-by-layer twin (SRWN_ENC_FUSED=0).  The chain is the default only while it beats the twin by more
                 than the spread at B = 1, pool 512: the last line printed says whether it does
  (c) start() to the first frame
  (d) device bytes of the encoder's buffers and of its weights

Every comparison alternates its sides in one process, best of --reps each with the spread of each; every timed region is
device-synchronised and holds >= --seconds of work after a warm-up.
usage: python tools/encode_bench.py [--seconds 0.3] [--reps 3] [--quick]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EN = importlib.import_module("sr-wavenet_amd.encoder")

L, EC, S, LAT, RATE = 30, 128, 256, 16, 16000


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


def frame_encoder(w, P, B, max_frames, fused):
    os.environ["SRWN_ENC_FUSED"] = "1" if fused else "0"
    fe = EN.FrameEncoder(w, P, max_batch=B, max_frames=max_frames)
    assert fe.fused == fused
    return fe


def best(v):
    return "best %.3f ms (spread %.3f)" % (min(v), max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="B = 1 and 8 only")
    a = ap.parse_args()
    dt = torch.bfloat16
    rng = np.random.default_rng(0)
    w = EN.EncoderWeights(L, EC, S, LAT, 2, dt)
    wbytes = sum(t.numel() * t.element_size() for t in (w.params, w.packed, w.packer.idx, w.bs_sum))

    # ---- (a) one-shot against the training encoder's forward pass
    B, T, P = 8, 16000, 125
    es = EN.EncoderStack(L, B, T, P, EC, S, LAT, 2, dt)
    es.params.copy_(w.params); es.repack()
    x = torch.tensor(rng.uniform(-1, 1, (B, T)), dtype=torch.float32, device="cuda")
    es.x.copy_(x)
    fused, twin = frame_encoder(w, P, B, 32, True), frame_encoder(w, P, B, 32, False)
    ref = es.forward().view(B, T // P, LAT).clone()
    for name, fe in (("fused", fused), ("twin", twin)):
        got = fe.encode(x)
        print("(a) %s vs EncoderStack.forward: max |diff| %.3e of max |enc| %.3e" % (name, (got - ref).abs().max().item(),
                                                                                ref.abs().max().item()))
    t_es, t_f, t_t = [], [], []
    for _ in range(a.reps):
        t_es.append(timed(es.forward, a.seconds))
        t_f.append(timed(lambda: fused.encode(x), a.seconds))
        t_t.append(timed(lambda: twin.encode(x), a.seconds))
    print("(a) one-shot %d x %d, pool %d: EncoderStack.forward %s | FrameEncoder fused %s | twin %s" %
          (B, T, P, best(t_es), best(t_f), best(t_t)))
    es_bytes = sum(t.numel() * t.element_size() for t in vars(es).values() if isinstance(t, torch.Tensor))
    print("(d) device bytes at that shape: EncoderStack %.1f MB | FrameEncoder(max_batch 8, max_frames 32) fused %.2f MB, "
          "twin %.1f MB | weights %.2f MB" % (es_bytes / 1e6, fused.device_bytes() / 1e6, twin.device_bytes() / 1e6, wbytes / 1e6))
    del es, fused, twin
    torch.cuda.empty_cache()

    # ---- (b) one frame per push, (c) start to the first frame
    rule = None
    print("%4s %5s %22s %22s %10s %10s" % ("P", "B", "fused ms/push", "twin ms/push", "x realtime", "twin/fused"))
    for P in (128, 512):
        for B in ((1, 8) if a.quick else (1, 8, 32)):
            pair = {}
            for fu in (True, False):
                fe = frame_encoder(w, P, B, 32, fu)
                head = torch.tensor(rng.uniform(-1, 1, (B, P + L + 1)), dtype=torch.float32, device="cuda")
                chunk = torch.tensor(rng.uniform(-1, 1, (B, P)), dtype=torch.float32, device="cuda")
                fe.push(fe.start(B), head)                   # first use of the kernels
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = fe.start(B)
                out = fe.push(st, head)
                torch.cuda.synchronize()
                first = (time.perf_counter() - t0) * 1e3
                assert out.shape == (B, 1, LAT)

                def step(fe=fe, st=st, chunk=chunk):
                    assert fe.push(st, chunk).shape[1] == 1
                pair[fu] = (step, first, fe)
            tf, tt = [], []
            for _ in range(a.reps):
                tf.append(timed(pair[True][0], a.seconds))
                tt.append(timed(pair[False][0], a.seconds))
            print("%4d %5d %22s %22s %10.1f %10.2f" % (P, B, "%.3f (spread %.3f)" % (min(tf), max(tf) - min(tf)),
                                                     "%.3f (spread %.3f)" % (min(tt), max(tt) - min(tt)),
                                                     (P / RATE * 1e3) / min(tf), min(tt) / min(tf)))
            print("     (c) start() to the first frame: fused %.3f ms, twin %.3f ms; (d) buffers at max_frames 32: fused %.2f MB, "
                  "twin %.1f MB" % (pair[True][1], pair[False][1], pair[True][2].device_bytes() / 1e6,
                                    pair[False][2].device_bytes() / 1e6))
            if (P, B) == (512, 1):
                rule = (min(tf), min(tt), max(max(tf) - min(tf), max(tt) - min(tt)))
            del pair
            torch.cuda.empty_cache()
    fe = frame_encoder(w, 512, 2, 32, True)
    print("(d) FrameEncoder(pool 512, max_batch 2, max_frames 32): fused %d bytes; twin %d bytes; weights %d bytes" %
          (fe.device_bytes(), frame_encoder(w, 512, 2, 32, False).device_bytes(), wbytes))
    f, t, spread = rule
    print("default rule (B = 1, pool 512): fused %.3f ms, twin %.3f ms, spread %.3f -> the chain %s the bf16 default; "
          "encoder.ENC_FUSED_DEFAULT is %r" % (f, t, spread, "earns" if t - f > spread else "does NOT earn",
                                               EN.ENC_FUSED_DEFAULT))


if __name__ == "__main__":
    main()
