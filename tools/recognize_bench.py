#!/usr/bin/env python3
"""The streaming classifier on one MI355X: recognizer.StreamClassifier in bf16 at the reference's classifier shape
(train.py --classifier: 2 x [1..512] dilations, 32 residual and 128 skip channels, 16000 samples, 12 classes), hop 160,
window 16000.

  (a) one hop    push of exactly one hop in the steady state (every push emits) at B = 1, 8, 32: ms per push and x real
                 time at 16 kHz, the one-launch head (srwn_pooled_stream_head) against its parity twin
                 (SRWN_RECOG_FUSED=0); beside it the only alternative without this module: one WaveNet.predict of the
                 last 16000 samples per hop, on the same box
  (b) launches per step and device bytes by buffer family
  (c) old path  with --parent-lib: FlowSynthesizer.step of this build against another build of the library (the parent
                 commit's), B = 8, n = 160 and 1600, alternating fresh processes (tools/synth_pool_bench.py's
                 measurement): srwn_group.hip gained an instantiation

Every comparison alternates its sides in one process, best of --reps each with the spread of each; every timed region is
device-synchronised and holds >= --seconds of work after a warm-up.
usage: python tools/recognize_bench.py [--seconds 0.3] [--reps 3] [--quick] [--parent-lib ab/libsrwn_parent.so]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 2
R, S, CLASSES, WINDOW, HOP, RATE = 32, 128, 12, 16000, 160, 16000


def fmt(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="B = 1 and 8 only")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for (c)")
    a = ap.parse_args()
    from synth_pool_bench import timed
    RC = importlib.import_module("sr-wavenet_amd.recognizer")
    M = importlib.import_module("sr-wavenet_amd.model")
    dt = torch.bfloat16
    rng = np.random.default_rng(0)
    model = M.WaveNet(WINDOW, CLASSES, DIL, dilation_channels=R, skip_channels=S, output_channels=CLASSES, dtype=dt)
    model._engine(1, WINDOW)
    w = RC.ClassifierWeights.from_engine(model._primary)
    print("%5s %24s %24s %10s %24s %14s" % ("B", "fused ms/push", "twin ms/push", "x realtime", "predict per hop ms", "predict/fused"))
    for B in ((1, 8) if a.quick else (1, 8, 32)):
        side = {}
        for fused in (True, False):
            os.environ["SRWN_RECOG_FUSED"] = "1" if fused else "0"
            c = RC.StreamClassifier(w, max_batch=B, hop=HOP, window=WINDOW, max_hops=8)
            assert c.fused == fused
            st = c.start(B)
            warm = torch.tensor(rng.uniform(-1, 1, (B, WINDOW)), dtype=torch.float32, device="cuda")
            assert c.push(st, warm).shape[1] == 1          # the first full window: from here on every hop emits
            chunk = torch.tensor(rng.uniform(-1, 1, (B, HOP)), dtype=torch.float32, device="cuda")

            def step(c=c, st=st, chunk=chunk):
                assert c.push(st, chunk).shape[1] == 1
            side[fused] = (step, c)
        eng = model._engine(B, WINDOW)
        clip = torch.tensor(rng.uniform(-1, 1, (B, WINDOW)), dtype=torch.float32, device="cuda")

        def predict(eng=eng, clip=clip):      # WaveNet.predict without its host round trip
            eng.set_inputs(clip)
            eng.forward(with_loss=False)
            return eng.probs.clone()
        tf, tt, tp = [], [], []
        for _ in range(a.reps):
            tf.append(timed(side[True][0], a.seconds))
            tt.append(timed(side[False][0], a.seconds))
            tp.append(timed(predict, a.seconds))
        print("%5d %24s %24s %10.1f %24s %14.1f" % (B, fmt(tf), fmt(tt), (HOP / RATE * 1e3) / min(tf), fmt(tp), min(tp) / min(tf)))
        for fused in (True, False):
            c = side[fused][1]
            print("      (b) %s: %d launches per step; bytes %s" % ("fused" if fused else "twin", c.launches_per_step,
                                                                 json.dumps(c.buffer_bytes())))
        del side
        torch.cuda.empty_cache()
    if a.parent_lib:
        print("== (c) the path that was there before, against the parent commit's library")
        import synth_pool_bench
        a.seconds = max(a.seconds, 0.5)
        synth_pool_bench.old_path(a)



if __name__ == "__main__":
    main()
