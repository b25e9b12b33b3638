#!/usr/bin/env python3
"""The streaming likelihood scorer on one MI355X: scorer.StreamScorer in bf16 at the benchmark teacher's shape (3 x [1..512]
dilations, 64 residual and 256 skip channels, 256 mu-law classes).

  (a) push      ms per push of 160 and of 1600 samples in the steady state at B = 1, 8, 32, and x real time at 16 kHz: the
                one-launch head (srwn_stream_score_head) against its parity twin (SRWN_SCORE_FUSED=0)
  (b) score     whole recordings of 8 x 16000 through StreamScorer.score against WaveNetTeacher.loss at the same shape (the
                forward pass of the training engine, the only way to the same number without this module)
  (c) launches per step and device bytes by buffer family on both paths; the training engine's bytes beside them
  (d) old path  with --parent-lib: StreamClassifier.push at B = 8 of this build against another build of the library (the
                parent commit's), alternating fresh processes

Every comparison alternates its sides in one process, best of --reps each with the spread of each; every timed region is
device-synchronised and holds >= --seconds of work after a warm-up.
usage: python tools/score_bench.py [--seconds 0.3] [--reps 3] [--quick] [--parent-lib ab/libsrwn_parent.so]"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
R, S, CLASSES, RATE, CLIP = 64, 256, 256, 16000, 16000


def fmt(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def old_path_child(a):
    """StreamClassifier.push of one hop of 160 at B = 8 in the steady state, on whatever library SRWN_LIB_PATH names."""
    import torch
    from synth_pool_bench import modules, timed
    modules()
    RC = importlib.import_module("sr-wavenet_amd.recognizer")
    dil = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 2
    w = RC.ClassifierWeights(dil, 32, 128, 12, 2, torch.bfloat16)
    w.params.copy_(torch.tensor(np.random.default_rng(0).normal(0, 0.05, w.nparams), dtype=torch.float32))
    w.repack()
    c = RC.StreamClassifier(w, max_batch=8, hop=160, window=16000, max_hops=8)
    st = c.start(8)
    rng = np.random.default_rng(1)
    c.push(st, torch.tensor(rng.uniform(-1, 1, (8, 16000)), dtype=torch.float32, device="cuda"))
    chunk = torch.tensor(rng.uniform(-1, 1, (8, 160)), dtype=torch.float32, device="cuda")
    print("ABRESULT " + json.dumps([timed(lambda: c.push(st, chunk), a.seconds) for _ in range(a.reps)]))


def old_path(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so")), ("parent", os.path.join(ROOT, a.parent_lib))]
    print("== (d) StreamClassifier.push, B = 8, one hop of 160: this build against %s, alternating fresh processes" % a.parent_lib)
    got = {k: [] for k, _ in libs}
    for r in range(a.rounds):
        for name, path in libs:
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "old-path-child", "--seconds",
                                 str(max(a.seconds, 0.5)), "--reps", str(a.reps)], env=dict(os.environ, SRWN_LIB_PATH=path),
                                cwd=ROOT, capture_output=True, text=True, timeout=300)
            line = [l for l in pr.stdout.splitlines() if l.startswith("ABRESULT ")]
            if pr.returncode or not line:
                print("FAILED", name, pr.stderr[-2000:], flush=True)
                return
            d = json.loads(line[0][9:])
            got[name] += d
            print("round %d %-6s %s" % (r, name, " ".join("%.4f" % m for m in d)), flush=True)
    t, p = got["this"], got["parent"]
    print("this build best %.4f ms (spread %.4f), parent best %.4f ms (spread %.4f): difference %+.4f ms"
          % (min(t), max(t) - min(t), min(p), max(p) - min(p), min(t) - min(p)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="B = 1 and 8 only")
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for (d)")
    ap.add_argument("--only", default=None, choices=["old-path", "old-path-child"])
    a = ap.parse_args()
    if a.only == "old-path-child":
        return old_path_child(a)
    if a.only == "old-path":
        if not a.parent_lib:
            sys.exit("--only old-path needs --parent-lib")
        return old_path(a)
    import torch
    from synth_pool_bench import timed
    SC = importlib.import_module("sr-wavenet_amd.scorer")
    M = importlib.import_module("sr-wavenet_amd.model")
    dt = torch.bfloat16
    rng = np.random.default_rng(0)
    model = M.WaveNetTeacher(CLIP, 0, DIL, dilation_channels=R, skip_channels=S, quantization_channels=CLASSES, dtype=dt)
    model._engine(1, 1024)
    w = SC.ScorerWeights.from_engine(model._primary)
    nb = lambda ts: int(sum(t.numel() * t.element_size() for t in ts))
    print("== (a) ms per push, best of %d (spread)" % a.reps)
    print("%5s %6s %24s %24s %12s" % ("B", "n", "fused ms/push", "twin ms/push", "x realtime"))
    for B in ((1, 8) if a.quick else (1, 8, 32)):
        side = {}
        for fused in (True, False):
            os.environ["SRWN_SCORE_FUSED"] = "1" if fused else "0"
            s = SC.StreamScorer(w, max_batch=B, max_chunk=1600)
            assert s.fused == fused
            side[fused] = s
        for n in (160, 1600):
            chunk = torch.tensor(rng.uniform(-1, 1, (B, n)), dtype=torch.float32, device="cuda")
            steps = {}
            for fused, s in side.items():
                st = s.start(B)
                s.push(st, torch.tensor(rng.uniform(-1, 1, (B, 3200)), dtype=torch.float32, device="cuda"))
                steps[fused] = (lambda s=s, st=st: s.push(st, chunk))
            tf, tt = [], []
            for _ in range(a.reps):
                tf.append(timed(steps[True], a.seconds))
                tt.append(timed(steps[False], a.seconds))
            print("%5d %6d %24s %24s %12.1f" % (B, n, fmt(tf), fmt(tt), (n / RATE * 1e3) / min(tf)))
        for fused in (True, False):
            s = side[fused]
            print("      (c) %s: %d launches per step; bytes %s" % ("fused" if fused else "twin", s.launches_per_step,
                                                                 json.dumps(s.buffer_bytes())))
        if B == 8:
            print("== (b) whole recordings of %d x %d, best of %d (spread)" % (B, CLIP, a.reps))
            clip = torch.tensor(rng.uniform(-1, 1, (B, CLIP)), dtype=torch.float32, device="cuda")
            clip_np = clip.cpu().numpy()
            eng = model._engine(B, CLIP)

            def loss(eng=eng, clip=clip):      # WaveNetTeacher.loss without its host round trip
                eng.set_inputs(clip, SC.K.mu_law_encode(clip, CLASSES), None)
                eng.forward()
                return eng.loss
            ts, tw, tl = [], [], []
            for _ in range(a.reps):
                ts.append(timed(lambda: side[True].score(clip), a.seconds))
                tw.append(timed(lambda: side[False].score(clip), a.seconds))
                tl.append(timed(loss, a.seconds))
            got = float(side[True].score(clip).double().mean())
            print("score fused %s ms, twin %s ms, WaveNetTeacher.loss %s ms; mean nll %.5f, loss %.5f"
                  % (fmt(ts), fmt(tw), fmt(tl), got, float(model.loss(clip_np))))
            tens = [v for v in vars(eng).values() if isinstance(v, torch.Tensor) and v.is_cuda]
            print("      (c) training engine at %d x %d: %d bytes in %d device tensors (lists of tensors not counted)"
                  % (B, CLIP, nb(tens), len(tens)))
            del eng, tens
            model._engines.pop((B, CLIP), None)
        del side
        torch.cuda.empty_cache()
    if a.parent_lib:
        old_path(a)


if __name__ == "__main__":
    main()
