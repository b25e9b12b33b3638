#!/usr/bin/env python3
"""The streaming likelihood scorer of the conditioned mixture-of-logistics decoder on one MI355X: scorer.MolStreamScorer in
bf16 at BASELINE config 5's widths (3 x [1..512] dilations, 64 residual and 256 skip channels, 10 mixtures, 16 latent
channels, pool 125; tools/live_decode_bench.py's decoder).

  (a) push      ms per push of 160 and of 1600 samples in the steady state at B = 1, 8, 32 (every frame the push needs fed
                before the timed region's pushes: a feed of its own per push, timed with it), and x real time at 16 kHz:
                the one-launch head (srwn_stream_mol_score_head) against its parity twin (SRWN_SCORE_FUSED=0)
  (b) score     whole recordings of 8 x 16000 through AutoEncoderScorer.score (encoder included) and through
                score_with_encoding (the decoder alone) against the forward pass and loss of WaveNetAutoEncoder's decoder
                engine at the same shape (the only way to the same number without this module)
  (c) launches per step and device bytes by buffer family on both paths; the training engine's bytes beside them
  (d) old path  with --parent-lib: StreamScorer.push (the softmax scorer, whose head shares its device body with the new
                one) at B = 8, 160 samples, of this build against another build of the library (the parent commit's),
                alternating fresh processes

Every comparison alternates its sides in one process, best of --reps each with the spread of each; every timed region is
device-synchronised and holds >= --seconds of work after a warm-up.
usage: python tools/mol_score_bench.py [--seconds 0.3] [--reps 3] [--quick] [--parent-lib ab/libsrwn_parent.so]"""
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
R, S, MIX, LAT, POOL, RATE, CLIP = 64, 256, 10, 16, 125, 16000, 16000
MAX_FRAMES = 64           # a ring long enough for a push of 1600 samples behind a history of 1023


def fmt(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def old_path_child(a):
    """StreamScorer.push of 160 samples at B = 8 in the steady state, on whatever library SRWN_LIB_PATH names."""
    import torch
    from synth_pool_bench import modules, timed
    modules()
    SC = importlib.import_module("sr-wavenet_amd.scorer")
    w = SC.ScorerWeights(DIL, R, S, 256, 2, torch.bfloat16)
    w.params.copy_(torch.tensor(np.random.default_rng(0).normal(0, 0.05, w.nparams), dtype=torch.float32))
    w.repack()
    s = SC.StreamScorer(w, max_batch=8, max_chunk=1600)
    st = s.start(8)
    rng = np.random.default_rng(1)
    s.push(st, torch.tensor(rng.uniform(-1, 1, (8, 3200)), dtype=torch.float32, device="cuda"))
    chunk = torch.tensor(rng.uniform(-1, 1, (8, 160)), dtype=torch.float32, device="cuda")
    print("ABRESULT " + json.dumps([timed(lambda: s.push(st, chunk), a.seconds) for _ in range(a.reps)]))


def old_path(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so")), ("parent", os.path.join(ROOT, a.parent_lib))]
    print("== (d) StreamScorer.push, B = 8, 160 samples: this build against %s, alternating fresh processes" % a.parent_lib)
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
    model = M.WaveNetAutoEncoder(CLIP, 0, MIX, DIL, dilation_channels=R, skip_channels=S, latent_channels=LAT,
                                 pool_stride=POOL, dtype=dt)
    eng = model._engine(8, CLIP)
    w = SC.MolScorerWeights.from_engine(eng.dec)
    nb = lambda ts: int(sum(t.numel() * t.element_size() for t in ts))
    print("== (a) ms per feed + push, best of %d (spread)" % a.reps)
    print("%5s %6s %24s %24s %12s" % ("B", "n", "fused ms/push", "twin ms/push", "x realtime"))
    for B in ((1, 8) if a.quick else (1, 8, 32)):
        side = {}
        for fused in (True, False):
            os.environ["SRWN_SCORE_FUSED"] = "1" if fused else "0"
            s = SC.MolStreamScorer(w, max_batch=B, max_chunk=1600, max_frames=MAX_FRAMES)
            assert s.fused == fused
            side[fused] = s
        for n in (160, 1600):
            chunk = torch.tensor(rng.uniform(-1, 1, (B, n)), dtype=torch.float32, device="cuda")
            frames = torch.tensor(rng.normal(size=(B, MAX_FRAMES, LAT)), dtype=torch.float32, device="cuda")
            steps = {}
            for fused, s in side.items():
                st = s.start(B)

                def step(s=s, st=st):      # the frames the push needs (never more than the ring has room for), then the push
                    k = -(-(st.t + n - st.fed * POOL) // POOL)
                    if k > 0:
                        s.feed(st, frames[:, :k])
                    s.push(st, chunk)
                for _ in range(3200 // n):
                    step()
                steps[fused] = step
            tf, tt = [], []
            for _ in range(a.reps):
                tf.append(timed(steps[True], a.seconds))
                tt.append(timed(steps[False], a.seconds))
            print("%5d %6d %24s %24s %12.1f" % (B, n, fmt(tf), fmt(tt), (n / RATE * 1e3) / min(tf)))
        for fused in (True, False):
            s = side[fused]
            print("      (c) %s: %d launches per step; bytes %s" % ("fused" if fused else "twin", s.launches_per_step,
                                                                 json.dumps(s.buffer_bytes())))
        del side
        torch.cuda.empty_cache()
    B = 8
    print("== (b) whole recordings of %d x %d, best of %d (spread)" % (B, CLIP, a.reps))
    os.environ["SRWN_SCORE_FUSED"] = "1"
    sc = model.scorer(max_batch=B, max_chunk=1600, max_frames=MAX_FRAMES)
    clip_np = rng.uniform(-1, 1, (B, CLIP)).astype(np.float32)
    clip = torch.tensor(clip_np, device="cuda")
    enc = sc.encoder._eng.encode(clip)
    model._stage(clip_np, None)
    model._put_encoding(eng, enc.cpu().numpy())

    def loss():      # the decoder engine's forward pass and loss on inputs staged once
        eng.dec.forward()
        return eng.dec.loss
    ts, te, tl = [], [], []
    for _ in range(a.reps):
        ts.append(timed(lambda: sc._eng.score(clip, enc), a.seconds))
        te.append(timed(lambda: sc._eng.score(clip, sc.encoder._eng.encode(clip)), a.seconds))
        tl.append(timed(loss, a.seconds))
    got = float(sc._eng.score(clip, enc).double().sum())
    print("score_with_encoding %s ms, score (encoder included) %s ms, decoder forward + loss %s ms; sum nll %.3f, loss %.3f"
          % (fmt(ts), fmt(te), fmt(tl), got, float(loss().item())))
    tens = [v for v in vars(eng.dec).values() if isinstance(v, torch.Tensor) and v.is_cuda]
    print("      (c) decoder training engine at %d x %d: %d bytes in %d device tensors (lists of tensors not counted); "
          "scorer %s" % (B, CLIP, nb(tens), len(tens), json.dumps(sc._eng.buffer_bytes())))
    if a.parent_lib:
        old_path(a)


if __name__ == "__main__":
    main()
