#!/usr/bin/env python3
"""Mixture-of-logistics scorer pools on one MI355X: scorer.MolScorerPool and model.AutoEncoderScorerPool in bf16 at the shape
of tools/mol_score_bench.py (BASELINE config 5's widths: 3 x [1..512] dilations, 64 residual and 256 skip channels, 10
mixtures, 16 latent channels, pool 125), a conditioning ring of 64 frames, max_chunk 1600, 160 samples per stream per round
in the steady state (every stream has its whole history behind it), graph replay.

  pool        a round of 160 samples per stream at B = 1, 8, 32: lockstep MolStreamScorer feed + push of device tensors
              against the all-active pool's round (one push of B host pieces + one ragged feed + one step), the round's
              three parts alone, and B batch-one scorers fed and pushed one after the other
  pair        the same for the whole auto-encoder: AutoEncoderScoreStream.push of a [B, 160] host array against one
              AutoEncoderScorerPool round (push + step), B batch-one streams, and the pair's push alone with its two uploads
              beside the encoder pool's one
  memory      buffer_bytes() of a capacity-32 pool beside the lockstep scorer's and beside 32 batch-one scorers'
  old path    with --parent-lib: MolStreamScorer.push and StreamScorer.push at B = 8 of this build against another build
              of the library (the parent commit's), alternating fresh processes

Every timed region is device-synchronised and holds >= --seconds of work after a warm-up; best of --reps with the spread.
Each section runs in a process of its own (--only).
usage: python tools/mol_score_pool_bench.py [--seconds 0.3] [--reps 3] [--only SECTION] [--parent-lib ab/libsrwn_parent.so]"""
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
R, S, MIX, LAT, POOL, MAX_CHUNK, MAX_FRAMES, N, WARM = 64, 256, 10, 16, 125, 1600, 64, 160, 3200
BS = (1, 8, 32)


def fmt(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def weights():
    import torch
    import synth_pool_bench
    synth_pool_bench.modules()      # (an older library under SRWN_LIB_PATH: its missing symbols leave the table)
    SC = importlib.import_module("sr-wavenet_amd.scorer")
    w = SC.MolScorerWeights(DIL, R, S, MIX, LAT, POOL, 2, torch.bfloat16)
    rng = np.random.default_rng(0)
    w.params.copy_(torch.tensor(rng.normal(0, 0.05, w.nparams), dtype=torch.float32))
    w.repack()
    return SC, w


class Lockstep:
    """MolStreamScorer: the frames the next 160 samples need, then the push, for ever (device tensors)."""

    def __init__(self, SC, w, B):
        import torch
        self.c = SC.MolStreamScorer(w, max_batch=B, max_chunk=MAX_CHUNK, max_frames=MAX_FRAMES)
        self.st = self.c.start(B)
        rng = np.random.default_rng(1)
        self.x = torch.tensor(rng.uniform(-1, 1, (B, N)), dtype=torch.float32, device="cuda")
        self.frames = torch.tensor(rng.normal(size=(B, 2, LAT)), dtype=torch.float32, device="cuda")
        for _ in range(WARM // N):
            self()

    def __call__(self):
        st = self.st
        k = -(-(st.t + N - st.fed * POOL) // POOL)
        if k > 0:
            self.c.feed(st, self.frames[:, :k])
        assert self.c.push(st, self.x).shape[1] == N


class PoolRound:
    """One pool round for ever: every slot gets 160 samples in one push and the frames they need in one feed, then one step."""

    def __init__(self, SC, w, B):
        import torch
        c = SC.MolStreamScorer(w, max_batch=B, max_chunk=MAX_CHUNK, max_frames=MAX_FRAMES)
        self.P = P = c.pool()
        self.us = P.join(B)
        rng = np.random.default_rng(1)
        self.x = [rng.uniform(-1, 1, N).astype(np.float32) for _ in self.us]
        self.frames = torch.tensor(rng.normal(size=(2, LAT)), dtype=torch.float32, device="cuda")
        for _ in range(WARM // N):
            self()
        assert all(P.scored[u] == WARM for u in self.us)

    def _feed(self):
        P = self.P
        k = int(-(-(P._received[self.us[0]] - P._fed[self.us[0]] * POOL) // POOL))
        if k > 0:
            P.feed(self.us, [self.frames[:k]] * len(self.us))

    def __call__(self):
        self.P.push(self.us, self.x)
        self._feed()
        assert len(self.P.step()) == len(self.us)

    # the round's parts alone (the clocks are moved by hand: only the time is of interest)
    def push_only(self):
        self.P.push(self.us, self.x)
        self.P._received[self.us] -= N

    def feed_only(self):      # one frame per slot, the ragged form: a piece per slot
        self.P.feed(self.us, [self.frames[:1]] * len(self.us))
        self.P._fed[self.us] -= 1

    def step_only(self):
        P = self.P
        P._received[self.us] += N
        P._fed[self.us] = -(-P._received[self.us] // POOL)
        assert len(P.step()) == len(self.us)


def pool(a):
    from synth_pool_bench import timed
    SC, w = weights()
    print("== MolScorerPool: a round of %d samples per stream, ms, best of %d (spread)" % (N, a.reps))
    for B in BS:
        ls, pr = Lockstep(SC, w, B), PoolRound(SC, w, B)
        ones = [Lockstep(SC, w, 1) for _ in range(B)]

        def each():
            for o in ones:
                o()
        t = {k: [] for k in ("lockstep feed + push", "pool round", "pool push", "pool feed", "pool step", "B x batch-one")}
        for _ in range(a.reps):
            t["lockstep feed + push"].append(timed(ls, a.seconds))
            t["pool round"].append(timed(pr, a.seconds))
            t["B x batch-one"].append(timed(each, a.seconds))
        for _ in range(a.reps):
            t["pool push"].append(timed(pr.push_only, a.seconds))
            t["pool feed"].append(timed(pr.feed_only, a.seconds))
            t["pool step"].append(timed(pr.step_only, a.seconds))
        print("B = %2d: " % B + "; ".join("%s %s" % (k, fmt(v)) for k, v in t.items()), flush=True)
        print("        B x batch-one / pool round: %.1f x; pool round - lockstep: %+.3f ms; launches per step: %d lockstep, %d "
              "pool" % (min(t["B x batch-one"]) / min(t["pool round"]), min(t["pool round"]) - min(t["lockstep feed + push"]),
                        ls.c.launches_per_step, pr.P.launches_per_step), flush=True)
        del ls, pr, ones


def _autoencoder():
    import torch
    M = importlib.import_module("sr-wavenet_amd.model")
    return M.WaveNetAutoEncoder(16000, 0, MIX, DIL, dilation_channels=R, skip_channels=S, latent_channels=LAT, pool_stride=POOL,
                                dtype=torch.bfloat16)


class PairStream:
    """AutoEncoderScoreStream.push of a [B, 160] host array for ever."""

    def __init__(self, model, B):
        self.sc = model.scorer(max_batch=B, max_chunk=MAX_CHUNK, max_frames=MAX_FRAMES)
        self.st = self.sc.stream(B)
        self.x = np.random.default_rng(1).uniform(-1, 1, (B, N)).astype(np.float32)
        for _ in range(WARM // N):
            self()

    def __call__(self):
        self.st.push(self.x)


class PairRound:
    """One AutoEncoderScorerPool round for ever: 160 samples into every slot (both halves' rings), then one step."""

    def __init__(self, model, B):
        self.sc = model.scorer(max_batch=B, max_chunk=MAX_CHUNK, max_frames=MAX_FRAMES)
        self.P = self.sc.pool()
        self.us = self.P.join(n=B)
        rng = np.random.default_rng(1)
        self.x = [rng.uniform(-1, 1, N).astype(np.float32) for _ in self.us]
        for _ in range(WARM // N):
            self()

    def __call__(self):
        self.P.push(self.us, self.x)
        self.P.step()

    def push_both(self):      # (the clocks are moved by hand: only the time is of interest)
        P = self.P
        P.push(self.us, self.x)
        P._enc._received[self.us] -= N
        P._mol._received[self.us] -= N

    def push_encoder_half(self):
        P = self.P
        P._enc.push(self.us, self.x)
        P._enc._received[self.us] -= N


def pair(a):
    from synth_pool_bench import timed
    model = _autoencoder()
    print("== AutoEncoderScorerPool: a round of %d samples per stream, ms, best of %d (spread)" % (N, a.reps))
    for B in BS:
        ls, pr = PairStream(model, B), PairRound(model, B)
        ones = [PairStream(model, 1) for _ in range(B)]

        def each():
            for o in ones:
                o()
        t = {k: [] for k in ("AutoEncoderScoreStream.push", "pool round", "B x batch-one", "push, two uploads", "push, encoder half")}
        for _ in range(a.reps):
            t["AutoEncoderScoreStream.push"].append(timed(ls, a.seconds))
            t["pool round"].append(timed(pr, a.seconds))
            t["B x batch-one"].append(timed(each, a.seconds))
        for _ in range(a.reps):
            t["push, two uploads"].append(timed(pr.push_both, a.seconds))
            t["push, encoder half"].append(timed(pr.push_encoder_half, a.seconds))
        print("B = %2d: " % B + "; ".join("%s %s" % (k, fmt(v)) for k, v in t.items()), flush=True)
        print("        B x batch-one / pool round: %.1f x; scorer ring %d, encoder ring %d samples per slot"
              % (min(t["B x batch-one"]) / min(t["pool round"]), pr.P._mol.audio_ring, pr.P._enc.audio_ring), flush=True)
        del ls, pr, ones


def memory(a):
    SC, w = weights()
    c = SC.MolStreamScorer(w, max_batch=32, max_chunk=MAX_CHUNK, max_frames=MAX_FRAMES)
    lock = c.buffer_bytes()
    pl = c.pool().buffer_bytes()
    one = SC.MolStreamScorer(w, max_batch=1, max_chunk=MAX_CHUNK, max_frames=MAX_FRAMES).buffer_bytes()
    print("== device bytes, capacity / batch 32, max_chunk %d, %d frames" % (MAX_CHUNK, MAX_FRAMES))
    print("lockstep: total %d  %s" % (sum(lock.values()), json.dumps(lock)))
    print("pool:     total %d  %s" % (sum(pl.values()), json.dumps(pl)))
    print("batch 1:  total %d (x 32 callers = %d; the images %d are shared)  %s"
          % (sum(one.values()), 32 * (sum(one.values()) - one["images"]) + one["images"], one["images"], json.dumps(one)))
    print("launches per step: %d either way" % c.launches_per_step)


def old_path_child(a):
    import torch
    from synth_pool_bench import timed
    SC, w = weights()
    mol = Lockstep(SC, w, 8)
    ws = SC.ScorerWeights(DIL, R, S, 256, 2, torch.bfloat16)
    ws.params.copy_(torch.tensor(np.random.default_rng(0).normal(0, 0.05, ws.nparams), dtype=torch.float32))
    ws.repack()
    s = SC.StreamScorer(ws, max_batch=8, max_chunk=MAX_CHUNK)
    st = s.start(8)
    rng = np.random.default_rng(1)
    s.push(st, torch.tensor(rng.uniform(-1, 1, (8, WARM)), dtype=torch.float32, device="cuda"))
    chunk = torch.tensor(rng.uniform(-1, 1, (8, N)), dtype=torch.float32, device="cuda")
    print("ABRESULT " + json.dumps({"MolStreamScorer.push": [timed(mol, a.seconds) for _ in range(a.reps)],
                                    "StreamScorer.push": [timed(lambda: s.push(st, chunk), a.seconds) for _ in range(a.reps)]}))


def old_path(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so")), ("parent", os.path.join(ROOT, a.parent_lib))]
    print("== the existing pushes, B = 8, %d samples: this build against %s, alternating fresh processes" % (N, a.parent_lib))
    got = {k: {} for k, _ in libs}
    for r in range(a.rounds):
        for name, path in libs:
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "old-path-child", "--seconds",
                                 str(max(a.seconds, 0.5)), "--reps", str(a.reps)], env=dict(os.environ, SRWN_LIB_PATH=path),
                                cwd=ROOT, capture_output=True, text=True, timeout=300)
            line = [l for l in pr.stdout.splitlines() if l.startswith("ABRESULT ")]
            if pr.returncode or not line:
                print("FAILED", name, pr.stderr[-2000:], flush=True)
                return
            for k, d in json.loads(line[0][9:]).items():
                got[name].setdefault(k, []).extend(d)
                print("round %d %-6s %-22s %s" % (r, name, k, " ".join("%.4f" % m for m in d)), flush=True)
    for k in got["this"]:
        t, p = got["this"][k], got["parent"][k]
        print("%s: this build best %.4f ms (spread %.4f), parent best %.4f ms (spread %.4f): difference %+.4f ms"
              % (k, min(t), max(t) - min(t), min(p), max(p) - min(p), min(t) - min(p)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for the old path")
    sections = {"pool": pool, "pair": pair, "memory": memory, "old-path": old_path, "old-path-child": old_path_child}
    ap.add_argument("--only", default=None, choices=sorted(sections))
    a = ap.parse_args()
    if a.only == "old-path" and not a.parent_lib:
        sys.exit("--only old-path needs --parent-lib")
    if a.only:
        return sections[a.only](a)
    for name in ("pool", "pair", "memory"):      # one process per section
        subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name, "--seconds", str(a.seconds), "--reps",
                        str(a.reps)], cwd=ROOT, check=True)
    if a.parent_lib:
        old_path(a)


if __name__ == "__main__":
    main()
