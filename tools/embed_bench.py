#!/usr/bin/env python3
"""The streaming embedder on one MI355X: embedder.StreamEmbedder and its pool in bf16 at siamese.py's widths (32 residual and
256 skip channels, 2 x [1..512] dilations, 2 output dimensions), hop 160, window 16000, max_hops 8, with N = 1, 64 and 1024
templates enrolled, in the steady state (every stream has a full window behind it), graph replay.

  push        ms per push of one hop at B = 1, 8, 32: the one-launch head (srwn_window_embed_match) against its twin
              (SRWN_EMBED_FUSED=0: srwn_window_mean + srwn_gallery_match), and StreamClassifier.push at the same shape
              (C = D) beside them
  pool        a round of one hop per slot at capacity 32 (one push of 32 host pieces + one step): fused, twin, and the
              classifier pool's round
  old path    with --parent-lib: StreamClassifier.push at B = 8 of this build against another build of the library (the
              parent commit's), alternating fresh processes

Every timed region is device-synchronised and holds >= --seconds of work after a warm-up; best of --reps with the spread.
Each section runs in a process of its own (--only).
usage: python tools/embed_bench.py [--seconds 0.3] [--reps 3] [--only SECTION] [--parent-lib ab/libsrwn_parent.so]"""
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

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 2
R, S, D, HOP, WINDOW, MAX_HOPS = 32, 256, 2, 160, 16000, 8
BS, NS, CAPACITY = (1, 8, 32), (1, 64, 1024), 32
WARM = WINDOW + 4 * HOP


def fmt(v):
    return "%.3f (spread %.3f)" % (min(v), max(v) - min(v))


def weights(cls_name="EmbedderWeights", module="embedder"):
    import torch
    import synth_pool_bench
    synth_pool_bench.modules()      # (an older library under SRWN_LIB_PATH: its missing symbols leave the table)
    mod = importlib.import_module("sr-wavenet_amd." + module)
    w = getattr(mod, cls_name)(DIL, R, S, D, 2, torch.bfloat16)
    w.params.copy_(torch.tensor(np.random.default_rng(0).normal(0, 0.05, w.nparams), dtype=torch.float32))
    w.repack()
    return mod, w


class Pusher:
    """``push`` of one hop [B, 160] (a device tensor) for ever, behind a full window."""

    def __init__(self, make, B, n_gallery=0):
        import torch
        self.c = make(B)
        if n_gallery:
            self.c.enroll(torch.tensor(np.random.default_rng(2).normal(size=(n_gallery, D)), dtype=torch.float32))
        self.st = self.c.start(B)
        rng = np.random.default_rng(1)
        self.c.push(self.st, torch.tensor(rng.uniform(-1, 1, (B, WARM)), dtype=torch.float32, device="cuda"))
        self.x = torch.tensor(rng.uniform(-1, 1, (B, HOP)), dtype=torch.float32, device="cuda")

    def __call__(self):
        self.c.push(self.st, self.x)


class Round:
    """One pool round for ever: every slot gets one hop in one push, then one step."""

    def __init__(self, make, n_gallery=0):
        import torch
        self.c = make(CAPACITY)
        if n_gallery:
            self.c.enroll(torch.tensor(np.random.default_rng(2).normal(size=(n_gallery, D)), dtype=torch.float32))
        self.P = self.c.pool()
        self.us = self.P.join(CAPACITY)
        rng = np.random.default_rng(1)
        self.x = [rng.uniform(-1, 1, HOP).astype(np.float32) for _ in self.us]
        for _ in range(WARM // HOP):
            self()
        assert len(self()) == len(self.us)      # every slot has a full window behind it: each round emits for all

    def __call__(self):
        self.P.push(self.us, self.x)
        return self.P.step()


def _makers(fused):
    """(embedder maker, classifier maker) with SRWN_EMBED_FUSED set for the embedders built from now on."""
    os.environ["SRWN_EMBED_FUSED"] = "1" if fused else "0"
    E, we = weights()
    RC, wc = weights("ClassifierWeights", "recognizer")
    emb = lambda B, mg=1024: E.StreamEmbedder(we, max_batch=B, hop=HOP, window=WINDOW, max_hops=MAX_HOPS, max_gallery=mg)
    cls = lambda B: RC.StreamClassifier(wc, max_batch=B, hop=HOP, window=WINDOW, max_hops=MAX_HOPS)
    return emb, cls


def push(a):
    from synth_pool_bench import timed
    print("== StreamEmbedder.push of one hop (%d samples), ms, best of %d (spread)" % (HOP, a.reps))
    for B in BS:
        _, cls = _makers(True)
        pc = Pusher(cls, B)
        tc = [timed(pc, a.seconds) for _ in range(a.reps)]
        print("B = %2d: StreamClassifier.push %s; launches per step %d" % (B, fmt(tc), pc.c.launches_per_step), flush=True)
        for N in NS:
            pf = Pusher(_makers(True)[0], B, N)
            pt = Pusher(_makers(False)[0], B, N)
            assert pf.c.embed_fused and not pt.c.embed_fused
            t = {"fused": [], "twin": []}
            for _ in range(a.reps):      # alternating, so that a drift of the box reaches both
                t["fused"].append(timed(pf, a.seconds))
                t["twin"].append(timed(pt, a.seconds))
            print("        N = %4d: fused %s; twin %s; fused - twin %+.4f ms; fused - classifier %+.4f ms; launches per step "
                  "%d / %d" % (N, fmt(t["fused"]), fmt(t["twin"]), min(t["fused"]) - min(t["twin"]), min(t["fused"]) - min(tc),
                               pf.c.launches_per_step, pt.c.launches_per_step), flush=True)
            del pf, pt
        del pc


def pool(a):
    from synth_pool_bench import timed
    print("== EmbedderPool: a round of one hop per slot at capacity %d, ms, best of %d (spread)" % (CAPACITY, a.reps))
    rc = Round(_makers(True)[1])
    tc = [timed(rc, a.seconds) for _ in range(a.reps)]
    print("ClassifierPool round %s" % fmt(tc), flush=True)
    for N in NS:
        rf, rt = Round(_makers(True)[0], N), Round(_makers(False)[0], N)
        t = {"fused": [], "twin": []}
        for _ in range(a.reps):
            t["fused"].append(timed(rf, a.seconds))
            t["twin"].append(timed(rt, a.seconds))
        print("N = %4d: fused %s; twin %s; fused - twin %+.4f ms; fused - classifier pool %+.4f ms"
              % (N, fmt(t["fused"]), fmt(t["twin"]), min(t["fused"]) - min(t["twin"]), min(t["fused"]) - min(tc)), flush=True)
        del rf, rt


def old_path_child(a):
    from synth_pool_bench import timed
    RC, wc = weights("ClassifierWeights", "recognizer")
    p = Pusher(lambda B: RC.StreamClassifier(wc, max_batch=B, hop=HOP, window=WINDOW, max_hops=MAX_HOPS), 8)
    print("ABRESULT " + json.dumps({"StreamClassifier.push": [timed(p, a.seconds) for _ in range(a.reps)]}))


def old_path(a):
    libs = [("this", os.path.join(ROOT, "sr-wavenet_amd", "libsrwn.so")), ("parent", os.path.join(ROOT, a.parent_lib))]
    print("== StreamClassifier.push, B = 8, one hop: this build against %s, alternating fresh processes" % a.parent_lib)
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
            d = json.loads(line[0][9:])["StreamClassifier.push"]
            got[name].extend(d)
            print("round %d %-6s %s" % (r, name, " ".join("%.4f" % m for m in d)), flush=True)
    t, p = got["this"], got["parent"]
    print("StreamClassifier.push: this build best %.4f ms (spread %.4f), parent best %.4f ms (spread %.4f): difference %+.4f ms"
          % (min(t), max(t) - min(t), min(p), max(p) - min(p), min(t) - min(p)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another build of libsrwn.so (relative to the repository) for the old path")
    sections = {"push": push, "pool": pool, "old-path": old_path, "old-path-child": old_path_child}
    ap.add_argument("--only", default=None, choices=sorted(sections))
    a = ap.parse_args()
    if a.only == "old-path" and not a.parent_lib:
        sys.exit("--only old-path needs --parent-lib")
    if a.only:
        return sections[a.only](a)
    for name in ("push", "pool"):      # one process per section
        subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name, "--seconds", str(a.seconds), "--reps",
                        str(a.reps)], cwd=ROOT, check=True)
    if a.parent_lib:
        old_path(a)


if __name__ == "__main__":
    main()
