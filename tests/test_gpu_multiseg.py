"""The group kernels with SEVERAL segments per workgroup.  A group kernel's grid is min(segments, CUs) and each workgroup
walks segments blockIdx.x, blockIdx.x + gridDim.x, ...: at one segment per workgroup (every other test, and the benchmark's
8 x 16000) the second trip never runs -- the partial sums carried from one segment to the next (fp32 slabs, bf16 blocks,
bias column sums, the fused input conv's gradient), the LDS state a segment leaves behind, the segment map for
sblk >= gridDim.x.  SRWN_GROUP_GRID = cap (a test hook, csrc/srwn_group.h group_grid) gives the launches at most `cap`
workgroups and partial slabs with the segment geometry unchanged, so that:

  capped vs uncapped   same engine config: activations, the chain and the loss bit-equal; the weight gradients summed
                       through the per-workgroup partials equal to their summation order; run twice, bit-identical
  vs the fp64 oracle   config 2 at 8 x 16000 with 8 and 16 segments per workgroup, and at its depth geometry (fp32)
  bf16 partials        how the bf16 partial blocks' error grows with segments per workgroup (k = 1 .. 32)
  production           16 x 16000 on the default path: more segments than CUs in every group, no hook
"""
import math
import os

import numpy as np
import pytest
import torch

from tests._pkg import sub
from tests.test_gpu_depth import CONFIG2_SHAPE, DIL30, _assert_bf16, _check, _config2_case
from tests.test_gpu_depth import _engine as _depth_engine
from tests.test_gpu_fullsize import BF16_FULL_SIZE, _full_size_oracle
from tests.test_gpu_fullsize import _engine as _full_engine
from tests.test_gpu_group import PART16_TOL, SHAPES, _pair, _rel
from tests.test_gpu_kernels import dev

pytestmark = pytest.mark.gpu

ORDER_TOL = 2e-6      # fp32 partial sums regrouped over fewer workgroups: summation order only


def _nsegs(eng, seg_rows=0):
    """Segments of each multi-layer group of `eng` (the weight-gradient-tile cut; the plain kernels' is the same or close)."""
    K = sub("kernels")
    out = []
    for l0, l1 in eng.groups:
        if l1 - l0 < 2:
            continue
        d = eng.dil[l0:l1]
        W = K.group_wt_geometry(d, eng.B, eng.T, eng.R, eng.dt, seg_rows)[0]
        st = math.gcd(*d)
        J = -(-eng.T // st)                       # positions per residue class
        out.append(eng.B * st * -(-J // W))
    return out


def _outputs(e):
    """What a forward + backward leaves that the grid may not change (and the gradients, compared separately)."""
    out = {"loss": e.loss.clone(), "zs": e.zs.clone(), "grads": e.grads.clone()}
    for l0, l1 in e.groups:
        out["x%d" % l1] = e.xs[l1].clone()        # (weight-gradient-tile mode: only the groups' top layers store x)
        out["g%d" % l0] = e.gs[l0].clone()        # the groups' bottom gradients
    if e.fused_wt:
        out["xTs"], out["cTs"] = e.xTs.clone(), e.cTs.clone()
    return out


def _run(monkeypatch, cap, dil, B, T, R, S, C, dt, seg, fuse_wt, E=0, pool=1, twice=False):
    if cap:
        monkeypatch.setenv("SRWN_GROUP_GRID", str(cap))
    else:
        monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    _, eng = _pair(monkeypatch, dil, B, T, R, S, C, dt, E=E, pool=pool, seg_rows=seg, fuse_wt=fuse_wt)
    runs = []
    for _ in range(2 if twice else 1):
        eng.forward(); eng.backward()
        torch.cuda.synchronize()
        runs.append(_outputs(eng))
    monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    return eng, runs


MS_SHAPES = [
    # dilations,                     B, T,    R,  S,   seg_rows, E,  pool, classes   segments per group
    SHAPES[0] + (0, 1, 256),                                                           # 10 (not a multiple of 8)
    SHAPES[2] + (0, 1, 256),                                                           # 64 (stride 32: residue classes)
    SHAPES[3] + (0, 1, 64),                                                            # 16 (stride 4, forced short segments)
    ([1, 2, 4, 8, 16] * 2,           2, 1500, 32, 128, 64,       0,  1,    64),        # 48, R = 32
    ([1, 2, 4, 8, 16, 32, 64],       2, 400,  64, 256, 128,      16, 8,    64),        # 8 and 64, conditioned
]
MODES = [  # dtype, SRWN_FUSE_WT, SRWN_PART16 (2: bf16 partial blocks even where a workgroup runs several segments)
    (torch.float32, "0", "1"), (torch.float32, "1", "1"),
    (torch.bfloat16, "0", "1"), (torch.bfloat16, "1", "0"), (torch.bfloat16, "1", "1"), (torch.bfloat16, "1", "2"),
]


@pytest.mark.parametrize("dt,fuse_wt,part16", MODES)
@pytest.mark.parametrize("dil,B,T,R,S,seg,E,pool,C", MS_SHAPES)
def test_capped_grid_equals_uncapped(monkeypatch, dt, fuse_wt, part16, dil, B, T, R, S, seg, E, pool, C):
    """Caps 1, 3, 7 and nseg - 1 (one workgroup of the largest group takes a second segment) against the uncapped grid of
    the same engine config.  Which workgroup runs which segment must not change any stored activation, the chain or the
    loss; the weight gradients summed through the per-workgroup partials (conv taps, residual 1x1, their biases; the input
    conv's when the first group forms it; the skip 1x1's when srwn_wgrad_skip_wt does) change only by their summation
    order -- bf16 partial blocks by their rounding too -- and nothing else may change at all.  Every capped case runs
    twice: a race between a workgroup's segments would show as a difference from one run to the next.  (Default bf16
    partial blocks: a group with more segments than workgroups falls back to fp32 slabs, asserted here; SRWN_PART16=2
    keeps the blocks there, whose error grows with the segments per workgroup -- bounded by the k-curve test below.)"""
    monkeypatch.setenv("SRWN_PART16", part16)
    base, (want,) = _run(monkeypatch, 0, dil, B, T, R, S, C, dt, seg, fuse_wt, E, pool)
    assert base.fuse_fwd and base.fused_bwd and base.fused_wt == (fuse_wt == "1")
    nsegs = _nsegs(base, seg)
    nseg = max(nsegs)
    caps = sorted({c for c in (1, 3, 7, nseg - 1) if 1 <= c < nseg})
    assert caps, nseg
    assert base.group_p16 == ([base.part16] * len(nsegs) if base.fused_wt else [])
    names = set()
    if base.fused_wt:
        names = {"WF", "WR", "BF", "BR"} | ({"init_w", "init_b"} if base.fuse_icg else set()) | ({"WS", "BS"} if base.skip_wt else set())
    if base.Cp != 256:      # (fewer classes: the head's last 1x1 is summed over the engine's partial slabs as well)
        names |= {"head_w2", "head_b2"}
    p16 = ({"WF", "WR"} | ({"WS"} if base.skip_parts16 is not None else set())) if base.part16 else set()
    for cap in caps:
        eng, (got, again) = _run(monkeypatch, cap, dil, B, T, R, S, C, dt, seg, fuse_wt, E, pool, twice=True)
        if eng.fused_wt:
            assert eng.nslabs == cap < base.nslabs, (cap, eng.nslabs, base.nslabs)
            assert eng.group_p16 == [eng.part16 and (n <= cap or part16 == "2") for n in nsegs], (cap, eng.group_p16)
            assert eng.fuse_icg == base.fuse_icg      # (with fp32 slabs too: the first group still forms init_w / init_b)
        for k in got:
            assert torch.equal(got[k], again[k]), "cap %d: %s differs between two runs" % (cap, k)
        for k in want:
            if k != "grads":
                assert torch.equal(got[k], want[k]), "cap %d: %s" % (cap, k)
        for n in base.sections:      # (per kind: every layer's WF together, ...)
            w, g = base.view(n, want["grads"]), eng.view(n, got["grads"])
            if n in names:
                assert bool(torch.isfinite(g).all()), (cap, n)
                if n in p16 and part16 == "2":
                    continue        # (bf16 running sums over several segments: test_bf16_partial_error_vs_segments_per_workgroup)
                tol = PART16_TOL if n in p16 else ORDER_TOL
                assert _rel(g, w) < tol, (cap, n, _rel(g, w))
            else:
                assert torch.equal(g, w), (cap, n)
        del eng


@pytest.mark.parametrize("cap", [32, 16])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_full_size_many_segments_per_workgroup_vs_oracle(monkeypatch, dt, cap):
    """Config 2 at 8 x 16000 (256 segments in every group) on 32 and 16 workgroups -- 8 and 16 segments each -- against
    oracle (ii) on the same inputs as test_full_size_vs_oracle, with its bounds: fp32 1e-3, bf16 BF16_FULL_SIZE."""
    ref = _full_size_oracle()
    monkeypatch.setenv("SRWN_GROUP_GRID", str(cap))
    eng = _full_engine(dt)
    eng.load_oracle_params(ref["sp"])
    assert eng.fused_wt and eng.nslabs == cap
    if dt == torch.bfloat16:      # the timed path, 256 segments per group, on `cap` workgroups
        assert eng.skip_wt and eng.head_chain and eng.part16 and sorted(set(eng.wt_seg_rows)) == [500]
        assert _nsegs(eng) == [256] * len(eng.groups)
        assert not any(eng.group_p16)      # more segments than workgroups: fp32 partial slabs in every group
    else:                         # (fp32 mode's smaller segment images: 664 and 768 segments per group)
        assert min(_nsegs(eng)) > 256
    eng.set_inputs(dev(ref["audio"]), dev(ref["codes"], torch.int32))
    errs = _check(eng, ref["logits"], ref["loss"], ref["grads"], dt)
    if errs is not None:
        if os.environ.get("SRWN_PRINT_BF16_ERRS"):
            print("MEASURED full size bf16, %d segments per workgroup: logits %.3e loss %.3e worst grad %.3e (%s)" % (
                256 // cap, errs["logits"], errs["loss"], *max((v, k) for k, v in errs.items() if k not in ("logits", "loss"))))
        _assert_bf16(errs, *BF16_FULL_SIZE)


def test_config2_depth_capped_grid_vs_oracle_fp32(monkeypatch):
    """Config 2's depth geometry (2 x 4300, 66 and 64 segments per group) in fp32 on 7 workgroups: about ten segments each,
    the last trip partial; the 1e-3 bound of test_config2_depth_and_dilations_vs_oracle."""
    sp, audio, codes, (logits, loss, grads) = _config2_case()
    monkeypatch.setenv("SRWN_GROUP_GRID", "7")
    eng = _depth_engine(sp, DIL30, *CONFIG2_SHAPE, torch.float32)
    assert eng.fused_wt and eng.nslabs == 7 and min(_nsegs(eng)) > 7 * 8
    eng.set_inputs(dev(audio), dev(codes, torch.int32))
    assert _check(eng, logits, loss, grads, torch.float32) is None


K_CURVE = (1, 2, 4, 8, 16, 32)
K_BLOCKS_OK = 8      # most segments per workgroup at which the bf16 running sums stay within PART16_TOL (measured: 3.9e-3)


def test_bf16_partial_error_vs_segments_per_workgroup(monkeypatch):
    """bf16 partial blocks against fp32 slabs at k = 1 .. 32 segments per workgroup: config 2's stack on one 4096-sample clip
    cut into 128-position segments, 32 segments in every group, on 32 / k workgroups.  A later segment re-reads the
    workgroup's bf16 block, adds its fp32 sum and rounds again: k roundings of the running sum per partial, and the error
    grows with k (SRWN_PART16=2 keeps the blocks in every group; SRWN_PRINT_ERR=1 prints the curve): within
    PART16_TOL up to K_BLOCKS_OK.  The default (SRWN_PART16=1) keeps blocks only where k = 1 and is held to PART16_TOL at
    every k.  (The skip 1x1s' blocks, srwn_wgrad_skip_wt, sum a slab's segments in registers: one rounding at any k.)"""
    EG = sub("engine")
    B, T, R, S, C = 1, 4096, 64, 256, 256
    cfg = EG.StackConfig(dilations=DIL30, dilation_channels=R, skip_channels=S, output_channels=C, shift_input=True,
                         dtype=torch.bfloat16)
    monkeypatch.setenv("SRWN_SEG_ROWS", "128")
    rng = np.random.default_rng(3)
    audio = torch.tensor(np.clip(0.5 * np.sin(np.arange(B * T).reshape(B, T) * 0.05) + 0.1 * rng.normal(size=(B, T)), -1, 1),
                         dtype=torch.float32, device="cuda")
    tg = torch.tensor(rng.integers(0, C, size=(B, T)), dtype=torch.int32, device="cuda")
    curve = {"2": {}, "1": {}}
    for k in K_CURVE:
        monkeypatch.setenv("SRWN_GROUP_GRID", str(32 // k))
        grads = {}
        for p16 in ("0", "1", "2"):
            monkeypatch.setenv("SRWN_PART16", p16)
            e = EG.WaveNetEngine(cfg, B, T, "cuda", seed=3)
            assert e.fused_wt and e.skip_wt and e.part16 == (p16 != "0") and e.nslabs == 32 // k
            assert _nsegs(e, 128) == [32] * len(e.groups)
            assert e.group_p16 == [p16 == "2" or (p16 == "1" and k == 1)] * len(e.groups)      # the fallback
            e.set_inputs(audio, tg)
            e.forward(); e.backward()
            torch.cuda.synchronize()
            grads[p16] = {n: e.view(n, e.grads).clone() for n in ("WF", "WR", "WS")}
            del e
        for p16 in ("1", "2"):
            curve[p16][k] = {n: _rel(grads[p16][n], grads["0"][n]) for n in ("WF", "WR", "WS")}
    if os.environ.get("SRWN_PRINT_ERR"):
        for p16, what in (("2", "bf16 blocks in every group"), ("1", "default")):
            print("MEASURED part16 vs fp32 partials by segments per workgroup, %s (rel L2):" % what,
                  {k: {n: "%.2e" % v for n, v in c.items()} for k, c in curve[p16].items()})
    for k in K_CURVE:
        for n in ("WF", "WR", "WS"):
            assert curve["1"][k][n] < PART16_TOL, (k, n, curve["1"][k][n])
            if k <= K_BLOCKS_OK:
                assert curve["2"][k][n] < PART16_TOL, (k, n, curve["2"][k][n])


def test_production_geometry_more_segments_than_cus_vs_oracle():
    """No hook: config 2 bf16 at 16 x 16000 -- one engine batch of SiameseWaveNet's 8-pair 'wide' case -- on the default
    path.  Every group has more segments than the 256 workgroups, so each workgroup runs a second one; against oracle (ii)
    on all 16 clips with BF16_FULL_SIZE."""
    assert "SRWN_GROUP_GRID" not in os.environ
    ref = _full_size_oracle(16)
    eng = _full_engine(torch.bfloat16, batch=16)
    eng.load_oracle_params(ref["sp"])
    assert eng.fused_wt and eng.skip_wt and eng.head_chain and eng.part16
    assert eng.nslabs == 256
    nseg = _nsegs(eng)
    assert all(n > eng.nslabs for n in nseg), nseg
    assert not any(eng.group_p16) and eng.fuse_icg      # the fallback: fp32 partial slabs in every group (input conv fused)
    eng.set_inputs(dev(ref["audio"]), dev(ref["codes"], torch.int32))
    errs = _check(eng, ref["logits"], ref["loss"], ref["grads"], torch.bfloat16)
    if os.environ.get("SRWN_PRINT_BF16_ERRS"):
        print("MEASURED 16 x 16000 bf16 (segments per group %s): logits %.3e loss %.3e worst grad %.3e (%s)" % (
            sorted(set(nseg)), errs["logits"], errs["loss"], *max((v, k) for k, v in errs.items() if k not in ("logits", "loss"))))
    _assert_bf16(errs, *BF16_FULL_SIZE)
