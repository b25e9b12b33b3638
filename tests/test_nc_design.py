"""CPU checks of tests/nc_design.py for every shape tests/test_gpu_nc_entries.py runs: the range conditions that make the
chained designs exact, their coverage, the quotas of exact zeros and of rounding ties, the mask-word codec against a
scalar statement of the layout, the figures the per-entry bounds' constants come from and the cap on undecided relu
entries.  No GPU, no import of the product."""
import os

import numpy as np
import pytest

from tests import gemm_design as G
from tests import nc_design as N


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR") == "1":
        print(*a)


@pytest.mark.parametrize("B,T", N.SHAPES)
def test_forward_design_is_exact_covers_and_meets_zeros_and_ties(B, T):
    c = N.check_fwd_exact(B, T)
    _say("fwd (%d, %d): S1 %d S2 %d  pre_a > 0 %.3f = 0 %.3f  pre_r = 0 %.3f  ties of r' %.3f"
         % (B, T, c["S1"], c["S2"], c["pos_a"], c["zeros_a"], c["zeros_r"], c["ties_r"]))
    assert c["S1"] <= G.S_MAX16 and c["S2"] < G.S_MAX
    if B * T >= 31:       # (one row: 128 entries, the quotas are those of the shapes with a tile's worth of rows)
        assert c["zeros_a"] >= 0.01 and c["zeros_r"] >= 0.01 and c["ties_r"] >= 0.01
        assert 0.4 < c["pos_a"] < 0.6
    if (B, T) == (3, 22405):       # the figures DESIGN.md quotes
        assert c["S1"] <= 200 and c["S2"] <= 3500
        assert 0.02 < c["zeros_a"] < 0.04 and 0.02 < c["zeros_r"] < 0.05 and 0.05 < c["ties_r"] < 0.10
    # the second relu's zeros sit where the design put them, and nowhere by accident of a dense column only
    assert (c["pre_r"][:, list(N.ZERO_COLS)] == 0).sum() >= 0.9 * (c["pre_r"] == 0).sum()


@pytest.mark.parametrize("B,T", N.SHAPES)
def test_backward_design_is_exact_covers_and_meets_ties(B, T):
    c = N.check_bwd_exact(B, T)
    _say("bwd (%d, %d): S1 %d S2 %d  ties of dpre %s" % (B, T, c["S1"], c["S2"], ["%.3f" % t for t in c["ties"]]))
    assert c["S1"] <= G.S_MAX16 and c["S2"] < G.S_MAX
    assert len(c["ties"]) == 1 + len(N.fadd_cases(B, T))
    if B * T >= 31:
        assert min(c["ties"]) >= 0.01


def test_fadd_cases_cover_what_the_kernel_distinguishes():
    for (B, T) in N.SHAPES:
        cases = N.fadd_cases(B, T)
        for (pool, frames, ld, off) in cases:
            assert frames * pool >= T and ld >= N.C and off + N.C <= ld and pool >= 1
        assert any(p == 25 for p, *_ in cases)
        if (B, T) in N.SMALL:
            assert {1, 25, 32, T + 3} == {p for p, *_ in cases}
            assert any(f * p > T + p - 1 for p, f, *_ in cases)                   # a whole spare frame
            assert any(ld > N.C and off > 0 for _, _, ld, off in cases)
    assert N.FADD_SCALE not in [1.0 / p for (B, T) in N.SHAPES for p, *_ in N.fadd_cases(B, T)]
    assert all(B >= 2 for (B, T) in N.SHAPES if T > 32)                          # a clip boundary wherever there is a tile edge
    assert [B * -(-T // 32) for (B, T) in N.LARGE] == [1056, 2103]


# ---- the mask words -----------------------------------------------------------------------------------------------------
def _word_scalar(x, B, T, tile, lane):
    """One word, written out from the documented layout, one value at a time."""
    ntb = -(-T // 32)
    b, t = tile // ntb, 32 * (tile % ntb) + (lane % 32)
    half = lane // 32
    if t >= T:
        return None
    word = 0
    for mt in range(4):
        for q in range(16):
            ch = 32 * mt + 8 * (q >> 2) + 4 * half + (q & 3)
            if x[b * T + t, ch] > 0:
                word |= 1 << (32 * (mt >> 1) + 31 - (16 * (mt & 1) + q))
    return word


@pytest.mark.parametrize("B,T", [(1, 1), (2, 33), (3, 50), (2, 64)])
def test_mask_words_follow_the_layout_and_invert(B, T):
    rng = np.random.default_rng(B * 100 + T)
    x = rng.choice([-1.0, -0.0, 0.0, 2.0 ** -126, 1.0], (B * T, N.C))
    inside = N.lanes_inside(B, T)
    assert inside.size == N.nwords(B, T) and inside.sum() == 2 * B * T
    for beyond in (0, 1):
        w = N.mask_words(x, B, T, beyond)
        assert w.dtype == np.uint64 and w.size == N.nwords(B, T)
        for i in rng.choice(w.size, min(w.size, 40), replace=False):
            want = _word_scalar(x, B, T, i // 64, i % 64)
            assert (want is None) == (not inside[i])
            assert int(w[i]) == (want if want is not None else (0xFFFFFFFFFFFFFFFF if beyond else 0))
        assert np.array_equal(N.mask_unwords(w, B, T), x > 0)
    # every (channel, time row) owns exactly one bit: a single positive value sets a single bit
    for ch in (0, 5, 36, 127):
        one = np.zeros((B * T, N.C)); one[B * T - 1, ch] = 1.0
        w = N.mask_words(one, B, T)
        assert sum(bin(int(v)).count("1") for v in w) == 1


def test_mask_words_at_the_large_shapes_invert():
    for (B, T) in N.LARGE:
        m = N.bwd_exact(B, T)["mr"]
        assert np.array_equal(N.mask_unwords(N.mask_words(m, B, T, 1), B, T), m > 0)


# ---- the bound's constants and the undecided share ----------------------------------------------------------------------
def measured():
    out, und = {}, {}
    for (B, T) in N.RANDOM_SHAPES:
        d = N.fwd_random(B, T)
        a32, r32 = N.restate32_fwd(d, B, T)
        pre_a, S1, _, ref_r, ref_S2 = N.fwd_ref(d, B, T)
        pre_r, S2 = G.contract(a32, d["wr"], d["br"])                     # fed the restatement's own stored a
        for key, got, pre, S, K in (("nc_fwd_a", a32, pre_a, S1, 2 * N.C), ("nc_fwd_r", r32, pre_r, S2, N.C)):
            r, undecided, wrong = N.relu_entries(got, pre, S, K, key)
            assert not wrong.any()
            out[key] = max(out.get(key, 0.0), float(r.max()))
        # the undecided share, on the reference alone
        und[("nc_fwd_a", B, T)] = float(N.relu_entries(np.maximum(pre_a, 0), pre_a, S1, 2 * N.C, "nc_fwd_a")[1].mean())
        und[("nc_fwd_r", B, T)] = float(N.relu_entries(np.maximum(ref_r, 0), ref_r, ref_S2, N.C, "nc_fwd_r")[1].mean())
        d = N.bwd_random(B, T)
        dh32, dp32 = N.restate32_bwd(d, B, T)
        dh, S1 = N.bwd_dh_ref(d, B, T)
        fa = d["scale"] * N.frame_rows(d["fadd"], B, T, d["pool"])
        dpre, S2 = N.bwd_dpre_ref(dh32, d, fa)
        out["nc_bwd_dh"] = max(out.get("nc_bwd_dh", 0.0), float(G.ratio(dh32, dh, S1, 2 * N.C, "bf16").max()))
        out["nc_bwd_dpre"] = max(out.get("nc_bwd_dpre", 0.0), float(G.ratio(dp32, dpre, S2, N.C + 1, "bf16").max()))
    return out, und


def test_bound_constants_come_from_the_float32_restatement_and_few_entries_are_undecided():
    m, und = measured()
    _say("\nfloat32 restatement, worst error / bound scale:", {k: round(v, 3) for k, v in m.items()})
    _say("undecided share:", {k: "%.5f" % v for k, v in und.items()})
    assert set(m) == set(N.C_CPU)
    for k, v in m.items():
        assert 0 < v and N.C_CPU[k] == G.rounded_up(v), (k, v, N.C_CPU[k])
        assert N.C_GPU[k] == 4 * N.C_CPU[k]
    assert max(und.values()) <= N.UNDECIDED_CAP, und
