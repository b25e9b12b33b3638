"""CPU proofs for tests/group_design.py (no GPU): the designs are on their grids and cover every weight row, column
and tap and every time row; the float32 NumPy restatement of a layer -- the kernel's stand-in -- stays within C_CPU of
the float64 layer-local reference and agrees with it BIT FOR BIT on every decided entry (so the reach is wide enough);
in bf16 mode at least 90 % of every stored tensor is decided and no time row or channel column is wholly undecided,
with df stored (srwn_residual_group_bwd) and with df reconstructed (srwn_residual_group_bwd_wt); the exact corners' sums
are in range; the tile decode returns the rows it was given; the gate of a stored z and the row-by-row weight gradients
stay within their constants.  SRWN_PRINT_ERR=1 pytest -s prints the measured ratios and shares."""
import os

import numpy as np
import pytest

from tests import gemm_design as G
from tests import group_design as D

MODES = ["bf16", "fp32"]
WORST = {}


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _runs():
    return D.RUNS


def test_runs_reach_every_variant_and_width():
    runs = D.RUNS
    assert {v for _, _, v in runs} == set(D.VARIANTS) and {R for _, R, _ in runs} == {32, 64}
    assert {i for i, _, _ in runs} == set(range(len(D.CASES)))


def test_rounding_helpers():
    rng = np.random.default_rng(1)
    x32 = (rng.normal(size=4000) * 2.0 ** rng.integers(-12, 6, 4000)).astype(np.float32).astype(np.float64)
    assert np.array_equal(D.round_to(x32, "bf16"), G.bf16_round(x32))            # one step = G's rounding on fp32 values
    ties = np.array([1.00390625, 1.01171875, -3.0234375, 0.0])                    # odd multiples of half a bf16 ulp, zero
    assert np.array_equal(D.round_to(ties, "bf16"), [1.0, 1.015625, -3.03125, 0.0])
    assert np.array_equal(D.midpoint_distance(ties, "bf16"), [0.0, 0.0, 0.0, np.inf])
    v = np.array([1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23, 3.0])
    assert np.array_equal(D.midpoint_distance(v, "fp32"), [0.0, 2.0 ** -24, 2.0 ** -23])
    assert np.array_equal(D.midpoint_distance(x32, "bf16"), G.midpoint_distance(x32))
    assert np.array_equal(D.ulp_of(np.array([1.0, 1.5, 2.0, 0.75]), "bf16"), [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8])
    assert float(D.SQRT_HALF32) == float(np.float32(G.SQRT_HALF))


def test_derivative_is_exact_at_zero_and_small_at_one():
    """c'(0) = 1/2 exactly in both restatements (df = dc / 2 there: the exact corner); c'(+-1) = 0 in fp32 mode (1 - z^2)
    and the polynomial's residue, below 1e-6, in bf16 mode."""
    for mode in MODES:
        assert float(G.dgate32(np.array([0.0]), mode)[0]) == 0.5 and D.f_abs_z(np.array([0.0]), mode)[0] == 0
    assert not G.dgate32(np.array([-1.0, 1.0]), "fp32").any()
    assert 0 < np.abs(G.dgate32(np.array([-1.0, 1.0]), "bf16")).max() < 1e-6


@pytest.mark.parametrize("i", range(len(D.CASES)))
def test_designs_on_grid_and_covering(i):
    dil, B, T, seg = D.CASES[i]
    for R in (32, 64):
        for v in D.VARIANTS:
            d = D.design(dil, B, T, R, v)
            D.check_design(d)
            assert (d["dcs"] is None) == (v == "gtop") and (d["g_top"] is None) == (v == "dcs")
            for l in range(len(dil)):
                for k in range(2):                  # every row and column of every tap, and of the 1x1
                    assert np.abs(d["wf"][l, k]).sum(0).min() > 0 and np.abs(d["wf"][l, k]).sum(1).min() > 0
                assert np.abs(d["wr"][l]).sum(0).min() > 0 and np.abs(d["wr"][l]).sum(1).min() > 0
            for k in ("dcs", "g_top"):              # every time row (so every residue class, segment and tile position)
                if d[k] is not None:                # and every channel carries a non-zero operand
                    assert (np.abs(d[k]) > 0).all()
            assert set(np.unique(d["z"])) == set(D.Z_GRID) or B * T * R < 500


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i,R,variant", D.RUNS)
def test_restatement_within_c_cpu_and_exact_where_decided(i, R, variant, mode):
    dil, B, T, seg = D.CASES[i]
    d = D.design(dil, B, T, R, variant)
    n = len(dil)
    df32, G32 = D.restate_chain(d, mode)
    Gup = d["g_top"]
    for l in range(n - 1, -1, -1):
        rdf = D.layer_df_ref(d, l, Gup, mode)
        rG = D.layer_G_ref(d, l, Gup, df32[l], mode)
        pre = {"df": D.restate_df32(d, l, Gup, mode)[0], "G": D.restate_G32(d, l, Gup, df32[l], mode)[0]}
        for key, r, got in (("df", rdf, df32[l]), ("G", rG, G32[l])):
            what = "%s %s R %d %s layer %d %s" % (D.CASES[i], variant, R, mode, l, key)
            err = np.abs(pre[key] - r["x"])
            assert (err[r["e"] == 0] == 0).all(), what + ": e = 0 but the fp32 evaluation is not exact"
            assert np.array_equal(D.round_to(r["x"], mode)[r["e"] == 0], r["x"][r["e"] == 0]) or mode == "bf16"
            rp = np.where(r["e"] > 0, err / np.where(r["e"] > 0, r["e"], 1.0), 0.0)
            ro = D.out_ratio(got, r, mode)
            for k2, val in (("grp_%s_pre" % key, rp.max()), ("grp_%s_out" % key, ro.max())):
                WORST[(k2, mode)] = max(WORST.get((k2, mode), 0.0), float(val))
                assert val <= D.C_CPU[k2][mode], "%s: %s %.3f > C_CPU %.3f" % (what, k2, val, D.C_CPU[k2][mode])
            dec = D.decided(r, mode, D.REACH[key][mode])
            assert G.same_bits(got, r["ref"])[dec].all(), what + ": a decided entry of the restatement differs"
            assert (np.abs(got - r["x"]) <= D.bound(r, mode, D.C_GPU[key][mode])).all(), what
            share = dec.mean()
            WORST[("decided_%s" % key, mode)] = min(WORST.get(("decided_%s" % key, mode), 1.0), float(share))
            if mode == "bf16":                      # the cap (fp32: decided only where e = 0, see tests/group_design.py)
                assert share >= D.CAP, "%s: %.1f %% decided" % (what, 100 * share)
                assert dec.any(0).all() and dec.any(1).all(), what + ": a row or a column wholly undecided"
            else:
                assert np.array_equal(dec, r["e"] == 0) or (dec >= (r["e"] == 0)).all()
        Gup = G32[l]
    _say("%-40s %-5s R %d %-4s worst so far %s" % (D.CASES[i], variant, R, mode,
                                                    {k[0]: round(v, 4) for k, v in sorted(WORST.items()) if k[1] == mode}))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i", range(len(D.CASES)))
def test_exact_corner(i, mode):
    """g_top = None, z = 0: the top layer is a dyadic design in range (its fp32 restatement equals the float64 reference
    rounded once, no entry excluded), and in every layer df is decided wherever that layer's Wr has a zero row."""
    dil, B, T, seg = D.CASES[i]
    for R in (32, 64):
        d = D.design(dil, B, T, R, exact_corner=True)
        D.check_design(d)
        n = len(dil)
        df, t, units = D.exact_top(d)
        assert units.max() < G.S_MAX and np.array_equal(df / (0.5 * D.GD), np.rint(df / (0.5 * D.GD)))
        df32, G32 = D.restate_chain(d, mode)
        assert G.same_bits(df32[n - 1], D.round_to(df, mode)).all()
        assert G.same_bits(G32[n - 1], D.round_to(t, mode)).all()
        Gup = None
        for l in range(n - 1, -1, -1):
            zero_rows = ~np.abs(d["wr"][l]).any(1)
            assert zero_rows.sum() == R // 4
            r = D.layer_df_ref(d, l, Gup, mode)
            assert (r["e"][:, zero_rows] == 0).all() and D.decided(r, mode, D.REACH["df"][mode])[:, zero_rows].all()
            assert np.array_equal(r["ref"][:, zero_rows], 0.5 * d["dcs"][l][:, zero_rows])
            Gup = G32[l]


@pytest.mark.parametrize("B,T,st,W", [(2, 77, 1, 40), (2, 45, 4, 33), (1, 100, 32, 32), (3, 1, 1, 1), (2, 131, 4, 24)])
def test_tile_decode_returns_the_rows(B, T, st, W):
    """D.ct_decode(G.ct_encode(c)) holds row G.ct_rows of c in every owned element and the poison elsewhere; every time
    row is owned by exactly one tile element."""
    R = 32
    c = np.arange(B * T * R, dtype=np.float64).reshape(B * T, R) + 1.0
    row, ok = G.ct_rows(B, T, st, W)
    got = D.ct_decode(G.ct_encode(c, B, T, R, st, W, -7.0), row.shape[0], row.shape[1], R)
    assert np.array_equal(got[ok], c[row[ok]]) and (got[~ok] == -7.0).all()
    assert np.array_equal(np.sort(row[ok]), np.arange(B * T))
    assert np.array_equal(D.tile_written(B, T, st, W), (G.ct_geometry(B, T, st, W)[5][:, None] > 32 * np.arange(row.shape[1])))


@pytest.mark.parametrize("mode", MODES)
def test_gate_of_stored_z_within_c_cpu(mode):
    f = np.linspace(-3, 3, 40001)
    z, c = D.gate_restate32(f, mode)
    r = np.abs(c - G.gate64(z)) / D.gate_scale(z, mode)
    _say("gate of the stored z, %s: worst error / scale %.3f (C_CPU %g)" % (mode, r.max(), D.C_CPU_GATE[mode]))
    assert r.max() <= D.C_CPU_GATE[mode]


def test_input_conv_design_is_exact():
    for shift in (0, 1):
        d = D.ic_design(2, 45, 64)
        x = D.ic_x0(d, 2, 45, shift)
        assert G.is_bf16(x) and G.is_bf16(d["audio"]) and np.abs(x).sum(1).min() > 0
        f = np.float32       # two orders of the three fp32 terms
        a1 = G.shift_rows(d["audio"].reshape(-1, 1), 2, 45, 1 + shift).astype(f); a0 = G.shift_rows(d["audio"].reshape(-1, 1), 2, 45, shift).astype(f)
        one = (d["b"].astype(f) + a1 * d["w"][0].astype(f)) + a0 * d["w"][1].astype(f)
        two = (a0 * d["w"][1].astype(f) + a1 * d["w"][0].astype(f)) + d["b"].astype(f)
        assert np.array_equal(one, x) and np.array_equal(two, x)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i", range(len(D.CASES)))
def test_weight_gradient_restatement_within_c_cpu(i, mode):
    """dWf's current tap summed row by row in float32 against the float64 contraction, on the restatement's df; and the
    tiles' operands are on their grids with every row and column covered."""
    dil, B, T, seg = D.CASES[i]
    R = 32
    d = D.wt_design(dil, B, T, R)
    for k, grid in (("x", D.GX), ("c", D.GC), ("audio", 1.0 / 16)):
        assert G.is_bf16(d[k]) and np.array_equal(d[k] / grid, np.rint(d[k] / grid))
    for k in ("x", "c"):
        assert np.abs(d[k]).sum(1).min() > 0 and np.abs(d[k]).sum(2).min() > 0
    df32, G32 = D.restate_chain(d, mode)
    worst = 0.0
    for l in range(len(dil)):
        val, S, _ = D.wgrad_refs(d, l, None, df32[l], np.zeros_like(df32[l]))["dWf"]
        x, dfl = d["x"][l].astype(np.float32), df32[l].astype(np.float32)
        acc = np.zeros((R, R), np.float32)
        for t in range(B * T):
            acc += x[t][:, None] * dfl[t][None, :]
        r = np.where(S[1] > 0, np.abs(acc - val[1]) / np.maximum(D.wgrad_scale(S[1], B * T, 0.0), 1e-300), 0.0)
        worst = max(worst, float(r.max()))
    _say("weight gradient %s %s: worst error / scale %.3f (C_CPU %g)" % (D.CASES[i], mode, worst, D.C_CPU_WGRAD))
    assert worst <= D.C_CPU_WGRAD


def test_exact_corner_of_the_weight_gradients_is_in_range():
    """g_top = None, z = 0, Wr_top = 0: df_top = dcs / 2, G_top = its taps; the sums x^T df_top, c^T G_top and the column
    sums stay below 2^22 units of their product grids in every case."""
    for dil, B, T, seg in D.CASES:
        for blocks in (False, True):
            d = D.wt_design(dil, B, T, 64, exact_corner=True, blocks=blocks)
            D.check_design(d)
            n = len(dil)
            assert n > 1 and not d["wr"][n - 1].any()
            df, t, units = D.exact_top(d)
            assert units.max() < G.S_MAX
            refs = D.wgrad_refs(d, n - 1, None, df, np.zeros_like(df))
            uf, ur = D.GX * 0.5 * D.GD, D.GC * 0.5 * D.GD * G.GW
            assert refs["dWf"][1].max() / uf < G.S_MAX and refs["dbf"][1].max() / (0.5 * D.GD) < G.S_MAX
            below = D.wgrad_refs(d, n - 2, D.round_to(t, "bf16"), df, np.zeros_like(df))
            assert below["dWr"][1].max() / ur < G.S_MAX and below["dbr"][1].max() / (0.5 * D.GD * G.GW) < G.S_MAX
            for k in ("dWf", "dWr"):      # every value is on its product grid: the float64 contraction is exact
                v, u = (refs[k][0], uf) if k == "dWf" else (below[k][0], ur)
                assert np.array_equal(v / u, np.rint(v / u))
            if blocks:                    # most sums stay within what a bf16 partial holds exactly, and none is empty
                assert (refs["dWf"][1] / uf <= G.S_MAX16).mean() >= 0.5 and (below["dWr"][1] / ur <= G.S_MAX16).mean() >= 0.5
                assert np.abs(d["x"]).sum(1).min() > 0 and np.abs(d["c"]).sum(1).min() > 0


@pytest.mark.parametrize("i,R,variant", D.RUNS)
def test_wt_design_keeps_the_cap_without_a_stored_df(i, R, variant):
    """srwn_residual_group_bwd_wt stores G only: with df reconstructed, a G entry is decided only if every df entry it
    reads is.  bf16 mode: still at least 90 % of every layer's G, no row or column wholly undecided, and the restatement
    agrees bit for bit there and stays within the widened bound elsewhere."""
    dil, B, T, seg = D.CASES[i]
    d = D.wt_design(dil, B, T, R, variant)
    D.check_design(d)
    for l in range(len(dil)):
        for k in range(2):
            assert np.abs(d["wf"][l, k]).sum(0).min() > 0 and np.abs(d["wf"][l, k]).sum(1).min() > 0
    df32, G32 = D.restate_chain(d, "bf16")
    Gup = d["g_top"]
    for l in range(len(dil) - 1, -1, -1):
        rdf, udf, rG, extra, dec = D.wt_layer_refs(d, l, Gup, "bf16")
        assert dec.mean() >= D.CAP and dec.any(0).all() and dec.any(1).all(), (D.CASES[i], R, variant, l, dec.mean())
        assert G.same_bits(G32[l], rG["ref"])[dec].all()
        assert (np.abs(G32[l] - rG["x"]) <= D.bound(rG, "bf16", D.C_GPU["G"]["bf16"]) + extra).all()
        Gup = G32[l]
