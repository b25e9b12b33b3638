"""CPU checks of tests/wngate_design.py: the range conditions that make the gate kernels' designs exact, their coverage,
the bit-count condition of the DOWN products, the saturation design's reach and finiteness, and the figures the per-entry
bounds' constants come from.  No GPU, no import of the product."""
import os

import numpy as np
import pytest

from tests import gemm_design as G
from tests import wngate_design as W


def test_every_exact_contraction_meets_its_range_conditions_and_covers_its_operands():
    names = set()
    for name, a, w, b, ga, gw, live in W.cases():
        assert name not in names, name
        names.add(name)
        S = G.check_exact(a, w, b, ga, gw)
        assert S.shape == (a.shape[0], w.shape[1])
        if live is None:       # a shifted tap of the weight gradient: its first rows are zero by design; dy is full
            assert np.abs(w).sum(1).min() > 0 and np.abs(w).sum(0).min() > 0, name
        elif name.startswith("wgrad"):
            G.check_cover(a, w)
        else:                  # every tap inside the clip is covered; one outside it contributes exact zeros
            G.check_cover(a[:, live], w[live])
            dead = np.setdiff1d(np.arange(a.shape[1]), live)
            assert not a[:, dead].any(), name
    assert len(names) > 300


@pytest.mark.parametrize("part", range(4))
def test_float32_in_two_summation_orders_equals_the_integer_reference(part):
    """The exactness claim without a GPU, on the designs of up to a few thousand rows (a quarter per case)."""
    small = [c for c in W.cases() if c[1].shape[0] * c[1].shape[1] <= 1 << 20 and not c[0].startswith("wgrad")]
    for name, a, w, b, ga, gw, live in small[part::4]:
        G.check_order_free(a, w, b, "fp32")
        if name.startswith("bwd"):
            G.check_order_free(a, w, b, "bf16")


def test_clip_edges_hold_the_top_of_the_range_inside_the_exactness_condition():
    for (R, B, T, dil) in W.FWD:
        if B < 2:
            continue
        x = W.fwd(R, B, T, dil)["x"].reshape(B, T, R)
        assert (np.abs(x[:-1, -1]) == 4).all() and (np.abs(x[1:, 0]) == 4).all() and np.abs(x).max() == 4
        D = W.bwd_up(R, B, T, dil)["D"].reshape(B, T, 2 * R) / W.GA
        assert (np.abs(D[:-1, -1]) == 15).all() and (np.abs(D[1:, 0]) == 15).all() and np.abs(D).max() == 15
        assert np.abs(D[:, 2:T - 2]).max() <= 3
    for (R, B, T, dil) in W.FWD:      # (the first and last row of every clip carry no zero: a tap at d = T - 1 has a term)
        assert np.abs(W.fwd(R, B, T, dil, sat=True)["x"].reshape(B, T, R)[:, [0, -1]]).min() >= 1


def test_down_products_meet_the_bit_count_condition():
    worst = 0
    for (R, S, B, T) in W.DOWN + [(W.BIG[0], W.BIG_S, W.BIG[1], W.BIG[2])]:
        d = W.bwd_down(R, S, B, T)
        for form in W.SKIP_FORMS:
            dc = W.down_dc(d, form)
            worst = max(worst, W.down_bits(dc, d["z"], d["s"]))
            assert G.is_bf16(d["dcs"])
            # the claim itself: float32 in two associations equals float64, bit for bit
            f = np.float32
            dc32, z, s = dc.astype(f), d["z"].astype(f), d["s"].astype(f)
            ref = W.down_D(dc, d["z"], d["s"])
            one = np.concatenate([dc32 * s * (f(1) - z * z), dc32 * z * s * (f(1) - s)], 1)
            two = np.concatenate([dc32 * (s * (f(1) - z * z)), (dc32 * z) * (s * (f(1) - s))], 1)
            assert np.array_equal(one.astype(np.float64), ref) and np.array_equal(two.astype(np.float64), ref)
            G.round_out(ref, "bf16")
        for v in W.DOWN_Z:
            assert (d["z"] == v).any() or B * T * R < 64
        for v in W.DOWN_S:
            assert (d["s"] == v).any() or B * T * R < 64
    assert 16 <= worst <= 24


def test_saturation_design_reaches_both_overflow_points_and_stays_finite():
    seen = {k: set() for k in ("f", "g")}
    for sat in (False, True):
        for (R, B, T, dil) in W.FWD + [W.BIG]:
            d = W.fwd(R, B, T, dil, sat)
            f, g = W.fwd_pre(d, B, T, dil, sat)
            for mode in W.MODES:
                z, s, c = W.fwd_gate32(f, g, mode)
                for v in (z, s, c, np.tanh(f), W.sigmoid64(g)):
                    assert np.isfinite(v).all()
                assert np.abs(z).max() <= 1 and s.min() >= 0 and s.max() <= 1
                assert (z[f == 0] == 0).all()
            if sat:
                for k, v in (("f", f), ("g", g)):
                    for name, m in (("zero", v == 0), ("small", (v != 0) & (np.abs(v) <= 2.25)), ("+48", (v > 44.4) & (v < 88.7)),
                                    ("-48", (v < -44.4) & (v > -88.7)), ("+96", v > 88.7), ("-96", v < -88.7)):
                        if m.any():
                            seen[k].add(name)
                if B * T >= 31:     # every shape but the single row reaches every range on both sides
                    assert (np.abs(f) > 88.7).any() and (np.abs(g) > 88.7).any() and (f == 0).any()
    for k in seen:
        assert seen[k] == {"zero", "small", "+48", "-48", "+96", "-96"}, (k, seen[k])


def test_conditioned_designs_do_not_divide_the_clip():
    assert W.FWD_COND
    for (R, B, T, dil) in W.FWD_COND:
        d = W.fwd(R, B, T, dil, cond=True)
        assert d["frames"] * W.POOL > T and T % W.POOL and d["cond"].shape == (B, d["frames"], 3 * R)
        assert (d["cond"][:, :, R:] == 64).all() and np.abs(d["cond"][:, :, :R]).max() <= 0.75
        assert np.abs(W.cond_rows(d, B, T)).sum(1).min() > 0


def _worst(out, key, mode, r):
    assert np.isfinite(r).all(), key
    out[key][mode] = max(out[key][mode], float(np.max(r)))


def measured_ratios():
    """The float32 NumPy restatements against float64 on the designs of the bounded GPU cases: worst error / bound scale."""
    out = {k: {m: 0.0 for m in W.MODES} for k in W.C_CPU}
    for mode in W.MODES:
        for sat in (False, True):
            for cond, shapes in ((False, W.FWD + [W.BIG]), (True, W.FWD_COND)):
                for (R, B, T, dil) in shapes:
                    d = W.fwd(R, B, T, dil, sat, cond)
                    f, g = W.fwd_pre(d, B, T, dil, sat)
                    z, s, c = W.fwd_gate32(f, g, mode)
                    _worst(out, "wn_z", mode, G.ratio(z, np.tanh(f), 0.0, 0, mode, W.f_abs_z(mode, sat)))
                    _worst(out, "wn_s", mode, G.ratio(s, W.sigmoid64(g), 0.0, 0, mode, W.f_abs_s(mode, sat)))
                    _worst(out, "wn_c", mode, G.ratio(c, np.tanh(f) * W.sigmoid64(g), 0.0, 0, mode, W.f_abs_c(mode, sat)))
                    ref, Sm = W.h_ref(d, c, B, T)
                    _worst(out, "wn_h", mode, G.ratio(W.h_restate32(d, c, B, T, mode), ref, Sm, R, mode))
        for (R, B, T, dil) in W.BWD_UP:
            up = W.bwd_up(R, B, T, dil)
            ref, Sm, K = W.g2_gin_ref(up, B, T, dil)
            _worst(out, "wn_g2_gin", mode, G.ratio(W.g2_gin_restate32(up, B, T, dil, mode), ref, Sm, K, mode))
            dn = W.bwd_down(R, 2 * R, B, T)
            for form in W.SKIP_FORMS:
                Gx, ref, Sm, K = W.updown_ref(up, dn, B, T, dil, form, mode)
                _worst(out, "wn_D", mode, G.ratio(W.updown_restate32(up, dn, B, T, dil, form, mode), ref, Sm, K, mode))
    return out


def test_bound_constants_come_from_the_float32_restatement():
    """C_CPU holds the measured worst ratios rounded up; the GPU tests assert 4 x them."""
    m = measured_ratios()
    if os.environ.get("SRWN_PRINT_ERR") == "1":
        print("\nfloat32 restatement, worst error / bound scale:", {k: {q: round(v, 3) for q, v in c.items()} for k, c in m.items()})
    assert set(m) == set(W.C_CPU)
    for k, c in m.items():
        for mode, v in c.items():
            assert 0 < v and W.C_CPU[k][mode] == G.rounded_up(v), (k, mode, v, W.C_CPU[k][mode])
            assert W.C_GPU[k][mode] == 4 * W.C_CPU[k][mode]
    for mode in W.MODES:
        for sat in (False, True):
            assert 0 < W.f_abs_z(mode, sat) < 8 * G.EPS and 0 < W.f_abs_s(mode, sat) < 8 * G.EPS
