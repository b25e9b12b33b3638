"""CPU checks of tests/serve_design.py: the range and cover conditions that make the chained head design exact stage by
stage, its zeros, ties and shares, the order-freedom of the hop sums, the exactness of the entry, window and match designs,
and the figures the per-entry bounds' constants come from.  No GPU, no import of the product."""
import os

import numpy as np
import pytest

from tests import gemm_design as G
from tests import serve_design as D

HEAD_ROWS = 2 * (2 * 96 + 3)          # the largest buffer of the pooled head's GPU cases


def _pooled_designs():
    for (R, S) in D.WIDTHS:
        for L in (1, 3):
            for hop in D.HOPS:
                yield D.head(L, R, S, 2 * (2 * hop + 3))


def _score_designs():
    for (R, S) in D.WIDTHS:
        for C in (D.SCORE_C if (R, S) == (32, 128) else (256, 100)):
            for (B, n) in D.SCORE_CLIPS:
                yield D.head(3, R, S, B * n, C)


def _mol_designs():
    for M in D.MOL_M:
        for (B, n) in D.MOL_CLIPS:
            yield D.head(3, 32, 128, B * n, 4 * M)


def test_every_stage_of_the_chained_design_is_exact_on_its_own_grid_and_covered():
    worst = {}
    n = 0
    for d in list(_pooled_designs()) + list(_score_designs()) + list(_mol_designs()) + [D.head(5, 64, 256, HEAD_ROWS, 256)]:
        for name, a, w, b, ga, gw in D.head_stages(d):
            S = G.check_exact(a, w, b, ga, gw)
            worst[name] = max(worst.get(name, 0), S.max())
            assert np.abs(w).sum(1).min() > 0 and np.abs(w).sum(0).min() > 0, name      # every k and column has a weight
            if a.shape[0] >= 31:
                G.check_cover(a, w)
            n += 1
        r1 = D.head_ref(d, "bf16")[0]
        assert np.abs(r1).sum(0).max() / (D.GW * D.GW / 256) < 2 ** 24          # any hop's sum is order-free
    assert n > 300 and max(worst.values()) < G.S_MAX
    if os.environ.get("SRWN_PRINT_ERR") == "1":
        print("\nlargest S per stage (units):", worst)


def test_relu_zeros_and_ties_at_zero():
    for d in _pooled_designs():
        stages = D.head_stages(d)
        for name, a, w, b, ga, gw in stages[:2]:
            pre = a @ w + b
            rows = pre.shape[0]
            assert ((pre == 0).sum(0) >= 1).all(), name                         # a tie at 0 in every column
            if rows >= 31:
                share = (pre <= 0).mean()
                assert 0.25 < share < 0.45, (name, share)


def test_float32_in_two_summation_orders_equals_the_integer_reference():
    for d in (D.head(3, 32, 128, 2 * (2 * 33 + 3)), D.head(3, 64, 256, 66, 100), D.head(1, 32, 256, 45, 256)):
        for name, a, w, b, ga, gw in D.head_stages(d):
            G.check_order_free(a, w, b, "fp32")
            if name != "w2":
                G.check_order_free(a, w, b, "bf16")


def test_hop_sums_are_order_free_and_the_butterfly_is_what_the_header_says():
    for hop in D.HOPS:
        x = D.hopsum(6, hop, 3, 1, "dyadic", "fp32")[:, :3 * hop].reshape(1, 3, hop, 6)
        assert np.array_equal(D.hop_sum32(x).astype(np.float64), x.sum(2))
        g = D.hopsum(6, hop, 3, 1, "gauss", "fp32")[:, :3 * hop].reshape(1, 3, hop, 6)
        h = D.hop_sum32(g).astype(np.float64)
        assert np.abs(h - g.sum(2)).max() < 64 * G.EPS * np.abs(g).sum(2).max()
    v = np.random.default_rng(1).normal(size=(5, 32)).astype(np.float32)
    want = v.copy()
    for s in (1, 2, 4, 8, 16):
        want = want + want[:, np.arange(32) ^ s]
    assert np.array_equal(D.butterfly32(v), want[:, 7])                         # every lane ends with the same bits


def test_score_design_ties_shares_and_gap_classes():
    for d in _score_designs():
        C, rows = d["C"], d["z"].shape[1]
        r1, _, lg, _ = D.head_ref(d, "bf16")
        assert not d["w2"][:, C:].any() and not d["b2"][C:].any()
        assert np.array_equal(np.sort(np.concatenate([np.ravel(p) for p in d["pairs"]] or [[]])),
                              np.unique(np.concatenate([np.ravel(p) for p in d["pairs"]] or [[]])))
        best, gap = D.top_gap(lg, d["pairs"])
        if C >= 2:
            assert d["pairs"] and d["pairs"][0][1] - d["pairs"][0][0] == 1
        if C >= 12:
            assert len(d["pairs"]) == 2 and d["pairs"][1][1] - d["pairs"][1][0] == 8
        for (c0, c1) in d["pairs"]:
            assert np.array_equal(lg[:, c0], lg[:, c1])
            if rows >= 31 and C > 2:
                assert (best == c0).mean() >= 0.1, (C, rows, c0, (best == c0).mean())
            assert not (best == c1).any()                                      # the lowest index wins
        tg = np.clip(D.codes(d), 0, C - 1)
        if rows >= 31 and C >= 7:
            assert len(np.unique(tg)) >= min(C, rows) // 2
            assert (best == tg).mean() < 0.5
            assert (D.codes(d) == -1).sum() == 1 and (D.codes(d) == C).sum() == 1
            assert lg.max() - lg.min() > 2.0 and np.abs(lg).max() < 64          # a trained head's spread, not a flat softmax
        # fp32 mode: at least 90 % of the rows have a top-two gap above twice the logits bound (on the reference alone)
        _, _, lg32, e2 = D.head_ref(d, "fp32")
        best32, gap32 = D.top_gap(lg32, d["pairs"])
        c = D.C_GPU["score_logits_fp32"]["fp32"]
        bound = c * (D.EPS * np.abs(lg32) + e2).max(1)
        if C > 2:
            assert (gap32 > 2 * bound).mean() >= 0.9, (C, rows)


def test_entry_window_roll_and_match_designs():
    for R in (32, 64):
        e = D.entry(R)
        a = D.audio((200,), R)
        assert np.abs(a).max() == D.A_TOP and np.abs(a).min() > 0
        for mode in D.MODES:
            D.entry_ref(e, a[:-1], a[1:], mode)
    for (hop, nW) in D.WINDOWS:
        win = hop * nW
        ring = D.ringrows(1, nW + 2, 100)[0]
        tot = np.stack([D.window_sum(ring, nW + j, nW) for j in range(6)])
        m = D.mean32(tot, win)
        if D.pow2(win):
            assert np.array_equal(m, tot / win)
            for C in D.WM_C:
                h = D.wm_head(100, C, C + 3)
                G.check_exact(m, h["w2"][:, :C], h["b2"], 0.25 / win, D.GW)
                G.check_cover(m, h["w2"][:, :C])
                assert np.array_equal(D.fma_chain32(m, h["w2"][:, :C], h["b2"]), m @ h["w2"][:, :C] + h["b2"])
                assert np.abs(h["w2"][:, C:]).min() >= 128
        assert not D.window_sum(ring, nW - 2, nW).any() or nW == 1
    v = D.roll_values(3, 2, 1203, 64)
    assert len(np.unique(v)) == v.size and np.array_equal(v.astype(np.float32).astype(np.int64), v)
    b = D.roll_bits16(v)
    assert (b > 0).all() and (b < 0x7F80).all() and (b[:, :, 1:] != b[:, :, :-1]).all() and (b[..., 1:] != b[..., :-1]).all()
    for Dm in D.MATCH_D:
        d = D.match(Dm)
        dist, near, dmin = D.match_ref(d["emb"], d["gal"], D.MAX_GALLERY)
        assert dist[0, 2] == D.SQRT_EPS and near[0] == 2 and dist[0, 3] == dist[0, 6] == D.SQRT_EPS
        assert near[1] == 8 and (dist[1, 8:12] == dmin[1]).all() and (np.delete(dist[1], range(8, 12)) > dmin[1]).all()
        assert near[2] == 69 and dist[2, 71] == dmin[2]
        assert D.match_ref(d["emb"], d["gal"], 70)[1][2] == 69
        assert D.match_ref(d["emb"], d["gal"], 0)[1][0] == -1


def measured_ratios():
    """The float32 NumPy restatements against float64 on the designs of the bounded GPU cases: worst error / bound scale."""
    out = {k: {m: 0.0 for m in c} for k, c in D.C_CPU.items()}

    def worst(key, mode, r):
        assert np.isfinite(r).all(), key
        out[key][mode] = max(out[key][mode], float(np.max(r)))

    for (R, S) in D.WIDTHS:
        for L in (1, 3):
            for hop in D.HOPS:
                B, k, mc = 2, 2, 2 * hop + 3
                d = D.head(L, R, S, B * mc)
                r1, e1, _, _ = D.head_ref(d, "fp32")
                got = D.hop_sum32(D.hop_rows(D.head_restate32(d, "fp32")[0], B, k, hop, mc))
                worst("pooled_ring_fp32", "fp32", D.ratio(got, D.hop_rows(r1, B, k, hop, mc).sum(2), D.hop_rows(e1, B, k, hop, mc).sum(2)))
    for d in _score_designs():
        C = d["C"]
        for mode in D.MODES:
            r1, e1, lg, e2 = D.head_ref(d, mode)
            lg32 = D.head_restate32(d, mode)[1]
            if mode == "fp32":
                worst("score_logits_fp32", "fp32", D.ratio(lg32, lg, e2))
            else:
                assert np.array_equal(lg32, lg)
            ref, m, lc, ls = D.nll64(lg32, D.codes(d))
            worst("score_nll", mode, D.ratio(D.nll32(lg32, D.codes(d)), ref, D.nll_scale(ref, m, lc, ls, C) - D.EPS * np.abs(ref)))
    for (hop, nW) in D.WINDOWS:
        win = hop * nW
        if D.pow2(win):
            continue
        for S in D.WM_S:
            ring = D.ringrows(2, nW + 2, S)
            m = np.stack([D.mean32(D.window_sum(ring[b], nW + 1 + b, nW), win) for b in range(2)])
            for C in D.WM_C:
                h = D.wm_head(S, C, C + 3)
                ref, Sm = G.contract(m, h["w2"][:, :C], h["b2"])
                worst("window_logits", "fp32", D.ratio(D.fma_chain32(m, h["w2"][:, :C], h["b2"]), ref, S * D.EPS * Sm))
    return out


def test_bound_constants_come_from_the_float32_restatement():
    """C_CPU holds the measured worst ratios rounded up; the GPU tests assert 4 x them."""
    m = measured_ratios()
    if os.environ.get("SRWN_PRINT_ERR") == "1":
        print("\nfloat32 restatement, worst error / bound scale:", {k: {q: round(v, 4) for q, v in c.items()} for k, c in m.items()})
    assert set(m) == set(D.C_CPU)
    for k, c in m.items():
        for mode, v in c.items():
            assert 0 < v and D.C_CPU[k][mode] == G.rounded_up(v), (k, mode, v, D.C_CPU[k][mode])
            assert D.C_GPU[k][mode] == 4 * D.C_CPU[k][mode]
    assert 0 < G.f_abs_gate32() < 8 * G.EPS
