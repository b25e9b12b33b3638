"""CPU checks of tests/gemm_design.py: the range conditions that make a design exact, its coverage, its rounding ties, the
exactness claim itself (two float32 summation orders against the integer reference, bit for bit), the gate constants, the
tile encoder, and the figures the per-entry bounds' constants come from.  No GPU, no import of the product."""
import os

import numpy as np
import pytest

from tests import gemm_design as G

CASES = list(G.cases())


def test_every_design_meets_its_range_conditions_and_covers_its_operands():
    names = set()
    for name, a, w, b, ga, gw, bf16_out, part16, full in CASES:
        assert name not in names, name
        names.add(name)
        S = G.check_exact(a, w, b, ga, gw, part16)
        assert S.shape == (a.shape[0], w.shape[1])
        if full:
            G.check_cover(a, w)
        else:       # a shifted tap: its first `shift` rows of every clip are zero by design; the other operand is full
            assert np.abs(w).sum(1).min() > 0 and np.abs(w).sum(0).min() > 0, name
    assert len(CASES) > 100


def test_bf16_outputs_meet_rounding_ties():
    """Where the output is bf16 the exact reference must hit exact ties (nearest-even decides), and rounding must matter:
    a kernel that truncates, or rounds the bias in separately, differs."""
    fam = {}
    for name, a, w, b, ga, gw, bf16_out, part16, full in CASES:
        if not bf16_out:
            continue
        y, _ = G.contract(a, w, b)
        t = G.ties(y)
        k = name.split()[0]
        fam.setdefault(k, [0, 0, 0])
        fam[k][0] += int(t.sum())
        fam[k][1] += int((G.round_out(y, "bf16") != y).sum())
        fam[k][2] += y.size
        # ties resolve to even in the reference
        r = G.round_out(y, "bf16")
        assert ((G.bf16_bits(r[t].astype(np.float32)) & 1) == 0).all()
    assert set(fam) == {"rowgemm", "skipsum", "colgemm", "ychunks", "chain", "bwd", "tap"}
    for k, (nt, nr, n) in fam.items():
        assert nt >= 20 and nr >= n // 20, (k, nt, nr, n)


@pytest.mark.parametrize("part", range(4))
def test_float32_in_two_summation_orders_equals_the_integer_reference(part):
    """The exactness claim, without a GPU: every partial sum of an in-range design is an exact float32 number, so the
    order does not matter.  (A quarter of the designs per case.)"""
    for name, a, w, b, ga, gw, bf16_out, part16, full in CASES[part::4]:
        G.check_order_free(a, w, b, "fp32")
        if bf16_out:
            G.check_order_free(a, w, b, "bf16")


def test_an_out_of_range_design_is_not_order_free():
    """The check has teeth: operands exact in bf16 and on their grids, all of one sign, K = 4096 -- check_exact refuses the
    design at the range condition itself, and past 2^24 units the two summation orders really disagree."""
    a = np.abs(G.exact((4, 4096), 255, 1.0, 1))
    w = np.abs(G.exact((4096, 8), 255, 1.0, 2))
    assert G.is_bf16(a) and G.is_bf16(w) and (np.abs(a) @ np.abs(w)).min() > 2 ** 24
    with pytest.raises(AssertionError, match="not below 2\\^22"):
        G.check_exact(a, w, None, 1.0, 1.0)
    G.check_exact(a[:, :32], w[:32], None, 1.0, 1.0)           # the same operands, cut to an in-range K, are accepted
    assert not np.array_equal(G.eval32(a, w, None, range(4096)), G.eval32_blocked(a, w, None, 16))


def test_gate_constants_are_derived_and_clear_of_midpoints():
    g = G.gate_constants()
    assert g[0.0] == 0.0
    assert g[1.0] * 256 == 187 and g[-1.0] * 256 == -69          # what the derivation must arrive at
    z = np.array([-1.0, 0.0, 1.0])
    assert np.array_equal(G.gate_poly32(z), [g[-1.0], 0.0, g[1.0]])
    assert np.array_equal(G.gated(z), G.gate_poly32(z))
    # both products lie 5.9e-4 from the bf16 number they round to, and 1.4e-3 / 3.9e-4 from the nearest rounding midpoint:
    # hundreds of times the polynomial's error
    for z, mid in ((1.0, 1.363e-3), (-1.0, 3.87e-4)):
        v = float(G.gate64(z))
        assert abs(abs(v - g[z]) - 5.9e-4) < 1e-5
        assert abs(G.midpoint_distance(v) - mid) < 1e-6 and mid > 100 * G.POLY_ERR
    # the polynomial restatement against the fp64 sigmoid on [-1, 1]: inside the header's quoted error
    x = np.linspace(-1, 1, 2001).astype(np.float32)
    err = np.abs(G.sigmoid_poly32(x).astype(np.float64) - 1 / (1 + np.exp(-x.astype(np.float64)))).max()
    assert err < 1.2 * G.POLY_ERR, err


def test_rounding_helpers():
    x = np.array([1.0, 1.00390625, 1.01171875, 257.0, 259.0, -257.0, 0.0, 3.0e-3], np.float64)
    r = G.bf16_round(x.astype(np.float32).astype(np.float64))
    assert r[:6].tolist() == [1.0, 1.0, 1.015625, 256.0, 260.0, -256.0]
    assert G.ties(x[:6]).tolist() == [False, True, True, True, True, True]
    assert G.same_bits(np.array([0.0, 1.0, np.nan]), np.array([-0.0, 1.0, np.nan])).tolist() == [True, True, False]
    import torch
    v = np.random.default_rng(0).standard_normal(10000).astype(np.float32)
    assert np.array_equal(G.bf16_round(v.astype(np.float64)), torch.tensor(v).bfloat16().double().numpy())


def _decode_tiles(tiles, B, Tn, R, st, W):
    """The decoder of tests/test_gpu_group.py::test_skip_wgrad_from_tiles_equals_wgrad256, written out from that test (and
    from nothing in tests/gemm_design.py): element (c, kg, j) of tile k of segment (clip b, residue r, first position j0) is
    time r + st (j0 + 32 k + kordW(kg, j)); a tile = four fragments of 16 channels, each [kg][channel][j]."""
    kg, j = np.meshgrid(np.arange(4), np.arange(8), indexing="ij")
    kord = 16 * (kg >> 1) + 2 * (kg & 1) + (j >> 2) + 4 * (j & 3)
    J = -(-Tn // st); nsub = -(-J // W); KT = -(-W // 32)
    nseg = B * st * nsub
    t = tiles[:nseg * KT * R * 32].reshape(nseg, KT, R // 16, 4, 16, 8).transpose(0, 1, 2, 4, 3, 5)
    t = t.reshape(nseg, KT, R, 4, 8)
    c = np.full((B * Tn, R), np.nan)
    beyond = []
    for seg in range(nseg):
        b, rem = seg // (st * nsub), seg % (st * nsub)
        r, j0 = (rem, 0) if nsub == 1 else (rem // nsub, (rem % nsub) * W)
        Jr = (Tn - r + st - 1) // st
        wseg = min(Jr - j0, W)
        for k in range(KT):
            for q in range(4):
                for e in range(8):
                    pos = 32 * k + kord[q, e]
                    if pos < wseg:
                        row = b * Tn + r + st * (j0 + pos)
                        assert np.isnan(c[row]).all(), "a row in two tile elements"
                        c[row] = t[seg, k, :, q, e]
                    else:
                        beyond.append(t[seg, k, :, q, e])
    return c, np.array(beyond)


@pytest.mark.parametrize("B,T,st,W", [(2, 77, 1, 64), (2, 77, 4, 32), (1, 100, 32, 32), (2, 45, 4, 40), (3, 1, 1, 32)])
def test_tile_encoder_inverts_the_decoder(B, T, st, W):
    R = 64
    c = G.exact((B * T, R), 2, 0.7, B + T + st)
    tiles = G.ct_encode(c, B, T, R, st, W, 99.0)
    nseg, KT = G.ct_geometry(B, T, st, W)[:2]
    assert tiles.size == nseg * KT * R * 32
    back, beyond = _decode_tiles(tiles, B, T, R, st, W)
    assert np.array_equal(back, c)                    # every row of c sits in exactly one tile element
    assert (beyond == 99.0).all() and beyond.size + c.size == tiles.size


def _worst(name, r, out):
    out[name] = max(out.get(name, 0.0), float(np.max(r)))


def measured_ratios():
    """The float32 NumPy restatement against fp64 on the designs of the bounded GPU cases: worst error / bound scale."""
    out = {}
    fa = G.f_abs_gate32()
    for (L, R, S, rows) in G.SKIPSUM:
        d = G.skipsum(L, R, S, rows)
        z = G.skipsum_a(d["z"])
        ref, Sm = G.contract(G.gate64(z), d["w"], d["b"])
        got = G.eval32(G.gate32(z).astype(np.float64), d["w"], d["b"], range(L * R))
        _worst("skip_sum_gate_fp32", G.ratio(got, ref, Sm, L * R, "fp32", fa * np.abs(d["w"]).sum(0)), out)
    d = G.wgrad(64, 64, 2, 45, gate=True)
    for l, sh in enumerate(G.wgrad_shifts(45)):
        a64, w = G.wgrad_ops(G.gate64(d["x"][l]), d["dy"][l], 2, 45, sh)
        a32, _ = G.wgrad_ops(G.gate32(d["x"][l]).astype(np.float64), d["dy"][l], 2, 45, sh)
        ref, Sm = G.contract(a64, w)
        got = G.eval32(a32, w, None, range(90))
        _worst("wgrad_gate_fp32", G.ratio(got, ref, Sm, 90, "fp32", fa * np.abs(w).sum(0)), out)
    for (R, B, T, pool, ns) in G.LAYERS:
        d = G.layers(R, B, T, pool)
        for l in range(4):
            ref, Sm = G.contract(G.gate64(d["z"][l]).T, d["g"][l])
            got = G.eval32(G.gate32(d["z"][l]).astype(np.float64).T, d["g"][l], None, range(B * T))
            _worst("wgrad_gate_fp32", G.ratio(got, ref, Sm, B * T, "fp32", fa * np.abs(d["g"][l]).sum(0)), out)
    for (mode, cw, dw, L) in G.WIDE:
        for rows in G.WIDE_ROWS + [257]:
            if mode == "stack":
                d = G.wide(mode, cw, dw, L, rows)
                z = G.skipsum_a(d["a"])
                ref, Sm = G.contract(G.gate64(z).T, d["d"])
                got = G.eval32(G.gate32(z).astype(np.float64).T, d["d"], None, range(rows))
                _worst("wgrad_gate_fp32", G.ratio(got, ref, Sm, rows, "fp32", fa * np.abs(d["d"]).sum(0)), out)
    for rows in G.CHAIN_ROWS:
        d = G.chain(rows, 256)
        pre, r1, logits = G.chain_forward(d)
        dl = G.dlogits32(logits, d["tg"], 1.0 / rows, "bf16")
        ref, Sm, p = G.dlogits_ref(logits, d["tg"], 1.0 / rows)
        _worst("softmax_dlogits", G.ratio(dl, ref, Sm, 256, "bf16"), out)
        ref, Sm = G.contract(dl, d["w2"].T)
        da1 = G.bf16_round(G.eval32(dl, d["w2"].T, None, range(256)).astype(np.float64)) * (r1 > 0)
        _worst("chain_product", G.ratio(da1, ref * (r1 > 0), Sm, 256, "bf16"), out)
        ref, Sm = G.contract(da1, d["w1"].T)
        dtot = G.bf16_round(G.eval32(da1, d["w1"].T, None, range(256)).astype(np.float64)) * (d["r0"] > 0)
        _worst("chain_product", G.ratio(dtot, ref * (d["r0"] > 0), Sm, 256, "bf16"), out)
    for (R, B, T, dil) in G.FWD:
        d = G.fwd_layer(R, B, T, dil)
        f = G.fwd_pre(d, B, T, dil)
        for mode in ("fp32", "bf16"):
            z, h = G.fwd_restate32(d, f, mode)
            _worst("fwd_z", G.ratio(z, np.tanh(f), 0.0, 0, mode, G.f_abs_tanh(mode)), out)
            ref, Sm, fa = G.fwd_h_ref(d, f, mode)
            _worst("fwd_h", G.ratio(h, ref, Sm, R, mode, fa), out)
    for (R, S, B, T) in G.BWD_DOWN:
        d = G.bwd_down(R, S, B, T)
        dc, _ = G.contract(d["d"], d["ws"].T)
        for mode in ("fp32", "bf16"):
            got = (dc.astype(np.float32) * G.dgate32(d["z"], mode)).astype(np.float64)
            got = G.bf16_round(got) if mode == "bf16" else got
            _worst("bwd_df", G.ratio(got, dc * G.dgate64(d["z"]), 0.0, 0, mode, G.f_abs_dgate(mode) * np.abs(dc)), out)
    for C in G.HEAD_CLASSES:
        d = G.head(C)
        logits, _ = G.contract(d["x"], d["w"], d["b"])
        for dt in ("fp32", "bf16"):
            ref, Sm, p = G.dlogits_ref(logits, d["tg"], 1.0 / G.HEAD_ROWS)
            got = G.dlogits32(logits, d["tg"], 1.0 / G.HEAD_ROWS, dt)
            _worst("softmax_dlogits", G.ratio(got, ref, Sm, C, dt), out)
    return out


def test_bound_constants_come_from_the_float32_restatement():
    """C_CPU holds the measured worst ratios rounded up; the GPU tests assert 4 x them."""
    m = measured_ratios()
    if os.environ.get("SRWN_PRINT_ERR") == "1":
        print("\nfloat32 restatement, worst error / bound scale:", {k: round(v, 3) for k, v in m.items()})
    assert set(m) == set(G.C_CPU)
    for k, v in m.items():
        assert 0 < v and G.C_CPU[k] == G.rounded_up(v), (k, v, G.C_CPU[k])      # the next 1/16 below 1, the next half above
        assert G.C_GPU[k] == 4 * G.C_CPU[k]
    assert 0 < G.f_abs_gate32() < 8 * G.EPS
