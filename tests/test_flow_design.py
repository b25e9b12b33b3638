"""CPU checks of tests/flow_design.py: the range conditions that make each design exact (asserted where the design is
formed), the exactness claim itself (float32 in two orders against the float64 reference, bit for bit), the rounding ties of
the bf16 gradient, each reference against the independent oracle where oracle/ has one, and the figures the per-entry bounds'
constants come from.  No GPU, no import of the product."""
import os

import numpy as np
import pytest

from oracle import wavenet_np as O
from tests import flow_design as D
from tests import gemm_design as G


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _same(got, want):
    assert G.same_bits(got, want).all()


# ---- flow head ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", D.FLOW_RS)
def test_flow_fwd_designs_are_exact_where_they_claim(R):
    """Forming a design asserts its range conditions; here: float32 sums in two orders equal prm and the per-block entropy
    partials bit for bit, the exact design's x_out too, and the designs hold what they promise (p0 = 0; p0 non-zero,
    inside [-80, 80], with the overflow stratum; every kind of h)."""
    f = np.float32
    strata = 0
    for rows in D.FLOW_ROWS:
        for general in (False, True):
            d = D.flow_fwd(rows, R, general)
            a, w2 = D.relu(d["h"]).astype(f), d["w2"].astype(f)
            one = np.zeros((rows, 2), f)
            for c in range(R):
                one = D.fma32(a[:, c:c + 1], w2[c:c + 1], one)
            two = np.zeros((rows, 2), f)
            for c in list(range(8, R))[::-1] + list(range(8)):
                two += a[:, c:c + 1] * w2[c:c + 1]
            b2 = d["b2"].astype(f)
            _same(one + b2, d["prm"]); _same(two + b2, d["prm"])
            p0 = d["prm"][:, 0].astype(f)
            ent = np.array([p0[s:s + 256][::-1].sum(dtype=f) for s in range(0, rows, 256)])      # (pairwise, reversed)
            seq = np.array([np.cumsum(p0[s:s + 256], dtype=f)[-1] for s in range(0, rows, 256)])
            _same(ent, d["ent"]); _same(seq, d["ent"])
            assert d["ent"].shape == (-(-rows // 256),)
            h = d["h"]
            assert (h < 0).any() and ((h == 0) & np.signbit(h)).any() and (h > 0).any()
            if general:
                strata += int(d["inf_rows"].sum())
                assert rows < 33 or d["inf_rows"].any()
                assert np.isinf(d["x_out"][d["inf_rows"]]).all() and np.isfinite(d["x_out"][~d["inf_rows"]]).all()
                assert (np.sign(d["x_out"][d["inf_rows"]]) == np.sign(d["x_in"][d["inf_rows"]])).all()
                assert (d["prm"][:, 0] != 0).mean() > 0.9
                if rows >= 255:
                    p = d["prm"][~d["inf_rows"], 0]
                    assert p.min() < -60 and p.max() > 60 and (np.abs(p) < 10).any()
                    assert (d["ent"] != 0).all()
            else:
                assert ((h == 0) & ~np.signbit(h)).any()
                _same(D.flow_fwd32(d), d["x_out"])
                assert (d["ent"] == 0).all() and (d["prm"][:, 1] != 0).any()
    assert strata > 100


@pytest.mark.parametrize("R", D.FLOW_RS)
def test_flow_bwd_exact_design_is_exact_and_meets_rounding_ties(R):
    nt = nr = n = ntr = 0
    for rows in D.FLOW_ROWS:
        for eg in D.ENT_GRADS:
            d = D.flow_bwd(rows, R, False, eg)
            assert (d["prm"][:, 0] == 0).all() and (d["prm"][:, 1] == D.PRM1_JUNK).all() and d["exact_cols"].all()
            for mode in ("fp32", "bf16"):
                g, dx_in, wp = D.flow_bwd32(d, eg, mode)
                _same(g, G.round_out(d["g"], mode)); _same(dx_in, d["dx_in"]); _same(wp, d["wp"])
            # another order of the block sums
            a = D.relu(d["h"])
            rev = D.block_sum((a * (d["dx_out"] * d["x_in"] + eg)[:, None])[::-1].astype(np.float32), 256)
            assert rows % 256 or G.same_bits(rev[::-1], d["wp"][:, 0:2 * R:2]).all()
            # g is exactly +0 wherever h <= 0 (zeros of both signs among them) and those entries add nothing
            assert (d["g"][~d["pos"]] == 0).all() and ((d["h"] == 0) & ~d["pos"]).any()
            t = G.ties(d["g"])
            nt += int(t.sum()); nr += int((G.round_out(d["g"], "bf16") != d["g"]).sum()); n += d["g"].size
            r = G.round_out(d["g"], "bf16")
            assert ((G.bf16_bits(r[t].astype(np.float32)) & 1) == 0).all()
            trunc = (np.ascontiguousarray(_f32(d["g"])).view(np.uint32) & 0xFFFF0000).view(np.float32)
            ntr += int((trunc != r).sum())
    _say("flow_bwd exact design, R %d: %d entries of g, %d bf16 ties, %d rounded, %d where truncation differs" % (R, n, nt, nr, ntr))
    assert nt >= 100 and nr >= n // 20 and ntr >= n // 40, (nt, nr, ntr, n)


def test_flow_references_equal_the_autodiff_of_the_oracle_head():
    """prm, x_out, the entropy term and the backward's g, dx_in and weight gradients of the DESIGNS against torch autograd
    in float64.  This is a restatement in torch of the last two lines of oracle/wavenet_torch.py's flow_forward (relu(h) @
    W2 + b2; x_in exp(prm0) + prm1; ent_grad on prm0), not a call of it: flow_forward derives h from x_in through the
    input conv, so it cannot be handed a designed h.  The test below calls the oracle itself."""
    import torch
    R, rows, eg = 32, 257, -0.25
    d = D.flow_fwd(rows, R, True)
    keep = ~d["inf_rows"]
    h = torch.tensor(d["h"][keep], dtype=torch.float64, requires_grad=True)
    w2 = torch.tensor(d["w2"], dtype=torch.float64, requires_grad=True)
    b2 = torch.tensor(d["b2"], dtype=torch.float64, requires_grad=True)
    x_in = torch.tensor(d["x_in"][keep], dtype=torch.float64, requires_grad=True)
    prm = torch.einsum("tr,rc->tc", torch.relu(h), w2) + b2            # oracle/wavenet_torch.py flow_forward, last lines
    x_out = x_in * torch.exp(prm[..., 0]) + prm[..., 1]
    assert np.allclose(prm.detach().numpy(), d["prm"][keep], rtol=0, atol=0)
    assert np.allclose(x_out.detach().numpy(), d["x_out"][keep], rtol=1e-14, atol=0)
    assert np.isclose(prm[:, 0].sum().item(), d["ent"].sum() - 89.0 * d["inf_rows"].sum(), rtol=1e-13)
    # backward: the design's own h, w2, prm, x_in, dx_out
    b = D.flow_bwd(rows, R, True, eg)
    h = torch.tensor(np.where(b["h"] == 0, 0.0, b["h"]), dtype=torch.float64, requires_grad=True)
    w2 = torch.tensor(b["w2"], dtype=torch.float64, requires_grad=True)
    # a bias that reproduces the designed prm on top of relu(h) @ w2: the autodiff sees the same prm0
    off = torch.tensor(b["prm"] - D.relu(b["h"]) @ b["w2"], dtype=torch.float64, requires_grad=True)
    x_in = torch.tensor(b["x_in"], dtype=torch.float64, requires_grad=True)
    prm = torch.relu(h) @ w2 + off
    x_out = x_in * torch.exp(prm[:, 0]) + prm[:, 1]
    loss = (x_out * torch.tensor(b["dx_out"])).sum() + eg * prm[:, 0].sum()
    loss.backward()
    tol = dict(rtol=1e-12, atol=0)
    assert np.allclose(h.grad.numpy(), b["g"], **tol)                  # (torch's relu passes no gradient at h = 0 either)
    assert np.allclose(x_in.grad.numpy(), b["dx_in"], **tol)
    gw = b["wp"][:, :2 * R].sum(0).reshape(R, 2)
    assert np.allclose(w2.grad.numpy(), gw, rtol=1e-9, atol=1e-9 * np.abs(gw).max())
    assert np.allclose(off.grad.numpy().sum(0), b["wp"][:, 2 * R:].sum(0), rtol=1e-9)


def test_flow_formulas_equal_the_autodiff_of_the_oracle_flow_forward():
    """oracle/wavenet_torch.py's flow_forward itself, on a flow without residual layers (input conv, then the head): its prm
    and x_out, and autograd's gradients of sum(dx_out x_out) + ent_grad sum(prm0), against the design file's formulas on
    the h the oracle's input conv gives -- head_w2 / head_b2 (the sums of w_partials), init_b (the column sums of g), and x_in
    (dx_in plus g carried back through the input conv by the NumPy oracle's _conv_backward)."""
    import torch
    from oracle import wavenet_torch as OT
    R, B, T, eg = 32, 3, 41, -0.25
    sp = O.init_flow_params(11, [], 2, R, R, 0, bias_scale=0.3)
    rng = np.random.default_rng(12)
    x = rng.normal(0, 1, (B, T)); dxo = rng.normal(0, 1, (B, T))
    st = OT.TorchStack(sp)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    scale, mean, x_out, prm = OT.flow_forward(st, xt, None, 1)
    (x_out * torch.tensor(dxo)).sum().add(eg * prm[..., 0].sum()).backward()
    xs = O.right_shift(x[:, :, None])
    h = O.dilated_causal_conv1d_bias(xs, sp.init_w, sp.init_b, 1).reshape(B * T, R)
    assert (h > 0).any() and (h < 0).any()
    prm_ref = D.relu(h) @ sp.head_w2 + sp.head_b2
    tol = dict(rtol=1e-10, atol=1e-12)
    assert np.allclose(prm.detach().numpy().reshape(-1, 2), prm_ref, **tol)
    assert np.allclose(x_out.detach().numpy().reshape(-1), x.reshape(-1) * np.exp(prm_ref[:, 0]) + prm_ref[:, 1], **tol)
    d0, d1, k0, g, dx_in = D.flow_bwd_formulas(h, sp.head_w2, prm_ref[:, 0], x.reshape(-1), dxo.reshape(-1), eg)
    a = D.relu(h)
    gw = np.stack([a.T @ d0, a.T @ d1], 1)
    assert np.allclose(st.head_w2.grad.numpy(), gw, **tol)
    assert np.allclose(st.head_b2.grad.numpy(), [d0.sum(), d1.sum()], **tol)
    assert np.allclose(st.init_b.grad.numpy(), g.sum(0), **tol)
    dxs, dw = O._conv_backward(xs, sp.init_w, 1, g.reshape(B, T, R))
    assert np.allclose(st.init_w.grad.numpy(), dw, **tol)
    assert np.allclose(xt.grad.numpy(), dx_in.reshape(B, T) + _advance_oracle(dxs, 1)[..., 0], **tol)
    assert (k0 >= np.abs(d0)).all()


def test_flow_bound_constants_are_the_measured_ones():
    """C_CPU: the worst ratio of the float32 NumPy restatement against float64 on the general designs, rounded up."""
    worst = {k: 0.0 for k in D.C_CPU}
    for R in D.FLOW_RS:
        for rows in D.FLOW_ROWS:
            d = D.flow_fwd(rows, R, True)
            keep = ~d["inf_rows"]
            got = D.flow_fwd32(d)
            assert np.array_equal(got[~keep], d["x_out"][~keep])
            worst["x_out"] = max(worst["x_out"], D.ratio(got[keep], d["x_out"][keep], d["x_scale"][keep]).max(initial=0))
            for eg in D.ENT_GRADS:
                b = D.flow_bwd(rows, R, True, eg)
                for mode in ("fp32", "bf16"):
                    g, dx_in, wp = D.flow_bwd32(b, eg, mode)
                    assert (g[~b["pos"]] == 0).all()
                    worst["g_" + mode] = max(worst["g_" + mode], D.ratio(g, b["g"], D.g_scale(b, mode)).max())
                    ex = b["exact_cols"]
                    _same(wp[:, ex], b["wp"][:, ex])
                    worst["w_partials"] = max(worst["w_partials"], D.ratio(wp[:, ~ex], b["wp"][:, ~ex], b["wp_scale"][:, ~ex]).max())
                    worst["dx_in"] = max(worst["dx_in"], D.ratio(dx_in, b["dx_in"], D.EPS * np.abs(b["dx_in"])).max())
    _say("float32 NumPy restatement, worst error / bound scale:", {k: round(float(v), 3) for k, v in worst.items()})
    for k, v in worst.items():
        assert np.isfinite(v) and v > 0, k
        # another NumPy build's exp (an ulp apart) may move a figure: the constant is the rounded-up one or the step above
        assert v <= D.C_CPU[k] <= G.rounded_up(v) + (1 / 16 if v < 1 else 0.5), (k, v, D.C_CPU[k])
        assert D.C_GPU[k] == 4 * D.C_CPU[k]


# ---- convolutions -------------------------------------------------------------------------------------------------------
def _advance_oracle(x, n):
    """The adjoint of oracle.right_shift."""
    out = np.zeros_like(x)
    if n < x.shape[1]:
        out[:, :x.shape[1] - n] = x[:, n:]
    return out


def _shifted(x, shift):
    """(the oracle's input of a conv with `shift`, the first output row that counts): right_shift for shift >= 0.  The
    kernels fold shift and tap into ONE offset and zero-fill once, so the non-causal shift < 0 is the causal conv of the
    clip with -shift zero rows appended, read from row -shift on."""
    if shift >= 0:
        return O.right_shift(x, shift), 0
    return np.concatenate([x, np.zeros((x.shape[0], -shift) + x.shape[2:])], 1), -shift


@pytest.mark.parametrize("shape", D.DGRAD_SHAPES)
def test_dgrad_reference_equals_the_oracle_and_is_order_free(shape):
    K, Cin, Cout = shape
    assert K * Cin * Cout * 4 <= 48 * 1024 and (shape != D.DGRAD_SHAPES[-1] or K * Cin * Cout * 4 == 48 * 1024)
    assert np.prod(D.DGRAD_REFUSED) * 4 > 48 * 1024
    for T in D.DGRAD_TS:
        d = D.dgrad(T, K, Cin, Cout)
        assert (np.abs(d["dy"][:, :2]) == 15 * D.GCW).all() and (T <= 2 or np.abs(d["dy"][:, 2:]).max() <= 3 * D.GCW)
        for dil in D.dilations(T):
            for shift in D.dgrad_shifts(T):
                ref = D.dgrad_ref(d, dil, shift, False)
                dx, _ = O._conv_backward(np.zeros((D.DGRAD_B, T, Cin)), d["w"], dil, d["dy"])
                assert np.array_equal(_advance_oracle(dx, shift), ref)          # y = conv(right_shift(x, shift))
                acc = D.dgrad_ref(d, dil, shift, True)
                assert np.array_equal(acc, d["dx0"] + 0.5 * ref)
                if Cin <= 3:
                    # float32, taps and channels in another order
                    f = np.float32
                    s = np.zeros(ref.shape, f)
                    for k in range(K):
                        for o in range(Cout)[::-1]:
                            s += D.delay(d["dy"], -(shift + (K - 1 - k) * dil))[..., o:o + 1].astype(f) * d["w"][k, :, o].astype(f)
                    _same(s, ref)
    assert D.dilations(1) == [1, 6] and D.dilations(256) == [1, 255, 256, 261]


def test_conv_fwd_reference_equals_the_oracle_and_covers_every_path():
    paths = set()
    for (B, T, Cin, Cout, K) in D.CONV_FWD:
        paths.add(D.conv_path(Cin, Cout, K))
        d = D.conv_fwd(B, T, Cin, Cout, K)
        for dil in D.conv_dilations(T):
            for shift in D.CONV_SHIFTS:
                for bias in (True, False):
                    ref = D.conv_fwd_ref(d, dil, shift, bias)
                    xs, first = _shifted(d["x"], shift)
                    got = O.dilated_causal_conv1d_bias(xs, d["w"], d["b"] if bias else None, dil)
                    assert np.array_equal(got[:, first:first + T], ref)
                    G.round_out(ref, "bf16")
        if Cout <= 64 and T <= 257:
            f = np.float32
            y = np.zeros(ref.shape, f)
            for k in range(K)[::-1]:
                y += D.delay(d["x"], (K - 1 - k) * dil + shift).astype(f) @ d["w"][k].astype(f)
            _same(y, ref)
    assert paths == {"cin1_k2", "cin1_any", "generic"}
    rows8 = [B * T for (B, T, Cin, Cout, K) in D.CONV_FWD if Cout == 8]
    assert 2049 in rows8 and 9 in [B * T for (B, T, Cin, Cout, K) in D.CONV_FWD if Cout == 2048]
    assert any(Cout == 24 for (_, _, _, Cout, _) in D.CONV_FWD) and any(Cout == 10 for (_, _, _, Cout, _) in D.CONV_FWD)
    # bf16 outputs round, and meet ties
    d = D.conv_fwd(1, 257, 1, 64, 3)
    ref = D.conv_fwd_ref(d, 1, 0, True)
    assert G.ties(ref).sum() >= 20 and (G.round_out(ref, "bf16") != ref).sum() > ref.size // 20


@pytest.mark.parametrize("clip", [c for c in D.IC_CLIPS if c[0] * c[1] <= 1000])
def test_init_conv_wgrad_reference_equals_the_oracle(clip):
    B, T = clip
    R = 32
    ic = D.init_conv(B, T, R)
    assert (np.abs(ic.audio[:, 0]) == 15 * D.GCX).all() and (np.abs(ic.audio[:, -1]) == 15 * D.GCX).all()
    for K in D.IC_KS:
        for shift in (-1, 0, 1):
            p = ic.partials(K, shift)
            assert p.shape == (-(-B * T // 256), K + 1, R)
            x = ic.audio[..., None]
            xs, first = _shifted(x, shift)
            gp = np.concatenate([np.zeros((B, first, R)), ic.g], 1)
            _, dw = O._conv_backward(xs, np.zeros((K, 1, R)), 1, gp)
            assert np.array_equal(p.sum(0)[:K], dw[:, 0, :])
            assert np.array_equal(p.sum(0)[K], ic.g.sum((0, 1)))
            # float32, rows in reverse
            f = np.float32
            k = K - 1
            xs32 = D.delay(x, shift).reshape(-1, 1).astype(f)[::-1]
            _same((xs32 * ic.g.reshape(-1, R).astype(f)[::-1]).sum(0, dtype=f), p.sum(0)[k])


def test_init_conv_wgrad_designs_cover_the_block_geometry():
    nparts = {c: -(-c[0] * c[1] // D.IC_BLOCK) for c in D.IC_CLIPS}
    assert nparts[(65, 256)] == 65 and nparts[(1, 16640)] == 65 and nparts[(6, 100)] == 3      # > 64 partials; mid-clip starts
    assert 256 % 100 and (2 * 256) % 100                           # blocks 1 and 2 of (6, 100) start inside a clip
    for R in D.IC_RS:                                               # 8192 (K + 1) bytes whatever R
        assert D.ic_lds(R, 7) == 65536 and D.ic_lds(R, D.IC_K_REFUSED) == 73728 and max(D.IC_KS) == 7
    for c in ((65, 256), (1, 16640)):                               # the range condition at the longest sums
        D.init_conv(c[0], c[1], 32).partials(7, 1)


# ---- clipping and the small kernels -------------------------------------------------------------------------------------
def test_sumsq_and_clip_scale_references():
    for n in D.SUMSQ_NS:
        d = D.sumsq(n)
        assert d["parts"].shape == (-(-n // D.SQ_CHUNK),)
        g = d["g"].astype(np.float32)
        got = [np.cumsum((g[s:s + 4096] * g[s:s + 4096])[::-1], dtype=np.float32)[-1] for s in range(0, n, 4096)]
        _same(np.array(got), d["parts"])
    kinds = set()
    for m in D.CLIP_COUNTS:
        for name, parts, clip, pre in D.clip_cases(m):
            scale, norm = D.clip_ref(parts, clip, pre)
            # the oracle clips the all-reduced mean: gradients pre_scale * g with sum g^2 = sum of the partials
            g = pre * np.sqrt(parts)
            clipped, gn = O.clip_by_global_norm([g], clip)
            assert np.float32(gn) == norm or abs(gn - norm) <= 2 ** -24 * norm
            s = clip / max(gn, clip)
            assert abs(scale - pre * s) <= 2 ** -23 * scale
            kinds.add(name)
            if name == "below":
                assert norm < clip and scale == pre
            elif name == "above":
                assert norm > clip and scale < pre
            elif name == "equal":
                assert norm == clip and scale == pre and parts.sum() == 4.0
            else:
                assert norm == 0 and scale == pre and np.isfinite(scale)
    assert kinds == {"below", "above", "equal", "zero"}


def test_small_kernel_designs():
    for n in D.POWER_NS:
        d = D.power(n)
        _same(D.power_dpow32(d), d["dpow"])
        diff = (d["pt"] - d["po"]).astype(np.float32)
        assert np.float32(D.POWER_GAMMA) * (diff * diff)[::-1].sum(dtype=np.float32) == d["loss"]
    for n in D.REDUCE_NS:
        d = D.reduce_loss(n)
        assert d["p"].shape == (n,) and np.float32(d["out"]) == d["out"]
    assert D.reduce_loss(0)["out"] == 0
    for n in D.AXPY_NS:
        d = D.axpy(n)
        for s in D.AXPY_SCALES:
            ref = d["y"] + D.AXPY_ALPHA * s * d["x"]
            _same(D.fma32(np.float32(D.AXPY_ALPHA) * np.float32(s), d["x"], d["y"]), ref)
    for lo, hi in D.CLAMP_BOUNDS:
        sp = D.clamp_specials(lo, hi)
        assert len(set(sp[:6].tolist())) == (6 if lo < hi else 3) and np.isinf(sp).sum() == 2
        for n in D.CLAMP_NS:
            d = D.clamp(n, lo, hi)
            assert d["y"].min() >= lo and d["y"].max() <= hi and (d["dy"] != 0).all()
            inside = (d["x"] >= lo) & (d["x"] <= hi)
            assert np.array_equal(d["dx"] != 0, inside)
            if n >= 255:
                assert inside.any() and (~inside).any() and (d["x"] == lo).any() and (d["x"] == hi).any()
