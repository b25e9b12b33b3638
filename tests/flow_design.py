"""Exact (dyadic) and general input designs for the Parallel-WaveNet student's own kernels (csrc/srwn_flow.hip) and for the
Cin = 1 input-conv kernels every model starts with (csrc/srwn_util.hip), their float64 references, the float32
restatements and the bound constants.  Host code only (NumPy); tests/test_flow_design.py proves the designs' conditions on
the CPU and tests/test_gpu_flow_entries.py holds the kernels to them.  The vocabulary is tests/gemm_design.py's: ``exact``,
``bf16_round``, ``round_out``, ``same_bits``, the 2^22-unit rule.

Dyadic designs.  Operands are small integers times a power of two (exact in bf16 where a kernel reads bf16).  Each
design states its proof obligation through ``units``: every partial sum of every order is an integer below 2^22 units
of the product grid, an exact float32 number, so the result does not depend on the FMA chain, the shuffle tree, the block
cut or the reduction order.  The reference is formed in float64 and rounded ONCE, nearest-even, to the output dtype; a
kernel must equal it bit for bit.

  flow_affine_fwd   "exact": w2[:, 0] = 0 and b2[0] = 0, so prm[:, 0] = 0 and expf gives exactly 1: prm, x_out and the
                    (zero) ent_partials are exact.  "general": p0 is exact too (dyadic h, w2, b2), non-zero, so prm and
                    every ent_partials[block] stay bit for bit; only x_out passes through expf.
  flow_affine_bwd   "exact": a DESIGNED prm with prm[:, 0] = 0 (prm[:, 1] = 64, never to be read), not the forward's
                    output.  g's values need up to 13 bits: the bf16 store rounds, and exact ties occur.  "general": the
                    columns of w_partials that carry dprm1 = dx_out stay exact.
  conv / wgrad      range-top values (15 where the rest is <= 3) on the first and last rows of every clip: a tap read
                    across a clip boundary shows.

General designs (what passes through expf).  p0 is exact and spread over [-80, 80]; in the forward every seventh row
holds p0 = 89 exactly, where expf overflows and x_out must be +-inf with the sign of x_in (x_in != 0 everywhere).
Per entry, with eps = 2^-24 and d0 = dx_out x_in e^p0 + ent_grad, k0 = |dx_out x_in| e^p0 + |d0|:

    x_out        |err| <= c eps (|x_in| e^p0 + |ref|)
    dx_in        |err| <= c eps |ref|
    g[row, c]    |err| <= c (u_out |ref| + eps (k0 |w2[c, 0]| + |dx_out w2[c, 1]|))        (exactly 0 where h <= 0)
    w_partials   |err| <= c eps sum over the block's rows of relu(h) k0    (column 2R: of k0)

These expressions hold on this file's grids only, where p0, x_in, dx_out, w2 and ent_grad are exact float32 values: the
only errors are expf's, the roundings of the two fma and the accumulation.  c = C_GPU = 4 x C_CPU; C_CPU is the worst ratio
the float32 NumPy restatement of the same formulas reaches against float64 on the same designs, as
tests/test_flow_design.py measures it (SRWN_PRINT_ERR=1 pytest -s prints the figures), rounded up by
gemm_design.rounded_up.  Nothing comes from a GPU.  No entry is excluded: every written element is compared.

    measured (float32 NumPy)   x_out 1.623   dx_in 2.939   g_fp32 1.197   g_bf16 1.981   w_partials 1.900
    C_CPU                      x_out 2.0     dx_in 3.0     g_fp32 1.5     g_bf16 2.0     w_partials 2.0
(dx_in = dx_out expf(p0) is NumPy's float32 exp at |p0| up to 80: 1.5 ulp.  g_bf16 is the output rounding's: half an ulp is
up to 2^-8 of a binade's lower end, against u_out = 2^-9.)
"""
import functools
import math

import numpy as np

from tests.gemm_design import EPS, S_MAX, U_OUT, bf16_round, exact, is_bf16, round_out, rounded_up, same_bits, ties  # noqa: F401

FLOW_BLOCK = 256          # rows per ent / weight-gradient partial (srwn_flow_partials)
IC_BLOCK = 256            # rows per input-conv weight-gradient partial (srwn_init_conv_wgrad_partials)
SQ_CHUNK = 4096           # elements per sum-of-squares partial (srwn_sumsq_partials)

C_CPU = {"x_out": 2.0, "dx_in": 3.0, "g_fp32": 1.5, "g_bf16": 2.0, "w_partials": 2.0}
C_GPU = {k: 4.0 * v for k, v in C_CPU.items()}


def _seed(*k):
    return int(sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) % (2 ** 31))


def units(x, grid, what=""):
    """The proof obligation of a dyadic quantity: x (a sum of absolute values of the terms) is on `grid` and below 2^22
    units of it.  Returns the units."""
    u = np.asarray(x, np.float64) / grid
    assert np.array_equal(u, np.rint(u)), what + ": off the grid"
    assert np.abs(u).max(initial=0) < S_MAX, "%s: %g units: not below 2^22" % (what, np.abs(u).max())
    return u


def block_sum(x, block):
    """Sums of consecutive groups of `block` rows (the last one ragged): [ceil(rows / block), ...]."""
    return np.add.reduceat(x, np.arange(0, x.shape[0], block), axis=0)


def fma32(p, q, r):
    """fmaf on float32 arrays: the product of two float32 numbers is exact in float64; one rounding to float32 follows."""
    f = np.float32
    return (np.asarray(p, f).astype(np.float64) * np.asarray(q, f).astype(np.float64) + np.asarray(r, f).astype(np.float64)).astype(f)


def ratio(got, ref, scale):
    """|got - ref| / scale per entry; 0 where the error is 0 (an exact entry, whatever its scale), inf where a non-zero
    error meets a zero scale."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / scale)


# ---- srwn_flow_affine_fwd / _bwd ----------------------------------------------------------------------------------------
FLOW_RS = (32, 64)
FLOW_ROWS = (1, 33, 65, 255, 256, 257, 513)     # row-group edges of both lane layouts (64 rows per pass at R = 32, 32 at 64)
ENT_GRADS = (0.0, -0.25)
GH, GW2, GX, GD = 0.25, 0.125, 0.25, 0.125      # grids of h, w2, x_in, dx_out
B2_1 = 5.0 / 32
PRM1_JUNK = 64.0                                # prm[:, 1] of the designed prm: the backward must not read it


def flow_h(rows, R, seed):
    """h [rows, R] on the grid 1/4, |int| <= 7: half negative, an eighth +0.0, an eighth -0.0 (the ReLU ties); the first
    row starts +0.0, -0.0, -1/4, +1/2 so that one row holds every kind."""
    rng = np.random.default_rng(seed + 101)
    h = exact((rows, R), 7, 1.0, seed, GH)
    u = rng.random((rows, R))
    h = np.where(u < 0.125, 0.0, np.where(u < 0.25, -0.0, h))
    h[0, :4] = [0.0, -0.0, -0.25, 0.5]
    return h


def relu(h):
    return np.where(h > 0, h, 0.0)


@functools.lru_cache(maxsize=None)
def flow_fwd(rows, R, general):
    """h, w2 [R, 2], b2 [2], x_in [rows] and the float64 references prm [rows, 2], x_out [rows], ent [blocks], the bound
    scale of x_out and the rows of the overflow stratum."""
    s = _seed(rows, R, general, 3)
    h = flow_h(rows, R, s)
    w2 = exact((R, 2), 15, 1.0, s + 1, GW2)
    x_in = exact((rows,), 15, 1.0, s + 2, GX)
    inf_rows = np.zeros(rows, bool)
    if not general:
        w2[:, 0] = 0.0
        b2 = np.array([0.0, B2_1])
    else:
        # channels 0 / 1 carry p0 = +-8 h: q in [-72, 72] on the grid 1; the rest adds a few units (|w2[c, 0]| <= 3/8)
        rng = np.random.default_rng(s + 3)
        w2[:, 0] = exact((R,), 3, 1.0, s + 4, GW2)
        w2[0, 0], w2[1, 0] = 8.0, -8.0
        q = rng.integers(-72, 73, rows)
        h[:, 0] = np.where(q > 0, q / 8.0, -0.25)
        h[:, 1] = np.where(q < 0, -q / 8.0, -0.0)
        b2 = np.array([1.0, B2_1])
        inf_rows = np.arange(rows) % 7 == 3
        h[inf_rows] = -np.abs(h[inf_rows])
        h[inf_rows, 0] = 11.0                    # p0 = 8 * 11 + 1 = 89: expf overflows (e^89 = 4.5e38 > 3.4e38)
    a = relu(h)
    prm = a @ w2 + b2
    S = np.abs(a) @ np.abs(w2) + np.abs(b2)
    assert is_bf16(h) and not np.isnan(h).any()
    gp = GH * GW2 / 2 if general else GH * GW2       # (the carriers of the general design are on the grid 1/8)
    units(S, gp, "prm")
    ent = block_sum(prm[:, 0], FLOW_BLOCK)
    units(block_sum(S[:, 0], FLOW_BLOCK), gp, "ent_partials")
    if general:
        assert (prm[inf_rows, 0] == 89.0).all() and np.abs(prm[~inf_rows, 0]).max(initial=0) <= 80.0
        assert (x_in != 0).all()
    else:
        assert (prm[:, 0] == 0).all()
        units(np.abs(x_in) + S[:, 1], gp, "x_out")
    e = np.exp(prm[:, 0])
    x_out = np.where(inf_rows, np.sign(x_in) * np.inf, x_in * e + prm[:, 1])
    with np.errstate(invalid="ignore"):
        scale = np.where(inf_rows, 0.0, EPS * (np.abs(x_in) * e + np.abs(x_out)))
    return dict(h=h, w2=w2, b2=b2, x_in=x_in, prm=prm, x_out=x_out, ent=ent, x_scale=scale, inf_rows=inf_rows)


def flow_fwd32(d):
    """x_out of the float32 restatement: fmaf(x_in, expf(p0), p1) on the exact p0, p1."""
    f = np.float32
    with np.errstate(over="ignore"):
        return fma32(d["x_in"], np.exp(d["prm"][:, 0].astype(f)), d["prm"][:, 1]).astype(np.float64)


def flow_bwd_formulas(h, w2, p0, x_in, dxo, ent_grad):
    """include/srwn.h's backward in float64, for any operands: (dprm0, dprm1, k0, g [rows, R], dx_in)."""
    sc = np.exp(p0)
    d0 = dxo * x_in * sc + ent_grad
    k0 = np.abs(dxo * x_in) * sc + np.abs(d0)
    g = (h > 0) * (d0[:, None] * w2[None, :, 0] + dxo[:, None] * w2[None, :, 1])
    return d0, dxo, k0, g, dxo * sc


@functools.lru_cache(maxsize=None)
def flow_bwd(rows, R, general, ent_grad):
    """h, w2, the designed prm, x_in, dx_out and the float64 references g [rows, R] (unrounded), dx_in, w_partials
    [blocks, 2R + 2] with the bound scales of the general design.  `exact_cols`: the columns of w_partials that are dyadic."""
    s = _seed(rows, R, general, int(ent_grad * 4), 5)
    rng = np.random.default_rng(s + 4)
    h = flow_h(rows, R, s)
    w2 = exact((R, 2), 15, 1.0, s + 1, GW2)
    top = 7 if general else 15
    x_in = exact((rows,), top, 1.0, s + 2, GX)
    dxo = exact((rows,), top, 0.9 if rows > 1 else 1.0, s + 3, GD)
    p0 = rng.integers(-320, 321, rows) / 4.0 if general else np.zeros(rows)
    prm = np.stack([p0, np.full(rows, PRM1_JUNK)], 1)
    a, pos = relu(h), h > 0
    d0, d1, k0, g, dx_in = flow_bwd_formulas(h, w2, p0, x_in, dxo, ent_grad)
    wp = np.empty((-(-rows // FLOW_BLOCK), 2 * R + 2))
    wp_scale = np.zeros_like(wp)
    wp[:, 0:2 * R:2] = block_sum(a * d0[:, None], FLOW_BLOCK)
    wp[:, 1:2 * R:2] = block_sum(a * d1[:, None], FLOW_BLOCK)
    wp[:, 2 * R] = block_sum(d0, FLOW_BLOCK)
    wp[:, 2 * R + 1] = block_sum(d1, FLOW_BLOCK)
    wp_scale[:, 0:2 * R:2] = EPS * block_sum(a * k0[:, None], FLOW_BLOCK)
    wp_scale[:, 2 * R] = EPS * block_sum(k0, FLOW_BLOCK)
    exact_cols = np.ones(2 * R + 2, bool)
    units(block_sum(a * np.abs(d1)[:, None], FLOW_BLOCK), GH * GD, "w_partials, dprm1")
    units(block_sum(np.abs(d1), FLOW_BLOCK), GD, "w_partials, sum dprm1")
    if general:
        exact_cols[0:2 * R:2] = False
        exact_cols[2 * R] = False
    else:
        gd0 = GD * GX                        # d0 on the grid 1/32 (ent_grad is on it)
        units(np.abs(dxo * x_in) + abs(ent_grad), gd0, "dprm0")
        units(np.abs(d0)[:, None] * np.abs(w2[None, :, 0]) + np.abs(d1)[:, None] * np.abs(w2[None, :, 1]), gd0 * GW2, "g")
        units(block_sum(a * np.abs(d0)[:, None], FLOW_BLOCK), GH * gd0, "w_partials, dprm0")
        units(block_sum(np.abs(d0), FLOW_BLOCK), gd0, "w_partials, sum dprm0")
    return dict(h=h, w2=w2, prm=prm, x_in=x_in, dx_out=dxo, g=g, dx_in=dx_in, wp=wp, wp_scale=wp_scale, exact_cols=exact_cols,
                pos=pos, g_scale_eps=EPS * (k0[:, None] * np.abs(w2[None, :, 0]) + np.abs(d1[:, None] * w2[None, :, 1])) * pos)


def g_scale(d, mode):
    return U_OUT[mode] * np.abs(d["g"]) + d["g_scale_eps"]


def flow_bwd32(d, ent_grad, mode):
    """The float32 restatement in the kernel's written order: (g, dx_in, w_partials) as float64 (g rounded to bf16 in bf16
    mode); the weight-gradient sums run over a block's rows in order."""
    f = np.float32
    h, w2 = d["h"].astype(f), d["w2"].astype(f)
    dxo, x_in = d["dx_out"].astype(f), d["x_in"].astype(f)
    sc = np.exp(d["prm"][:, 0].astype(f))
    d0 = fma32(dxo * x_in, sc, f(ent_grad))
    d1 = dxo
    g = np.where(d["pos"], fma32(d0[:, None], w2[None, :, 0], d1[:, None] * w2[None, :, 1]), f(0))
    dx_in = dxo * sc
    a = np.where(d["pos"], h, f(0))
    rows, R = h.shape
    nb = -(-rows // FLOW_BLOCK)
    wp = np.zeros((nb, 2 * R + 2), f)
    pad = nb * FLOW_BLOCK - rows
    ap = np.concatenate([a, np.zeros((pad, R), f)]).reshape(nb, FLOW_BLOCK, R)
    d0p = np.concatenate([d0, np.zeros(pad, f)]).reshape(nb, FLOW_BLOCK)
    d1p = np.concatenate([d1, np.zeros(pad, f)]).reshape(nb, FLOW_BLOCK)
    for r in range(FLOW_BLOCK):
        wp[:, 0:2 * R:2] = fma32(ap[:, r], d0p[:, r, None], wp[:, 0:2 * R:2])
        wp[:, 1:2 * R:2] = fma32(ap[:, r], d1p[:, r, None], wp[:, 1:2 * R:2])
        wp[:, 2 * R] += d0p[:, r]
        wp[:, 2 * R + 1] += d1p[:, r]
    g = g.astype(np.float64)
    return (bf16_round(g) if mode == "bf16" else g), dx_in.astype(np.float64), wp.astype(np.float64)


# ---- the convolutions ---------------------------------------------------------------------------------------------------
def delay(x, off):
    """x [B, T, ...] -> out[:, t] = x[:, t - off] (0 outside the clip); off of either sign."""
    out = np.zeros_like(x)
    T = x.shape[1]
    if abs(off) < T:
        if off >= 0:
            out[:, off:] = x[:, :T - off]
        else:
            out[:, :T + off] = x[:, -off:]
    return out


def edged(x, top, grid, first_only=False):
    """Range-top values (+-top * grid) on the first two (and last two) rows of every clip."""
    T = x.shape[1]
    n = min(2, T)
    x[:, :n] = top * grid * np.sign(x[:, :n])
    if not first_only:
        x[:, T - n:] = top * grid * np.sign(x[:, T - n:])
    return x


def dilations(T):
    return sorted({1, max(T - 1, 1), T, T + 5})


GCX, GCW = 0.25, 0.125
DGRAD_B = 3
DGRAD_TS = (1, 2, 255, 256, 257)
DGRAD_SHAPES = ((1, 1, 8), (2, 1, 64), (3, 3, 32), (2, 96, 64))      # (K, Cin, Cout); the last: exactly 48 KiB of weights
DGRAD_REFUSED = (2, 97, 64)
DGRAD_SCALE = 0.5


def dgrad_shifts(T):
    return sorted({0, 1, T})


@functools.lru_cache(maxsize=None)
def dgrad(T, K, Cin, Cout):
    """dy [B, T, Cout] (1/8, |int| <= 3, 15 on every clip's first rows), w [K, Cin, Cout] (1/8), the dx [B, T, Cin] to
    accumulate into (1/64, non-zero)."""
    s = _seed(T, K, Cin, Cout, 7)
    dy = edged(exact((DGRAD_B, T, Cout), 3, 1.0, s, GCW), 15, GCW, first_only=True)
    w = exact((K, Cin, Cout), 15, 1.0, s + 1, GCW)
    dx0 = exact((DGRAD_B, T, Cin), 15, 1.0, s + 2, GCW * GCW)
    assert is_bf16(dy)
    return dict(dy=dy, w=w, dx0=dx0)


def dgrad_ref(d, dil, shift, accumulate):
    """dx[b, u, i] (+)= scale sum_k sum_o w[k, i, o] dy[b, u + shift + (K - 1 - k) dil, o], with its proof obligation."""
    K = d["w"].shape[0]
    s = np.zeros_like(d["dx0"])
    S = np.zeros_like(s)
    for k in range(K):
        off = shift + (K - 1 - k) * dil
        s += np.einsum("bto,io->bti", delay(d["dy"], -off), d["w"][k])
        S += np.einsum("bto,io->bti", delay(np.abs(d["dy"]), -off), np.abs(d["w"][k]))
    if not accumulate:
        units(S, GCW * GCW, "dgrad")
        return s
    units(np.abs(d["dx0"]) + DGRAD_SCALE * S, GCW * GCW * DGRAD_SCALE, "dgrad, accumulated")
    return d["dx0"] + DGRAD_SCALE * s


# (B, T, Cin, Cout, K): the four code paths of srwn_causal_conv1d_fwd
CONV_FWD = ([(1, T, 1, 64, K) for T in (255, 256, 257) for K in (2, 3)]          # Cin = 1, K = 2 / K != 2: B T around a block edge
            + [(3, 45, 1, 64, 1), (3, 1, 1, 64, 2), (3, 1, 1, 64, 3)]               # K = 1; T = 1
            + [(3, 45, 3, 32, 2), (3, 45, 3, 32, 3), (3, 1, 3, 32, 2)]              # generic: Cin = 3
            + [(3, 45, 1, 24, 2), (3, 45, 1, 10, 3), (3, 45, 1, 10, 2)]             # generic: Cout / 8 no divisor of 256; Cout % 8 != 0
            + [(3, 683, 1, 8, 2), (3, 683, 1, 8, 3)]                               # B T = 2049: a block covers 2048 rows
            + [(3, 3, 1, 2048, 2), (3, 3, 1, 2048, 1)])                            # B T = 9: a block covers 8 rows
CONV_SHIFTS = (-1, 0, 1)                                                          # -1: the non-causal encoder's


def conv_path(Cin, Cout, K):
    """The kernel srwn_causal_conv1d_fwd picks: "cin1_k2", "cin1_any" or "generic"."""
    if Cin == 1 and Cout % 8 == 0 and 256 % (Cout // 8) == 0:
        return "cin1_k2" if K == 2 else "cin1_any"
    return "generic"


def conv_dilations(T):
    return sorted({1, T, T + 5}) if T > 300 or T < 3 else dilations(T)


@functools.lru_cache(maxsize=None)
def conv_fwd(B, T, Cin, Cout, K):
    """x [B, T, Cin] (1/4, |int| <= 3, 15 at both ends of every clip), w [K, Cin, Cout] (1/8), bias [Cout] on the finer grid
    1/256: the sums need more than 8 bits, so a bf16 output rounds and meets ties."""
    s = _seed(B, T, Cin, Cout, K, 11)
    x = edged(exact((B, T, Cin), 3, 1.0, s, GCX), 15, GCX)
    return dict(x=x, w=exact((K, Cin, Cout), 15, 1.0, s + 1, GCW), b=exact((Cout,), 15, 1.0, s + 2, GCX * GCW / 8))


def conv_fwd_ref(d, dil, shift, bias):
    """y[b, t, o] = bias[o] + sum_k sum_i x[b, t - (K - 1 - k) dil - shift, i] w[k, i, o] (include/srwn.h)."""
    K = d["w"].shape[0]
    y = np.zeros(d["x"].shape[:2] + (d["w"].shape[2],))
    S = np.zeros_like(y)
    for k in range(K):
        off = (K - 1 - k) * dil + shift
        y += delay(d["x"], off) @ d["w"][k]
        S += delay(np.abs(d["x"]), off) @ np.abs(d["w"][k])
    if bias:
        y, S = y + d["b"], S + np.abs(d["b"])
    units(S, GCX * GCW / 8, "conv_fwd")
    return y


IC_RS = (32, 64, 128)
IC_KS = (1, 2, 3, 7)              # the reduction buffer takes 8192 (K + 1) bytes of LDS whatever R: K = 7 fills 64 KiB exactly
IC_K_REFUSED = 8                  # ... and K = 8 (72 KiB) is refused by the entry's own check at every R
IC_CLIPS = ((1, 255), (1, 256), (1, 257), (6, 100), (3, 1), (65, 256), (1, 16640))


def ic_lds(R, K):
    """Bytes of dynamic LDS srwn_init_conv_wgrad's first stage asks for: [256 / (R / 8) row groups][(K + 1) R] floats."""
    return (256 // (R // 8)) * (K + 1) * R * 4


class InitConv:
    """audio [B, T] (1/4, |int| <= 3, 15 at both ends of every clip), g [B, T, R] (1/8, |int| <= 3); per-block partial sums
    by tap offset, formed once and shared by every (K, shift)."""

    def __init__(self, B, T, R):
        s = _seed(B, T, R, 13)
        self.B, self.T, self.R = B, T, R
        self.audio = edged(exact((B, T, 1), 3, 1.0, s, GCX), 15, GCX)[..., 0]
        self.g = exact((B, T, R), 3, 1.0, s + 1, GCW)
        self._off = {}
        assert is_bf16(self.g)

    def _partial(self, off):
        """[blocks, R]: sum over the block's rows of audio[b, t - off] g[b, t, :] (off None: of g)."""
        if off not in self._off:
            g = self.g.reshape(-1, self.R)
            x = np.ones((self.B * self.T, 1)) if off is None else delay(self.audio[..., None], off).reshape(-1, 1)
            units(block_sum(np.abs(x * g), IC_BLOCK).sum(0), GCX * GCW, "init_conv_wgrad")       # (the whole sum: gw / gb too)
            self._off[off] = block_sum(x * g, IC_BLOCK)
        return self._off[off]

    def partials(self, K, shift):
        """[blocks, K + 1, R]: [gw | gb] per block; gw[k, o] = sum audio[b, t - (K - 1 - k) - shift] g[b, t, o]."""
        return np.stack([self._partial((K - 1 - k) + shift) for k in range(K)] + [self._partial(None)], 1)


@functools.lru_cache(maxsize=None)
def init_conv(B, T, R):
    return InitConv(B, T, R)


# ---- clipping -----------------------------------------------------------------------------------------------------------
SUMSQ_NS = (1, 4095, 4096, 4097, 12288, 12289)
CLIP_COUNTS = (1, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def sumsq(n):
    """g [n] (1/4, |int| <= 15) and its chunk sums of squares: at most 4096 * 225 units of 1/16."""
    g = exact((n,), 15, 1.0, _seed(n, 17), 0.25)
    units(block_sum(g * g, SQ_CHUNK), 1.0 / 16, "sumsq")
    return dict(g=g, parts=block_sum(g * g, SQ_CHUNK))


def clip_cases(m):
    """(name, partials [m], clip_norm, pre_scale): dyadic partials (their double sum is exact), dyadic clip_norm."""
    p = np.abs(exact((m,), 15, 1.0, _seed(m, 19), 1.0 / 16))
    four = np.full(m, 2.0 ** -8)
    four[0] = 4.0 - (m - 1) * 2.0 ** -8
    assert p.min() >= 1.0 / 16 and math.fsum(four) == 4.0 and four[0] > 0
    for pre in (1.0, 0.5):
        yield ("below", p, 64.0, pre)                 # norm <= sqrt(1000 * 15 / 16) < 64
        yield ("above", p, 2.0 ** -4, pre)            # norm >= pre sqrt(1/16) >= 1/8
        yield ("equal", four, 2.0 * pre, pre)         # pre sqrt(4) == clip_norm exactly (clip_norm 2 at pre_scale 1)
        yield ("zero", np.zeros(m), 2.0, pre)         # scale == pre_scale, finite


def clip_ref(parts, clip_norm, pre_scale):
    """include/srwn.h's formula in float64, rounded once to float32: (scale, norm)."""
    s = math.fsum(parts.tolist())
    assert s == float(np.sum(parts)) and float(np.float32(clip_norm)) == clip_norm and float(np.float32(pre_scale)) == pre_scale
    norm = pre_scale * math.sqrt(s)
    return np.array([np.float32(pre_scale * clip_norm / max(norm, clip_norm)), np.float32(norm)], np.float64)


AXPY_NS = CLAMP_NS = (1, 255, 256, 257)
AXPY_SCALES = (0.0, 1.0, 0.125)
AXPY_ALPHA = 0.25                                    # 1 / B for B = 4


@functools.lru_cache(maxsize=None)
def axpy(n):
    """y [n] (1/64), x [n] (1/4): y + alpha scale x is on the grid 1/128 for every scale of AXPY_SCALES."""
    s = _seed(n, 23)
    d = dict(y=exact((n,), 15, 1.0, s, 1.0 / 64), x=exact((n,), 15, 1.0, s + 1, 0.25))
    units(np.abs(d["y"]) + np.abs(d["x"]), 1.0 / 128, "axpy")
    return d


POWER_NS = (1, 257, 771)
POWER_GAMMA, POWER_GSCALE = 0.5, 0.25


@functools.lru_cache(maxsize=None)
def power(n):
    """power_truth, power_out [n] (1/4): loss = gamma sum (pt - po)^2 and dpow = -2 gamma gscale (pt - po), both dyadic."""
    s = _seed(n, 29)
    pt, po = exact((n,), 15, 1.0, s, 0.25), exact((n,), 15, 1.0, s + 1, 0.25)
    diff = pt - po
    units(np.array([(diff * diff).sum() * POWER_GAMMA]), 1.0 / 32, "power_loss")
    return dict(pt=pt, po=po, loss=POWER_GAMMA * (diff * diff).sum(), dpow=-2.0 * POWER_GAMMA * POWER_GSCALE * diff)


def power_dpow32(d):
    """dpow in float32, in the kernel's written order ((-2 gamma) gscale) d."""
    f = np.float32
    return (f(-2.0) * f(POWER_GAMMA) * f(POWER_GSCALE) * (d["pt"].astype(f) - d["po"].astype(f))).astype(np.float64)


REDUCE_NS = (0, 1, 255, 256, 257, 1000)
REDUCE_SCALE = 2.0 ** -5


@functools.lru_cache(maxsize=None)
def reduce_loss(n):
    p = exact((n,), 255, 1.0, _seed(n, 31), 0.125)
    units(np.array([np.abs(p).sum()]), 0.125 * REDUCE_SCALE, "reduce_loss")
    return dict(p=p, out=p.sum() * REDUCE_SCALE)


CLAMP_BOUNDS = ((-1.0, 1.0), (0.5, 0.5))


def clamp_specials(lo, hi):
    f = np.float32
    inf = f(np.inf)
    return np.array([lo, hi, np.nextafter(f(lo), inf), np.nextafter(f(lo), -inf), np.nextafter(f(hi), inf),
                     np.nextafter(f(hi), -inf), 0.0, -0.0, np.inf, -np.inf], np.float64)


def clamp(n, lo, hi, first=0):
    """x [n]: the values on, just inside and just outside both bounds, +-0 and +-inf (from special number `first` on), then
    the grid 1/4 up to +-3.75; dy [n] (1/8, non-zero).  References: y, dx."""
    s = _seed(n, int(lo * 4), int(hi * 4), 37)
    sp = np.roll(clamp_specials(lo, hi), -first)
    x = exact((n,), 15, 1.0, s, 0.25)
    x[:min(n, len(sp))] = sp[:n]
    dy = exact((n,), 15, 1.0, s + 1, 0.125)
    return dict(x=x, dy=dy, y=np.minimum(np.maximum(x, lo), hi), dx=np.where((x >= lo) & (x <= hi), dy, 0.0))
