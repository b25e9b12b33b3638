"""Layer-local float64 references, the mask-word codec and the input designs for the fused encoder layer kernels
(csrc/srwn_nc.hip: srwn_nc_layer_fwd, srwn_nc_layer_bwd, srwn_nc_mask_bits).  Host code only (NumPy);
tests/test_nc_design.py checks the designs on the CPU and tests/test_gpu_nc_entries.py holds the kernels to them.  The
arithmetic helpers (exact, cover, check_exact, check_cover, round_out, same_bits, ties, bound, ratio, rounded_up) are
those of tests/gemm_design.py.

The operations, from the kernel's header comment, on UNPACKED weights W [K = 2, Cin, Cout] and Wr [Cin, Cout] (C = 128):

  forward    a[t]   = relu(bc + r[t] W[0] + r[t + 1] W[1])          nothing taken from beyond the clip's end
             r'[t]  = relu(br + bf16(a[t]) Wr)
  backward   dh[t]  = [r > 0] (dpre_up[t] W[0]^T + dpre_up[t - 1] W[1]^T)     nothing taken from before the clip's start
             dpre[t] = [a > 0] (bf16(dh[t]) Wr_below^T + scale * frame_add[b, t // pool])

The packed images the kernels read are made by the project's own kernels.Packer and packing.py in the GPU file
(pack_conv, pack_linear(perm=True), pack_conv_T, pack_linear_T(perm=True)), so a wrong image shows against these.

Mask words (the documented layout, not the kernel's code): one uint64 per 32-row tile and lane at index tile * 64 + lane,
tile = b ceil(T / 32) + t // 32, lane = (t % 32) + 32 half; value (mt, q) of a lane is channel
32 mt + 8 (q >> 2) + 4 half + (q & 3) and sits at bit 31 - (16 (mt & 1) + q) of the 32-bit half-word mt >> 1 (half-word 0
= the low 32 bits); the bit is set exactly when the value is > 0.

Exact chained designs.  The first product of either kernel lands on bf16-exact values (check_exact(..., partial16=True):
sum |x||w| + |b| <= 256 units of the product grid), so its bf16 rounding for the chain is the identity, and the second
product only has to stay below 2^22 units.  Forward: r = exact(2, .5) on the grid 1/4, conv taps exact(1, .5) on 1/8, conv
bias exact(8, 1) on 1/32: S1 <= 167 of 256 over the shapes used, the pre-activations of a split 48 % > 0, 2.9 % exactly 0,
49 % < 0.  Wr = exact(4, 1) on 1/8 and br = exact(64, 1) on 1/256: S2 <= 3260, 6 to 8 % of r' on bf16 ties.  A dense integer product of
that spread is exactly 0 in about 0.1 % of its entries, too few to hold the second relu at 0; so the ZERO_COLS (8 of the
128 output columns, two per row tile, one per lane half) of Wr carry ONE entry each and no bias: their pre-activation is
w a[t, m], exactly 0 wherever a[t, m] is (half of the rows), which puts 3 % of r's pre-activations on an exact zero.  The
backward mirrors it (dpre_up = exact(2, .5) on 1/4, W^T of the same taps, frame_add integers <= 64 on a grid that the
power-of-two scale carries onto the product grid 1/256), with both relu masks drawn independently of the values and
encoded by mask_words.  The designs assert >= 1 % exact zeros in each forward pre-activation and >= 1 % ties in each output
that is really rounded (r', dpre; a and dh are bf16 numbers before they are stored).

Random designs for the bound path: inputs standard normals rounded to bf16, weights of O.init_encoder_params' scale
(Xavier uniform: +-sqrt(6 / 512) for the taps, +-sqrt(6 / 256) for a 1x1) rounded to bf16, fp32 biases.  Every product is
compared with a float64 reference fed the kernel's OWN stored first-stage tensor (a_out, dh_out), per entry, within
    |got - ref| <= c (u_out |ref| + K 2^-24 S + f_abs),   c = 4 C_CPU
C_CPU being the worst ratio of a float32 NumPy restatement of the same two products (restate32_*) on the same design,
measured by tests/test_nc_design.py and rounded up by rounded_up; never a GPU figure.  An entry of a relu'd tensor is
undecided when its reference pre-activation lies within the bound of 0: it may then be 0 or the value; every other entry
must carry the reference's mask.  The undecided share is at most 1 % of any tensor (asserted on the CPU, on the reference).
"""
import functools

import numpy as np

from tests import gemm_design as G

C = 128
GR, GW, GB1 = 0.25, 0.125, 0.25 * 0.125          # grids: inputs, weights, first product (1/32)
GB2 = GB1 * GW                                   # second product (1/256)
ZERO_COLS = (3, 20, 41, 62, 67, 84, 105, 126)    # one per (row tile mt, lane half): 32 mt + 8 g + 4 half + e

# (B, T) of the GPU file: one row; ragged and full last tiles with a clip boundary on, before and after a tile edge; 1056
# tiles, the first second trip of the grid-stride loops (> 1024 = 256 workgroups x 4 waves); 2103 tiles, no multiple of 4,
# where some waves take three tiles and the rest two
SMALL = [(1, 1), (1, 31), (1, 32), (2, 33), (3, 50), (2, 64), (3, 96)]
LARGE = [(33, 1024), (3, 22405)]
SHAPES = SMALL + LARGE
RANDOM_SHAPES = [(3, 50), (33, 1024)]
FADD_SCALE = 0.125                               # a power of two, and not 1 / pool: a free argument of the C ABI


def fadd_cases(B, T):
    """(pool, frames, ld, column offset) of the frame_add runs at a shape: pools 32, 25 (frames change inside a tile), 1 and
    > T; frames * pool > T wherever pool does not divide T, and by a whole spare frame at pool 32; a table wider than 128
    read at a column offset, as the encoder passes it."""
    if B * T > 4096:
        return [(25, -(-T // 25), 3 * C, C)]
    out = [(32, T // 32 + 1, 2 * C + 64, 64), (25, -(-T // 25), 3 * C, C), (1, T, C, 0), (T + 3, 1, C + 4, 4),
           (T + 3, 2, 2 * C, C)]
    return out


def _seed(*k):
    return G._seed(*k, 61)


# ---- float64 references -------------------------------------------------------------------------------------------------
def ahead(x, B, T):
    """Row (b, t) holds x[b, t + 1]; 0 in the last row of every clip."""
    x = x.reshape(B, T, -1)
    out = np.zeros_like(x)
    out[:, :T - 1] = x[:, 1:]
    return out.reshape(B * T, -1)


def behind(x, B, T):
    """Row (b, t) holds x[b, t - 1]; 0 in the first row of every clip."""
    x = x.reshape(B, T, -1)
    out = np.zeros_like(x)
    out[:, 1:] = x[:, :T - 1]
    return out.reshape(B * T, -1)


def fwd_conv_ops(r, w, B, T):
    """The conv as one contraction: a [rows, 2 C] = [r[t] | r[t + 1]], w [2 C, C] = [W[0]; W[1]]."""
    return np.concatenate([r, ahead(r, B, T)], 1), np.concatenate([w[0], w[1]], 0)


def bwd_conv_ops(dp, w, B, T):
    """The conv's data gradient as one contraction: [dpre_up[t] | dpre_up[t - 1]] with [W[0]^T; W[1]^T]."""
    return np.concatenate([dp, behind(dp, B, T)], 1), np.concatenate([w[0].T, w[1].T], 0)


def frame_rows(fadd, B, T, pool):
    """fadd [B, frames, C] -> [B T, C]: frame t // pool of clip b for row (b, t)."""
    idx = np.arange(T) // pool
    return fadd[:, idx, :].reshape(B * T, -1)


def fwd_ref(d, B, T):
    """(pre_a, S1, a, pre_r, S2) in float64; a = relu(pre_a) is what the 1x1 reads (exact designs: a bf16 number)."""
    x, w = fwd_conv_ops(d["r"], d["w"], B, T)
    pre_a, S1 = G.contract(x, w, d["bc"])
    a = np.maximum(pre_a, 0.0)
    pre_r, S2 = G.contract(a, d["wr"], d["br"])
    return pre_a, S1, a, pre_r, S2


def bwd_dh_ref(d, B, T):
    """(dh, S1): the masked conv data gradient."""
    x, w = bwd_conv_ops(d["dp"], d["w"], B, T)
    y, S1 = G.contract(x, w)
    return y * d["mr"], S1


def bwd_dpre_ref(dh, d, fa):
    """(dpre, S2) from a given dh [rows, C]; fa [rows, C] = scale * frame_add rows, or None."""
    y, S2 = G.contract(dh, d["wr"].T)
    if fa is not None:
        y, S2 = y + fa, S2 + np.abs(fa)
    return y * d["ma"], S2


# ---- mask words ---------------------------------------------------------------------------------------------------------
def _lane_channels():
    """(channel [2 halves, 64 values], bit [64 values]) of value (mt, q) = 16 mt + q of a lane."""
    mt, q = np.meshgrid(np.arange(4), np.arange(16), indexing="ij")
    ch = np.stack([32 * mt + 8 * (q >> 2) + 4 * half + (q & 3) for half in (0, 1)]).reshape(2, 64)
    bit = (32 * (mt >> 1) + 31 - (16 * (mt & 1) + q)).reshape(64)
    return ch, bit


def nwords(B, T):
    return B * (-(-T // 32)) * 64


def mask_words(x, B, T, beyond=0):
    """x [B T, 128] -> uint64 [B ceil(T / 32) 64]: bit set exactly where x > 0.  Lanes of a ragged last tile whose time row
    lies beyond T hold all zeros (beyond = 0) or all ones (beyond = 1)."""
    ntb = -(-T // 32)
    ch, bit = _lane_channels()
    pos = np.full((B, ntb * 32, C), bool(beyond))
    pos[:, :T] = (np.asarray(x).reshape(B, T, C) > 0)
    pos = pos.reshape(B, ntb, 32, C)
    words = np.zeros((B, ntb, 2, 32), np.uint64)
    for half in (0, 1):
        for v in range(64):
            words[:, :, half, :] |= pos[..., ch[half, v]].astype(np.uint64) << np.uint64(bit[v])
    return words.reshape(-1)


def mask_unwords(words, B, T):
    """The inverse: uint64 words -> bool [B T, 128] (lanes beyond T are dropped)."""
    ntb = -(-T // 32)
    ch, bit = _lane_channels()
    words = np.asarray(words, np.uint64).reshape(B, ntb, 2, 32)
    pos = np.zeros((B, ntb, 32, C), bool)
    for half in (0, 1):
        for v in range(64):
            pos[..., ch[half, v]] = ((words[:, :, half, :] >> np.uint64(bit[v])) & np.uint64(1)).astype(bool)
    return pos.reshape(B, ntb * 32, C)[:, :T].reshape(B * T, C)


def lanes_inside(B, T):
    """bool [B ceil(T / 32) 64]: the lane's time row lies inside the clip (what the kernels' words are compared on)."""
    ntb = -(-T // 32)
    t = 32 * np.arange(ntb)[:, None, None] + np.arange(32)[None, None, :]
    return np.broadcast_to(t < T, (B, ntb, 2, 32)).reshape(-1).copy()


# ---- exact designs ------------------------------------------------------------------------------------------------------
def _wr_exact(seed):
    """Wr [C, C] = exact(4, 1) on 1/8 and br = exact(64, 1) on 1/256, but for ZERO_COLS: one entry per column, no bias."""
    rng = np.random.default_rng(seed + 7)
    wr = G.exact((C, C), 4, 1.0, seed, GW)
    br = G.exact((C,), 64, 1.0, seed + 1, GB2)
    for j in ZERO_COLS:
        m = int(rng.integers(C))
        keep = wr[m, j]
        wr[:, j] = 0.0
        wr[m, j] = keep
        br[j] = 0.0
    return wr, br


@functools.lru_cache(maxsize=2)
def fwd_exact(B, T):
    """r [B T, C] (1/4), w [2, C, C] (1/8), bc [C] (1/32), wr [C, C] (1/8), br [C] (1/256).  One time row per clip has no
    second tap (the clip's end), so at T = 1 only 128 of the 256 k carry a term and r is drawn dense."""
    s = _seed(B, T, 1)
    r = G.cover(G.exact((B * T, C), 2, 1.0 if T == 1 else 0.5, s, GR), 0, s + 5, GR)
    w = G.exact((2, C, C), 1, 0.5, s + 1, GW)
    wr, br = _wr_exact(s + 3)
    return dict(r=r, w=w, bc=G.exact((C,), 8, 1.0, s + 2, GB1), wr=wr, br=br)


@functools.lru_cache(maxsize=2)
def bwd_exact(B, T):
    """dp = dpre_up [B T, C] (1/4), the taps w (1/8), wr = Wr_below [C, C] (1/8, dense), both masks mr, ma in {0, 1} drawn
    independently of every value, fadd [B, T, C]: integers <= 64 on the grid 1/256 / FADD_SCALE, from which a case with
    `frames` frames takes its first `frames` rows per clip."""
    s = _seed(B, T, 2)
    rng = np.random.default_rng(s + 4)
    dp = G.cover(G.exact((B * T, C), 2, 1.0 if T == 1 else 0.5, s, GR), 0, s + 5, GR)
    return dict(dp=dp, w=G.exact((2, C, C), 1, 0.5, s + 1, GW), wr=G.exact((C, C), 4, 1.0, s + 2, GW),
                mr=(rng.random((B * T, C)) < 0.5).astype(np.float64), ma=(rng.random((B * T, C)) < 0.5).astype(np.float64),
                fadd=G.exact((B, T, C), 64, 1.0, s + 3, GB2 / FADD_SCALE))


def _cover_second(a, w, rows):
    """check_cover of a second product whose first operand is relu'd or masked: a third of it is zero by design, so with
    fewer than 31 rows a k index (and with it a one-entry column) may be left without a term; then only the rows and w are
    held."""
    if rows >= 31:
        G.check_cover(a, w)
    else:
        assert np.abs(a).sum(1).min() > 0 and np.abs(w).sum(1).min() > 0 and np.abs(w).sum(0).min() > 0


def check_fwd_exact(B, T):
    """Every obligation of the forward design; returns (pre_a, a, pre_r, share of zeros in pre_a, in pre_r, of ties in r')."""
    d = fwd_exact(B, T)
    x, w = fwd_conv_ops(d["r"], d["w"], B, T)
    k = 2 * C if T > 1 else C                          # (T = 1: the second tap has no row to read)
    S1 = G.check_exact(x[:, :k], w[:k], d["bc"], GR, GW, partial16=True)
    G.check_cover(x[:, :k], w[:k])
    pre_a, _, a, pre_r, _ = fwd_ref(d, B, T)
    assert G.is_bf16(pre_a) and np.array_equal(G.round_out(a, "bf16"), a)      # the chain's rounding is the identity
    S2 = G.check_exact(a, d["wr"], d["br"], GB1, GW)
    _cover_second(a, d["wr"], B * T)
    z1, z2 = float((pre_a == 0).mean()), float((pre_r == 0).mean())
    t2 = float(G.ties(np.maximum(pre_r, 0.0)).mean())
    return dict(pre_a=pre_a, a=a, pre_r=pre_r, S1=S1.max(), S2=S2.max(), zeros_a=z1, zeros_r=z2, ties_r=t2,
                pos_a=float((pre_a > 0).mean()))


def check_bwd_exact(B, T):
    """Every obligation of the backward design, for each frame_add case of the shape; returns the shares of ties."""
    d = bwd_exact(B, T)
    x, w = bwd_conv_ops(d["dp"], d["w"], B, T)
    k = 2 * C if T > 1 else C
    S1 = G.check_exact(x[:, :k], w[:k], None, GR, GW, partial16=True)
    G.check_cover(x[:, :k], w[:k])
    dh, _ = bwd_dh_ref(d, B, T)
    assert np.array_equal(G.round_out(dh, "bf16"), dh)
    assert 0.4 < d["mr"].mean() < 0.6 and 0.4 < d["ma"].mean() < 0.6 if B * T >= 31 else True
    out = dict(S1=S1.max(), S2=0.0, ties=[])
    for (pool, frames, ld, off) in [(None, 0, 0, 0)] + fadd_cases(B, T):
        fa = None if pool is None else FADD_SCALE * frame_rows(d["fadd"][:, :frames], B, T, pool)
        # (a row of dh is zero in a 2^-128 of the draws; frame_add enters as a bias per row)
        S2 = np.abs(dh / GB1) @ np.abs(d["wr"].T / GW) + (0.0 if fa is None else np.abs(fa / GB2))
        assert fa is None or np.array_equal(fa / GB2, np.rint(fa / GB2)), "frame_add off the product grid"
        G.check_exact(dh, d["wr"].T, None, GB1, GW)
        assert S2.max() < G.S_MAX
        _cover_second(dh, d["wr"].T, B * T)
        dpre, _ = bwd_dpre_ref(dh, d, fa)
        out["S2"] = max(out["S2"], float(S2.max()))
        out["ties"].append(float(G.ties(dpre).mean()))
    return out


# ---- random designs and the bound ---------------------------------------------------------------------------------------
def _bf16(x):
    return G.bf16_round(np.asarray(x, np.float64).astype(np.float32).astype(np.float64))


def _weights(rng):
    lim_c, lim_r = np.sqrt(6.0 / (2 * C + 2 * C)), np.sqrt(6.0 / (C + C))      # O.xavier_uniform for [2, C, C] and [1, C, C]
    return _bf16(rng.uniform(-lim_c, lim_c, (2, C, C))), _bf16(rng.uniform(-lim_r, lim_r, (C, C)))


@functools.lru_cache(maxsize=2)
def fwd_random(B, T):
    rng = np.random.default_rng(_seed(B, T, 3))
    w, wr = _weights(rng)
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    return dict(r=_bf16(rng.standard_normal((B * T, C))), w=w, wr=wr, bc=f32(0.1 * rng.standard_normal(C)),
                br=f32(0.1 * rng.standard_normal(C)))


@functools.lru_cache(maxsize=2)
def bwd_random(B, T, pool=25):
    """The masks are given bits here too (independent draws); frame_add [B, ceil(T / pool), C] fp32 of the gradient's size."""
    rng = np.random.default_rng(_seed(B, T, 4))
    w, wr = _weights(rng)
    frames = -(-T // pool)
    return dict(dp=_bf16(rng.standard_normal((B * T, C))), w=w, wr=wr, mr=(rng.random((B * T, C)) < 0.5).astype(np.float64),
                ma=(rng.random((B * T, C)) < 0.5).astype(np.float64), pool=pool, frames=frames,
                fadd=np.asarray(pool * rng.standard_normal((B, frames, C)), np.float32).astype(np.float64), scale=1.0 / pool)


# Worst ratio of the float32 NumPy restatement on RANDOM_SHAPES as tests/test_nc_design.py measures it (SRWN_PRINT_ERR=1
# pytest -s prints the figures), rounded up by gemm_design.rounded_up:
#   measured   nc_fwd_a 1.919   nc_fwd_r 1.970   nc_bwd_dh 1.948   nc_bwd_dpre 1.977      (undecided relu entries: <= 0.13 %)
# (all four are set by their bf16 outputs: a correctly rounded result reaches 2 against u_out = 2^-9 at a binade's lower end.)
C_CPU = {"nc_fwd_a": 2.0, "nc_fwd_r": 2.0, "nc_bwd_dh": 2.0, "nc_bwd_dpre": 2.0}
C_GPU = {k: 4.0 * v for k, v in C_CPU.items()}
UNDECIDED_CAP = 0.01


def _eval32(a, w, b, rows=2048):
    """G.eval32 (one k at a time, in order, bias first) in blocks of rows that stay in the cache."""
    return np.concatenate([G.eval32(a[i:i + rows], w, b, range(a.shape[1])) for i in range(0, a.shape[0], rows)], 0)


def restate32_fwd(d, B, T):
    """The forward layer in float32 NumPy: (a, r') as stored (bf16 numbers, float64 arrays)."""
    x, w = fwd_conv_ops(d["r"], d["w"], B, T)
    a = G.bf16_round(np.maximum(_eval32(x, w, d["bc"]), np.float32(0)).astype(np.float64))
    r = G.bf16_round(np.maximum(_eval32(a, d["wr"], d["br"]), np.float32(0)).astype(np.float64))
    return a, r


def restate32_bwd(d, B, T):
    """The backward layer in float32 NumPy: (dh, dpre) as stored."""
    x, w = bwd_conv_ops(d["dp"], d["w"], B, T)
    dh = G.bf16_round((_eval32(x, w, None) * d["mr"].astype(np.float32)).astype(np.float64))
    fa = (frame_rows(d["fadd"], B, T, d["pool"]).astype(np.float32) * np.float32(d["scale"]))
    # (a bias per row, first in the sum: the kernel starts its accumulator at scale * frame_add)
    acc = np.concatenate([_eval32_rowbias(dh[i:i + 2048], d["wr"].T, fa[i:i + 2048]) for i in range(0, B * T, 2048)], 0)
    dpre = G.bf16_round((acc * d["ma"].astype(np.float32)).astype(np.float64))
    return dh, dpre


def _eval32_rowbias(a, w, bias_rows):
    f = np.float32
    a32, w32 = a.astype(f), w.astype(f)
    acc = bias_rows.astype(f).copy()
    for k in range(a.shape[1]):
        acc += a32[:, k:k + 1] * w32[k:k + 1, :]
    return acc


def relu_entries(got, pre, S, K, key):
    """A relu'd tensor against its reference pre-activation, per entry: (ratio of the decided entries and of the undecided
    ones that kept their value, undecided [bool], wrong-mask [bool]).  Undecided: |pre| <= c x the bound's scale; such an
    entry may be 0 or the value.  Every other entry must be > 0 exactly where pre is."""
    got = np.asarray(got, np.float64)
    scale = G.bound_scale(pre, S, K, "bf16")
    undecided = np.abs(pre) <= C_GPU[key] * scale
    wrong = ~undecided & ((got > 0) != (pre > 0))
    ref = np.where(undecided & (got == 0), 0.0, np.where(undecided, pre, np.maximum(pre, 0.0)))
    err = np.abs(got - ref)
    return np.where(err == 0, 0.0, err / scale), undecided, wrong
