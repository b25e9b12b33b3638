"""Layer-local references for the multi-layer (group) kernels of csrc/srwn_group.hip.  Host code only (NumPy);
tests/test_group_design.py checks the designs on the CPU, tests/test_gpu_group_entries.py holds the kernels to them.
The helpers of tests/gemm_design.py (G) are reused, not copied.

The chain through sqrt(1/2) and the gate has no exact design, but the kernels STORE their intermediates: df_g and G_g of
every layer, and the gradient handed from layer to layer is the stored one.  So each layer is compared with a float64
restatement of that ONE layer, fed with the kernel's own stored operands of the layer above:

    p_g  = fl32( G_{g+1} * 0.7071067811865476f )              one IEEE fp32 product: reproduced bit for bit in NumPy
    a_g  = rnd_T( p_g )                                       the MFMA operand (bf16 mode rounds it again; fp32: a = p)
    dc_g = Wr_g a_g + dcs_g
    df_g = rnd_T( dc_g c'(z_g) )                              c' = d(z sigmoid z)/df, csrc/srwn_common.h
    G_g  = rnd_T( p_g + sum_k Wf_g[k] df_g[t + (K-1-k) d_g] ) df_g = the STORED df (zero beyond the clip's end)

p and a are deterministic functions of the stored G_{g+1}: no uncertainty enters through them, and no error travels
further than one layer.  Weights, dcs, the top gradient and z are dyadic (signed small integers times a power of two,
z on the grid {-1, -1/2, 0, 1/2, 1}); what is left is the fp32 accumulation (at most K 2^-24 S), the fp32 restatement
of c' (f_abs(z), measured per grid value; 0 at z = 0 where c' = 1/2 exactly) and the product's own fp32 rounding.  Their
sum is the REACH of an entry: how far the value the kernel rounds to T can lie from the float64 one,

    e_df = K 2^-24 S_dc |c'| [Wr a != 0 somewhere in the sum] + f_abs(z) |dc| + 2^-24 |df| [z != 0]
    e_G  = K 2^-24 (|p| + S_taps) [S_taps != 0]                K = the non-zero terms of the entry's own sum
(the accumulation term also vanishes where the entry's terms share a unit 2^-b and S <= 2^24 units: every partial sum
is then an exact fp32 number in any order, `sums_exactly` -- the top layer without g_top, and many sums of bf16 terms)

and an entry is DECIDED when e = 0, or when the float64 value lies farther than REACH x e from the nearest rounding
midpoint of T (`midpoint_distance`): then every admissible evaluation rounds the same way and the kernel must match
the reference BIT FOR BIT.  The others are held to  ulp_T(ref) + c (u_out |ref| + e).  REACH = 4 x the worst |fp32 NumPy
restatement (before its rounding to T) - float64| / e on these designs, c = 4 x the worst ratio of the rounded
restatement against u_out |ref| + e (C_CPU below, measured by tests/test_group_design.py; never a GPU figure).

fp32 mode: half an ulp of the output (2^-25 |ref|) lies below the accumulation's own K 2^-24 S, so an fp32 entry is
decided exactly when e = 0 -- no Wr term and z = 0 (df = dcs / 2), or no tap term (G = p) -- and every other fp32 entry
is held by the bound (whose u_out is 2^-24: four orders sharper than the norms it replaces).  The cap on undecided
entries (at most 10 % of every stored tensor, no wholly undecided time row or channel column) is a statement about
bf16 mode, where the existing tests hold the group kernel only to 2e-2 in a norm; in fp32 mode the kernel is bit-equal
to the per-layer twin (tests/test_gpu_group.py), which tests/test_gpu_gemm_entries.py holds per entry.
"""
import numpy as np

from tests import gemm_design as G

F32 = np.float32
SQRT_HALF32 = F32(0.7071067811865476)        # kSqrtHalf of csrc/srwn_common.h, as the compiler rounds the literal
MANT = {"bf16": 7, "fp32": 23}
CAP = 0.90                                    # decided share of every stored tensor, bf16 mode

# (dilations, B, T, seg_rows): the smallest shapes that reach each path of the kernels
CASES = [
    ([1, 2, 4], 3, 1, 0),                     # one position
    ([2, 2, 2], 1, 31, 0),                    # less than a tile, stride 2, classes of 16 and 15
    ([1, 2, 4, 8, 16], 2, 150, 40),           # halo 31, several segments per clip, ragged last
    ([1, 2, 4, 8, 16], 1, 520, 500),          # 17 tiles, the three-tile body (fp32: cut into 8-tile images)
    ([4, 8, 16, 32], 2, 131, 0),              # residue classes whose lengths differ by one
    ([4, 8, 16, 32], 2, 131, 24),             # ... in short segments
    ([32, 64], 1, 70, 0),                     # classes of 3 and 2 positions, no halo
    ([3, 6], 2, 65, 0),                       # gcd 3
    ([1, 2, 4, 8, 1, 2, 4, 8], 1, 100, 0),    # kMaxGroup layers within halo 30
]
GRID2 = [2, 5]                                # indices of CASES that run again with two workgroups (several segments each)
VARIANTS = ["both", "gtop", "dcs"]            # which of g_top / dcs the launch gets
# (case index, R, variant) of every run: both widths with both operands everywhere, the single-operand launches at four shapes
RUNS = [(i, R, v) for i in range(9) for R in (64, 32) for v in VARIANTS
        if v == "both" or (i in (2, 4, 7) and R == 64) or (i == 1 and R == 32)]
Z_GRID = G.BWD_Z
Z_PROB = np.array([0.01, 0.33, 0.32, 0.33, 0.01])      # +-1 (c' = 0: absolute bound only in bf16 mode) kept rare
GD, GG = 0.25, 0.25                           # grids of dcs and g_top; weights on G.GW = 1/8


# ---- rounding ------------------------------------------------------------------------------------------------------------
def round_to(x, mode):
    """float64 -> nearest-even rounding to bf16 / fp32 in ONE step (no detour through fp32), as float64."""
    x = np.asarray(x, np.float64)
    if mode == "fp32":
        return x.astype(F32).astype(np.float64)
    out = np.zeros_like(x)
    nz = x != 0
    e = np.floor(np.log2(np.abs(x[nz])))
    ulp = 2.0 ** (e - MANT[mode])
    out[nz] = np.rint(x[nz] / ulp) * ulp
    return out


def ulp_of(x, mode):
    x = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore"):
        e = np.where(x > 0, np.floor(np.log2(np.where(x > 0, x, 1.0))), -126.0)
    return 2.0 ** (e - MANT[mode])


def midpoint_distance(v, mode):
    """G.midpoint_distance for either output type: distance of v to the nearest midpoint between two adjacent T numbers."""
    if mode == "bf16":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(np.asarray(v) != 0, G.midpoint_distance(np.where(np.asarray(v) != 0, v, 1.0)), np.inf)
    v = np.abs(np.asarray(v, np.float64))
    ulp = ulp_of(v, mode)
    frac = (v / ulp) % 1.0
    return np.where(v != 0, np.abs(frac - 0.5) * ulp, np.inf)


def f_abs_z(z, mode):
    """|c' restated in float32 (G.dgate32: expf form / the bf16 mode's polynomial) - c' in float64|, per entry of z."""
    return np.abs(G.dgate32(z, mode).astype(np.float64) - G.dgate64(z))


# ---- the designs ---------------------------------------------------------------------------------------------------------
def design(dil, B, T, R, variant="both", exact_corner=False):
    """wf [n, 2, R, R] ([tap][in][out], ops.py:14) and wr [n, R, R] ([in][out]) sparse on the grid 1/8 with every row,
    column and tap covered; z [n, B T, R] on Z_GRID; dcs [n, B T, R] and g_top [B T, R] on the grid 1/4, |int| <= 15, the
    last two rows of every clip but the last and the first two of every clip but the first at 15 (a tap that reads across
    a clip's end shows).  exact_corner: z = 0,
    no g_top, and a quarter of the rows of every Wr zero (df = dcs / 2 there, whatever the chain hands down)."""
    n = len(dil)
    s = G._seed(R, B, T, n, dil[0], dil[-1], VARIANTS.index(variant), 61 + exact_corner)
    rng = np.random.default_rng(s)
    wf = G.exact((n, 2, R, R), 3, 0.25, s + 1, G.GW)
    wr = G.exact((n, R, R), 3, 0.25, s + 2, G.GW)
    for l in range(n):
        for k in range(2):
            wf[l, k] = G.cover(G.cover(wf[l, k], 0, s + 3, G.GW), 1, s + 4, G.GW)
        wr[l] = G.cover(G.cover(wr[l], 0, s + 5, G.GW), 1, s + 6, G.GW)
        if exact_corner:
            wr[l, rng.permutation(R)[:R // 4], :] = 0.0
    z = rng.choice(Z_GRID, (n, B * T, R), p=Z_PROB)
    if exact_corner:
        z[:] = 0.0

    def rows(seed):
        v = G.exact((B, T, R), 15, 1.0, seed, GD)
        if B > 1:
            v[:-1, max(T - 2, 0):, :] = 15 * GD * np.sign(v[:-1, max(T - 2, 0):, :])
            v[1:, :2, :] = 15 * GD * np.sign(v[1:, :2, :])
        return v.reshape(B * T, R)

    dcs = np.stack([rows(s + 10 + l) for l in range(n)]) if (variant != "gtop" or exact_corner) else None
    g_top = rows(s + 7) if (variant != "dcs" and not exact_corner) else None
    return dict(wf=wf, wr=wr, z=z, dcs=dcs, g_top=g_top, dil=list(dil), B=B, T=T, R=R)


def check_design(d):
    """Every operand is exact in bf16 (so both modes read the same numbers) and on its grid."""
    for k, grid in (("wf", G.GW), ("wr", G.GW), ("dcs", GD), ("g_top", GG), ("z", 0.5)):
        v = d[k]
        if v is None:
            continue
        assert G.is_bf16(v), k
        assert np.array_equal(v / grid, np.rint(v / grid)) and np.abs(v / grid).max() <= G.INT_MAX, k


# ---- one layer -----------------------------------------------------------------------------------------------------------
def finest_bit(v, w, mode, w_grid=G.GW):
    """-log2 of a common unit of the terms v[t, o] w[i, o] of every entry (t, i): v holds T numbers (multiples of their
    own ulp), w multiples of w_grid; -inf where an entry has no term."""
    with np.errstate(divide="ignore"):
        bits = np.where(v != 0, -np.log2(ulp_of(v, mode)), -np.inf)                   # [rows, o]
    out = np.full((v.shape[0], w.shape[0]), -np.inf)
    for i in range(w.shape[0]):
        nz = w[i] != 0
        if nz.any():
            out[:, i] = bits[:, nz].max(1)
    return out - np.log2(w_grid)


def sums_exactly(S, bits):
    """Every term is a multiple of 2^-bits and the sum of their magnitudes stays within 2^24 such units: every partial
    sum, in any order, is an exact fp32 number."""
    with np.errstate(invalid="ignore", over="ignore"):
        return S * 2.0 ** np.where(np.isfinite(bits), bits, 0.0) <= 2.0 ** 24


def scaled(Gup, mode):
    """(p, a) of the layer below a stored gradient Gup [B T, R] (None: zeros): the fp32 product and the MFMA operand."""
    p = (np.asarray(Gup, np.float64).astype(F32) * SQRT_HALF32).astype(np.float64)
    return p, (G.bf16_round(p) if mode == "bf16" else p)


def layer_df_ref(d, l, Gup, mode):
    """The float64 df of layer l from the stored gradient of the layer above: dict(x = unrounded value, ref = rounded to T,
    e = reach scale, S, dc)."""
    R = d["R"]
    z = d["z"][l]
    dcs = d["dcs"][l] if d["dcs"] is not None else np.zeros_like(z)
    if Gup is None:
        a = np.zeros_like(z)
    else:
        _, a = scaled(Gup, mode)
    dc = dcs + a @ d["wr"][l].T
    Sa = np.abs(a) @ np.abs(d["wr"][l]).T
    S = Sa + np.abs(dcs)
    cp = G.dgate64(z)
    x = dc * cp
    K = (a != 0).astype(np.float64) @ (d["wr"][l] != 0).T.astype(np.float64) + (dcs != 0)      # terms of the entry's own sum
    bits = np.maximum(finest_bit(a, d["wr"][l], mode), np.where(dcs != 0, -np.log2(GD), -np.inf))
    inexact = (Sa > 0) & ~sums_exactly(S, bits)
    e = K * G.EPS * S * np.abs(cp) * inexact + f_abs_z(z, mode) * np.abs(dc) + G.EPS * np.abs(x) * (z != 0)
    return dict(x=x, ref=round_to(x, mode), e=e, dc=dc, S=S)


def taps(d, l, df):
    """(sum_k Wf[k] df[t + (K-1-k) d], S, number of non-zero terms): tap 0 is the delayed one (ops.py:6-10), its adjoint reads df d steps ahead,
    inside the clip."""
    dil, B, T = d["dil"][l], d["B"], d["T"]
    adv = G._advance(df, B, T, dil)
    w0, w1 = d["wf"][l, 0].T, d["wf"][l, 1].T
    nz = lambda v: (v != 0).astype(np.float64)
    return adv @ w0 + df @ w1, np.abs(adv) @ np.abs(w0) + np.abs(df) @ np.abs(w1), nz(adv) @ nz(w0) + nz(df) @ nz(w1)


def layer_G_ref(d, l, Gup, df_stored, mode):
    """The float64 G of layer l from the stored gradient of the layer above and the stored df of this layer."""
    R = d["R"]
    p = np.zeros_like(df_stored) if Gup is None else scaled(Gup, mode)[0]
    t, St, Kt = taps(d, l, df_stored)
    x = p + t
    S = np.abs(p) + St
    dil, B, T = d["dil"][l], d["B"], d["T"]
    with np.errstate(divide="ignore"):
        bits = np.where(p != 0, -np.log2(ulp_of(p, "fp32")), -np.inf)
    bits = np.maximum(bits, np.maximum(finest_bit(G._advance(df_stored, B, T, dil), d["wf"][l, 0], mode),
                                       finest_bit(df_stored, d["wf"][l, 1], mode)))
    e = (Kt + (p != 0)) * G.EPS * S * ((St > 0) & ~sums_exactly(S, bits))
    return dict(x=x, ref=round_to(x, mode), e=e, S=S)


def decided(r, mode, reach):
    """Entries whose rounding to T no admissible evaluation can change."""
    return (r["e"] == 0) | ((r["x"] != 0) & (midpoint_distance(r["x"], mode) > reach * r["e"]))


def bound(r, mode, c):
    """What an undecided entry may differ from the float64 value by."""
    return ulp_of(r["ref"], mode) + c * (G.U_OUT[mode] * np.abs(r["x"]) + r["e"])


def out_ratio(got, r, mode):
    """|got - x| / (u_out |x| + e): what C_CPU["grp_*_out"] is measured as and what the GPU tests print."""
    err = np.abs(np.asarray(got, np.float64) - r["x"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / (G.U_OUT[mode] * np.abs(r["x"]) + r["e"]))


# ---- the float32 restatement (the kernel's stand-in on the CPU) ----------------------------------------------------------
def restate_df32(d, l, Gup, mode):
    """(value before the rounding to T, stored value): fp32 products and sums, one k at a time, dcs first."""
    z = d["z"][l]
    acc = (d["dcs"][l] if d["dcs"] is not None else np.zeros_like(z)).astype(F32)
    if Gup is not None:
        a = scaled(Gup, mode)[1].astype(F32)
        w = d["wr"][l].T.astype(F32)
        for k in range(w.shape[0]):
            acc += a[:, k:k + 1] * w[k:k + 1, :]
    pre = acc * G.dgate32(z, mode)
    assert pre.dtype == F32
    pre = pre.astype(np.float64)
    return pre, round_to(pre, mode)


def restate_G32(d, l, Gup, df_stored, mode):
    dil, B, T = d["dil"][l], d["B"], d["T"]
    acc = (np.zeros_like(df_stored) if Gup is None else scaled(Gup, mode)[0]).astype(F32)
    for src, w in ((G._advance(df_stored, B, T, dil), d["wf"][l, 0].T), (df_stored, d["wf"][l, 1].T)):
        s32, w32 = src.astype(F32), w.astype(F32)
        for k in range(w.shape[0]):
            acc += s32[:, k:k + 1] * w32[k:k + 1, :]
    pre = acc.astype(np.float64)
    return pre, round_to(pre, mode)


def restate_chain(d, mode):
    """The whole group, top layer first, every layer fed with the restatement's own stored values: (df, G) stacks
    [n, B T, R] -- what the kernel's outputs stand in for on a machine without one."""
    n = len(d["dil"])
    df, Gs = [None] * n, [None] * n
    Gup = d["g_top"]
    for l in range(n - 1, -1, -1):
        df[l] = restate_df32(d, l, Gup, mode)[1]
        Gs[l] = restate_G32(d, l, Gup, df[l], mode)[1]
        Gup = Gs[l]
    return np.stack(df), np.stack(Gs)


# ---- the exact corner ----------------------------------------------------------------------------------------------------
def exact_top(d):
    """g_top = None and z = 0: the top layer's df = dcs / 2 and G = the taps of df are sums of dyadic products; returns
    (df, G, S in units of the product grid) in float64, to be rounded once."""
    n = len(d["dil"])
    assert d["g_top"] is None and not d["z"].any()
    df = 0.5 * d["dcs"][n - 1]
    t, St, _ = taps(d, n - 1, df)
    return df, t, St / (0.5 * GD * G.GW)


# Worst ratios of the float32 NumPy restatement on the designs above (tests/test_group_design.py measures them;
# SRWN_PRINT_ERR=1 pytest -s prints the figures), rounded up by G.rounded_up, per mode:
#   measured   grp_df_pre  bf16 1.000  fp32 0.824      grp_G_pre  bf16 0.109  fp32 0.431
#              grp_df_out  bf16 1.992  fp32 0.481      grp_G_out  bf16 1.990  fp32 0.382
# *_pre: |value before the rounding to T - float64| / e (sets REACH); *_out: |stored - float64| / (u_out |ref| + e) (sets
# c; a correctly rounded bf16 output reaches 2 against u_out, see tests/gemm_design.py).  grp_df_pre in bf16 mode is set
# at z = +-1, where the float64 value is 0 and e is the polynomial's own residue times |dc|: the ratio is 1 up to the
# product's rounding, so it is entered as just above 1 (rounded up: 1.5); everywhere else it stays below 0.5.
C_CPU = {"grp_df_pre": {"bf16": 1.5, "fp32": 0.875}, "grp_G_pre": {"bf16": 0.3125, "fp32": 0.4375},
         "grp_df_out": {"bf16": 2.0, "fp32": 0.5}, "grp_G_out": {"bf16": 2.0, "fp32": 0.4375}}
REACH = {k: {m: 4.0 * C_CPU["grp_%s_pre" % k][m] for m in MANT} for k in ("df", "G")}
C_GPU = {k: {m: 4.0 * C_CPU["grp_%s_out" % k][m] for m in MANT} for k in ("df", "G")}


# ---- the forward kernels' weight-gradient tiles --------------------------------------------------------------------------
def ct_decode(flat, nseg, KT, R):
    """The inverse of G.ct_encode: the flat tile image [nseg][KT][R/16][kg 4][channel 16][j 8] -> [nseg, KT, 4, 8, R], element
    (kg, j) of a tile being position kordW(kg, j) of it (csrc/srwn_group.h; G.ct_rows gives its time row)."""
    v = np.asarray(flat)[:nseg * KT * R * 32].reshape(nseg, KT, R // 16, 4, 16, 8)
    return v.transpose(0, 1, 3, 5, 2, 4).reshape(nseg, KT, 4, 8, R)


def tile_written(B, T, st, W):
    """[nseg, KT]: the tiles a segment owns a position of -- the forward kernel writes these whole (zeros beyond the
    segment in xT) and no other."""
    return G.ct_rows(B, T, st, W)[1].any((2, 3))


def fwd_design(dil, B, T, R, cond_pool=None):
    """A forward group on which layer 0's pre-activation is exact (G.fwd_layer at the group's first dilation: one weight
    of +-1/4 per tap and column); deeper layers: sparse weights on the grid 1/8, biases on 1/32.  cond_pool: conditioning
    rows [B, frames, n R] on the grid 1/4 (frames * pool > T, T no multiple of pool)."""
    n = len(dil)
    d0 = G.fwd_layer(R, B, T, dil[0])
    s = G._seed(R, B, T, n, dil[0], dil[-1], 67)
    wf = G.exact((n, 2, R, R), 3, 0.1, s, G.GW)
    wr = G.exact((n, R, R), 3, 0.25, s + 1, G.GW)
    wf[0], wr[0] = d0["wf"], d0["wr"]
    bf = G.exact((n, R), 15, 1.0, s + 2, G.GA * G.GW)
    br = G.exact((n, R), 15, 1.0, s + 3, G.GA * G.GW)
    bf[0], br[0] = d0["bf"], d0["br"]
    out = dict(x=d0["x"], wf=wf, wr=wr, bf=bf, br=br, dil=list(dil), B=B, T=T, R=R, cond=None, frames=1)
    if cond_pool:
        out["frames"] = T // cond_pool + 1
        out["cond"] = G.exact((B, out["frames"], n * R), 3, 1.0, s + 4, G.GA)
    return out


def ic_design(B, T, R):
    """Dyadic audio (|int| <= 7 on 1/16) and a dyadic input conv (kernel +-{1, 2, 3} / 8, bias |int| <= 15 on 1/128):
    x_0[t, c] = b[c] + w[0][c] audio[t - 1 - shift] + w[1][c] audio[t - shift] has at most 57 units of 1/128 -- exact in
    fp32 in any order and exact in bf16."""
    s = G._seed(B, T, R, 71)
    return dict(audio=G.exact((B, T), 7, 0.9, s, 1.0 / 16), w=G.exact((2, R), 3, 1.0, s + 1, G.GW),
                b=G.exact((R,), 15, 1.0, s + 2, 1.0 / 128))


def ic_x0(d, B, T, shift):
    a = d["audio"][:, :, None]
    x = (d["b"] + G.shift_rows(a.reshape(B * T, 1), B, T, 1 + shift) * d["w"][0]
         + G.shift_rows(a.reshape(B * T, 1), B, T, shift) * d["w"][1])
    assert np.array_equal(x * 128, np.rint(x * 128)) and np.abs(x * 128).max() <= G.INT_MAX
    return x


# c = z sigmoid(z) of a tile against the gate of the STORED z.  bf16 mode: the kernel gates the unrounded tanh and stores
# its bf16 rounding, so c differs from gate64(z stored) by the gate's slope (<= 1 on [-1, 1]) times one rounding of z, the
# polynomial's error and c's own rounding; fp32 mode: z is stored as computed and only gate32's error and c's rounding remain.
def gate_scale(z_st, mode):
    c = G.gate64(z_st)
    if mode == "bf16":
        return G.U_OUT[mode] * (np.abs(c) + np.abs(z_st)) + G.POLY_ERR
    return G.U_OUT[mode] * np.abs(c) + G.f_abs_gate32()


def gate_restate32(f, mode):
    """(z stored, c of the tile) from a pre-activation f as the forward kernels form them, in float32 NumPy."""
    if mode == "bf16":
        z = G.tanh_bf16_mode32(f)
        return G.bf16_round(z.astype(np.float64)), G.bf16_round((z * G.sigmoid_poly32(z)).astype(np.float64))
    z = np.tanh(np.asarray(f, F32))
    return z.astype(np.float64), G.gate32(z).astype(np.float64)


# worst |c - gate64(z stored)| / gate_scale of the restatement on 40001 pre-activations in [-3, 3]
# (tests/test_group_design.py): bf16 1.435, fp32 0.846; rounded up by G.rounded_up
C_CPU_GATE = {"bf16": 1.5, "fp32": 0.875}
C_GPU_GATE = {m: 4.0 * v for m, v in C_CPU_GATE.items()}


# ---- srwn_residual_group_bwd_wt: the chain without a stored df, and the layer weight gradients -----------------------------
GX, GC = 0.25, 0.25                           # grids of the tiles' x and c (|int| <= 3 and <= 2, half of the entries zero)


def wt_design(dil, B, T, R, variant="both", exact_corner=False, blocks=False):
    """D.design plus the operands of the weight-gradient tiles, x and c [n, B T, R], every row and column covered, and
    dyadic audio [B, T] for the first group's input conv gradient.  exact_corner: also Wr of the top layer = 0, so that
    df_top = dcs / 2 whatever else, and the top layer's dWf, dbf and the layer below's dWr, dbr are sums of dyadic products;
    blocks: the same with operands so sparse and small that most sums stay within the 256 units a bf16 partial holds."""
    d = design(dil, B, T, R, variant, exact_corner)
    n = len(dil)
    s = G._seed(R, B, T, n, dil[0], 73 + exact_corner)
    rng = np.random.default_rng(s + 50)
    if exact_corner:
        d["wr"][n - 1] = 0.0
    else:
        # df is not stored by this kernel: a G entry is decided only if every df entry it reads is.  So the conv is
        # sparser here (about four weights per row and tap, every row, column and tap still covered) and z stays off
        # +-1, where the bf16 polynomial's residue leaves df undecided (the plain kernel's design keeps both)
        wf = G.exact((n, 2, R, R), 3, 4.0 / R, s + 51, G.GW)
        for l in range(n):
            for k in range(2):
                wf[l, k] = G.cover(G.cover(wf[l, k], 0, s + 52, G.GW), 1, s + 53, G.GW)
        d["wf"] = wf
        d["z"] = rng.choice(np.array([-0.5, 0.0, 0.5]), d["z"].shape, p=[0.2, 0.6, 0.2])
    d["x"] = np.stack([G.cover(G.cover(G.exact((B * T, R), 3, 0.5, s + l, GX), 0, s, GX), 1, s + 1, GX) for l in range(n)])
    d["c"] = np.stack([G.cover(G.cover(G.exact((B * T, R), 2, 0.5, s + 20 + l, GC), 0, s, GC), 1, s + 1, GC) for l in range(n)])
    d["audio"] = G.exact((B, T), 7, 0.9, s + 40, 1.0 / 16)
    if blocks:      # the exact corner for bf16 partial blocks: about six terms of a few units per sum, so that S <= 256 units
        assert exact_corner
        dens = min(1.0, 6.0 / (B * T))
        for k, grid in (("x", GX), ("c", GC)):
            d[k] = np.stack([G.cover(G.cover(G.exact((B * T, R), 1, dens, s + 60 + l, grid), 0, s, grid), 1, s + 1, grid)
                             for l in range(n)])
        d["dcs"] = np.stack([G.exact((B * T, R), 3, 1.0, s + 70 + l, GD) for l in range(n)])
    return d


def through_taps(d, l, u):
    """A per-entry uncertainty u >= 0 of df pushed through |Wf| onto G (both taps)."""
    dil, B, T = d["dil"][l], d["B"], d["T"]
    return G._advance(u, B, T, dil) @ np.abs(d["wf"][l, 0]).T + u @ np.abs(d["wf"][l, 1]).T


def wt_layer_refs(d, l, Gup, mode):
    """One layer of the chain when df is not stored: (df reference, its per-entry uncertainty -- 0 where decided --, G
    reference through the reference df, what the undecided df entries add to G's bound, G's decided entries)."""
    rdf = layer_df_ref(d, l, Gup, mode)
    udf = np.where(decided(rdf, mode, REACH["df"][mode]), 0.0, bound(rdf, mode, C_GPU["df"][mode]) + ulp_of(rdf["ref"], mode))
    rG = layer_G_ref(d, l, Gup, rdf["ref"], mode)
    extra = through_taps(d, l, udf)
    return rdf, udf, rG, extra, decided(rG, mode, REACH["G"][mode]) & (extra == 0)


def wgrad_refs(d, l, Gup, df, udf):
    """The four weight gradients of layer l in float64 from the tiles' operands, the stored gradient of the layer above
    (Gup, None = zero) and this layer's df (reference; udf >= 0 its per-entry uncertainty): {name: (value, S, extra)} --
    dWf [2, R, R] ([tap][x channel][df channel]), dbf [R], dWr [R, R] ([c channel][G channel]), dbr [R]."""
    dil, B, T, R = d["dil"][l], d["B"], d["T"], d["R"]
    x, c = d["x"][l], d["c"][l]
    adv, uadv = G._advance(df, B, T, dil), G._advance(udf, B, T, dil)
    ax = np.abs(x).T
    out = {"dWf": (np.stack([x.T @ adv, x.T @ df]), np.stack([ax @ np.abs(adv), ax @ np.abs(df)]), np.stack([ax @ uadv, ax @ udf])),
           "dbf": (df.sum(0), np.abs(df).sum(0), udf.sum(0))}
    Gu = np.zeros_like(df) if Gup is None else np.asarray(Gup, np.float64)
    out["dWr"] = (c.T @ Gu, np.abs(c).T @ np.abs(Gu), np.zeros((R, R)))
    out["dbr"] = (Gu.sum(0), np.abs(Gu).sum(0), np.zeros(R))
    return out


def ic_refs(d, G0, shift):
    """The input conv's kernel and bias gradient [3, R] from the stored bottom gradient: rows k = 0, 1:
    sum_t audio[t - (1 - k) - shift] G_0[t][c]; row 2: sum_t G_0[t][c]."""
    B, T = d["B"], d["T"]
    a = d["audio"].reshape(B * T, 1)
    taps_ = [G.shift_rows(a, B, T, 1 + shift), G.shift_rows(a, B, T, shift), np.ones_like(a)]
    return (np.stack([(t * G0).sum(0) for t in taps_]), np.stack([(np.abs(t) * np.abs(G0)).sum(0) for t in taps_]))


def wgrad_scale(S, rows, extra, blocks16_roundings=0):
    """rows 2^-24 S + the undecided-df term (+ k roundings of a bf16 partial block: half an ulp is at most 2^-8 of it)."""
    return rows * G.EPS * S + extra + blocks16_roundings * 2.0 ** -8 * S


# worst |fp32 NumPy row-by-row sum - float64| / (rows 2^-24 S) of the weight gradients on the designs
# (tests/test_group_design.py): 0.594 (at B T = 3 rows; 0.1 and less from 31 rows on); rounded up by G.rounded_up
C_CPU_WGRAD = 0.625
C_GPU_WGRAD = 4.0 * C_CPU_WGRAD
