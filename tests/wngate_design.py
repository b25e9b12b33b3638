"""Exact input designs, float64 references, float32 restatements and bound constants for the canonical WaveNet-gate layer
kernels of csrc/srwn_wngate.hip (srwn_wavenet_layer_fwd / _bwd) and for srwn_wgrad at the gate's shapes.  Host code only
(NumPy); tests/test_wngate_design.py checks the designs on the CPU and tests/test_gpu_wngate_entries.py holds the kernels
to them.  Built on tests/gemm_design.py (G): the same operands, range conditions, roundings and bound.

Forward.  x holds integers in [-4, 4], both convolutions one weight per tap and output column, the biases {-1, 0, 1}/4:
the pre-activations f and g are exact on the grid 1/4 (asserted in ``fwd_pre``), so z, s and c = z s are held per entry to
tanh(f), sigmoid(g) and their product with no contraction error at all.
  grid design         the weight is +-1/4: |f|, |g| <= 2.25
  saturation design   the weight is +-1/4, +-16 or +-32 by column: f and g also pass 44.4 (where the exp2 of
                      Math<bf16_t>::tanh_ overflows) and 88.7 (the exp2 of wn_sigmoid<bf16_t>, expf in fp32 mode)
h is held to the layer-local reference (x + c_dev Wr + br) sqrt(1/2) + cond, c_dev being the c the kernel stored.

Backward.
  UP           g2 = sum_k [WfT | WgT][k] D_up[t + (K - 1 - k) d]: dyadic D_up and weights, bit-exact; with a dyadic
               g_in only sqrt(1/2) and the roundings remain: per entry
  DOWN         z in {-1, -1/2, 0, 1/2, 1}, s in {0, 1/4, 1/2, 3/4, 1}, dc exact (a dyadic dcs, or dtotal Ws^T):
               every factor and partial product of dc s (1 - z^2) and dc z s (1 - s) is an exact fp32 number in any
               association (``down_bits``), so both halves of D are bit-exact
  UP + DOWN    g_in = None: the residual operand round_T(float32(G) float32(sqrt(1/2))) is computed exactly here
               (``res_operand``); the Wr product's fp32 accumulation is all that is inexact: D per entry

Clip boundaries: with B >= 2 the last rows of every clip but the last and the first rows of every clip but the first
hold the top of the design's range (x: 4; D_up: 15 where the rest is <= 3): a tap mask wrong by one row moves an entry by
far more than any bound.

Bound for what is not exact, per entry (the project's rule, tests/gemm_design.py):
    |got - ref| <= c (u_out |ref| + K 2^-24 S + f_abs),   c = 4 x C_CPU[key][mode]
f_abs: the absolute error of the float32 restatement of tanh / sigmoid against float64 on the design's own grid
(``f_abs_z``, ``f_abs_s``).  C_CPU: the restatement's worst ratio on the same designs, measured by
tests/test_wngate_design.py, never a figure from a GPU.
"""
import functools

import numpy as np

from tests import gemm_design as G

GA, GW = G.GA, G.GW
SQRT_HALF = G.SQRT_HALF
MODES = ("bf16", "fp32")

# ---- shapes ---------------------------------------------------------------------------------------------------------------
RS = (32, 64)
CLIPS = [(1, 1), (2, 31), (2, 32), (2, 33), (3, 45), (1, 513)]      # (B, T): one row; 31 / 32 / 33; ragged; 17 tiles
BIG = (64, 2049, 33, 32)       # R, B, T, dilation: 4098 tiles > 4 waves x 512 workgroups; every second tile has one valid row
POOL = 8


def dilations(T):
    """1, 31, 32, T - 1, T and 512 wherever they differ for this T."""
    return sorted({d for d in (1, 31, 32, T - 1, T, 512) if d >= 1})


FWD = [(R, B, T, d) for R in RS for (B, T) in CLIPS for d in dilations(T)]
FWD_COND = [(R, B, T, d) for R in RS for (B, T) in CLIPS if T % POOL for d in sorted({1, max(T - 1, 1)})]
BWD_UP = FWD
DOWN = list(G.BWD_DOWN) + [c for c in ((R, 2 * R, B, T) for R in RS for (B, T) in CLIPS) if c not in G.BWD_DOWN]   # R, S, B, T
SKIP_FORMS = ("dcs", "dtotal")
WGRAD_SHAPES = [(64, 128), (32, 64)]                                 # engine._wgrad_wavenet_convs: cin = R, cout = 2R


def _sign(v):
    return np.where(v < 0, -1.0, 1.0)


def _edges(x, top):
    """x [B, T, C]: the last two rows of every clip but the last and the first two rows of every clip but the first take
    magnitude `top`; the first and the last row of every clip carry no zero."""
    T = x.shape[1]
    for r in (0, T - 1):
        x[:, r] = np.where(x[:, r] == 0, 1.0, x[:, r])
    if x.shape[0] > 1:
        x[:-1, max(T - 2, 0):] = top * _sign(x[:-1, max(T - 2, 0):])
        x[1:, :2] = top * _sign(x[1:, :2])
    return x


# ---- forward --------------------------------------------------------------------------------------------------------------
SAT_MAGS = (0.25, 16.0, 32.0)
F_MAX = {False: 2.25, True: 256.25}          # |f|, |g| of the grid / saturation design


def fwd(R, B, T, dil, sat=False, cond=False):
    """x [B T, R] integers in [-4, 4] (edges: see _edges); wf, wg [2, R, R] one entry per tap and output column (+-1/4;
    saturation: +-1/4, +-16, +-32 by column, both taps of a column alike); bf, bg in {-1, 0, 1}/4; wr (1/8, |int| <= 3),
    br (1/32).  cond: [B, frames, 3R], frames = T // 8 + 1, dyadic (1/4, |int| <= 3) in the first R columns and 64 in
    the rest, which the kernel must not read."""
    s = G._seed(R, B, T, dil, 61 + 2 * sat + cond)
    rng = np.random.default_rng(s)
    x = G.exact((B * T, R), 4, 0.9, s + 1, 1.0)
    x = G.cover(G.cover(x, 0, s + 4), 1, s + 5)
    x = _edges(x.reshape(B, T, R), 4.0).reshape(B * T, R)
    out = dict(x=x, wr=G.exact((R, R), 3, 1.0, s + 2, GW), br=G.exact((R,), 15, 1.0, s + 3, GA * GW), cond=None, frames=1)
    for name in ("f", "g"):
        w = np.zeros((2, R, R))
        mag = np.array(SAT_MAGS)[rng.permutation(R) % 3] if sat else np.full(R, 0.25)
        for k in range(2):
            w[k, rng.permutation(R), np.arange(R)] = mag * rng.choice([-1.0, 1.0], R)
        out["w" + name] = w
        out["b" + name] = rng.integers(-1, 2, R) * 0.25
    if cond:
        assert T % POOL
        out["frames"] = T // POOL + 1
        cb = np.full((B, out["frames"], 3 * R), 64.0)
        cb[:, :, :R] = G.exact((B, out["frames"], R), 3, 1.0, s + 6, GA)
        out["cond"] = cb
    return out


def fwd_ops(d, B, T, dil):
    """Both convolutions as one contraction: a [B T, 2R] = [x(t - d) | x(t)], w [2R, 2R] = [Wf | Wg], b = [bf | bg]."""
    a = np.concatenate([G.shift_rows(d["x"], B, T, dil), d["x"]], 1)
    w = np.concatenate([np.concatenate([d["wf"][0], d["wg"][0]], 1), np.concatenate([d["wf"][1], d["wg"][1]], 1)], 0)
    return a, w, np.concatenate([d["bf"], d["bg"]])


def fwd_pre(d, B, T, dil, sat=False):
    """The exact pre-activations (f, g), each [B T, R] (tap 0 is the delayed one)."""
    a, w, b = fwd_ops(d, B, T, dil)
    y = a @ w + b
    assert np.array_equal(y * 4, np.rint(y * 4)) and np.abs(y).max() <= F_MAX[sat]
    R = d["x"].shape[1]
    return y[:, :R], y[:, R:]


def cond_rows(d, B, T):
    """The conditioning rows the kernel adds: [B T, R] (zeros without conditioning)."""
    R = d["x"].shape[1]
    if d["cond"] is None:
        return np.zeros((B * T, R))
    return G.pool_rows(d["cond"][:, :, :R], B, T, POOL)


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def tanh32(x, mode):
    """Math<T>::tanh_ in float32: tanhf ("fp32"), 1 - 2 rcp(exp2(2.885.. x) + 1) ("bf16")."""
    with np.errstate(over="ignore"):
        return np.tanh(np.asarray(x, np.float32)) if mode == "fp32" else G.tanh_bf16_mode32(x)


def sigmoid32(x, mode):
    """wn_sigmoid<T> in float32: 1 / (1 + expf(-x)) ("fp32"), rcp(1 + exp2(-1.4427.. x)) ("bf16")."""
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(over="ignore"):
        e = np.exp(-x) if mode == "fp32" else np.exp2(f(-1.4426950408889634) * x)
        return f(1.0) / (f(1.0) + e)


def _grid(sat):
    n = int(4 * F_MAX[sat]) + 3
    return np.arange(-n, n + 1) / 4.0


@functools.lru_cache(None)
def f_abs_z(mode, sat=False):
    """Worst |tanh32 - tanh| on the design's grid (1/4, |f| <= 3 / <= 257)."""
    g = _grid(sat)
    return float(np.abs(tanh32(g, mode).astype(np.float64) - np.tanh(g)).max())


@functools.lru_cache(None)
def f_abs_s(mode, sat=False):
    g = _grid(sat)
    return float(np.abs(sigmoid32(g, mode).astype(np.float64) - sigmoid64(g)).max())


def f_abs_c(mode, sat=False):
    """c = z s with |z|, |s| <= 1: the two functions' errors add."""
    return f_abs_z(mode, sat) + f_abs_s(mode, sat)


def _out(v, mode):
    v = np.asarray(v, np.float32).astype(np.float64)
    return G.bf16_round(v) if mode == "bf16" else v


def fwd_gate32(f, g, mode):
    """The float32 restatement of the gate: (z, s, c) as stored (float64 arrays, rounded to bf16 in bf16 mode); c is the
    product of the UNROUNDED z and s, as the kernel forms it."""
    z, s = tanh32(f, mode), sigmoid32(g, mode)
    return _out(z, mode), _out(s, mode), _out(z * s, mode)


def h_ref(d, c, B, T):
    """(h, S) of the layer-local reference h = (x + c Wr + br) sqrt(1/2) + cond in float64, for a given stored c."""
    y, S = G.contract(c, d["wr"], d["br"])
    cr = cond_rows(d, B, T)
    return (d["x"] + y) * SQRT_HALF + cr, (np.abs(d["x"]) + S) * SQRT_HALF + np.abs(cr)


def h_restate32(d, c, B, T, mode):
    f = np.float32
    acc = G.eval32(c, d["wr"], d["br"], range(c.shape[1]))
    h = (d["x"].astype(f) + acc) * f(SQRT_HALF) + cond_rows(d, B, T).astype(f)
    return _out(h, mode)


# ---- backward, UP ---------------------------------------------------------------------------------------------------------
def bwd_up(R, B, T, dil):
    """D_up [B T, 2R] (1/4; |int| <= 3, 15 at the clip edges), wf, wg [2, R, R] (1/8, |int| <= 15), g_in [B T, R] (1/4)."""
    s = G._seed(R, B, T, dil, 67)
    D = _edges(G.exact((B, T, 2 * R), 3, 1.0, s, GA) / GA, 15.0).reshape(B * T, 2 * R) * GA
    return dict(D=D, wf=G.exact((2, R, R), 15, 1.0, s + 1, GW), wg=G.exact((2, R, R), 15, 1.0, s + 2, GW),
                g_in=G.exact((B * T, R), 15, 1.0, s + 3, GA))


def bwd_up_ops(d, B, T, dil):
    """a [B T, 4R] = [D_up(t + d) | D_up(t)], w [4R, R] = [Wf[0]^T; Wg[0]^T; Wf[1]^T; Wg[1]^T]."""
    a = np.concatenate([G._advance(d["D"], B, T, dil), d["D"]], 1)
    w = np.concatenate([d["wf"][0].T, d["wg"][0].T, d["wf"][1].T, d["wg"][1].T], 0)
    return a, w


def g2_gin_ref(d, B, T, dil):
    """(g2, S, K) with g_in: g_in sqrt(1/2) + the exact contraction."""
    a, w = bwd_up_ops(d, B, T, dil)
    y, S = G.contract(a, w)
    return d["g_in"] * SQRT_HALF + y, np.abs(d["g_in"]) * SQRT_HALF + S, a.shape[1] + 1


def g2_gin_restate32(d, B, T, dil, mode):
    f = np.float32
    a, w = bwd_up_ops(d, B, T, dil)
    acc = G.eval32(a, w, (d["g_in"].astype(f) * f(SQRT_HALF)).astype(np.float64), range(a.shape[1]))
    return _out(acc, mode)


# ---- backward, DOWN -------------------------------------------------------------------------------------------------------
DOWN_Z = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
DOWN_S = np.array([0.0, 0.25, 0.5, 0.75, 1.0])


def bwd_down(R, S, B, T):
    """z, s [B T, R] drawn from DOWN_Z, DOWN_S; dcs [B T, R] (1/32, |int| <= 255); dtotal [B T, S] (1/4), ws [R, S] (1/8);
    wr [R, R] (1/8, |int| <= 3)."""
    sd = G._seed(R, S, B, T, 71)
    rng = np.random.default_rng(sd + 3)
    return dict(z=rng.choice(DOWN_Z, (B * T, R)), s=rng.choice(DOWN_S, (B * T, R)), dcs=G.exact((B * T, R), 255, 1.0, sd, GA * GW),
                dtotal=G.exact((B * T, S), 15, 1.0, sd + 1, GA), ws=G.exact((R, S), 15, 1.0, sd + 2, GW),
                wr=G.exact((R, R), 3, 1.0, sd + 4, GW))


def down_dc(d, form):
    """The exact dc of a skip form: the dyadic dcs, or dtotal Ws^T."""
    return d["dcs"] if form == "dcs" else d["dtotal"] @ d["ws"].T


def down_bits(dc, z, s):
    """The bit-count condition of the DOWN products: dc is an integer of n bits on the grid 1/32; z is 0 or a power of two
    (no bits), s and 1 - s are k/4 with k <= 3 (two bits each), 1 - z^2 is 0, 3/4 or 1 (two bits): every product of a
    subset of the factors of dc s (1 - z^2) and dc z s (1 - s), in any association, is an integer of at most n + 4 bits
    times a power of two -- an exact fp32 number while n + 4 <= 24 (and 1 - z z is exact with or without an fma).
    Returns n + 4."""
    i = dc / (GA * GW)
    assert np.array_equal(i, np.rint(i))
    assert np.isin(z, DOWN_Z).all() and np.isin(s, DOWN_S).all()
    n = int(np.abs(i).max()).bit_length() + 2 + 2
    assert n <= 24, n
    return n


def down_D(dc, z, s):
    """[dc s (1 - z^2) | dc z s (1 - s)] in float64."""
    return np.concatenate([dc * s * (1.0 - z * z), dc * z * s * (1.0 - s)], 1)


# ---- backward, UP + DOWN --------------------------------------------------------------------------------------------------
def res_operand(Gx, mode):
    """The residual MFMA operand the kernel builds from its accumulators: round_T(float32(G) * float32(sqrt(1/2)))."""
    f = np.float32
    g32 = Gx.astype(f)
    assert np.array_equal(g32.astype(np.float64), Gx)
    return _out(g32 * f(SQRT_HALF), mode)


def updown_ref(up, dn, B, T, dil, form, mode):
    """(G, D, S_D, K): the exact G of the UP part; D of dc = op Wr^T + the skip term, and the bound's S and K per entry
    of D (the gate factors scale S; three more roundings for the elementwise products)."""
    a, w = bwd_up_ops(up, B, T, dil)
    Gx = a @ w
    op = res_operand(Gx, mode)
    y, S = G.contract(op, dn["wr"].T)
    if form == "dcs":
        y, S, K = y + dn["dcs"], S + np.abs(dn["dcs"]), op.shape[1] + 1
    else:
        ys, Ss = G.contract(dn["dtotal"], dn["ws"].T)
        y, S, K = y + ys, S + Ss, op.shape[1] + dn["ws"].shape[1]
    z, s = dn["z"], dn["s"]
    return Gx, down_D(y, z, s), down_D(S, np.abs(z), s), K + 3


def updown_restate32(up, dn, B, T, dil, form, mode):
    """dc accumulated in float32 in the kernel's order (dcs first, the Wr product, the skip product), the gate factors in
    float32, one rounding to the output dtype."""
    f = np.float32
    a, w = bwd_up_ops(up, B, T, dil)
    op = res_operand(a @ w, mode)
    R = op.shape[1]
    acc = G.eval32(op, dn["wr"].T, dn["dcs"] if form == "dcs" else np.zeros_like(dn["dcs"]), range(R))
    if form == "dtotal":
        acc = G.eval32(dn["dtotal"], dn["ws"].T, acc.astype(np.float64), range(dn["ws"].shape[1]))
    z, s = dn["z"].astype(f), dn["s"].astype(f)
    return _out(np.concatenate([acc * s * (f(1.0) - z * z), acc * z * s * (f(1.0) - s)], 1), mode)


# ---- srwn_wgrad at the gate's shapes --------------------------------------------------------------------------------------
def wgrad_dilations(T):
    """One dilation per stacked layer: 1, 31, T - 1 and beyond T."""
    return [1, 31, max(T - 1, 1), T + 3]


def wgrad_cases(slab_rows=3072):
    """(cin, cout, B, T) at G.WGRAD_CLIPS plus the slab-plus-one-row case."""
    return [(cin, cout, B, T) for (cin, cout) in WGRAD_SHAPES for (B, T) in G.wgrad_clips(slab_rows + 1)]


BIG_S = 128


def cases(wgrad_slab_rows=3072):
    """Every contraction the GPU file calls exact, as (name, a, w, b, ga, gw, live): `live` = the k indices whose tap lies
    inside the clip for some row (a tap at d >= T is zero by design); what tests/test_wngate_design.py checks."""
    big = [BIG]
    for sat in (False, True):
        for cond, shapes in ((False, FWD + big), (True, FWD_COND)):
            for (R, B, T, dil) in shapes:
                d = fwd(R, B, T, dil, sat, cond)
                a, w, b = fwd_ops(d, B, T, dil)
                fwd_pre(d, B, T, dil, sat)
                yield ("fwd pre sat %d cond %d R %d B %d T %d d %d" % (sat, cond, R, B, T, dil), a, w, b, 1.0, 0.25,
                       np.arange(0 if dil < T else R, 2 * R))
    for (R, B, T, dil) in BWD_UP + big:
        d = bwd_up(R, B, T, dil)
        a, w = bwd_up_ops(d, B, T, dil)
        yield ("bwd up R %d B %d T %d d %d" % (R, B, T, dil), a, w, None, GA, GW, np.arange(0 if dil < T else 2 * R, 4 * R))
    for (R, S, B, T) in DOWN + [(BIG[0], BIG_S, BIG[1], BIG[2])]:
        d = bwd_down(R, S, B, T)
        yield ("bwd down R %d S %d B %d T %d" % (R, S, B, T), d["dtotal"], d["ws"].T, None, GA, GW, np.arange(S))
    for (cin, cout, B, T) in wgrad_cases(wgrad_slab_rows):
        d = G.wgrad(cin, cout, B, T)
        for l, dil in enumerate(wgrad_dilations(T)):
            for tap, sh in enumerate((dil, 0)):
                a, w = G.wgrad_ops(d["x"][l], d["dy"][l], B, T, sh)
                yield ("wgrad %d %d B %d T %d layer %d tap %d" % (cin, cout, B, T, l, tap), a, w, None, GA, GW,
                       np.arange(B * T) if sh == 0 else None)


# ---- the bound's constants ------------------------------------------------------------------------------------------------
# Worst ratio of the float32 NumPy restatement on the designs above, as tests/test_wngate_design.py measures it
# (SRWN_PRINT_ERR=1 pytest -s prints the figures), rounded up by G.rounded_up:
#   measured (bf16 | fp32)   wn_z 1.265 | 0.568   wn_s 1.349 | 0.581   wn_c 1.814 | 0.609   wn_h 1.989 | 0.111
#                            wn_g2_gin 1.949 | 0.005   wn_D 1.982 | 0.118
# (bf16 outputs: a correctly rounded result reaches 2 against u_out = 2^-9, see tests/gemm_design.py.  fp32 products: K 2^-24 S
# is the worst case of K roundings of one sign; a random design stays one or two orders below it.)
C_CPU = {"wn_z": {"bf16": 1.5, "fp32": 0.625}, "wn_s": {"bf16": 1.5, "fp32": 0.625}, "wn_c": {"bf16": 2.0, "fp32": 0.625},
         "wn_h": {"bf16": 2.0, "fp32": 0.125}, "wn_g2_gin": {"bf16": 2.0, "fp32": 0.0625}, "wn_D": {"bf16": 2.0, "fp32": 0.125}}
C_GPU = {k: {m: 4.0 * v for m, v in c.items()} for k, c in C_CPU.items()}
