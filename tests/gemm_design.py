"""Exact (dyadic) input designs for the contraction kernels, their integer references and the per-entry bound for what is
not exact.  Host code only (NumPy); tests/test_gemm_design.py checks the designs on the CPU and
tests/test_gpu_gemm_entries.py holds the MFMA kernels to them.

Exact designs.  ``exact(shape, values, density, seed, grid)`` draws integers in [-values, values] times one power of two
(the operand's grid), non-zero with probability ``density``.  For y[i, j] = sum_k a[i, k] w[k, j] (+ b[j]) the design
carries its proof obligation, ``check_exact``:

  * operands are exact in bf16: |integer| <= 256 on the grid;
  * S[i, j] = sum_k |a||w| + |b| < 2^22 units of the product grid: every partial sum of every summation order is an
    integer below 2^22 in magnitude, an exact fp32 number with two bits to spare, so the result does not depend on the
    order, the MFMA shape, the slab cut or the wave count;
  * where a kernel stores bf16 partial sums, S <= 256 units: every possible partial is exact in bf16.

The reference is formed in float64 (exact: all integers stay far below 2^53) and rounded ONCE, to nearest-even, to the
output dtype (``round_out``).  A kernel must equal it bit for bit (``same_bits``), in both dtypes.

Gate prologue (c = z sigmoid(z)) in bf16 mode: for z in {-1, 0, +1} the bf16 rounding of c is 0 and two constants that
``gate_constants`` derives from the fp64 sigmoid, asserting that both the fp64 value and the polynomial of
csrc/srwn_common.h lie far (> 100 x the polynomial's quoted 2.7e-6) from the nearest bf16 rounding midpoint.  Gated
bf16 designs are therefore exact on the grid 1/256.

Bound for what is not exact (tanh, the gate in fp32 mode, its derivative, the softmax, sqrt(1/2)), per entry:

    |got - ref| <= c ( u_out |ref| + K 2^-24 S + f_abs )

u_out = half an ulp of the output dtype relative (2^-9 bf16, 2^-24 fp32), S the entry's own sum |a||w|, f_abs the
absolute error of the elementwise function (``f_abs_*``, measured on the float32 restatements below against fp64) carried
to the entry.  c = 4 x the worst ratio the float32 NumPy restatement reaches on the same design (C_CPU, measured by
tests/test_gemm_design.py), never a figure from a GPU.
"""
import numpy as np

U_OUT = {"bf16": 2.0 ** -9, "fp32": 2.0 ** -24}
EPS = 2.0 ** -24
S_MAX = 2 ** 22          # product-grid units
S_MAX16 = 256            # ... where partial sums are stored as bf16
INT_MAX = 256            # operand integers exact in bf16


# ---- operands -----------------------------------------------------------------------------------------------------------
def exact(shape, values, density, seed, grid=1.0):
    """Integers in [-values, values] (non-zero with probability `density`; density 1 = no zeros) times `grid`, float64."""
    assert values <= INT_MAX and np.log2(grid) == int(np.log2(grid))
    rng = np.random.default_rng(seed)
    mag = rng.integers(1, values + 1, shape)
    v = mag * rng.choice([-1, 1], shape)
    if density < 1:
        v = v * (rng.random(shape) < density)
    return v.astype(np.float64) * grid


def cover(a, axis, seed=0, value=1.0):
    """Makes every line of `a` along `axis` carry a non-zero entry (sparse designs): sets one entry of an all-zero line."""
    rng = np.random.default_rng(seed)
    a = np.moveaxis(a, axis, -1)
    flat = a.reshape(-1, a.shape[-1])
    for i in np.nonzero(~flat.any(-1))[0]:
        flat[i, rng.integers(flat.shape[-1])] = value
    return np.moveaxis(flat.reshape(a.shape), -1, axis)


def bf16_bits(x32):
    """float32 -> the uint16 bits of its bf16 rounding (nearest, ties to even; no NaN / inf in the designs)."""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(x):
    """Nearest-even bf16 rounding of float32-exact values, as float64."""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), np.asarray(x, np.float64)), "not a float32 value: double rounding"
    return (bf16_bits(x32).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def is_bf16(x):
    x = np.asarray(x, np.float64)
    return bool(np.array_equal(bf16_round(x.astype(np.float32).astype(np.float64)), x))


def round_out(ref, dtype):
    """The one rounding of an exact reference to the output dtype ("bf16" / "fp32"), as float64."""
    ref = np.asarray(ref, np.float64)
    r32 = ref.astype(np.float32).astype(np.float64)
    assert np.array_equal(r32, ref), "the exact reference must be a float32 number"
    return bf16_round(ref) if dtype == "bf16" else r32


def ties(ref):
    """Entries of an exact reference that lie exactly halfway between two bf16 numbers."""
    ref = np.asarray(ref, np.float64)
    u = np.ascontiguousarray(ref, np.float32).view(np.uint32)
    return (u & 0xFFFF) == 0x8000


def same_bits(got, want):
    """Bit equality of float arrays (their float32 bits); a zero equals a zero of either sign, a NaN equals nothing."""
    g = np.ascontiguousarray(np.asarray(got, np.float64).astype(np.float32)).view(np.uint32)
    w = np.ascontiguousarray(np.asarray(want, np.float64).astype(np.float32)).view(np.uint32)
    zero = ((g << 1) == 0) & ((w << 1) == 0)          # the sign of a zero sum is the order's, not the design's
    return ((g == w) | zero) & ~np.isnan(np.asarray(got, np.float64))


# ---- the contraction and its proof obligation ---------------------------------------------------------------------------
def contract(a, w, b=None):
    """(y, S) in float64: y = a @ w (+ b), S = |a| @ |w| (+ |b|).  Exact for the designs (asserted by check_exact)."""
    y = a @ w
    S = np.abs(a) @ np.abs(w)
    if b is not None:
        y = y + b
        S = S + np.abs(b)
    return y, S


def check_exact(a, w, b, ga, gw, partial16=False):
    """The range conditions of an exact design (a on grid ga, w on gw, b on ga gw); returns S in product-grid units."""
    ia, iw = a / ga, w / gw
    assert np.array_equal(ia, np.rint(ia)) and np.array_equal(iw, np.rint(iw)), "off the grid"
    # exact in bf16: |integer| <= 256 on the grid suffices (what `exact` draws); a stored bf16 intermediate (the r1 of the
    # head chain) is on the grid and exact in bf16 by construction, whatever its size
    assert is_bf16(a) and is_bf16(w)
    S = np.abs(ia) @ np.abs(iw)
    if b is not None:
        ib = b / (ga * gw)
        assert np.array_equal(ib, np.rint(ib)), "bias off the product grid"
        S = S + np.abs(ib)
    assert S.max() < S_MAX, "S = %g units: not below 2^22" % S.max()
    if partial16:
        assert S.max() <= S_MAX16, S.max()
    return S


def check_cover(a, w):
    """Every input row, every k on both sides and every output column carries a non-zero term: a dropped row, column,
    k-slice or tile cannot vanish into zeros."""
    assert np.abs(a).sum(1).min() > 0, "an input row of zeros"
    assert np.abs(a).sum(0).min() > 0 and np.abs(w).sum(1).min() > 0, "a k index without a term"
    assert np.abs(w).sum(0).min() > 0, "an output column without a term"
    # ... and the product itself is non-zero in every output column and for every k (one (i, k, j) term at least)
    assert ((np.abs(a) > 0).astype(np.float64) @ (np.abs(w) > 0).astype(np.float64)).max(0).min() > 0


def eval32(a, w, b, order):
    """The contraction in float32 NumPy, one k at a time in the given order of k (bias first): [M, N] float32."""
    f = np.float32
    a32, w32 = a.astype(f), w.astype(f)
    acc = np.zeros((a.shape[0], w.shape[1]), f) if b is None else np.broadcast_to(b.astype(f), (a.shape[0], w.shape[1])).copy()
    for k in order:
        acc += a32[:, k:k + 1] * w32[k:k + 1, :]
    assert acc.dtype == f
    return acc


def eval32_blocked(a, w, b, block):
    """The same in another association: fp32 partial sums of `block` consecutive k (as a slab or a k-split forms them),
    summed last to first, bias last."""
    f = np.float32
    K = a.shape[1]
    parts = [eval32(a[:, s:s + block], w[s:s + block], None, range(min(block, K - s))[::-1]) for s in range(0, K, block)]
    acc = np.zeros_like(parts[0])
    for p in parts[::-1]:
        acc += p
    if b is not None:
        acc += b.astype(f)
    return acc


def check_order_free(a, w, b, dtype="fp32"):
    """The exactness claim itself, without a GPU: two float32 evaluations in different orders equal the integer reference
    bit for bit (after the one rounding to the output dtype)."""
    y, _ = contract(a, w, b)
    want = round_out(y, dtype)
    K = a.shape[1]
    one = eval32(a, w, b, range(K))
    two = eval32_blocked(a, w, b, 16 if K > 16 else 3)
    for got in (one, two):
        g = got.astype(np.float64)
        g = bf16_round(g) if dtype == "bf16" else g
        assert same_bits(g, want).all()
    return y


# ---- the gate -----------------------------------------------------------------------------------------------------------
POLY_ERR = 2.7e-6        # csrc/srwn_common.h: the quoted error of the bf16-mode sigmoid polynomial


def sigmoid_poly32(x):
    """Math<bf16_t>::sigmoid_ of csrc/srwn_common.h in float32 (fma emulated in float64, rounded once per fma)."""
    f = np.float32
    x = np.asarray(x, f)
    fma = lambda p, q, r: (p.astype(np.float64) * q.astype(np.float64) + np.float64(r)).astype(f)
    u = x * x
    t = fma(u, np.broadcast_to(f(0.00175846), u.shape), f(-0.02067844))
    t = fma(u, t, f(0.24998121))
    return fma(x, t, f(0.5))


def gate_poly32(z):
    """gate_pair: z sigmoid_(z) in float32, rounded to bf16 -> float64."""
    z32 = np.asarray(z, np.float32)
    return bf16_round((z32 * sigmoid_poly32(z32)).astype(np.float64))


def gate64(z):
    z = np.asarray(z, np.float64)
    return z / (1.0 + np.exp(-z))


def gate32(z):
    """gate_of_z<float>: z * (1 / (1 + expf(-z))) in float32."""
    f = np.float32
    z = np.asarray(z, f)
    return z * (f(1.0) / (f(1.0) + np.exp(-z)))


def midpoint_distance(v):
    """Distance of v (float64) to the nearest midpoint between two adjacent bf16 numbers, in absolute terms."""
    v = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(v))
    ulp = 2.0 ** (e - 7)
    frac = (v / ulp) % 1.0
    return np.abs(frac - 0.5) * ulp


def gate_constants():
    """{z: bf16(z sigmoid(z))} for z in (-1, 0, 1), derived from fp64; asserts that the fp64 value and the kernel's
    polynomial both stay > 100 x POLY_ERR away from a rounding midpoint, and that both round to the same constant."""
    out = {0.0: 0.0}
    for z in (-1.0, 1.0):
        c = float(gate64(z))
        c32 = float(np.float32(z) * sigmoid_poly32(np.float32(z)))
        assert midpoint_distance(c) > 100 * POLY_ERR and midpoint_distance(c32) > 100 * POLY_ERR, (z, c, c32)
        assert abs(c - c32) < 2 * POLY_ERR
        r = bf16_round(np.array([np.float64(np.float32(c))])).item()
        assert r == gate_poly32(np.array([z])).item(), (z, r)
        assert r * 256 == round(r * 256) and abs(r * 256) <= INT_MAX       # on the grid 1/256
        out[z] = r
    return out


def gated(z):
    """bf16-mode gate of a z in {-1, 0, 1} design: exact values on the grid 1/256."""
    g = gate_constants()
    z = np.asarray(z, np.float64)
    assert np.isin(z, [-1.0, 0.0, 1.0]).all()
    return np.where(z > 0, g[1.0], np.where(z < 0, g[-1.0], 0.0))


def f_abs_gate32():
    """Worst |gate32 - gate64| on [-1, 1] (the fp32-mode gate prologue's own error), measured on 4001 points."""
    z = np.linspace(-1, 1, 4001)
    return float(np.abs(gate32(z).astype(np.float64) - gate64(z.astype(np.float32).astype(np.float64))).max())


# ---- the bound ----------------------------------------------------------------------------------------------------------
def bound_scale(ref, S, K, dtype, f_abs=0.0):
    """u_out |ref| + K 2^-24 S + f_abs per entry: the bound without its constant c."""
    return U_OUT[dtype] * np.abs(ref) + K * EPS * S + f_abs


def bound(ref, S, K, dtype, f_abs=0.0, c=4.0):
    return c * bound_scale(ref, S, K, dtype, f_abs)


def ratio(got, ref, S, K, dtype, f_abs=0.0):
    """|got - ref| / (the bound's scale), per entry: what C_CPU is measured as and what the GPU tests print."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bound_scale(ref, S, K, dtype, f_abs))      # (0 / 0: an exact entry)


# Worst ratio of the float32 NumPy restatement on the designs of tests/test_gpu_gemm_entries.py, as
# tests/test_gemm_design.py measures it (SRWN_PRINT_ERR=1 pytest -s prints the figures), rounded up (to the next 1/16
# below 1, the next half above) so that another NumPy build's exp (an ulp apart) stays inside:
#   measured   skip_sum_gate_fp32 0.105   wgrad_gate_fp32 0.173 (one-row products; 0.037 at 90 rows)   softmax_dlogits 1.99
#              chain_product 1.97   fwd_z 1.27   fwd_h 1.98   bwd_df 1.99
# (softmax_dlogits, chain_product, fwd_h and bwd_df are set by their bf16 outputs: half an ulp is 2^-9 of the binade's upper end and up to 2^-8 of its lower end, so a
# correctly rounded result reaches a ratio of 2 against u_out = 2^-9.)
# (K 2^-24 S is the worst case of K roundings of one sign; a random design stays an order below it.)
C_CPU = {"skip_sum_gate_fp32": 0.125, "wgrad_gate_fp32": 0.1875, "softmax_dlogits": 2.0, "chain_product": 2.0, "fwd_z": 1.5,
         "fwd_h": 2.0, "bwd_df": 2.0}
C_GPU = {k: 4.0 * v for k, v in C_CPU.items()}


def rounded_up(v):
    """The rounding rule of C_CPU: the next 1/16 below 1, the next half above."""
    step = 16.0 if v < 1 else 2.0
    return float(np.ceil(v * step) / step)


# ---- restatements for the bounded quantities ----------------------------------------------------------------------------
def softmax64(logits):
    m = logits.max(-1, keepdims=True)
    e = np.exp(logits - m)
    return e / e.sum(-1, keepdims=True)


def softmax32(logits):
    f = np.float32
    l = logits.astype(f)
    e = np.exp(l - l.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True, dtype=f)


def dlogits_ref(logits, targets, scale):
    """(softmax - onehot) * scale in fp64 and the bound's S: the entry's own softmax value plus the one-hot (the two
    terms of the difference), times |scale|.  The callers pass K = C (the C-term sum of the normaliser) and no f_abs."""
    p = softmax64(logits)
    oh = np.zeros_like(p); oh[np.arange(len(targets)), targets] = 1.0
    return (p - oh) * scale, (p + oh) * abs(scale), p


def dlogits32(logits, targets, scale, dtype):
    f = np.float32
    p = softmax32(logits)
    oh = np.zeros_like(p); oh[np.arange(len(targets)), targets] = f(1.0)
    d = (p - oh) * f(scale)
    return bf16_round(d.astype(np.float64)) if dtype == "bf16" else d.astype(np.float64)


# ---- shifted rows (weight gradients) ------------------------------------------------------------------------------------
def shift_rows(x, B, T, shift):
    """x [B*T, C] -> row (b, t) holds x[b, t - shift] (0 before the clip start): the delayed tap of a causal conv."""
    x = x.reshape(B, T, -1)
    out = np.zeros_like(x)
    if 0 <= shift < T:
        out[:, shift:] = x[:, :T - shift]
    return out.reshape(B * T, -1)


def pool_rows(cond, B, T, pool):
    """cond [B, frames, C] -> [B*T, C]: frame t // pool for row (b, t)."""
    return np.repeat(cond, pool, axis=1)[:, :T].reshape(B * T, -1)


# ---- the transposed gate tiles srwn_wgrad_skip_wt reads ------------------------------------------------------------------
def _kord():
    kg, j = np.meshgrid(np.arange(4), np.arange(8), indexing="ij")
    return 16 * (kg >> 1) + 2 * (kg & 1) + (j >> 2) + 4 * (j & 3)            # [4, 8]: position of element (kg, j) in a tile


def ct_geometry(B, T, st, W):
    """Segments of a layer whose group runs at stride st with segments of W positions (csrc/srwn_group.h): per segment
    clip b, residue r, first position j0, length wseg; KT tiles of 32 positions each."""
    J = -(-T // st); nsub = -(-J // W); KT = -(-W // 32)
    nseg = B * st * nsub
    seg = np.arange(nseg)
    b, rem = seg // (st * nsub), seg % (st * nsub)
    r, j0 = (rem, np.zeros_like(rem)) if nsub == 1 else (rem // nsub, (rem % nsub) * W)
    Jr = (T - r + st - 1) // st
    wseg = np.clip(np.minimum(Jr - j0, W), 0, None)
    return nseg, KT, b, r, j0, wseg


def ct_rows(B, T, st, W):
    """(row [nseg, KT, 4, 8], ok): the time row b T + r + st (j0 + 32 k + kord(kg, j)) of every tile element, and whether
    it lies inside its segment."""
    nseg, KT, b, r, j0, wseg = ct_geometry(B, T, st, W)
    pos = 32 * np.arange(KT)[None, :, None, None] + _kord()[None, None]
    ok = pos < wseg[:, None, None, None]
    row = b[:, None, None, None] * T + r[:, None, None, None] + st * (j0[:, None, None, None] + pos)
    return np.where(ok, row, -1), ok


def ct_encode(c, B, T, R, st, W, poison):
    """c [B*T, R] -> the flat tile image [nseg][KT][R/16][kg 4][channel 16][j 8]; elements beyond a segment's length hold
    `poison`."""
    row, ok = ct_rows(B, T, st, W)
    nseg, KT = row.shape[:2]
    vals = np.where(ok[..., None], c[np.where(ok, row, 0)], poison)          # [nseg, KT, 4, 8, R]
    vals = vals.reshape(nseg, KT, 4, 8, R // 16, 16).transpose(0, 1, 4, 2, 5, 3)
    return np.ascontiguousarray(vals).reshape(-1)


# ---- the designs the GPU tests use ---------------------------------------------------------------------------------------
# Operand grids differ per operand (1/4, 1/8, ...) so that a kernel cannot pass by treating values as integers; every
# magnitude is <= 15 so that S stays below 2^22 for every K used here (225 K <= 2^22 up to K = 18 641) while sums pass
# 256 units often enough for bf16 outputs to hit rounding ties.
GA, GW = 0.25, 0.125
ROWGEMM_SHAPES = [(64, 256), (256, 256), (256, 32), (32, 64), (64, 96), (128, 128), (256, 128), (64, 128)]
ROWGEMM_ROWS = [1, 31, 32, 33, 257]
ROWGEMM_VALID = [(64, 32, 28), (64, 128, 100)]            # (Cin, cout_pad, cout_valid): cout_valid must be a multiple of 4
SKIPSUM = [(L, R, 4 * R, rows) for L in (1, 5) for R in (32, 64) for rows in (1, 33, 150)]
COLGEMM = [(R, S, L, rows) for (R, S) in ((64, 256), (32, 128)) for L in (1, 3) for rows in (1, 33, 257)]
HEAD_CLASSES = [30, 32, 100, 256]
HEAD_ROWS = 45
WGRAD_SHAPES = [(64, 256), (64, 64), (40, 64), (32, 32)]   # the three block shapes of srwn_wgrad and a ragged cin
YCHUNKS = (3, 64, 16, 200)                                 # L, R, Cin, rows: 200 rows take the one-row-tile launch
KSPLIT = (4, 128, 256, 33)                                 # L, channels per slice, S, rows
WGRAD_COND = (2, 45, 64, 64, 3)                            # B, T, cin, cout, shift
WGRAD_POOLS = [(8, 6), (16, 3)]                            # (pool_stride, frames): frames * pool > T = 45, no divisor of it
WGRAD_CLIPS = [(1, 1), (1, 31), (1, 32), (1, 33), (2, 45)]  # (B, T); + one slab plus one row, from srwn_wgrad_slabs


def _seed(*k):
    return int(sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) % (2 ** 31))


def rowgemm(Cin, Cout, rows):
    """x [rows, Cin] (grid 1/4), w [Cin, Cout] (1/8), b [Cout] (1/32), aux [rows, Cout] with zeros of both signs."""
    s = _seed(Cin, Cout, rows)
    x = exact((rows, Cin), 15, 1.0, s, GA)
    w = exact((Cin, Cout), 15, 1.0, s + 1, GW)
    b = exact((Cout,), 15, 1.0, s + 2, GA * GW)
    aux = exact((rows, Cout), 3, 0.6, s + 3, GA)
    aux = np.where((aux == 0) & (np.random.default_rng(s + 4).random(aux.shape) < 0.5), -0.0, aux)
    return dict(x=x, w=w, b=b, aux=aux)


def skipsum(L, R, S, rows):
    """z [L, rows, R] in {-1, 0, 1}, w [L R, S] (1/8), b [S] on the product grid 2^-11."""
    s = _seed(L, R, S, rows, 5)
    z = exact((L, rows, R), 1, 0.8 if rows > 1 else 1.0, s, 1.0)      # (one row: a zero would leave its k without a term)
    z = cover(z, 1, s + 3)
    w = exact((L * R, S), 7, 1.0, s + 1, GW)
    b = exact((S,), 15, 1.0, s + 2, GW / 256)
    return dict(z=z, w=w, b=b)


def skipsum_a(z):
    """[L, rows, R] -> the [rows, L R] operand of the contraction."""
    return np.transpose(z, (1, 0, 2)).reshape(z.shape[1], -1)


def colgemm(R, S, L, rows):
    """d [rows, S] (1/4), ws [L, R, S] (1/8): dcs[l] = d @ ws[l].T."""
    s = _seed(R, S, L, rows, 9)
    return dict(d=exact((rows, S), 15, 1.0, s, GA), ws=exact((L, R, S), 15, 1.0, s + 1, GW))


def head(C, rows=HEAD_ROWS, S=64):
    """x [rows, S] (1/4), w [S, C] (1/8), b [C] (1/32), targets [rows]: logits of a few units, as a trained head's."""
    s = _seed(C, rows, S, 11)
    rng = np.random.default_rng(s + 3)
    return dict(x=exact((rows, S), 3, 1.0, s, GA), w=exact((S, C), 3, 1.0, s + 1, GW), b=exact((C,), 15, 1.0, s + 2, GA * GW),
                tg=rng.integers(0, C, rows).astype(np.int32))


def wgrad_clips(slab_plus_one):
    """(B, T) of WGRAD_CLIPS and the factorisation of `slab_plus_one` rows into B clips of an odd T."""
    n = int(slab_plus_one)
    for B in (7, 3, 5, 11, 13, 1):
        if n % B == 0:
            return WGRAD_CLIPS + [(B, n // B)]


def wgrad_shifts(T):
    return [0, 1, max(T - 1, 0), T + 3]


def wgrad(cin, cout, B, T, nbatch=4, gate=False):
    """x [nbatch, B T, cin] (1/4; z in {-1, 0, 1} when gated), dy [nbatch, B T, cout] (1/8).  The last rows of every clip
    but the last hold values of 15 where the rest holds |v| <= 3: a shifted tap that reads across a clip start shows."""
    s = _seed(cin, cout, B, T, 13 + gate)
    rows = B * T
    if gate:
        x = cover(cover(exact((nbatch, rows, cin), 1, 0.8, s, 1.0), 1, s + 2), 2, s + 3)
    else:
        x = exact((nbatch, B, T, cin), 3, 1.0, s, GA)
        if B > 1:
            x[:, :-1, max(T - 2, 0):, :] = 15 * GA * np.sign(x[:, :-1, max(T - 2, 0):, :])
        x = x.reshape(nbatch, rows, cin)
    dy = exact((nbatch, rows, cout), 3, 1.0, s + 1, GW)
    return dict(x=x, dy=dy)


def wgrad_cond(cin, cout, B, T, pool, frames):
    """x + cond exact in bf16: x (grid 1/4, |int| <= 3) + cond [B, frames, cin] (grid 1/4, |int| <= 3) has |int| <= 6."""
    s = _seed(cin, cout, B, T, pool, 17)
    return dict(x=exact((1, B * T, cin), 3, 1.0, s, GA), dy=exact((1, B * T, cout), 3, 1.0, s + 1, GW),
                cond=exact((B, frames, cin), 3, 1.0, s + 2, GA))


def ksplit(L, EC, S, rows):
    """x [L, rows, EC] (1/4), w [L EC, S] (1/8), b [S] (1/32): slice l of the split contracts chunk l."""
    s = _seed(L, EC, S, rows, 19)
    return dict(x=exact((L, rows, EC), 15, 1.0, s, GA), w=exact((L * EC, S), 15, 1.0, s + 1, GW),
                b=exact((S,), 15, 1.0, s + 2, GA * GW))


def wgrad_ops(x, dy, B, T, shift):
    """The contraction's operands: a = shifted x transposed [cin, rows], w = dy [rows, cout]."""
    return shift_rows(x, B, T, shift).T, dy


WIDE = [("stack", 64, 256, 6), ("stack", 64, 256, 8), ("stack", 32, 128, 6), ("stack", 32, 256, 10),
        ("flat", 64, 256, 4), ("flat", 64, 128, 2)]      # (mode, chunk width, D width, chunks): 8 x 64 takes 4 chunks per block
WIDE_ROWS = [1, 31, 32, 33]                               # + one slab plus one row, from srwn_wgrad_wide_slabs
# (R, B, T, pool, nslabs; None = srwn_wgrad_slabs(rows), 1 here): ragged clips, conditioning, one row and 31 / 32 / 33 rows
# for both row-staging widths (R = 64: 32 rows per step, R = 32: 64), and two / three slabs whose last one is ragged
LAYERS = ([(64, 2, 45, None, None), (32, 2, 45, None, None), (64, 2, 600, None, None), (64, 2, 45, 8, None), (32, 2, 45, 16, None)]
          + [(R, 1, T, None, None) for R in (64, 32) for T in (1, 31, 32, 33)]
          + [(64, 2, 45, None, 2), (32, 2, 45, None, 2), (64, 2, 600, None, 3), (32, 2, 600, 16, 3)])
CHAIN_ROWS = [1, 32, 33, 100]
BWD_UP = [(R, B, T, d) for R in (32, 64) for (B, T) in ((2, 33), (1, 100)) for d in (1, 32, 512)]


def layer_dilations(T):
    return [1, 31, 512, T + 5]


WIDE_PAIR_ROWS = [1, 31, 32, 33, 257]


def wide(mode, cw, dw, L, rows, variant=0):
    """stack: z [L, rows, cw] in {-1, 0, 1} (gated in the prologue); flat: a [rows, L cw] (1/4).  d [rows, dw] (1/8)."""
    s = _seed(cw, dw, L, rows, 23 + (mode == "flat"), variant)
    d = exact((rows, dw), 3, 1.0, s + 1, GW)
    if mode == "stack":
        z = exact((L, rows, cw), 1, 0.8 if rows > 1 else 1.0, s, 1.0)
        return dict(a=cover(z, 1, s + 2), d=d)
    return dict(a=exact((rows, L * cw), 3, 1.0, s, GA), d=d)


def layers(R, B, T, pool, L=4):
    """srwn_wgrad_layers: x (1/4), z in {-1, 0, 1}, df and g (1/8) as [L, B T, R] stacks; cond [B frames, L R] (1/4) with
    frames = T // pool + 1 (frames * pool > T, T no multiple of pool).  Large values before every clip start."""
    s = _seed(R, B, T, pool or 0, 29)
    rows = B * T
    x = exact((L, B, T, R), 3, 1.0, s, GA)
    x[:, :-1, max(T - 2, 0):, :] = 15 * GA * np.sign(x[:, :-1, max(T - 2, 0):, :])
    out = dict(x=x.reshape(L, rows, R), z=cover(cover(exact((L, rows, R), 1, 0.8, s + 1, 1.0), 1, s + 5), 2, s + 6),
               df=exact((L, rows, R), 3, 1.0, s + 2, GW), g=exact((L, rows, R), 3, 1.0, s + 3, GW), cond=None, frames=1)
    if pool:
        out["frames"] = T // pool + 1
        out["cond"] = exact((B * out["frames"], L * R), 3, 1.0, s + 4, GA)
    return out


def layers_xin(d, l, B, T, R, pool):
    """Layer l's conv input: x (+ its conditioning rows)."""
    if d["cond"] is None:
        return d["x"][l]
    cb = d["cond"].reshape(B, d["frames"], -1, R)[:, :, l, :]
    return d["x"][l] + pool_rows(cb, B, T, pool)


def layers_ops(d, l, B, T, R, pool, dil):
    """The three contractions of layer l as (a, w): delayed tap, current tap, residual 1x1 (c = gated z, bf16 mode)."""
    xin = layers_xin(d, l, B, T, R, pool)
    return [(shift_rows(xin, B, T, dil).T, d["df"][l]), (xin.T, d["df"][l]), (gated(d["z"][l]).T, d["g"][l])]


def chain(rows, C=256, S=256):
    """srwn_head_chain: r0 [rows, S] >= 0 with a third exact zeros (1/4), W1 [S, S] and W2 [S, 256] (1/8, columns from C on
    zero), b2 (1/256, zero from C on), targets; b1 on the grid 1/32 chosen so that the pre-activation of r1 is EXACTLY 0 at
    (row j mod rows, column j) for every second j: ties of the mask (r1 > 0) at 0."""
    s = _seed(rows, C, S, 31)
    rng = np.random.default_rng(s + 5)
    r0 = np.abs(exact((rows, S), 7, 0.67, s, GA))
    r0 = cover(r0, 1, s + 7, GA)
    w1 = exact((S, S), 7, 1.0, s + 1, GW)         # pre-activations of a few hundred units: bf16 ties in r1
    w2 = cover(cover(exact((S, 256), 1, 0.1, s + 2, GW), 0, s + 8, GW), 1, s + 9, GW)    # sparse: logits of a few units
    w2[:, C:] = 0.0
    b1 = exact((S,), 15, 1.0, s + 3, GA * GW)
    j = np.arange(0, S, 2)
    b1[j] = -(r0[j % rows] * w1[:, j].T).sum(-1)
    b2 = exact((256,), 15, 1.0, s + 4, 1.0 / 256)
    b2[C:] = 0.0
    return dict(r0=r0, w1=w1, w2=w2, b1=b1, b2=b2, tg=rng.integers(0, C, rows).astype(np.int32))


def chain_forward(d):
    """(pre-activation, r1 as stored in bf16, logits): all exact -- r1's bf16 rounding keeps it on the grid 1/32 and the
    second product's sums stay in range (asserted through cases())."""
    pre, _ = contract(d["r0"], d["w1"], d["b1"])
    r1 = round_out(np.maximum(pre, 0.0), "bf16")
    logits, _ = contract(r1, d["w2"], d["b2"])
    return pre, r1, logits


def bwd_up(R, B, T, dil):
    """The UP-only output of srwn_residual_layer_bwd: g2[t] = df_up[t + d] Wf[0]^T + df_up[t] Wf[1]^T (ops.py:6-20's
    adjoint; K = 2).  df_up [B T, R] (1/4), wf [2, R, R] (1/8)."""
    s = _seed(R, B, T, dil, 37)
    return dict(df=exact((B * T, R), 15, 1.0, s, GA), wf=exact((2, R, R), 15, 1.0, s + 1, GW))


def bwd_up_ops(d, B, T, dil):
    a = np.concatenate([_advance(d["df"], B, T, dil), d["df"]], 1)
    w = np.concatenate([d["wf"][0].T, d["wf"][1].T], 0)
    return a, w


def _advance(x, B, T, d):
    """row (b, t) holds x[b, t + d] (0 behind the clip end)."""
    x = x.reshape(B, T, -1)
    out = np.zeros_like(x)
    if d < T:
        out[:, :T - d] = x[:, d:]
    return out.reshape(B * T, -1)


SKIP_WT = [(2, 77, [1, 1, 4, 32], [40, 40, 33, 40]),       # (B, T, st per layer, segment length per layer): blocks of 2, 1, 1
           (2, 45, [4, 4, 4, 4], [33, 33, 33, 33]),          # layers; one block of four (no idle wave: the column-sum kernel)
           (1, 100, [32, 1], [32, 100])]
CT_POISON = 256.0                                           # tile elements beyond a segment: finite, large, must not count


def skip_wt(B, T, L, part16):
    """srwn_wgrad_skip_wt: c [L, B T, 64] in {0, +-1, +-2} (grid 1), d [B T, 256] (1/8); part16: sparse, so that S <= 256."""
    s = _seed(B, T, L, 41 + part16)
    dens = 0.3 if part16 else 0.8
    c = exact((L, B * T, 64), 2, dens, s, 1.0)
    d = exact((B * T, 256), 3, dens if part16 else 1.0, s + 1, GW)
    return dict(c=cover(cover(c, 1, s + 2), 2, s + 3), d=cover(cover(d, 0, s + 4, GW), 1, s + 5, GW))


TAP = (3, 100, 128, 25)                                    # B, T, Cin, pool: the shapes of tests/test_gpu_autoencoder.py
NC = (3, 2, 173, 128, 5)                                   # L, B, T, C, slabs


def tap(cout):
    """srwn_tap_linear: x [B T, Cin] (1/4), w [2, Cin, cout] (1/8), b (1/32), aux, fadd [B frames, cout + 64] on the grid
    1/16 (it enters times 1/2: on the product grid)."""
    B, T, Cin, pool = TAP
    s = _seed(cout, 43)
    aux = exact((B * T, cout), 3, 0.6, s + 3, GA)
    aux = np.where((aux == 0) & (np.random.default_rng(s + 5).random(aux.shape) < 0.5), -0.0, aux)
    return dict(x=exact((B * T, Cin), 15, 1.0, s, GA), w=exact((2, Cin, cout), 15, 1.0, s + 1, GW),
                b=exact((cout,), 15, 1.0, s + 2, GA * GW), aux=aux, fadd=exact((B * (T // pool), cout + 64), 15, 1.0, s + 4, 2 * GA * GW))


def tap_ops(d, step):
    """Both taps as one contraction: tap k reads row t + k step inside the clip."""
    B, T, Cin, pool = TAP
    other = _advance(d["x"], B, T, 1) if step > 0 else shift_rows(d["x"], B, T, 1)
    return np.concatenate([d["x"], other], 1), np.concatenate([d["w"][0], d["w"][1]], 0)


def nc():
    """srwn_wgrad_nc_layers: r, a (1/4) and dpre, dh (1/8) as [L, B T, C] stacks."""
    L, B, T, C, ns = NC
    s = _seed(L, B, T, C, 47)
    return dict(r=exact((L, B * T, C), 3, 1.0, s, GA), a=exact((L, B * T, C), 3, 1.0, s + 1, GA),
                dp=exact((L, B * T, C), 3, 1.0, s + 2, GW), dh=exact((L, B * T, C), 3, 1.0, s + 3, GW))


def nc_ops(d, l):
    """Layer l's three contractions (a, w): tap 0 (r[t] dpre[t]), tap 1 (r[t + 1] dpre[t], inside the clip), the 1x1."""
    L, B, T, C, ns = NC
    return [(d["r"][l].T, d["dp"][l]), (_advance(d["r"][l], B, T, 1).T, d["dp"][l]), (d["a"][l].T, d["dh"][l])]


# ---- srwn_residual_layer_fwd: an exact pre-activation -------------------------------------------------------------------
FWD = [(R, B, T, d) for R in (32, 64) for (B, T, d) in ((2, 33, 1), (1, 33, 32), (1, 513, 512), (1, 513, 32))]
SQRT_HALF = float(np.sqrt(0.5))


def tanh_bf16_mode32(x):
    """Math<bf16_t>::tanh_ in float32: 1 - 2 / (exp2(x * 2.88539...) + 1)."""
    f = np.float32
    x = np.asarray(x, f)
    e = np.exp2(x * f(2.8853900817779268))
    return f(1.0) - f(2.0) * (f(1.0) / (e + f(1.0)))


def fwd_layer(R, B, T, dil):
    """x [B T, R] integers in [-4, 4]; both conv taps one entry of +-1/4 per output column; bias in {-1, 0, 1} / 4: the
    pre-activation f = x[t, p(o)] s1 / 4 + x[t - d, q(o)] s0 / 4 + bf[o] is exact, on the grid 1/4, in [-2.25, 2.25].
    wr [R, R] (1/8, |int| <= 3), br (1/32)."""
    s = _seed(R, B, T, dil, 53)
    rng = np.random.default_rng(s)
    x = exact((B * T, R), 4, 0.9, s + 1, 1.0)
    wf = np.zeros((2, R, R))
    for k in range(2):
        wf[k, rng.permutation(R), np.arange(R)] = rng.choice([-0.25, 0.25], R)
    bf = rng.integers(-1, 2, R) * 0.25
    return dict(x=x, wf=wf, bf=bf, wr=exact((R, R), 3, 1.0, s + 2, GW), br=exact((R,), 15, 1.0, s + 3, GA * GW))


def fwd_pre(d, B, T, dil):
    """The exact pre-activation f [B T, R] (tap 0 is the delayed one, ops.py:6-20)."""
    f = shift_rows(d["x"], B, T, dil) @ d["wf"][0] + d["x"] @ d["wf"][1] + d["bf"]
    assert np.array_equal(f * 4, np.rint(f * 4)) and np.abs(f).max() <= 3.0
    return f


def fwd_c_bf16(f):
    """bf16 mode: the c entering the residual 1x1 = bf16(z sigmoid(z)), z = tanh(f) unrounded (csrc/srwn_fwd.hip rounds c
    where it builds the MFMA operand).  f takes the 19 values of the grid 1/4 in [-2.25, 2.25]; each one's c lies further
    than 4 x the polynomial's 2.7e-6 from a bf16 rounding midpoint (the nearest: 6.5e-5, at f = -1.5), in fp64 and in the
    float32 restatement alike, so the rounded c is the same whichever implementation of tanh formed it, and the residual
    product of bf16 mode is exact."""
    z64 = np.tanh(f)
    c64 = z64 / (1.0 + np.exp(-z64))
    z32 = tanh_bf16_mode32(f)
    c32 = (z32 * sigmoid_poly32(z32)).astype(np.float64)
    nz = c64 != 0
    assert (midpoint_distance(c64[nz]) > 4 * POLY_ERR).all() and (midpoint_distance(c32[nz]) > 4 * POLY_ERR).all()
    assert np.abs(c64 - c32).max() < 2 * POLY_ERR
    cq = bf16_round(c32)
    assert np.array_equal(cq, bf16_round(c64.astype(np.float32).astype(np.float64)))
    return cq


def fwd_h_ref(d, f, mode):
    """(h, S, f_abs) of h = (x + c Wr + br) sqrt(1/2) in fp64: c = the bf16 values of fwd_c_bf16 ("bf16") or the fp64 gate
    ("fp32": f_abs carries the float32 error of tanh and the gate through |Wr|)."""
    if mode == "bf16":
        c, fa = fwd_c_bf16(f), 0.0
    else:
        z = np.tanh(f)
        c = gate64(z)
        g = np.arange(-12, 13) / 4.0
        e = np.abs(gate32(np.tanh(g.astype(np.float32))).astype(np.float64) - gate64(np.tanh(g))).max()
        fa = e * np.abs(d["wr"]).sum(0) * SQRT_HALF
    y, S = contract(c, d["wr"], d["br"])
    return (d["x"] + y) * SQRT_HALF, (np.abs(d["x"]) + S) * SQRT_HALF, fa


def fwd_restate32(d, f, mode):
    """The float32 restatement of the layer: (z, h) as float64 arrays, rounded to bf16 in bf16 mode."""
    f32 = np.float32
    if mode == "bf16":
        z = tanh_bf16_mode32(f)
        c = bf16_round((z * sigmoid_poly32(z)).astype(np.float64))
    else:
        z = np.tanh(f.astype(f32))
        c = gate32(z).astype(np.float64)
    acc = eval32(c, d["wr"], d["br"], range(c.shape[1]))
    h = (d["x"].astype(f32) + acc) * f32(SQRT_HALF)
    z, h = z.astype(np.float64), h.astype(np.float64)
    return (bf16_round(z), bf16_round(h)) if mode == "bf16" else (z, h)


def f_abs_tanh(mode):
    """Worst |float32 restatement - fp64| of tanh on the grid 1/4 in [-3, 3]: "fp32" np.tanh in float32, "bf16" the
    exp2 / reciprocal form of Math<bf16_t>::tanh_."""
    g = np.arange(-12, 13) / 4.0
    got = np.tanh(g.astype(np.float32)) if mode == "fp32" else tanh_bf16_mode32(g)
    return float(np.abs(got.astype(np.float64) - np.tanh(g)).max())


# ---- srwn_residual_layer_bwd, DOWN only: df = (dtotal Ws^T) d(z sigmoid z)/df ------------------------------------------
BWD_DOWN = [(64, 256, 2, 33), (32, 128, 1, 100), (32, 64, 2, 33)]       # R, S, B, T
BWD_Z = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])


def dgate64(z):
    z = np.asarray(z, np.float64)
    sg = 1.0 / (1.0 + np.exp(-z))
    return (sg + z * sg * (1.0 - sg)) * (1.0 - z * z)


def dgate32(z, mode):
    """dgate_df<float> (expf form) / dgate_df<bf16_t> (one polynomial, fma emulated in float64) of csrc/srwn_common.h in
    float32."""
    f = np.float32
    z = np.asarray(z, f)
    if mode == "fp32":
        sg = f(1.0) / (f(1.0) + np.exp(-z))
        return (sg + z * sg * (f(1.0) - sg)) * (f(1.0) - z * z)
    fma = lambda p, q, r: (np.asarray(p, np.float64) * np.asarray(q, np.float64) + np.asarray(r, np.float64)).astype(f)
    u = z * z
    r = fma(u, f(0.00142598), f(-0.01381972))
    for cst in (0.0957148, -0.5833199, 0.49999976):
        r = fma(u, r, f(cst))
    return fma(z, r, fma(u, f(-0.5), f(0.5)))


def f_abs_dgate(mode):
    """Worst |dgate32 - dgate64| over the z of the design (bf16: the polynomial's error, 9e-7 by the header)."""
    return float(np.abs(dgate32(BWD_Z, mode).astype(np.float64) - dgate64(BWD_Z)).max())


def bwd_down(R, S, B, T):
    """dtotal [B T, S] (1/4), ws [R, S] (1/8), z [B T, R] drawn from BWD_Z: dc = dtotal ws^T is exact; dgate(0) = 1/2 makes
    df exact where z = 0, dgate(+-1) = 0 bounds df absolutely there."""
    s = _seed(R, S, B, T, 59)
    rng = np.random.default_rng(s + 2)
    return dict(d=exact((B * T, S), 15, 1.0, s, GA), ws=exact((R, S), 15, 1.0, s + 1, GW), z=rng.choice(BWD_Z, (B * T, R)))


def cases(wgrad_slab_rows=3072, wide_slab_rows=256):
    """Every exact contraction the GPU file runs, as (name, a, w, b, ga, gw, bf16_out, part16, full): what
    tests/test_gemm_design.py checks on the CPU; `full` = no operand row or column is zero by design (a shifted tap's
    first rows are).  The slab lengths are the entry points' (asserted on the GPU)."""
    for (Cin, Cout) in ROWGEMM_SHAPES:
        for rows in ROWGEMM_ROWS:
            d = rowgemm(Cin, Cout, rows)
            yield ("rowgemm %d %d %d" % (Cin, Cout, rows), d["x"], d["w"], d["b"], GA, GW, True, False, True)
    for (Cin, Cp, Cv) in ROWGEMM_VALID:
        d = rowgemm(Cin, Cp, 33)
        yield ("rowgemm valid %d of %d" % (Cv, Cp), d["x"], d["w"][:, :Cv], d["b"][:Cv], GA, GW, True, False, True)
    for (L, R, S, rows) in SKIPSUM:
        d = skipsum(L, R, S, rows)
        yield ("skipsum %d %d %d" % (L, R, rows), gated(skipsum_a(d["z"])), d["w"], d["b"], 1.0 / 256, GW, True, False, True)
    for (R, S, L, rows) in COLGEMM:
        d = colgemm(R, S, L, rows)
        for l in range(L):
            yield ("colgemm %d %d %d/%d %d" % (R, S, l, L, rows), d["d"], d["ws"][l].T, None, GA, GW, True, False, True)
    for C in HEAD_CLASSES:
        d = head(C)
        yield ("head %d" % C, d["x"], d["w"], d["b"], GA, GW, False, False, True)
    for (cin, cout) in WGRAD_SHAPES:
        for (B, T) in wgrad_clips(wgrad_slab_rows + 1):
            d = wgrad(cin, cout, B, T)
            for l, sh in enumerate(wgrad_shifts(T)):
                a, w = wgrad_ops(d["x"][l], d["dy"][l], B, T, sh)
                yield ("wgrad %d %d B%d T%d tap %d shift %d" % (cin, cout, B, T, l, sh), a, w, None, GA, GW, False, False, sh == 0)
    L, R, Cin, rows = YCHUNKS
    d = rowgemm(Cin, L * R, rows)
    yield ("ychunks", d["x"], d["w"], d["b"], GA, GW, True, False, True)
    L, EC, S, rows = KSPLIT
    d = ksplit(L, EC, S, rows)
    yield ("ksplit", skipsum_a(d["x"]), d["w"], d["b"], GA, GW, False, False, True)
    B, T, cin, cout, shift = WGRAD_COND
    for pool, frames in WGRAD_POOLS:
        d = wgrad_cond(cin, cout, B, T, pool, frames)
        xin = d["x"][0] + pool_rows(d["cond"], B, T, pool)
        a, w = wgrad_ops(xin, d["dy"][0], B, T, shift)
        yield ("wgrad cond pool %d" % pool, a, w, None, GA, GW, False, False, False)
    d = wgrad(64, 64, 2, 45, gate=True)
    for l, sh in enumerate(wgrad_shifts(45)):
        a, w = wgrad_ops(gated(d["x"][l]), d["dy"][l], 2, 45, sh)
        yield ("wgrad gate shift %d" % sh, a, w, None, 1.0 / 256, GW, False, False, sh == 0)
    for (mode, cw, dw, L) in WIDE:
        for rows in WIDE_ROWS + [wide_slab_rows + 1]:
            d = wide(mode, cw, dw, L, rows)
            if mode == "stack":
                yield ("wide stack %d %d %d rows %d" % (cw, dw, L, rows), gated(skipsum_a(d["a"])).T, d["d"], None, 1.0 / 256,
                       GW, False, False, True)
            else:
                yield ("wide flat %d %d %d rows %d" % (cw, dw, L, rows), d["a"].T, d["d"], None, GA, GW, False, False, True)
    for rows in WIDE_PAIR_ROWS:
        d = wide("flat", 64, 256, 4, rows, variant=1)
        yield ("wide pair second product rows %d" % rows, d["a"].T, d["d"], None, GA, GW, False, False, True)
    for (R, B, T, pool, ns) in LAYERS:
        d = layers(R, B, T, pool)
        for l, dil in enumerate(layer_dilations(T)):
            for n, (a, w) in enumerate(layers_ops(d, l, B, T, R, pool, dil)):
                yield ("layers %d %d %d %s slabs %s layer %d product %d" % (R, B, T, pool, ns, l, n), a, w, None,
                       1.0 / 256 if n == 2 else GA, GW, False, False, n > 0)
    for rows in CHAIN_ROWS:
        for C in (256, 250):
            d = chain(rows, C)
            pre, r1, logits = chain_forward(d)
            yield ("chain r1 rows %d C %d" % (rows, C), d["r0"], d["w1"], d["b1"], GA, GW, True, False, False)
            yield ("chain logits rows %d C %d" % (rows, C), r1, d["w2"][:, :C], d["b2"][:C], GA * GW, GW, False, False, False)
    for (B, T, st, seg) in SKIP_WT:
        for part16 in (False, True):
            d = skip_wt(B, T, len(st), part16)
            for l in range(len(st)):
                yield ("skip_wt B %d T %d layer %d part16 %d" % (B, T, l, part16), d["c"][l].T, d["d"], None, 1.0, GW, False,
                       part16, True)
    for (R, S, B, T) in BWD_DOWN:
        d = bwd_down(R, S, B, T)
        yield ("bwd down %d %d %d %d" % (R, S, B, T), d["d"], d["ws"].T, None, GA, GW, True, False, True)
    for (R, B, T, dil) in FWD:
        d = fwd_layer(R, B, T, dil)
        f = fwd_pre(d, B, T, dil)
        a = np.concatenate([shift_rows(d["x"], B, T, dil), d["x"]], 1)
        yield ("fwd pre %d %d %d %d" % (R, B, T, dil), a, np.concatenate([d["wf"][0], d["wf"][1]], 0), d["bf"], 1.0, 0.25,
               False, False, False)
        yield ("fwd residual %d %d %d %d" % (R, B, T, dil), fwd_c_bf16(f), d["wr"], d["br"], 2.0 ** -11, GW, False, False, False)
    for cout in (128, 256):
        d = tap(cout)
        for step in (1, -1):
            a, w = tap_ops(d, step)
            yield ("tap %d step %d" % (cout, step), a, w, d["b"], GA, GW, True, False, False)
        B, T, Cin, pool = TAP
        fa = pool_rows(d["fadd"].reshape(B, T // pool, -1)[:, :, :cout], B, T, pool)
        yield ("tap %d 1x1" % cout, d["x"], d["w"][0], d["b"] + 0.5 * fa, GA, GW, True, False, True)       # (a bias per row)
    d = nc()
    for l in range(NC[0]):
        for n, (a, w) in enumerate(nc_ops(d, l)):
            yield ("nc layer %d product %d" % (l, n), a, w, None, GA, GW, False, False, n != 1)
    for (R, B, T, dil) in BWD_UP:
        d = bwd_up(R, B, T, dil)
        a, w = bwd_up_ops(d, B, T, dil)
        yield ("bwd up %d %d %d %d" % (R, B, T, dil), a, w, None, GA, GW, True, False, False)
