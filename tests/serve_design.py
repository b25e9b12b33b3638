"""Exact input designs, float64 references, float32 restatements and bound constants for the kernels that stand around the
streamed stack: csrc/srwn_recog.hip (stream entry, pooled head, hop sum, window mean, roll), csrc/srwn_embed.hip (window
embed match, gallery match) and the softmax half of csrc/srwn_score.hip (pool entry with its codes, score head, nll rows),
each with its slot form.  Host code only (NumPy); tests/test_serve_design.py checks the designs on the CPU and
tests/test_gpu_serve_entries.py holds the kernels to them.  Built on tests/gemm_design.py (G): the same operands, range
conditions, roundings and bound.

The chained head design (pooled head, score head) composes G.skipsum with G.chain:
  z [L, rows, R] in {-1, 0, 1}          bf16 mode: G.gated makes the gate exactly 0, 187/256, -69/256
  Ws [L R, S] sparse in {-1, 0, 1}/8    bs_sum on the product grid 2^-11;  r0 = round_out(relu(.), "bf16")
  W1 [S, S]   sparse in {-1, 0, 1}/8    b1 on r0's product grid 2^-14;     r1 = round_out(relu(.), "bf16")
  W2 [S, Cp]  sparse, |int| <= 16, /8   b2 on the grid 2^-17, the columns from C on zero (the scorer only)
Each bias is minus the column's own value at its lower-third row: a third of every column's pre-activations are <= 0 and
one of them is EXACTLY 0 (a tie of the relu at 0, as G.chain places with b1).  Every stage passes G.check_exact on its own
grid (``head_stages``), the hop sums of r1 stay below 2^24 units (order-free), so in bf16 mode every quantity through the
ring row and through logits_out is exact.  In fp32 mode the gate is inexact and relu is 1-Lipschitz, so the per-entry
bound carries through the chain (``head_ref`` returns it):
  e0 = f_abs_gate32 |Ws|^T 1 + K0 2^-24 S0;  e1 = |W1|^T e0 + K1 2^-24 S1;  ring: the sum of e1 over the hop's rows;
  logits: |W2|^T e1 + K1 2^-24 S2.                Held per entry: |got - ref| <= c (2^-24 |ref| + that scale).

W2 carries built ties (``ties``): one column copied into its neighbour (the next lane of row_nll) and, where C has room,
another copied into the column 8 further on (the same lane), with biases lifted so that each pair is the row maximum in at
least a tenth of the rows.
Because the copies are exact copies, the device's logits tie too in fp32 mode: ``top_gap`` is the gap between the maximum
and the best column that is NOT a copy of it, and the lowest index must win in both modes.

Bound for what is not exact (the project's rule, tests/gemm_design.py): c = 4 x C_CPU[key][mode], C_CPU the worst ratio of
the float32 NumPy restatement on the same designs, measured by tests/test_serve_design.py, never a figure from a GPU.
"""
import functools

import numpy as np

from tests import gemm_design as G

GW = G.GW
MODES = ("bf16", "fp32")
EPS = G.EPS
WIDTHS = [(32, 128), (32, 256), (64, 128), (64, 256)]
HOPS = [1, 31, 32, 33, 40, 96]
DENS = (0.25, 0.1, 0.1)                     # Ws, W1, W2
W2_INT = 16                                 # the headroom of the third product, spent on the spread of the logits


# ---- the chained head ----------------------------------------------------------------------------------------------------
def _third_bias(pre, grid):
    """-(the column's value at its lower-third row): a third of the column <= 0, one entry exactly 0."""
    rows = pre.shape[0]
    k = rows // 3
    b = -np.partition(pre, k, axis=0)[k]
    assert np.array_equal(b / grid, np.rint(b / grid))
    return b


@functools.lru_cache(None)
def head(L, R, S, rows, C=0):
    """The chained design for `rows` rows (C = 0: the classifier's two products only)."""
    s = G._seed(L, R, S, rows, C, 73)
    z = G.exact((L, rows, R), 1, 0.8 if rows > 1 else 1.0, s, 1.0)
    z = G.cover(z, 1, s + 1)
    a = G.gated(G.skipsum_a(z))
    ws = G.cover(G.cover(G.exact((L * R, S), 1, DENS[0], s + 2, GW), 0, s + 3, GW), 1, s + 4, GW)
    bs = _third_bias(a @ ws, GW / 256)
    r0 = G.round_out(np.maximum(a @ ws + bs, 0.0), "bf16")
    w1 = G.cover(G.cover(G.exact((S, S), 1, DENS[1], s + 5, GW), 0, s + 6, GW), 1, s + 7, GW)
    b1 = _third_bias(r0 @ w1, GW * GW / 256)
    d = dict(z=z, ws=ws, bs=bs, w1=w1, b1=b1, C=C)
    if C:
        Cp = (C + 31) // 32 * 32
        r1 = G.round_out(np.maximum(r0 @ w1 + b1, 0.0), "bf16")
        w2 = np.zeros((S, Cp))
        w2[:, :C] = G.cover(G.cover(G.exact((S, C), W2_INT, DENS[2], s + 8, GW), 0, s + 9, GW), 1, s + 10, GW)
        g2 = GW ** 3 / 256
        b2 = np.zeros(Cp)
        b2[:C] = G.exact((C,), 255, 1.0, s + 11, g2 * 256)
        pairs = ties(C)
        for (c0, c1) in pairs:
            w2[:, c1] = w2[:, c0]
        tied = {c: p for p in pairs for c in p}
        for kk in np.nonzero(~w2[:, :C].any(1))[0]:      # (a copy may have taken a k's only weight: give it one back)
            c = int((kk * 5 + 1) % C)
            w2[kk, list(tied.get(c, (c,)))] = GW
        for (c0, c1) in pairs:                 # lift the pair until it is the row maximum in a quarter of the rows (the next pair takes some back)
            lg = r1 @ w2[:, :C] + b2[:C]
            other = np.delete(lg, [c0, c1], axis=1).max(1) if C > 2 else np.full(rows, -1.0)
            need = np.sort(other - (lg[:, c0] - b2[c0]))[::-1]
            lift = np.ceil((need[min(rows - 1, rows // 4)] + 1.0 / 64) / g2) * g2
            b2[c0] = b2[c1] = lift
        rng = np.random.default_rng(s + 12)
        tg = (np.arange(rows) * 7 + rng.integers(0, C, rows)) % C
        d.update(w2=w2, b2=b2, tg=tg.astype(np.int32), pairs=pairs)
    return d


def ties(C):
    """The built ties of W2: (column, its copy) at distance 1 and at distance 8, where C has room for them."""
    out = []
    if C >= 2:
        out.append((C // 3 if C // 3 + 1 < C else 0, (C // 3 if C // 3 + 1 < C else 0) + 1))
    if C >= 12:
        c0 = 2 * C // 3
        c0 = c0 if c0 + 8 < C else C - 9
        if c0 not in (out[0][0], out[0][1]) and c0 + 8 not in (out[0][0], out[0][1]):
            out.append((c0, c0 + 8))
    elif C >= 9 and out[0][0] != 0 and out[0][1] != 8 and out[0][0] != 8:
        out.append((0, 8))
    return out


def codes(d):
    """The targets as the kernel is given them: one -1 (scores as 0) and one C (scores as C - 1)."""
    tg = d["tg"].copy()
    if len(tg) > 2:
        tg[1], tg[len(tg) - 1] = -1, d["C"]
    return tg


def head_gate(d, mode):
    """The gate operand [rows, L R]: exact on the grid 1/256 (bf16), the float64 gate of z (fp32)."""
    a = G.skipsum_a(d["z"])
    return G.gated(a) if mode == "bf16" else G.gate64(a)


def _rnd(v, mode):
    return G.round_out(v, "bf16") if mode == "bf16" else v


def head_ref(d, mode):
    """float64 (r1, e1, logits, e2): r1 [rows, S] with its per-entry error scale e1 (zeros in bf16 mode: exact), and for
    the scorer the logits [rows, C] with theirs."""
    a = head_gate(d, mode)
    K0, K1 = a.shape[1], d["w1"].shape[0]
    pre0, S0 = G.contract(a, d["ws"], d["bs"])
    r0 = _rnd(np.maximum(pre0, 0.0), mode)
    pre1, S1 = G.contract(r0, d["w1"], d["b1"])
    r1 = _rnd(np.maximum(pre1, 0.0), mode)
    if mode == "bf16":
        e0 = e1 = None
    else:
        e0 = G.f_abs_gate32() * np.abs(d["ws"]).sum(0)[None, :] + K0 * EPS * S0
        e1 = e0 @ np.abs(d["w1"]) + K1 * EPS * S1
    if not d["C"]:
        return r1, e1, None, None
    C = d["C"]
    lg, S2 = G.contract(r1, d["w2"][:, :C], d["b2"][:C])
    e2 = None if mode == "bf16" else e1 @ np.abs(d["w2"][:, :C]) + K1 * EPS * S2
    return r1, e1, lg, e2


def head_stages(d):
    """The three exact contractions of bf16 mode as (name, a, w, b, ga, gw) for G.check_exact / G.check_cover."""
    a = head_gate(d, "bf16")
    r0 = G.round_out(np.maximum(a @ d["ws"] + d["bs"], 0.0), "bf16")
    out = [("skip", a, d["ws"], d["bs"], 1.0 / 256, GW), ("w1", r0, d["w1"], d["b1"], GW / 256, GW)]
    if d["C"]:
        r1 = G.round_out(np.maximum(r0 @ d["w1"] + d["b1"], 0.0), "bf16")
        C = d["C"]
        out.append(("w2", r1, d["w2"][:, :C], d["b2"][:C], GW * GW / 256, GW))
    return out


def head_restate32(d, mode):
    """The chain in float32 NumPy, k in order, bias first: (r1, logits) as float64 arrays."""
    f = np.float32
    a = G.skipsum_a(d["z"])
    a = G.gated(a) if mode == "bf16" else G.gate32(a).astype(np.float64)
    r0 = _rnd32(np.maximum(G.eval32(a, d["ws"], d["bs"], range(a.shape[1])), f(0)), mode)
    r1 = _rnd32(np.maximum(G.eval32(r0, d["w1"], d["b1"], range(r0.shape[1])), f(0)), mode)
    if not d["C"]:
        return r1, None
    C = d["C"]
    return r1, G.eval32(r1, d["w2"][:, :C], d["b2"][:C], range(r1.shape[1])).astype(np.float64)


def _rnd32(v32, mode):
    v = v32.astype(np.float64)
    return G.bf16_round(v) if mode == "bf16" else v


def hop_rows(x, B, k, hop, mc):
    """x [B mc, S] -> [B, k, hop, S]: the chunk's rows of every hop."""
    S = x.shape[1]
    return x.reshape(B, mc, S)[:, :k * hop].reshape(B, k, hop, S)


def top_gap(lg, pairs):
    """(argmax with the lowest index, gap to the best column that is no copy of the maximum) per row."""
    m = lg.max(1)
    group = np.arange(lg.shape[1])
    for (c0, c1) in pairs:
        group[c1] = c0
    best = group[lg.argmax(1)]      # (a float64 product may leave a copy an ulp from its original: the pair is one column)
    masked = np.where(group[None, :] == group[best][:, None], -np.inf, lg)
    return best, m - masked.max(1)


# ---- butterfly sums (the hop sum's documented order) ----------------------------------------------------------------------
def butterfly32(v):
    """v [..., n] float32, n a power of two: the xor butterfly 1, 2, 4, ... as every lane ends with it."""
    v = np.asarray(v, np.float32).copy()
    n = v.shape[-1]
    idx = np.arange(n)
    s = 1
    while s < n:
        v = v + v[..., idx ^ s]
        s <<= 1
    assert v.dtype == np.float32
    return v[..., 0]


def hop_sum32(r1):
    """r1 [..., hop, S] float32 -> [..., S]: tiles of 32 rows in time order, masked rows add +0, each tile an xor butterfly."""
    r1 = np.asarray(r1, np.float32)
    hop = r1.shape[-2]
    h = np.zeros(r1.shape[:-2] + r1.shape[-1:], np.float32)
    for t0 in range(0, hop, 32):
        tile = np.zeros(r1.shape[:-2] + (32, r1.shape[-1]), np.float32)
        n = min(32, hop - t0)
        tile[..., :n, :] = r1[..., t0:t0 + n, :]
        h = h + butterfly32(np.moveaxis(tile, -2, -1))
    assert h.dtype == np.float32
    return h


@functools.lru_cache(None)
def hopsum(S, hop, k, B, kind, mode):
    """r1 [B, k hop + 2, S]: dyadic (1/4, |int| <= 15) or float32 Gaussian (rounded to bf16 in bf16 mode); the two rows
    behind the chunk hold 2^10 times the design's values."""
    s = G._seed(S, hop, k, B, 79 + (kind == "gauss"))
    mc = k * hop + 2
    if kind == "dyadic":
        x = G.exact((B, mc, S), 15, 1.0, s, 0.25)
    else:
        x = np.random.default_rng(s).normal(0, 1, (B, mc, S)).astype(np.float32).astype(np.float64)
        if mode == "bf16":
            x = G.bf16_round(x)
    x[:, k * hop:] *= 1024.0
    return x


# ---- stream entry --------------------------------------------------------------------------------------------------------
A_TOP = 1.0


@functools.lru_cache(None)
def entry(R, seed=0):
    """w [2, R] on 1/8 (|int| <= 15), bias on the product grid 2^-7."""
    s = G._seed(R, seed, 83)
    return dict(w=G.exact((2, R), 15, 1.0, s, 0.125), b=G.exact((R,), 15, 1.0, s + 1, 1.0 / 128))


def audio(shape, seed):
    """Dyadic samples in [-1, 1] on the grid 1/16, no zeros."""
    return G.exact(shape, 16, 1.0, G._seed(seed, 89), 1.0 / 16)


def entry_ref(e, x0, x1, mode):
    """b + x0 w0 + x1 w1 per row, exact: x0, x1 [rows] -> [rows, R] rounded once to the output dtype."""
    y = e["b"][None, :] + x0[:, None] * e["w"][0][None, :] + x1[:, None] * e["w"][1][None, :]
    assert np.array_equal(y * 128, np.rint(y * 128)) and np.abs(y * 128).max() < 2 ** 22
    return G.round_out(y, mode)


# ---- window mean ---------------------------------------------------------------------------------------------------------
WINDOWS = [(32, 1), (64, 2), (32, 3), (40, 8), (16, 8), (160, 2)]        # (hop, nW): windows 32, 128, 96, 320, 128, 320
WM_S = [1, 100, 128, 256]
WM_C = [1, 12, 40]


def pow2(n):
    return n & (n - 1) == 0


@functools.lru_cache(None)
def ringrows(B, ring_rows, S, seed=0):
    """Dyadic ring rows [B, ring_rows, S] on the grid 1/4, |int| <= 15, no zeros."""
    return G.exact((B, ring_rows, S), 15, 1.0, G._seed(B, ring_rows, S, seed, 97), 0.25)


def window_sum(ring, j, nW):
    """ring [ring_rows, S], hop index j -> the exact sum of the nW rows that end at j (zeros while j < nW - 1)."""
    rr = ring.shape[0]
    if j < nW - 1:
        return np.zeros(ring.shape[1])
    return sum(ring[(j - nW + 1 + w) % rr] for w in range(nW))


def mean32(total, window):
    """The exact sum divided once in float32: the float64 quotient of two float32 numbers rounded to float32."""
    t32 = np.asarray(total, np.float32)
    assert np.array_equal(t32.astype(np.float64), total)
    return (t32.astype(np.float64) / np.float64(np.float32(window))).astype(np.float32).astype(np.float64)


@functools.lru_cache(None)
def wm_head(S, C, ldw):
    """w2 [S, ldw] on 1/8 (|int| <= 15; the columns from C on hold 2^10 times as much), b2 [C] on the grid 2^-7 (a multiple of every
    power-of-two window's product grid)."""
    s = G._seed(S, C, ldw, 101)
    w2 = G.exact((S, ldw), 15, 1.0, s, GW)
    w2[:, C:] *= 1024.0
    return dict(w2=w2, b2=G.exact((C,), 255, 1.0, s + 1, 2.0 ** -7))


def fma_chain32(m, w2, b2):
    """acc = b2; acc = fmaf(m[s], w2[s], acc) for s in order, in float32 (each fma rounded once, through float64)."""
    f = np.float32
    acc = np.broadcast_to(b2.astype(f), (m.shape[0], len(b2))).copy()
    m32, w32 = m.astype(f), w2.astype(f)
    for s in range(m.shape[1]):
        acc = (m32[:, s:s + 1].astype(np.float64) * w32[s:s + 1].astype(np.float64) + acc.astype(np.float64)).astype(f)
    return acc.astype(np.float64)


# ---- roll ------------------------------------------------------------------------------------------------------------------
ROLL_HISTS = [1, 63, 64, 65, 255, 256, 257, 600]
ROLL_CASES = [((63, 64, 65), (40, 64, 100)), ((255, 256, 257), (100, 256, 300)), ((1, 600, 64), (1, 7, 601)), ((600,), (160,)),
              ((), (5,))]                    # (hist per buffer, the chunk lengths n)


def roll_values(nbuf, B, rows, R):
    """A distinct fp32 integer per (buffer, stream, row, column): [nbuf, B, rows, R]."""
    v = np.arange(nbuf * B * rows * R, dtype=np.int64).reshape(nbuf, B, rows, R) + 1
    assert v.max() < 2 ** 24
    return v


def roll_bits16(v):
    """Their bf16 counterparts: finite positive bf16 bit patterns, adjacent rows and columns distinct."""
    return ((v * 40503) % 0x7F00 + 0x80).astype(np.int16)


# ---- softmax rows --------------------------------------------------------------------------------------------------------
SCORE_C = [1, 7, 8, 9, 30, 32, 33, 100, 256]
SCORE_CLIPS = [(1, 1), (2, 31), (1, 32), (2, 33), (2, 45)]      # (B, n)
MOL_M = [1, 10, 16]                                             # mixtures: 4 M logits on the same chained design
MOL_CLIPS = [(2, 33), (1, 45)]


def nll64(lg, code):
    """float64: (nll, m, l_code, log sum) per row of lg [rows, C]; codes clamped into [0, C)."""
    code = np.clip(code, 0, lg.shape[1] - 1)
    m = lg.max(1)
    ls = np.log(np.exp(lg - m[:, None]).sum(1))
    lc = lg[np.arange(len(code)), code]
    return ls + m - lc, m, lc, ls


def nll_scale(ref, m, lc, ls, C):
    return EPS * (np.abs(ref) + np.abs(m) + np.abs(lc) + np.abs(ls)) + (-(-C // 8) + 5) * EPS


def nll32(lg, code):
    """row_nll's lane map in float32 NumPy: 8 lanes striding the columns in rising order, butterfly 1, 2, 4."""
    f = np.float32
    lg = np.asarray(lg, f)
    rows, C = lg.shape
    code = np.clip(code, 0, C - 1)
    m = lg.max(1)
    part = np.zeros((rows, 8), f)
    for c in range(C):
        part[:, c % 8] = part[:, c % 8] + np.exp(lg[:, c] - m)
    sm = butterfly32(part)
    out = np.log(sm) + m - lg[np.arange(rows), code]
    assert out.dtype == f
    return out.astype(np.float64)


# ---- gallery match ---------------------------------------------------------------------------------------------------------
MATCH_D = [1, 2, 63, 64, 65, 256]
MAX_GALLERY = 72
MATCH_N = [-3, 0, 1, 3, 4, 5, 70, MAX_GALLERY, MAX_GALLERY + 7]
SQRT_EPS = float(np.sqrt(np.float32(1e-8)))


@functools.lru_cache(None)
def match(D, rows=3):
    """emb [rows, D] and gallery [MAX_GALLERY, D] on the grid 1/4 (|int| <= 7).  Gallery row 2 equals embedding 0 and is
    repeated in row 3 (another wave), row 6 (the same wave) -- and, for embedding 1, rows 8..11 (all four waves) are one
    row at the smallest distance of the gallery; embedding 2 has its nearest at rows 69 and 71 (beyond N = 70: one left)."""
    s = G._seed(D, rows, 103)
    emb = G.exact((rows, D), 7, 1.0, s, 0.25)
    gal = G.exact((MAX_GALLERY, D), 7, 1.0, s + 1, 0.25)
    emb[:, 0] = np.array([-1.5, 0.25, 1.5])[np.arange(rows) % 3]      # the embeddings lie >= 1.25 apart, and every drawn
    gal[:, 0] = np.random.default_rng(s + 2).choice([-1.0, -0.75, -0.5, -0.25, 0.75, 1.0], MAX_GALLERY)      # row >= 0.5 from each
    gal[2] = gal[3] = gal[6] = emb[0]
    near1 = emb[1].copy(); near1[0] += 0.25
    gal[8:12] = near1
    near2 = emb[2].copy(); near2[-1] -= 0.25
    gal[69] = gal[71] = near2
    return dict(emb=emb, gal=gal)


def match_ref(emb, gal, N):
    """(dist [rows, N] float32-exact, nearest, dmin): sqrt_f32(f32(1e-8) + ss), ss the exact sum of squares."""
    f = np.float32
    N = int(np.clip(N, 0, gal.shape[0]))
    ss = ((emb[:, None, :] - gal[None, :N, :]) ** 2).sum(-1)
    assert np.array_equal(ss * 16, np.rint(ss * 16)) and (ss * 16).max(initial=0) < 2 ** 24
    dist = np.sqrt(f(1e-8) + ss.astype(f)).astype(np.float64)
    assert np.sqrt(f(1e-8) + ss.astype(f)).dtype == f
    if N == 0:
        return dist, np.full(len(emb), -1), np.full(len(emb), np.inf)
    return dist, dist.argmin(1), dist.min(1)


# ---- the bound's constants -----------------------------------------------------------------------------------------------
# Worst ratio of the float32 NumPy restatement on the designs above, as tests/test_serve_design.py measures it
# (SRWN_PRINT_ERR=1 pytest -s prints the figures), rounded up by G.rounded_up:
#   measured   pooled_ring_fp32 0.0049   score_logits_fp32 0.0022   score_nll 0.434 (bf16) | 0.447 (fp32)
#              window_logits 0.363 (at S = 1: one rounding against K = 1)
# (K 2^-24 S is the worst case of K roundings of one sign; a random design stays two orders below it.)
C_CPU = {"pooled_ring_fp32": {"fp32": 0.0625}, "score_logits_fp32": {"fp32": 0.0625}, "score_nll": {"bf16": 0.4375, "fp32": 0.5},
         "window_logits": {"fp32": 0.375}}
C_GPU = {k: {m: 4.0 * v for m, v in c.items()} for k, c in C_CPU.items()}


def ratio(got, ref, scale):
    """|got - ref| / (2^-24 |ref| + scale) per entry (0 for an exact entry)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / (EPS * np.abs(ref) + scale))
