"""Designs and references for ONE STEP of the queue-cached generators (csrc/srwn_gen.hip: throughput body,
csrc/srwn_gen16.hip: latency body; ring layout csrc/srwn_gen_ring.h).  Host code only (NumPy): tests/test_gen_design.py
proves the designs' conditions on the CPU, tests/test_gpu_gen_entries.py holds the kernels to them.  The helpers of
tests/gemm_design.py (G) and tests/group_design.py (D) are reused, not copied.

The step, as both bodies compute it (T = engine dtype, rnd_T = one nearest-even rounding, fl32 = one IEEE fp32 operation):

    x_0[t]   = rnd_T( fmaf(iw[0][n], a[t-2], fmaf(iw[1][n], a[t-1], ib[n])) )      a[] = forced samples or the carry
    cond:      x_l = rnd_T( base + cb_l[u, frame] ), base = the rounded x_0 (l = 0) / the unrounded layer output (l > 0)
    ring:      x_l[t] -> slot t mod (d_l+1) (slot forms: the pool's clock for t); the delayed tap is read from slot
               (t+1) mod (d_l+1) -- zero while t - d_l < 0 in the throughput body's resume forms; the latency body and every
               slot form read what the ring holds (their callers hand the rings over zero-filled or prompt-filled)
    f        = bf + Wf[0] x_l[t-d] + Wf[1] x_l[t]          fp32 accumulation on the matrix pipe
    z        = rnd_T( tanh_(f) ),  c = rnd_T( z * sigmoid_(z) )                      Math<T> of csrc/srwn_common.h
    x_{l+1}  = rnd_T( fl32( fl32( x_l[t] + (br + Wr c) ) * kSqrtHalf ) [+ cb_{l+1}] )   (the last one is not stored)
    head:      r0 = rnd_T(relu(sum_l bs_l + sum_l Ws_l c_l)), r1 = rnd_T(relu(b1 + W1 r0)), logits = b2 + W2 r1 (fp32)
    softmax, mode "argmax": the FIRST maximum of the logits (per lane `>` over its four classes in rising order, between
               lanes the greater value and on equal values the lower index); audio = its mu-law decode; mixture of
               logistics, the same mode 0 (mode="argmax" or "mean"): the mixture is a Gumbel-max draw (out of scope
               here), audio = clamp(mean of the selected mixture, -1, 1); the carry becomes (a[t], a[t-1]) of the
               samples the next step reads

DESIGN A ("planted", bf16 mode, bit for bit, no entry left out).  Every slot of every ring is written before the launch
with integers |v| <= 4.  Wf[0] is one entry of +-1/4 per output column on a permutation, bf in {-1, 0, 1}/4, Wf[1] is
non-zero in layer 0 only, where the current input is designed too (samples on the grid 1/2, init_w in {-2, 2}, init_b an
integer: x_0 an integer, |x_0| <= 6; conditioned: cb_0 an integer in [-1, 1]).  So every f is on the grid 1/4 in [-3, 3]:
25 values, for each of which tanh in float64 and in the kernel's exp2 / reciprocal form round to the same bf16 z with a
margin of at least 100 x the restatement's error (tests/test_gen_design.py).  c is then a function of that bf16 z through
IEEE fma / mul only (G.sigmoid_poly32).  Wr, Ws, W1, W2 are sparse on the grid 1/8 with every row and column covered, the
biases dyadic: every product sum is a sum of exact terms whose partial sums are fp32 numbers in any order (D.sums_exactly,
asserted per entry by `step_a`).  What is left -- two fp32 roundings and rnd_T -- NumPy reproduces.  Conditioned: the last
`+ cb` may be contracted with the kSqrtHalf product into one fma (the two bodies are written differently there), so the
reference carries BOTH admissible values of every entry (`cands`), through the layers above as well.

The planted ring of the latency body and the comparison of the bodies with each other use `plant(..., pad=True)`: the
slots of steps before the clip's start hold the zero padding the callers of that body guarantee.  The throughput body
also runs on the ring without the padding (every slot non-zero): its reference is the same, since it must not read them.

DESIGN B ("free run", either mode, per entry on the kernel's own rings).  Dyadic weights of density 1/4 on both taps;
the run is N one-step launches from a zeroed ring and the ring is copied after each.  Layer l of step t is compared
with a float64 restatement of that one layer fed with the STORED x_l[t] and x_l[t-d], the logits with one of the skip
sum and head fed with all stored x_l[t] (`layer_b`, `head_b`): no error travels further than one layer.  Bound per entry,
as in tests/group_design.py:  |got - x| <= ulp_T(ref) + c (u_out |x| + e), the reach e built from K 2^-24 S of each
accumulation (dropped where D.sums_exactly), the float32 restatement's error of tanh and the gate (TANH_ERR, GATE_ERR:
measured on the CPU) and one ulp_T of every z / c / r0 / r1 whose float64 value lies within reach of a rounding midpoint,
pushed through |Wr| (|Ws|, |W1|, |W2|; relu is 1-Lipschitz).  Entries with midpoint distance > REACH x e must match bit
for bit.  c = 4 x C_CPU, REACH = 4 x C_CPU_PRE: worst ratios of the float32 NumPy restatement on these designs
(tests/test_gen_design.py measures them; never a GPU figure).
"""
import numpy as np

from tests import gemm_design as G
from tests import group_design as D

F32 = np.float32
K32 = D.SQRT_HALF32
GRID_F = np.arange(-12, 13) / 4.0             # the 25 values f takes on design A

# ---- shapes ---------------------------------------------------------------------------------------------------------------
DILS = {"d1": [1], "d12": [1, 2], "d312": [3, 1, 2], "d7": [1, 2, 4, 8, 1, 2, 5], "d4": [4, 8, 4, 16]}
# (dilations key, R, S, B, head, C or M, conditioned): every width, head size, depth residue and stream count once at least
CASES_A = [
    ("d1", 64, 256, 1, "softmax", 256, False),
    ("d12", 32, 128, 33, "softmax", 100, False),
    ("d312", 64, 128, 32, "softmax", 30, False),
    ("d7", 64, 256, 33, "softmax", 100, False),
    ("d4", 64, 256, 33, "softmax", 256, False),
    ("d312", 32, 128, 33, "mol", 5, False),
    ("d12", 64, 256, 33, "mol", 10, True),
    ("d7", 64, 128, 32, "mol", 5, True),
    ("d4", 32, 128, 1, "mol", 10, True),
]
CASES_B = [
    ("d312", 64, 256, 33, "softmax", 256, False),
    ("d7", 32, 128, 33, "softmax", 100, False),
    ("d12", 64, 128, 32, "mol", 10, True),
    ("d1", 64, 256, 1, "softmax", 30, False),
]
POOL, ENC = 4, 6                              # conditioned decoder: pool stride and encoding channels


def steps_a(dil):
    """Absolute steps of design A: taps before the clip's start, the ring wrap, a large absolute step."""
    dm = max(dil)
    return sorted({0, 1, 2, dm, dm + 1, 1000})


def length_b(dil):
    return 2 * (max(dil) + 1) + 3


def frames_of(nsteps_total):
    """Frames of a conditioned run: enough for every step, and no divisor of the steps."""
    return nsteps_total // POOL + 1


# ---- the ring -------------------------------------------------------------------------------------------------------------
def ring_shape(dil, R, B):
    """(groups, elements of one group, [element offset of layer l])."""
    off, offs = 0, []
    for d in dil:
        offs.append(off)
        off += (d + 1) * 32 * R
    return (B + 31) // 32, off, offs


def ring_unpack(flat, dil, R, B):
    """The flat ring [groups * elems] -> per layer [depth, groups * 32, R] (row = 32 * group + column), float64."""
    g, elems, offs = ring_shape(dil, R, B)
    flat = np.asarray(flat, np.float64).reshape(g, elems)
    out = []
    for d, o in zip(dil, offs):
        v = flat[:, o:o + (d + 1) * 32 * R].reshape(g, d + 1, 32, R)
        out.append(v.transpose(1, 0, 2, 3).reshape(d + 1, g * 32, R).copy())
    return out


def ring_pack(layers, dil, R, B):
    g, elems, offs = ring_shape(dil, R, B)
    flat = np.zeros((g, elems))
    for v, d, o in zip(layers, dil, offs):
        flat[:, o:o + (d + 1) * 32 * R] = v.reshape(d + 1, g, 32, R).transpose(1, 0, 2, 3).reshape(g, -1)
    return flat.reshape(-1)


def plant(d, t, pad, key=0):
    """Integers in [-4, 4] (nine in ten non-zero) in every slot of every layer ring, seeded per (design, step, layer); pad:
    the slots of steps before 0 -- slot s holds the step t' = s (mod depth) of [t - d_l, t - 1] -- are zero."""
    out = []
    n = 32 * ((d["B"] + 31) // 32)
    for l, dl in enumerate(d["dil"]):
        v = G.exact((dl + 1, n, d["R"]), 4, 0.9, G._seed(d["seed"], t, l, key, 83), 1.0)
        if pad:
            for s in range(dl + 1):
                tp = t - 1 - ((t - 1 - s) % (dl + 1))          # the latest step <= t - 1 that sits in slot s
                if tp < 0 and s != t % (dl + 1):
                    v[s] = 0.0
        out.append(v)
    return out


# ---- design A -------------------------------------------------------------------------------------------------------------
def _sparse(shape, per_col, seed, values=3):
    """[in, out] on the grid 1/8: about per_col entries per output column, every row and column covered."""
    w = G.exact(shape, values, min(1.0, per_col / shape[0]), seed, G.GW)
    return G.cover(G.cover(w, 0, seed + 1, G.GW), 1, seed + 2, G.GW)


def design_a(dkey, R, S, B, head, CM, cond):
    dil = DILS[dkey]
    L = len(dil)
    C = CM if head == "softmax" else 4 * CM
    s = G._seed(sum((i + 1) * v for i, v in enumerate(dil)), R, S, B, C, int(cond), 79)
    rng = np.random.default_rng(s)
    wf = np.zeros((L, 2, R, R))
    for l in range(L):
        wf[l, 0, rng.permutation(R), np.arange(R)] = rng.choice([-0.25, 0.25], R)
    wf[0, 1, rng.permutation(R), np.arange(R)] = rng.choice([-0.25, 0.25], R)
    d = dict(dil=list(dil), L=L, R=R, S=S, B=B, C=C, head=head, M=CM if head == "mol" else 0, cond=cond, seed=s,
             init_w=rng.choice([-2.0, 2.0], (2, R)), init_b=rng.integers(-2, 3, R).astype(np.float64),
             wf=wf, bf=rng.integers(-1, 2, (L, R)) * 0.25,
             wr=np.stack([_sparse((R, R), 4, s + 10 * l + 1) for l in range(L)]), br=G.exact((L, R), 15, 1.0, s + 2, 1 / 32),
             ws=np.stack([_sparse((R, S), 3, s + 10 * l + 3, 2) for l in range(L)]),
             bs=np.abs(G.exact((L, S), 3, 1.0, s + 4, 1 / 8)),               # positive: most relus pass, so that a wrong
             w1=_sparse((S, S), 4, s + 5, 2), b1=0.25 + np.abs(G.exact((S,), 3, 1.0, s + 6, 1 / 8)),   # c shows in the logits
             w2=_sparse((S, C), 6, s + 7, 2), b2=G.exact((C,), 3, 1.0, s + 8, 1 / 8))
    if head == "softmax":      # every seventh class has a twin three places on: exact ties, also among the maxima
        for k in range(0, C - 3, 7):
            d["w2"][:, k + 3], d["b2"][k + 3] = d["w2"][:, k], d["b2"][k]
        for i in np.nonzero(~d["w2"].any(1))[0]:      # (a k index the twins left without a term: one in a class without twin)
            d["w2"][i, 7 * int(rng.integers(0, (C - 2) // 7 + 1)) + 1] = G.GW
    if cond:
        wc = np.zeros((L, ENC, R))
        for l in range(L):
            wc[l, rng.integers(0, ENC, R), np.arange(R)] = rng.choice([-1.0, 1.0], R) * (1.0 if l == 0 else 0.25)
        d["wc"] = wc
        d["bc"] = np.concatenate([np.zeros((1, R)), rng.integers(-1, 2, (L - 1, R)) * 0.25])
    return d


def encoding(d, frames, key=0):
    """enc [B, frames, ENC] in {-1, 0, 1}: cb_l = enc Wc_l + bc_l has one product per entry -- exact, cb_0 an integer."""
    return G.exact((d["B"], frames, ENC), 1, 0.8, G._seed(d["seed"], frames, key, 89), 1.0)


def cond_table(d, enc):
    """cb [L, B, frames, R] in float64 (exact for design A; design B: rounded to T by the caller)."""
    return np.stack([enc @ d["wc"][l] + d["bc"][l] for l in range(d["L"])])


def samples_a(d, t, n, key=0):
    """(carry [B, 2] = (a[t-1], a[t-2]), forced [B, n]) on the grid 1/2 in [-1, 1]."""
    rng = np.random.default_rng(G._seed(d["seed"], t, n, key, 97))
    return rng.integers(-2, 3, (d["B"], 2)) * 0.5, rng.integers(-2, 3, (d["B"], n)) * 0.5


def _pad_rows(v, n):
    out = np.zeros((n,) + v.shape[1:])
    out[:v.shape[0]] = v
    return out


def lowest_bit(v):
    """-log2 of the lowest set bit of every entry (the finest unit the value is a multiple of); -inf for a zero."""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(v)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(v != 0, 53.0 - e - np.log2(np.where(mi != 0, low, 1.0)), -np.inf)


def _bits_of(v, w, bias_bits):
    """-log2 of a common unit of the terms v[t, k] w[k, j] (each v a multiple of its own lowest set bit, w on the grid 1/8)
    and the bias: per entry (t, j), over the k that carry a term."""
    lb = lowest_bit(v)
    out = np.full((v.shape[0], w.shape[1]), -np.inf)
    for j in range(w.shape[1]):
        nz = w[:, j] != 0
        if nz.any():
            out[:, j] = lb[:, nz].max(1)
    return np.maximum(out + 3.0, bias_bits)


def _exact_sum(v, w, b, bias_bits, what):
    """b + v @ w with the per-entry proof that every partial sum is an fp32 number in any order."""
    y, S = G.contract(v, w, b)
    ok = D.sums_exactly(S, _bits_of(v, w, bias_bits))
    assert ok.all(), "%s: %d entries whose sum is not exact in fp32" % (what, int((~ok).sum()))
    return y


def _eval32(v, w, b, reverse):
    k = range(v.shape[1])
    return G.eval32(v, w, b, k[::-1] if reverse else k).astype(np.float64)


def fma32(a, b, c):
    """fl32(a * b + c) of float32 values, one rounding: the product is exact in float64; the float64 sum's own rounding
    error (TwoSum) decides the one case a second rounding could get wrong, a sum on a float32 midpoint."""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    s = np.where(err > 0, np.nextafter(s, np.inf), np.where(err < 0, np.nextafter(s, -np.inf), s))
    return s.astype(F32).astype(np.float64)


def residual32(x, acc, cb_next):
    """The admissible values of rnd_bf16(fl32(fl32(x + acc) * kSqrtHalf) [+ cb]): one, or the separate add and the fma."""
    s = F32(x) + F32(acc)
    p = s * K32
    assert p.dtype == F32
    if cb_next is None:
        return [G.bf16_round(p.astype(np.float64))]
    sep = (p + F32(cb_next)).astype(np.float64)
    return [G.bf16_round(sep), G.bf16_round(fma32(s, K32, cb_next))]


def _dedupe(cands):
    out = []
    for c in cands:
        if not any(np.array_equal(c, o) for o in out):
            out.append(c)
    return out


def twin_pairs(C):
    """The softmax designs' twin classes (k, k + 3): identical columns of W2 and entries of b2."""
    return [(k, k + 3) for k in range(0, C - 3, 7)]


BOOST = 1.5                                   # b2 of the step's boosted twins: above every other logit of the designs


def b2_step(d, t):
    """The last bias of step t (softmax designs; the kernels read it from the parameters at every launch, so a test sets
    it per launch): up to three twin pairs, chosen per step, get b2 = BOOST -- at even steps pairs inside one lane's four
    classes (k / 4 == (k + 3) / 4), at odd steps pairs that straddle two lanes (for 256 classes one of them lanes 31 | 32,
    the halves the last shuffle merges).  The maximum of every row is then an EXACT TIE of two twins (asserted on the
    CPU), which pair wins differs from step to step, and the code must be the lower twin."""
    if d["head"] != "softmax":
        return d["b2"]
    pairs = [p for p in twin_pairs(d["C"]) if (p[0] // 4 == p[1] // 4) == (t % 2 == 0)]
    rng = np.random.default_rng(G._seed(d["seed"], t, 107))
    pick = [pairs[i] for i in rng.choice(len(pairs), min(3, len(pairs)), replace=False)]
    if (126, 129) in pairs:
        pick[-1] = (126, 129)
    b2 = d["b2"].copy()
    for p in pick:
        b2[list(p)] = BOOST
    return b2


def tie_kinds(logits):
    """(rows whose maximum is tied inside one lane's four classes, rows whose maximum is tied across lanes, the winners)."""
    lg = np.asarray(logits)
    first = np.argmax(lg, -1)
    same = cross = 0
    for r, k in enumerate(first):
        others = np.flatnonzero(lg[r] == lg[r, k])[1:]
        same += bool((others // 4 == k // 4).any())
        cross += bool((others // 4 != k // 4).any())
    return same, cross, first


def step_a(d, ring, t, a1, a2, cb=None, tap_from_ring=False, arith="ref", slot=None, b2=None):
    """One step of design A.  ring: per layer [depth, rows, R] (rows >= B, only the first B are used), t the absolute step
    (slot forms: `slot` = the pool's clock, t unused for the ring), a1 / a2 [B] = a[t-1] / a[t-2], cb [L, B, R] the
    conditioning rows of this step's frame.  arith "ref": float64 with the exactness assertions; "f32": the float32 NumPy
    restatement (products one k at a time, the kernel's tanh form).  Returns dict(x = [per layer: list of admissible
    written rows [B, R]], logits [B, C], wslot = [written slot per layer], diff = entries the two conditioned forms
    differ on)."""
    B, L, R = d["B"], d["L"], d["R"]
    clock = t if slot is None else slot
    b2 = b2_step(d, clock) if b2 is None else b2
    x0 = d["init_w"][0] * a2[:, None] + d["init_w"][1] * a1[:, None] + d["init_b"]
    assert np.array_equal(x0, np.rint(x0)) and np.abs(x0).max() <= 6
    if cb is not None:
        x0 = x0 + cb[0]
        assert np.array_equal(x0, np.rint(x0)) and np.abs(x0).max() <= 7
    cands, xs, cs, wslots, diff = [x0], [], [], [], 0
    for l, dl in enumerate(d["dil"]):
        depth = dl + 1
        wslots.append(clock % depth)
        xs.append(cands)
        tap = ring[l][(clock + 1) % depth][:B]
        if not tap_from_ring and t - dl < 0:
            tap = np.zeros_like(tap)
        assert l == 0 or not d["wf"][l, 1].any()
        xin = np.concatenate([tap, cands[0]], 1)
        wcat = np.concatenate([d["wf"][l, 0], d["wf"][l, 1]], 0)
        if arith == "ref":
            f = xin @ wcat + d["bf"][l]
            assert np.array_equal(f * 4, np.rint(f * 4)) and np.abs(f).max() <= 3.0
            z = D.round_to(np.tanh(f), "bf16")
        else:
            f = _eval32(xin, wcat, d["bf"][l], l & 1)
            z = G.bf16_round(G.tanh_bf16_mode32(f).astype(np.float64))
        c = G.gate_poly32(z)
        cs.append(c)
        if arith == "ref":
            acc = _exact_sum(c, d["wr"][l], d["br"][l], 5.0, "residual 1x1 of layer %d" % l)
        else:
            acc = _eval32(c, d["wr"][l], d["br"][l], not (l & 1))
        cbn = cb[l + 1] if (cb is not None and l + 1 < L) else None
        nxt = []
        for x in cands:
            r = residual32(x, acc, cbn)
            if len(r) == 2:
                diff += int((r[0] != r[1]).sum())
            nxt += r
        cands = _dedupe(nxt)
    call = np.concatenate(cs, 1)
    wsall = np.concatenate(list(d["ws"]), 0)
    bs = d["bs"].sum(0)
    if arith == "ref":
        skip = _exact_sum(call, wsall, bs, 3.0, "skip sum")
        r0 = G.bf16_round(np.maximum(skip, 0.0))
        r1 = G.bf16_round(np.maximum(_exact_sum(r0, d["w1"], d["b1"], 3.0, "head 1"), 0.0))
        logits = _exact_sum(r1, d["w2"], b2, 3.0, "head 2")
        assert np.array_equal(logits.astype(F32).astype(np.float64), logits)
    else:
        r0 = G.bf16_round(np.maximum(_eval32(call, wsall, bs, True), 0.0))
        r1 = G.bf16_round(np.maximum(_eval32(r0, d["w1"], d["b1"], False), 0.0))
        logits = _eval32(r1, d["w2"], b2, True)
    return dict(x=xs, logits=logits, wslot=wslots, diff=diff, c=cs, r0=r0, r1=r1)


def run_a(d, ring, t, carry, forced, n, cb_of=None, tap_from_ring=False, arith="ref"):
    """n planted steps from absolute step t in ONE launch (n <= min dilation: every tap read is a planted one), teacher
    forced: the reference ring after the launch (first admissible value), the per-step results and the carry out."""
    assert n == 1 or (n <= min(d["dil"]) and cb_of is None)
    ring = [v.copy() for v in ring]
    prev = [carry[:, 0].copy(), carry[:, 1].copy()]
    steps = []
    b2 = b2_step(d, t)                         # (one launch, one bias: that of its first step)
    for j in range(n):
        a1 = forced[:, j - 1] if j >= 1 else prev[0]
        a2 = forced[:, j - 2] if j >= 2 else (prev[0] if j == 1 else prev[1])
        r = step_a(d, ring, t + j, a1, a2, None if cb_of is None else cb_of(t + j), tap_from_ring, arith, b2=b2)
        for l in range(d["L"]):
            ring[l][r["wslot"][l], :d["B"]] = r["x"][l][0]
        steps.append(r)
    return ring, steps


def first_max(logits):
    """The generators' argmax: the first maximum."""
    return np.argmax(logits, -1)


def matches_any(got, cands):
    ok = np.zeros(np.shape(got), bool)
    for c in cands:
        ok |= G.same_bits(got, c)
    return ok


# ---- design A, the tanh grid ----------------------------------------------------------------------------------------------
def tanh_grid():
    """(z bf16 per grid value, worst restatement error, smallest midpoint distance of the float64 tanh) on GRID_F."""
    z64 = np.tanh(GRID_F)
    z32 = G.tanh_bf16_mode32(GRID_F).astype(np.float64)
    nz = GRID_F != 0
    md = G.midpoint_distance(z64[nz])
    return D.round_to(z64, "bf16"), G.bf16_round(z32), float(np.abs(z32 - z64).max()), float(md.min()), GRID_F[nz][md.argmin()]


# ---- design B -------------------------------------------------------------------------------------------------------------
def design_b(dkey, R, S, B, head, CM, cond):
    dil = DILS[dkey]
    L = len(dil)
    C = CM if head == "softmax" else 4 * CM
    s = G._seed(sum((i + 1) * v for i, v in enumerate(dil)), R, S, B, C, int(cond), 101)
    rng = np.random.default_rng(s)
    dens = lambda shape, seed, vals: G.cover(G.cover(G.exact(shape, vals, 0.25, seed, G.GW), 0, seed + 1, G.GW), 1, seed + 2, G.GW)
    d = dict(dil=list(dil), L=L, R=R, S=S, B=B, C=C, head=head, M=CM if head == "mol" else 0, cond=cond, seed=s,
             init_w=G.exact((2, R), 3, 1.0, s + 1, 0.5), init_b=G.exact((R,), 7, 1.0, s + 2, 1 / 8),
             wf=np.stack([np.stack([dens((R, R), s + 20 * l + 3 + 4 * k, 2) for k in range(2)]) for l in range(L)]),
             bf=G.exact((L, R), 7, 1.0, s + 4, 1 / 16),
             wr=np.stack([dens((R, R), s + 20 * l + 11, 2) for l in range(L)]), br=G.exact((L, R), 15, 1.0, s + 5, 1 / 32),
             ws=np.stack([dens((R, S), s + 20 * l + 15, 2) for l in range(L)]), bs=G.exact((L, S), 3, 1.0, s + 6, 1 / 8),
             w1=dens((S, S), s + 7, 1), b1=G.exact((S,), 3, 1.0, s + 8, 1 / 8),
             w2=dens((S, C), s + 9, 1), b2=G.exact((C,), 3, 1.0, s + 10, 1 / 8))
    if cond:
        d["wc"] = np.stack([G.exact((ENC, R), 2, 0.5, s + 30 + l, 0.25) for l in range(L)])
        d["bc"] = G.exact((L, R), 3, 1.0, s + 12, 0.25)
    return d


def audio_b(d, n):
    """Teacher-forced audio of a free run on the grid 1/16 in [-1, 1]."""
    return G.exact((d["B"], n), 16, 0.95, G._seed(d["seed"], n, 103), 1 / 16)


def _grid_err(fn32, fn64, lo, hi, n=48001):
    x = np.linspace(lo, hi, n).astype(F32)
    return float(np.abs(fn32(x).astype(np.float64) - fn64(x.astype(np.float64))).max())


# the float32 restatement's own error on a dense grid (measured on the CPU, tests/test_gen_design.py asserts them as upper
# figures): tanh on [-9, 9] in the exp2 / reciprocal form (bf16 mode) and np.tanh in float32 (fp32 mode); the gate on [-1, 1]
TANH_ERR = {"bf16": 2.5e-7, "fp32": 1.2e-7}
GATE_ERR = {"bf16": G.POLY_ERR + 6e-8, "fp32": 1.2e-7}
GATE_SLOPE = 1.1                              # max |d(z sigmoid z)/dz| on [-1, 1] = 1.0998 at z = 1


def measured_errs():
    return ({"bf16": _grid_err(G.tanh_bf16_mode32, np.tanh, -9, 9), "fp32": _grid_err(lambda x: np.tanh(x), np.tanh, -9, 9)},
            {"bf16": _grid_err(lambda z: z * G.sigmoid_poly32(z), G.gate64, -1, 1), "fp32": _grid_err(G.gate32, G.gate64, -1, 1)})


def _acc(v, w, b, mode, w_grid_bits, extra=None):
    """(y, S, e_acc): b + v @ w in float64, the sum of magnitudes, and K 2^-24 S where the sum is not provably exact
    (+ `extra` >= 0 per entry of v pushed through |w|)."""
    y, S = G.contract(v, w, b)
    K = (v != 0).astype(np.float64) @ (w != 0).astype(np.float64) + (np.asarray(b) != 0)
    bits = np.maximum(D.finest_bit(v, w.T, mode), w_grid_bits)
    e = K * G.EPS * S * ~D.sums_exactly(S, bits)
    if extra is not None:
        e = e + extra @ np.abs(w)
    return y, S, e


def _rounded(x, e, mode, reach, lipschitz_in=1.0):
    """A value the kernel rounds to T, known in float64 up to e: (reference, its uncertainty) -- zero where no admissible
    evaluation can round differently, else e + one ulp_T.  fp32 mode: T's rounding is the evaluation's own: e."""
    if mode == "fp32":
        return x, e + G.EPS * np.abs(x)
    ref = D.round_to(x, mode)
    safe = (e == 0) | ((x != 0) & (D.midpoint_distance(x, mode) > reach * e))
    return ref, np.where(safe, 0.0, e + D.ulp_of(ref, mode))


def gate_b(f, e_f, mode, reach):
    """(c reference, its uncertainty) from a pre-activation known up to e_f."""
    zref, dz = _rounded(np.tanh(f), e_f + TANH_ERR[mode], mode, reach)
    if mode == "bf16":
        # the gate is a function of the bf16 z through IEEE operations only: where z is decided, so is c, bit for bit
        c = G.gate_poly32(zref)
        return c, np.where(dz == 0, 0.0, GATE_SLOPE * dz + GATE_ERR[mode] + D.ulp_of(c, mode))
    return G.gate64(zref), GATE_SLOPE * dz + GATE_ERR[mode]


def layer_b(d, l, x_t, x_tap, cb_next, mode, reach):
    """One layer from the STORED x_l[t] and x_l[t-d] [B, R] (x_tap zeros before the clip's start): dict(x = float64 value
    of x_{l+1} before rnd_T, ref, e, c, dc)."""
    xin = np.concatenate([x_tap, x_t], 1)
    wcat = np.concatenate([d["wf"][l, 0], d["wf"][l, 1]], 0)
    f, _, e_f = _acc(xin, wcat, d["bf"][l], mode, 4.0)
    c, dc = gate_b(f, e_f, mode, reach)
    acc, S, e_a = _acc(c, d["wr"][l], d["br"][l], mode, 5.0, dc)
    y = (x_t + acc) * float(K32)
    e = e_a * float(K32) + 2 * G.EPS * np.abs(y)
    if cb_next is not None:
        y = y + cb_next
        e = e + G.EPS * np.abs(y)
    return dict(x=y, ref=D.round_to(y, mode), e=e, c=c, dc=dc)


def head_b(d, cs, dcs, mode, reach):
    call, dcall = np.concatenate(cs, 1), np.concatenate(dcs, 1)
    wsall = np.concatenate(list(d["ws"]), 0)
    skip, _, e0 = _acc(call, wsall, d["bs"].sum(0), mode, 3.0, dcall)
    r0, d0 = _rounded(np.maximum(skip, 0.0), e0, mode, reach)
    h1, _, e1 = _acc(r0, d["w1"], d["b1"], mode, 3.0, d0)
    r1, d1 = _rounded(np.maximum(h1, 0.0), e1, mode, reach)
    lg, _, e2 = _acc(r1, d["w2"], d["b2"], mode, 3.0, d1)
    return dict(x=lg, ref=lg.astype(F32).astype(np.float64), e=e2 + G.EPS * np.abs(lg))


def x0_b(d, a1, a2, cb0, mode):
    """x_0 of design B: dyadic and exact in fp32 (init_w on 1/2, audio on 1/16, init_b on 1/8: units of 1/32, < 2^24)."""
    x0 = d["init_w"][0] * a2[:, None] + d["init_w"][1] * a1[:, None] + d["init_b"]
    x0 = D.round_to(x0, mode)
    if cb0 is not None:
        x0 = D.round_to(x0 + cb0, mode)      # (dyadic + dyadic: exact in float64, so one rounding)
    return x0


def decided_b(r, mode, reach):
    return (r["e"] == 0) | ((r["x"] != 0) & (D.midpoint_distance(r["x"], mode) > reach * r["e"]))


def bound_b(r, mode, c):
    return D.ulp_of(r["ref"], mode) + c * (G.U_OUT[mode] * np.abs(r["x"]) + r["e"])


def ratio_b(got, r, mode):
    err = np.abs(np.asarray(got, np.float64) - r["x"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / (G.U_OUT[mode] * np.abs(r["x"]) + r["e"]))


# ---- design B, the float32 restatement (the kernel's stand-in on the CPU) --------------------------------------------------
def _rnd(v, mode):
    return G.bf16_round(np.asarray(v, np.float64)) if mode == "bf16" else np.asarray(v, np.float64)


def restate_b(d, ring, t, a1, a2, cb, mode):
    """One free-run step in float32 NumPy on the restatement's own ring: dict(x = [x_l[t] stored], pre = [value of
    x_{l+1} before rnd_T], logits)."""
    B, L = d["B"], d["L"]
    x = x0_b(d, a1, a2, None if cb is None else cb[0], mode)
    xs, pres, cs = [], [], []
    for l, dl in enumerate(d["dil"]):
        xs.append(x)
        tap = ring[l][(t + 1) % (dl + 1)][:B] if t - dl >= 0 else np.zeros_like(x)
        f = G.eval32(np.concatenate([tap, x], 1), np.concatenate([d["wf"][l, 0], d["wf"][l, 1]], 0), d["bf"][l],
                     range(2 * d["R"]))
        if mode == "bf16":
            z = _rnd(G.tanh_bf16_mode32(f), mode)
            c = G.gate_poly32(z)
        else:
            z = np.tanh(f)
            c = G.gate32(z).astype(np.float64)
        cs.append(c)
        acc = G.eval32(c, d["wr"][l], d["br"][l], range(d["R"]))
        p = (F32(x) + acc) * K32
        if cb is not None and l + 1 < L:
            p = p + F32(cb[l + 1])
        assert p.dtype == F32
        pres.append(p.astype(np.float64))
        x = _rnd(p, mode)
    call = np.concatenate(cs, 1)
    r0 = _rnd(np.maximum(G.eval32(call, np.concatenate(list(d["ws"]), 0), d["bs"].sum(0), range(call.shape[1])), 0), mode)
    r1 = _rnd(np.maximum(G.eval32(r0, d["w1"], d["b1"], range(d["S"])), 0), mode)
    return dict(x=xs, pre=pres, logits=G.eval32(r1, d["w2"], d["b2"], range(d["S"])).astype(np.float64))


def check_b(d, ring_before, ring_after, t, logits, cb, mode, reach, c):
    """(c: {"x": .., "logits": ..}, the bound's constant per quantity)"""
    return _check_b(d, ring_before, ring_after, t, logits, cb, mode, reach, c["x"], c["logits"])


def _check_b(d, ring_before, ring_after, t, logits, cb, mode, reach, c, c_lg):
    """Holds one free-run step to the layer-local references.  ring_before / ring_after: per layer [depth, rows, R] around
    the step; logits [B, C]; cb [L, B, R] or None.  Returns dict(worst = {name: worst ratio}, decided = (n, of), bad =
    [messages])."""
    B, L = d["B"], d["L"]
    worst, bad, ndec, nall = {"x": 0.0, "logits": 0.0}, [], 0, 0
    cs, dcs = [], []
    for l, dl in enumerate(d["dil"]):
        x_t = ring_after[l][t % (dl + 1)][:B]
        x_tap = ring_before[l][(t + 1) % (dl + 1)][:B] if t - dl >= 0 else np.zeros_like(x_t)
        r = layer_b(d, l, x_t, x_tap, cb[l + 1] if (cb is not None and l + 1 < L) else None, mode, reach)
        cs.append(r["c"]); dcs.append(r["dc"])
        if l + 1 == L:
            break
        got = ring_after[l + 1][t % (d["dil"][l + 1] + 1)][:B]
        dec = decided_b(r, mode, reach)
        ndec += int(dec.sum()); nall += dec.size
        worst["x"] = max(worst["x"], float(ratio_b(got, r, mode).max()))
        miss = dec & ~G.same_bits(got, r["ref"])
        if miss.any():
            bad.append("step %d layer %d: %d decided entries differ in bits" % (t, l + 1, int(miss.sum())))
        over = np.abs(got - r["x"]) > bound_b(r, mode, c)
        if over.any():
            bad.append("step %d layer %d: %d entries beyond the bound" % (t, l + 1, int(over.sum())))
    h = head_b(d, cs, dcs, mode, reach)
    worst["logits"] = float(ratio_b(logits, h, "fp32").max())
    dec = decided_b(h, "fp32", reach)
    miss = dec & ~G.same_bits(logits, h["ref"])
    over = np.abs(logits - h["x"]) > bound_b(h, "fp32", c_lg)
    if miss.any():
        bad.append("step %d logits: %d decided entries differ in bits" % (t, int(miss.sum())))
    if over.any():
        bad.append("step %d logits: %d entries beyond the bound" % (t, int(over.sum())))
    return dict(worst=worst, decided=(ndec, nall), bad=bad)


# Worst ratios of the float32 NumPy restatement on CASES_B (tests/test_gen_design.py measures them; SRWN_PRINT_ERR=1
# pytest -s prints the figures), rounded up by G.rounded_up, per mode and quantity -- from the CPU, never from a GPU:
#   pre:     |value before rnd_T - float64| / e                              (sets REACH)
#   x:       |stored ring entry - float64| / (u_out |x| + e)     (a correctly rounded bf16 output reaches 2 against u_out)
#   logits:  |logit - float64| / (2^-24 |x| + e)
#   measured   pre  bf16 0.946  fp32 0.121      x  bf16 1.992  fp32 0.113      logits  bf16 0.479  fp32 0.001
C_CPU_PRE = {"bf16": 1.0, "fp32": 0.125}
C_CPU = {"bf16": {"x": 2.0, "logits": 0.5}, "fp32": {"x": 0.125, "logits": 0.0625}}
REACH = {m: 4.0 * v for m, v in C_CPU_PRE.items()}
C_GPU = {m: {k: 4.0 * v for k, v in q.items()} for m, q in C_CPU.items()}
