"""A stratified input design for the mixture-of-logistics (MoL) kernels, the per-entry bounds they are held to and the
fp32 restatement of the oracle those bounds come from.  Host code only (NumPy); tests/test_mol_design.py checks the design
on the CPU and tests/test_gpu_mol_entries.py holds srwn_mol_loss, srwn_mol_loss_dx, srwn_mol_nll_rows and
srwn_mol_score_rows(_slots) to it.

Design.  ``design(M)`` -> a Design of (x [N], l [N, 4M]) from a fixed seed, every value a float32.  A row belongs to one of
six strata and ALL its M components are drawn from that stratum, so the branch of ops.py:169 the posterior's dominant
component takes is known (delta = (x - mean) / scale):

  edge-   x in {-1, -0.9995}       delta ~ N(0, 1)
  edge+   x in {1, 0.9995}         delta ~ N(0, 1)
  centre  x in [-0.99, 0.99]       delta ~ N(0, 1)
  lower   x in [-0.99, 0.99]       delta in -[3, 9]     both sigmoid arguments negative: well conditioned
  upper   x in [-0.99, 0.99]       delta in +[3, 9]     both sigmoids near 1: cdf_delta cancels
  far     x in [-0.99, 0.99]       |delta| in [18, 60]  the pdf branch

Raw log-scales are uniform on [-9, 0] (about a quarter below the floor of -7) and 5 % of them are exactly -7.0 (the
gradient mask is a strict >); mixture logits are N(0, 1.5); coefficients are random.  A candidate row is REJECTED when a
component with posterior weight > 1e-7 lies in a non-edge branch with cdf_delta in (2.5e-6, 4e-5): the two formulas on
either side of the 1e-5 threshold of ops.py:169 differ by up to about 2 nats at narrow scales, so a branch flip between
fp32 and fp64 there is the reference's own behaviour, not an error of a kernel.  Candidates are drawn until every stratum
holds QUOTA rows whose dominant component takes the stratum's branch.

Bound.  With eps = 2^-24 and, per row, from the fp64 oracle's aux,

  kappa = 1 + |nll| + sum_m w_m |mid_in_m| + sum_m w_m [branch = cdf] / cdf_delta_m

an entry is compared at its natural scale:  nll and the mixture-logit gradient  |err| <= c eps kappa;  the mean gradient
|err| / inv_m <= c eps kappa;  the log-scale gradient  |err| / (1 + |mid_in_m|) <= c eps kappa;  dx the sum over m of the
mean-gradient bounds.  c comes from the reference evaluated in float32 (``restatement32`` below, NumPy), never from a GPU:
C_CPU holds the worst error / (eps kappa) of the restatement over the designs of MIXTURES, rounded up, and C_GPU = 4 C_CPU
(the device's expf / log1pf / division each differ from NumPy's by an ulp or two and are chained about four deep).
"""
from collections import namedtuple

import numpy as np

from oracle import wavenet_np as O

EPS = 2.0 ** -24
MIXTURES = [1, 8, 9, 16]          # the eight-lane boundary of row_mol_nll (lane j owns j and j + 8) and the ABI's maximum
STRATA = ["edge-", "edge+", "centre", "lower", "upper", "far"]
BRANCH = [0, 1, 2, 2, 2, 3]       # the case of O.mol_log_probs' aux the dominant component of a stratum's row takes
QUOTA = 128
BATCH = 256                       # candidate rows per stratum and round
LIVE = 1e-7                       # posterior weight from which a component counts
BAND = (2.5e-6, 4e-5)             # cdf_delta of a live non-edge component: rejected (ops.py:169's threshold is 1e-5)
QUANTITIES = ["nll", "logit", "mean", "log_scale", "dx"]

# Worst error / (eps kappa) of restatement32 against the fp64 oracle over design(M), M in MIXTURES, per quantity, as
# tests/test_mol_design.py measures it (pytest -s prints the figures), rounded up to the next half so that another NumPy
# build's exp / log1p (an ulp apart) stays inside:
#   measured   nll 4.16   logit 2.36   mean 1.30   log_scale 2.25   dx 1.28
# The GPU tests assert 4 x these and print what they measure (SRWN_PRINT_ERR=1); tests/test_gpu_mol_entries.py's header
# records the figures of the MI355X next to them.
C_CPU = {"nll": 4.5, "logit": 2.5, "mean": 1.5, "log_scale": 2.5, "dx": 1.5}
C_GPU = {k: 4.0 * v for k, v in C_CPU.items()}

Design = namedtuple("Design", "M x l stratum ref aux w nll kappa rejected candidates")


def _draw(rng, M, n):
    """n candidate rows per stratum, interleaved (row i is of stratum i % 6), in float32."""
    N = n * len(STRATA)
    s = np.arange(N) % len(STRATA)
    x = rng.uniform(-0.99, 0.99, N)
    x[s == 0] = rng.choice([-1.0, -0.9995], (s == 0).sum())
    x[s == 1] = rng.choice([1.0, 0.9995], (s == 1).sum())
    x = x.astype(np.float32)
    raw = rng.uniform(-9.0, 0.0, (N, M))
    raw[rng.random((N, M)) < 0.05] = -7.0
    raw = raw.astype(np.float32)
    delta = rng.standard_normal((N, M))
    tail = rng.uniform(3.0, 9.0, (N, M))
    far = rng.uniform(18.0, 60.0, (N, M)) * rng.choice([-1.0, 1.0], (N, M))
    sk = s[:, None]
    delta = np.where(sk == 3, -tail, np.where(sk == 4, tail, np.where(sk == 5, far, delta)))
    scale = np.exp(np.maximum(raw.astype(np.float64), -7.0))
    l = np.empty((N, 4 * M), np.float32)
    l[:, :M] = rng.normal(0.0, 1.5, (N, M))
    l[:, M:2 * M] = x.astype(np.float64)[:, None] - delta * scale
    l[:, 2 * M:3 * M] = raw
    l[:, 3 * M:] = rng.standard_normal((N, M))
    return x, l, s


def reference(x, l):
    """The fp64 oracle on float32 (x [N], l [N, 4M]): dict of nll [N], g = d sum(nll) / dl [N, 4M], dx [N], aux, w [N, M]
    (the posterior weights) and kappa [N]."""
    x64, l64 = x.astype(np.float64), l.astype(np.float64)
    lp, aux = O.mol_log_probs(x64, l64)
    nll = -O.log_sum_exp(lp)
    w = O.softmax(lp)
    cdf = np.where(aux["case"] == 2, 1.0 / np.maximum(aux["cdf_delta"], 1e-300), 0.0)
    kappa = 1.0 + np.abs(nll) + (w * np.abs(aux["mid_in"])).sum(-1) + (w * cdf).sum(-1)
    g = O.mol_dlogits(x64, l64)
    return dict(nll=nll, g=g, dx=O.mol_dx(x64, l64), aux=aux, w=w, kappa=kappa)


_DESIGNS = {}


def design(M, seed=20240):
    """The design of M mixtures: computed once, shared, read-only."""
    if M in _DESIGNS:
        return _DESIGNS[M]
    rng = np.random.default_rng(seed + M)
    xs, ls, ss = [], [], []
    count = np.zeros(len(STRATA), int)
    candidates = rejected = 0
    while count.min() < QUOTA:
        x, l, s = _draw(rng, M, BATCH)
        r = reference(x, l)
        a = r["aux"]
        band = (r["w"] > LIVE) & (a["case"] >= 2) & (a["cdf_delta"] > BAND[0]) & (a["cdf_delta"] < BAND[1])
        keep = ~band.any(-1)
        candidates += len(x); rejected += int((~keep).sum())
        xs.append(x[keep]); ls.append(l[keep]); ss.append(s[keep])
        dom = np.take_along_axis(a["case"], r["w"].argmax(-1)[:, None], 1)[:, 0]
        for k in range(len(STRATA)):
            count[k] += int((keep & (s == k) & (dom == BRANCH[k])).sum())
        assert candidates <= 40 * BATCH * len(STRATA), "the design does not fill its quotas: %s" % count
    x, l, s = np.concatenate(xs), np.concatenate(ls), np.concatenate(ss)
    r = reference(x, l)
    for a in (x, l, s, r["nll"], r["g"], r["dx"], r["w"], r["kappa"]) + tuple(r["aux"].values()):
        a.setflags(write=False)
    d = Design(M, x, l, s, r, r["aux"], r["w"], r["nll"], r["kappa"], rejected, candidates)
    check(d)
    _DESIGNS[M] = d
    return d


def check(d):
    """What the tests rely on: every stratum holds QUOTA rows on its branch, the branch most of its rows' dominant
    components take is the intended one, and few rows leave the log-scale gradient nothing to check."""
    dom = dominant_branch(d)
    for k, name in enumerate(STRATA):
        rows = d.stratum == k
        hits = np.bincount(dom[rows], minlength=4)
        assert hits[BRANCH[k]] >= QUOTA, (d.M, name, hits)
        assert hits.argmax() == BRANCH[k] and 10 * hits[BRANCH[k]] >= 9 * hits.sum(), (d.M, name, hits)
    share = float(clamped_only(d).mean())
    if d.M > 1:
        assert share < 0.05, (d.M, share)
    else:      # one component: the row is clamped-only whenever its one raw log-scale is, 0.05 + 0.95 * 2 / 9 = 0.26 of them
        assert 0.18 < share < 0.34, share
    assert np.unique(d.aux["case"]).tolist() == [0, 1, 2, 3]
    assert (d.l[:, 2 * d.M:3 * d.M] == -7.0).mean() > 0.03


def dominant_branch(d):
    """The case of the component with the largest posterior weight, per row."""
    return np.take_along_axis(d.aux["case"], d.w.argmax(-1)[:, None], 1)[:, 0]


def clamped_only(d):
    """Rows on which every live component's raw log-scale is at or below -7: their log-scale gradient is all zeros."""
    return ((d.w <= LIVE) | ~d.aux["clamp"]).all(-1)


# ---- the bounds ---------------------------------------------------------------------------------------------------------
def scales(ref, M):
    """The natural scale eps kappa [..] of every quantity, without c: dict nll [N], logit / mean / log_scale [N, M], dx [N]."""
    a = ref["aux"]
    ek = EPS * ref["kappa"]
    mean = ek[:, None] * a["inv"]
    return dict(nll=ek, logit=np.broadcast_to(ek[:, None], mean.shape), mean=mean,
                log_scale=ek[:, None] * (1.0 + np.abs(a["mid_in"])), dx=mean.sum(-1))


def ratios(ref, M, nll=None, g=None, dx=None, grad_scale=1.0, extra=None):
    """error / (eps kappa at the entry's natural scale) of what is given, per quantity: dict name -> array.  g [N, >=3M]
    holds d loss / dl * grad_scale; extra [N, 3M] (bf16 outputs: 2^-8 |ref entry|) is taken off an entry's error first."""
    sc = scales(ref, M)
    out = {}
    if nll is not None:
        out["nll"] = np.abs(np.asarray(nll, np.float64) - ref["nll"]) / sc["nll"]
    if g is not None:
        err = np.abs(np.asarray(g, np.float64)[:, :3 * M] - grad_scale * ref["g"][:, :3 * M])
        if extra is not None:
            err = np.maximum(err - extra, 0.0)
        for i, k in enumerate(("logit", "mean", "log_scale")):
            out[k] = err[:, i * M:(i + 1) * M] / (abs(grad_scale) * sc[k])
    if dx is not None:
        out["dx"] = np.abs(np.asarray(dx, np.float64) - grad_scale * ref["dx"]) / (abs(grad_scale) * sc["dx"])
    return out


def worst(r):
    return {k: float(v.max()) for k, v in r.items()}


def partial_bounds(ref, rows, c_nll):
    """Per 256-row block of the first ``rows`` rows: (the oracle's sum of the block's own nll, the bound on a fp32
    partial of it = the sum of the rows' nll bounds + 256 eps sum |nll|)."""
    nll, ek = ref["nll"][:rows], EPS * ref["kappa"][:rows]
    nb = (rows + 255) // 256
    want = np.array([nll[b * 256:(b + 1) * 256].sum() for b in range(nb)])
    tol = np.array([c_nll * ek[b * 256:(b + 1) * 256].sum() + 256 * EPS * np.abs(nll[b * 256:(b + 1) * 256]).sum()
                    for b in range(nb)])
    return want, tol


# ---- the reference at fp32 ----------------------------------------------------------------------------------------------
def restatement32(x, l):
    """O.mol_log_probs / O.mol_dlogits / O.mol_dx line by line with every operand and result a float32 (the oracle's own
    functions upcast in log_prob_from_logits): (nll [N], g [N, 4M], dx [N]) in float32 and the branch taken [N, M]."""
    f = np.float32
    x, l = x.astype(f), l.astype(f)
    M = l.shape[-1] // 4

    def softplus(v):
        return np.logaddexp(f(0.0), v)

    def sigmoid(v):
        with np.errstate(over="ignore"):
            return f(1.0) / (f(1.0) + np.exp(-v))

    def log_softmax(v):
        m = v.max(-1, keepdims=True)
        return v - m - np.log(np.exp(v - m).sum(-1, keepdims=True, dtype=f))

    def softmax(v):
        e = np.exp(v - v.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True, dtype=f)

    logit_probs, means, raw = l[:, :M], l[:, M:2 * M], l[:, 2 * M:3 * M]
    ls = np.maximum(raw, f(-7.0))
    xx = x[:, None]
    cen = xx - means
    inv = np.exp(-ls)
    plus_in = inv * (cen + f(1.0) / f(255.0))
    min_in = inv * (cen - f(1.0) / f(255.0))
    mid_in = inv * cen
    sp, smn, smd = sigmoid(plus_in), sigmoid(min_in), sigmoid(mid_in)
    cdf_delta = sp - smn
    case = np.where(xx < f(-0.999), 0, np.where(xx > f(0.999), 1, np.where(cdf_delta > f(1e-5), 2, 3)))
    den = np.maximum(cdf_delta, f(1e-12))
    comp = np.select([case == 0, case == 1, case == 2],
                     [plus_in - softplus(plus_in), -softplus(min_in), np.log(den)],
                     mid_in - ls - f(2.0) * softplus(mid_in) - np.log(f(127.5)))
    lp = comp + log_softmax(logit_probs)
    m = lp.max(-1)
    nll = -(m + np.log(np.exp(lp - m[:, None]).sum(-1, dtype=f)))
    w = softmax(lp)
    g = np.zeros_like(l)
    g[:, :M] = -(w - softmax(logit_probs))
    one = f(1.0)
    dm = np.select([case == 0, case == 1, case == 2],
                   [(one - sp) * -inv, -smn * -inv, (sp * (one - sp) * -inv - smn * (one - smn) * -inv) / den],
                   (one - f(2.0) * smd) * -inv)
    ds = np.select([case == 0, case == 1, case == 2],
                   [(one - sp) * -plus_in, -smn * -min_in, (sp * (one - sp) * -plus_in - smn * (one - smn) * -min_in) / den],
                   (one - f(2.0) * smd) * -mid_in - one)
    g[:, M:2 * M] = -w * dm
    g[:, 2 * M:3 * M] = -w * ds * (raw > f(-7.0))
    dx = -g[:, M:2 * M].sum(-1, dtype=f)
    assert nll.dtype == f and g.dtype == f and dx.dtype == f and case.dtype.kind == "i"
    return nll, g, dx, case


# ---- the comparison x < -0.999 / x > 0.999 ------------------------------------------------------------------------------
def threshold_block(M):
    """Rows around the float32 comparison against -0.999f / 0.999f, which the reference evaluates on float32 tensors: x is
    float32(-+0.999) and its two float32 neighbours, log-scales >= -2 (one ulp of x moves the nll by less than 1e-6).
    Returns (x [6 R] float32, l [6 R, 4M] float32, edge [6 R] bool, ref): the threshold value and its inner neighbour are
    interior, the outer neighbour is edge, and ref is the fp64 oracle of an x nudged by 1e-7 to that side."""
    rng = np.random.default_rng(77 + M)
    R = 8
    lo, hi = np.float32(-0.999), np.float32(0.999)
    inf = np.float32(np.inf)
    xs = np.array([np.nextafter(lo, -inf), lo, np.nextafter(lo, inf), np.nextafter(hi, -inf), hi, np.nextafter(hi, inf)],
                  np.float32)
    edge = np.array([True, False, False, False, False, True])
    side = np.array([-1.0, 1.0, 1.0, -1.0, -1.0, 1.0])         # where the fp64 oracle's x is nudged to
    x = np.repeat(xs, R); edge = np.repeat(edge, R); side = np.repeat(side, R)
    N = len(x)
    l = np.empty((N, 4 * M), np.float32)
    l[:, :M] = rng.normal(0.0, 1.5, (N, M))
    raw = rng.uniform(-2.0, 0.0, (N, M))
    l[:, M:2 * M] = x.astype(np.float64)[:, None] - rng.standard_normal((N, M)) * np.exp(raw)
    l[:, 2 * M:3 * M] = raw
    l[:, 3 * M:] = rng.standard_normal((N, M))
    x64 = x.astype(np.float64) + 1e-7 * side
    assert np.array_equal(x64 < -0.999, edge & (x < 0)) and np.array_equal(x64 > 0.999, edge & (x > 0))
    lp, aux = O.mol_log_probs(x64, l.astype(np.float64))
    nll = -O.log_sum_exp(lp)
    w = O.softmax(lp)
    cdf = np.where(aux["case"] == 2, 1.0 / np.maximum(aux["cdf_delta"], 1e-300), 0.0)
    kappa = 1.0 + np.abs(nll) + (w * np.abs(aux["mid_in"])).sum(-1) + (w * cdf).sum(-1)
    # the other side's value is far from this one, so a kernel on the wrong side cannot pass
    other = -O.log_sum_exp(O.mol_log_probs(x.astype(np.float64) - 1e-6 * side, l.astype(np.float64))[0])
    return x, l, edge, dict(nll=nll, kappa=kappa, aux=aux, w=w, other=other)
