"""CPU tests of the input designs and bounds the per-entry GPU tests rest on (tests/mol_design.py, tests/stft_design.py;
the GPU side is tests/test_gpu_mol_entries.py).  pytest -s prints every measured figure.

  design       quotas, the dominant branch per stratum, exact -7.0 log-scales, few clamped-only rows, float32 values; the
               rejected share is printed (3.9 % .. 28.6 % for M = 1 .. 16)
  restatement  the oracle restated in float32 takes the fp64 oracle's branch on every live component and stays within
               C_CPU = C_GPU / 4 of it, per quantity, at each entry's natural scale
  bound        the bound has teeth where max|a - b| / max|b| has none: a flipped sign in the mixture-logit block, a mask that
               lets raw == -7.0 through and a row's NLL off by 0.01 nat all break it
  threshold    the block around x = -+0.999: the fp64 expectation follows the float32 comparison
  stft         the float32 direct DFT against the fp64 oracle, bin by bin
"""
import numpy as np
import pytest

from oracle import wavenet_np as O
from tests import mol_design as D
from tests import stft_design as SD


@pytest.mark.parametrize("M", D.MIXTURES + [5, 10])
def test_design_quotas_and_branches(M):
    d = D.design(M)                       # (design() runs check(): quotas, dominant branches, clamped-only rows)
    D.check(d)
    share = d.rejected / d.candidates
    print("M=%d: %d rows kept of %d candidates, %.1f %% rejected, %.1f %% clamped-only, strata %s" % (
        M, len(d.x), d.candidates, 100 * share, 100 * D.clamped_only(d).mean(), np.bincount(d.stratum).tolist()))
    assert 0.0 < share < 0.4
    assert d.x.dtype == np.float32 and d.l.dtype == np.float32 and d.l.shape == (len(d.x), 4 * M)
    assert len(d.x) >= 257                # the row counts 1, 255, 256, 257 come from the head
    assert len(set(d.stratum[:255].tolist())) == 6
    a = d.aux
    band = (d.w > D.LIVE) & (a["case"] >= 2) & (a["cdf_delta"] > D.BAND[0]) & (a["cdf_delta"] < D.BAND[1])
    assert not band.any()
    assert np.isfinite(d.nll).all() and np.isfinite(d.ref["g"]).all() and np.isfinite(d.kappa).all()
    # the design is what the GPU tests are for: one tensor that mixes magnitudes
    g = np.abs(d.ref["g"])
    if M > 1:
        assert g[:, M:3 * M].max() > 100 * g[:, :M].max()


@pytest.mark.parametrize("M", D.MIXTURES)
def test_float32_restatement_within_a_quarter_of_the_gpu_bound(M):
    d = D.design(M)
    nll, g, dx, case = D.restatement32(d.x, d.l)
    assert not ((case != d.aux["case"]) & (d.w > D.LIVE)).any()
    got = D.worst(D.ratios(d.ref, M, nll=nll, g=g, dx=dx))
    print("M=%d restatement32 error / (eps kappa): %s" % (M, {k: round(v, 2) for k, v in got.items()}))
    for k in D.QUANTITIES:
        assert got[k] <= D.C_CPU[k], (k, got[k])
        assert D.C_GPU[k] == 4 * D.C_CPU[k]
    want, tol = D.partial_bounds(d.ref, len(d.x), D.C_CPU["nll"])
    part = np.array([nll[b * 256:(b + 1) * 256].sum(dtype=np.float32) for b in range(len(want))])
    assert (np.abs(part - want) <= tol).all()


def test_float32_restatement_against_the_oracle_on_plain_inputs():
    """restatement32 is the oracle's arithmetic: in fp64 terms the two agree to float32 rounding on benign rows."""
    rng = np.random.default_rng(1)
    M = 5
    x = rng.uniform(-0.9, 0.9, 200).astype(np.float32)
    l = rng.standard_normal((200, 4 * M)).astype(np.float32)
    r = D.reference(x, l)
    nll, g, dx, _ = D.restatement32(x, l)
    assert np.abs(nll - r["nll"]).max() < 1e-4
    assert np.abs(g - r["g"]).max() < 1e-3 * np.abs(r["g"]).max()
    assert np.abs(dx - r["dx"]).max() < 1e-3 * np.abs(r["dx"]).max()


@pytest.mark.parametrize("M", [8, 9])
def test_bound_bites_where_max_over_max_does_not(M):
    d = D.design(M)
    g = d.ref["g"]

    def rel_err(a, b):
        return np.abs(a - b).max() / np.abs(b).max()

    def breaks(bad, k):
        return D.worst(D.ratios(d.ref, M, g=bad))[k] > D.C_GPU[k]

    flipped = g.copy()                                          # the sign of the mixture-logit block, wherever |g| < 0.4
    flipped[:, :M] = np.where(np.abs(g[:, :M]) < 0.4, -g[:, :M], g[:, :M])
    assert rel_err(flipped, g) < 1e-3 and breaks(flipped, "logit")
    # a mask that lets raw == -7.0 through: the unmasked gradient of those entries
    l64 = d.l.astype(np.float64)
    at = l64[:, 2 * M:3 * M] == -7.0
    nudged = l64.copy(); nudged[:, 2 * M:3 * M][at] += 1e-9
    unmasked = g.copy()
    unmasked[:, 2 * M:3 * M][at] = O.mol_dlogits(d.x.astype(np.float64), nudged)[:, 2 * M:3 * M][at]
    assert (g[:, 2 * M:3 * M][at] == 0).all() and (unmasked[:, 2 * M:3 * M][at] != 0).any()
    assert breaks(unmasked, "log_scale")
    off = d.nll + 0.01 * (d.stratum == 2)                      # the centre rows' NLL off by 0.01 nat
    assert np.abs(off - d.nll).max() < 1e-3 * np.abs(d.nll).max()
    assert D.worst(D.ratios(d.ref, M, nll=off))["nll"] > D.C_GPU["nll"]


@pytest.mark.parametrize("M", D.MIXTURES)
def test_threshold_block(M):
    x, l, edge, ref = D.threshold_block(M)
    f = np.float32
    assert np.array_equal((x < f(-0.999)) | (x > f(0.999)), edge)          # the float32 comparison the kernels make
    assert set(np.unique(x).tolist()) == {float(v) for v in np.unique(x)} and len(np.unique(x)) == 6
    case = ref["aux"]["case"]
    assert np.array_equal((case < 2).all(-1), edge) and np.array_equal((case >= 2).all(-1), ~edge)
    assert (l[:, 2 * M:3 * M] >= -2.0).all()
    # one ulp of x moves the nll by less than 1e-6; the other side of the comparison lies far outside the bound
    moved = -O.log_sum_exp(O.mol_log_probs(np.nextafter(x, f(0)).astype(np.float64), l.astype(np.float64))[0])
    same = np.nextafter(x, f(0)) != f(0.999)                              # (the inner neighbour of an edge x is interior)
    same &= np.nextafter(x, f(0)) != f(-0.999)
    assert np.abs(moved - ref["nll"])[same].max() < 1e-6
    bound = 2 * D.C_GPU["nll"] * D.EPS * ref["kappa"]
    assert (np.abs(ref["other"] - ref["nll"]) > 100 * bound).all()
    nll, _, _, c32 = D.restatement32(x, l)
    assert np.array_equal(c32, case)
    assert (np.abs(nll - ref["nll"]) <= D.C_CPU["nll"] * D.EPS * ref["kappa"] + 1e-6).all()


@pytest.mark.parametrize("T", SD.LENGTHS)
def test_stft_float32_reference(T):
    r = SD.reference(T)
    nf = SD.frames_of(T)
    assert nf == {512: 1, 768: 2, 1000: 2}[T] and T - (nf + 1) * SD.FS == {512: 0, 768: 0, 1000: 232}[T]
    print("T=%d: float32 direct DFT, worst per-bin relative error %.3g; one-bin gradient, worst error / max %.3g; "
          "power %.3g .. %.3g" % (T, r["fwd32"], r["bwd32"], r["power"].min(), r["power"].max()))
    assert 0 < r["fwd32"] < 1e-4 and 0 < r["bwd32"] < 1e-4
    assert r["power"].max() < 1e4 * r["power"].min()          # white noise: no bin hides behind another
    for f in SD.BINS:
        g = r["grads"][f]
        assert (g[:, (nf + 1) * SD.FS:] == 0).all() and np.abs(g).max() > 0
        x, peak, err = SD.tone_reference(T, f)
        assert err <= r["fwd32"] * 4, (f, err)
