"""GPU tests that hold the mixture-of-logistics (MoL) loss kernels and the STFT power kernels to the fp64 oracle ENTRY BY
ENTRY, each entry at its own natural scale, where max|a - b| / max|b| checks nothing because one tensor mixes magnitudes
(a dlogits row holds mixture-logit gradients <= 1 beside mean gradients up to e^7 and log-scale gradients of |mid_in|).

  loss        srwn_mol_loss: the three column blocks of dlogits per entry (fp32 and bf16, grad_scale 1 and 0.37, leading
              dimensions 4M and padded with the padding of the logits poisoned), columns [3M, ldd) and masked log-scale entries
              (raw <= -7, raw == -7.0 among them) exactly 0, every 256-row loss partial against the oracle's sum over its own
              rows; row counts 1, 255, 256, 257
  dx          srwn_mol_loss_dx: dx per row and the same partials
  rows        srwn_mol_nll_rows per row through a strided ldl; srwn_mol_score_rows and srwn_mol_score_rows_slots per row
              with two streams / three slots, n no multiple of 32, a slot that ran fewer rows and one that ran none; rows
              the header calls untouched keep their poison
  agreement   the three NLL implementations (srwn_pool.hip, srwn_ops.hip, srwn_score.hip) pairwise per row, and all three on
              the block around the float32 comparison x < -0.999 / x > 0.999
  stft        srwn_stft_power bin by bin on white noise and on pure tones at bins 0, 1, 128, 255, 256; srwn_stft_power_bwd
              with a one-hot dpower at each of those bins, plain and accumulating

The inputs, the bounds and where their constants come from: tests/mol_design.py and tests/stft_design.py (checked on the
CPU by tests/test_mol_design.py).  Every bound is 4 x what the REFERENCE evaluated in float32 (NumPy) measures against the
fp64 oracle; none is taken from a GPU run.  SRWN_PRINT_ERR=1 pytest -s prints every measured figure.

Worst error / (eps kappa at the entry's natural scale), eps = 2^-24, over M = 1, 8, 9, 16:
                       nll     logit   mean    log_scale   dx
  float32 NumPy (CPU)  4.16    2.36    1.30    2.25        1.28      -> C_CPU 4.5 2.5 1.5 2.5 1.5 (rounded up)
  bound = 4 x C_CPU    18      10      6       10          6
  MI355X, measured     4.85    4.04    1.50    2.20        0.91      (nll: srwn_score.hip 4.85, srwn_pool.hip and srwn_ops.hip
                                                                      4.48; bf16 dlogits: <= 0.3 beyond the output rounding)
  the three NLL implementations against each other, per row: <= 6.84 (bound 2 x 18); the threshold block: <= 3.55
  256-row loss partials: <= 0.022 of their bound
STFT, worst per-bin relative error of the power, T = 512 / 768 / 1000:
  float32 direct DFT (CPU)   5.60e-6 / 2.35e-6 / 1.82e-6      bound = 4 x;   one-bin gradient, error / max: 5.3e-7 / 8.7e-7 / 7.2e-7
  MI355X, measured           3.86e-6 / 2.35e-6 / 1.92e-6 (Nyquist bin 2.6e-6 / 4.0e-7 / 1.2e-7; tones 1.2e-7);
                             one-bin gradient 8.8e-7 / 9.4e-7 / 7.2e-7 (accumulating 8.7e-7 / 9.5e-7 / 7.2e-7)
"""
import os

import numpy as np
import pytest
import torch

from tests import mol_design as D
from tests import stft_design as SD
from tests._pkg import sub

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
POISON = -5.0


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _dev(a, dt=F32):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


def _padded(M):
    return 64 if 4 * M < 64 else 96


def _logits(l, ld, first_poisoned):
    """l [N, 4M] in a device buffer [N, ld] whose columns from first_poisoned on are NaN (never read, says the header)."""
    out = torch.full((l.shape[0], ld), NAN, dtype=F32, device=DEV)
    keep = min(first_poisoned, l.shape[1])
    out[:, :keep] = _dev(l[:, :keep])
    return out


def _check(what, r, keys=None):
    got = D.worst(r)
    _say("%-44s %s" % (what, "  ".join("%s %.2f (<= %g)" % (k, v, D.C_GPU[k]) for k, v in got.items())))
    for k in keys or got:
        bad = np.argwhere(r[k] > D.C_GPU[k])
        assert len(bad) == 0, "%s: %s error / (eps kappa) %.3g > %g at %s (%d entries)" % (
            what, k, got[k], D.C_GPU[k], bad[0].tolist(), len(bad))


def _check_partials(what, parts, ref, rows):
    want, tol = D.partial_bounds(ref, rows, D.C_GPU["nll"])
    got = parts.double().cpu().numpy()
    assert got.shape == want.shape
    _say("%-44s partials: worst error / bound %.3f" % (what, float((np.abs(got - want) / tol).max())))
    assert (np.abs(got - want) <= tol).all(), (what, got - want, tol)


# ---- srwn_mol_loss ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("padded,gs", [(False, 1.0), (True, 0.37)], ids=["ld4M-gs1", "ldpad-gs0.37"])
@pytest.mark.parametrize("M", D.MIXTURES)
def test_mol_loss_per_entry(M, padded, gs, dt):
    K = sub("kernels")
    d = D.design(M)
    N = len(d.x)
    ld = _padded(M) if padded else 4 * M
    lg = _logits(d.l, ld, 4 * M)
    nb = (N + 255) // 256
    parts = torch.full((nb + 1,), POISON, dtype=F32, device=DEV)
    dl = torch.full((N, ld), NAN, dtype=dt, device=DEV)
    K.mol_loss(lg, _dev(d.x), M, parts, dl, gs)
    torch.cuda.synchronize()
    g = dl.double().cpu().numpy()
    assert np.isfinite(g).all()
    assert (g[:, 3 * M:] == 0).all(), "columns [3M, ldd) are written as 0"
    masked = d.l[:, 2 * M:3 * M] <= -7.0
    assert masked.any() and (d.l[:, 2 * M:3 * M] == -7.0).any()
    assert (g[:, 2 * M:3 * M][masked] == 0).all(), "log-scale gradient below or AT the floor (raw > -7 is strict)"
    assert (g[:, 2 * M:3 * M][~masked & (d.w > D.LIVE)] != 0).any()
    extra = 2.0 ** -8 * np.abs(gs * d.ref["g"][:, :3 * M]) if dt == BF16 else None
    what = "mol_loss M=%d ld=%d gs=%g %s" % (M, ld, gs, "bf16" if dt == BF16 else "fp32")
    _check(what, D.ratios(d.ref, M, g=g, grad_scale=gs, extra=extra))
    assert float(parts[nb]) == POISON
    _check_partials(what, parts[:nb], d.ref, N)


@pytest.mark.parametrize("rows", [1, 255, 256, 257])
@pytest.mark.parametrize("M", D.MIXTURES)
def test_mol_loss_row_counts(M, rows):
    """The design's head: the last block's rows beyond ``rows`` (real rows of the design) stay out of its partial, and
    neither their dlogits nor a further partial is written."""
    L = sub("_lib"); K = sub("kernels")
    d = D.design(M)
    ld = _padded(M)
    lg = _logits(d.l[:300], ld, 4 * M)
    x = _dev(d.x[:300])
    nb = (rows + 255) // 256
    head = {k: ({a: b[:rows] for a, b in v.items()} if k == "aux" else v[:rows]) for k, v in d.ref.items()}
    for with_dx in (False, True):
        parts = torch.full((3,), POISON, dtype=F32, device=DEV)
        if with_dx:
            dx = torch.full((300,), POISON, dtype=F32, device=DEV)
            L.call("srwn_mol_loss_dx", lg.data_ptr(), ld, x.data_ptr(), M, parts.data_ptr(), dx.data_ptr(), rows, 0.37,
                   K._stream())
            torch.cuda.synchronize()
            assert (dx[rows:] == POISON).all()
            r = D.ratios(head, M, dx=dx[:rows].double().cpu().numpy(), grad_scale=0.37)
        else:
            dl = torch.full((300, ld), POISON, dtype=F32, device=DEV)
            L.call("srwn_mol_loss", lg.data_ptr(), ld, x.data_ptr(), M, parts.data_ptr(), dl.data_ptr(), ld, rows, 1.0,
                   K.abi_dtype(F32), K._stream())
            torch.cuda.synchronize()
            assert (dl[rows:] == POISON).all()
            r = D.ratios(head, M, g=dl[:rows].double().cpu().numpy())
        what = "mol_loss%s M=%d rows=%d" % ("_dx" if with_dx else "", M, rows)
        _check(what, r)
        assert (parts[nb:] == POISON).all()
        _check_partials(what, parts[:nb], d.ref, rows)


# ---- srwn_mol_loss_dx ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padded,gs", [(False, 1.0), (True, 0.37)], ids=["ld4M-gs1", "ldpad-gs0.37"])
@pytest.mark.parametrize("M", D.MIXTURES)
def test_mol_loss_dx_per_row(M, padded, gs):
    K = sub("kernels")
    d = D.design(M)
    N = len(d.x)
    ld = _padded(M) if padded else 4 * M
    lg = _logits(d.l, ld, 4 * M)
    nb = (N + 255) // 256
    parts = torch.full((nb,), POISON, dtype=F32, device=DEV)
    dx = torch.full((N,), NAN, dtype=F32, device=DEV)
    K.mol_loss_dx(lg, _dev(d.x), M, parts, dx, gs)
    torch.cuda.synchronize()
    what = "mol_loss_dx M=%d ld=%d gs=%g" % (M, ld, gs)
    _check(what, D.ratios(d.ref, M, dx=dx.double().cpu().numpy(), grad_scale=gs))
    _check_partials(what, parts, d.ref, N)


# ---- the three NLL implementations, per row -----------------------------------------------------------------------------
def _pool_nll(x, l, M, ld):
    """srwn_pool.hip's NLL per row: srwn_mol_loss_dx on one row at a time (its only per-row output is the partial of a
    block, so a block of one row).  float64 [N]."""
    L = sub("_lib"); K = sub("kernels")
    N = len(x)
    lg = _logits(l, ld, 4 * M)
    xd = _dev(x)
    out = torch.full((N,), NAN, dtype=F32, device=DEV)
    dx = torch.empty((N,), dtype=F32, device=DEV)
    st = K._stream()
    pl, px, po, pd = lg.data_ptr(), xd.data_ptr(), out.data_ptr(), dx.data_ptr()
    for i in range(N):
        L.call("srwn_mol_loss_dx", pl + 4 * ld * i, ld, px + 4 * i, M, po + 4 * i, pd + 4 * i, 1, 1.0, st)
    torch.cuda.synchronize()
    return out.double().cpu().numpy()


def _ops_nll(x, l, M, ld):
    """srwn_mol_nll_rows through a strided ldl.  float64 [N]."""
    L = sub("_lib"); K = sub("kernels")
    N = len(x)
    lg = _logits(l, ld, 4 * M)
    xd = _dev(x)
    out = torch.full((N + 3,), POISON, dtype=F32, device=DEV)
    L.call("srwn_mol_nll_rows", lg.data_ptr(), ld, xd.data_ptr(), M, out.data_ptr(), N, K._stream())
    torch.cuda.synchronize()
    assert (out[N:] == POISON).all()
    return out[:N].double().cpu().numpy()


def _table(ran):
    return torch.tensor([[7, 7 + r] for r in ran], dtype=torch.int64, device=DEV)      # SrwnSynthSlot: (t, t_end)


def _score_nll(x, l, M, ld, slots):
    """srwn_mol_score_rows (two streams) or srwn_mol_score_rows_slots (three slots: one runs the whole chunk, one 37 rows
    fewer, one none) on the rows of (x, l) dealt to the streams in turn; columns from 3M on, the buffers' rows behind the
    chunk and the idle slot's rows are NaN.  float64 [N]: row i's value from the first stream that scored it."""
    L = sub("_lib"); K = sub("kernels")
    N = len(x)
    n = (N + 1) // 2
    if n % 32 == 0:
        n += 1
    ran = [n, max(n - 37, 1), 0] if slots else [n, n]
    Bn = len(ran)
    clip, xs, os_ = n + 5, n + 3, n + 7
    idx = (np.arange(Bn)[:, None] * n + np.arange(n)[None, :]) % N                      # the design row of (stream, t)
    lg = torch.full((Bn, clip, ld), NAN, dtype=F32, device=DEV)
    xb = torch.full((Bn, xs), NAN, dtype=F32, device=DEV)
    for b in range(Bn):
        if ran[b]:
            lg[b, :n, :3 * M] = _dev(l[idx[b]][:, :3 * M])
            xb[b, :n] = _dev(x[idx[b]])
    nll = torch.full((Bn, os_), POISON, dtype=F32, device=DEV)
    lo = torch.full((Bn, os_, 4 * M), POISON, dtype=F32, device=DEV)
    args = [lg.data_ptr(), ld, clip, xb.data_ptr(), xs, nll.data_ptr(), lo.data_ptr(), os_, Bn, n, M]
    if slots:
        table = _table(ran)
        L.call("srwn_mol_score_rows_slots", *args, table.data_ptr(), K._stream())
    else:
        L.call("srwn_mol_score_rows", *args, K._stream())
    torch.cuda.synchronize()
    out = np.full(N, np.nan)
    got = nll.double().cpu().numpy()
    for b in reversed(range(Bn)):
        assert (nll[b, ran[b]:] == POISON).all() and (lo[b, ran[b]:] == POISON).all(), "rows >= ran are not touched"
        out[idx[b, :ran[b]]] = got[b, :ran[b]]
        # logits_out takes the real columns as they are (the coefficients' NaN among them)
        assert torch.equal(lo[b, :ran[b], :3 * M], lg[b, :ran[b], :3 * M])
    return out


def _all_nll(x, l, M):
    return {"pool": _pool_nll(x, l, M, _padded(M)), "ops": _ops_nll(x, l, M, _padded(M)),
            "score": _score_nll(x, l, M, 64, False), "slots": _score_nll(x, l, M, 4 * M, True)}


@pytest.mark.parametrize("M", D.MIXTURES)
def test_nll_per_row_and_the_three_implementations_agree(M):
    d = D.design(M)
    got = _all_nll(d.x, d.l, M)
    covered = ~np.isnan(got["slots"])                 # (the slot that ran fewer rows leaves some of the design out)
    assert covered.sum() >= len(d.x) - 40 and not np.isnan(got["score"]).any()
    ek = D.EPS * d.kappa
    for name, v in got.items():
        rows = covered if name == "slots" else np.ones(len(d.x), bool)
        r = np.abs(v[rows] - d.nll[rows]) / ek[rows]
        _say("nll M=%d %-6s error / (eps kappa) %.2f (<= %g), per stratum %s" % (
            M, name, r.max(), D.C_GPU["nll"],
            [round(float(r[d.stratum[rows] == k].max()), 2) for k in range(len(D.STRATA))]))
        assert r.max() <= D.C_GPU["nll"], (name, int(np.argmax(r)), r.max())
    assert np.array_equal(got["score"][covered], got["slots"][covered])      # one device routine
    for a, b in (("pool", "ops"), ("pool", "score"), ("ops", "score")):
        r = np.abs(got[a] - got[b]) / ek
        _say("nll M=%d %s vs %s: %.2f (<= %g)" % (M, a, b, r.max(), 2 * D.C_GPU["nll"]))
        assert r.max() <= 2 * D.C_GPU["nll"], (a, b, int(np.argmax(r)), r.max())


@pytest.mark.parametrize("M", D.MIXTURES)
def test_threshold_comparison_in_float32(M):
    """x = float32(-+0.999) and its two float32 neighbours: all three implementations take the side of the float32
    comparison (the value on the other side lies more than 100 bounds away, tests/test_mol_design.py)."""
    x, l, edge, ref = D.threshold_block(M)
    got = _all_nll(x, l, M)
    ek = D.EPS * ref["kappa"]
    for name, v in got.items():
        rows = ~np.isnan(v)
        assert rows.sum() >= len(x) - 40 if name == "slots" else rows.all()
        r = np.abs(v[rows] - ref["nll"][rows]) / ek[rows]
        _say("threshold M=%d %-6s error / (eps kappa) %.2f" % (M, name, r.max()))
        assert r.max() <= D.C_GPU["nll"], (name, x[rows][np.argmax(r)], edge[rows][np.argmax(r)], r.max())
    assert np.abs(got["pool"] - got["ops"]).max() <= (2 * D.C_GPU["nll"] * ek).max()


# ---- STFT power, bin by bin ---------------------------------------------------------------------------------------------
def _stft(x):
    K = sub("kernels")
    B, T = x.shape
    nf = K.stft_frames(T)
    assert nf == SD.frames_of(T)
    spec = torch.full((B, nf, SD.NB, 2), NAN, device=DEV); fp = torch.full((B, nf, SD.NB), NAN, device=DEV)
    pw = torch.full((B, SD.NB), NAN, device=DEV)
    K.stft_power(_dev(x), spec, fp, pw)
    torch.cuda.synchronize()
    return spec, pw.double().cpu().numpy()


@pytest.mark.parametrize("T", SD.LENGTHS)
def test_stft_power_bin_by_bin(T):
    r = SD.reference(T)
    bound = 4 * r["fwd32"]
    _, pw = _stft(r["x"])
    err = np.abs(pw - r["power"]) / r["power"]
    _say("stft_power T=%d noise: worst per-bin relative error %.3g at bin %d (float32 DFT %.3g, bound %.3g); Nyquist %.3g" % (
        T, err.max(), int(err.max(0).argmax()), r["fwd32"], bound, err[:, 256].max()))
    assert np.isfinite(pw[:, 256]).all(), "the Nyquist bin (thread 0's second trip through the bins) is written"
    assert np.isfinite(pw).all()
    assert (err[:, 256] <= bound).all(), ("the Nyquist bin", err[:, 256], bound)
    assert (err <= bound).all(), (np.argwhere(err > bound)[:5].tolist(), err.max(), bound)
    for f in SD.BINS:
        x, peak, _ = SD.tone_reference(T, f)
        _, pw = _stft(x)
        e = np.abs(pw[:, f] - peak) / peak
        _say("stft_power T=%d tone at bin %d: relative error %.3g" % (T, f, e.max()))
        assert (e <= bound).all(), (f, e, bound)


@pytest.mark.parametrize("T", SD.LENGTHS)
def test_stft_power_bwd_one_bin_at_a_time(T):
    """One bin per run means one scale: dx against oracle (ii)'s autograd of that bin's power, normalised by the run's own
    max.  The bound is 4 x (the float32 backward formula's error + the float32 spectrum's), both of the reference."""
    K = sub("kernels")
    r = SD.reference(T)
    nf = SD.frames_of(T)
    bound = 4 * r["bwd32"]
    spec, _ = _stft(r["x"])
    tail = (nf + 1) * SD.FS
    for f in SD.BINS:
        want = r["grads"][f]
        dpow = torch.zeros((SD.B, SD.NB), device=DEV); dpow[:, f] = 1.0
        dx = torch.full((SD.B, T), NAN, device=DEV)
        K.stft_power_bwd(spec, dpow, dx)
        base = torch.linspace(-1.0, 1.0, SD.B * T, device=DEV).reshape(SD.B, T).contiguous()
        acc = base.clone()
        K.stft_power_bwd(spec, dpow, acc, accumulate=True)
        torch.cuda.synchronize()
        got = dx.double().cpu().numpy()
        e = np.abs(got - want).max() / np.abs(want).max()
        ea = np.abs((acc.double() - base.double()).cpu().numpy() - want).max() / np.abs(want).max()
        _say("stft_power_bwd T=%d bin %d: error / max %.3g, accumulating %.3g (float32 formula %.3g, bound %.3g)" % (
            T, f, e, ea, r["bwd32"], bound))
        assert e <= bound, (f, e, bound)
        # the accumulating form adds to a value of up to 1: one rounding of the sum, 2^-24 of it, on top
        assert ea <= bound + 2.0 ** -24 * (1.0 + np.abs(want).max()) / np.abs(want).max(), (f, ea, bound)
        assert (got[:, tail:] == 0).all() and torch.equal(acc[:, tail:], base[:, tail:])
        assert tail == T or T == 1000
