"""GPU tests of the generators' sampling controls (srwn.h, SrwnGenSampling: temperature, top-k, nucleus).

The rule is restated here in NumPy fp64 (`ref_rule`) and the kernels are held to it draw for draw: through
srwn_sample_filtered on logits this file chooses, and inside the generators on the logits they report.  A draw that
disagrees must be excusable -- the uniform within 1e-4 of an edge of the reference's class in the reference CDF, or a prefix
mass of the nucleus order within 1e-4 of top_p (the window tests/test_gpu_generate.py uses for the plain sampler) -- and
excusable draws are capped at 0.5 % of every (row kind, temperature, top_k, top_p) cell."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev

pytestmark = pytest.mark.gpu

CONTROLS = [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.5, 0, 1.0), (1.0, 8, 1.0), (1.0, 50, 1.0), (1.0, 0, 0.9), (1.0, 0, 0.5),
            (0.8, 40, 0.95), (1.0, 1, 1.0), (1.0, 0, 1e-6)]
WINDOW, CAP = 1e-4, 0.005


def _gen_uniform(seed, u, t):
    """Host replica of the kernels' counter-based generator (splitmix64 finaliser), as tests/test_gpu_generate.py."""
    M64 = (1 << 64) - 1
    x = (seed + 0x9E3779B97F4A7C15 * ((u * 0x100000001 + t + 1) & M64)) & M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return np.float32((np.float32(x >> 40) + np.float32(0.5)) * np.float32(1.0 / 16777216.0))


def ref_rule(logits, tau, k, p, u):
    """The rule of srwn.h in fp64, row by row: logits [n, C] (the kernel's own fp32 values), tau / k / p [n] already
    sanitised as the header says (k = 0: off), u [n].  Returns (codes, excusable [n] bool, kept [n, C] bool)."""
    z = logits.astype(np.float64) / tau[:, None]
    n, Cn = z.shape
    order = np.argsort(-z, axis=1, kind="stable")                    # descending, equal values by lower class first
    zs = np.take_along_axis(z, order, 1)
    rank = np.arange(Cn)[None, :]
    keep_s = rank < np.where(k > 0, k, Cn)[:, None]                  # top-k
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(keep_s, np.exp(zs - zs[:, :1]), 0.0)
    cs = np.cumsum(e, 1)
    frac = cs / cs[:, -1:]
    jstar = (cs >= p[:, None] * cs[:, -1:]).argmax(1)                # shortest prefix with mass >= p * kept mass
    keep_s &= (rank <= jstar[:, None]) | (p[:, None] >= 1.0)
    kept = np.zeros_like(keep_s)
    np.put_along_axis(kept, order, keep_s, 1)
    with np.errstate(invalid="ignore"):
        ec = np.where(kept, np.exp(z - z.max(1, keepdims=True)), 0.0)
    cdf = np.cumsum(ec, 1)
    cdf /= cdf[:, -1:]
    codes = (cdf > u[:, None]).argmax(1)
    hi = cdf[np.arange(n), codes]
    lo = np.where(codes > 0, cdf[np.arange(n), np.maximum(codes - 1, 0)], 0.0)
    near_edge = (np.abs(u - lo) <= WINDOW) | (np.abs(u - hi) <= WINDOW)
    near_p = (p < 1.0) & (np.abs(frac - p[:, None]) <= WINDOW).any(1)
    return codes, near_edge | near_p, kept


def _sanitised(tau, k, p, Cn):
    """What the header says the kernels make of any row."""
    tau = np.asarray(tau, np.float32); p = np.asarray(p, np.float32); k = np.asarray(k, np.int64)
    with np.errstate(invalid="ignore"):
        tau = np.where(np.isfinite(tau) & (tau > 0), tau, np.float32(1))
        p = np.where((p > 0) & (p <= 1), p, np.float32(1))
    k = np.where((k >= 1) & (k < Cn), k, 0)
    return tau.astype(np.float64), k, p.astype(np.float64)


def _table(tau, k, p):
    L = sub("_lib")
    tab = np.zeros(len(tau), dtype=np.dtype(L.SrwnGenSampling))
    tab["temperature"], tab["top_k"], tab["top_p"] = tau, k, p
    return tab


def _filtered(logits, tab, u):
    """srwn_sample_filtered through the C-ABI (no Python-side range checks: hostile rows reach the kernel)."""
    L = sub("_lib")
    x = torch.tensor(logits, dtype=torch.float32, device=DEV).contiguous()
    ud = torch.tensor(u, dtype=torch.float32, device=DEV)
    sd = None if tab is None else torch.from_numpy(tab.view(np.int32).reshape(len(tab), 4).copy()).to(DEV)
    out = torch.full((x.shape[0],), -7, dtype=torch.int32, device=DEV)
    L.call("srwn_sample_filtered", x.data_ptr(), x.shape[1], None if sd is None else sd.data_ptr(), ud.data_ptr(),
           out.data_ptr(), x.shape[0], x.shape[1], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _grid_uniforms(rng, n):
    """Uniforms on the kernels' 24-bit grid (the top point, which rounds to 1.0 in fp32, left out)."""
    i = rng.integers(0, (1 << 24) - 1, n)
    return ((i.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def _hand_rows(rng, Cn):
    """Hand-made rows: all equal; two-way ties straddling the k-th place (k = 1, 8, 40, 50); one class at -inf; one class
    holding 0.999 of the mass.  Returns (rows, tied-or-inf mask)."""
    rows, special = [], []
    rows.append(np.full(Cn, 0.25, np.float32)); special.append(True)
    for kk in (1, 8, 40, 50):
        r = rng.normal(0, 2, Cn).astype(np.float32)
        if kk < Cn:
            o = np.argsort(-r, kind="stable")
            r[o[kk]] = r[o[kk - 1]]                                  # the k-th and (k+1)-th largest are equal
        rows.append(r); special.append(True)
    r = rng.normal(0, 2, Cn).astype(np.float32); r[int(rng.integers(Cn))] = -np.inf
    rows.append(r); special.append(True)
    r = np.zeros(Cn, np.float32); r[int(rng.integers(Cn))] = np.float32(np.log(0.999 * (Cn - 1) / 0.001))
    rows.append(r); special.append(False)
    r = np.zeros(Cn, np.float32); r[3] = -0.0; r[1] = 0.0              # +0 and -0 are one value
    rows.append(r); special.append(True)
    return np.stack(rows), np.array(special)


def _check_cells(got, logits, tau, k, p, u, cell_ids, what):
    """Acceptance of the issue: every disagreement excusable, at most 0.5 % of any cell; never a dropped class."""
    want, excusable, kept = ref_rule(logits, tau, k, p, u)
    Cn = logits.shape[1]
    assert got.min() >= 0 and got.max() < Cn, what
    diff = got != want
    assert not (diff & ~excusable).any(), (what, "unexcused", np.flatnonzero(diff & ~excusable)[:8],
                                           got[diff & ~excusable][:8], want[diff & ~excusable][:8])
    worst = 0.0
    for c in np.unique(cell_ids):
        m = cell_ids == c
        frac = diff[m].mean()
        worst = max(worst, frac)
        if m.sum() >= 200:
            assert frac <= CAP, (what, "cell", c, "disagreeing draws", int(diff[m].sum()), "of", int(m.sum()))
    print("MEASURED %s: %d draws, %d disagree (all excusable), worst cell %.4f" % (what, len(got), int(diff.sum()), worst))
    # the top-k set of the kernel's own fp32 input is exact: a code is never a dropped class
    order = np.argsort(-logits.astype(np.float64), axis=1, kind="stable")
    rk = np.empty_like(order)
    np.put_along_axis(rk, order, np.broadcast_to(np.arange(Cn), order.shape).copy(), 1)
    lim = np.where(k > 0, k, Cn)
    assert (rk[np.arange(len(got)), got] < lim).all(), what
    return want


# ---------------------------------------------------------------------------------------------------------------------
# 1. the rule on chosen logits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [256, 200, 37])
def test_filtered_draw_follows_the_rule(Cn):
    rng = np.random.default_rng(100 + Cn)
    N = 1500
    logits, tau, k, p, cell, special = [], [], [], [], [], []
    hand, hand_special = _hand_rows(rng, Cn)
    cid = 0
    for ci, (t_, k_, p_) in enumerate(CONTROLS):
        for sigma in (0.05, 0.3, 2.0, 5.0):
            logits.append(rng.normal(0, sigma, (N, Cn)).astype(np.float32))
            tau += [t_] * N; k += [k_] * N; p += [p_] * N; cell += [cid] * N; special += [False] * N
            cid += 1
        reps = 40                                                     # every hand-made row, many uniforms
        logits.append(np.repeat(hand, reps, 0))
        n = len(hand) * reps
        tau += [t_] * n; k += [k_] * n; p += [p_] * n; cell += [cid] * n; special += list(np.repeat(hand_special, reps))
        cid += 1
    logits = np.concatenate(logits)
    tau, k, p = np.array(tau, np.float32), np.array(k, np.int64), np.array(p, np.float32)
    cell, special = np.array(cell), np.array(special)
    u = _grid_uniforms(rng, len(logits))
    got = _filtered(logits, _table(tau, k, p), u)
    st, sk, sp_ = _sanitised(tau, k, p, Cn)                           # (top_k 50 / 40 on 37 classes: out of range = off)
    _check_cells(got, logits, st, sk, sp_, u.astype(np.float64), cell, "sample_filtered C=%d" % Cn)
    # top_k = 1 and top_p = 1e-6 are the argmax (ties to the lower class), with no exceptions; so is every tied / -inf row
    am = np.argmax(np.where(logits == 0, 0.0, logits.astype(np.float64)), 1)
    exact = ((k == 1) & (p == 1)) | ((k == 0) & (p < 1e-5))
    assert exact.sum() >= 2 * 4 * N and np.array_equal(got[exact], am[exact])
    # NULL sampling = all defaults = the (1, 0, 1) rows
    d = np.flatnonzero((tau == 1) & (k == 0) & (p == 1))
    assert np.array_equal(_filtered(logits[d], None, u[d]), got[d])


def test_filtered_draw_survives_hostile_rows():
    rng = np.random.default_rng(5)
    for Cn in (256, 37):
        hostile = [(np.nan, 0, 1.0), (0.0, 0, 1.0), (-2.0, 0, 1.0), (np.inf, 0, 1.0), (1.0, -5, 1.0), (1.0, 10 ** 6, 1.0),
                   (1.0, 0, 0.0), (1.0, 0, 2.0), (1.0, 0, np.nan), (np.nan, -5, np.nan), (1.0, Cn, 1.0), (1e-30, 0, 1.0),
                   (1e30, 3, 0.5), (1e-30, 5, 0.3)]
        N = 200
        logits = rng.normal(0, 2, (len(hostile) * N, Cn)).astype(np.float32)
        tau = np.repeat(np.array([h[0] for h in hostile], np.float32), N)
        k = np.repeat(np.array([h[1] for h in hostile], np.int64), N)
        p = np.repeat(np.array([h[2] for h in hostile], np.float32), N)
        u = _grid_uniforms(rng, len(logits))
        tab = _table(tau, k.astype(np.int32), p)
        tab["reserved"] = 0x7fffffff                                   # not read
        got = _filtered(logits, tab, u)
        assert got.min() >= 0 and got.max() < Cn
        # fields out of range count as their defaults: the first 11 kinds are the plain draw
        plain = _filtered(logits, None, u)
        m = np.arange(len(logits)) < 11 * N
        assert np.array_equal(got[m], plain[m])
        # a temperature of 1e-30 is the argmax
        cold = np.isin(np.arange(len(logits)) // N, [11, 13])
        assert np.array_equal(got[cold], logits[cold].argmax(1))


def test_ops_sample_filtered():
    ops = sub("ops")
    rng = np.random.default_rng(8)
    logits = rng.normal(0, 2, (64, 256)).astype(np.float32)
    u = _grid_uniforms(rng, 64)
    got = ops.sample_filtered(torch.tensor(logits), torch.tensor(u), temperature=0.8, top_k=40, top_p=0.95).cpu().numpy()
    want = _filtered(logits, _table(np.full(64, 0.8, np.float32), np.full(64, 40), np.full(64, 0.95, np.float32)), u)
    assert np.array_equal(got, want)
    assert np.array_equal(ops.sample_filtered(torch.tensor(logits), torch.tensor(u), top_k=1).cpu().numpy(), logits.argmax(1))
    with pytest.raises(ValueError, match="top_k"):
        ops.sample_filtered(torch.tensor(logits), torch.tensor(u), top_k=300)


# ---------------------------------------------------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------------------------------------------------
DIL = [1, 2, 4, 8, 16, 1, 2, 4]


def _softmax_engine(dt, Cn=256, dil=DIL):
    EG = sub("engine")
    sp = O.init_stack_params(4, dil, 2, 64, 256, Cn, bias_scale=0.05)
    cfg = EG.StackConfig(dilations=dil, dilation_channels=64, skip_channels=256, output_channels=Cn, shift_input=True,
                         dtype=dt)
    eng = EG.WaveNetEngine(cfg, 1, 64, DEV)
    eng.load_oracle_params(sp)
    return eng


def _mol_engine(dt, E=6, pool=16, M=10, dil=DIL):
    EG = sub("engine")
    sp = O.init_stack_params(7, dil, 2, 64, 256, 4 * M, cond_channels=E, bias_scale=0.05)
    cfg = EG.StackConfig(dilations=dil, dilation_channels=64, skip_channels=256, output_channels=4 * M, cond_channels=E,
                         pool_stride=pool, shift_input=True, head_mode="mol", dtype=dt)
    eng = EG.WaveNetEngine(cfg, 1, pool, DEV)
    eng.load_oracle_params(sp)
    return eng


def _bits(x):
    return x.contiguous().view(torch.int32).cpu().numpy()


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _mix(B):
    """A per-utterance mix of controls, some rows at the defaults."""
    c = [CONTROLS[u % len(CONTROLS)] for u in range(B)]
    return dict(temperature=[x[0] for x in c], top_k=[x[1] for x in c], top_p=[x[2] for x in c])


# ---------------------------------------------------------------------------------------------------------------------
# 2. defaults are the bits of the calls without controls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 33, 70])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("head", ["softmax", "mol"])
def test_defaults_are_the_plain_bits(monkeypatch, head, dt, B):
    EG = sub("engine")
    L = sub("_lib")
    T = 48
    eng = _softmax_engine(dt) if head == "softmax" else _mol_engine(dt)
    cond = dev(np.random.default_rng(2).standard_normal((B, T // 16, 6))) if head == "mol" else None
    bodies = [{"SRWN_GEN16": "0"}]
    if dt == torch.bfloat16:
        bodies += [{"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "1"}, {"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "2"}]
    for env in bodies:
        for kk, v in env.items():
            monkeypatch.setenv(kk, v)
        kw = dict(mode="sample", seed=13, want_logits=True, batch=B, cond=cond)
        plain = eng.generate(T, **kw)
        assert _same(plain, eng.generate(T, temperature=1.0, top_k=0, top_p=1.0, **kw)), env
        assert _same(plain, eng.generate(T, temperature=[1.0] * B, top_k=[0] * B, top_p=[1.0] * B, **kw)), env
        # and through the kernels that read the array: an all-default DEVICE array into the *_sampled twins
        tab = np.zeros(B, dtype=np.dtype(L.SrwnGenSampling))
        tab["temperature"], tab["top_p"] = 1.0, 1.0
        st = eng.generation_state(B, cond, 13)
        st.sampling = EG._sampling_to_device(tab, DEV)
        assert _same(plain, eng.generate_chunk(st, T, mode="sample", want_logits=True)), env


# ---------------------------------------------------------------------------------------------------------------------
# 3. draw for draw inside the generators
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,env", [(torch.float32, {"SRWN_GEN16": "0"}), (torch.bfloat16, {"SRWN_GEN16": "0"}),
                                    (torch.bfloat16, {"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "1"}),
                                    (torch.bfloat16, {"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "2"})])
@pytest.mark.parametrize("Cn", [256, 100])
def test_generators_draw_by_the_rule(monkeypatch, dt, env, Cn):
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    B, T, seed = 70, 120, 21
    eng = _softmax_engine(dt, Cn)
    mix = _mix(B)
    a, c, lg = eng.generate(T, mode="sample", seed=seed, want_logits=True, batch=B, **mix)
    lg = lg.cpu().numpy()
    codes = c.cpu().numpy().astype(np.int64)
    assert np.isfinite(lg).all()
    tau, k, p = _sanitised(np.repeat(mix["temperature"], T), np.repeat(mix["top_k"], T), np.repeat(mix["top_p"], T), Cn)
    u = np.array([[float(_gen_uniform(seed, b, t)) for t in range(T)] for b in range(B)]).reshape(-1)
    cell = np.repeat(np.arange(B) % len(CONTROLS), T)
    _check_cells(codes.reshape(-1), lg.reshape(B * T, Cn), tau, k, p, u, cell, "generate %s %s C=%d" % (dt, env, Cn))
    # the emitted samples are the mu-law decode of the emitted codes
    assert np.array_equal(a.cpu().numpy().view(np.uint32), O.mu_law_decode(codes.astype(np.int32), Cn).view(np.uint32))
    # rows at the defaults are the rows of the call without controls; top_k = 1 rows are the argmax rows
    plain = eng.generate(T, mode="sample", seed=seed, want_logits=True, batch=B)
    amax = eng.generate(T, mode="argmax", seed=seed, want_logits=True, batch=B)
    d = [b for b in range(B) if CONTROLS[b % len(CONTROLS)] == (1.0, 0, 1.0)]
    g = [b for b in range(B) if CONTROLS[b % len(CONTROLS)][1] == 1 or CONTROLS[b % len(CONTROLS)][2] < 1e-5]
    assert len(d) >= 7 and len(g) >= 14
    for i in range(3):
        assert np.array_equal(_bits(a if i == 0 else c if i == 1 else torch.tensor(lg))[d],
                              _bits(plain[i])[d])
        assert np.array_equal(_bits(a if i == 0 else c if i == 1 else torch.tensor(lg))[g], _bits(amax[i])[g])
    # mode 0 ignores the controls
    assert _same(amax, eng.generate(T, mode="argmax", seed=seed, want_logits=True, batch=B, **mix))


def _mol_restated(l, u1, u2, tau):
    """The mixture head with a temperature (srwn.h), fp64: l [..., 4M], u1 [..., M], u2 [...], tau [...]."""
    M = l.shape[-1] // 4
    sel = np.argmax(l[..., :M] / tau[..., None] - np.log(-np.log(u1)), axis=-1)
    mean = np.take_along_axis(l[..., M:2 * M], sel[..., None], -1)[..., 0]
    ls = np.maximum(np.take_along_axis(l[..., 2 * M:3 * M], sel[..., None], -1)[..., 0], -7.0)
    x = mean + tau * np.exp(ls) * (np.log(u2) - np.log(1.0 - u2))
    return np.minimum(np.maximum(x, -1.0), 1.0), sel, mean


@pytest.mark.parametrize("dt,env", [(torch.float32, {"SRWN_GEN16": "0"}), (torch.bfloat16, {"SRWN_GEN16": "0"}),
                                    (torch.bfloat16, {"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "1"}),
                                    (torch.bfloat16, {"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "2"})])
def test_mol_temperature_draw_for_draw(monkeypatch, dt, env):
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    B, T, M, seed = 35, 96, 10, 11
    eng = _mol_engine(dt, M=M)
    cond = dev(np.random.default_rng(3).standard_normal((B, T // 16, 6)))
    taus = np.array([[1.0, 0.5, 0.7, 1.3, 2.0][b % 5] for b in range(B)])
    a, sel, lg = eng.generate(T, mode="sample", seed=seed, want_logits=True, batch=B, cond=cond, temperature=list(taus))
    lg, a, sel = lg.cpu().numpy().astype(np.float64), a.cpu().numpy(), sel.cpu().numpy()
    assert np.isfinite(a).all() and np.abs(a).max() <= 1.0 and sel.min() >= 0 and sel.max() < M
    u1 = np.array([[[1e-5 + (1 - 2e-5) * float(_gen_uniform(seed, b, t * (M + 1) + m)) for m in range(M)]
                    for t in range(T)] for b in range(B)])
    u2 = np.array([[1e-5 + (1 - 2e-5) * float(_gen_uniform(seed, b, t * (M + 1) + M)) for t in range(T)] for b in range(B)])
    want, wsel, _ = _mol_restated(lg, u1, u2, np.broadcast_to(taus[:, None], (B, T)))
    close = np.abs(a - want) < 1e-3
    print("MEASURED mol temperature %s %s: %.5f of %d draws within 1e-3" % (dt, env, close.mean(), close.size))
    assert close.mean() >= 0.995
    # where log_scale > -7 the oracle's sampler says the same, fed with logit / tau and log_scale + log tau
    l2 = lg.copy()
    l2[..., :M] /= taus[:, None, None]
    l2[..., 2 * M:3 * M] += np.log(taus)[:, None, None]
    ok = (lg[..., 2 * M:3 * M] > -7.0).all(-1) & (l2[..., 2 * M:3 * M] > -7.0).all(-1)
    if ok.any():
        assert (np.abs(a - O.mol_sample(l2, u1, u2))[ok] < 1e-3).mean() >= 0.995
    # rows at temperature 1 are the rows of the call without controls; mode "mean" ignores the temperature
    plain = eng.generate(T, mode="sample", seed=seed, want_logits=True, batch=B, cond=cond)
    d = np.flatnonzero(taus == 1.0)
    assert np.array_equal(a[d].view(np.uint32), plain[0].cpu().numpy()[d].view(np.uint32))
    assert _same(eng.generate(T, mode="mean", seed=seed, batch=B, cond=cond),
                 eng.generate(T, mode="mean", seed=seed, batch=B, cond=cond, temperature=0.5))
    # the spread shrinks with the temperature: same seeds, same (teacher-forced) logits
    forced = dev(O.synthetic_audio(B, T, seed=9) * 0.3)
    spread = {}
    for t_ in (0.5, 1.0):
        fa, fsel, flg = eng.generate(T, mode="sample", seed=seed, forced=forced, want_logits=True, batch=B, cond=cond,
                                     temperature=t_)
        mean = np.take_along_axis(flg.cpu().numpy()[..., M:2 * M], fsel.cpu().numpy()[..., None].astype(np.int64), -1)[..., 0]
        spread[t_] = float(np.std(fa.cpu().numpy() - mean))
    print("MEASURED mol spread: tau 0.5 %.5f, tau 1 %.5f" % (spread[0.5], spread[1.0]))
    assert spread[0.5] < spread[1.0]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the invariances of generation hold with controls on
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 35])
@pytest.mark.parametrize("dt,body", [(torch.float32, "0"), (torch.bfloat16, "0"), (torch.bfloat16, "1")])
@pytest.mark.parametrize("head", ["softmax", "mol"])
def test_chunks_and_prompts_with_controls(monkeypatch, head, dt, body, B):
    monkeypatch.setenv("SRWN_GEN16", body)
    T = 1 + 16 + 160 + 3
    if head == "softmax":
        eng, cond, ctl = _softmax_engine(dt), None, _mix(B)
        if B == 1:
            ctl = dict(temperature=0.8, top_k=40, top_p=0.95)
    else:
        eng = _mol_engine(dt)
        cond = dev(np.random.default_rng(2).standard_normal((B, -(-T // 16), 6)))
        ctl = dict(temperature=[[0.6, 1.0, 1.4][b % 3] for b in range(B)])
    one = eng.generate(T, mode="sample", seed=13, want_logits=True, batch=B, cond=cond, **ctl)
    plain = eng.generate(T, mode="sample", seed=13, want_logits=True, batch=B, cond=cond)
    assert not np.array_equal(_bits(one[0]), _bits(plain[0]))          # the controls do something
    st = eng.generation_state(B, cond, 13, **ctl)
    out = [eng.generate_chunk(st, n, mode="sample", want_logits=True) for n in (1, 16, 160, 3)]
    got = [torch.cat([o[i] for o in out], dim=1) for i in range(3)]
    assert _same(got, one)
    # prime, then chunk: a prompted run in chunks of 1, 16 and the rest is the prompted run in one chunk
    P = 37
    prompt = dev(O.synthetic_audio(B, P, seed=6) * 0.5)
    s1 = eng.generation_state(B, cond, 5, **ctl); eng.prime(s1, prompt)
    whole = eng.generate_chunk(s1, 60, mode="sample", want_logits=True)
    s2 = eng.generation_state(B, cond, 5, **ctl); eng.prime(s2, prompt)
    parts = [eng.generate_chunk(s2, n, mode="sample", want_logits=True) for n in (1, 16, 43)]
    assert _same([torch.cat([o[i] for o in parts], dim=1) for i in range(3)], whole)
    s3 = eng.generation_state(B, cond, 5); eng.prime(s3, prompt)
    assert not np.array_equal(_bits(eng.generate_chunk(s3, 60, mode="sample")[0]), _bits(whole[0]))
    if head == "softmax":      # the primed run draws by the rule too (counters start at the prompt's length)
        mixl = ctl if B > 1 else dict(temperature=[0.8], top_k=[40], top_p=[0.95])
        tau, k, p = _sanitised(np.repeat(mixl["temperature"], 60), np.repeat(mixl["top_k"], 60),
                               np.repeat(mixl["top_p"], 60), 256)
        u = np.array([[float(_gen_uniform(5, b, P + t)) for t in range(60)] for b in range(B)]).reshape(-1)
        _check_cells(whole[1].cpu().numpy().astype(np.int64).reshape(-1), whole[2].cpu().numpy().reshape(B * 60, 256),
                     tau, k, p, u, np.zeros(B * 60, int), "primed %s body %s B=%d" % (dt, body, B))


@pytest.mark.parametrize("head", ["softmax", "mol"])
def test_latency_bodies_agree_with_controls(monkeypatch, head):
    """The two workgroup sizes of the latency body are bit-equal with controls on; against the throughput body the codes
    agree on > 0.9 of the steps (teacher-forced, the bound of tests/test_gpu_generate.py)."""
    B, T = 37, 128
    if head == "softmax":
        eng, cond, ctl = _softmax_engine(torch.bfloat16), None, _mix(B)
    else:
        eng = _mol_engine(torch.bfloat16)
        cond = dev(np.random.default_rng(2).standard_normal((B, T // 16, 6)))
        ctl = dict(temperature=[[0.6, 1.0, 1.4][b % 3] for b in range(B)])
    forced = dev(O.synthetic_audio(B, T, seed=21))
    out = {}
    for name, env in (("thr", {"SRWN_GEN16": "0"}), ("lat1", {"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "1"}),
                      ("lat2", {"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "2"})):
        for kk, v in env.items():
            monkeypatch.setenv(kk, v)
        out[name] = (eng.generate(T, mode="sample", seed=3, forced=forced, want_logits=True, batch=B, cond=cond, **ctl),
                     eng.generate(T, mode="sample", seed=3, want_logits=True, batch=B, cond=cond, **ctl))
    assert _same(out["lat1"][0], out["lat2"][0]) and _same(out["lat1"][1], out["lat2"][1])
    agree = (out["lat1"][0][1] == out["thr"][0][1]).float().mean()
    print("MEASURED latency vs throughput body with controls (%s): codes agree on %.4f" % (head, float(agree)))
    assert agree > 0.9


@pytest.mark.parametrize("dt,body", [(torch.float32, "0"), (torch.bfloat16, "0"), (torch.bfloat16, "1")])
@pytest.mark.parametrize("head", ["softmax", "mol"])
def test_pool_slots_with_controls_equal_batch_of_one(monkeypatch, head, dt, body):
    """A slot with controls gives the bits of a batch-of-one run with its seed, prompt and controls -- whichever slot it
    sits in, whatever its neighbours' controls, across a neighbour's leave and the re-join of another with other
    controls, and in a pool where some slots have no controls at all."""
    monkeypatch.setenv("SRWN_GEN16", body)
    rng = np.random.default_rng(4)
    frames = 12
    if head == "softmax":
        eng = _softmax_engine(dt)
        ctls = [dict(temperature=0.7, top_k=0, top_p=1.0), dict(temperature=1.0, top_k=50, top_p=1.0), None,
                dict(temperature=1.0, top_k=0, top_p=0.9), dict(temperature=0.8, top_k=40, top_p=0.95),
                dict(temperature=1.0, top_k=1, top_p=1.0)]
        pool = eng.generation_pool(40)
        encs = [None] * 6
    else:
        eng = _mol_engine(dt)
        ctls = [dict(temperature=0.6), None, dict(temperature=1.4), dict(temperature=0.9), dict(temperature=2.0), None]
        pool = eng.generation_pool(40, frames=frames)
        encs = [rng.standard_normal((frames, 6)).astype(np.float32) for _ in range(6)]
    prompts = [None, (rng.standard_normal(21) * 0.3).astype(np.float32), None,
               (rng.standard_normal(5) * 0.3).astype(np.float32), None, None]
    seeds = [11, 12, 13, 14, 15, 16]
    total = 96

    def solo(i, n):
        cond = None if encs[i] is None else dev(encs[i][None])
        st = eng.generation_state(1, cond, seeds[i], **(ctls[i] or {}))
        if prompts[i] is not None:
            eng.prime(st, dev(prompts[i][None]))
        return eng.generate_chunk(st, n, mode="sample", want_logits=True)

    def join(i, slot):
        kw = {} if ctls[i] is None else {kk: [v] for kk, v in ctls[i].items()}
        pool.join([seeds[i]], prompts=[prompts[i]], cond=None if encs[i] is None else [encs[i]], slots=[slot], **kw)

    where = {0: 0, 1: 1, 2: 33, 3: 34, 4: 39}                            # streams 0..4 over both ring groups
    got = {i: [] for i in range(6)}
    join(2, where[2])                                                    # a stream without controls first: no array yet
    a, c, lg, ran = pool.step(8, want_logits=True)
    got[2].append((a[33:34, :8], c[33:34, :8], lg[33:34, :8]))
    for i in (0, 1, 3, 4):
        join(i, where[i])
    a, c, lg, ran = pool.step(40, want_logits=True)
    for i, s in where.items():
        got[i].append((a[s:s + 1], c[s:s + 1], lg[s:s + 1]))
    pool.leave([where[1]])                                               # a neighbour leaves; another joins its slot
    where2 = dict(where); del where2[1]; where2[5] = where[1]
    join(5, where[1])
    a, c, lg, ran = pool.step(48, want_logits=True)
    for i, s in where2.items():
        got[i].append((a[s:s + 1], c[s:s + 1], lg[s:s + 1]))
    lens = {0: 88, 1: 40, 2: 96, 3: 88, 4: 88, 5: 48}
    for i in range(6):
        cat = [torch.cat([o[j] for o in got[i]], dim=1) for j in range(3)]
        assert cat[0].shape[1] == lens[i]
        assert _same(cat, solo(i, lens[i])), (head, dt, body, "stream", i)
    assert total == lens[2]


# ---------------------------------------------------------------------------------------------------------------------
# 5. model level
# ---------------------------------------------------------------------------------------------------------------------
def test_model_level_controls():
    M = sub("model")
    dil = [1, 2, 4, 8, 16, 32]
    m = M.WaveNetTeacher(512, 0, dil, dilation_channels=64, skip_channels=256, quantization_channels=256,
                         learning_rate=1e-2)
    x = O.synthetic_audio(4, 512, seed=3)
    for _ in range(3):
        m.train(x)
    am = m.generate(3, 200, mode="argmax", seed=7)
    assert np.array_equal(m.generate(3, 200, mode="sample", seed=7, top_k=1).view(np.uint32), am.view(np.uint32))
    one = m.generate(3, 200, mode="sample", seed=7, temperature=0.7, top_p=0.9)
    blocks = list(m.stream(3, 64, mode="sample", seed=7, temperature=0.7, top_p=0.9, max_samples=200))
    assert np.array_equal(np.concatenate(blocks, 1).view(np.uint32), one.view(np.uint32))
    assert not np.array_equal(one, m.generate(3, 200, mode="sample", seed=7))
    pool = m.generation_pool(4)
    s = pool.join(seed=[7], temperature=0.7, top_p=0.9)
    out = pool.step(200)
    solo = m.generate(1, 200, mode="sample", seed=7, temperature=0.7, top_p=0.9)
    assert np.array_equal(out[s[0]].view(np.uint32), solo[0].view(np.uint32))
    B, T, pool_stride, lat = 2, 256, 32, 8
    ae = M.WaveNetAutoEncoder(input_size=T, condition_size=0, num_mixtures=5, dilations=[1, 2, 4, 8, 16],
                              dilation_channels=64, skip_channels=256, latent_channels=lat, pool_stride=pool_stride,
                              dtype=torch.float32)
    xa = O.synthetic_audio(B, T, seed=2)
    for _ in range(3):
        ae.train(xa)
    enc = ae.encode(xa)
    g = ae.generate(enc, seed=5, temperature=0.6)
    assert g.shape == (B, T) and np.isfinite(g).all() and np.abs(g).max() <= 1.0
    assert not np.array_equal(g, ae.generate(enc, seed=5))
    assert np.array_equal(np.concatenate(list(ae.stream(enc, chunk_size=100, seed=5, temperature=0.6)), 1).view(np.uint32),
                          g.view(np.uint32))
