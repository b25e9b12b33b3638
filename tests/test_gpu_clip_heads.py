"""GPU tests of the two clip-level heads -- the pooled classifier (class WaveNet, head_mode "pooled") and the Siamese
contrastive head (class SiameseWaveNet, head_mode "contrastive") -- at the shapes their drivers run.

  kernels   srwn_time_mean (slab split, ragged and one-row last slabs, 250 slabs), srwn_pooled_head (any B: rows go
            through LDS in chunks; soft, one-hot, unnormalised and absent labels; logits near 80; padding columns) and
            srwn_bcast_mask (+0, -0 and negative activations; ragged grids) against float64 numpy, every output filled
            with NaN beforehand and followed by a guard region that must come back untouched
  engines   the pooled classifier at the reference train.py's shape (2 x [1..512], R 32 / S 128, 16 384 samples) and a
            ragged length, once with the canonical gate; the contrastive head at examples/siamese.py's shape
            (3 x [1..512], D 2, 5 120 samples) -- both dtypes against the fp64 TorchStack oracle
  limits    B = 64 clips of a 256-way classifier trains and matches the oracle; the contrastive head's LDS limit is
            refused when the engine is built
"""
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from oracle import wavenet_torch as OT
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev, rel_err
from tests.test_siamese import contrastive_loss

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
GUARD = 67                 # floats after every output that must come back untouched
SENTINEL = 12288.0           # exact in bf16 too
PH_LDS_FLOATS = 65536 // 4   # srwn_pooled_head's LDS budget: chunk * C + 256 floats


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(n, fill=np.nan, dt=torch.float32):
    """n output elements filled with `fill`, then GUARD sentinel elements."""
    t = torch.full((n + GUARD,), SENTINEL, dtype=dt, device=DEV)
    t[:n] = fill
    return t


def _body(t, n):
    assert bool((t[n:].float() == SENTINEL).all()), "write past the end of the output"
    return t[:n].float().cpu().numpy()


def _bf16_round(a):
    return torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


# --- srwn_time_mean -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,T,C", [(1, 1, 32), (3, 255, 128), (2, 256, 128), (2, 257, 256), (1, 16384, 128),
                                   (2, 64000, 32)])
def test_time_mean_kernel(B, T, C, dtype):
    """One row; a slab boundary on either side; a one-row last slab; 64 and 250 slabs.  The bf16 reference is the mean
    of the bf16-rounded values."""
    L = sub("_lib")
    rng = np.random.default_rng(B * 7 + T + C)
    x = rng.normal(0.5, 1.0, (B, T, C)).astype(np.float32)
    if dtype == BF16:
        x = _bf16_round(x)
    ref = x.astype(np.float64).mean(axis=1)
    gx = dev(x, torch.float32 if dtype == F32 else torch.bfloat16)
    ns = int(L.load().srwn_time_mean_slabs(T))
    assert ns == -(-T // 256)
    parts = _out(B * ns * C)
    out = _out(B * C)
    L.call("srwn_time_mean", gx.data_ptr(), parts.data_ptr(), out.data_ptr(), B, T, C, dtype, _stream())
    torch.cuda.synchronize()
    _body(parts, B * ns * C)
    got = _body(out, B * C).reshape(B, C)
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err < 2e-6, (B, T, C, err)


# --- srwn_pooled_head -----------------------------------------------------------------------------------------------
def _np_pooled_head(mean, w2, b2, labels, C):
    """float64: probs, loss, gw2 [S,C], gb2 [C], dmean [B,S], and the size of what each of loss, gw2, gb2 and dmean
    sums (the same sums over absolute values): the fp32 kernel is judged against those, so that a gradient that cancels
    to ~0 (a one-hot label on a dominant class) is not held to relative precision it cannot have."""
    mean = mean.astype(np.float64)
    w = w2[:, :C].astype(np.float64)
    lg = mean @ w + b2[:C].astype(np.float64)
    m = lg.max(-1, keepdims=True)
    lse = m + np.log(np.exp(lg - m).sum(-1, keepdims=True))
    probs = np.exp(lg - lse)
    if labels is None:
        return probs, None, None, None, None, None
    y = labels.astype(np.float64)
    B = mean.shape[0]
    loss = float(np.mean(-(y * (lg - lse)).sum(-1)))
    sl = y.sum(-1, keepdims=True)
    dl = (probs * sl - y) / B                             # d loss / d logits: rows need not sum to 1
    adl = (probs * sl + y) / B
    size = {"loss": float(np.mean((y * (np.abs(lg) + np.abs(lse))).sum(-1))), "gw2": (mean.T @ adl).max(),
            "gb2": adl.sum(0).max(), "dmean": (adl @ np.abs(w).T).max()}
    return probs, loss, mean.T @ dl, dl.sum(0), dl @ w.T, size


def _labels(kind, rng, B, C):
    if kind == "none":
        return None
    if kind == "onehot":
        y = np.zeros((B, C), np.float32)
        y[np.arange(B), rng.integers(0, C, B)] = 1.0
        return y
    y = rng.random((B, C)).astype(np.float32) + 0.01
    if kind == "soft":
        return (y / y.sum(-1, keepdims=True)).astype(np.float32)
    return (y * rng.uniform(0.3, 3.0, (B, 1))).astype(np.float32)      # "unnorm": rows that do not sum to 1


def _pooled_head_case(L, rng, B, S, C, ldw, kind):
    mean = rng.random((B, S)).astype(np.float32)             # time-means of relu outputs: >= 0
    mean[0] *= 10.0                                          # one row with a spread of ~30 between its logits
    w2 = np.full((S, ldw), 7.0, np.float32)                  # padding columns: never read
    w2[:, :C] = rng.normal(0, 3.0 / np.sqrt(S / 3.0), (S, C))
    b2 = np.full(ldw, 7.0, np.float32)
    b2[:C] = 80.0 + rng.normal(0, 1.0, C)                    # logits near 80: exp overflows fp32 unless max is subtracted
    labels = _labels(kind, rng, B, C)
    probs, loss, gw2, gb2, dmean = _out(B * C), _out(1), _out(S * ldw), _out(ldw), _out(B * S)
    if labels is None:                                       # no labels: the gradient buffers stay untouched
        for t in (gw2, gb2, dmean):
            t.fill_(3.0)
    g_mean, g_w2, g_b2 = dev(mean), dev(w2), dev(b2)      # (held: a temporary's memory is reused before the launch)
    g_lab = None if labels is None else dev(labels)
    L.call("srwn_pooled_head", g_mean.data_ptr(), g_w2.data_ptr(), g_b2.data_ptr(),
           None if g_lab is None else g_lab.data_ptr(), probs.data_ptr(), loss.data_ptr(), gw2.data_ptr(),
           gb2.data_ptr(), dmean.data_ptr(), B, S, C, ldw, _stream())
    torch.cuda.synchronize()
    r_probs, r_loss, r_gw2, r_gb2, r_dmean, size = _np_pooled_head(mean, w2, b2, labels, C)
    tag = (B, S, C, ldw, kind)
    p = _body(probs, B * C).reshape(B, C)
    assert rel_err(p, r_probs) < 1e-4, tag
    assert np.abs(p.sum(-1) - 1).max() < 1e-4, tag
    if labels is None:
        assert float(_body(loss, 1)[0]) == 0.0, tag
        for t in (gw2, gb2, dmean):
            assert bool((t == 3.0).all()), tag
        return
    lv = float(_body(loss, 1)[0])
    assert abs(lv - r_loss) <= 1e-6 * size["loss"], (tag, lv, r_loss)
    gw = _body(gw2, S * ldw).reshape(S, ldw)
    gb = _body(gb2, ldw)
    assert not gw[:, C:].any() and not gb[C:].any(), ("padding columns of gw2 / gb2 must be written as 0", tag)
    for name, got, ref in (("gw2", gw[:, :C], r_gw2), ("gb2", gb[:C], r_gb2),
                           ("dmean", _body(dmean, B * S).reshape(B, S), r_dmean)):
        assert np.isfinite(got).all(), (name, tag)
        if C == 1:                          # one class: softmax is exactly 1, every gradient exactly 0
            assert not got.any(), (name, tag)
        err = np.abs(got - ref).max() / size[name]
        assert err < 1e-4, (name, tag, err)


@pytest.mark.parametrize("S", [32, 128, 256])
@pytest.mark.parametrize("C", [1, 2, 30, 255, 256])
def test_pooled_head_kernel(C, S):
    """B in {1, 3, 17} and around the rows one LDS chunk holds (the largest B the old one-chunk kernel allowed, one
    more, and three chunks); ldw = the engine's padded width."""
    L = sub("_lib")
    ldw = (C + 31) // 32 * 32
    bmax = (PH_LDS_FLOATS - 256) // C
    Bs = [1, 3, 17, bmax, bmax + 1] + ([2 * bmax + 5] if C >= 30 else [])
    rng = np.random.default_rng(1000 * C + S)
    for B in Bs:
        for kind in ("soft", "onehot", "unnorm", "none"):
            _pooled_head_case(L, rng, B, S, C, ldw, kind)


def test_pooled_head_chunks_give_the_same_bits():
    """Rows that fit one chunk and the same rows inside a batch that needs three: identical probs and dmean rows, and
    the gradient sums that continue across chunks equal a float64 sum to fp32 round-off."""
    L = sub("_lib")
    S, C, ldw = 128, 256, 256
    bmax = (PH_LDS_FLOATS - 256) // C
    rng = np.random.default_rng(4)
    B = 2 * bmax + 5
    mean = rng.random((B, S)).astype(np.float32)
    w2 = rng.normal(0, 0.2, (S, ldw)).astype(np.float32)
    b2 = rng.normal(0, 0.1, ldw).astype(np.float32)
    y = _labels("soft", rng, B, C)
    res = {}
    for n in (B, 5):
        probs, loss, gw2, gb2, dmean = _out(n * C), _out(1), _out(S * ldw), _out(ldw), _out(n * S)
        ins = [dev(mean[:n]), dev(w2), dev(b2), dev(y[:n])]
        L.call("srwn_pooled_head", *[t.data_ptr() for t in ins], probs.data_ptr(), loss.data_ptr(), gw2.data_ptr(),
               gb2.data_ptr(), dmean.data_ptr(), n, S, C, ldw, _stream())
        torch.cuda.synchronize()
        res[n] = (_body(probs, n * C).reshape(n, C), _body(dmean, n * S).reshape(n, S) * n)   # dl carries 1/B
    assert np.array_equal(res[B][0][:5], res[5][0])
    assert rel_err(res[B][1][:5], res[5][1]) < 1e-6


# --- srwn_bcast_mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("S", [4, 36, 128, 256])
def test_bcast_mask_kernel(S, dtype):
    """da1 = (r1 > 0) ? dmean * scale : 0, strict like TF's relu gradient: +0 and -0 are masked.  B*T*S/4 threads are
    not a multiple of the 256-thread block."""
    L = sub("_lib")
    B, T = 3, 333
    assert (B * T * S // 4) % 256
    rng = np.random.default_rng(S + dtype)
    r1 = rng.normal(0, 1, (B, T, S)).astype(np.float32)
    flat = r1.reshape(-1)
    idx = rng.permutation(flat.size)
    flat[idx[:flat.size // 8]] = 0.0
    flat[idx[flat.size // 8:flat.size // 4]] = -0.0
    flat[idx[:4]] = 0.0
    flat[idx[4:8]] = -0.0
    assert (np.signbit(r1) & (r1 == 0)).any() and (~np.signbit(r1) & (r1 == 0)).any()
    dmean = rng.normal(0, 1, (B, S)).astype(np.float32)
    scale = np.float32(1.0 / T)
    tdt = torch.float32 if dtype == F32 else torch.bfloat16
    g_r1 = dev(r1, tdt)
    assert bool(((g_r1 == 0) & torch.signbit(g_r1)).any())           # -0 survives the bf16 conversion
    out = _out(B * T * S, dt=tdt)
    g_dmean = dev(dmean)
    L.call("srwn_bcast_mask", g_dmean.data_ptr(), g_r1.data_ptr(), out.data_ptr(), B, T, S, float(scale), dtype,
           _stream())
    torch.cuda.synchronize()
    assert bool((out[B * T * S:].float() == SENTINEL).all()), "write past the end of the output"
    prod = (dmean * scale)[:, None, :]                               # the one fp32 rounding of dmean * scale
    ref = torch.tensor(np.where(g_r1.float().cpu().numpy() > 0, prod, np.float32(0.0)).astype(np.float32))
    ref = ref.reshape(-1).to(tdt)                                    # ... and, in bf16, the one rounding to bf16
    got = out[:B * T * S].cpu()
    assert torch.equal(got.view(torch.int16 if dtype else torch.int32), ref.view(torch.int16 if dtype else torch.int32))


# --- the engines at their drivers' shapes ---------------------------------------------------------------------------
# bf16 bounds: 2x the errors measured on one MI355X (probs or embedding max-relative, loss relative, worst per-tensor
# relative L2 gradient error; SRWN_PRINT_ERR=1 pytest -s prints them).  Measured:
#   pooled T=16384 C=10   2.53e-4 / 4.74e-6 / 1.66e-2 (init_w)
#   pooled T=16384 C=256  4.37e-4 / 3.34e-7 / 8.94e-3 (init_w)
#   pooled T=5000 C=10    2.58e-4 / 4.35e-6 / 1.49e-2 (init_w)
#   contrastive P=1       1.73e-3 / 4.13e-2 / 5.86e-2 (head_b1), distance 2.09e-2
#   contrastive P=4       1.99e-3 / 8.33e-3 / 3.88e-2 (l7.br), distance 5.06e-3
BF16_POOLED = {
    (16384, 10): (5.1e-4, 9.5e-6, 3.4e-2),
    (16384, 256): (8.8e-4, 6.7e-7, 1.8e-2),
    (5000, 10): (5.2e-4, 8.7e-6, 3.0e-2),
}
BF16_CONTRASTIVE = {1: (3.5e-3, 8.3e-2, 1.2e-1), 4: (4.0e-3, 1.7e-2, 7.8e-2)}
BF16_DIST = {1: 4.2e-2, 4: 1.02e-2}        # the pair distance, max-relative

DIL_TRAIN = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 2     # reference train.py (classifier)
DIL_SIAMESE = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3   # examples/siamese.py
R, S = 32, 128

_ORACLE = {}


def _grads_of(st, gate_mode):
    # (the top layer's residual 1x1 feeds nothing, model.py:45-50: autograd leaves it None -- the engine must give 0)
    g = {n: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy() for n, t in st.named(include_cond=False)}
    if gate_mode == "wavenet":
        for i, l in enumerate(st.layers):
            g[f"l{i}.wg"] = l["wg"].grad.numpy()
            g[f"l{i}.bg"] = l["bg"].grad.numpy()
    return g


def _pooled_setup(T, C, B=2, gate_mode="reference", dil=DIL_TRAIN, seed=21):
    """Parameters, audio, soft labels and the fp64 oracle (cached for both dtypes): probs, loss, every gradient."""
    key = ("pooled", T, C, B, gate_mode, len(dil), seed)
    if key not in _ORACLE:
        sp = O.init_stack_params(seed, dil, 2, R, S, C, bias_scale=0.05)
        audio = O.synthetic_audio(B, T, seed=seed).astype(np.float64)
        rng = np.random.default_rng(seed)
        y = rng.random((B, C)); y /= y.sum(-1, keepdims=True)
        st = OT.TorchStack(sp)
        logits = st.forward(torch.tensor(audio), gate_mode=gate_mode)       # no RightShift (model.py:162)
        loss = OT.loss_pooled(logits, torch.tensor(y))
        loss.backward()
        probs = torch.softmax(logits.detach().mean(dim=1), dim=-1).numpy()
        _ORACLE[key] = (sp, audio, y, probs, float(loss.detach()), _grads_of(st, gate_mode))
    return _ORACLE[key]


def _contrastive_setup(P, T=5120, D=2, dil=DIL_SIAMESE, seed=23):
    """Labels 1, 0, 0.25 and pairs on both sides of the margin (the median distance), as in test_gpu_siamese."""
    key = ("contrastive", P, T, D, len(dil), seed)
    if key not in _ORACLE:
        sp = O.init_stack_params(seed, dil, 2, R, S, D, bias_scale=0.05)
        audio = O.synthetic_audio(2 * P, T, seed=seed).astype(np.float64)     # left clips, then right ones
        labels = np.resize(np.array([1.0, 0.0, 0.0, 0.25], np.float32), P)
        st = OT.TorchStack(sp)
        emb = st.forward(torch.tensor(audio)).mean(dim=1)                     # no RightShift (model.py:692)
        d = torch.sqrt(1e-8 + ((emb[:P] - emb[P:]) ** 2).sum(-1)).detach().numpy()
        margin = float(np.median(d)) if P > 1 else 2.0 * float(d[0])
        loss, d = contrastive_loss(emb, torch.tensor(labels, dtype=torch.float64), margin)
        loss.backward()
        _ORACLE[key] = (sp, audio, labels, margin, emb.detach().numpy(), d.detach().numpy(), float(loss.detach()),
                        _grads_of(st, "reference"))
    return _ORACLE[key]


def _judge(tag, eng, out_err, loss_err, ref_grads, dt, bounds, zero=()):
    """fp32: the worst element of every gradient < 1e-3 of the tensor's max; bf16: every tensor in relative L2 under
    bounds[2].  Tensors the oracle leaves at zero (and the names in `zero`) must be exactly zero."""
    got = eng.named_tensors(eng.grads)
    errs = {}
    for n, ref in ref_grads.items():
        g = got[n].float().cpu().numpy()
        assert np.isfinite(g).all(), (tag, n)
        scale = np.abs(ref).max()
        if scale < 1e-12 or n in zero:
            assert scale < 1e-12, (tag, n, scale)
            assert not g.any(), (tag, n, "must be exactly zero")
            continue
        errs[n] = (np.abs(g - ref).max() / scale if dt == torch.float32 else
                   float(np.linalg.norm(g - ref) / np.linalg.norm(ref)))
    worst = max((v, k) for k, v in errs.items())
    if os.environ.get("SRWN_PRINT_ERR"):
        print("MEASURED %s %s: out %.3e loss %.3e worst grad %.3e (%s)" % (tag, dt, out_err, loss_err, worst[0], worst[1]))
    tol = (1e-3, 1e-3, 1e-3) if dt == torch.float32 else bounds
    assert out_err < tol[0], (tag, out_err)
    assert loss_err < tol[1], (tag, loss_err)
    assert worst[0] < tol[2], (tag, worst)


def _pooled_engine(sp, B, T, C, dt, gate_mode="reference", dil=DIL_TRAIN, lr=1e-3):
    EG = sub("engine")
    cfg = EG.StackConfig(dilations=list(dil), dilation_channels=R, skip_channels=S, output_channels=C, dtype=dt,
                         head_mode="pooled", gate_mode=gate_mode, learning_rate=lr)
    eng = EG.WaveNetEngine(cfg, B, T, DEV)
    eng.load_oracle_params(sp)
    return eng


def _run_pooled(T, C, dt, gate_mode="reference"):
    sp, audio, y, r_probs, r_loss, r_grads = _pooled_setup(T, C, gate_mode=gate_mode)
    eng = _pooled_engine(sp, 2, T, C, dt, gate_mode)
    eng.set_inputs(dev(audio), dev(y))
    eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    L = len(DIL_TRAIN)
    _judge("pooled T=%d C=%d %s" % (T, C, gate_mode), eng, rel_err(eng.probs.cpu().numpy(), r_probs),
           abs(float(eng.loss.item()) - r_loss) / r_loss, r_grads, dt, BF16_POOLED.get((T, C)),
           zero=("l%d.wr" % (L - 1), "l%d.br" % (L - 1)))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,C", [(16384, 10), (16384, 256), (5000, 10)])
def test_pooled_classifier_at_train_py_shape(T, C, dt):
    """The reference train.py's classifier: 2 x [1..512], R 32 / S 128, B 2 clips of 16 384 samples (64 time-mean
    slabs), 10 and 256 classes; and 5 000 samples, a multiple of neither the 256-row slab nor the segment width."""
    _run_pooled(T, C, dt)


def test_pooled_classifier_wavenet_gate_at_train_py_shape():
    """The canonical gate under a clip-level head (the only such check), fp32."""
    _run_pooled(16384, 10, torch.float32, gate_mode="wavenet")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("P", [1, 4])
def test_contrastive_at_siamese_py_shape(P, dt):
    """examples/siamese.py: 3 x [1..512], R 32 / S 128, D 2, 2P clips of 5 120 samples; head_b2 exactly 0."""
    sp, audio, labels, margin, r_emb, r_d, r_loss, r_grads = _contrastive_setup(P)
    EG = sub("engine")
    cfg = EG.StackConfig(dilations=DIL_SIAMESE, dilation_channels=R, skip_channels=S, output_channels=2, dtype=dt,
                         head_mode="contrastive", margin=margin)
    eng = EG.WaveNetEngine(cfg, 2 * P, 5120, DEV)
    eng.load_oracle_params(sp)
    eng.set_inputs(dev(audio), dev(labels))
    eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    e_dist = rel_err(eng.dist.cpu().numpy(), r_d)
    if os.environ.get("SRWN_PRINT_ERR"):
        print("MEASURED contrastive P=%d %s: dist %.3e" % (P, dt, e_dist))
    assert e_dist < (1e-3 if dt == torch.float32 else BF16_DIST[P])
    L = len(DIL_SIAMESE)
    _judge("contrastive P=%d" % P, eng, rel_err(eng.emb.cpu().numpy(), r_emb),
           abs(float(eng.loss.item()) - r_loss) / r_loss, r_grads, dt, BF16_CONTRASTIVE[P],
           zero=("head_b2", "l%d.wr" % (L - 1), "l%d.br" % (L - 1)))


# --- the head-size limits -------------------------------------------------------------------------------------------
def test_pooled_classifier_batch_64_of_256_classes_trains():
    """B*C = 16 384 floats of logits: more than one workgroup's LDS holds at once.  The head runs its rows in chunks,
    so the engine builds, matches the oracle and trains."""
    dil = [1, 2, 4, 8, 16, 32]
    B, T, C = 64, 200, 256
    sp, audio, y, r_probs, r_loss, r_grads = _pooled_setup(T, C, B=B, dil=dil, seed=8)
    eng = _pooled_engine(sp, B, T, C, torch.float32, dil=dil)
    eng.set_inputs(dev(audio), dev(y))
    eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    _judge("pooled B=64 C=256", eng, rel_err(eng.probs.cpu().numpy(), r_probs),
           abs(float(eng.loss.item()) - r_loss) / r_loss, r_grads, torch.float32, None)
    l0 = float(eng.loss.item())
    for _ in range(5):
        eng.train_step()
    assert float(eng.loss.item()) < l0


def test_contrastive_head_lds_limit():
    """rows*D + 2P floats at the 64 KiB limit run and match float64; one past it the call returns SRWN_E_SHAPE and
    writes nothing.  (Labelled: rows*(D+1); embedding only: rows*D.)"""
    from tests.test_gpu_siamese import _np_head
    L = sub("_lib")
    Sx = 32
    rng = np.random.default_rng(9)
    for rows, D, labelled, fits in ((256, 63, True, True), (6, 2730, True, False),
                                    (128, 128, False, True), (113, 145, False, False)):
        assert (rows * D + (rows if labelled else 0) <= PH_LDS_FLOATS) == fits
        ldw = (D + 31) // 32 * 32
        P = rows // 2
        mean = rng.random((rows, Sx)).astype(np.float32)
        w2 = rng.normal(0, 0.3, (Sx, ldw)).astype(np.float32)
        b2 = rng.normal(0, 0.1, ldw).astype(np.float32)
        labels = np.resize(np.array([1.0, 0.0, 0.25], np.float32), P)
        margin = 1.0
        emb, dist, loss = _out(rows * D), _out(P), _out(1)
        gw2, gb2, dmean = _out(Sx * ldw), _out(ldw), _out(rows * Sx)
        ins = [dev(mean), dev(w2), dev(b2), dev(labels)]
        args = (ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
                ins[3].data_ptr() if labelled else None, margin, emb.data_ptr(),
                dist.data_ptr() if labelled else None, loss.data_ptr() if labelled else None,
                gw2.data_ptr() if labelled else None, gb2.data_ptr() if labelled else None,
                dmean.data_ptr() if labelled else None, rows, Sx, D, ldw, _stream())
        if not fits:
            with pytest.raises(RuntimeError, match=r"code -2"):
                L.call("srwn_contrastive_head", *args)
            torch.cuda.synchronize()
            for t in (emb, dist, loss, gw2, gb2, dmean):
                assert bool(torch.isnan(t[:-GUARD]).all()) and bool((t[-GUARD:] == SENTINEL).all())
            continue
        L.call("srwn_contrastive_head", *args)
        torch.cuda.synchronize()
        r_emb, r_d, r_loss, r_gw2, _, r_dmean = _np_head(mean, w2, b2, labels, margin, D)
        assert rel_err(_body(emb, rows * D).reshape(rows, D), r_emb) < 1e-5
        if labelled:
            assert rel_err(_body(dist, P), r_d) < 1e-5
            assert abs(float(_body(loss, 1)[0]) - r_loss) <= 1e-5 * r_loss
            gw = _body(gw2, Sx * ldw).reshape(Sx, ldw)
            assert rel_err(gw[:, :D], r_gw2) < 1e-4 and not gw[:, D:].any()
            assert not _body(gb2, ldw).any()
            assert rel_err(_body(dmean, rows * Sx).reshape(rows, Sx), r_dmean) < 1e-4
        else:
            for t in (dist, loss, gw2, gb2, dmean):
                assert bool(torch.isnan(t[:-GUARD]).all())


def test_contrastive_limit_is_refused_when_built():
    """The engine refuses a contrastive batch the head kernel cannot hold when it is built (naming B, D and the limit),
    and SiameseWaveNet passes that on; the largest batch that fits builds and runs."""
    EG = sub("engine")
    M = sub("model")
    dil = [1, 2, 4]
    cfg = EG.StackConfig(dilations=dil, dilation_channels=R, skip_channels=S, output_channels=63,
                         head_mode="contrastive", dtype=torch.float32)
    with pytest.raises(ValueError, match=r"B=258 .*D=63.*16384"):
        EG.WaveNetEngine(cfg, 258, 128, DEV)
    P, T = 128, 128
    sp = O.init_stack_params(3, dil, 2, R, S, 63, bias_scale=0.05)
    eng = EG.WaveNetEngine(cfg, 2 * P, T, DEV)
    eng.load_oracle_params(sp)
    audio = O.synthetic_audio(2 * P, T, seed=3).astype(np.float64)
    labels = np.resize(np.array([1.0, 0.0, 0.25], np.float32), P)
    eng.set_inputs(dev(audio), dev(labels))
    eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    st = OT.TorchStack(sp)
    emb = st.forward(torch.tensor(audio)).mean(dim=1)
    loss, d = contrastive_loss(emb, torch.tensor(labels, dtype=torch.float64), float(eng.cfg.margin))
    loss.backward()
    _judge("contrastive at the LDS limit", eng, rel_err(eng.emb.cpu().numpy(), emb.detach().numpy()),
           abs(float(eng.loss.item()) - float(loss)) / float(loss), _grads_of(st, "reference"), torch.float32, None,
           zero=("head_b2", "l2.wr", "l2.br"))
    m = M.SiameseWaveNet(T, 63, dil, dilation_channels=R, skip_channels=S, dtype=torch.float32)
    xs = O.synthetic_audio(261, T, seed=4).astype(np.float32)
    with pytest.raises(ValueError, match=r"B=261 .*D=63"):
        m.get_embedding(None, xs)
