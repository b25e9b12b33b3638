"""GPU tests of the streaming classifier (srwn_version() 113; recognizer.StreamClassifier, model.WaveNet.recognizer).

  kernels     srwn_pooled_stream_head alone against fp64 NumPy on random z (all four widths, hops of 32 / 40 / 96 rows, a
              ring that wraps); srwn_residual_group_fwd_stream_z against the existing stream form (x_out, bits) and the
              whole-clip group kernel (z, bits)
  end to end  against the fp64 oracle's sliding AVG pool (oracle.wavenet_np.stack_forward), both dtypes, both head paths
  invariants  chunking, batch rows and graph replay leave every bit where it was
  model       window = input_size = T: the single emission is WaveNet.predict's
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev, rel_err

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
# fp32: the project's bound.  bf16: twice the worst error measured on MI355X against the fp64 oracle (DESIGN 2's
# convention; SRWN_PRINT_ERR=1 pytest -s prints every figure).  Measured, relative to the largest oracle value (the fused
# head and its twin give the same figures):
#   case a: logits 1.72e-3, probabilities 2.91e-4        case b: logits 1.93e-3, probabilities 3.68e-4
TOL_F32 = 1e-3
MEASURED_BF16_LOGITS, MEASURED_BF16_PROBS = 1.93e-3, 3.68e-4
TOL_BF16_LOGITS, TOL_BF16_PROBS = 2 * MEASURED_BF16_LOGITS, 2 * MEASURED_BF16_PROBS
# (margin of the bf16 logit bound to the oracle's smallest step between consecutive emissions: 2.7 x in case a, 1.7 x in
# case b -- not the 3 x that the fp32 bound has on every pair; see _check_oracle)
# fused head against its parity twin: twice the worst relative difference measured on the end-to-end cases, per dtype.
# Measured: 0 in all four (ring rows are sums of the same r1 bits in the same order, and both forms of the two products
# start at the bias and take their k-steps in order), so the bound is 0: the pooled logits agree bit for bit.
MEASURED_TWIN = {F32: 0.0, BF16: 0.0}

CASES = {      # name: dilations, R, S, C, B, T, window, hop, max_hops
    "a": ([1, 2, 4, 8, 16, 32, 64, 1, 2, 4], 32, 128, 12, 3, 416, 128, 32, 4),
    "b": ([1, 2, 4, 8, 16, 32, 64, 128, 256, 512], 64, 256, 12, 2, 1640, 320, 40, 8),
}
_ORACLE = {}


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _oracle(name):
    """(params, audio, pooled logits [B, n_emit, C], probabilities) of a case: computed once, shared, never changed."""
    if name not in _ORACLE:
        dil, R, S, Cc, B, T, window, hop, _ = CASES[name]
        sp = O.init_stack_params(11, dil, 2, R, S, Cc, bias_scale=0.05)
        audio = O.synthetic_audio(B, T, seed=4)
        logits_t, _ = O.stack_forward(sp, audio.astype(np.float64))
        pos = [(j + 1) * hop - window for j in range(window // hop - 1, T // hop)]
        lg = np.stack([logits_t[:, p:p + window].mean(1) for p in pos], 1)      # tf.nn.pool AVG VALID at `pos`
        e = np.exp(lg - lg.max(-1, keepdims=True))
        for a in (audio, lg):
            a.setflags(write=False)
        _ORACLE[name] = (sp, audio, lg, e / e.sum(-1, keepdims=True))
    return _ORACLE[name]


def _classifier(name, dt, monkeypatch=None, fused=True, max_batch=None, max_hops=None):
    R_ = sub("recognizer")
    dil, R, S, Cc, B, T, window, hop, mh = CASES[name]
    if monkeypatch is not None:
        monkeypatch.setenv("SRWN_RECOG_FUSED", "1" if fused else "0")
    w = R_.ClassifierWeights(dil, R, S, Cc, 2, dt)
    w.load_oracle_params(_oracle(name)[0])
    return R_.StreamClassifier(w, max_batch=max_batch or B, hop=hop, window=window, max_hops=max_hops or mh)


# ---- the head kernel alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("hop", [32, 40, 96])
@pytest.mark.parametrize("R,S", [(32, 128), (32, 256), (64, 128), (64, 256)])
def test_head_kernel_against_numpy(R, S, hop, dt):
    R_ = sub("recognizer"); K = sub("kernels"); L_ = sub("_lib")
    L, B, k, ring_rows, j0 = 3, 3, 2, 3, 2           # hops 2 and 3 land in ring rows 2 and 0: the ring wraps
    sp = O.init_stack_params(7, [1, 2, 4], 2, R, S, 12, bias_scale=0.1)
    w = R_.ClassifierWeights([1, 2, 4], R, S, 12, 2, dt)
    w.load_oracle_params(sp)
    rng = np.random.default_rng(hop + R + S)
    mc = k * hop + 8                                 # rows behind the chunk are never read
    z = torch.tensor(rng.uniform(-1, 1, size=(L, B, mc, R)), dtype=dt, device=DEV)
    ring = torch.full((B, ring_rows, S), float("nan"), device=DEV)
    clock = torch.tensor([j0 * hop], dtype=torch.int64, device=DEV)
    L_.call("srwn_pooled_stream_head", z.data_ptr(), B * mc * R, mc, L, w.wptr(w.o_skip), w.bs_sum.data_ptr(),
            w.wptr(w.o_w1), w.view("head_b1").data_ptr(), ring.data_ptr(), ring_rows, clock.data_ptr(), B, k, hop, mc, R, S,
            K.abi_dtype(dt), K._stream())
    torch.cuda.synchronize()
    got = ring.cpu().numpy()
    zz = z.double().cpu().numpy()[:, :, :k * hop]
    c = zz / (1 + np.exp(-zz))
    tot = sum(c[l] @ sp.layers[l].ws for l in range(L)) + sum(l.bs for l in sp.layers)
    r1 = np.maximum(np.maximum(tot, 0) @ sp.head_w1 + sp.head_b1, 0)              # [B, k * hop, S]
    want = r1.reshape(B, k, hop, S).sum(2)
    assert np.isnan(got[:, 1]).all()                                             # the row no hop of the chunk owns
    err = rel_err(got[:, [2, 0]], want)
    _say("head kernel R=%d S=%d hop=%d %s: %.3g" % (R, S, hop, dt, err))
    # (bf16: the images, the gate, r0 and r1 are each rounded to 8 significant bits, 2^-8 apiece at the worst; doubled)
    assert err < (1e-4 if dt == F32 else 3e-2)


# ---- the z stream form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", [32, 64])
@pytest.mark.parametrize("dil", [[1, 2, 4, 8, 16], [32, 64, 128, 256, 512]])
def test_z_stream_form_keeps_the_bits(dil, R, dt):
    R_ = sub("recognizer"); K = sub("kernels"); L_ = sub("_lib")
    B, chunks, S = 2, (40, 160, 40), 128
    T, mc, nl, hist = sum(chunks), max(chunks), len(dil), sum(dil)
    sp = O.init_stack_params(3, dil, 2, R, S, 12, bias_scale=0.1)
    w = R_.ClassifierWeights(dil, R, S, 12, 2, dt)
    w.load_oracle_params(sp)
    x0 = torch.tensor(np.random.default_rng(R).normal(0, 0.5, size=(B, T, R)), dtype=dt, device=DEV)
    conv, res = [w.wptr(o) for o in w.o_conv], [w.wptr(o) for o in w.o_res]
    bf, br = [w.view("BF")[l] for l in range(nl)], [w.view("BR")[l] for l in range(nl)]
    x_whole = torch.zeros((nl, B, T, R), dtype=dt, device=DEV)
    z_whole = torch.zeros((nl, B, T, R), dtype=dt, device=DEV)
    K.residual_group_fwd(x0, x_whole, z_whole, conv, res, bf, br, dil)
    buf = torch.zeros((B, hist + mc, R), dtype=dt, device=DEV)
    clock = torch.zeros(1, dtype=torch.int64, device=DEV)
    dl = (C.c_int32 * nl)(*dil)
    ptrs = lambda ts: K._ptr_array([t.data_ptr() for t in ts])
    t = 0
    for n in chunks:
        buf[:, hist:hist + n] = x0[:, t:t + n]
        out_a = torch.full((B, mc, R), float("nan"), dtype=dt, device=DEV)
        out_b = torch.full((B, mc, R), float("nan"), dtype=dt, device=DEV)
        z = torch.full((nl, B, mc, R), float("nan"), dtype=dt, device=DEV)
        tail = (K._ptr_array(conv), K._ptr_array(res), ptrs(bf), ptrs(br), None, 1, 1, R, dl, nl, B, n, mc, R, 2,
                K.abi_dtype(dt), clock.data_ptr(), K._stream())
        L_.call("srwn_residual_group_fwd_stream", buf.data_ptr(), hist + mc, out_a.data_ptr(), mc, 0, *tail)
        L_.call("srwn_residual_group_fwd_stream_z", buf.data_ptr(), hist + mc, out_b.data_ptr(), mc, 0, z.data_ptr(),
                B * mc * R, *tail)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out_a[:, :n]), _bits(out_b[:, :n]))
        assert torch.equal(_bits(out_b[:, :n]), _bits(x_whole[nl - 1][:, t:t + n]))
        assert torch.equal(_bits(z[:, :, :n]), _bits(z_whole[:, :, t:t + n]))
        assert torch.isnan(z[:, :, n:].float()).all() and torch.isnan(out_b[:, n:].float()).all()   # nothing behind the chunk
        buf[:, :hist] = buf[:, n:n + hist].clone()
        clock += n
        t += n


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _check_oracle(name, dt, probs, logits, what):
    _, _, lg, pr = _oracle(name)
    assert probs.shape == pr.shape and logits.shape == lg.shape
    el, ep = rel_err(logits, lg), rel_err(probs, pr)
    _say("%s case %s %s: logits %.3g probs %.3g" % (what, name, dt, el, ep))
    tl, tp = (TOL_F32, TOL_F32) if dt == F32 else (TOL_BF16_LOGITS, TOL_BF16_PROBS)
    # the check can tell one window position from the next: consecutive oracle emissions differ by >= 3 x the bound
    # applied, every pair of every stream -- in fp32.  With the bf16 bound that cannot hold on these inputs, whatever the
    # code does: the oracle's smallest single step is 1.03e-2 (case a) / 6.45e-3 (case b) of the logit scale, 2.7 x / 1.7 x
    # the bf16 bound of 3.86e-3.  What is asserted there is what these inputs give: every pair differs by more than the
    # bound itself, and the largest step of every stream -- which is what the error above (the largest deviation anywhere
    # over the largest oracle logit) shows when a window is one hop off, since every emission of the stream then sits
    # where its neighbour belongs -- by >= 3 x the bound (4.6e-2 / 5.5e-2 for the stream where it is smallest).  The fp32
    # runs hold the same indexing to the per-pair form.
    steps = np.abs(np.diff(lg, axis=1)).max(-1) / np.abs(lg).max()               # [B, n_emit - 1]
    pair, stream = steps.min(), steps.max(-1).min()
    _say("%s case %s: oracle steps between consecutive emissions, of the logit scale: smallest pair %.3g, smallest "
         "per-stream largest %.3g" % (what, name, pair, stream))
    if dt == F32:
        assert pair >= 3 * tl, (pair, tl)
    else:
        assert pair > tl and stream >= 3 * tl, (pair, stream, tl)
    assert el < tl and ep < tp, (el, ep)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["a", "b"])
def test_against_the_oracle(name, fused, dt, monkeypatch):
    c = _classifier(name, dt, monkeypatch, fused)
    assert c.fused == fused
    probs, logits = c.classify(_oracle(name)[1], return_logits=True)
    n_emit = {"a": 10, "b": 34}[name]
    assert probs.shape[1] == n_emit and c._state.emitted == n_emit and c._state.t == CASES[name][5]
    _check_oracle(name, dt, probs.cpu().numpy(), logits.cpu().numpy(), "fused" if fused else "twin")


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("name", ["a", "b"])
def test_fused_against_twin(name, dt, monkeypatch):
    a = _classifier(name, dt, monkeypatch, True).classify(_oracle(name)[1], return_logits=True)[1].cpu().numpy()
    b = _classifier(name, dt, monkeypatch, False).classify(_oracle(name)[1], return_logits=True)[1].cpu().numpy()
    d = rel_err(a, b)
    _say("fused against twin, case %s %s: %.3g" % (name, dt, d))
    assert d <= 2 * MEASURED_TWIN[dt]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("fused", [True, False])
def test_chunking_changes_no_bit(fused, dt, monkeypatch):
    c = _classifier("a", dt, monkeypatch, fused)
    audio = torch.tensor(_oracle("a")[1])
    whole = c.classify(audio, return_logits=True)
    st = c.start(audio.shape[0])
    parts, at = [], 0
    for n in (1, 31, 33, 160, 7, audio.shape[1]):
        n = min(n, audio.shape[1] - at)
        parts.append(c.push(st, audio[:, at:at + n], return_logits=True))
        at += n
        assert st.t == at and st.pending == at % 32
    assert [p[0].shape[1] for p in parts] == [0, 0, 0, 4, 0, 6] and st.emitted == 10
    for i in (0, 1):
        assert torch.equal(_bits(torch.cat([p[i] for p in parts], 1)), _bits(whole[i]))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_batch_rows_change_no_bit(dt, monkeypatch):
    c = _classifier("a", dt, monkeypatch, True)
    audio = torch.tensor(_oracle("a")[1])
    whole = c.classify(audio, return_logits=True)
    alone = c.classify(audio[2:3], return_logits=True)
    for i in (0, 1):
        assert torch.equal(_bits(alone[i][0]), _bits(whole[i][2]))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_graph_replay_changes_no_bit(dt, monkeypatch):
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "1")
    g = _classifier("a", dt, monkeypatch, True)
    e = _classifier("a", dt, monkeypatch, True)
    e.use_graphs = False
    audio = torch.tensor(_oracle("a")[1])
    want = e.classify(audio, return_logits=True)
    for rep in range(3):      # eager, capture + replay, replay
        got = g.classify(audio, return_logits=True)
        for i in (0, 1):
            assert torch.equal(_bits(got[i]), _bits(want[i])), rep
    assert g._graphs and not e._graphs


def test_single_window_is_predict():
    """window = input_size = T: the one emission is WaveNet.predict's probabilities (another summation order, so within
    the fp32 bound, not bit for bit)."""
    M = sub("model")
    dil, T, B, Cc = [1, 2, 4, 8, 16, 32, 64, 1, 2, 4], 200, 2, 12
    sp = O.init_stack_params(11, dil, 2, 32, 128, Cc, bias_scale=0.05)
    audio = O.synthetic_audio(B, T, seed=9)
    m = M.WaveNet(T, Cc, dil, dilation_channels=32, skip_channels=128, output_channels=Cc, dtype=F32)
    m._engine(B, T).load_oracle_params(sp)
    want = m.predict(audio)
    rec = m.recognizer(max_batch=B)
    assert (rec.hop, rec.window) == (T, T)
    got = rec.classify(audio)
    assert got.shape == want.shape == (B, 1, Cc)
    assert rel_err(got, want) < 1e-3
    s = rec.stream(B)
    assert s.push(audio[:, :150]).shape == (B, 0, Cc) and (s.t, s.emitted) == (150, 0)
    assert np.array_equal(s.push(audio[:, 150:]), got) and (s.t, s.emitted) == (T, 1)
    with pytest.raises(ValueError, match="samples"):      # predict keeps its length refusal
        m.predict(audio[:, :150])


@pytest.mark.parametrize("fmt", ["pt", "tf"])
def test_checkpoint_round_trip(fmt, tmp_path):
    """WaveNet.save -> StreamingClassifier.from_checkpoint (ClassifierWeights.load by the reference's variable names, both
    file forms) classifies as WaveNet.recognizer() on the same weights does, bit for bit."""
    M = sub("model")
    dil, R, S, Cc, B, T, window, hop, _ = CASES["a"]
    m = M.WaveNet(200, Cc, dil, dilation_channels=R, skip_channels=S, output_channels=Cc, dtype=F32)
    m._engine(B, 200).load_oracle_params(_oracle("a")[0])
    assert m.save(str(tmp_path), 3, force=True, fmt=fmt)
    audio = np.array(_oracle("a")[1])
    want = m.recognizer(max_batch=B, hop=hop, window=window).classify(audio, return_logits=True)
    rec = M.StreamingClassifier.from_checkpoint(str(tmp_path), dil, Cc, R, S, dtype=F32, max_batch=B, hop=hop, window=window)
    got = rec.classify(audio, return_logits=True)
    assert got[0].shape == (B, 10, Cc) and rel_err(got[1], _oracle("a")[2]) < TOL_F32
    for i in (0, 1):
        assert np.array_equal(got[i], want[i])
    with pytest.raises(FileNotFoundError):
        M.StreamingClassifier.from_checkpoint(str(tmp_path / "none"), dil, Cc, R, S, dtype=F32)
