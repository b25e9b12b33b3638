"""GPU tests of the streaming likelihood scorer (srwn_version() 116; scorer.StreamScorer, model.WaveNetTeacher.scorer).

  oracle      nll, logits and the most likely code against the fp64 oracle's teacher forward (stack_forward with
              shift_input, log_prob_from_logits, mu_law_encode), all four widths, 256 and 100 classes (Cp = 128: the padded
              columns must stay out of the log-sum-exp), one stream and three, both dtypes
  engine      the mean of score(audio) against WaveNetTeacher.loss on a training engine of that (B, T)
  invariants  chunking, batch rows, a second start, the parity twin and graph replay leave every bit where it was
  model       WaveNetTeacher.scorer() scores with the trained weights and keeps them; from_checkpoint; bits_per_sample
"""
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_kernels import rel_err

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 1, 2, 5]      # several layer groups of both kinds (stride 1, residue classes), history > a chunk
T, MAX_CHUNK, BMAX = 300, 128, 3                   # steps of 128, 128 and 44 rows: whole tiles and a masked last one
WIDTHS = [(64, 256), (32, 128), (32, 256), (64, 128)]
CLASSES = [256, 100]
# Largest |nll - oracle nll| in nats over the cases of test_against_the_oracle, per dtype: the bounds are twice the worst
# measured on MI355X (the project's convention; SRWN_PRINT_ERR=1 pytest -s prints every figure; the fused head
# and its twin give the same bits, so the same figures).
#   fp32 7.72e-7 .. 9.41e-7 (nll 4.2 .. 5.9 nats: two units in the last place)      bf16 8.24e-4 .. 1.76e-3
#   (logits, max-abs / max-abs: fp32 6.9e-7 .. 1.1e-6, bf16 3.6e-3 .. 5.6e-3; argmax agreement fp32 1.0000, bf16 >= 0.9867)
MEASURED_NLL = {F32: 9.41e-7, BF16: 1.76e-3}
# |mean(score) - WaveNetTeacher.loss| in nats, same rule; fp32 is also held to the project's fp32 loss bound, 1e-3 |loss|.
#   fp32 1.78e-7 .. 2.74e-7      bf16 1.65e-7 .. 3.19e-7      (losses 4.62 and 5.55: both paths sum the same rows' values, the
#   engine in its own order; the difference is below one fp32 unit in the last place of the loss in every case)
MEASURED_LOSS = {F32: 2.74e-7, BF16: 3.19e-7}
TOL_LOGITS = {F32: 1e-3, BF16: 6e-2}              # the bounds the project holds generation logits to (test_gpu_generate.py)
_ORACLE = {}


def _bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(t))
    return t.contiguous().view(torch.uint8)


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _tol(table, dt):
    assert table[dt] is not None, "no measured figure recorded for %s" % dt
    return 2 * table[dt]


def _oracle(R, S, Cc):
    """(params, audio [BMAX, T], nll [BMAX, T], logits [BMAX, T, C]) of a case in fp64: computed once, shared, never
    changed.  The first row of the batch is the one-stream case."""
    key = (R, S, Cc)
    if key not in _ORACLE:
        sp = O.init_stack_params(11, DIL, 2, R, S, Cc, bias_scale=0.05)
        audio = O.synthetic_audio(BMAX, T, seed=4)
        logits, _ = O.stack_forward(sp, audio.astype(np.float64), shift_input=True)
        codes = O.mu_law_encode(audio, Cc)
        nll = -np.take_along_axis(O.log_prob_from_logits(logits), codes[..., None].astype(np.int64), -1)[..., 0]
        for a in (audio, nll, logits):
            a.setflags(write=False)
        _ORACLE[key] = (sp, audio, nll, logits)
    return _ORACLE[key]


def _scorer(R, S, Cc, dt, monkeypatch, fused=True, max_batch=BMAX, max_chunk=MAX_CHUNK, graphs=True):
    Sc = sub("scorer")
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1" if fused else "0")
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "1" if graphs else "0")
    w = Sc.ScorerWeights(DIL, R, S, Cc, 2, dt)
    w.load_oracle_params(_oracle(R, S, Cc)[0])
    s = Sc.StreamScorer(w, max_batch=max_batch, max_chunk=max_chunk)
    assert s.fused == fused and s.use_graphs == graphs
    assert s.launches_per_step == 2 + len(s.groups) + (1 if fused else 4) and len(s.groups) >= 2
    return s


# ---- against the fp64 oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cc", CLASSES)
@pytest.mark.parametrize("R,S", WIDTHS)
def test_against_the_oracle(R, S, Cc, B, dt, monkeypatch):
    _, audio, want_nll, want_logits = _oracle(R, S, Cc)
    s = _scorer(R, S, Cc, dt, monkeypatch)
    nll, logits, best = s.score(audio[:B], return_logits=True, return_best=True)
    assert nll.shape == (B, T) and logits.shape == (B, T, Cc) and best.shape == (B, T)
    assert nll.dtype == torch.float32 and best.dtype == torch.int32 and s._state.t == T
    nll, logits, best = nll.cpu().numpy(), logits.cpu().numpy(), best.cpu().numpy()
    e_nll = float(np.abs(nll - want_nll[:B]).max())
    e_log = rel_err(logits, want_logits[:B])
    agree = float((best == want_logits[:B].argmax(-1)).mean())
    _say("oracle R=%d S=%d C=%d B=%d %s: nll abs %.3g (nll in [%.3g, %.3g]) logits rel %.3g argmax %.4f"
         % (R, S, Cc, B, dt, e_nll, want_nll.min(), want_nll.max(), e_log, agree))
    assert np.isfinite(nll).all() and (nll > 0).all()
    assert 0 <= best.min() and best.max() < Cc                 # never a padded column
    assert e_log < TOL_LOGITS[dt], e_log
    if dt == F32:
        assert agree > 0.999, agree
    assert e_nll < _tol(MEASURED_NLL, dt), e_nll


def test_padded_columns_stay_out_of_the_log_sum_exp(monkeypatch):
    """C = 100 pads to 128 columns whose logits are exactly 0.  With every real logit pushed far below 0 (the last bias at
    -30) a padded column that reached the max or the sum would lift the log-sum-exp by ~30 nats and win the argmax."""
    R, S, Cc = 32, 128, 100
    _, audio, _, _ = _oracle(R, S, Cc)
    for fused in (True, False):
        s = _scorer(R, S, Cc, F32, monkeypatch, fused=fused, max_batch=1)
        s.w.view("head_b2")[:Cc] -= 30.0
        nll, logits, best = s.score(audio[:1, :70], return_logits=True, return_best=True)
        lg = logits.double().cpu().numpy()
        assert lg.max() < -20.0
        want = -np.take_along_axis(O.log_prob_from_logits(lg), O.mu_law_encode(audio[:1, :70], Cc)[..., None].astype(np.int64),
                                   -1)[..., 0]
        assert np.abs(nll.cpu().numpy() - want).max() < 1e-4
        assert np.array_equal(best.cpu().numpy(), lg.argmax(-1))


# ---- against the training engine ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("R,S,Cc,B", [(64, 256, 256, 3), (32, 128, 100, 1)])
def test_mean_is_the_training_loss(R, S, Cc, B, dt, monkeypatch):
    M = sub("model")
    sp, audio, want_nll, _ = _oracle(R, S, Cc)
    m = M.WaveNetTeacher(T, 0, DIL, dilation_channels=R, skip_channels=S, quantization_channels=Cc, dtype=dt)
    m._engine(B, T).load_oracle_params(sp)
    loss = float(m.loss(audio[:B]))
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1")
    got = float(m.scorer(max_batch=B, max_chunk=MAX_CHUNK).score(audio[:B]).astype(np.float64).mean())
    _say("engine R=%d S=%d C=%d B=%d %s: loss %.6f mean nll %.6f diff %.3g (oracle %.6f)"
         % (R, S, Cc, B, dt, loss, got, abs(got - loss), want_nll[:B].mean()))
    if dt == F32:
        assert abs(got - loss) < 1e-3 * abs(loss), (got, loss)
    assert abs(got - loss) < _tol(MEASURED_LOSS, dt), (got, loss)


# ---- invariants ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fused", [True, False])
def test_chunking_changes_no_bit(fused, dt, monkeypatch):
    R, S, Cc = 64, 256, 100
    audio = torch.tensor(_oracle(R, S, Cc)[1])
    s = _scorer(R, S, Cc, dt, monkeypatch, fused=fused)
    whole = s.score(audio, return_logits=True, return_best=True)
    st = s.start(BMAX)
    parts, at = [], 0
    for n in (1, 31, 33, 97, 0, 128, 10):
        parts.append(s.push(st, audio[:, at:at + n], return_logits=True, return_best=True))
        assert parts[-1][0].shape == (BMAX, n)
        at += n
        assert st.t == at
    assert at == T
    for i in range(3):
        assert torch.equal(_bits(torch.cat([p[i] for p in parts], 1)), _bits(whole[i])), i
    again = s.score(audio, return_logits=True, return_best=True)      # a second start on the same object
    for i in range(3):
        assert torch.equal(_bits(again[i]), _bits(whole[i])), i


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_batch_rows_change_no_bit(dt, monkeypatch):
    R, S, Cc = 32, 128, 256
    audio = torch.tensor(_oracle(R, S, Cc)[1])
    whole = _scorer(R, S, Cc, dt, monkeypatch).score(audio, return_logits=True, return_best=True)
    one = _scorer(R, S, Cc, dt, monkeypatch, max_batch=1)
    for b in range(BMAX):
        alone = one.score(audio[b:b + 1], return_logits=True, return_best=True)
        for i in range(3):
            assert torch.equal(_bits(alone[i][0]), _bits(whole[i][b])), (b, i)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Cc", CLASSES)
@pytest.mark.parametrize("R,S", WIDTHS)
def test_fused_against_twin(R, S, Cc, dt, monkeypatch):
    audio = _oracle(R, S, Cc)[1]
    a = _scorer(R, S, Cc, dt, monkeypatch, fused=True).score(audio, return_logits=True, return_best=True)
    b = _scorer(R, S, Cc, dt, monkeypatch, fused=False).score(audio, return_logits=True, return_best=True)
    _say("fused against twin R=%d S=%d C=%d %s: nll max diff %.3g" % (R, S, Cc, dt, float((a[0] - b[0]).abs().max())))
    for i in range(3):
        assert torch.equal(_bits(a[i]), _bits(b[i])), i


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_graph_replay_changes_no_bit(dt, monkeypatch):
    R, S, Cc = 64, 128, 100
    audio = torch.tensor(_oracle(R, S, Cc)[1])
    e = _scorer(R, S, Cc, dt, monkeypatch, graphs=False)
    g = _scorer(R, S, Cc, dt, monkeypatch, graphs=True)
    want = e.score(audio, return_logits=True, return_best=True)
    for rep in range(3):      # eager + capture + replay, then replays
        got = g.score(audio, return_logits=True, return_best=True)
        for i in range(3):
            assert torch.equal(_bits(got[i]), _bits(want[i])), (rep, i)
    assert g._graphs and not e._graphs
    plain = g.score(audio)    # another key: no optional output
    assert torch.equal(_bits(plain), _bits(want[0]))


def test_buffer_bytes(monkeypatch):
    s = _scorer(32, 128, 100, BF16, monkeypatch)
    bb = s.buffer_bytes()
    assert bb["z"] == len(DIL) * BMAX * MAX_CHUNK * 32 * 2 and bb["scores"] == 2 * BMAX * MAX_CHUNK * 4
    s.score(_oracle(32, 128, 100)[1], return_logits=True)
    assert s.buffer_bytes()["scores"] == bb["scores"] + BMAX * MAX_CHUNK * 100 * 4
    assert "twin r0/r1/logits" in _scorer(32, 128, 100, BF16, monkeypatch, fused=False).buffer_bytes()


# ---- the model face --------------------------------------------------------------------------------------------------------
def test_model_face(tmp_path):
    M = sub("model")
    dil, B, Tm, R, S, Cc = [1, 2, 4, 8, 1, 2], 2, 200, 32, 128, 256
    audio = O.synthetic_audio(B, Tm, seed=6)
    m = M.WaveNetTeacher(Tm, 0, dil, dilation_channels=R, skip_channels=S, quantization_channels=Cc, dtype=F32,
                         learning_rate=1e-3)
    untrained = float(m.loss(audio))
    for _ in range(3):
        m.train(audio)
    sc = m.scorer(max_batch=B, max_chunk=64)
    nll = sc.score(audio)
    loss = float(m.loss(audio))
    assert isinstance(nll, np.ndarray) and nll.shape == (B, Tm) and nll.dtype == np.float32
    assert abs(float(nll.astype(np.float64).mean()) - loss) < 1e-3 * abs(loss)       # the trained weights ...
    # ... which are not the initial ones: the untrained loss lies further off than twice the bound just applied, so the
    # match above cannot hold for both sets of weights
    assert abs(loss - untrained) > 2 * 1e-3 * abs(loss)
    for _ in range(2):
        m.train(audio)                                                               # later training does not reach it
    assert np.array_equal(sc.score(audio), nll)
    # save -> from_checkpoint round-trips
    assert m.save(str(tmp_path), 5, force=True)
    want = m.scorer(max_batch=B, max_chunk=64).score(audio, return_best=True)
    got = M.StreamingScorer.from_checkpoint(str(tmp_path), dtype=F32, max_batch=B, max_chunk=64).score(audio, return_best=True)
    for i in range(2):
        assert np.array_equal(got[i], want[i])
    assert not np.array_equal(want[0], nll)                                          # (the teacher itself did move on)
    # a stream, and bits per sample on noise
    st = sc.stream(B)
    assert np.isnan(st.bits_per_sample()).all()
    noise = np.random.default_rng(0).uniform(-1, 1, size=(B, 150)).astype(np.float32)
    parts = [st.push(noise[:, :70]), st.push(noise[:, 70:70]), st.push(noise[:, 70:])]
    assert [p.shape for p in parts] == [(B, 70), (B, 0), (B, 80)] and st.t == 150
    bps = st.bits_per_sample()
    assert bps.shape == (B,) and np.isfinite(bps).all() and (bps > 0).all()
    allnll = np.concatenate(parts, 1).astype(np.float64)
    assert np.allclose(bps, allnll.mean(1) / np.log(2.0), rtol=1e-6)
    assert np.array_equal(np.concatenate(parts, 1), sc.score(noise))
