"""GPU tests of the streaming likelihood scorer of the conditioned mixture-of-logistics decoder (srwn_version() 117;
scorer.MolStreamScorer, model.AutoEncoderScorer, model.WaveNetTeacher.mol_scorer).

  oracle      nll and logits against the fp64 oracle's decoder forward (stack_forward with shift_input and cond,
              mol_log_probs, log_sum_exp): all four widths, M = 4 (lanes of a row without a mixture, Cp = 32) and M = 10
              (lanes with one and with two, Cp = 64), unconditioned and conditioned through a ring that wraps, one stream
              and three, both dtypes
  branches    an input on which every tf.where branch of the head and the log-scale floor are taken
  engine      the sum of score(audio) against the loss of WaveNetAutoEncoder's decoder engine and of a mixture-of-logistics
              WaveNetTeacher on the same parameters (the engines' reduction is a SUM)
  invariants  chunking x feed cuts, batch rows, a second start, the parity twin and graph replay leave every bit in place
  model       AutoEncoderScorer: score == score_with_encoding(encode), a ragged stream == score, snapshots, from_checkpoint,
              bits_per_sample; WaveNetTeacher.mol_scorer
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
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 1, 2, 5]      # several layer groups of both kinds, the longest history > a chunk
T, MAX_CHUNK, BMAX = 300, 128, 3                   # steps of 128, 128 and 44 rows: whole tiles and a masked last one
WIDTHS = [(64, 256), (32, 128), (32, 256), (64, 128)]
MIXTURES = [4, 10]
CONDS = [0, 6]
POOL, FRAMES = 20, 15
# Largest |nll - oracle nll| in nats over the cases of test_against_the_oracle, per dtype: the bounds are twice the worst
# measured on MI355X (the project's convention; SRWN_PRINT_ERR=1 pytest -s prints every figure; the fused head
# and its twin give the same bits, so the same figures).
#   fp32 1.30e-5 .. 4.22e-5 (nll 5.8 .. 6.9 nats; the head multiplies an error of the means by exp(-log_scale))
#   bf16 3.18e-4 .. 5.37e-3
#   (logits, max-abs / max-abs: fp32 5.6e-7 .. 1.3e-6, bf16 3.8e-3 .. 9.0e-3; |sum - oracle sum| / |sum|: fp32 <= 2.4e-7,
#   bf16 <= 1.2e-4)
MEASURED_NLL = {F32: 4.22e-5, BF16: 5.37e-3}
# the same on the input of test_all_four_branches (fp32 only: bf16 is held to fused == twin there)
#   fp32 3.77e-4 (32 x 128, M = 4) and 5.50e-4 (64 x 256, M = 10), nll 0.85 .. 8.6 nats: at the log-scale floor of -7 the
#   head multiplies an error of a mean by e^7
MEASURED_NLL_BRANCHES = {F32: 5.50e-4}
# |sum(score) - engine loss| in nats, same rule; fp32 is also held to the project's fp32 loss bound, 1e-3 |loss|.
#   fp32 4.34e-5 (loss 1948.97) and 2.02e-4 (loss 5629.54)      bf16 6.48e-5 and 1.22e-4      the same figures against the
#   auto-encoder's decoder engine and against the teacher's; every one lies below one fp32 unit in the last place of the
#   loss (1.2e-4 and 4.9e-4): both paths sum the same rows' values, the engine in fp32 in its own order
MEASURED_LOSS = {F32: 2.02e-4, BF16: 1.22e-4}
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


def _oracle(R, S, M, E, branches=False):
    """(params, audio [BMAX, T], cond [BMAX, FRAMES, E] or None, nll [BMAX, T], logits [BMAX, T, 4M], aux) of a case in
    fp64: computed once, shared, never changed.  The first row of the batch is the one-stream case.  branches: the input
    of test_all_four_branches."""
    key = (R, S, M, E, branches)
    if key not in _ORACLE:
        sp = O.init_stack_params(11, DIL, 2, R, S, 4 * M, cond_channels=E, bias_scale=0.05)
        audio = O.synthetic_audio(BMAX, T, seed=4).copy()
        if branches:
            audio[:, [5, 150]] = -1.0
            audio[:, [9, 299]] = 1.0
            sp.head_b2[2 * M:2 * M + M // 2] -= 9.0
        cond = np.random.default_rng(7).normal(size=(BMAX, FRAMES, E)) if E else None
        logits, _ = O.stack_forward(sp, audio.astype(np.float64), shift_input=True, cond=cond, pool_stride=POOL)
        lp, aux = O.mol_log_probs(audio.astype(np.float64), logits)
        nll = -O.log_sum_exp(lp)
        for a in (audio, nll, logits) + ((cond,) if E else ()):
            a.setflags(write=False)
        _ORACLE[key] = (sp, audio, cond, nll, logits, aux)
    return _ORACLE[key]


def _hist_max():
    """The largest group history of the scorer's plan for DIL (the halo a chunk recomputes with its conditioning)."""
    from types import SimpleNamespace
    return max(sum(DIL[a:b]) for a, b in sub("scorer").MolStreamScorer._plan(SimpleNamespace(dil=DIL)))


def _max_frames(hist_max=None):
    """One frame more than the smallest ring a live stream can run on."""
    return sub("student").live_min_frames(_hist_max() if hist_max is None else hist_max, POOL) + 1


def _scorer(R, S, M, E, dt, monkeypatch, fused=True, max_batch=BMAX, max_chunk=MAX_CHUNK, graphs=True, branches=False):
    Sc = sub("scorer")
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1" if fused else "0")
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "1" if graphs else "0")
    w = Sc.MolScorerWeights(DIL, R, S, M, E, POOL, 2, dt)
    w.load_oracle_params(_oracle(R, S, M, E, branches)[0])
    hist_max = _hist_max()
    s = Sc.MolStreamScorer(w, max_batch=max_batch, max_chunk=max_chunk, max_frames=_max_frames(hist_max))
    assert s.fused == fused and s.use_graphs == graphs
    assert s.launches_per_step == 2 + len(s.groups) + (1 if fused else 4) and len(s.groups) >= 2
    if E:      # the ring is shorter than the clip: it wraps
        assert s.hist_max == hist_max and s.max_frames == _max_frames(hist_max) < FRAMES, (s.max_frames, FRAMES)
    return s


def _enc(cond, B=None):
    return None if cond is None else torch.tensor(cond[:B] if B else cond, dtype=torch.float32)


# ---- against the fp64 oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E", CONDS)
@pytest.mark.parametrize("M", MIXTURES)
@pytest.mark.parametrize("R,S", WIDTHS)
def test_against_the_oracle(R, S, M, E, B, dt, monkeypatch):
    _, audio, cond, want_nll, want_logits, _ = _oracle(R, S, M, E)
    s = _scorer(R, S, M, E, dt, monkeypatch)
    nll, logits = s.score(audio[:B], _enc(cond, B), return_logits=True)
    assert nll.shape == (B, T) and logits.shape == (B, T, 4 * M)
    assert nll.dtype == torch.float32 and s._state.t == T and s._state.fed == (FRAMES if E else 0)
    nll, logits = nll.cpu().numpy(), logits.cpu().numpy()
    e_nll = float(np.abs(nll - want_nll[:B]).max())
    e_log = rel_err(logits, want_logits[:B])
    e_sum = abs(float(nll.astype(np.float64).sum()) - float(want_nll[:B].sum()))
    _say("oracle R=%d S=%d M=%d E=%d B=%d %s: nll abs %.3g (nll in [%.3g, %.3g]) sum diff %.3g of %.6g logits rel %.3g"
         % (R, S, M, E, B, dt, e_nll, want_nll.min(), want_nll.max(), e_sum, want_nll[:B].sum(), e_log))
    assert np.isfinite(nll).all()
    assert e_log < TOL_LOGITS[dt], e_log
    if dt == F32:
        assert e_sum < 1e-3 * abs(float(want_nll[:B].sum())), e_sum
    assert e_nll < _tol(MEASURED_NLL, dt), e_nll


@pytest.mark.parametrize("R,S,M", [(32, 128, 4), (64, 256, 10)])
def test_all_four_branches(R, S, M, monkeypatch):
    """Samples at -1 and +1 (the two edge branches), half the log-scales pushed under the floor of -7 (a bin narrow enough
    for cdf_delta <= 1e-5: the pdf branch) and the ordinary bin branch: the oracle says each one is taken."""
    E = 6
    _, audio, cond, want_nll, want_logits, aux = _oracle(R, S, M, E, branches=True)
    counts = [int((aux["case"] == c).sum()) for c in range(4)]
    _say("branches R=%d S=%d M=%d: case counts %s, log-scales above the floor %.3f" % (R, S, M, counts, aux["clamp"].mean()))
    assert all(c > 0 for c in counts), counts
    assert not aux["clamp"].all() and aux["clamp"].any()
    s = _scorer(R, S, M, E, F32, monkeypatch, branches=True)
    nll, logits = s.score(audio, _enc(cond), return_logits=True)
    e_nll = float(np.abs(nll.cpu().numpy() - want_nll).max())
    e_log = rel_err(logits.cpu().numpy(), want_logits)
    _say("branches R=%d S=%d M=%d fp32: nll abs %.3g (nll in [%.3g, %.3g]) logits rel %.3g"
         % (R, S, M, e_nll, want_nll.min(), want_nll.max(), e_log))
    assert torch.isfinite(nll).all()
    assert e_log < TOL_LOGITS[F32], e_log
    assert e_nll < _tol(MEASURED_NLL_BRANCHES, F32), e_nll
    a = _scorer(R, S, M, E, BF16, monkeypatch, fused=True, branches=True).score(audio, _enc(cond), return_logits=True)
    b = _scorer(R, S, M, E, BF16, monkeypatch, fused=False, branches=True).score(audio, _enc(cond), return_logits=True)
    assert torch.isfinite(a[0]).all()
    for i in range(2):
        assert torch.equal(_bits(a[i]), _bits(b[i])), i


# ---- against the training engines ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("R,S,M,B", [(64, 256, 10, 3), (32, 128, 4, 1)])
def test_sum_is_the_training_loss(R, S, M, B, dt, monkeypatch):
    Md = sub("model")
    E = 6
    sp, audio, cond, want_nll, _, _ = _oracle(R, S, M, E)
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1")
    # the auto-encoder's decoder engine on the oracle's parameters and encoding
    ae = Md.WaveNetAutoEncoder(T, 0, M, DIL, dilation_channels=R, skip_channels=S, latent_channels=E, pool_stride=POOL,
                               dtype=dt)
    eng = ae._engine(B, T)
    eng.dec.load_oracle_params(sp)
    ae._stage(audio[:B], None)
    ae._put_encoding(eng, cond[:B])
    eng.dec.forward()
    loss_ae = float(eng.dec.loss.item())
    got_ae = float(ae.scorer(max_batch=B, max_chunk=MAX_CHUNK, max_frames=_max_frames())
                   .score_with_encoding(audio[:B], cond[:B]).astype(np.float64).sum())
    # a mixture-of-logistics teacher on the same parameters
    te = Md.WaveNetTeacher(T, 0, DIL, dilation_channels=R, skip_channels=S, latent_channels=E, pool_stride=POOL,
                           use_encoding=True, dtype=dt, head="mol", num_mixtures=M)
    te._engine(B, T).load_oracle_params(sp)
    loss_te = float(te.loss(audio[:B], encoding=cond[:B]))
    got_te = float(te.mol_scorer(max_batch=B, max_chunk=MAX_CHUNK, max_frames=_max_frames())
                   .score(audio[:B], cond[:B]).astype(np.float64).sum())
    want = float(want_nll[:B].sum())
    _say("engine R=%d S=%d M=%d B=%d %s: AE loss %.6f sum nll %.6f diff %.3g | teacher loss %.6f sum nll %.6f diff %.3g "
         "(oracle %.6f)" % (R, S, M, B, dt, loss_ae, got_ae, abs(got_ae - loss_ae), loss_te, got_te, abs(got_te - loss_te),
                            want))
    for got, loss in ((got_ae, loss_ae), (got_te, loss_te)):
        if dt == F32:
            assert abs(got - loss) < 1e-3 * abs(loss), (got, loss)
        assert abs(got - loss) < _tol(MEASURED_LOSS, dt), (got, loss)


# ---- invariants ----------------------------------------------------------------------------------------------------------
def _cut_run(s, audio, cond, cuts, feed_all):
    """The stream pushed in pieces of `cuts` samples, fed one frame at a time (or, feed_all, as many as the ring has room
    for) whenever the next piece needs more than is available."""
    st = s.start(audio.shape[0])
    parts, at = [], 0
    for n in cuts:
        got, left = [], n
        while True:      # a piece larger than what the ring can cover at once goes in several pushes
            if cond is not None:
                while s.available(st) < left and st.fed < FRAMES and s.room(st) > 0:
                    k = min(s.room(st), FRAMES - st.fed) if feed_all else 1
                    s.feed(st, cond[:, st.fed:st.fed + k])
            m = int(min(left, s.available(st)))
            got.append(s.push(st, audio[:, at:at + m], return_logits=True))
            at, left = at + m, left - m
            if left == 0:
                break
            assert m > 0
        parts.append((torch.cat([g[0] for g in got], 1), torch.cat([g[1] for g in got], 1)))
        assert parts[-1][0].shape == (audio.shape[0], n) and st.t == at
    return parts


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("E", CONDS)
def test_chunking_and_feed_cuts_change_no_bit(E, fused, dt, monkeypatch):
    R, S, M = 64, 256, 10
    _, audio, cond, _, _, _ = _oracle(R, S, M, E)
    audio, cond = torch.tensor(audio), _enc(cond)
    s = _scorer(R, S, M, E, dt, monkeypatch, fused=fused)
    whole = s.score(audio, cond, return_logits=True)
    cuts = (1, 31, 33, 97, 0, 128, 10)
    assert sum(cuts) == T
    for feed_all in ((False, True) if E else (False,)):
        parts = _cut_run(s, audio, cond, cuts, feed_all)
        for i in range(2):
            assert torch.equal(_bits(torch.cat([p[i] for p in parts], 1)), _bits(whole[i])), (feed_all, i)
    again = s.score(audio, cond, return_logits=True)      # a second start on the same object
    for i in range(2):
        assert torch.equal(_bits(again[i]), _bits(whole[i])), i


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_batch_rows_change_no_bit(dt, monkeypatch):
    R, S, M, E = 32, 128, 4, 6
    _, audio, cond, _, _, _ = _oracle(R, S, M, E)
    audio, cond = torch.tensor(audio), _enc(cond)
    whole = _scorer(R, S, M, E, dt, monkeypatch).score(audio, cond, return_logits=True)
    one = _scorer(R, S, M, E, dt, monkeypatch, max_batch=1)
    for b in range(BMAX):
        alone = one.score(audio[b:b + 1], cond[b:b + 1], return_logits=True)
        for i in range(2):
            assert torch.equal(_bits(alone[i][0]), _bits(whole[i][b])), (b, i)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("E", CONDS)
@pytest.mark.parametrize("M", MIXTURES)
@pytest.mark.parametrize("R,S", WIDTHS)
def test_fused_against_twin(R, S, M, E, dt, monkeypatch):
    _, audio, cond, _, _, _ = _oracle(R, S, M, E)
    a = _scorer(R, S, M, E, dt, monkeypatch, fused=True).score(audio, _enc(cond), return_logits=True)
    b = _scorer(R, S, M, E, dt, monkeypatch, fused=False).score(audio, _enc(cond), return_logits=True)
    _say("fused against twin R=%d S=%d M=%d E=%d %s: nll max diff %.3g" % (R, S, M, E, dt, float((a[0] - b[0]).abs().max())))
    for i in range(2):
        assert torch.equal(_bits(a[i]), _bits(b[i])), i


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_graph_replay_changes_no_bit(dt, monkeypatch):
    R, S, M, E = 64, 128, 10, 6
    _, audio, cond, _, _, _ = _oracle(R, S, M, E)
    audio, cond = torch.tensor(audio), _enc(cond)
    e = _scorer(R, S, M, E, dt, monkeypatch, graphs=False)
    g = _scorer(R, S, M, E, dt, monkeypatch, graphs=True)
    want = e.score(audio, cond, return_logits=True)
    for rep in range(3):      # eager + capture + replay, then replays
        got = g.score(audio, cond, return_logits=True)
        for i in range(2):
            assert torch.equal(_bits(got[i]), _bits(want[i])), (rep, i)
    assert g._graphs and not e._graphs
    plain = g.score(audio, cond)    # another key: no optional output
    assert torch.equal(_bits(plain), _bits(want[0]))


def test_buffer_bytes(monkeypatch):
    s = _scorer(32, 128, 4, 6, BF16, monkeypatch)
    bb = s.buffer_bytes()
    assert bb["z"] == len(DIL) * BMAX * MAX_CHUNK * 32 * 2 and bb["scores"] == BMAX * MAX_CHUNK * 4
    assert bb["conditioning"] == BMAX * s.max_frames * (2 * len(DIL) * 32 * 2 + 16 * 2)
    assert "twin r0/r1/logits" in _scorer(32, 128, 4, 6, BF16, monkeypatch, fused=False).buffer_bytes()


# ---- the model face --------------------------------------------------------------------------------------------------------
def test_autoencoder_face(tmp_path):
    Md = sub("model")
    dil, B, P, R, S, M, lat = [1, 2, 4, 8, 1, 2], 2, 16, 32, 128, 4, 8
    Tm = 12 * P
    audio = O.synthetic_audio(B, Tm, seed=6)
    m = Md.WaveNetAutoEncoder(Tm, 0, M, dil, dilation_channels=R, skip_channels=S, latent_channels=lat,
                              pool_stride=P, dtype=F32, learning_rate=1e-3)
    eng = m._stage(audio, None)
    eng.forward()
    untrained = float(eng.loss.item())
    for _ in range(3):
        m.train(audio)
    sc = m.scorer(max_batch=B, max_chunk=64, max_frames=4)
    nll = sc.score(audio)
    eng = m._stage(audio, None)
    eng.forward()
    loss = float(eng.loss.item())
    assert isinstance(nll, np.ndarray) and nll.shape == (B, Tm) and nll.dtype == np.float32
    assert abs(float(nll.astype(np.float64).sum()) - loss) < 1e-3 * abs(loss)         # the trained weights ...
    assert abs(loss - untrained) > 2 * 1e-3 * abs(loss)                               # ... which are not the initial ones
    # score is score_with_encoding on the encoder's frames
    enc = m.encode(audio)
    assert enc.shape == (B, Tm // P, lat)
    assert np.array_equal(sc.score_with_encoding(audio, enc), nll)
    for _ in range(2):
        m.train(audio)                                                                # later training does not reach it
    assert np.array_equal(sc.score(audio), nll)
    # a length that is no multiple of the pool stride: the samples whose frames exist
    assert sc.score(audio[:, :5 * P + 7]).shape == (B, 5 * P)
    # save -> from_checkpoint round-trips
    assert m.save(str(tmp_path), 5, force=True)
    want = m.scorer(max_batch=B, max_chunk=64, max_frames=4).score(audio)
    got = Md.AutoEncoderScorer.from_checkpoint(str(tmp_path), dtype=F32, max_batch=B, max_chunk=64, max_frames=4).score(audio)
    assert np.array_equal(got, want) and not np.array_equal(want, nll)                # (the model itself did move on)
    # a stream in ragged pieces: score, bit for bit
    st = sc.stream(B)
    assert np.isnan(st.bits_per_sample()).all()
    parts, at = [], 0
    for n in (1, 40, 0, 23, 64, Tm - 128):
        parts.append(st.push(audio[:, at:at + n]))
        at += n
        assert parts[-1].shape[0] == B and st.received == at and st.t <= at
    assert at == Tm and parts[0].shape == (B, 0)                                       # no frame is complete after 1 sample
    parts.append(st.finish())
    assert st.t == Tm
    assert np.array_equal(np.concatenate(parts, 1), nll)
    bps = st.bits_per_sample()
    assert bps.shape == (B,) and np.isfinite(bps).all()
    assert np.allclose(bps, nll.astype(np.float64).mean(1) / np.log(2.0), rtol=1e-6)
    with pytest.raises(ValueError, match="closed"):
        st.push(audio[:, :1])


def test_teacher_face():
    Md = sub("model")
    dil, B, Tm, R, S, M = [1, 2, 4, 8, 1, 2], 2, 200, 32, 128, 10
    audio = O.synthetic_audio(B, Tm, seed=6)
    m = Md.WaveNetTeacher(Tm, 0, dil, dilation_channels=R, skip_channels=S, dtype=F32, learning_rate=1e-3, head="mol",
                          num_mixtures=M)
    for _ in range(2):
        m.train(audio)
    sc = m.mol_scorer(max_batch=B, max_chunk=64)
    nll = sc.score(audio)
    loss = float(m.loss(audio))
    assert nll.shape == (B, Tm) and abs(float(nll.astype(np.float64).sum()) - loss) < 1e-3 * abs(loss)
    st = sc.stream(B)
    parts = [st.push(audio[:, :70]), st.push(audio[:, 70:70]), st.push(audio[:, 70:])]
    assert [p.shape for p in parts] == [(B, 70), (B, 0), (B, 130)] and st.t == Tm
    assert np.array_equal(np.concatenate(parts, 1), nll)
    with pytest.raises(ValueError, match="not conditioned"):
        st.feed(np.zeros((B, 1, 4), np.float32))
