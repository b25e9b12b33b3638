"""GPU tests of the standalone streaming encoder (encoder.FrameEncoder, model.AudioEncoder): both paths -- the one-launch
chain srwn_nc_encode_frames and the layer-by-layer twin -- against the fp64 oracle, the bit-equalities the streaming
contract rests on (chunking, batch, launch size, clip order), the clip end, and the model face."""
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub

pytestmark = pytest.mark.gpu

# The bounds test_autoencoder_forward_backward holds the training encoder to
F32_TOL, BF16_TOL = 1e-3, 6e-2
# Both bf16 paths against the fp64 oracle, max-abs / max-abs: 2 x the worst measured on MI355X over the 144 shapes of
# test_against_the_oracle (SRWN_PRINT_ERR=1 pytest -s prints them): 1.26e-3 .. 5.92e-3, the same range for the one-launch
# chain and for the twin (worst at L = 1, P = 512; 30 layers: <= 2.35e-3); fp32 twin: 9.2e-8 .. 6.3e-7
ENC_STREAM_ORACLE_TOL = 1.2e-2

# (name, dtype, SRWN_ENC_FUSED)
PATHS = [("fused", torch.bfloat16, "1"), ("twin16", torch.bfloat16, "0"), ("twin32", torch.float32, "0")]
S_, LAT = 64, 8


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _note(what, e):
    if os.environ.get("SRWN_PRINT_ERR"):
        print("MEASURED %s: %.3e" % (what, e))


_EP, _REF = {}, {}


def _params(L, seed=0):
    if (L, seed) not in _EP:
        _EP[(L, seed)] = O.init_encoder_params(seed, L, 2, 128, S_, LAT, bias_scale=0.05)
    return _EP[(L, seed)]


def _encoder(monkeypatch, path, L, P, max_batch, max_frames=32, seed=0):
    name, dt, fused = path
    monkeypatch.setenv("SRWN_ENC_FUSED", fused)
    E = sub("encoder")
    w = E.EncoderWeights(L, 128, S_, LAT, 2, dt)
    w.load_oracle_params(_params(L, seed))
    fe = E.FrameEncoder(w, P, max_batch=max_batch, max_frames=max_frames)
    assert fe.fused == (name == "fused")
    return fe


def _clip(B, T, seed):
    return np.random.default_rng(seed).uniform(-1, 1, size=(B, T)).astype(np.float32)


# ---- against the fp64 oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("L", [1, 3, 30])
@pytest.mark.parametrize("P", [25, 32, 128, 512])
def test_against_the_oracle(monkeypatch, path, L, P):
    fe = _encoder(monkeypatch, path, L, P, max_batch=9, max_frames=2)        # (3 frames: two launches)
    ep = _params(L)
    worst = 0.0
    for B in (1, 3, 9):
        for T in (P - 1, P, 3 * P, 3 * P + 7, 3 * P + L + 1):
            x = _clip(B, T, 100 * B + T)
            got = fe.encode(torch.as_tensor(x)).cpu().numpy()
            if (L, P, B, T) not in _REF:
                _REF[(L, P, B, T)] = O.encoder_forward(ep, x.astype(np.float64), P)
            ref = _REF[(L, P, B, T)]
            assert got.shape == ref.shape == (B, T // P, LAT)
            if T < P:
                continue
            assert np.isfinite(got).all()
            e = rel_err(got, ref)
            _note("%s encode vs oracle L=%d P=%d B=%d T=%d" % (path[0], L, P, B, T), e)
            worst = max(worst, e)
            if path[1] == torch.float32:
                assert e < F32_TOL, (B, T, e)
            else:
                assert e < BF16_TOL and e < ENC_STREAM_ORACLE_TOL, (B, T, e)
    _note("%s encode vs oracle L=%d P=%d WORST" % (path[0], L, P), worst)


def test_fused_is_as_accurate_as_the_training_encoder(monkeypatch):
    """30 layers, P = 512: the one-launch chain's error against the oracle is at most twice EncoderStack.forward's, at the
    same weights and clip."""
    L, P, B = 30, 512, 3
    T = 3 * P
    E = sub("encoder")
    ep = _params(L)
    x = _clip(B, T, 5)
    ref = O.encoder_forward(ep, x.astype(np.float64), P)
    fe = _encoder(monkeypatch, PATHS[0], L, P, max_batch=B)
    e_fused = rel_err(fe.encode(torch.as_tensor(x)).cpu().numpy(), ref)
    es = E.EncoderStack(L, B, T, P, 128, S_, LAT, 2, torch.bfloat16)
    es.load_oracle_params(ep)
    e_stack = rel_err(es.forward(torch.as_tensor(x, device="cuda")).view(B, T // P, LAT).cpu().numpy(), ref)
    _note("30 layers P=512: fused vs oracle", e_fused)
    _note("30 layers P=512: EncoderStack.forward vs oracle", e_stack)
    assert e_fused <= 2 * e_stack, (e_fused, e_stack)


# ---- bit-equality: what streaming rests on -------------------------------------------------------------------------------
def _stream(fe, x, chunk):
    st = fe.start(x.shape[0])
    outs, t = [], 0
    while t < x.shape[1]:
        outs.append(fe.push(st, x[:, t:t + chunk]))
        assert outs[-1].shape[0] == x.shape[0] and outs[-1].shape[2] == LAT
        assert st.tail.shape[1] < fe.P + fe.L + 1 and st.received == min(t + chunk, x.shape[1])
        t += chunk
    outs.append(fe.finish(st))
    assert st.closed and st.emitted == x.shape[1] // fe.P
    with pytest.raises(ValueError, match="closed"):
        fe.push(st, x[:, :1])
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("L,P", [(5, 32), (30, 128)])
def test_chunking_does_not_change_a_bit(monkeypatch, path, L, P):
    fe = _encoder(monkeypatch, path, L, P, max_batch=2, max_frames=4)
    x = torch.as_tensor(_clip(2, 5 * P + 17, 9))
    whole = fe.encode(x)
    assert whole.shape == (2, 5, LAT)
    for chunk in (1, 7, P, P + 1, 3 * P - 5, x.shape[1]):
        if chunk == 1 and P > 32:
            continue                                   # (one sample at a time: at the small stride only, for the clock)
        got = _stream(fe, x, chunk)
        assert torch.equal(got, whole), (chunk, (got - whole).abs().max().item())
    st = fe.start(2)
    assert fe.push(st, x[:, :0]).shape == (2, 0, LAT)                       # nothing in, nothing out
    assert fe.push(st, x[:, :P + L]).shape == (2, 0, LAT)                   # one sample short of the first frame
    assert torch.equal(fe.push(st, x[:, P + L:P + L + 1]), whole[:, :1])    # ... and there it is
    assert torch.equal(fe.finish(st), whole[:, 1:1])                        # the clip ended at P + L + 1: no more frames


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_batch_launch_size_and_history_do_not_change_a_bit(monkeypatch, path):
    L, P = 30, 128
    fe = _encoder(monkeypatch, path, L, P, max_batch=5, max_frames=32)
    x = torch.as_tensor(_clip(5, 6 * P + 50, 11))
    whole = fe.encode(x)
    for b in (0, 3, 4):                                # a stream in a batch of 5 = the same clip alone
        assert torch.equal(fe.encode(x[b:b + 1]), whole[b:b + 1]), b
    two = _encoder(monkeypatch, path, L, P, max_batch=5, max_frames=2)      # max_frames = 2 = max_frames = 32
    assert torch.equal(two.encode(x), whole)
    y = torch.as_tensor(_clip(3, 2 * P + 9, 12))       # two clips back to back on one object do not see each other
    ey = two.encode(y)
    assert torch.equal(fe.encode(y), ey) and torch.equal(fe.encode(x), whole) and torch.equal(two.encode(y), ey)
    a, b = fe.start(2), fe.start(1)                    # nor do two interleaved streams
    ga = [fe.push(a, x[:2, :3 * P])]; gb = [fe.push(b, y[:1, :P + 40])]
    ga.append(fe.push(a, x[:2, 3 * P:])); gb.append(fe.push(b, y[:1, P + 40:]))
    ga.append(fe.finish(a)); gb.append(fe.finish(b))
    assert torch.equal(torch.cat(ga, 1), whole[:2]) and torch.equal(torch.cat(gb, 1), ey[:1])


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("L,P", [(8, 32), (30, 128)])
def test_the_clip_end_reaches_no_further_than_the_look_ahead(monkeypatch, path, L, P):
    fe = _encoder(monkeypatch, path, L, P, max_batch=2)
    x = torch.as_tensor(_clip(2, 3 * P + L + 1 + 5, 13))
    short, plus5 = fe.encode(x[:, :3 * P]), fe.encode(x[:, :3 * P + 5])
    assert short.shape == plus5.shape == (2, 3, LAT)
    assert torch.equal(short[:, :2], plus5[:, :2])            # 5 more samples: no frame before the last one moves
    assert not torch.equal(short[:, 2], plus5[:, 2])          # the last one saw padding where there is audio now
    full, beyond = fe.encode(x[:, :3 * P + L + 1]), fe.encode(x)
    assert torch.equal(full, beyond)                          # samples past the look-ahead change nothing
    assert torch.equal(full[:, :2], short[:, :2]) and not torch.equal(full[:, 2], plus5[:, 2])


# ---- the model face ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_model_face(tmp_path, monkeypatch, path):
    M = sub("model")
    dt = path[1]
    monkeypatch.setenv("SRWN_ENC_FUSED", path[2])
    dil = [1, 2, 4, 8]
    B, T, pool, lat = 2, 1024, 64, 8
    tol = F32_TOL if dt == torch.float32 else BF16_TOL
    ae = M.WaveNetAutoEncoder(input_size=T, condition_size=0, num_mixtures=5, dilations=dil, latent_channels=lat,
                              skip_channels=128, pool_stride=pool, learning_rate=1e-3, dtype=dt)
    x = O.synthetic_audio(B, T, seed=4)
    ae.train(x)
    want = ae.encode(x)
    enc = ae.encoder(max_batch=3, max_frames=8)
    assert enc._eng.fused == (path[0] == "fused")
    got = enc.encode(x)
    assert got.shape == want.shape == (B, T // pool, lat) and got.dtype == np.float32
    e = rel_err(got, want)
    _note("AudioEncoder.encode vs WaveNetAutoEncoder.encode (%s)" % dt, e)
    assert e < tol, e
    assert set(enc.network_params) == {k for k in ae.network_params if "/Encoder/" in k}
    # a stream through the NumPy face = encode, bit for bit
    s = enc.stream(B)
    parts = [s.push(x[:, :300]), s.push(x[:, 300:301]), s.push(x[:, 301:])]
    assert (s.t, s.frames) == (T, (T - len(dil) - 1) // pool)
    parts.append(s.finish())
    assert s.frames == T // pool and np.array_equal(np.concatenate(parts, axis=1), got)
    with pytest.raises(ValueError, match="closed"):
        s.push(x[:, :1])
    with pytest.raises(ValueError, match="max_batch"):
        enc.encode(np.zeros((4, 100), np.float32))
    # after more training the old snapshot stays, a fresh one follows the new weights
    for _ in range(3):
        ae.train(x)
    want2 = ae.encode(x)
    assert not np.array_equal(want2, want)
    assert np.array_equal(enc.encode(x), got)
    assert rel_err(ae.encoder(max_batch=B).encode(x), want2) < tol
    # save -> AudioEncoder.from_checkpoint, both formats; the decoder's variables in the file are ignored
    for fmt in ("pt", "tf"):
        d = str(tmp_path / fmt)
        assert ae.save(d, 3, force=True, fmt=fmt)
        dep = M.AudioEncoder.from_checkpoint(d, dtype=dt, max_batch=B, max_frames=4)
        assert (dep.num_layers, dep.pool_stride, dep.latent_channels) == (len(dil), pool, lat)
        assert np.array_equal(dep.encode(x), ae.encoder(max_batch=B, max_frames=4).encode(x)), fmt
    with pytest.raises(FileNotFoundError):
        os.makedirs(str(tmp_path / "empty"))
        import json
        json.dump(dict(ae._ctor), open(str(tmp_path / "empty" / "config.json"), "w"))
        M.AudioEncoder.from_checkpoint(str(tmp_path / "empty"), dtype=dt)
    # the chain: a clip of a length the model object was NOT built for -> encoding -> decoder and student
    y = O.synthetic_audio(1, 5 * pool + 3, seed=6)
    ey = enc.encode(y)
    assert ey.shape == (1, 5, lat) and np.isfinite(ey).all()
    audio = ae.generate(ey, seed=1)
    assert audio.shape == (1, 5 * pool) and np.isfinite(audio).all()
    syn = M.StudentSynthesizer(dil, 2, dilation_channels=64, latent_channels=lat, condition_size=0, pool_stride=pool,
                               dtype=dt, max_batch=1, max_chunk=200, max_frames=8)
    out = syn.synthesize(ey, seed=2)
    assert out.shape == (1, 5 * pool, 1) and np.isfinite(out).all()


def test_the_default_path(monkeypatch):
    """Without SRWN_ENC_FUSED: the one-launch chain in bf16 up to the kernel's depth, the twin in fp32 and beyond it."""
    monkeypatch.delenv("SRWN_ENC_FUSED", raising=False)
    E = sub("encoder")
    assert E.ENC_FUSED_DEFAULT == "1"
    for dt, L, fused in ((torch.bfloat16, 3, True), (torch.float32, 3, False), (torch.bfloat16, 33, False)):
        assert E.FrameEncoder(E.EncoderWeights(L, 128, S_, LAT, 2, dt), 32).fused == fused, (dt, L)
