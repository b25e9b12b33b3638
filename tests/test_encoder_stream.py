"""CPU tests of the standalone streaming encoder: the C-ABI of srwn_nc_encode_frames, the windowing scheme restated on
the fp64 oracle and driven by the product's own planning helper (encoder.plan_frames), and the refusals that come before
any device work."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import wavenet_np as O
from tests._pkg import ROOT, sub


# ---- C-ABI -------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_listed_and_bound_by_both_bindings():
    L = sub("_lib")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    for name in ("srwn_nc_encode_frames", "srwn_nc_encode_partials", "srwn_nc_encode_max_layers"):
        assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared in srwn.h"
        assert name in L.SIGNATURES
        for binding in ("pybind11", "ctypes"):
            assert callable(getattr(L.bind(binding), name)), (binding, name)
    assert L.load().srwn_version() >= 109
    B = sub("build")
    assert "srwn_ncstream.hip" in B.SOURCES and "nc_encode_frames_kernel" in B.NO_SPILL["srwn_ncstream.hip"]


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    L = sub("_lib")
    lib = L.bind(binding)
    names = ["x", "ld", "nc_w", "nc_b", "nc_wr", "nc_br", "wconv", "wconv_stride", "wres", "wres_stride", "bias_c", "bias_r",
             "partials", "means", "B", "nframes", "pool", "valid", "L", "C", "K", "dtype", "stream"]
    ok = dict(x=1, ld=600, nc_w=1, nc_b=1, nc_wr=1, nc_br=1, wconv=1, wconv_stride=49152, wres=1, wres_stride=49152,
              bias_c=1, bias_r=1, partials=1, means=1, B=2, nframes=1, pool=512, valid=543, L=30, C=128, K=2,
              dtype=L.BF16, stream=None)
    run = lambda **kw: lib.srwn_nc_encode_frames(*[dict(ok, **kw)[n] for n in names])
    assert run(B=0) == 0 and run(nframes=0) == 0                  # empty work returns before any launch
    for p in ("x", "nc_w", "nc_b", "nc_wr", "nc_br", "wconv", "wres", "bias_c", "bias_r", "partials", "means"):
        assert run(**{p: None}) == -3, p
        assert b"null" in lib.srwn_last_error()
    assert run(C=64) == -4 and run(K=3) == -4                     # widths the kernel is not built for
    assert run(dtype=L.F32) == -4                                 # fp32: the layer-by-layer path
    assert run(dtype=7) == -1
    assert run(valid=511) == -2                                   # fewer samples than the frames hold
    assert run(valid=512 + 30 + 2) == -2                          # more than the frames can see
    assert run(valid=543, ld=542) == -2                           # rows shorter than the window
    assert run(L=33, valid=512) == -2 and run(L=0, valid=512) == -2
    assert b"layers" in lib.srwn_last_error()
    assert run(pool=0) == -2
    assert lib.srwn_nc_encode_max_layers() == 32
    assert lib.srwn_nc_encode_partials(2, 32, 512, 30) == 6 * 30 * 2 * 32 * 128       # ceil(512 / 96) segments


# ---- the windowing scheme on the fp64 oracle -----------------------------------------------------------------------------
def _chunkings(rng, T, P):
    """A random cut of T samples: 0- and 1-sample chunks, ordinary ones, and one long enough for several frames."""
    sizes, left = [0], T
    for n in (1, 2 * P + int(rng.integers(1, P + 1))):
        n = min(n, left)
        sizes.append(n)
        left -= n
    while left > 0:
        n = min(left, int(rng.choice([0, 1, rng.integers(2, P + 2), rng.integers(P, 3 * P + 1)])))
        sizes.append(n)
        left -= n
    rng.shuffle(sizes)
    return [int(n) for n in sizes]


@pytest.mark.parametrize("L", [1, 5, 30])
@pytest.mark.parametrize("P", [16, 25, 128])
def test_windows_reproduce_the_whole_clip(L, P):
    E = sub("encoder")
    rng = np.random.default_rng(1000 * L + P)
    ep = O.init_encoder_params(7 + L, L, 2, 8, 8, 4, bias_scale=0.05)
    for T in (4 * P, 4 * P + 7, 3 * P + L + 1, P - 1, P):
        clip = rng.uniform(-1, 1, size=(2, T))
        whole = O.encoder_forward(ep, clip, P)
        for trial in range(4):
            sizes = _chunkings(rng, T, P) if trial < 3 else [0, 1, T - 1]      # (the last: nearly everything at once)
            max_frames = [None, 1, 2, None][trial]
            received = emitted = 0
            outs, several = [], False
            for n in sizes:
                received += n
                plans = E.plan_frames(received, emitted, L, P, False, max_frames)
                several |= sum(p[1] for p in plans) > 1
                for (f0, k, start, valid) in plans:
                    assert f0 == emitted and start == f0 * P
                    assert (f0 + k) * P + L + 1 <= received, "a frame was emitted before its look-ahead was in"
                    assert valid == k * P + L + 1
                    assert max_frames is None or k <= max_frames
                    outs.append(O.encoder_forward(ep, clip[:, start:start + valid], P)[:, :k])
                    emitted += k
                assert emitted == max(0, (received - L - 1) // P), "a frame whose look-ahead is in was held back"
                assert received - emitted * P < P + L + 1      # what a stream keeps
            assert received == T
            plans = E.plan_frames(received, emitted, L, P, True, max_frames)
            assert sum(p[1] for p in plans) == T // P - emitted
            for (f0, k, start, valid) in plans:
                assert f0 == emitted and k * P <= valid <= k * P + L + 1 and start + valid <= T
                outs.append(O.encoder_forward(ep, clip[:, start:start + valid], P)[:, :k])
                emitted += k
            assert emitted == T // P
            got = np.concatenate(outs, axis=1) if outs else np.zeros((2, 0, 4))
            assert got.shape == whole.shape
            if whole.size:
                assert np.abs(got - whole).max() <= 1e-12
            if trial == 3 and (T - L - 1) // P >= 2:
                assert several, "no chunk completed several frames at once"


def test_the_look_ahead_bound_is_tight():
    """Frame f needs the samples up to (f+1) P + L + 1: one sample fewer changes it (so nothing may be emitted earlier),
    and nothing before f P matters (so a stream needs no look-back)."""
    E = sub("encoder")
    L, P, T = 5, 16, 200
    ep = O.init_encoder_params(3, L, 2, 8, 8, 4, bias_scale=0.05)
    clip = np.random.default_rng(0).uniform(-1, 1, size=(1, T))
    whole = O.encoder_forward(ep, clip, P)
    f = 4
    need = (f + 1) * P + L + 1
    assert np.abs(O.encoder_forward(ep, clip[:, :need], P)[:, :f + 1] - whole[:, :f + 1]).max() <= 1e-12
    assert np.abs(O.encoder_forward(ep, clip[:, :need - 1], P)[:, f] - whole[:, f]).max() > 1e-9
    assert np.abs(O.encoder_forward(ep, clip[:, 2 * P:need], P)[:, :f - 1] - whole[:, 2:f + 1]).max() <= 1e-12
    assert E.plan_frames(need, 0, L, P) == [(0, f + 1, 0, need)]
    assert E.plan_frames(need - 1, 0, L, P) == [(0, f, 0, f * P + L + 1)]
    assert E.plan_frames(L + 1 + P - 1, 0, L, P) == [] and E.plan_frames(0, 0, L, P, True) == []
    assert E.plan_frames(P - 1, 0, L, P, True) == []                     # T < P: no frame
    assert E.plan_frames(3 * P + 2, 1, L, P, True, 32) == [(1, 2, P, 2 * P + 2)]
    for bad in (dict(received=-1), dict(emitted=-1), dict(pool_stride=0), dict(emitted=20), dict(max_frames=0)):
        with pytest.raises(ValueError):
            E.plan_frames(**dict(dict(received=100, emitted=0, nlayers=L, pool_stride=P), **bad))


# ---- refusals come first -------------------------------------------------------------------------------------------------
def _bare(cls, **attrs):
    """An object without its device state (constructing one needs a GPU): what the refusals check first."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_frame_encoder_refuses_first():
    E = sub("encoder")
    with pytest.raises(NotImplementedError, match="128"):
        E.FrameEncoder(SimpleNamespace(EC=64, Kw=2), 16)
    with pytest.raises(NotImplementedError, match="filter_width"):
        E.FrameEncoder(SimpleNamespace(EC=128, Kw=3), 16)
    with pytest.raises(ValueError, match="max_batch"):
        E.FrameEncoder(SimpleNamespace(EC=128, Kw=2), 16, max_batch=0)
    with pytest.raises(NotImplementedError, match="128"):
        E.EncoderWeights(5, encoder_channels=64)
    with pytest.raises(NotImplementedError, match="filter_width"):
        E.EncoderWeights(5, filter_width=3)
    fe = _bare(E.FrameEncoder, max_batch=2, max_frames=4, P=16, L=5, lat=4, w=None)
    other = _bare(E.FrameEncoder, max_batch=2, max_frames=4, P=16, L=5, lat=4, w=None)
    with pytest.raises(ValueError, match="max_batch"):
        fe.encode(np.zeros((3, 100), np.float32))
    with pytest.raises(ValueError, match="batch, samples"):
        fe.encode(np.zeros(100, np.float32))
    with pytest.raises(ValueError, match="max_batch"):
        fe.start(3)
    st = E.EncoderStreamState(fe, 2, None)
    for bad in (E.EncoderStreamState(other, 2, None), object(), None):
        with pytest.raises(ValueError, match="not started by this encoder"):
            fe.push(bad, np.zeros((2, 10), np.float32))
    with pytest.raises(ValueError, match="2"):
        fe.push(st, np.zeros((1, 10), np.float32))                # one stream into a state of two
    with pytest.raises(ValueError, match="batch, samples"):
        fe.push(st, np.zeros((2, 10, 1), np.float32))
    with pytest.raises(ValueError, match="floating"):
        fe.push(st, __import__("torch").zeros((2, 10), dtype=__import__("torch").int32))
    assert (st.received, st.emitted, st.closed, st.tail) == (0, 0, False, None)      # untouched
    st.closed = True
    for call in (lambda: fe.push(st, np.zeros((2, 10), np.float32)), lambda: fe.finish(st)):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_audio_encoder_refuses_first_and_has_no_cpu_fallback():
    import torch
    M = sub("model")
    with pytest.raises(NotImplementedError, match="128"):
        M.AudioEncoder(5, encoder_channels=64)
    with pytest.raises(NotImplementedError, match="filter_width"):
        M.AudioEncoder(5, filter_width=3)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.AudioEncoder(5)
    a = _bare(M.AudioEncoder, max_batch=2, _eng=None)
    with pytest.raises(ValueError, match="max_batch"):
        a.encode(np.zeros((3, 50)))
    with pytest.raises(ValueError, match="batch, samples"):
        a.encode(np.zeros(50))
    with pytest.raises(ValueError, match="max_batch"):
        a.stream(3)
    s = _bare(M.EncoderStream, _owner=a, batch_size=2, _st=SimpleNamespace(closed=False, received=7, emitted=0))
    assert (s.t, s.frames) == (7, 0)
    with pytest.raises(ValueError, match="streams"):
        s.push(np.zeros((1, 10)))
    s._st.closed = True
    with pytest.raises(ValueError, match="closed"):
        s.push(np.zeros((2, 10)))
    assert hasattr(M.WaveNetAutoEncoder, "encoder")
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dropin_model", os.path.join(ROOT, "sr-wavenet_amd", "dropin", "model.py"))
    d = importlib.util.module_from_spec(spec); spec.loader.exec_module(d)
    assert d.AudioEncoder is M.AudioEncoder


# ---- the default path ---------------------------------------------------------------------------------------------------
def test_the_default_path_is_the_measured_one_and_the_documents_say_so():
    """The one-launch chain is the bf16 default because tools/encode_bench.py measured it ahead of the twin at B = 1,
    pool 512; the code, the README's knob table and the README's results block state the same default."""
    E = sub("encoder")
    assert E.ENC_FUSED_DEFAULT == "1"
    readme = open(os.path.join(ROOT, "README.md")).read()
    row = re.search(r"^\| `SRWN_ENC_FUSED` \| `([01])` \|", readme, flags=re.M)
    assert row and row.group(1) == E.ENC_FUSED_DEFAULT
    assert "has not been run" not in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Not measured in this change" not in design and "has not been run on the card" not in design
