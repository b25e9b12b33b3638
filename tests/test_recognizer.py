"""CPU tests of the streaming classifier (srwn_version() 113): the emission arithmetic against brute force; the hop-sum
scheme restated in NumPy on the fp64 oracle against the sliding AVG pool of the reference graph; every refusal, before any
device work; the new entry points declared, bound, generated and exported."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import wavenet_np as O
from tests._pkg import ROOT, sub

NEW = ["srwn_recog_stream_in", "srwn_residual_group_fwd_stream_z", "srwn_pooled_stream_head", "srwn_hop_sum",
       "srwn_window_mean", "srwn_recog_roll"]
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _lib(binding):
    L = sub("_lib")
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "sr-wavenet_amd", "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.build()
    return L.bind(binding)


def _bare(cls, **attrs):
    """An object without its device state (constructing one needs a GPU): what the checks read first."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


# ---- emission arithmetic ---------------------------------------------------------------------------------------------
def test_emissions_due_against_brute_force():
    R = sub("recognizer")
    for hop, window in ((1, 1), (1, 5), (3, 3), (3, 12), (40, 320), (32, 128), (7, 7)):
        def brute(t):      # emissions a stream holding t samples owes in all: hops j whose window lies in [0, t)
            return [j for j in range(t // hop + 2) if (j + 1) * hop <= t and (j + 1) * hop - window >= 0]
        for t0 in range(0, 3 * window + 2 * hop, max(1, hop // 3)):
            for dt in (0, 1, hop - 1, hop, hop + 1, 2 * hop + 1, window, window + hop):
                first, count = R.emissions_due(t0, t0 + dt, hop, window)
                want = [j for j in brute(t0 + dt) if j not in brute(t0)]
                assert count == len(want), (hop, window, t0, dt)
                if want:
                    assert list(range(first, first + count)) == want, (hop, window, t0, dt)
    with pytest.raises(ValueError):
        R.emissions_due(5, 4, 1, 1)
    with pytest.raises(ValueError):
        R.emissions_due(0, 4, 3, 10)
    with pytest.raises(ValueError):
        R.emissions_due(0, 4, 0, 10)


# ---- the scheme on the oracle ------------------------------------------------------------------------------------------
def _scheme(r1, hop, window, ring_rows, w2, b2, chunks):
    """The device scheme in fp64: hop sums by 32-row tiles in time order into a ring of `ring_rows` rows, chunk by
    chunk (hops per chunk from `chunks`, cycled); per chunk first every hop sum, then the chunk's window means."""
    T, S = r1.shape
    nW = window // hop
    ring = np.zeros((ring_rows, S))
    out = []
    j, ci = 0, 0
    while (j + 1) * hop <= T:
        k = min(chunks[ci % len(chunks)], T // hop - j)
        ci += 1
        assert ring_rows >= nW + k - 1
        for i in range(k):
            h = np.zeros(S)
            for t0 in range(0, hop, 32):
                h = h + r1[(j + i) * hop + t0:(j + i) * hop + min(t0 + 32, hop)].sum(0)
            ring[(j + i) % ring_rows] = h
        for i in range(k):
            if j + i >= nW - 1:
                m = np.zeros(S)
                for w in range(nW):
                    m = m + ring[(j + i - nW + 1 + w) % ring_rows]
                out.append((m / window) @ w2 + b2)
        j += k
    return np.array(out)


@pytest.mark.parametrize("hop,window,chunks", [(40, 320, (3, 1, 2)), (12, 48, (1,)), (32, 128, (4,)), (5, 5, (2, 3)),
                                               (1, 7, (3,))])
def test_hop_sum_scheme_is_the_sliding_pool(hop, window, chunks):
    dil = [1, 2, 4, 8, 1, 2]
    sp = O.init_stack_params(5, dil, 2, 8, 16, 6, bias_scale=0.1)
    T = 3 * window + 2 * hop + 3      # more hops than ring rows; a tail that fills no hop
    audio = O.synthetic_audio(2, T, seed=3).astype(np.float64)
    logits, cache = O.stack_forward(sp, audio)
    nW = window // hop
    ring_rows = nW + max(chunks) - 1
    assert T // hop > ring_rows
    for b in range(2):
        got = _scheme(cache["r1"][b], hop, window, ring_rows, sp.head_w2, sp.head_b2, chunks)
        pos = [(j + 1) * hop - window for j in range(nW - 1, T // hop)]
        want = np.array([logits[b, p:p + window].mean(0) for p in pos])      # tf.nn.pool AVG VALID stride 1 at `pos`
        assert got.shape == want.shape == (T // hop - nW + 1, 6)
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())


# ---- refusals, before any device work ----------------------------------------------------------------------------------
def test_classifier_refuses_first():
    R = sub("recognizer")
    with pytest.raises(ValueError, match="multiple of hop"):
        R.StreamClassifier(None, max_batch=1, hop=48, window=100)
    with pytest.raises(ValueError, match="multiple of hop"):
        R.StreamClassifier(None, max_batch=1, hop=64, window=32)
    for hop in (0, -160):
        with pytest.raises(ValueError, match="hop"):
            R.StreamClassifier(None, max_batch=1, hop=hop, window=160)
    with pytest.raises(ValueError, match="max_batch"):
        R.StreamClassifier(None, max_batch=0, hop=16, window=32)
    with pytest.raises(ValueError, match="max_hops"):
        R.StreamClassifier(None, max_batch=1, hop=16, window=32, max_hops=0)
    c = _bare(R.StreamClassifier, max_batch=2, _state=None, _serial=0)
    with pytest.raises(ValueError, match="max_batch"):
        c.start(3)
    with pytest.raises(ValueError, match="max_batch"):
        c.start(0)
    with pytest.raises(ValueError, match="max_batch"):
        c.classify(np.zeros((3, 10), np.float32))
    for bad in (np.zeros(10, np.float32), np.zeros((1, 2, 10), np.float32)):
        with pytest.raises(ValueError, match=r"\[batch, samples\]"):
            c.classify(bad)
    st = R.RecogState(2, 1, None)
    c._state, c._serial = st, 1
    with pytest.raises(ValueError, match="streams"):
        c.push(st, np.zeros((1, 10), np.float32))
    with pytest.raises(ValueError, match=r"\[batch, samples\]"):
        c.push(st, np.zeros(10, np.float32))
    with pytest.raises(ValueError, match="current"):
        c.push(R.RecogState(2, 0, None), np.zeros((2, 10), np.float32))
    assert (st.t, st.emitted) == (0, 0)                                  # refusals leave the state untouched


def test_weights_refuse_first():
    R = sub("recognizer")
    for r, s in ((48, 256), (128, 256), (32, 192), (64, 64), (16, 128)):
        with pytest.raises(NotImplementedError, match="built for"):
            R.ClassifierWeights([1, 2], r, s, 12)
    with pytest.raises(NotImplementedError, match="filter_width"):
        R.ClassifierWeights([1, 2], 32, 128, 12, filter_width=3)
    with pytest.raises(NotImplementedError, match="output_channels"):
        R.ClassifierWeights([1, 2], 32, 128, 300)
    with pytest.raises(ValueError, match="dilations"):
        R.ClassifierWeights([1, 0], 32, 128, 12)
    cfg = dict(head_mode="pooled", gate_mode="reference", shift_input=False, cond_channels=0)
    with pytest.raises(ValueError, match="pooled"):
        R.ClassifierWeights.from_engine(SimpleNamespace(cfg=SimpleNamespace(**dict(cfg, head_mode="per_timestep"))))
    with pytest.raises(ValueError, match="pooled"):
        R.ClassifierWeights.from_engine(SimpleNamespace(cfg=SimpleNamespace(**dict(cfg, head_mode="contrastive"))))
    with pytest.raises(NotImplementedError, match="wavenet"):
        R.ClassifierWeights.from_engine(SimpleNamespace(cfg=SimpleNamespace(**dict(cfg, gate_mode="wavenet"))))
    with pytest.raises(ValueError, match="RightShift"):
        R.ClassifierWeights.from_engine(SimpleNamespace(cfg=SimpleNamespace(**dict(cfg, shift_input=True))))


def test_models_refuse_first():
    M = sub("model")
    ok = dict(input_size=128, filter_width=2, dilation_channels=32, skip_channels=128, gate_mode="reference", _primary=None)
    with pytest.raises(ValueError, match="multiple of hop"):
        _bare(M.WaveNet, **ok).recognizer(hop=48)
    with pytest.raises(ValueError, match="hop"):
        _bare(M.WaveNet, **ok).recognizer(hop=0)
    with pytest.raises(NotImplementedError, match="wavenet"):
        _bare(M.WaveNet, **dict(ok, gate_mode="wavenet")).recognizer()
    with pytest.raises(NotImplementedError, match="filter_width"):
        _bare(M.WaveNet, **dict(ok, filter_width=3)).recognizer()
    with pytest.raises(NotImplementedError, match="built for"):
        _bare(M.WaveNet, **dict(ok, skip_channels=64)).recognizer()
    with pytest.raises(NotImplementedError, match="built for"):
        M.StreamingClassifier.from_checkpoint("/nonexistent", [1, 2], 12, dilation_channels=48)
    with pytest.raises(ValueError, match="multiple of hop"):
        M.StreamingClassifier.from_checkpoint("/nonexistent", [1, 2], 12, hop=7, window=16)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n
    # the z form is the stream form plus (z_out, z_layer_stride) after out_hist
    a0, a1 = L.SIGNATURES["srwn_residual_group_fwd_stream"][1], L.SIGNATURES["srwn_residual_group_fwd_stream_z"][1]
    assert list(a1) == list(a0[:5]) + [L._p, L._i64] + list(a0[5:])
    assert "model.py:33-62" in open(os.path.join(ROOT, "include", "srwn.h")).read()


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_version_and_exports(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 113
    for n in NEW:
        assert callable(getattr(lib, n))


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)

    def head(z=A, zst=2 * 64 * 32, zrows=64, L=3, ring=A, rr=5, clock=A, B=2, k=2, hop=32, mc=64, R=32, S=128, dt=1):
        return lib.srwn_pooled_stream_head(z, zst, zrows, L, A, A, A, A, ring, rr, clock, B, k, hop, mc, R, S, dt, None)

    assert head(z=None) == E_NULL
    assert head(clock=None) == E_NULL
    assert head(R=48) == E_UNSUPPORTED
    assert head(S=192) == E_UNSUPPORTED
    assert head(k=3) == E_SHAPE                    # 3 hops of 32 rows in a chunk buffer of 64
    assert head(zrows=32) == E_SHAPE
    assert head(zst=100) == E_SHAPE
    assert head(L=0) == E_SHAPE
    assert head(dt=7) == E_DTYPE
    assert b"pooled_stream_head" in lib.srwn_last_error()

    def wmean(ring=A, rr=5, mean=A, clock=A, B=2, k=2, hop=32, window=128, S=128, logits=None, w2=None):
        return lib.srwn_window_mean(ring, rr, mean, clock, B, k, hop, window, S, w2, w2, logits, 12, 32, None)

    assert wmean(ring=None) == E_NULL
    assert wmean(logits=A) == E_NULL               # logits without the last 1x1
    assert wmean(window=100) == E_SHAPE            # not a multiple of hop
    assert wmean(hop=0) == E_SHAPE
    assert wmean(rr=4) == E_SHAPE                  # 4 window rows + 2 hops per launch - 1 = 5
    assert wmean(S=512) == E_SHAPE

    def hsum(r1=A, rows=64, k=2, hop=32, mc=64, S=128, dt=1):
        return lib.srwn_hop_sum(r1, rows, A, 5, A, 2, k, hop, mc, S, dt, None)

    assert hsum(r1=None) == E_NULL
    assert hsum(k=3) == E_SHAPE
    assert hsum(S=7) == E_SHAPE
    assert hsum(dt=7) == E_DTYPE

    def entry(x=A, stride=64, rows=31 + 64, hist=31, n=40, mc=64, R=32, dt=1):
        return lib.srwn_recog_stream_in(x, stride, A, A, A, A, rows, hist, 2, n, mc, R, dt, None)

    assert entry(x=None) == E_NULL
    assert entry(R=48) == E_UNSUPPORTED
    assert entry(n=65) == E_SHAPE
    assert entry(n=0) == E_SHAPE
    assert entry(rows=64) == E_SHAPE
    assert entry(stride=40) == E_SHAPE
    assert entry(dt=7) == E_DTYPE

    def roll(table=A, n=40, mc=64, R=32, dt=1, clock=A):
        return lib.srwn_recog_roll(table, 2, A, 64, A, clock, 2, n, mc, R, dt, None)

    assert roll(table=None) == E_NULL
    assert roll(clock=None) == E_NULL
    assert roll(R=16) == E_UNSUPPORTED
    assert roll(n=65) == E_SHAPE
    assert roll(dt=7) == E_DTYPE

    import ctypes as C
    d = (C.c_int32 * 2)(1, 2)
    ptrs = (C.c_void_p * 2)(A, A)

    def group(z=A, zst=2 * 64 * 64, n=40, R=32):
        return lib.srwn_residual_group_fwd_stream_z(A, 3 + 64, A, 64, 0, z, zst, ptrs, ptrs, ptrs, ptrs, None, 1, 1, R, d, 2, 2,
                                                    n, 64, R, 2, 1, A, None)

    assert group(z=None) == E_NULL
    assert group(zst=100) == E_SHAPE
    assert group(n=65) == E_SHAPE
    assert group(R=48) == E_UNSUPPORTED
