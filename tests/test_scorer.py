"""CPU tests of the streaming likelihood scorer (srwn_version() 116): the two entry points declared, bound, generated and
exported; their argument errors without a GPU; every refusal of the Python classes before any device work; the cut of a
push into steps against brute force; the staging of the delayed audio restated in NumPy against the oracle's RightShift."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import wavenet_np as O
from tests._pkg import ROOT, sub

NEW = ["srwn_stream_score_head", "srwn_nll_rows"]
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


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    raw = open(os.path.join(ROOT, "include", "srwn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n
    assert "srwn_version() 116" in raw
    B = sub("build")
    assert "srwn_score.hip" in B.SOURCES and B.NO_SPILL["srwn_score.hip"] == ["stream_score_head_kernel"]


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_version_and_exports(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 116
    for n in NEW:
        assert callable(getattr(lib, n))


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)

    def head(z=A, zst=2 * 64 * 32, zrows=64, L=3, w2=A, codes=A, nll=A, best=None, lo=None, ostride=64, B=2, n=40, mc=64,
             R=32, S=128, C=256, dt=7):
        # (dt = 7 by default: a call whose other arguments are all good ends at the dtype check, before any launch)
        return lib.srwn_stream_score_head(z, zst, zrows, L, A, A, A, A, w2, A, codes, nll, best, lo, ostride, B, n, mc, R, S,
                                          C, dt, None)

    assert head() == E_DTYPE                       # every other check passed; best and logits_out may be NULL
    assert b"stream_score_head" in lib.srwn_last_error()
    assert head(best=A, lo=A) == E_DTYPE
    for name in ("z", "w2", "codes", "nll"):
        assert head(**{name: None}) == E_NULL, name
    assert head(R=48) == E_UNSUPPORTED
    assert head(S=192) == E_UNSUPPORTED
    assert head(S=64) == E_UNSUPPORTED
    assert head(n=0) == E_SHAPE
    assert head(n=-3) == E_SHAPE
    assert head(n=65) == E_SHAPE                   # a chunk beyond max_chunk
    assert head(B=0) == E_SHAPE
    assert head(C=0) == E_SHAPE
    assert head(C=257) == E_SHAPE
    assert head(C=1) == E_DTYPE and head(C=100) == E_DTYPE
    assert head(zrows=32) == E_SHAPE               # z buffers shorter than max_chunk
    assert head(ostride=39) == E_SHAPE             # outputs shorter than the chunk
    assert head(zst=100) == E_SHAPE
    assert head(L=0) == E_SHAPE
    assert head(mc=0) == E_SHAPE

    def rows(logits=A, ld=128, crows=64, codes=A, nll=A, ostride=64, B=2, n=40, C=100):
        return lib.srwn_nll_rows(logits, ld, crows, codes, nll, None, None, ostride, B, n, C, None)

    for name in ("logits", "codes", "nll"):
        assert rows(**{name: None}) == E_NULL, name
    assert b"nll_rows" in lib.srwn_last_error()
    assert rows(n=0) == E_SHAPE
    assert rows(B=0) == E_SHAPE
    assert rows(C=0) == E_SHAPE
    assert rows(C=257, ld=512) == E_SHAPE
    assert rows(ld=96) == E_SHAPE                  # rows shorter than the classes
    assert rows(crows=39) == E_SHAPE
    assert rows(ostride=39) == E_SHAPE


# ---- refusals, before any device work ----------------------------------------------------------------------------------
def test_weights_refuse_first():
    S = sub("scorer")
    cfg = dict(head_mode="per_timestep", gate_mode="reference", shift_input=True, cond_channels=0)
    eng = lambda **kw: SimpleNamespace(cfg=SimpleNamespace(**dict(cfg, **kw)))
    with pytest.raises(ValueError, match="per_timestep"):
        S.ScorerWeights.from_engine(eng(head_mode="pooled"))
    with pytest.raises(ValueError, match="per_timestep"):
        S.ScorerWeights.from_engine(eng(head_mode="contrastive"))
    with pytest.raises(NotImplementedError, match="mixture-of-logistics"):
        S.ScorerWeights.from_engine(eng(head_mode="mol"))
    with pytest.raises(ValueError, match="RightShift"):
        S.ScorerWeights.from_engine(eng(shift_input=False))
    with pytest.raises(NotImplementedError, match="conditioned"):
        S.ScorerWeights.from_engine(eng(cond_channels=20))
    with pytest.raises(NotImplementedError, match="wavenet"):
        S.ScorerWeights.from_engine(eng(gate_mode="wavenet"))
    for r, s in ((48, 256), (128, 256), (32, 192), (64, 64)):
        with pytest.raises(NotImplementedError, match="streaming scorer.*built for"):
            S.ScorerWeights([1, 2], r, s, 256)
    with pytest.raises(NotImplementedError, match="filter_width"):
        S.ScorerWeights([1, 2], 32, 128, 256, filter_width=3)
    with pytest.raises(NotImplementedError, match="output_channels"):
        S.ScorerWeights([1, 2], 32, 128, 300)
    with pytest.raises(ValueError, match="dilations"):
        S.ScorerWeights([1, 0], 32, 128, 256)
    R = sub("recognizer")
    assert issubclass(S.ScorerWeights, R.StackWeights) and issubclass(R.ClassifierWeights, R.StackWeights)


def test_scorer_refuses_first():
    S = sub("scorer")
    with pytest.raises(ValueError, match="max_chunk"):
        S.StreamScorer(None, max_batch=1, max_chunk=0)
    with pytest.raises(ValueError, match="max_chunk"):
        S.StreamScorer(None, max_batch=1, max_chunk=-5)
    with pytest.raises(ValueError, match="max_batch"):
        S.StreamScorer(None, max_batch=0, max_chunk=16)
    c = _bare(S.StreamScorer, max_batch=2, _state=None, _serial=0)
    with pytest.raises(ValueError, match="max_batch"):
        c.start(3)
    with pytest.raises(ValueError, match="max_batch"):
        c.start(0)
    with pytest.raises(ValueError, match="max_batch"):
        c.score(np.zeros((3, 10), np.float32))
    for bad in (np.zeros(10, np.float32), np.zeros((1, 2, 10), np.float32)):
        with pytest.raises(ValueError, match=r"\[batch, samples\]"):
            c.score(bad)
    st = _bare(S.ScoreState, B=2, _serial=1, t=0)
    c._state, c._serial = st, 1
    with pytest.raises(ValueError, match="streams"):
        c.push(st, np.zeros((1, 10), np.float32))
    with pytest.raises(ValueError, match=r"\[batch, samples\]"):
        c.push(st, np.zeros(10, np.float32))
    with pytest.raises(ValueError, match="current"):                     # a stale state: start() began another
        c.push(_bare(S.ScoreState, B=2, _serial=0, t=0), np.zeros((2, 10), np.float32))
    assert st.t == 0                                                     # refusals leave the state untouched


def test_models_refuse_first():
    M = sub("model")
    cfg = dict(head_mode="per_timestep", gate_mode="reference", shift_input=True, cond_channels=0, filter_width=2,
               dilation_channels=32, skip_channels=128)
    teacher = lambda **kw: _bare(M.WaveNetTeacher, _cfg=SimpleNamespace(**dict(cfg, **kw)), _primary=None)
    with pytest.raises(NotImplementedError, match="mixture-of-logistics"):
        teacher(head_mode="mol").scorer()
    with pytest.raises(NotImplementedError, match="conditioned"):
        teacher(cond_channels=16).scorer()
    with pytest.raises(NotImplementedError, match="wavenet"):
        teacher(gate_mode="wavenet").scorer()
    with pytest.raises(NotImplementedError, match="filter_width"):
        teacher(filter_width=3).scorer()
    with pytest.raises(NotImplementedError, match="built for"):
        teacher(skip_channels=64).scorer()
    with pytest.raises(FileNotFoundError, match="config.json"):
        M.StreamingScorer.from_checkpoint("/nonexistent")
    for name in ("StreamingScorer", "ScorerStream"):
        assert isinstance(getattr(M, name), type)


def test_from_checkpoint_refuses_by_config(tmp_path):
    import json
    M = sub("model")
    ctor = dict(input_size=64, condition_size=0, dilations=[1, 2], filter_width=2, dilation_channels=32, skip_channels=128,
                quantization_channels=256, latent_channels=16, pool_stride=512, name="WaveNetTeacher", learning_rate=1e-3,
                use_encoding=False, seed=0, head="softmax", num_mixtures=5, gate_mode="reference")
    for change, err, match in ((dict(head="mol"), NotImplementedError, "mixture-of-logistics"),
                               (dict(use_encoding=True), NotImplementedError, "conditioned"),
                               (dict(gate_mode="wavenet"), NotImplementedError, "wavenet"),
                               (dict(dilation_channels=48), NotImplementedError, "built for")):
        with open(tmp_path / "config.json", "w") as f:
            json.dump(dict(ctor, **change), f)
        with pytest.raises(err, match=match):
            M.StreamingScorer.from_checkpoint(str(tmp_path))


# ---- the cut of a push -------------------------------------------------------------------------------------------------
def test_cut_push_against_brute_force():
    S = sub("scorer")
    for mc in (1, 2, 3, 7, 32, 128, 1600):
        for n in list(range(0, 3 * min(mc, 40) + 3)) + [mc - 1, mc, mc + 1, 2 * mc, 5 * mc + 3]:
            if n < 0:
                continue
            steps = S.cut_push(n, mc)
            owner = []                     # brute force: sample i belongs to step i // mc, at row i % mc
            for k, (a, rows) in enumerate(steps):
                assert 1 <= rows <= mc
                owner += [(k, r) for r in range(rows)]
                assert a == k * mc
            assert owner == [(i // mc, i % mc) for i in range(n)], (n, mc)
            assert all(rows == mc for _, rows in steps[:-1])
    assert S.cut_push(0, 5) == []
    with pytest.raises(ValueError):
        S.cut_push(-1, 5)
    with pytest.raises(ValueError):
        S.cut_push(5, 0)


def test_bits_per_sample_helper():
    S = sub("scorer")
    assert abs(S.bits_per_sample(np.log(256.0) * 10, 10) - 8.0) < 1e-12
    assert np.isnan(S.bits_per_sample(0.0, 0))


# ---- the delayed staging is the RightShift -------------------------------------------------------------------------------
def test_delayed_staging_is_the_right_shift():
    """What a push stages, restated in NumPy: x'[0] = the sample before the chunk (0 at the start), x'[1:n] = chunk[:n-1],
    the entry conv's x[-1] = the carry (the last staged sample of the chunk before).  Row t of the plain K = 2 conv on that
    stream is the oracle's input conv of the RightShifted audio: b + w0 a[t-2] + w1 a[t-1]."""
    S = sub("scorer")
    sp = O.init_stack_params(2, [1], 2, 8, 16, 6, bias_scale=0.1)
    audio = O.synthetic_audio(1, 61, seed=5).astype(np.float64)[0]
    want = O.dilated_causal_conv1d_bias(O.right_shift(audio[None, :, None]), sp.init_w, sp.init_b, 1)[0]
    got, last, carry, at = [], 0.0, 0.0, 0
    for n in (1, 1, 2, 7, 16, 3, 31):
        for a, rows in S.cut_push(n, 5):
            chunk = audio[at + a:at + a + rows]
            x = np.concatenate([[last], chunk[:-1]])
            for t in range(rows):
                x0 = x[t - 1] if t >= 1 else carry
                got.append(sp.init_b + x0 * sp.init_w[0, 0] + x[t] * sp.init_w[1, 0])
            last, carry = chunk[-1], x[-1]
        at += n
    assert at == 61
    assert np.abs(np.array(got) - want).max() < 1e-14
