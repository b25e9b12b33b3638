"""CPU tests of resumable generation (srwn_version() 104): the resume entry points and the ring fill are exported and
bound, their argument errors come back as negative codes without a GPU, and the model classes refuse a wrongly shaped
prompt and the canonical gate before any device work."""
import os
import re

import numpy as np
import pytest

from tests._pkg import ROOT, sub

NEW = ["srwn_generate_resume", "srwn_generate_mol_resume", "srwn_generate16_resume", "srwn_generate16_mol_resume",
       "srwn_generate_ring_fill"]
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _lib(binding):
    L = sub("_lib")
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "sr-wavenet_amd", "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.build()
    return L.bind(binding)


def test_new_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n
    # each resume form is its one-shot entry point's argument list plus (int32 t0, float* carry)
    for base in ("srwn_generate", "srwn_generate_mol", "srwn_generate16", "srwn_generate16_mol"):
        r0, a0 = L.SIGNATURES[base]
        r1, a1 = L.SIGNATURES[base + "_resume"]
        assert r0 is r1 and list(a1) == list(a0) + [L._i32, L._p], base


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_version_and_exports(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 104
    for n in NEW:
        assert callable(getattr(lib, n))


def _dl(dils):
    import ctypes as C
    return (C.c_int32 * len(dils))(*dils)


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_ring_fill_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    d = _dl([1, 2, 4])
    BF16, F32 = 1, 0

    def fill(xs=A, stride=2 * 10 * 64, T=10, P=5, dil=d, L=3, B=2, R=64, ring=A, dtype=BF16):
        return lib.srwn_generate_ring_fill(xs, stride, T, P, dil, L, B, R, ring, dtype, None)

    assert fill(B=0) == 0                                  # empty work, no launch
    assert fill(ring=None) == E_NULL
    assert fill(xs=None) == E_NULL                         # a prompt needs its layer inputs
    assert fill(dil=None) == E_NULL
    assert fill(P=-1) == E_SHAPE
    assert fill(P=11) == E_SHAPE                           # T_src < P
    assert fill(L=0) == E_SHAPE
    assert fill(L=65, dil=_dl([1] * 65)) == E_SHAPE
    assert fill(dil=_dl([1, 0, 4])) == E_SHAPE
    assert fill(R=48) == E_UNSUPPORTED
    assert fill(dtype=7) == E_DTYPE
    assert fill(stride=2 * 10 * 64 + 1) == E_SHAPE         # layer rows must stay 16-byte aligned
    assert fill(xs=A + 2) == E_SHAPE
    assert fill(dtype=F32, stride=2 * 10 * 64 - 4) == E_SHAPE   # layers would overlap
    msg = lib.srwn_last_error()
    assert msg and b"ring_fill" in msg


def _gen_args(which, t0, carry, B=2, R=64, S=256, L=2, dil=None, ring=A, nsteps=4, C=256):
    d = dil if dil is not None else _dl([1, 2])
    common = [A] * 11 + [ring, A, A, None, None, d, L, B, nsteps, nsteps, R, S]
    if which == "srwn_generate_resume":
        return common[:0] + [A] * 4 + common[4:] + [C, 2, 0, 0, 1, None, t0, carry]
    if which == "srwn_generate_mol_resume":
        return [A] * 4 + common[4:] + [2, 5, None, 1, 1, 0, 0, 0, 1, None, t0, carry]
    if which == "srwn_generate16_resume":
        return [A] * 3 + common[4:] + [C, 0, 0, None, t0, carry]
    return [A] * 3 + common[4:] + [5, None, 1, 1, 0, 0, 0, None, t0, carry]


RESUME = ["srwn_generate_resume", "srwn_generate_mol_resume", "srwn_generate16_resume", "srwn_generate16_mol_resume"]


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
@pytest.mark.parametrize("which", RESUME)
def test_resume_argument_errors_do_not_need_a_gpu(binding, which):
    lib = _lib(binding)
    f = getattr(lib, which)
    assert f(*_gen_args(which, -1, A)) == E_SHAPE                      # t0 < 0
    assert f(*_gen_args(which, 5, None)) == E_NULL                     # resuming needs the carry
    assert f(*_gen_args(which, 2 ** 31 - 3, A)) == E_SHAPE             # t0 + nsteps past int32
    assert f(*_gen_args(which, 0, None, ring=None)) == E_NULL
    assert f(*_gen_args(which, 3, A, ring=None)) == E_NULL
    assert f(*_gen_args(which, 3, A, R=48)) == E_UNSUPPORTED
    assert f(*_gen_args(which, 3, A, L=0)) == E_SHAPE
    assert f(*_gen_args(which, 3, A, L=65, dil=_dl([1] * 65))) == E_SHAPE
    assert f(*_gen_args(which, 3, A, dil=_dl([1, 0]))) == E_SHAPE
    assert f(*_gen_args(which, 3, A, B=0)) == 0                        # empty work, no launch
    assert f(*_gen_args(which, 3, A, nsteps=0)) == 0


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_resume_bad_dtype(binding):
    lib = _lib(binding)
    a = _gen_args("srwn_generate_resume", 3, A)
    a[-4] = 9                                                         # dtype
    assert lib.srwn_generate_resume(*a) == E_DTYPE
    a = _gen_args("srwn_generate_mol_resume", 3, A)
    a[-4] = 9
    assert lib.srwn_generate_mol_resume(*a) == E_DTYPE


def _bare(cls, **attrs):
    """A model object without its engines (constructing one needs a GPU): what generation checks first."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_teacher_refuses_bad_prompts_and_the_wavenet_gate_first():
    M = sub("model")
    t = _bare(M.WaveNetTeacher, head="softmax", use_encoding=False, gate_mode="reference", _primary=None)
    for bad in (np.zeros((3, 10)), np.zeros(10), np.zeros((2, 4, 1))):
        with pytest.raises(ValueError, match="prompt"):
            t.generate(2, 100, prompt=bad)
        with pytest.raises(ValueError, match="prompt"):
            t.stream(2, 16, prompt=bad)
    with pytest.raises(ValueError, match="chunk_size"):
        t.stream(2, 0)
    w = _bare(M.WaveNetTeacher, head="softmax", use_encoding=False, gate_mode="wavenet", _primary=None)
    with pytest.raises(NotImplementedError, match="wavenet"):
        w.generate(2, 100, prompt=np.zeros((2, 10)))
    with pytest.raises(NotImplementedError, match="wavenet"):
        w.stream(2, 16)
    c = _bare(M.WaveNetTeacher, head="softmax", use_encoding=True, gate_mode="reference", _primary=None)
    with pytest.raises(NotImplementedError):
        c.stream(2, 16)


def test_autoencoder_refuses_bad_prompts_first():
    M = sub("model")
    ae = _bare(M.WaveNetAutoEncoder, latent_channels=8, pool_stride=32, condition_size=0, _eng=None)
    enc = np.zeros((2, 4, 8), np.float32)
    with pytest.raises(ValueError, match="prompt"):
        ae.generate(enc, prompt=np.zeros((3, 10)))
    with pytest.raises(ValueError, match="prompt"):
        ae.stream(enc, prompt=np.zeros((2, 129)))                     # longer than frames * pool_stride
    with pytest.raises(ValueError, match="encoding"):
        ae.stream(enc[:, :, :3])
    with pytest.raises(ValueError, match="chunk_size"):
        ae.stream(enc, chunk_size=0)
