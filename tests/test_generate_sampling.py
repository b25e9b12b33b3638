"""CPU tests of the generators' sampling controls (srwn_version() 106): the *_sampled twins and srwn_sample_filtered are
declared, bound and generated with the argument lists of the calls they extend plus one pointer; the ctypes mirror of
SrwnGenSampling has the header's layout; argument errors come back as negative codes without a GPU; the engine, pool and
model classes refuse out-of-range controls, before any device work and after what generation already refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests._pkg import ROOT, sub

BASES = ["srwn_generate_resume", "srwn_generate_mol_resume", "srwn_generate16_resume", "srwn_generate16_mol_resume",
         "srwn_generate_slots", "srwn_generate_mol_slots", "srwn_generate16_slots", "srwn_generate16_mol_slots"]
TWINS = [b + "_sampled" for b in BASES]
NEW = TWINS + ["srwn_sample_filtered"]
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _lib(binding):
    L = sub("_lib")
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "sr-wavenet_amd", "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.build()
    return L.bind(binding)


def test_sampled_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n
    for b in BASES:      # each twin: the arguments of the call it extends, plus the device array
        r0, a0 = L.SIGNATURES[b]
        r1, a1 = L.SIGNATURES[b + "_sampled"]
        assert r0 is r1 and list(a1) == list(a0) + [L._p], b
        m = re.search(r"\b%s_sampled\s*\((.*?)\)\s*;" % b, hdr, flags=re.S)
        assert m and re.search(r"const\s+SrwnGenSampling\s*\*\s*sampling\s*$", m.group(1).strip()), b
    assert "SrwnGenSampling" in hdr and "SrwnGenSlot" in hdr


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_version_and_exports(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 106
    for n in NEW:
        assert callable(getattr(lib, n))


def test_sampling_struct_mirror_has_the_header_layout():
    L = sub("_lib")
    S = L.SrwnGenSampling
    assert C.sizeof(S) == 16
    assert (S.temperature.offset, S.top_p.offset, S.top_k.offset, S.reserved.offset) == (0, 4, 8, 12)
    cxx = os.environ.get("CXX", "g++")
    prog = ('#include <cstdio>\n#include <cstddef>\n#include "srwn.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu", '
            'sizeof(SrwnGenSampling), offsetof(SrwnGenSampling, temperature), offsetof(SrwnGenSampling, top_p), '
            'offsetof(SrwnGenSampling, top_k), offsetof(SrwnGenSampling, reserved), sizeof(SrwnGenSlot)); }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "l.cpp"), "w") as f:
            f.write(prog)
        subprocess.run([cxx, "-I", os.path.join(ROOT, "include"), os.path.join(d, "l.cpp"), "-o", os.path.join(d, "l")],
                       check=True)
        out = subprocess.run([os.path.join(d, "l")], capture_output=True, text=True, check=True).stdout
    assert out.split() == ["16", "0", "4", "8", "12", "16"]


def _dl(dils):
    return (C.c_int32 * len(dils))(*dils)


def _args(which, t0=0, carry=A, slots=A, B=2, R=64, S=256, L=2, dil=None, ring=A, nsteps=4, Tout=None, C_=256, dtype=1,
          sampling=A):
    """The argument list of a *_sampled twin (resume: (t0, carry); slots: (clock, carry, slots)), then `sampling`."""
    d = dil if dil is not None else _dl([1, 2])
    common = [A] * 7 + [ring, A, A, None, None, d, L, B, nsteps if Tout is None else Tout, nsteps, R, S]
    slot_form = "_slots" in which
    tail = [t0, carry] + ([slots] if slot_form else []) + [sampling]
    seed = [] if slot_form else [7]
    if which.startswith("srwn_generate16_mol"):
        return [A] * 3 + common + [5, None, 1, 1, 0, 0] + seed + [None] + tail
    if which.startswith("srwn_generate16"):
        return [A] * 3 + common + [C_, 0] + seed + [None] + tail
    if which.startswith("srwn_generate_mol"):
        return [A] * 4 + common + [2, 5, None, 1, 1, 0, 0] + seed + [dtype, None] + tail
    return [A] * 4 + common + [C_, 2, 0] + seed + [dtype, None] + tail


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
@pytest.mark.parametrize("which", TWINS)
@pytest.mark.parametrize("sampling", [A, None])
def test_twin_argument_errors_do_not_need_a_gpu(binding, which, sampling):
    lib = _lib(binding)
    f = getattr(lib, which)
    kw = dict(sampling=sampling)
    assert f(*_args(which, t0=-1, **kw)) == E_SHAPE
    assert f(*_args(which, t0=2 ** 31 - 3, **kw)) == E_SHAPE           # t0 / clock + nsteps past int32
    assert f(*_args(which, t0=3, carry=None, **kw)) == E_NULL          # resuming needs the carry
    if "_slots" in which:
        assert f(*_args(which, carry=None, **kw)) == E_NULL
        assert f(*_args(which, slots=None, **kw)) == E_NULL
    assert f(*_args(which, ring=None, **kw)) == E_NULL
    assert f(*_args(which, R=48, **kw)) == E_UNSUPPORTED
    assert f(*_args(which, S=192, **kw)) == E_UNSUPPORTED
    assert f(*_args(which, nsteps=5, Tout=4, **kw)) == E_SHAPE         # nsteps > Tout
    assert f(*_args(which, L=0, **kw)) == E_SHAPE
    assert f(*_args(which, dil=_dl([1, 0]), **kw)) == E_SHAPE
    if "_mol" not in which:
        assert f(*_args(which, C_=300, **kw)) == E_UNSUPPORTED
    if "generate16" not in which:
        assert f(*_args(which, dtype=9, **kw)) == E_DTYPE
    assert f(*_args(which, B=0, **kw)) == 0                            # empty work, no launch
    assert f(*_args(which, nsteps=0, Tout=4, **kw)) == 0
    assert b"generate" in lib.srwn_last_error()


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_sample_filtered_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)

    def f(logits=A, ld=256, sampling=A, uniforms=A, out=A, rows=8, C_=256):
        return lib.srwn_sample_filtered(logits, ld, sampling, uniforms, out, rows, C_, None)

    assert f(rows=0) == 0                                  # empty work, no launch
    assert f(C_=257) == E_UNSUPPORTED
    assert f(C_=0) == E_UNSUPPORTED
    assert f(uniforms=None) == E_NULL
    assert f(logits=None) == E_NULL
    assert f(out=None) == E_NULL
    assert f(rows=-1) == E_SHAPE
    assert f(ld=100, C_=200) == E_SHAPE                    # rows would overlap
    msg = lib.srwn_last_error()
    assert msg and b"sample_filtered" in msg


def test_sampling_table_ranges():
    EG = sub("engine")
    L = sub("_lib")
    T = EG.sampling_table
    assert T(3, 1.0, 0, 1.0, 256, False) is None            # all defaults: the calls without controls
    assert T(3, None, None, None, 256, False) is None
    assert T(2, [1.0, 1.0], [0, 0], [1.0, 1.0], 256, False) is None
    t = T(3, [0.5, 1.0, 2.0], 40, 0.9, 256, False)
    assert t.dtype == np.dtype(L.SrwnGenSampling) and t.dtype.itemsize == 16 and len(t) == 3
    assert t["temperature"].tolist() == [0.5, 1.0, 2.0] and t["top_k"].tolist() == [40] * 3
    assert np.allclose(t["top_p"], 0.9) and t["reserved"].tolist() == [0, 0, 0]
    assert T(1, 1.0, 256, 1.0, 256, False)["top_k"][0] == 256            # top_k = C is in range
    assert T(2, 0.7, 0, 1.0, 40, True)["temperature"].tolist() == [np.float32(0.7)] * 2
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="temperature"):
            T(2, bad, 0, 1.0, 256, False)
    with pytest.raises(ValueError, match=r"temperature.*3 entries.*2"):
        T(2, [1.0, 0.5, 0.2], 0, 1.0, 256, False)
    with pytest.raises(ValueError, match=r"top_k.*1 entries.*2"):
        T(2, 1.0, [5], 1.0, 256, False)
    with pytest.raises(ValueError, match=r"top_p.*3 entries.*2"):
        T(2, 1.0, 0, [0.5, 0.5, 0.5], 256, False)
    for bad in (257, -1, 10 ** 6):
        with pytest.raises(ValueError, match="top_k %d" % bad):
            T(2, 1.0, bad, 1.0, 256, False)
    with pytest.raises(ValueError, match="top_k 41"):
        T(2, 1.0, [3, 41], 1.0, 40, False)                               # top_k > C
    with pytest.raises(ValueError, match="top_k"):
        T(2, 1.0, 2.5, 1.0, 256, False)
    for bad in (0.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            T(2, 1.0, 0, bad, 256, False)
    with pytest.raises(ValueError, match=r"top_k 3.*mixture"):
        T(2, 0.7, 3, 1.0, 40, True)                                      # a mixture head: temperature only
    with pytest.raises(ValueError, match=r"top_p 0\.9.*mixture"):
        T(2, 0.7, 0, 0.9, 40, True)


def _bare(cls, **attrs):
    """An object without its device state (constructing one needs a GPU): what the checks see first."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_engine_refuses_bad_controls_before_device_work():
    EG = sub("engine")
    from types import SimpleNamespace
    ok = dict(wavenet=False, o_gen=0, cfg=SimpleNamespace(head_mode="per_timestep"), mol=False, E=0, C=256, B=2)
    e = _bare(EG.WaveNetEngine, **ok)
    with pytest.raises(ValueError, match="temperature 0"):
        e.generate(8, temperature=0)
    with pytest.raises(ValueError, match="top_k 300"):
        e.generate(8, top_k=300)
    with pytest.raises(ValueError, match=r"top_p.*3 entries.*2"):
        e.generate(8, top_p=[0.5, 0.5, 0.5])
    with pytest.raises(ValueError, match="top_p 2"):
        e.generation_state(2, top_p=2)
    with pytest.raises(ValueError, match=r"temperature.*1 entries.*2"):
        e.generation_state(2, temperature=[0.5])
    m = _bare(EG.WaveNetEngine, **dict(ok, mol=True, C=40, cfg=SimpleNamespace(head_mode="mol")))
    with pytest.raises(ValueError, match=r"top_k 4.*mixture"):
        m.generate(8, temperature=0.5, top_k=4)
    with pytest.raises(ValueError, match=r"top_p 0\.5.*mixture"):
        m.generation_state(2, top_p=0.5)
    # what generation already refuses comes first
    with pytest.raises(NotImplementedError, match="wavenet"):
        _bare(EG.WaveNetEngine, **dict(ok, wavenet=True)).generate(8, temperature=-1)
    with pytest.raises(NotImplementedError, match="wavenet"):
        _bare(EG.WaveNetEngine, **dict(ok, wavenet=True)).generation_state(2, temperature=-1)
    with pytest.raises(NotImplementedError):
        _bare(EG.WaveNetEngine, **dict(ok, o_gen=None)).generate(8, top_k=-1)
    # the controls are keyword-only
    with pytest.raises(TypeError):
        e.generation_state(2, None, 0, 0.5)


def _bare_pool(capacity=4, active=(), conditioned=False, frames=0, E=0, pool_stride=1, C_=256, mol=False):
    EG = sub("engine")
    act = np.zeros(capacity, bool)
    act[list(active)] = True
    return _bare(EG.GenerationPool, capacity=capacity, _active=act, conditioned=conditioned, frames=frames, E=E,
                 pool_stride=pool_stride, eng=None, C=C_, mol=mol)


def test_pool_refuses_bad_controls_before_device_work():
    p = _bare_pool()
    with pytest.raises(ValueError, match=r"temperature.*3 entries.*2"):
        p.join([1, 2], temperature=[0.5, 0.6, 0.7])
    with pytest.raises(ValueError, match="top_k 257"):
        p.join([1, 2], top_k=257)
    with pytest.raises(ValueError, match="top_p 0"):
        p.join([1], top_p=0.0)
    with pytest.raises(ValueError, match="temperature nan"):
        p.join([1], temperature=float("nan"))
    with pytest.raises(ValueError, match="no streams"):
        p.join([], temperature=0.5)                                      # the existing refusals still come first
    m = _bare_pool(C_=40, mol=True)
    with pytest.raises(ValueError, match=r"top_k 2.*mixture"):
        m.join([1], top_k=2)
    with pytest.raises(TypeError):
        p.join([1], None, None, None, None, 0.5)                         # keyword-only


def test_models_refuse_bad_controls_and_keep_their_refusals_first():
    M = sub("model")
    t = _bare(M.WaveNetTeacher, head="softmax", use_encoding=False, gate_mode="reference", _primary=None,
              quantization_channels=256, num_mixtures=5)
    with pytest.raises(ValueError, match="temperature -1"):
        t.generate(2, 16, temperature=-1)
    with pytest.raises(ValueError, match="top_k 257"):
        t.generate(2, 16, top_k=257)
    with pytest.raises(ValueError, match=r"top_p.*1 entries.*2"):
        t.generate(2, 16, top_p=[0.5])
    with pytest.raises(ValueError, match="top_p 1.5"):
        list(t.stream(2, 8, top_p=1.5))
    with pytest.raises(ValueError, match="top_k 300"):
        t.generate(2, 16, prompt=np.zeros((2, 4), np.float32), top_k=300)
    w = _bare(M.WaveNetTeacher, head="softmax", use_encoding=False, gate_mode="wavenet", _primary=None,
              quantization_channels=256, num_mixtures=5)
    with pytest.raises(NotImplementedError, match="wavenet"):
        w.generate(2, 16, temperature=0.5)
    with pytest.raises(NotImplementedError, match="wavenet"):
        w.stream(2, 8, temperature=0.5)
    c = _bare(M.WaveNetTeacher, head="softmax", use_encoding=True, gate_mode="reference", _primary=None,
              quantization_channels=256, num_mixtures=5)
    with pytest.raises(NotImplementedError, match="conditioned softmax"):
        c.generate(2, 16, temperature=0.5)
    with pytest.raises(NotImplementedError, match="conditioned softmax"):
        c.stream(2, 8, temperature=0.5, top_k=-3)
    m = _bare(M.WaveNetTeacher, head="mol", use_encoding=False, gate_mode="reference", _primary=None,
              quantization_channels=256, num_mixtures=10)
    with pytest.raises(ValueError, match=r"top_k 5.*mixture"):
        m.generate(2, 16, temperature=0.5, top_k=5)
    with pytest.raises(ValueError, match=r"top_p 0\.9.*mixture"):
        m.stream(2, 8, top_p=0.9)
    ae = _bare(M.WaveNetAutoEncoder, latent_channels=8, pool_stride=32, condition_size=0, _eng=None, num_mixtures=10)
    enc = np.zeros((2, 3, 8), np.float32)
    with pytest.raises(ValueError, match=r"top_k 3.*mixture"):
        ae.generate(enc, top_k=3)
    with pytest.raises(ValueError, match="temperature 0"):
        ae.generate(enc, temperature=0)
    with pytest.raises(ValueError, match=r"temperature.*3 entries.*2"):
        ae.stream(enc, temperature=[0.5, 0.5, 0.5])
    # the NumPy pool hands the controls to the engine pool's checks
    mp = M.GenerationPool(_bare_pool(capacity=4), t._pool_cond, "sample")
    with pytest.raises(ValueError, match="top_k 999"):
        mp.join(seed=[1, 2], top_k=999)
    with pytest.raises(ValueError, match=r"top_p.*3 entries.*2"):
        mp.join(seed=[1, 2], top_p=[0.5, 0.5, 0.5])
    ap = M.GenerationPool(_bare_pool(capacity=4, conditioned=True, frames=4, E=8, pool_stride=32, C_=40, mol=True),
                          ae._pool_cond, "sample")
    with pytest.raises(ValueError, match=r"top_p 0\.5.*mixture"):
        ap.join(seed=[1], encoding=[np.zeros((2, 8))], top_p=0.5)
