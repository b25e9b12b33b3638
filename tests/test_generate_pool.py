"""CPU tests of generation pools (srwn_version() 105): the slot entry points and the slot ring fill are declared, bound
and generated with the argument lists of their resume twins; their argument errors come back as negative codes without a
GPU; the ctypes mirror of SrwnGenSlot has the header's layout; the engine pool and the model classes refuse what
generation refuses, and malformed joins, before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests._pkg import ROOT, sub

SLOTS = ["srwn_generate_slots", "srwn_generate_mol_slots", "srwn_generate16_slots", "srwn_generate16_mol_slots"]
NEW = SLOTS + ["srwn_generate_ring_fill_slots"]
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _lib(binding):
    L = sub("_lib")
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "sr-wavenet_amd", "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.build()
    return L.bind(binding)


def test_slot_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n
    # each slot form is its resume twin without the seed, with (clock, carry, slots) in place of (t0, carry)
    for base in ("srwn_generate", "srwn_generate_mol", "srwn_generate16", "srwn_generate16_mol"):
        r0, a0 = L.SIGNATURES[base + "_resume"]
        r1, a1 = L.SIGNATURES[base + "_slots"]
        seeds = [i for i, t in enumerate(a0) if t is C.c_uint64]
        assert len(seeds) == 1, base
        want = [t for i, t in enumerate(a0) if i != seeds[0]][:-2] + [L._i32, L._p, L._p]
        assert r0 is r1 and list(a1) == want, base


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_version_and_exports(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 105
    for n in NEW:
        assert callable(getattr(lib, n))


def test_slot_struct_mirror_has_the_header_layout():
    L = sub("_lib")
    S = L.SrwnGenSlot
    assert C.sizeof(S) == 16
    assert (S.t.offset, S.t_end.offset, S.seed.offset) == (0, 4, 8)
    # and the header's own layout, as a C compiler sees it
    cxx = os.environ.get("CXX", "g++")
    prog = ('#include <cstdio>\n#include <cstddef>\n#include "srwn.h"\nint main() { std::printf("%zu %zu %zu %zu", '
            'sizeof(SrwnGenSlot), offsetof(SrwnGenSlot, t), offsetof(SrwnGenSlot, t_end), offsetof(SrwnGenSlot, seed)); }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "l.cpp"), "w") as f:
            f.write(prog)
        subprocess.run([cxx, "-I", os.path.join(ROOT, "include"), os.path.join(d, "l.cpp"), "-o", os.path.join(d, "l")],
                       check=True)
        out = subprocess.run([os.path.join(d, "l")], capture_output=True, text=True, check=True).stdout
    assert out.split() == ["16", "0", "4", "8"]


def _dl(dils):
    return (C.c_int32 * len(dils))(*dils)


def _slot_args(which, clock=0, carry=A, slots=A, B=2, R=64, S=256, L=2, dil=None, ring=A, nsteps=4, Tout=None, C_=256,
               dtype=1):
    d = dil if dil is not None else _dl([1, 2])
    common = [A] * 7 + [ring, A, A, None, None, d, L, B, nsteps if Tout is None else Tout, nsteps, R, S]
    tail = [clock, carry, slots]
    if which == "srwn_generate_slots":
        return [A] * 4 + common + [C_, 2, 0, dtype, None] + tail
    if which == "srwn_generate_mol_slots":
        return [A] * 4 + common + [2, 5, None, 1, 1, 0, 0, dtype, None] + tail
    if which == "srwn_generate16_slots":
        return [A] * 3 + common + [C_, 0, None] + tail
    return [A] * 3 + common + [5, None, 1, 1, 0, 0, None] + tail


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
@pytest.mark.parametrize("which", SLOTS)
def test_slot_argument_errors_do_not_need_a_gpu(binding, which):
    lib = _lib(binding)
    f = getattr(lib, which)
    assert f(*_slot_args(which, clock=-1)) == E_SHAPE                    # clock < 0
    assert f(*_slot_args(which, clock=2 ** 31 - 3)) == E_SHAPE           # clock + nsteps past int32
    assert f(*_slot_args(which, carry=None)) == E_NULL                   # the pool's carry is required
    assert f(*_slot_args(which, slots=None)) == E_NULL                   # ... and its slot table
    assert f(*_slot_args(which, ring=None)) == E_NULL
    assert f(*_slot_args(which, R=48)) == E_UNSUPPORTED
    assert f(*_slot_args(which, S=192)) == E_UNSUPPORTED
    assert f(*_slot_args(which, nsteps=5, Tout=4)) == E_SHAPE            # nsteps > Tout
    assert f(*_slot_args(which, L=0)) == E_SHAPE
    assert f(*_slot_args(which, dil=_dl([1, 0]))) == E_SHAPE
    if which in ("srwn_generate_slots", "srwn_generate16_slots"):
        assert f(*_slot_args(which, C_=300)) == E_UNSUPPORTED
    if which in ("srwn_generate_slots", "srwn_generate_mol_slots"):
        assert f(*_slot_args(which, dtype=9)) == E_DTYPE
    assert f(*_slot_args(which, B=0)) == 0                               # empty work, no launch
    assert f(*_slot_args(which, nsteps=0, Tout=4)) == 0
    assert b"generate" in lib.srwn_last_error()


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_ring_fill_slots_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    d = _dl([1, 2, 4])
    BF16, F32 = 1, 0

    def fill(xs=A, stride=2 * 10 * 64, T=10, n=2, dst=A, P=A, clock=3, dil=d, L=3, B=4, R=64, ring=A, dtype=BF16):
        return lib.srwn_generate_ring_fill_slots(xs, stride, T, n, dst, P, clock, dil, L, B, R, ring, dtype, None)

    assert fill(n=0) == 0                                  # empty work, no launch
    assert fill(n=-1) == E_SHAPE
    assert fill(ring=None) == E_NULL
    assert fill(dst=None) == E_NULL
    assert fill(P=None) == E_NULL
    assert fill(dil=None) == E_NULL
    assert fill(R=48) == E_UNSUPPORTED
    assert fill(dtype=7) == E_DTYPE
    assert fill(clock=-1) == E_SHAPE
    assert fill(B=0) == E_SHAPE
    assert fill(L=0) == E_SHAPE
    assert fill(L=65, dil=_dl([1] * 65)) == E_SHAPE
    assert fill(dil=_dl([1, 0, 4])) == E_SHAPE
    assert fill(stride=2 * 10 * 64 + 1) == E_SHAPE         # layer rows must stay 16-byte aligned
    assert fill(xs=A + 2) == E_SHAPE
    assert fill(dtype=F32, stride=2 * 10 * 64 - 4) == E_SHAPE   # layers would overlap
    assert fill(ring=A + 4) == E_SHAPE
    msg = lib.srwn_last_error()
    assert msg and b"ring_fill_slots" in msg


def _bare(cls, **attrs):
    """An object without its device state (constructing one needs a GPU): what the pool checks first."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_engine_refuses_what_generate_refuses_first():
    EG = sub("engine")
    from types import SimpleNamespace
    ok = dict(wavenet=False, o_gen=0, cfg=SimpleNamespace(head_mode="per_timestep"), mol=False, E=0)
    with pytest.raises(NotImplementedError, match="wavenet"):
        _bare(EG.WaveNetEngine, **dict(ok, wavenet=True)).generation_pool(4)
    with pytest.raises(NotImplementedError, match="conditioned softmax"):
        _bare(EG.WaveNetEngine, **dict(ok, E=6)).generation_pool(4)
    with pytest.raises(NotImplementedError):
        _bare(EG.WaveNetEngine, **dict(ok, cfg=SimpleNamespace(head_mode="pooled"))).generation_pool(4)   # clip-level
    with pytest.raises(NotImplementedError):
        _bare(EG.WaveNetEngine, **dict(ok, o_gen=None)).generation_pool(4)       # widths the generators do not build
    for cap in (0, -3):
        with pytest.raises(ValueError, match="capacity"):
            _bare(EG.WaveNetEngine, **ok).generation_pool(cap)
    with pytest.raises(ValueError, match="frames"):
        _bare(EG.WaveNetEngine, **dict(ok, mol=True, E=6)).generation_pool(4)     # a conditioned decoder needs frames
    with pytest.raises(ValueError, match="frames"):
        _bare(EG.WaveNetEngine, **ok).generation_pool(4, frames=3)


def _bare_pool(capacity=4, active=(), conditioned=False, frames=0, E=0, pool_stride=1):
    EG = sub("engine")
    act = np.zeros(capacity, bool)
    act[list(active)] = True
    return _bare(EG.GenerationPool, capacity=capacity, _active=act, conditioned=conditioned, frames=frames, E=E,
                 pool_stride=pool_stride, eng=None)


def test_pool_refuses_malformed_joins_first():
    p = _bare_pool(capacity=4, active=[1])
    with pytest.raises(ValueError, match="free slots"):
        p.join([1, 2, 3, 4])                                           # 3 free slots
    with pytest.raises(ValueError, match="prompts"):
        p.join([1, 2], prompts=[np.zeros(3)])                          # mismatched list lengths
    with pytest.raises(ValueError, match="max_samples"):
        p.join([1, 2], max_samples=[5])
    with pytest.raises(ValueError, match="1-D"):
        p.join([1], prompts=[np.zeros((1, 3))])                        # prompts are 1-D
    with pytest.raises(ValueError, match="1-D"):
        p.join([1], prompts=[np.float32(0.5)])
    with pytest.raises(ValueError, match="slots"):
        p.join([1], slots=[1])                                         # slot 1 is taken
    with pytest.raises(ValueError, match="slots"):
        p.join([1, 2], slots=[0, 0])
    with pytest.raises(ValueError, match="slots"):
        p.join([1], slots=[4])
    with pytest.raises(ValueError, match="not conditioned"):
        p.join([1], cond=[np.zeros((2, 6))])
    with pytest.raises(ValueError, match="no streams"):
        p.join([])
    c = _bare_pool(capacity=4, conditioned=True, frames=3, E=6, pool_stride=16)
    with pytest.raises(ValueError, match="conditioned"):
        c.join([1])                                                    # no encoding
    with pytest.raises(ValueError, match="cond"):
        c.join([1], cond=[np.zeros((4, 6))])                           # more frames than the pool holds
    with pytest.raises(ValueError, match="cond"):
        c.join([1], cond=[np.zeros((2, 5))])
    with pytest.raises(ValueError, match="encodings"):
        c.join([1, 2], cond=[np.zeros((2, 6))])
    with pytest.raises(ValueError, match="exceeds"):
        c.join([1], prompts=[np.zeros(33)], cond=[np.zeros((2, 6))])   # prompt past frames * pool_stride


def test_models_refuse_first():
    M = sub("model")
    w = _bare(M.WaveNetTeacher, head="softmax", use_encoding=False, gate_mode="wavenet", _primary=None)
    with pytest.raises(NotImplementedError, match="wavenet"):
        w.generation_pool(4)
    c = _bare(M.WaveNetTeacher, head="softmax", use_encoding=True, gate_mode="reference", _primary=None)
    with pytest.raises(NotImplementedError, match="conditioned softmax"):
        c.generation_pool(4, frames=2)
    t = _bare(M.WaveNetTeacher, head="softmax", use_encoding=False, gate_mode="reference", _primary=None)
    with pytest.raises(ValueError, match="capacity"):
        t.generation_pool(0)
    m = _bare(M.WaveNetTeacher, head="mol", use_encoding=True, gate_mode="reference", _primary=None, latent_channels=8,
              condition_size=0)
    with pytest.raises(ValueError, match="frames"):
        m.generation_pool(4)
    ae = _bare(M.WaveNetAutoEncoder, latent_channels=8, pool_stride=32, condition_size=0, _eng=None)
    with pytest.raises(ValueError, match="capacity"):
        ae.generation_pool(0, 4)
    with pytest.raises(ValueError, match="frames"):
        ae.generation_pool(4, None)
    # the NumPy pool checks its lists before the engine pool sees them
    mp = M.GenerationPool(_bare_pool(capacity=4), t._pool_cond, "sample")
    with pytest.raises(ValueError, match="prompts"):
        mp.join(seed=[1, 2], prompt=[np.zeros(3)])
    with pytest.raises(ValueError, match="1-D"):
        mp.join(seed=[1], prompt=[np.zeros((2, 3))])
    with pytest.raises(ValueError, match="not conditioned"):
        mp.join(seed=[1], encoding=[np.zeros((2, 8))])
    with pytest.raises(ValueError, match="free slots"):
        mp.join(seed=[1, 2, 3, 4, 5])
    ap = M.GenerationPool(_bare_pool(capacity=4, conditioned=True, frames=4, E=8, pool_stride=32), ae._pool_cond, "sample")
    with pytest.raises(ValueError, match="encoding"):
        ap.join(seed=[1])
    with pytest.raises(ValueError, match="encoding"):
        ap.join(seed=[1], encoding=[np.zeros((2, 5))])
    with pytest.raises(ValueError, match="encodings"):
        ap.join(seed=[1, 2], encoding=[np.zeros((2, 8))])
