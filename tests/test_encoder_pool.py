"""CPU tests of encoder and resynthesis pools (srwn_version() 111): the slot scheme restated in NumPy on the fp64 oracle and
driven by the product's own planning helper (encoder.plan_pool) over audio rings of the minimum length, the C-ABI of
srwn_nc_encode_frame_list and srwn_audio_ring_put, and every refusal that comes before any device work."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import wavenet_np as O
from tests._pkg import ROOT, sub

E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4


# ---- the slot scheme on the fp64 oracle ----------------------------------------------------------------------------------
class _NumpyPool:
    """EncoderPool's host side restated: per slot a ring of `ring` samples (sample s in column s mod ring), the counters
    and plan_pool.  Every emitted item is evaluated by the oracle on its own window read from the ring."""

    def __init__(self, E, ep, L, P, capacity, ring, max_rows):
        self.E, self.ep, self.L, self.P, self.ring_len, self.max_rows = E, ep, L, P, ring, max_rows
        self.ring = np.full((capacity, ring), np.nan)
        self.received = np.zeros(capacity, np.int64)
        self.emitted = np.zeros(capacity, np.int64)
        self.final = np.zeros(capacity, bool)
        self.active = np.zeros(capacity, bool)

    def room(self, u):
        return int(self.ring_len - (self.received[u] - self.emitted[u] * self.P))

    def join(self, u):
        assert not self.active[u]
        self.received[u] = self.emitted[u] = 0
        self.final[u], self.active[u] = False, True

    def push(self, u, x):
        assert len(x) <= self.room(u)
        self.ring[u, (self.received[u] + np.arange(len(x))) % self.ring_len] = x
        self.received[u] += len(x)

    def step(self, clips, limit):
        """clips: slot -> the whole clip of the stream it holds (to check what a window reads).  Returns {slot: frames}."""
        L, P = self.L, self.P
        before = self.emitted.copy()
        launches = self.E.plan_pool(self.received, self.emitted, self.final, self.active, L, P, self.max_rows, limit)
        flat = [it for items in launches for it in items]
        assert flat == sorted(flat, key=lambda it: (it[0], it[1])), "items are not ordered slot-then-frame"
        out = {}
        for items in launches:
            assert 1 <= len(items) <= self.max_rows
            for (u, f, first, valid) in items:
                assert self.active[u] and f == self.emitted[u] and first == f * P
                assert valid == min(self.received[u] - first, P + L + 1) and valid >= P
                assert before[u] * P <= first and first + valid <= self.received[u], "a window leaves [emitted*P, received)"
                if not self.final[u]:
                    assert (f + 1) * P + L + 1 <= self.received[u], "a frame was emitted before its look-ahead was in"
                win = self.ring[u, (first + np.arange(valid)) % self.ring_len]
                assert np.array_equal(win, clips[u][first:first + valid]), "the window read a stale column of the ring"
                out.setdefault(u, []).append(O.encoder_forward(self.ep, win[None], P)[0, :1])
                self.emitted[u] += 1
        for u in range(len(self.active)):
            if self.active[u]:
                cap = None if limit is None else limit[u]
                due = self.received[u] // P if self.final[u] else max(0, (self.received[u] - L - 1) // P)
                want = due if cap is None else min(due, before[u] + cap)
                assert self.emitted[u] == want, "a frame that is due and allowed was held back"
                assert self.received[u] - self.emitted[u] * P <= self.ring_len
                if self.final[u] and (self.emitted[u] + 1) * P > self.received[u]:
                    self.active[u] = False
        return {u: np.concatenate(v, 0) for u, v in out.items()}


@pytest.mark.parametrize("max_rows", [1, 3, 64])
@pytest.mark.parametrize("L", [1, 5])
@pytest.mark.parametrize("P", [7, 32])
def test_pool_plan_reproduces_every_clip(L, P, max_rows):
    E = sub("encoder")
    rng = np.random.default_rng(100 * L + P + max_rows)
    ep = O.init_encoder_params(5 + L, L, 2, 8, 8, 4, bias_scale=0.05)
    lengths = [6 * P + 5, P - 1, 3 * P + L + 1, 4 * P + 3]            # shorter than P; exactly k P + L + 1
    clips = [rng.uniform(-1, 1, size=T) for T in lengths]
    whole = [O.encoder_forward(ep, c[None], P)[0] for c in clips]
    join_at = [0, 0, 2, None]                                            # the fourth joins when a slot frees: a REUSED slot
    pool = _NumpyPool(E, ep, L, P, 3, P + L + 1, max_rows)               # rings of the minimum length: every stream wraps
    assert lengths[0] > 2 * (P + L + 1)                                  # (the long ones wrap the ring several times)
    holder, joined, got, pushed, held_by_zero = {}, [], {i: [] for i in range(4)}, [0] * 4, 0
    step = 0
    while len(joined) < 4 or pool.active.any():
        holder = {u: i for u, i in holder.items() if pool.active[u]}
        for i in range(4):
            free = np.flatnonzero(~pool.active)
            due = step >= join_at[i] if join_at[i] is not None else (len(joined) == 3 and len(free) > 0)
            if i in joined or not due:
                continue
            u = int(free[0])
            pool.join(u)
            assert pool.received[u] == 0 and pool.emitted[u] == 0 and not pool.final[u]      # a reused slot starts at 0
            holder[u] = i
            joined.append(i)
        for u, i in holder.items():
            if pool.final[u]:
                continue
            left = lengths[i] - pushed[i]
            n = min(int(rng.choice([0, 1, rng.integers(2, P + 2), rng.integers(P, 3 * P + 1)])), left, pool.room(u))
            pool.push(u, clips[i][pushed[i]:pushed[i] + n])
            pushed[i] += n
            if pushed[i] == lengths[i]:
                pool.final[u] = True
        limit = [None if rng.random() < 0.4 else int(rng.integers(0, 3)) for _ in range(3)]
        audio_before = pool.ring.copy(), pool.received.copy(), pool.emitted.copy()
        out = pool.step({u: clips[i] for u, i in holder.items()}, limit)
        for u in holder:
            if limit[u] == 0:                                           # a limit of 0 leaves the slot's audio untouched
                assert u not in out and pool.emitted[u] == audio_before[2][u] and pool.received[u] == audio_before[1][u]
                assert np.array_equal(pool.ring[u], audio_before[0][u], equal_nan=True)
                held_by_zero += 1
        for u, fr in out.items():
            got[holder[u]].append(fr)
        step += 1
        assert step < 4000
    assert held_by_zero > 0
    assert sorted(joined) == [0, 1, 2, 3] and joined[-1] == 3           # four streams through three slots: one was reused
    for i in range(4):
        g = np.concatenate(got[i], 0) if got[i] else np.zeros((0, 4))
        assert g.shape == whole[i].shape == (lengths[i] // P, 4), i      # a final stream emits received // P frames
        if g.size:
            assert np.abs(g - whole[i]).max() <= 1e-12, i


def test_plan_pool_rules():
    E = sub("encoder")
    L, P = 5, 16
    W = P + L + 1
    rec, emi = [3 * P + 2, 0, W, 5 * P], [1, 0, 0, 2]
    plan = E.plan_pool(rec, emi, [True, False, False, False], [True, True, True, True], L, P, 64)
    assert plan == [[(0, 1, P, W), (0, 2, 2 * P, P + 2), (2, 0, 0, W), (3, 2, 2 * P, W), (3, 3, 3 * P, W)]]
    assert E.plan_pool(rec, emi, [True] + [False] * 3, [True] * 4, L, P, 2) == [plan[0][:2], plan[0][2:4], plan[0][4:]]
    assert E.plan_pool(rec, emi, [True] + [False] * 3, [True, True, False, True], L, P, 64, [1, None, None, 0]) == [[(0, 1, P, W)]]
    assert E.plan_pool(rec, emi, [True] + [False] * 3, [True] * 4, L, P, 64, {3: 1}) == [plan[0][:4]]
    assert E.plan_pool([W - 1], [0], [False], [True], L, P, 4) == [] and E.plan_pool([P - 1], [0], [True], [True], L, P, 4) == []
    assert E.plan_pool([], [], [], [], L, P, 4) == []
    # a frame is due by plan_frames' rule, for every slot on its own
    for r in range(0, 4 * P):
        for fin in (False, True):
            one = E.plan_frames(r, 0, L, P, fin, 1)
            assert [it[1:] for launch in E.plan_pool([r], [0], [fin], [True], L, P, 64) for it in launch] == \
                   [(f0, start, valid) for (f0, _, start, valid) in one]
    for bad in (dict(max_rows=0), dict(pool_stride=0), dict(received=[-1]), dict(emitted=[9]), dict(limit=[-1]),
                dict(final=[True, False])):
        kw = dict(dict(received=[100], emitted=[0], final=[False], active=[True], nlayers=L, pool_stride=P, max_rows=4), **bad)
        with pytest.raises(ValueError):
            E.plan_pool(**kw)


# ---- C-ABI -------------------------------------------------------------------------------------------------------------
NAMES = ("srwn_nc_encode_frame_list", "srwn_nc_encode_list_partials", "srwn_audio_ring_put")


def test_symbols_are_declared_listed_and_bound_by_both_bindings():
    L = sub("_lib")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared in srwn.h"
        assert name in L.SIGNATURES and '"%s"' % name in src
        for binding in ("pybind11", "ctypes"):
            assert callable(getattr(L.bind(binding), name)), (binding, name)
    assert "typedef struct SrwnEncFrame" in txt
    import ctypes
    assert ctypes.sizeof(L.SrwnEncFrame) == 16 and [f[0] for f in L.SrwnEncFrame._fields_] == ["stream", "col", "valid", "reserved"]
    assert L.load().srwn_version() >= 111
    B = sub("build")
    assert any("NcListArgs" in k for k in B.NO_SPILL["srwn_ncstream.hip"])      # the list instantiation is held to no scratch


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    L = sub("_lib")
    lib = L.bind(binding)
    assert lib.srwn_version() >= 111
    names = ["ring", "ring_len", "capacity", "frames", "nitems", "nc_w", "nc_b", "nc_wr", "nc_br", "wconv", "wconv_stride",
             "wres", "wres_stride", "bias_c", "bias_r", "partials", "means", "pool", "L", "C", "K", "dtype", "stream"]
    ok = dict(ring=1, ring_len=543, capacity=4, frames=1, nitems=3, nc_w=1, nc_b=1, nc_wr=1, nc_br=1, wconv=1,
              wconv_stride=49152, wres=1, wres_stride=49152, bias_c=1, bias_r=1, partials=1, means=1, pool=512, L=30, C=128,
              K=2, dtype=L.BF16, stream=None)
    run = lambda **kw: lib.srwn_nc_encode_frame_list(*[dict(ok, **kw)[n] for n in names])
    assert run(nitems=0) == 0                                     # empty work returns before any launch
    for p in ("ring", "frames", "nc_w", "nc_b", "nc_wr", "nc_br", "wconv", "wres", "bias_c", "bias_r", "partials", "means"):
        assert run(**{p: None}) == E_NULL, p
        assert b"null" in lib.srwn_last_error()
    assert run(ring_len=542) == E_SHAPE                           # a ring shorter than one frame's window
    assert b"ring_len" in lib.srwn_last_error()
    assert run(nitems=-1) == E_SHAPE and run(capacity=0) == E_SHAPE and run(pool=0) == E_SHAPE
    assert run(L=33) == E_SHAPE and run(L=0) == E_SHAPE
    assert b"layers" in lib.srwn_last_error()
    assert run(C=64) == E_UNSUPPORTED and run(K=3) == E_UNSUPPORTED and run(dtype=L.F32) == E_UNSUPPORTED
    assert run(dtype=7) == E_DTYPE
    assert lib.srwn_nc_encode_list_partials(5, 512, 30) == 6 * 30 * 5 * 128 == lib.srwn_nc_encode_partials(1, 5, 512, 30)
    assert lib.srwn_nc_encode_list_partials(-1, 512, 30) == 0

    def put(ring=1, ring_len=100, capacity=4, src=1, streams=1, off=1, col=1, counts=1, n=2, max_count=50):
        return lib.srwn_audio_ring_put(ring, ring_len, capacity, src, streams, off, col, counts, n, max_count, None)
    assert put(n=0) == 0 and put(max_count=0) == 0
    for p in ("ring", "src", "streams", "off", "col", "counts"):
        assert put(**{p: None}) == E_NULL, p
        assert b"null" in lib.srwn_last_error()
    assert put(ring_len=0) == E_SHAPE and put(capacity=0) == E_SHAPE and put(n=-1) == E_SHAPE and put(max_count=-1) == E_SHAPE
    assert put(max_count=101) == E_SHAPE                          # more at once than a ring holds
    assert b"audio_ring_put" in lib.srwn_last_error()


# ---- refusals come first -------------------------------------------------------------------------------------------------
def _bare(cls, **attrs):
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _bare_pool(E, capacity=3, P=16, L=5, ring=40):
    return _bare(E.EncoderPool, fe=None, P=P, L=L, lat=4, capacity=capacity, window=P + L + 1, audio_ring=ring, max_rows=8,
                 _received=np.zeros(capacity, np.int64), _emitted=np.zeros(capacity, np.int64),
                 _final=np.zeros(capacity, bool), _active=np.zeros(capacity, bool), ring=None, stage=None, table=None)


def _state(p):
    return (p._received.tolist(), p._emitted.tolist(), p._final.tolist(), p._active.tolist())


def test_encoder_pool_refuses_first():
    import torch
    E = sub("encoder")
    fe = _bare(E.FrameEncoder, max_batch=3, max_frames=4, P=16, L=5, lat=4, w=None)
    with pytest.raises(ValueError, match="audio_ring"):
        fe.pool(audio_ring=16 + 5)                                # one sample short of a frame's window
    for bad in (0, 13):
        with pytest.raises(ValueError, match="max_rows"):
            fe.pool(max_rows=bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
            fe.pool()
    p = _bare_pool(E)
    assert p.free == [0, 1, 2] and p.active == []
    with pytest.raises(ValueError, match="free slots"):
        p.join(4)
    with pytest.raises(ValueError, match="outside"):
        p.join(slots=[3])
    assert p.join(2) == [0, 1] and p.join(slots=[2]) == [2] and p.active == [0, 1, 2]
    with pytest.raises(ValueError, match="not all free"):
        p.join(slots=[1])
    p.leave([1, 2])
    p._received[0], p._emitted[0] = 30, 1                         # 14 samples held: room for 26
    assert p.audio_room(0) == 26 and p.audio_room(1) == 40
    before = _state(p)
    x = np.zeros(10, np.float32)
    for slots, audio, what in (([1], [x], "holds no stream"), ([0], [np.zeros(27, np.float32)], "room for 26"),
                               ([0], [np.zeros(10, np.int32)], "floating"), ([0], [torch.zeros(10, dtype=torch.int64)], "floating"),
                               ([0], [np.zeros((2, 5), np.float32)], "1-D"), ([0, 0], [x, x], "distinct"),
                               ([0, 2], [x], "2 slots but 1"), ([5], [x], "outside"), (1, x, "holds no stream")):
        with pytest.raises(ValueError, match=what):
            p.push(slots, audio)
        assert _state(p) == before
    with pytest.raises(ValueError, match="do not all hold"):
        p.finish([0, 1])
    assert _state(p) == before
    p.finish(0)
    with pytest.raises(ValueError, match="was finished"):
        p.push([0], [x])
    p.leave(0)
    assert p.active == [] and p.join() == [0] and (p._received[0], p._emitted[0], p._final[0]) == (0, 0, False)
    assert p.step() == {}                                         # nothing due: nothing is launched (no device here)
    p.push([0], [np.zeros(0, np.float32)])                        # nothing in: no upload, no launch
    assert p._received[0] == 0


def test_faces_refuse_first_and_have_no_cpu_fallback():
    import torch
    M, E = sub("model"), sub("encoder")
    if not torch.cuda.is_available():
        for call in (lambda: M.AudioEncoder.pool(None), lambda: M.Resynthesizer.pool(None)):
            with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
                call()
    syn = SimpleNamespace(max_chunk=100, max_frames=3, max_batch=2, condition_size=3, _eng=SimpleNamespace(hist=[31, 224]))
    owner = SimpleNamespace(encoder=SimpleNamespace(max_batch=4), synthesizer=syn, pool_stride=64)
    for chunk in (0, 101):
        with pytest.raises(ValueError, match="chunk_size"):
            M.ResynthesisPool(owner, chunk, None)
    with pytest.raises(ValueError, match="max_frames >= 5"):      # ceil(224 / 64) + 1
        M.ResynthesisPool(owner, 50, None)
    ep = _bare_pool(E, capacity=2)
    rp = _bare(M.ResynthesisPool, capacity=2, _cs=3, _chunk=50, _enc=ep, _syn=None, _cond={})
    assert rp.step() == {} and rp.active == [] and rp.free == [0, 1]
    with pytest.raises(ValueError, match="free slots"):
        rp.join(np.zeros((3, 3)), n=3)
    with pytest.raises(ValueError, match="condition_size"):
        rp.join()
    with pytest.raises(ValueError, match=r"\[2, 3\]"):
        rp.join(np.zeros((2, 4)), n=2)
    for call in (lambda: rp.push([0], [np.zeros(4, np.float32)]), lambda: rp.finish(0), lambda: rp.leave([1])):
        with pytest.raises(ValueError, match="do not all hold a stream"):
            call()
    assert rp._cond == {} and _state(ep) == ([0, 0], [0, 0], [False, False], [False, False])
    rp._cond[0] = None
    ep.join(slots=[0])
    with pytest.raises(ValueError, match="room for 40"):
        rp.push(0, np.zeros(41, np.float32))
    assert rp.audio_room(0) == 40 and rp.received.tolist() == [0, 0]
    face = M.AudioEncoderPool(ep)
    with pytest.raises(ValueError, match="floating"):
        face.push([0], [np.zeros(3, np.int16)])
    with pytest.raises(ValueError, match="holds no stream"):
        face.push(1, np.zeros(3, np.float32))
    assert face.active == [0] and face.free == [1] and face.capacity == 2 and face.audio_room(0) == 40 and face.step() == {}
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dropin_model", os.path.join(ROOT, "sr-wavenet_amd", "dropin", "model.py"))
    d = importlib.util.module_from_spec(spec); spec.loader.exec_module(d)
    assert hasattr(d.AudioEncoder, "pool") and hasattr(d.Resynthesizer, "pool")
