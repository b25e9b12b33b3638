"""CPU tests of scorer pools (srwn_version() 118; scorer.plan_score_pool_step, scorer.ScorerPool): the step plan against
brute force and a drained ragged session, the audio ring's room and everything the pool refuses before it touches the
device, and what the three new entry points of the library refuse.  No GPU: the pools are built without their constructors,
and no call gets as far as a launch."""
import os
import re

import numpy as np
import pytest

from tests._pkg import ROOT, sub

NEW = ["srwn_score_stream_in_slots", "srwn_stream_score_head_slots", "srwn_nll_rows_slots"]
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _bare(cls, **attrs):
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _bare_pool(S_, capacity=3, max_chunk=32, ring=None):
    import torch
    ring = 2 * max_chunk + 2 if ring is None else ring
    return _bare(S_.ScorerPool, c=None, capacity=capacity, max_chunk=max_chunk, audio_ring=ring,
                 _received=np.zeros(capacity, np.int64), _scored=np.zeros(capacity, np.int64),
                 _nll_sum=torch.zeros(capacity, dtype=torch.float64), _active=np.zeros(capacity, bool), ring=None, stage=None,
                 table=None, _graphs={}, _seen=set(), _open=True)


def _state(p):
    return (p._received.tolist(), p._scored.tolist(), p._active.tolist())


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_plan_against_brute_force():
    S_ = sub("scorer")
    rng = np.random.default_rng(0)
    for trial in range(400):
        cap = int(rng.integers(1, 9))
        mc = int(rng.choice([1, 5, 31, 32, 33, 64, 100, 128, 1600]))
        scored = rng.integers(0, 5000, cap)
        received = scored + rng.integers(0, 3 * mc + 2, cap) * (rng.random(cap) < 0.8)
        active = rng.random(cap) < 0.7
        n, rows = S_.plan_score_pool_step(received, scored, active, mc)
        assert rows.shape == (cap,) and rows.dtype == np.int64
        waits = False
        for u in range(cap):
            w = 0                                              # brute force: one sample at a time
            while active[u] and w < mc and scored[u] + w < received[u]:
                w += 1
            assert rows[u] == w and rows[u] <= received[u] - scored[u] and rows[u] <= mc
            assert active[u] or rows[u] == 0
            waits = waits or w > 0
        assert (n == 0) == (not waits)
        assert n % 32 == 0 or n == mc
        assert rows.max() <= n <= mc
        assert n < rows.max() + 32                             # the least such n: no launch over rows nobody has
    n, rows = S_.plan_score_pool_step([400, 400], [0, 0], [False, False], 64)
    assert n == 0 and rows.tolist() == [0, 0]
    assert S_.plan_score_pool_step([], [], [], 64)[0] == 0
    n, rows = S_.plan_score_pool_step([1000, 41, 7], [40, 40, 7], [True, True, True], 100)
    assert n == 100 and rows.tolist() == [100, 1, 0]
    assert S_.plan_score_pool_step([33, 0], [0, 0], [True, True], 128)[0] == 64
    assert S_.plan_score_pool_step([1, 0], [0, 0], [True, True], 20)[0] == 20          # capped at max_chunk
    for bad in (lambda: S_.plan_score_pool_step([1], [0], [True], 0), lambda: S_.plan_score_pool_step([1, 2], [0], [True], 1),
                lambda: S_.plan_score_pool_step([1], [2], [True], 1), lambda: S_.plan_score_pool_step([1], [-1], [True], 1)):
        with pytest.raises(ValueError, match="plan_score_pool_step"):
            bad()


@pytest.mark.parametrize("mc", [1, 32, 50, 128])
def test_repeated_planning_drains_every_slot(mc):
    """Streams of different lengths arrive in random pieces; the plan alone scores every sample of every active stream
    exactly once, in order, in at most ceil(max_chunk / 32) different launch sizes."""
    S_ = sub("scorer")
    rng = np.random.default_rng(mc)
    cap, ring = 4, 2 * mc + 2
    lengths = [300, 1, 131, 517, 64, 0, int(rng.integers(0, 6 * mc + 1))]
    received, scored = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
    active = np.zeros(cap, bool)
    stream_of, sent, done, waiting, sizes = {}, {}, {}, list(range(len(lengths))), set()
    for rnd in range(100000):
        if not waiting and not active.any():
            break
        if waiting and (~active).any() and rng.random() < 0.5:
            u = int(np.flatnonzero(~active)[0])
            s = waiting.pop(0)
            stream_of[u], sent[s] = s, 0
            received[u] = scored[u] = 0
            active[u] = True
        for u in np.flatnonzero(active):
            s = stream_of[int(u)]
            room = ring - 2 - (received[u] - scored[u])
            k = int(min(rng.integers(0, 2 * mc + 2), room, lengths[s] - sent[s]))
            received[u] += k
            sent[s] += k
        while True:                                            # ScorerPool.step's loop
            n, rows = S_.plan_score_pool_step(received, scored, active, mc)
            if n == 0:
                break
            sizes.add(n)
            assert rows.max() >= 1
            scored += rows
            assert np.all(scored <= received)
        assert np.all(scored[active] == received[active])      # a step leaves nothing waiting
        for u in np.flatnonzero(active):
            s = stream_of[int(u)]
            if sent[s] == lengths[s]:
                done[s] = int(scored[u])
                active[u] = False
    assert done == dict(enumerate(lengths))
    assert len(sizes) <= (mc + 31) // 32 and all(n % 32 == 0 or n == mc for n in sizes)


# ---- the pool's refusals and its room ----------------------------------------------------------------------------------------
def test_pool_refuses_first():
    import torch
    S_ = sub("scorer")
    sc = _bare(S_.StreamScorer, max_batch=3, max_chunk=32, _pool=None, _state=None, _serial=0)
    with pytest.raises(ValueError, match="audio_ring"):
        sc.pool(audio_ring=33)                                       # one sample short of max_chunk + 2
    assert sc._pool is None and sc._serial == 0                      # a refused pool ends nothing
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sc.pool(audio_ring=34)
    p = _bare_pool(S_)
    assert p.free == [0, 1, 2] and p.active == [] and p.audio_ring == 66
    with pytest.raises(ValueError, match="free slots"):
        p.join(4)                                                    # (refused before the reset launch)
    with pytest.raises(ValueError, match="outside"):
        p.join(slots=[3])
    p._active[:] = [True, False, True]
    with pytest.raises(ValueError, match="not all free"):
        p.join(slots=[1, 2])
    p._received[0], p._scored[0] = 30, 24                            # 6 samples wait: 66 - 2 - 6
    assert p.audio_room(0) == 58 and p.audio_room(1) == 64
    assert np.isnan(p.bits_per_sample(1))
    p._nll_sum[0] = 24 * np.log(256.0)
    assert abs(p.bits_per_sample(0) - 8.0) < 1e-12
    before = _state(p)
    x = np.zeros(10, np.float32)
    for slots, audio, what in (([1], [x], "holds no stream"), (1, x, "holds no stream"),
                               ([0], [np.zeros(59, np.float32)], "room for 58"), ([0], [np.zeros(10, np.int16)], "floating"),
                               ([0], [np.zeros((2, 5), np.float32)], "1-D"), ([0, 0], [x, x], "not distinct"),
                               ([0, 2], [x], "2 slots but 1"), ([5], [x], "outside")):
        with pytest.raises(ValueError, match=what):
            p.push(slots, audio)
        assert _state(p) == before
    p._received[0] = 24                                              # nothing waits any more
    p.push([0, 2], [np.zeros(0, np.float32), np.zeros(0, np.float64)])      # nothing to upload: no device work
    assert p.step() == {} and p.step(return_logits=True, return_best=True) == ({}, {}, {}) and p.step(return_best=True) == ({}, {})
    assert p.received.tolist() == [24, 0, 0] and p.scored.tolist() == [24, 0, 0]
    p.leave([0, 1])
    assert p.active == [2]
    p._open = False
    for call in (lambda: p.join(), lambda: p.leave(2), lambda: p.push(2, x), lambda: p.step()):
        with pytest.raises(ValueError, match="closed"):
            call()
    M = sub("model")
    face = M.ScorerStreamPool(_bare_pool(S_))
    face._pool._active[0] = True
    with pytest.raises(ValueError, match="floating"):
        face.push([0], [np.zeros(3, np.int16)])
    with pytest.raises(ValueError, match="holds no stream"):
        face.push(1, np.zeros(3, np.float32))
    assert face.active == [0] and face.free == [1, 2] and face.capacity == 3 and face.audio_room(0) == 64
    assert face.step() == {} and face.received.tolist() == [0, 0, 0] and face.scored.tolist() == [0, 0, 0]
    assert np.isnan(face.bits_per_sample(0)) and face.audio_ring == 66
    for name in ("pool",):
        assert callable(getattr(M.StreamingScorer, name)) and callable(getattr(S_.StreamScorer, name))


def test_audio_room_keeps_the_two_samples_before_the_chunk():
    """A push of at most audio_room samples writes neither a sample that still waits nor the columns of the samples scored
    - 1 and scored - 2, the entry conv's taps before the next chunk -- through a whole random session of one slot."""
    S_ = sub("scorer")
    rng = np.random.default_rng(5)
    for mc, ring in ((32, 34), (32, 66), (5, 9), (1, 3)):
        p = _bare_pool(S_, capacity=1, max_chunk=mc, ring=ring)
        p._active[0] = True
        held = {}                                                    # ring column -> the sample it holds
        for rnd in range(400):
            room = p.audio_room(0)
            assert 0 <= room <= ring - 2
            n = int(rng.integers(0, room + 1)) if rnd % 7 else room  # (every seventh push fills the ring)
            r0, c0 = int(p._received[0]), int(p._scored[0])
            live = set(range(max(c0 - 2, 0), r0))                    # samples a later step still reads
            for s in range(r0, r0 + n):
                assert held.get(s % ring) not in live, (mc, ring, s)
                held[s % ring] = s
            p._received[0] += n
            k, rows = S_.plan_score_pool_step(p._received, p._scored, p._active, mc)
            if rnd % 3 == 0:                                         # (not every round steps: audio piles up to the ring's end)
                t0, t1 = int(p._scored[0]), int(p._scored[0] + rows[0])
                for s in range(max(t0 - 2, 0), t1):                  # what the step's entry reads is what was pushed
                    assert held[s % ring] == s
                p._scored[0] = t1
        assert p._received[0] > 20 * ring                            # the ring wrapped many times


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
    assert "srwn_version() 118" in raw


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_slot_argument_errors_do_not_need_a_gpu(binding):
    from tests.test_scorer import _lib
    lib = _lib(binding)
    assert lib.srwn_version() >= 118

    def named(entry):
        return lib.srwn_last_error().startswith(entry + b":")

    def entry(ring=A, ring_len=66, out=A, rows=31 + 64, hist=31, codes=A, cstride=64, cap=2, n=40, mc=64, R=32, C=256, dt=7,
              slots=A):
        # (dt = 7 by default: a call whose other arguments are all good ends at the dtype check, before any launch)
        return lib.srwn_score_stream_in_slots(ring, ring_len, A, A, out, rows, hist, codes, cstride, cap, n, mc, R, C, dt, slots,
                                              None)

    assert entry() == E_DTYPE and named(b"score_stream_in_slots")
    assert entry(cap=0) == 0 and entry(n=0) == 0                   # empty work is done
    assert entry(n=0, ring=None, R=48, dt=7) == 0                  # ... before anything else is looked at
    for name in ("ring", "out", "codes", "slots"):
        assert entry(**{name: None}) == E_NULL, name
    assert entry(R=48) == E_UNSUPPORTED
    assert entry(C=257) == E_UNSUPPORTED and entry(C=1) == E_UNSUPPORTED
    assert entry(C=100) == E_DTYPE and entry(C=2) == E_DTYPE
    assert entry(n=65) == E_SHAPE
    assert entry(n=-1) == E_SHAPE and entry(cap=-1) == E_SHAPE
    assert entry(rows=64) == E_SHAPE
    assert entry(cstride=63) == E_SHAPE
    assert entry(ring_len=65) == E_SHAPE                           # max_chunk + 1 samples: no room for a[t - 2] beside a whole chunk
    assert b"max_chunk + 2 = 66" in lib.srwn_last_error() and named(b"score_stream_in_slots")
    assert entry(slots=None, R=48) == E_NULL and entry(R=48, n=65) == E_UNSUPPORTED and entry(n=65, dt=1) == E_SHAPE

    def head(z=A, zst=2 * 64 * 32, zrows=64, L=3, w2=A, codes=A, nll=A, best=None, lo=None, ostride=64, cap=2, n=40, mc=64,
             R=32, S=128, C=256, dt=7, slots=A):
        return lib.srwn_stream_score_head_slots(z, zst, zrows, L, A, A, A, A, w2, A, codes, nll, best, lo, ostride, cap, n, mc,
                                                R, S, C, dt, slots, None)

    assert head() == E_DTYPE and named(b"stream_score_head_slots")
    assert head(best=A, lo=A) == E_DTYPE
    assert head(cap=0) == 0 and head(n=0) == 0 and head(n=0, z=None) == 0
    for name in ("z", "w2", "codes", "nll", "slots"):
        assert head(**{name: None}) == E_NULL, name
    assert head(R=48) == E_UNSUPPORTED and head(S=192) == E_UNSUPPORTED
    assert head(C=0) == E_UNSUPPORTED and head(C=257) == E_UNSUPPORTED
    assert head(C=1) == E_DTYPE and head(C=100) == E_DTYPE
    assert head(n=65) == E_SHAPE and head(n=-3) == E_SHAPE and head(cap=-1) == E_SHAPE
    assert head(zrows=32) == E_SHAPE and head(ostride=39) == E_SHAPE and head(zst=100) == E_SHAPE and head(L=0) == E_SHAPE
    assert named(b"stream_score_head_slots")

    def rows(logits=A, ld=128, crows=64, codes=A, nll=A, ostride=64, cap=2, n=40, C=100, slots=A):
        return lib.srwn_nll_rows_slots(logits, ld, crows, codes, nll, None, None, ostride, cap, n, C, slots, None)

    assert rows(cap=0) == 0 and rows(n=0) == 0 and rows(n=0, logits=None) == 0
    for name in ("logits", "codes", "nll", "slots"):
        assert rows(**{name: None}) == E_NULL, name
    assert named(b"nll_rows_slots")
    assert rows(C=0) == E_UNSUPPORTED and rows(C=257, ld=512) == E_UNSUPPORTED
    assert rows(ld=96) == E_SHAPE and rows(crows=39) == E_SHAPE and rows(ostride=39) == E_SHAPE
    assert rows(n=-1) == E_SHAPE and rows(cap=-2) == E_SHAPE
    assert named(b"nll_rows_slots")


# ---- a whole pool step on host memory: the launch list, the table and what step returns ------------------------------------
from tests.test_stream_stack import NAMES, Weights, _check_kinds, calls      # noqa: E402,F401  (the recorder in _lib.call's place)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twin"])
def test_pool_step_launch_list_on_host_memory(calls, monkeypatch, fused):
    """``_lib.call`` is a recorder and the weights are stand-ins on host memory: a pool step is the scorer's ONE launch list
    in its slot forms on the table uploaded for the pass, and step's dicts hold each slot's own rows."""
    import torch
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1" if fused else "0")
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    monkeypatch.setattr(sub("audio_ring"), "call", lambda name, *args: calls.append((name, args)))      # (the pool's push)
    S_ = sub("scorer")
    cap, mc = 3, 48
    s = S_.StreamScorer(Weights(), max_batch=cap, max_chunk=mc)
    st = s.start(2)
    pool = s.pool()
    assert s._state is None and s._pool is pool and pool.audio_ring == 2 * mc + 2 and pool.capacity == cap
    with pytest.raises(ValueError, match="current"):
        s.push(st, np.zeros((2, 4), np.float32))
    assert pool.join(2) == [0, 1] and [n for n, _ in calls] == ["srwn_flow_stream_reset_slots"]
    pool.push([0, 1], [np.zeros(70, np.float32), np.zeros(5, np.float32)])
    assert [n for n, _ in calls][1:] == ["srwn_audio_ring_put"] and pool.audio_room(0) == 2 * mc - 70
    del calls[:]
    out = pool.step(return_best=True)
    G = len(s.groups)
    head = ["srwn_stream_score_head_slots"] if fused else ["srwn_pw_linear"] * 3 + ["srwn_nll_rows_slots"]
    one = ["srwn_score_stream_in_slots"] + [NAMES[True, True]] * G + head + ["srwn_recog_roll_slots"]
    assert [n for n, _ in calls] == one * 2 and len(one) == pool.launches_per_step == s.launches_per_step
    for name, args in calls:
        _check_kinds(name, args)
    table = pool.table.data_ptr()
    rows = [a[10] for n, a in calls if n == "srwn_score_stream_in_slots"]
    assert rows == [48, 32]                                    # 48 = max_chunk, then 22 left: rounded up to 32
    for name, a in calls:
        if name == "srwn_score_stream_in_slots":
            assert a[:2] == (pool.ring.data_ptr(), pool.audio_ring) and a[7:10] == (s.codes.data_ptr(), mc, cap) and a[-2] == table
        elif name in (NAMES[True, True], "srwn_stream_score_head_slots", "srwn_nll_rows_slots", "srwn_recog_roll_slots"):
            assert table in a, name
    assert pool.table.tolist() == [[48, 70], [5, 5], [0, 0]]   # the second pass's table: nothing advanced it but the host
    assert isinstance(out, tuple) and len(out) == 2 and set(out[0]) == {0, 1} == set(out[1])
    assert out[0][0].shape == (70,) and out[0][1].shape == (5,) and out[1][0].dtype == torch.int32
    assert pool.scored.tolist() == [70, 5, 0] and pool.step() == {} and len(calls) == 2 * len(one)
    assert pool.nll_sum.tolist() == [0.0, 0.0, 0.0] and pool.bits_per_sample(0) == 0.0 and np.isnan(pool.bits_per_sample(2))
    lg = pool.step(return_logits=True)
    assert lg == ({}, {}) and s.logits_out is None             # nothing waited: nothing allocated, nothing launched
    s.start(1)                                                  # start() closes the pool
    with pytest.raises(ValueError, match="closed"):
        pool.step()
    assert s._pool is None
