"""CPU tests of the classifier pool's host side (recognizer.plan_pool_step, recognizer.ClassifierPool): the step plan
against brute force, a simulated ragged session through the plan and ``emissions_due``, everything the pool refuses before
it touches the device, the audio ring's room, and what the five slot entry points of the library refuse.  No GPU: the
pools are built without their constructors, and no call gets as far as a launch."""
import numpy as np
import pytest

from tests._pkg import sub


def _bare(cls, **attrs):
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _bare_pool(R_, capacity=3, hop=8, window=32, max_hops=4, ring=None):
    ring = 2 * max_hops * hop + 1 if ring is None else ring
    return _bare(R_.ClassifierPool, c=None, capacity=capacity, hop=hop, window=window, max_hops=max_hops, audio_ring=ring,
                 _received=np.zeros(capacity, np.int64), _consumed=np.zeros(capacity, np.int64),
                 _emitted=np.zeros(capacity, np.int64), _active=np.zeros(capacity, bool), ring=None, stage=None, table=None,
                 _graphs={}, _seen=set(), _open=True)


def _state(p):
    return (p._received.tolist(), p._consumed.tolist(), p._emitted.tolist(), p._active.tolist())


def _brute(received, consumed, active, hop, max_hops):
    hops = []
    for r, c, a in zip(received, consumed, active):
        h = 0
        while a and h < max_hops and c + (h + 1) * hop <= r:
            h += 1
        hops.append(h)
    return max(hops, default=0), hops


def test_plan_pool_step_against_brute_force():
    R_ = sub("recognizer")
    rng = np.random.default_rng(0)
    for trial in range(300):
        cap = int(rng.integers(1, 9))
        hop = int(rng.choice([1, 3, 40, 160]))
        max_hops = int(rng.integers(1, 9))
        consumed = rng.integers(0, 50, cap) * hop
        received = consumed + rng.integers(0, 3 * max_hops * hop + 2, cap)
        active = rng.random(cap) < 0.7
        k, hops = R_.plan_pool_step(received, consumed, active, hop, max_hops)
        wk, wh = _brute(received, consumed, active, hop, max_hops)
        assert k == wk and hops.tolist() == wh and hops.shape == (cap,)
    # all slots idle: nothing waits, or nobody is active
    assert R_.plan_pool_step([5, 39], [0, 0], [True, True], 40, 4)[0] == 0
    k, hops = R_.plan_pool_step([400, 400], [0, 0], [False, False], 40, 4)
    assert k == 0 and hops.tolist() == [0, 0]
    # one slot with more than max_hops hops waiting is cut at max_hops; its neighbour takes what it has
    k, hops = R_.plan_pool_step([1000, 85, 0], [40, 40, 0], [True, True, True], 40, 4)
    assert k == 4 and hops.tolist() == [4, 1, 0]
    # hop = 1: every sample is a hop
    k, hops = R_.plan_pool_step([7, 2, 9], [7, 0, 3], [True, True, False], 1, 3)
    assert k == 2 and hops.tolist() == [0, 2, 0]
    for bad in (lambda: R_.plan_pool_step([1], [0], [True], 0, 1), lambda: R_.plan_pool_step([1], [0], [True], 1, 0),
                lambda: R_.plan_pool_step([1, 2], [0], [True], 1, 1), lambda: R_.plan_pool_step([1], [2], [True], 1, 1)):
        with pytest.raises(ValueError, match="plan_pool_step"):
            bad()


@pytest.mark.parametrize("hop,window,max_hops", [(32, 128, 4), (40, 320, 8), (1, 5, 3), (160, 160, 1)])
def test_simulated_ragged_session(hop, window, max_hops):
    """Streams of different lengths arrive in random pieces and at different times; the plan and emissions_due alone carry
    every stream to max(0, T // hop - window // hop + 1) emissions, and consumed never passes received."""
    R_ = sub("recognizer")
    rng = np.random.default_rng(hop + window)
    cap = 4
    lengths = [int(v) for v in (window - 1, window, 3 * window + hop // 2, rng.integers(0, 6 * window), 5 * window + 1,
                                rng.integers(0, 6 * window))]
    ring = 2 * max_hops * hop + 1
    received, consumed, emitted = (np.zeros(cap, np.int64) for _ in range(3))
    active = np.zeros(cap, bool)
    stream_of, sent, done, waiting = {}, {}, {}, list(range(len(lengths)))
    for rnd in range(100000):
        if not waiting and not active.any():
            break
        if waiting and (~active).any() and rng.random() < 0.5:      # a stream joins a free slot
            u = int(np.flatnonzero(~active)[0])
            s = waiting.pop(0)
            stream_of[u], sent[s] = s, 0
            received[u] = consumed[u] = emitted[u] = 0
            active[u] = True
        for u in np.flatnonzero(active):                             # pieces of whatever length fits
            s = stream_of[int(u)]
            room = ring - 1 - (received[u] - consumed[u])
            n = int(min(rng.integers(0, 2 * max_hops * hop + 2), room, lengths[s] - sent[s]))
            received[u] += n
            sent[s] += n
        while True:                                                  # ClassifierPool.step's loop
            k, hops = R_.plan_pool_step(received, consumed, active, hop, max_hops)
            if k == 0:
                break
            assert 1 <= k <= max_hops and hops.max() == k
            for u in np.flatnonzero(hops):
                first, count = R_.emissions_due(consumed[u], consumed[u] + hops[u] * hop, hop, window)
                assert count <= hops[u] and (count == 0 or first + count == consumed[u] // hop + hops[u])
                emitted[u] += count
            consumed += hops * hop
            assert np.all(consumed <= received) and np.all(consumed % hop == 0)
        for u in np.flatnonzero(active):                             # a stream whose audio is all in and heard leaves
            s = stream_of[int(u)]
            if sent[s] == lengths[s]:
                assert received[u] - consumed[u] < hop
                done[s] = int(emitted[u])
                active[u] = False
    assert done == {s: max(0, T // hop - window // hop + 1) for s, T in enumerate(lengths)}


def test_pool_refuses_first():
    import torch
    R_ = sub("recognizer")
    sc = _bare(R_.StreamClassifier, max_batch=3, hop=8, window=32, max_hops=4, max_chunk=32, _pool=None, _state=None, _serial=0)
    with pytest.raises(ValueError, match="audio_ring"):
        sc.pool(audio_ring=32)                                       # one sample short of max_chunk + 1
    assert sc._pool is None and sc._serial == 0                      # a refused pool ends nothing
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sc.pool(audio_ring=33)
    p = _bare_pool(R_)
    assert p.free == [0, 1, 2] and p.active == [] and p.audio_ring == 65
    with pytest.raises(ValueError, match="free slots"):
        p.join(4)                                                    # (refused before the reset launch)
    with pytest.raises(ValueError, match="outside"):
        p.join(slots=[3])
    with pytest.raises(ValueError, match="not distinct"):
        p.join(slots=[1, 1])
    p._active[:] = [True, False, True]
    with pytest.raises(ValueError, match="not all free"):
        p.join(slots=[1, 2])
    with pytest.raises(ValueError, match="1 free slots"):
        p.join(2)
    p._received[0], p._consumed[0] = 30, 24                          # 6 samples wait, no whole hop: 65 - 1 - 6
    assert p.audio_room(0) == 58 and p.audio_room(1) == 64
    before = _state(p)
    x = np.zeros(10, np.float32)
    for slots, audio, what in (([1], [x], "holds no stream"), (1, x, "holds no stream"),
                               ([0], [np.zeros(59, np.float32)], "room for 58"), ([0], [np.zeros(10, np.int16)], "floating"),
                               ([0], [torch.zeros(10, dtype=torch.int64)], "floating"),
                               ([0], [np.zeros((2, 5), np.float32)], "1-D"), ([0, 0], [x, x], "not distinct"),
                               ([0, 2], [x], "2 slots but 1"), ([5], [x], "outside")):
        with pytest.raises(ValueError, match=what):
            p.push(slots, audio)
        assert _state(p) == before
    p.push([0, 2], [np.zeros(0, np.float32), np.zeros(0, np.float64)])      # nothing to upload: no device work
    assert _state(p) == before and p.step() == {} and p.step(return_logits=True) == ({}, {})
    p.leave([0, 1])
    assert p.active == [2]
    p._open = False
    for call in (lambda: p.join(), lambda: p.leave(2), lambda: p.push(2, x), lambda: p.step()):
        with pytest.raises(ValueError, match="closed"):
            call()
    M = sub("model")
    face = M.ClassifierPool(_bare_pool(R_))
    face._pool._active[0] = True
    with pytest.raises(ValueError, match="floating"):
        face.push([0], [np.zeros(3, np.int16)])
    with pytest.raises(ValueError, match="holds no stream"):
        face.push(1, np.zeros(3, np.float32))
    assert face.active == [0] and face.free == [1, 2] and face.capacity == 3 and face.audio_room(0) == 64
    assert face.step() == {} and face.received.tolist() == [0, 0, 0]


def test_audio_room_keeps_the_sample_before_the_chunk():
    """A push of at most audio_room samples writes neither a sample that still waits nor column (consumed - 1) mod
    audio_ring, the input conv's tap before the next chunk -- through a whole random session of one slot."""
    R_ = sub("recognizer")
    rng = np.random.default_rng(5)
    for hop, max_hops, ring in ((8, 4, 33), (8, 4, 65), (5, 3, 40), (1, 2, 3)):
        p = _bare_pool(R_, capacity=1, hop=hop, window=hop, max_hops=max_hops, ring=ring)
        p._active[0] = True
        held = {}                                                    # ring column -> the sample it holds
        for rnd in range(400):
            room = p.audio_room(0)
            assert 0 <= room <= ring - 1
            n = int(rng.integers(0, room + 1)) if rnd % 7 else room  # (every seventh push fills the ring)
            r0, c0 = int(p._received[0]), int(p._consumed[0])
            live = set(range(max(c0 - 1, 0), r0))                    # samples a later step still reads
            for s in range(r0, r0 + n):
                assert held.get(s % ring) not in live, (hop, ring, s)
                held[s % ring] = s
            p._received[0] += n
            k, hops = R_.plan_pool_step(p._received, p._consumed, p._active, hop, max_hops)
            t0, t1 = int(p._consumed[0]), int(p._consumed[0] + hops[0] * hop)
            for s in range(max(t0 - 1, 0), t1):                      # what the step's input conv reads is what was pushed
                assert held[s % ring] == s
            p._consumed[0] = t1
        assert p._received[0] > 20 * ring                            # the ring wrapped many times


# ---- the slot forms' refusals ------------------------------------------------------------------------------------------
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths this test takes


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_slot_argument_errors_do_not_need_a_gpu(binding):
    """The five slot entry points refuse what test_recognizer's test_argument_errors_do_not_need_a_gpu has the clock forms
    refuse, the table in the place of the clock, and what only they can be given wrong; every message names the slot
    entry."""
    from tests.test_recognizer import _lib
    lib = _lib(binding)

    def named(entry):      # the last refusal came from `entry` itself, not from its clock form
        return lib.srwn_last_error().startswith(entry + b":")

    def head(z=A, zst=2 * 64 * 32, zrows=64, L=3, ring=A, rr=5, slots=A, cap=2, k=2, hop=32, mc=64, R=32, S=128, dt=1):
        return lib.srwn_pooled_stream_head_slots(z, zst, zrows, L, A, A, A, A, ring, rr, slots, cap, k, hop, mc, R, S, dt, None)

    assert head(z=None) == E_NULL
    assert head(slots=None) == E_NULL
    assert head(R=48) == E_UNSUPPORTED
    assert head(S=192) == E_UNSUPPORTED
    assert head(k=3) == E_SHAPE                    # 3 hops of 32 rows in a chunk buffer of 64
    assert head(zrows=32) == E_SHAPE
    assert head(zst=100) == E_SHAPE
    assert head(L=0) == E_SHAPE
    assert head(cap=0) == E_SHAPE
    assert head(dt=7) == E_DTYPE
    assert named(b"pooled_stream_head_slots")

    def wmean(ring=A, rr=5, mean=A, slots=A, cap=2, k=2, hop=32, window=128, S=128, logits=None, w2=None):
        return lib.srwn_window_mean_slots(ring, rr, mean, slots, cap, k, hop, window, S, w2, w2, logits, 12, 32, None)

    assert wmean(ring=None) == E_NULL
    assert wmean(slots=None) == E_NULL
    assert wmean(logits=A) == E_NULL               # logits without the last 1x1
    assert wmean(window=100) == E_SHAPE            # not a multiple of hop
    assert wmean(hop=0) == E_SHAPE
    assert wmean(rr=4) == E_SHAPE                  # 4 window rows + 2 hops per launch - 1 = 5
    assert wmean(S=512) == E_SHAPE
    assert wmean(cap=0) == E_SHAPE and b"capacity=0" in lib.srwn_last_error()
    # slot form only: a slot's rows in the chunk are counted in int32, so k * hop must fit (capacity * k does here)
    assert wmean(cap=1, k=1 << 16, hop=1 << 16, window=1 << 16, rr=1 << 16) == E_SHAPE
    assert named(b"window_mean_slots")

    def hsum(r1=A, rows=64, slots=A, k=2, hop=32, mc=64, S=128, dt=1):
        return lib.srwn_hop_sum_slots(r1, rows, A, 5, slots, 2, k, hop, mc, S, dt, None)

    assert hsum(r1=None) == E_NULL
    assert hsum(slots=None) == E_NULL
    assert hsum(k=3) == E_SHAPE
    assert hsum(S=7) == E_SHAPE
    assert hsum(dt=7) == E_DTYPE
    assert named(b"hop_sum_slots")

    def entry(ring=A, ring_len=65, rows=31 + 64, hist=31, n=40, mc=64, R=32, dt=1, slots=A):
        return lib.srwn_recog_stream_in_slots(ring, ring_len, A, A, A, rows, hist, 2, n, mc, R, dt, slots, None)

    assert entry(ring=None) == E_NULL
    assert entry(slots=None) == E_NULL
    assert entry(R=48) == E_UNSUPPORTED
    assert entry(n=65) == E_SHAPE
    assert entry(n=0) == E_SHAPE
    assert entry(rows=64) == E_SHAPE
    assert entry(ring_len=64) == E_SHAPE           # max_chunk samples: no room for the sample before a whole chunk
    assert b"max_chunk + 1 = 65" in lib.srwn_last_error()
    assert entry(dt=7) == E_DTYPE
    assert named(b"recog_stream_in_slots")

    def roll(table=A, nroll=2, n=40, mc=64, R=32, dt=1, slots=A):
        return lib.srwn_recog_roll_slots(table, nroll, slots, 2, n, mc, R, dt, None)

    assert roll(table=None) == E_NULL
    assert roll(slots=None) == E_NULL
    assert roll(R=16) == E_UNSUPPORTED
    assert roll(n=65) == E_SHAPE
    assert roll(nroll=-1) == E_SHAPE
    assert lib.srwn_last_error() == b"recog_roll_slots: capacity=2 boundaries=-1 max_chunk=64"      # (no x, so no x stride)
    assert roll(dt=7) == E_DTYPE
    assert named(b"recog_roll_slots")
    assert roll(nroll=0, table=None) == 0          # no boundary buffers: nothing to roll, nothing launched
