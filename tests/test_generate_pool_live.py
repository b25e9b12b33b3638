"""CPU tests of live slots in generation pools (srwn_version() 114): the rule that realigns a resuming slot's layer rings
against a NumPy model of the rings, the per-slot room, every refusal with the state untouched, and the model faces'
argument handling.  No device: the pools are objects without their device state, as in tests/test_generate_pool.py."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests._pkg import sub
from tests.test_generate_pool import _bare

DEPTHS = [2, 3, 5, 6, 9, 17, 33]
INT32_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------------
# the shift rule against a NumPy model of one layer ring column
# ---------------------------------------------------------------------------------------------------
def _column_reads(depth, clock0, spans, rng, paused):
    """One column of a ring of `depth` positions that follows the pool's clock: a step at clock c reads the delayed tap at
    (c + 1) mod depth and writes its input at c mod depth.  `spans`: alternating (own steps, clock ticks waited).  Paused:
    the column stores nothing while it waits and is rotated by live_slot_shift when it runs again; not paused: its own
    steps simply follow one another.  Returns what its steps read."""
    shift = sub("engine").live_slot_shift
    ring = rng.standard_normal(depth)                                # the history a join's ring fill left at clock0
    clock, stopped, reads, k = clock0, clock0, [], 0
    for run, wait in spans:
        if paused and run > 0:
            ring = np.roll(ring, shift(clock, stopped))              # new[(p + s) mod D] = old[p]
        for _ in range(run):
            reads.append(ring[(clock + 1) % depth])
            ring[clock % depth] = 1000.0 + k                         # x_l of own step k
            k += 1
            clock += 1
        stopped = clock if run > 0 else stopped
        if paused:
            clock += wait                                            # the pool runs on; this column's stores are held back
    return reads


@pytest.mark.parametrize("depth", DEPTHS)
def test_rotation_by_the_shift_rule_restores_what_an_unpaused_column_reads(depth):
    waits = list(range(0, 3 * depth + 2)) + [7 * depth, 7 * depth + 1, 1000003]
    runs = [1, 2, depth - 1, depth, depth + 1, 3 * depth, 0, 5]
    spans = [(runs[i % len(runs)], w) for i, w in enumerate(waits)]
    for clock0 in (0, 1, depth, 57, 12345):
        want = _column_reads(depth, clock0, spans, np.random.default_rng(depth), paused=False)
        got = _column_reads(depth, clock0, spans, np.random.default_rng(depth), paused=True)
        assert len(want) == sum(r for r, _ in spans) and got == want, clock0
    eng = sub("engine")
    assert eng.live_slot_shift(57, 57) == 0 and eng.live_slot_shift(INT32_MAX, 0) == INT32_MAX
    for bad in ((5, 6), (5, -1), (INT32_MAX + 1, 0)):
        with pytest.raises(ValueError, match="live_slot_shift"):
            eng.live_slot_shift(*bad)


def test_the_model_of_the_rings_tells_a_missing_rotation(monkeypatch):
    eng = sub("engine")
    spans = [(4, 3), (4, 0), (2, 1), (6, 0)]
    want = _column_reads(5, 2, spans, np.random.default_rng(1), paused=False)
    monkeypatch.setattr(eng, "live_slot_shift", lambda clock, stopped: 0)
    assert _column_reads(5, 2, spans, np.random.default_rng(1), paused=True) != want


# ---------------------------------------------------------------------------------------------------
# bare pools
# ---------------------------------------------------------------------------------------------------
def _live_pool(capacity=4, frames=4, E=6, pool_stride=16, live=True):
    EG = sub("engine")
    z = lambda dt: np.zeros(capacity, dt)
    return _bare(EG.GenerationPool, capacity=capacity, _active=z(bool), conditioned=True, frames=frames, E=E,
                 pool_stride=pool_stride, eng=None, live=live, _live=z(bool), _closed=z(bool), _fed=z(np.int64),
                 _cap=np.full(capacity, INT32_MAX, np.int64), _t=z(np.int64), _end=z(np.int64), _stopped=z(np.int64),
                 _seed=[0] * capacity, clock=0, C=20, mol=True)


def _state(p):
    return tuple(np.array(getattr(p, k)).tolist() for k in ("_active", "_live", "_closed", "_fed", "_cap", "_t", "_end",
                                                              "_stopped")) + (p.clock,)


def _take(p, u, fed, t, live=True, closed=False):
    p._active[u], p._live[u], p._closed[u], p._fed[u], p._t[u] = True, live, closed, fed, t
    p._end[u] = fed * p.pool_stride


def test_room_per_slot_is_live_decode_room():
    EG = sub("engine")
    p = _live_pool(capacity=6, frames=4, pool_stride=16)
    cases = {0: (0, 0), 1: (4, 0), 2: (4, 17), 3: (11, 11 * 16), 4: (7, 63)}
    for u, (fed, t) in cases.items():
        _take(p, u, fed, t)
        assert p.room(u) == EG.live_decode_room(4, fed, t, 16) == 4 - fed + t // 16, u
    assert [p.room(u) for u in range(5)] == [4, 0, 1, 4, 0]
    assert p.room(5) == 0                                            # free
    p._live[0] = False
    p._closed[2] = True
    assert p.room(0) == 0 and p.room(2) == 0                         # a bounded stream, a closed one
    with pytest.raises(ValueError, match="slots"):
        p.room(6)
    q = _live_pool(live=False)
    _take(q, 0, 1, 0)
    assert q.room(0) == 0                                            # a pool made without live


def test_engine_refuses_live_pools_of_other_stacks_first():
    EG = sub("engine")
    ok = dict(wavenet=False, o_gen=0, cfg=SimpleNamespace(head_mode="per_timestep"), mol=False, E=0)
    with pytest.raises(ValueError, match="not conditioned"):
        _bare(EG.WaveNetEngine, **ok).generation_pool(4, live=True)                       # the unconditioned softmax teacher
    with pytest.raises(ValueError, match="not conditioned"):
        _bare(EG.WaveNetEngine, **dict(ok, mol=True)).generation_pool(4, live=True)       # an unconditioned mixture head
    with pytest.raises(NotImplementedError, match="conditioned softmax"):
        _bare(EG.WaveNetEngine, **dict(ok, E=6)).generation_pool(4, 3, live=True)
    with pytest.raises(NotImplementedError, match="wavenet"):
        _bare(EG.WaveNetEngine, **dict(ok, wavenet=True, mol=True, E=6)).generation_pool(4, 3, live=True)
    with pytest.raises(ValueError, match="frames"):
        _bare(EG.WaveNetEngine, **dict(ok, mol=True, E=6)).generation_pool(4, live=True)  # the ring length is required
    with pytest.raises(TypeError):
        _bare(EG.WaveNetEngine, **dict(ok, mol=True, E=6)).generation_pool(4, 3, True)    # keyword-only


def test_pool_refuses_with_its_state_untouched():
    z = lambda k: np.zeros((k, 6), np.float32)
    plain = _live_pool(live=False)
    before = _state(plain)
    with pytest.raises(ValueError, match="live=True"):
        plain.join([1], cond=[z(1)], live=True)                      # a pool made without live
    assert _state(plain) == before

    p = _live_pool(capacity=5, frames=4, pool_stride=16)
    _take(p, 0, 3, 20)                                               # live, open: room 4 - 3 + 1 = 2
    _take(p, 1, 2, 0, live=False)                                    # bounded
    _take(p, 2, 4, 64, closed=True)                                  # live, closed
    before = _state(p)
    with pytest.raises(ValueError, match="room for 2"):
        p.feed([0], [z(3)])                                          # k > room
    with pytest.raises(ValueError, match="no live, open stream"):
        p.feed([1], [z(1)])                                          # bounded
    with pytest.raises(ValueError, match="no live, open stream"):
        p.feed([2], [z(1)])                                          # closed
    with pytest.raises(ValueError, match="no live, open stream"):
        p.feed([3], [z(1)])                                          # free
    with pytest.raises(ValueError, match="no live, open stream"):
        p.feed([0, 3], [z(1), z(1)])                                 # one good slot does not let the other in
    with pytest.raises(ValueError, match="distinct slots"):
        p.feed([0], [z(1), z(1)])                                    # mismatched lengths
    with pytest.raises(ValueError, match="distinct slots"):
        p.feed([0, 0], [z(1), z(1)])
    with pytest.raises(ValueError, match=r"\[k, 6\]"):
        p.feed([0], [np.zeros((1, 5), np.float32)])
    with pytest.raises(ValueError, match="slots"):
        p.feed([5], [z(1)])
    with pytest.raises(ValueError, match="exceeds"):
        p.join([7], prompts=[np.zeros(33, np.float32)], cond=[z(2)], live=True)            # prompt > k_i * pool_stride
    with pytest.raises(ValueError, match="exceeds"):
        p.join([7], prompts=[np.zeros(1, np.float32)], cond=[None], live=True)             # ... with no frame at all
    with pytest.raises(ValueError, match=r"\[0\.\.4 frames, 6\]"):
        p.join([7], cond=[z(5)], live=True)                          # more first frames than the ring holds
    with pytest.raises(ValueError, match=r"\[1\.\.4 frames, 6\]"):
        p.join([7], cond=[z(0)])                                     # a bounded stream brings at least one
    with pytest.raises(ValueError, match="free slots"):
        p.join([7, 8, 9], cond=[z(1)] * 3, live=True)
    assert _state(p) == before
    p.feed([0], [z(0)])                                              # no frames: nothing to do, no device work
    assert _state(p) == before
    # close: at once where the stream already is at its end, otherwise at the end of what it was fed
    _take(p, 3, 2, 32)
    p.close([0, 3, 1])
    assert p._active.tolist() == [True, True, True, False, False] and p._closed.tolist() == [True, False, True, True, False]
    assert p.room(0) == 0


# ---------------------------------------------------------------------------------------------------
# the model faces
# ---------------------------------------------------------------------------------------------------
class _FakePool:
    capacity, active, free = 4, [], [0, 1, 2, 3]

    def __init__(self):
        self.calls = []

    def join(self, seeds, prompts, cond, mx, **kw):
        self.calls.append(("join", seeds, prompts, cond, mx, kw))
        return list(range(len(seeds)))

    def feed(self, slots, encs):
        self.calls.append(("feed", slots, encs))

    def room(self, slot):
        return 3

    def close(self, slots):
        self.calls.append(("close", slots))


def test_model_face_argument_handling(monkeypatch):
    M, K = sub("model"), sub("kernels")
    import torch
    ae = _bare(M.WaveNetAutoEncoder, latent_channels=8, pool_stride=16, condition_size=2, _eng=None)
    if not torch.cuda.is_available():
        fp = _FakePool()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.GenerationPool(fp, ae._pool_cond, "sample", 8, 2).join(seed=1, encoding=np.zeros((1, 8)), conditions=np.ones(2),
                                                                   live=True)
        assert fp.calls == []
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ae.generation_pool(2, 4, live=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            M.TeacherResynthesizer.pool(None)
    with pytest.raises(ValueError, match="capacity"):
        ae.generation_pool(0, 4, live=True)
    with pytest.raises(TypeError):
        ae.generation_pool(2, 4, "sample", True)                     # keyword-only
    monkeypatch.setattr(K, "_need_gpu", lambda: None)
    fp = _FakePool()
    gp = M.GenerationPool(fp, ae._pool_cond, "sample", 8, 2)
    e0 = np.arange(16, dtype=np.float32).reshape(2, 8)
    assert gp.join(seed=5, encoding=e0, conditions=np.array([1.0, 2.0]), live=True) == [0]      # a single 2-D array: one stream
    name, seeds, prompts, cond, mx, kw = fp.calls[-1]
    assert (name, seeds, prompts, mx, kw["live"]) == ("join", [5], [None], [None], True)
    assert len(cond) == 1 and cond[0].shape == (2, 10) and cond[0][:, 8:].tolist() == [[1.0, 2.0]] * 2
    assert np.array_equal(cond[0][:, :8], e0)
    assert gp.join(seed=[6, 7], encoding=[np.zeros((0, 8)), np.ones((1, 8))], conditions=[[3.0, 4.0], [5.0, 6.0]],
                   temperature=[0.5, 1.0], live=True) == [0, 1]
    assert fp.calls[-1][3][0].shape == (0, 10) and fp.calls[-1][5]["temperature"] == [0.5, 1.0]
    # the conditions of a live stream are kept per slot and tiled onto every frame fed later
    gp.feed(1, np.full((3, 8), 9.0, np.float32))                     # one slot, one 2-D array
    name, slots, encs = fp.calls[-1]
    assert (name, slots) == ("feed", [1]) and encs[0].shape == (3, 10) and encs[0][:, 8:].tolist() == [[5.0, 6.0]] * 3
    gp.feed([0, 1], [np.zeros((1, 8)), np.zeros((2, 8))])
    assert [e[:, 8:].tolist() for e in fp.calls[-1][2]] == [[[3.0, 4.0]], [[5.0, 6.0]] * 2]
    n = len(fp.calls)
    with pytest.raises(ValueError, match="2 slots but 1 encodings"):
        gp.feed([0, 1], [np.zeros((1, 8))])
    with pytest.raises(ValueError, match=r"\[k, 8\]"):
        gp.feed([0], [np.zeros((1, 7))])
    with pytest.raises(ValueError, match="not all live streams"):
        gp.feed([2], [np.zeros((1, 8))])                             # no live stream was joined there
    with pytest.raises(ValueError, match="slots"):
        gp.feed([4], [np.zeros((1, 8))])
    assert len(fp.calls) == n
    assert gp.room(1) == 3
    gp.close([0, 1])
    assert fp.calls[-1] == ("close", [0, 1])
    # a bounded join through the same face keeps its call
    gp.join(seed=[8], encoding=[np.zeros((2, 8))], conditions=[[0.0, 0.0]])
    assert fp.calls[-1][0] == "join" and fp.calls[-1][5] == {}
    # the shared resynthesis loop: both pools are one class's step / join / push / finish / leave
    assert M.TeacherResynthesisPool.step is M.ResynthesisPool.step is M._ResynthesisPool.step
    assert M.TeacherResynthesisPool.join is M.ResynthesisPool.join and M.TeacherResynthesisPool.free is sub("slots").SlotTable.free
    for name in ("join", "push", "finish", "leave", "step", "audio_room", "t", "received"):
        assert hasattr(M.TeacherResynthesisPool, name), name
    with pytest.raises(ValueError, match="chunk_size"):
        M.TeacherResynthesisPool(SimpleNamespace(), 0, None)
