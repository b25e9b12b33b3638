"""The bookkeeping the serving pools and streams share (slots.py and the bases in model.py): one slot table, one
per-stream broadcast, one drain loop.  No device anywhere: the objects are built without their constructors."""
import numpy as np
import pytest

from tests._pkg import sub

S = sub("slots")


def _bare(cls, **attrs):
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _table(capacity=4, taken=(1,)):
    act = np.zeros(capacity, bool)
    act[list(taken)] = True
    return _bare(S.SlotTable, capacity=capacity, _active=act)


def test_take_slots_picks_the_lowest_free_and_refuses_the_rest():
    t = _table()
    assert t.active == [1] and t.free == [0, 2, 3]
    assert t._take_slots(1, None) == [0] and t._take_slots(2, None) == [0, 2] and t._take_slots(3, None) == [0, 2, 3]
    assert t._take_slots(2, [3, 0]) == [3, 0] and t._take_slots(1, 2) == [2]       # the caller's slots, in its order
    assert t._take_slots(None, [2, 3]) == [2, 3]                                   # however many are named
    with pytest.raises(ValueError, match="join: 4 streams but 3 free slots"):
        t._take_slots(4, None)
    with pytest.raises(ValueError, match="free slots"):
        t._take_slots(0, None)
    for bad in ([0, 0], [1], [-1], [4], [0, 2], []):                               # twice, taken, outside, outside, two for one, none
        with pytest.raises(ValueError, match="slots"):
            t._take_slots(1, bad)
    with pytest.raises(ValueError, match="not all free slots"):
        t._take_slots(2, [0, 1])
    with pytest.raises(ValueError, match="slots"):
        t._take_slots(None, [])
    with pytest.raises(ValueError, match="^feed: "):
        t._take_slots(1, [1], who="feed")
    assert t.active == [1]                                                         # choosing marks nothing


def test_slot_list():
    t = _table()
    assert t._slot_list(2, "leave") == [2] and t._slot_list(np.int64(3), "leave") == [3]
    assert t._slot_list([3, 1, 1], "leave") == [3, 1, 1] and t._slot_list(np.array([0, 2]), "leave") == [0, 2]
    assert t._slot_list((), "leave") == []
    for bad in (4, -1, [0, 4]):
        with pytest.raises(ValueError, match="leave: slots .* outside the pool's 4"):
            t._slot_list(bad, "leave")
    with pytest.raises(ValueError, match="push: slots .* not distinct"):
        t._slot_list([3, 1, 1], "push", distinct=True)
    assert S.slot_list([1, 0], 2, "feed", distinct=True) == [1, 0]


def test_per_stream():
    assert S.per_stream(None, 3, "prompts") == [None, None, None]
    assert S.per_stream(None, 2, "temperature", default=1.0) == [1.0, 1.0]
    assert S.per_stream(5, 3, "max_samples") == [5, 5, 5] and S.per_stream(np.float32(0.5), 2, "top_p") == [0.5, 0.5]
    assert S.per_stream(np.array(7), 2, "seeds") == [7, 7]
    assert S.per_stream([1, 2, 3], 3, "seeds") == [1, 2, 3] and S.per_stream((4,), 1, "seeds") == [4]
    ragged = [np.zeros(3), np.zeros(5)]                                            # entries of different lengths stay entries
    assert S.per_stream(ragged, 2, "prompts")[1] is ragged[1]
    assert S.per_stream([None, 0.5], 2, "temperatures", default=1.0) == [1.0, 0.5]
    assert S.per_stream([None, 0.5], 2, "temperatures") == [None, 0.5]
    with pytest.raises(ValueError, match=r"join: prompts has 1 entries for 2 streams"):
        S.per_stream([np.zeros(3)], 2, "prompts")
    with pytest.raises(ValueError, match=r"stream: top_k has 3 entries for 2 utterances"):
        S.per_stream([1, 2, 3], 2, "top_k", who="stream", counted="utterances")


def test_the_pools_share_one_slot_table():
    pools = (sub("engine").GenerationPool, sub("student").SynthPool, sub("encoder").EncoderPool)
    for name in ("active", "free", "_slot_list", "_take_slots"):
        assert all(getattr(p, name) is getattr(S.SlotTable, name) for p in pools), name
    assert sub("model").ResynthesisPool.free is S.SlotTable.free


class _FakeLive:
    """The live half of a resynthesis stream as ``_drain`` sees it: a ring of 2 frames of 4 samples that frees its frames
    two at a time, and a record of the calls."""
    RING, POOL = 2, 4

    def __init__(self, tuples):
        self.fed, self.t, self.calls, self.tuples = 0, 0, [], tuples

    @property
    def room(self):
        return self.RING - self.fed + self.t // (self.RING * self.POOL) * self.RING

    @property
    def available(self):
        return self.fed * self.POOL - self.t

    def _feed_device(self, frames):
        k = frames.shape[1]
        assert 0 < k <= self.room
        self.calls.append(("feed", k, float(frames[0, 0, 0])))
        self.fed += k

    def _step_device(self, n):
        assert 0 < n <= self.available
        self.calls.append(("step", n))
        self.t += n
        a = np.full((1, n), self.t)
        return (a, None, None) if self.tuples else a


def test_the_resynthesis_streams_share_one_drain_loop():
    M = sub("model")
    assert M.ResynthesisStream._drain is M.TeacherResynthesisStream._drain
    assert M.ResynthesisStream.push is M.TeacherResynthesisStream.push
    assert M.ResynthesisStream.finish is M.TeacherResynthesisStream.finish
    frames = np.arange(5, dtype=np.float32)[None, :, None] * np.ones((1, 5, 3), np.float32)     # frame q holds q
    for cls, tuples, shape in ((M.ResynthesisStream, False, (1, 20, 1)), (M.TeacherResynthesisStream, True, (1, 20))):
        live = _FakeLive(tuples)
        st = _bare(cls, _live=live, _chunk=3, batch_size=1)
        outs = []
        st._drain(frames, outs)
        assert live.calls == [("feed", 2, 0.0), ("step", 3), ("step", 3), ("step", 2),
                              ("feed", 2, 2.0), ("step", 3), ("step", 3), ("step", 2),
                              ("feed", 1, 4.0), ("step", 3), ("step", 1)]
        assert (live.fed, live.t, st.t) == (5, 20, 20)
        assert [o.shape[1] for o in outs] == [3, 3, 2, 3, 3, 2, 3, 1] and all(isinstance(o, np.ndarray) for o in outs)
        assert st._result([]).shape == shape[:1] + (0,) + shape[2:] and st._result([]).dtype == np.float32
        n = len(live.calls)
        st._drain(frames[:, :0], outs)                                             # no frame due, no sample to make
        assert len(live.calls) == n
