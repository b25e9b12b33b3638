"""CPU tests of mixture-of-logistics scorer pools (srwn_version() 119; scorer.MolScorerPool, model.AutoEncoderScorerPool): what
the three new entry points refuse, the step plan with conditioning and the conditioning ring's room against brute force, the
encoder + scorer pair drained at its smallest rings, everything the pools refuse before they touch the device, and the
launch list.  No GPU: the pools stand on host memory or are built without their constructors, and no call gets as far as a
launch."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests._pkg import ROOT, sub
from tests.test_stream_stack import NAMES, Weights, _check_kinds, calls      # noqa: F401  (the recorder in _lib.call's place)

NEW = ["srwn_mol_score_stream_in_slots", "srwn_stream_mol_score_head_slots", "srwn_mol_score_rows_slots"]
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _bare(cls, **attrs):
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _bare_pool(capacity=3, max_chunk=32, ring=None, E=6, P=20, hist_max=55, frames=None):
    import torch
    S_ = sub("scorer")
    frames = S_.live_min_frames(hist_max, P) if frames is None else frames
    c = SimpleNamespace(E=E, pool=P if E else 1, hist_max=hist_max if E else 0, max_frames=frames if E else 1)
    return _bare(S_.MolScorerPool, c=c, capacity=capacity, max_chunk=max_chunk,
                 audio_ring=2 * max_chunk + 2 if ring is None else ring, _received=np.zeros(capacity, np.int64),
                 _scored=np.zeros(capacity, np.int64), _fed=np.zeros(capacity, np.int64),
                 _nll_sum=torch.zeros(capacity, dtype=torch.float64), _active=np.zeros(capacity, bool), ring=None, stage=None,
                 table=None, _graphs={}, _seen=set(), _open=True)


def _state(p):
    return (p._received.tolist(), p._scored.tolist(), p._fed.tolist(), p._active.tolist())


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    raw = open(os.path.join(ROOT, "include", "srwn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    block = raw[raw.index("mixture-of-logistics scorer pools (since srwn_version() 119"):]
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in block, n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_slot_argument_errors_do_not_need_a_gpu(binding):
    from tests.test_scorer import _lib
    lib = _lib(binding)
    assert lib.srwn_version() >= 119
    for n in NEW:
        assert hasattr(lib, n), n

    def named(entry):
        return lib.srwn_last_error().startswith(entry + b":")

    def entry(ring=A, ring_len=66, w=A, cond=A, frames=4, pool=20, cstride=96, out=A, rows=31 + 64, hist=31, x=A, xstride=64,
              cap=2, n=40, mc=64, R=32, dt=7, slots=A):
        # (dt = 7 by default: a call whose other arguments are all good ends at the dtype check, before any launch)
        return lib.srwn_mol_score_stream_in_slots(ring, ring_len, w, A, cond, frames, pool, cstride, out, rows, hist, x, xstride,
                                                  cap, n, mc, R, dt, slots, None)

    assert entry() == E_DTYPE and named(b"mol_score_stream_in_slots")
    assert entry(cap=0) == 0 and entry(n=0) == 0                   # empty work is done
    assert entry(n=0, ring=None, R=48, dt=7) == 0                  # ... before anything else is looked at
    for name in ("ring", "w", "cond", "out", "x", "slots"):
        assert entry(**{name: None}) == E_NULL, name
    assert entry(R=48) == E_UNSUPPORTED and entry(R=128) == E_UNSUPPORTED
    assert entry(frames=1, cstride=32) == E_DTYPE                  # an unconditioned decoder's one zero row per slot
    assert entry(n=65) == E_SHAPE and entry(n=-1) == E_SHAPE and entry(cap=-1) == E_SHAPE
    assert entry(rows=64) == E_SHAPE and entry(xstride=63) == E_SHAPE
    assert entry(frames=0) == E_SHAPE and entry(pool=0) == E_SHAPE and entry(cstride=31) == E_SHAPE and entry(cstride=36) == E_SHAPE
    assert entry(ring_len=65) == E_SHAPE                           # max_chunk + 1 samples: no room for a[t - 2] beside a whole chunk
    assert b"max_chunk + 2 = 66" in lib.srwn_last_error() and named(b"mol_score_stream_in_slots")
    assert entry(slots=None, R=48) == E_NULL and entry(R=48, n=65) == E_UNSUPPORTED and entry(n=65, dt=1) == E_SHAPE

    def head(z=A, zst=2 * 64 * 32, zrows=64, L=3, w2=A, x=A, xstride=64, nll=A, lo=None, ostride=64, cap=2, n=40, mc=64, R=32,
             S=128, M=10, dt=7, slots=A):
        return lib.srwn_stream_mol_score_head_slots(z, zst, zrows, L, A, A, A, A, w2, A, x, xstride, nll, lo, ostride, cap, n, mc,
                                                    R, S, M, dt, slots, None)

    assert head() == E_DTYPE and named(b"stream_mol_score_head_slots")
    assert head(lo=A) == E_DTYPE and head(M=1) == E_DTYPE and head(M=16) == E_DTYPE
    assert head(cap=0) == 0 and head(n=0) == 0 and head(n=0, z=None) == 0
    for name in ("z", "w2", "x", "nll", "slots"):
        assert head(**{name: None}) == E_NULL, name
    assert head(R=48) == E_UNSUPPORTED and head(S=192) == E_UNSUPPORTED
    assert head(M=0) == E_SHAPE and head(M=17) == E_SHAPE
    assert head(n=65) == E_SHAPE and head(n=-3) == E_SHAPE and head(cap=-1) == E_SHAPE
    assert head(zrows=32) == E_SHAPE and head(ostride=39) == E_SHAPE and head(xstride=39) == E_SHAPE
    assert head(zst=100) == E_SHAPE and head(L=0) == E_SHAPE
    assert named(b"stream_mol_score_head_slots")

    def rows(logits=A, ld=64, crows=64, x=A, xstride=64, nll=A, ostride=64, cap=2, n=40, M=10, slots=A):
        return lib.srwn_mol_score_rows_slots(logits, ld, crows, x, xstride, nll, None, ostride, cap, n, M, slots, None)

    assert rows(cap=0) == 0 and rows(n=0) == 0 and rows(n=0, logits=None) == 0
    for name in ("logits", "x", "nll", "slots"):
        assert rows(**{name: None}) == E_NULL, name
    assert named(b"mol_score_rows_slots")
    assert rows(M=0) == E_SHAPE and rows(M=17, ld=128) == E_SHAPE
    assert rows(ld=39) == E_SHAPE and rows(crows=39) == E_SHAPE and rows(ostride=39) == E_SHAPE and rows(xstride=39) == E_SHAPE
    assert rows(n=-1) == E_SHAPE and rows(cap=-2) == E_SHAPE
    assert named(b"mol_score_rows_slots")


# ---- the plan with conditioning ----------------------------------------------------------------------------------------
def test_plan_with_conditioning_against_brute_force():
    rng = np.random.default_rng(1)
    for trial in range(300):
        cap = int(rng.integers(1, 7))
        mc = int(rng.choice([1, 31, 32, 33, 64, 128]))
        P = int(rng.choice([1, 16, 20]))
        E = 6 if trial % 4 else 0
        p = _bare_pool(capacity=cap, max_chunk=mc, E=E, P=P, frames=1000)
        p._fed[:] = rng.integers(0, 40, cap)
        p._scored[:] = [rng.integers(0, f * P + 1) if E else rng.integers(0, 900) for f in p._fed]
        p._received[:] = p._scored + rng.integers(0, 3 * mc + 2, cap) * (rng.random(cap) < 0.8)
        p._active[:] = rng.random(cap) < 0.7
        n, rows = p._plan()
        for u in range(cap):
            w = 0                                                  # brute force: one sample at a time
            while (p._active[u] and w < mc and p._scored[u] + w < p._received[u]
                   and (not E or (p._scored[u] + w) // P < p._fed[u])):     # ... that has arrived and whose frame was fed
                w += 1
            assert rows[u] == w, (trial, u)
            bound = (min(p._received[u], p._fed[u] * P) if E else p._received[u]) - p._scored[u]
            assert rows[u] <= max(bound, 0) and rows[u] <= mc and (p._active[u] or rows[u] == 0)
            assert p.available(u) == max(bound, 0) or bound < 0
        assert (n == 0) == (rows.max() == 0) and rows.max() <= n <= mc and (n % 32 == 0 or n == mc)


@pytest.mark.parametrize("P,hist_max,mc", [(20, 255, 128), (16, 18, 64), (1, 7, 5), (512, 255, 128)])
def test_conditioning_ring_of_one_slot(P, hist_max, mc):
    """One slot through random joins, feeds, pushes and steps at the smallest ring (``live_min_frames``): ``room`` is the
    brute-force count of frames that can be written without touching one a later chunk still reads -- the halo reaches
    back to t - hist_max --, and what every chunk reads is what was fed."""
    S_ = sub("scorer")
    rng = np.random.default_rng(P + mc)
    F = S_.live_min_frames(hist_max, P)
    p = _bare_pool(capacity=1, max_chunk=mc, ring=mc + 2, E=6, P=P, hist_max=hist_max, frames=F)
    with pytest.raises(ValueError, match="free slots"):
        p.join(2)
    p._active[0] = True
    held, wraps = {}, 0                                            # ring row -> the frame it holds
    for rnd in range(600):
        if rnd % 150 == 149:                                       # the stream leaves, another joins the slot: nothing is zeroed
            p._received[0] = p._scored[0] = p._fed[0] = 0
        fed, t = int(p._fed[0]), int(p._scored[0])
        oldest = max(t - hist_max, 0) // P                         # the oldest frame a later chunk still reads
        brute = 0
        while fed + brute - F < oldest:                            # frame fed + brute would overwrite frame fed + brute - F
            brute += 1
        assert p.room(0) == brute and brute >= (1 if t == fed * P else 0)
        k = int(rng.integers(0, brute + 1))
        for q in range(fed, fed + k):
            assert held.get(q % F, -1) < oldest or held[q % F] >= fed, (rnd, q)      # (>= fed: an earlier stream's, never read)
            held[q % F] = q
        wraps += (fed + k) // F - fed // F
        p._fed[0] += k
        p._received[0] += int(rng.integers(0, p.audio_room(0) + 1))
        n, rows = p._plan()
        m = int(rows[0])
        if m:
            for q in range(oldest, (t + m - 1) // P + 1):          # halo rows included
                assert held[q % F] == q, (rnd, q)
            assert (t + m - 1) // P < p._fed[0]
        p._scored[0] += m
    assert wraps > 10


# ---- the encoder + scorer pair -----------------------------------------------------------------------------------------
def _host_pair(calls, monkeypatch, P, enc_layers, mc, cap=3, ring=None, frames=None):
    """An ``AutoEncoderScorerPool`` whose halves stand on host memory: a real ``MolScorerPool`` on stand-in weights (the
    recorder in ``call``'s place) and an ``EncoderPool`` built without its constructor whose launch returns zero frames."""
    import torch
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    monkeypatch.setattr(sub("audio_ring"), "call", lambda name, *args: calls.append((name, args)))
    S_, En, M = sub("scorer"), sub("encoder"), sub("model")
    lat = 2
    w = Weights(classes=40, E=lat, M=10, pool=P)
    hist_max = max(S_.StreamStack.plan(w.dil)[1])
    frames = S_.live_min_frames(hist_max, P) if frames is None else frames
    s = S_.MolStreamScorer(w, max_batch=cap, max_chunk=mc, max_frames=frames)
    need = S_.ae_pool_min_audio_ring(mc, P, enc_layers)
    mol = s.pool(need if ring is None else ring)
    ering = P + enc_layers + 1                                     # the encoder pool's own minimum
    enc = _bare(En.EncoderPool, fe=None, P=P, L=enc_layers, lat=lat, capacity=cap, window=ering, audio_ring=ering, max_rows=64,
                _received=np.zeros(cap, np.int64), _emitted=np.zeros(cap, np.int64), _final=np.zeros(cap, bool),
                _active=np.zeros(cap, bool), ring=torch.zeros((cap, ering)), stage=torch.zeros(4 * cap + cap * ering, dtype=torch.int32))
    enc._launch = lambda items: torch.zeros((len(items), lat))
    pair = _bare(M.AutoEncoderScorerPool, _owner=SimpleNamespace(pool_stride=P), capacity=cap, _cs=0, _enc=enc, _mol=mol, _cond={})
    return pair, s


@pytest.mark.parametrize("P,enc_layers,mc", [(16, 6, 64), (20, 30, 16), (40, 3, 8), (8, 2, 128)])
def test_pair_drains_at_its_smallest_rings(calls, monkeypatch, P, enc_layers, mc):
    """Sessions of random lengths pushed in random pieces, at the smallest scorer audio ring, the smallest encoder ring and the
    smallest conditioning ring: every one ends with scored == (T // P) * P and its slot freed, within a bound on the
    steps -- no deadlock."""
    S_ = sub("scorer")
    pair, s = _host_pair(calls, monkeypatch, P, enc_layers, mc)
    assert pair._mol.audio_ring == S_.ae_pool_min_audio_ring(mc, P, enc_layers) == max(mc + 2, P + enc_layers + 3)
    assert s.max_frames == S_.live_min_frames(s.hist_max, P)
    rng = np.random.default_rng(P)
    lengths = [5 * P + 3, P - 1, 0, 12 * P, 7 * P + enc_layers + 1, int(rng.integers(0, 9 * P))]
    waiting, stream_of, sent, got = list(range(len(lengths))), {}, {}, {i: 0 for i in range(len(lengths))}
    steps, bound = 0, 40 * len(lengths) + sum(lengths)
    while waiting or stream_of:
        steps += 1
        assert steps <= bound, "the pair stalled: %s" % (stream_of,)
        if waiting and pair.free:
            u, = pair.join()
            stream_of[u] = waiting.pop(0)
            sent[u] = 0
        for u, i in stream_of.items():
            if pair._enc._final[u]:
                continue
            room = pair.audio_room(u)
            assert room == min(pair._enc.audio_room(u), pair._mol.audio_room(u))
            k = int(min(rng.integers(0, 2 * P + 2), room, lengths[i] - sent[u]))
            pair.push(u, np.zeros(k, np.float32))
            sent[u] += k
            if sent[u] == lengths[i]:
                pair.finish(u)
        out = pair.step()
        for u, v in out.items():
            assert isinstance(v, np.ndarray) and v.shape[0] > 0
            got[stream_of[u]] += v.shape[0]
        assert np.all(pair._mol._scored <= pair._mol._fed * P) and np.all(pair._mol._fed == pair._enc._emitted)
        for u in [u for u in stream_of if u not in pair.active]:
            assert pair._mol._scored[u] == (lengths[stream_of[u]] // P) * P and not pair._mol._active[u] and not pair._enc._active[u]
            del stream_of[u]
    assert got == {i: (n // P) * P for i, n in enumerate(lengths)}


def test_pair_refuses_a_ring_below_the_minimum():
    M, S_ = sub("model"), sub("scorer")
    owner = SimpleNamespace(encoder=SimpleNamespace(_eng=SimpleNamespace(P=16, L=60, max_frames=4, max_batch=2)),
                            _eng=SimpleNamespace(max_chunk=64, max_batch=3), condition_size=0)
    need = S_.ae_pool_min_audio_ring(64, 16, 60)
    assert need == 16 + 60 + 3 > 64 + 2 and S_.ae_pool_min_audio_ring(64, 16, 6) == 66
    with pytest.raises(ValueError, match="at least %d" % need):
        M.AutoEncoderScorerPool(owner, need - 1)
    # one below the minimum does deadlock: the encoder cannot complete its next frame, the scorer has nothing to score
    mol = _bare_pool(capacity=1, max_chunk=64, ring=need - 1, E=2, P=16)
    mol._active[0] = True
    mol._received[0] = mol.audio_room(0)                             # all the scorer's ring takes at scored = emitted * P = 0
    assert (mol._received[0] - 60 - 1) // 16 == 0                    # encoder.plan_frames: no frame is due


# ---- refusals that leave the state untouched ---------------------------------------------------------------------------
def test_pool_refuses_first(calls, monkeypatch):
    import torch
    S_ = sub("scorer")
    sc = _bare(S_.MolStreamScorer, max_batch=3, max_chunk=32, _pool=None, _state=None, _serial=0)
    sc.pool = S_._PoolStride(20, sc)                                 # the pool stride, and the call that opens a pool
    assert sc.pool == 20 and isinstance(sc.pool, int) and 3 * sc.pool == 60
    with pytest.raises(ValueError, match="audio_ring"):
        sc.pool(audio_ring=33)                                       # one sample short of max_chunk + 2
    assert sc._pool is None and sc._serial == 0                      # a refused pool ends nothing
    p = _bare_pool()                                                 # hist_max 55 at P = 20: a ring of 4 frames
    p._active[:] = [True, False, True]
    p._received[0], p._scored[0], p._fed[0] = 70, 60, 4              # oldest frame read: (60 - 55) // 20 = 0
    assert p.c.max_frames == 4 and p.room(0) == 0 and p.room(2) == 4 and p.audio_room(0) == 66 - 2 - 10
    assert p.available(0) == 10 and p.available(2) == 0
    before = _state(p)
    f = lambda k, e=6: torch.zeros((k, e))
    for slots, frames, what in (([0], [f(1)], "room for 0"), ([2], [f(5)], "room for 4"), ([1], [f(1)], "holds no stream"),
                                ([2], [f(1, 5)], r"\[k, 6\]"), ([2, 2], [f(1), f(1)], "not distinct"),
                                ([0, 2], [f(0)], "2 slots but 1"), ([7], [f(1)], "outside"), ([2, 0], [f(1), f(1)], "room for 0")):
        with pytest.raises(ValueError, match=what):
            p.feed(slots, frames)
        assert _state(p) == before and not calls
    p.feed([0, 2], [f(0), f(0)])                                     # nothing to write: no device work
    assert not calls and _state(p) == before
    x = np.zeros(10, np.float32)
    for slots, audio, what in (([1], [x], "holds no stream"), ([0], [np.zeros(55, np.float32)], "room for 54")):
        with pytest.raises(ValueError, match=what):
            p.push(slots, audio)
        assert _state(p) == before
    un = _bare_pool(E=0)
    un._active[0] = True
    assert un.room(0) == 0
    with pytest.raises(ValueError, match="not conditioned"):
        un.feed([0], [f(1)])
    p._open = False
    for call in (lambda: p.join(), lambda: p.leave(2), lambda: p.push(2, x), lambda: p.feed([2], [f(1)]), lambda: p.step()):
        with pytest.raises(ValueError, match="closed"):
            call()
    assert _state(p) == before


def test_pair_refuses_first(calls, monkeypatch):
    pair, s = _host_pair(calls, monkeypatch, 16, 6, 64, ring=100)
    enc, mol = pair._enc, pair._mol
    assert pair.join(n=2) == [0, 1] and pair.active == [0, 1] and pair.free == [2]
    state = lambda: (enc._received.tolist(), enc._final.tolist(), enc._active.tolist(), _state(mol))
    del calls[:]
    before = state()
    x = np.zeros(5, np.float32)
    with pytest.raises(ValueError, match="do not all hold"):
        pair.push(2, x)                                              # a free slot
    assert enc.audio_room(0) == 23 and mol.audio_room(0) == 98 and pair.audio_room(0) == 23
    with pytest.raises(ValueError, match="room for 23"):
        pair.push(0, np.zeros(24, np.float32))                       # fits the scorer half only
    enc.audio_ring, mol_ring = 200, mol.audio_ring
    with pytest.raises(ValueError, match="room for 98"):
        pair.push([0, 1], [x, np.zeros(99, np.float32)])             # fits the encoder half only: neither slot is written
    enc.audio_ring = 23
    assert state() == before and not calls
    pair.finish(1)
    before = state()
    with pytest.raises(ValueError, match="finished"):
        pair.push([0, 1], [x, x])                                    # a finished stream: the other piece is not written either
    assert state() == before and not calls
    pair.push([0], [x])
    assert [n for n, _ in calls] == ["srwn_audio_ring_put"] * 2      # two uploads: the halves keep separate rings
    assert enc._received.tolist()[:2] == [5, 0] and mol._received.tolist()[:2] == [5, 0]
    s.start(1)                                                       # the scorer starts a batch: its pool is closed
    before = state()
    for call in (lambda: pair.join(), lambda: pair.push(0, x), lambda: pair.step(), lambda: pair.leave(0)):
        with pytest.raises(ValueError, match="closed"):
            call()
    assert state() == before


# ---- a whole pool step on host memory: the launch list -----------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twin"])
@pytest.mark.parametrize("E", [6, 0])
def test_pool_step_launch_list_on_host_memory(calls, monkeypatch, fused, E):
    """``_lib.call`` is a recorder and the weights are stand-ins on host memory: a pool step is the scorer's ONE launch list
    in its slot forms on the table uploaded for the pass -- the lockstep list name for name, as many launches."""
    import torch
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1" if fused else "0")
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    monkeypatch.setattr(sub("audio_ring"), "call", lambda name, *args: calls.append((name, args)))
    S_ = sub("scorer")
    cap, mc, P = 3, 48, 20
    s = S_.MolStreamScorer(Weights(classes=40, E=E, M=10, pool=P if E else 1), max_batch=cap, max_chunk=mc, max_frames=32)
    s._launch_step(cap, 17)
    lockstep = [n for n, _ in calls]
    del calls[:]
    st = s.start(2)
    pool = s.pool()
    assert s._state is None and s._pool is pool and pool.audio_ring == 2 * mc + 2 and pool.capacity == cap
    with pytest.raises(ValueError, match="current"):
        s.push(st, np.zeros((2, 4), np.float32))
    assert pool.join(2) == [0, 1] and [n for n, _ in calls] == ["srwn_flow_stream_reset_slots"]
    pool.push([0, 1], [np.zeros(70, np.float32), np.zeros(5, np.float32)])
    del calls[:]
    if E:
        assert pool.step() == {} and not calls                        # no frame fed: nothing to score, nothing launched
        pool.feed([0, 1], [torch.zeros((3, E)), torch.zeros((1, E))])
        assert [n for n, _ in calls] == ["srwn_pw_linear", "srwn_cond_ring_scatter_slots"]      # one of each, however many slots
        sc = calls[1][1]
        assert sc[4] == 4 and pool._dst[:4].tolist() == [0, 1, 2, 32] and sc[6] == cap * 32
        assert pool.fed.tolist() == [3, 1, 0] and pool.available(0) == 60 and pool.available(1) == 5
        del calls[:]
    out = pool.step(return_logits=True)
    G = len(s.groups)
    slot_form = {"srwn_flow_stream_in": "srwn_mol_score_stream_in_slots", NAMES[True, False]: NAMES[True, True],
                 "srwn_stream_mol_score_head": "srwn_stream_mol_score_head_slots", "srwn_mol_score_rows": "srwn_mol_score_rows_slots",
                 "srwn_recog_roll": "srwn_recog_roll_slots", "srwn_pw_linear": "srwn_pw_linear"}
    one = [slot_form[n] for n in lockstep]
    assert one[0] == "srwn_mol_score_stream_in_slots" and one.count(NAMES[True, True]) == G
    assert [n for n, _ in calls] == one * 2 and len(one) == pool.launches_per_step == s.launches_per_step
    for name, args in calls:
        _check_kinds(name, args)
    table = pool.table.data_ptr()
    es = s.ring.element_size()
    for name, a in calls:
        if name == "srwn_mol_score_stream_in_slots":
            assert a[:2] == (pool.ring.data_ptr(), pool.audio_ring) and a[4] == s.ring.data_ptr() and a[-2] == table
            assert a[5:8] == ((32, P, s.LR) if E else (1, 1, s.w.R)) and a[11:13] == (s.xbuf.data_ptr(), mc) and a[13] == cap
        elif name == NAMES[True, True]:
            assert a[-2] == table and (a[11] is not None) == bool(E)
        elif name in ("srwn_stream_mol_score_head_slots", "srwn_mol_score_rows_slots", "srwn_recog_roll_slots"):
            assert table in a, name
    assert [a[14] for n, a in calls if n == "srwn_mol_score_stream_in_slots"] == ([48, 32] if E else [48, 32])
    want = [60, 5, 0] if E else [70, 5, 0]
    assert pool.table.tolist() == [[48, want[0]], [5, 5], [0, 0]]  # the second pass's table: nothing advanced it but the host
    assert isinstance(out, tuple) and len(out) == 2 and set(out[0]) == {0, 1} == set(out[1])
    assert out[0][0].shape == (want[0],) and out[0][1].shape == (5,) and out[1][0].shape == (want[0], 40)
    assert pool.scored.tolist() == want and pool.step() == {}
    s.start(1)                                                       # start() closes the pool
    with pytest.raises(ValueError, match="closed"):
        pool.step()
    assert s._pool is None
    M = sub("model")
    for cls, name in ((M.StreamingMolScorer, "pool"), (M.AutoEncoderScorer, "pool"), (S_.MolStreamScorer, "pool")):
        assert callable(getattr(cls, name))
