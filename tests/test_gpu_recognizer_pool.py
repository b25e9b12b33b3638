"""GPU tests of classifier pools (srwn_version() 115; recognizer.ClassifierPool, model.StreamingClassifier.pool).

The one claim is bit equality: a stream's emissions from a pool are ``StreamClassifier(max_batch=1).classify`` of that
stream alone -- probabilities and pooled logits -- in any slot, whenever it joined, however its audio was cut, whatever
k the steps had and whatever the other slots hold or held before.  There is no tolerance in this file; the lockstep
classifier is held to the fp64 oracle in tests/test_gpu_recognizer.py, and bit equality carries those bounds over.

  kernel   srwn_residual_group_fwd_stream_z_slots against one srwn_residual_group_fwd_stream_z call per slot
  pool     a ragged session of five streams in four slots: both cases, both dtypes, both head paths; max_hops 1 against 8;
           graph replay against eager launches; the NumPy face; which of a classifier's faces is the current one
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
# The two cases of tests/test_gpu_recognizer.py, restated: the smallest shapes that reach both group kinds (stride 1 and the
# residue-class groups of dilations >= 32), a masked last tile (hop % 32 != 0) and both widths.
CASES = {      # name: dilations, R, S, C, window, hop, max_hops
    "a": ([1, 2, 4, 8, 16, 32, 64, 1, 2, 4], 32, 128, 12, 128, 32, 4),
    "b": ([1, 2, 4, 8, 16, 32, 64, 128, 256, 512], 64, 256, 12, 320, 40, 8),
}
CAPACITY = 4
_PARAMS, _AUDIO, _ALONE = {}, {}, {}


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _params(name):
    if name not in _PARAMS:
        dil, R, S, Cc = CASES[name][:4]
        _PARAMS[name] = O.init_stack_params(11, dil, 2, R, S, Cc, bias_scale=0.05)
    return _PARAMS[name]


def _streams(name):
    """Five streams of different lengths, the third shorter than the window (it emits nothing): computed once, read-only."""
    if name not in _AUDIO:
        _, _, _, _, window, hop, mh = CASES[name]
        lengths = [window + 5 * hop + 3, 6 * window + 7, window - 1, 2 * window + mh * hop + hop // 2, window + 2 * mh * hop + 1]
        audio = O.synthetic_audio(len(lengths), max(lengths), seed=4).astype(np.float32)
        audio.setflags(write=False)
        _AUDIO[name] = [audio[i, :T] for i, T in enumerate(lengths)]
    return _AUDIO[name]


def _classifier(name, dt, max_batch, max_hops=None):
    R_ = sub("recognizer")
    dil, R, S, Cc, window, hop, mh = CASES[name]
    w = R_.ClassifierWeights(dil, R, S, Cc, 2, dt)
    w.load_oracle_params(_params(name))
    return R_.StreamClassifier(w, max_batch=max_batch, hop=hop, window=window, max_hops=max_hops or mh)


def _alone(name, dt, fused):
    """(probabilities, logits) [n_emit, C] of every stream from a batch-one classifier, once per (case, dtype, head path);
    the caller has set SRWN_RECOG_FUSED."""
    key = (name, dt, fused)
    if key not in _ALONE:
        c = _classifier(name, dt, 1)
        assert c.fused == fused
        out = []
        for x in _streams(name):
            p, l = c.classify(np.array(x[None]), return_logits=True)
            out.append((p[0].clone(), l[0].clone()))
        _ALONE[key] = out
    return _ALONE[key]


# ---- the z slot form against the z clock form ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", [32, 64])
@pytest.mark.parametrize("dil", [[1, 2, 4, 8, 16], [32, 64, 128, 256, 512]])
def test_z_slot_form_keeps_the_bits(dil, R, dt):
    R_ = sub("recognizer"); K = sub("kernels"); L_ = sub("_lib")
    hop, k, S = 40, 4, 128
    n, mc, nl, hist = k * hop, k * hop + 8, len(dil), sum(dil)
    # four slots: t = 0, a young stream (its taps still reach before time 0), ran = 0, 0 < ran < n
    t = [0, 3 * hop, 50 * hop, 40 * hop]
    ran = [n, n, 0, 2 * hop]
    cap = len(t)
    w = R_.ClassifierWeights(dil, R, S, 12, 2, dt)
    w.load_oracle_params(O.init_stack_params(3, dil, 2, R, S, 12, bias_scale=0.1))
    rng = np.random.default_rng(R + len(dil))
    buf = torch.tensor(rng.normal(0, 0.5, size=(cap, hist + mc, R)), dtype=dt, device=DEV)      # history and chunk rows
    conv, res = [w.wptr(o) for o in w.o_conv], [w.wptr(o) for o in w.o_res]
    bf, br = [w.view("BF")[l] for l in range(nl)], [w.view("BR")[l] for l in range(nl)]
    ptrs = lambda ts: K._ptr_array([x.data_ptr() for x in ts])
    dl = (C.c_int32 * nl)(*dil)
    sentinel = 7.0

    def args(B, rows, when):
        return (K._ptr_array(conv), K._ptr_array(res), ptrs(bf), ptrs(br), None, 1, 1, R, dl, nl, B, rows, mc, R, 2,
                K.abi_dtype(dt), when.data_ptr(), K._stream())
    table = torch.tensor([[a, a + r] for a, r in zip(t, ran)], dtype=torch.int64, device=DEV)
    out = torch.full((cap, mc, R), sentinel, dtype=dt, device=DEV)
    z = torch.full((nl, cap, mc, R), sentinel, dtype=dt, device=DEV)
    L_.call("srwn_residual_group_fwd_stream_z_slots", buf.data_ptr(), hist + mc, out.data_ptr(), mc, 0, z.data_ptr(),
            cap * mc * R, *args(cap, n, table))
    torch.cuda.synchronize()
    for u in range(cap):
        assert torch.all(out[u, ran[u]:] == sentinel) and torch.all(z[:, u, ran[u]:] == sentinel), u
        if ran[u] == 0:
            continue
        one = buf[u:u + 1].clone()
        clock = torch.tensor([t[u]], dtype=torch.int64, device=DEV)
        out1 = torch.full((1, mc, R), sentinel, dtype=dt, device=DEV)
        z1 = torch.full((nl, 1, mc, R), sentinel, dtype=dt, device=DEV)
        L_.call("srwn_residual_group_fwd_stream_z", one.data_ptr(), hist + mc, out1.data_ptr(), mc, 0, z1.data_ptr(),
                mc * R, *args(1, ran[u], clock))
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[u, :ran[u]]), _bits(out1[0, :ran[u]])), u
        assert torch.equal(_bits(z[:, u, :ran[u]]), _bits(z1[:, 0, :ran[u]])), u
        assert not torch.all(z1[:, 0, :ran[u]] == sentinel)


# ---- the pool ------------------------------------------------------------------------------------------------------------
def _session(name, pool):
    """The ragged session: streams 0 and 1 join first, stream 2 (shorter than the window) a step later, stream 3 into an
    explicit slot later still; pieces of 0, fewer than hop and several max_chunk samples; slot 2 sits idle with no audio
    through several steps; stream 1 leaves mid-way and stream 4 joins its slot, whose history and ring rows are stale.
    Returns ({stream: ([probabilities pieces], [logits pieces])}, {stream: samples pushed})."""
    _, _, _, _, window, hop, mh = CASES[name]
    xs = _streams(name)
    got = {s: ([], []) for s in range(len(xs))}
    slot_of, at = {}, {s: 0 for s in range(len(xs))}
    mc = mh * hop
    assert pool.audio_ring == 2 * mc + 1

    def join(s, slots=None):
        u, = pool.join(1, slots)
        slot_of[s] = u

    def push(pieces):      # {stream: samples}: one push for all of them
        ss = [s for s in pieces]
        audio = []
        for s in ss:
            n = min(pieces[s], len(xs[s]) - at[s], pool.audio_room(slot_of[s]))
            audio.append(xs[s][at[s]:at[s] + n])
            at[s] += n
        pool.push([slot_of[s] for s in ss], audio)

    def step():
        probs, logits = pool.step(return_logits=True)
        assert set(probs) == set(logits)
        back = {u: s for s, u in slot_of.items()}
        for u in probs:
            assert probs[u].shape == logits[u].shape and probs[u].shape[0] > 0
            got[back[u]][0].append(probs[u]); got[back[u]][1].append(logits[u])
        return probs

    assert pool.step() == {}                                         # nothing joined: nothing launched
    join(0); join(1)
    assert (slot_of[0], slot_of[1]) == (0, 1)
    push({0: 0, 1: hop - 1}); assert step() == {}                    # 0 samples, fewer than a hop: nothing due
    push({0: hop + 3, 1: 1}); step()
    join(2)                                                          # slot 2: joined, no audio yet -- idle through steps
    push({0: 2 * mc, 1: 2 * mc}); step()                             # several max_chunk: more than one pass
    join(3, slots=[3])
    push({0: 7, 1: mc + 5, 3: 3 * hop}); step()
    push({0: 2 * mc, 1: 2 * mc, 3: hop // 2}); step()
    push({2: len(xs[2])}); assert slot_of[2] not in step()          # shorter than the window: it emits nothing
    assert at[1] < len(xs[1])
    pool.leave(slot_of.pop(1))                                       # stream 1 leaves mid-way ...
    join(4)                                                          # ... and stream 4 takes its slot, stale rows in place
    assert slot_of[4] == 1
    for rnd in range(64):
        live = [s for s in slot_of if at[s] < len(xs[s])]
        if not live:
            break
        push({s: (1, hop - 1, 2 * mc, mc + 1)[(rnd + s) % 4] for s in live}); step()
    assert not [s for s in slot_of if at[s] < len(xs[s])]
    assert pool.step() == {}
    recv = pool.received
    for s, u in slot_of.items():
        assert recv[u] == len(xs[s]) and pool.emitted[u] == max(0, len(xs[s]) // hop - window // hop + 1)
    return got, at


def _check_session(name, got, at, want, cat=torch.cat):
    _, _, _, Cc, window, hop, _ = CASES[name]
    for s, (pp, ll) in got.items():
        n_emit = max(0, at[s] // hop - window // hop + 1)
        if n_emit == 0:
            assert not pp and not ll, s
            continue
        p, l = cat(pp), cat(ll)
        assert p.shape == (n_emit, Cc), (s, p.shape)
        for g, w in ((p, want[s][0]), (l, want[s][1])):
            w = w[:n_emit]                                            # (stream 1 left mid-way: the emissions up to there)
            if isinstance(g, np.ndarray):
                assert np.array_equal(g.view(np.uint32), w.cpu().numpy().view(np.uint32)), s
            else:
                assert torch.equal(_bits(g), _bits(w)), s


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["a", "b"])
def test_pool_streams_equal_classify_alone(name, fused, dt, monkeypatch):
    monkeypatch.setenv("SRWN_RECOG_FUSED", "1" if fused else "0")
    want = _alone(name, dt, fused)
    c = _classifier(name, dt, CAPACITY)
    assert c.fused == fused
    pool = c.pool()
    assert pool.capacity == CAPACITY and pool.launches_per_step == c.launches_per_step
    extra = pool.buffer_bytes()
    assert extra["pool audio ring"] == CAPACITY * pool.audio_ring * 4 and set(c.buffer_bytes()) < set(extra)
    got, at = _session(name, pool)
    assert [len(x) for x in _streams(name)][2] < CASES[name][4] and not got[2][0]       # the short stream emitted nothing
    assert at[1] < len(_streams(name)[1]) and got[1][0]                                 # stream 1 emitted, then left early
    _check_session(name, got, at, want)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_max_hops_changes_no_bit(dt, monkeypatch):
    monkeypatch.setenv("SRWN_RECOG_FUSED", "1")
    want = _alone("b", dt, True)
    for mh in (1, 8):
        c = _classifier("b", dt, CAPACITY, max_hops=mh)
        pool = c.pool(audio_ring=2 * CASES["b"][6] * CASES["b"][5] + 1)      # the session's ring, whatever max_hops
        got, at = _session("b", pool)
        _check_session("b", got, at, want)
        assert set(pool._seen) <= set(range(1, mh + 1)) and mh in pool._seen


@pytest.mark.parametrize("dt", [F32, BF16])
def test_graph_replay_changes_no_bit(dt, monkeypatch):
    monkeypatch.setenv("SRWN_RECOG_FUSED", "1")
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "1")
    g = _classifier("a", dt, CAPACITY)
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    e = _classifier("a", dt, CAPACITY)
    assert g.use_graphs and not e.use_graphs
    want = _alone("a", dt, True)
    gp, ep = g.pool(), e.pool()
    for rep in range(2):      # the second session replays every graph the first one captured, on other slots' contents
        for pool in (gp, ep):
            for u in pool.active:
                pool.leave(u)
            got, at = _session("a", pool)
            _check_session("a", got, at, want)
    assert not ep._graphs and gp._graphs and set(gp._graphs) == set(gp._seen)      # every k that occurred was replayed


def test_numpy_face(monkeypatch):
    monkeypatch.setenv("SRWN_RECOG_FUSED", "1")
    M = sub("model")
    R_ = sub("recognizer")
    dil, R, S, Cc, window, hop, mh = CASES["a"]
    w = R_.ClassifierWeights(dil, R, S, Cc, 2, F32)
    w.load_oracle_params(_params("a"))
    one = M.StreamingClassifier(w, max_batch=1, hop=hop, window=window, max_hops=mh)
    want = []
    for x in _streams("a"):
        p, l = one.classify(np.array(x[None]), return_logits=True)
        assert isinstance(p, np.ndarray)
        want.append((torch.from_numpy(p[0]), torch.from_numpy(l[0])))
    rec = M.StreamingClassifier(w, max_batch=CAPACITY, hop=hop, window=window, max_hops=mh)
    pool = rec.pool()
    assert isinstance(pool, M.ClassifierPool) and pool.capacity == CAPACITY and pool.free == [0, 1, 2, 3]
    got, at = _session("a", pool)
    assert all(isinstance(p, np.ndarray) for s in got for p in got[s][0] + got[s][1])
    _check_session("a", got, at, want, cat=np.concatenate)


def test_one_face_at_a_time():
    c = _classifier("a", F32, 2)
    x = torch.tensor(np.stack([s[:200] for s in _streams("a")[:2]]))
    st = c.start(2)
    c.push(st, x[:, :50])
    pool = c.pool()
    with pytest.raises(ValueError, match="not the classifier's current"):
        c.push(st, x[:, 50:])                                        # the pool ended the state
    u, = pool.join()
    pool.push(u, x[0].numpy())
    assert pool.step()[u].shape == (200 // 32 - 4 + 1, 12)
    with pytest.raises(ValueError, match="audio_ring"):
        c.pool(audio_ring=4 * 32)                                    # refused: the pool in use stays
    pool.push(u, x[1, :32].numpy())
    other = c.pool()                                                 # another pool ends this one
    with pytest.raises(ValueError, match="closed"):
        pool.step()
    st = c.start(2)                                                  # ... and start() ends the pool
    for call in (lambda: other.join(), lambda: other.push(0, x[0].numpy()), lambda: other.step(), lambda: other.leave(0)):
        with pytest.raises(ValueError, match="closed"):
            call()
    assert c.push(st, x).shape == (2, 3, 12)
