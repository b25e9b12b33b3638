"""GPU tests of scorer pools (srwn_version() 118; scorer.ScorerPool, model.StreamingScorer.pool).  Every comparison in this
file is bit for bit; the one bound, on the running means, is fp64 round-off.

  entry       srwn_score_stream_in_slots against srwn_recog_stream_in on the hand-delayed audio of each slot alone and
              srwn_mu_law_encode of its samples: t = 0, one tap before time 0, ran = 0, a ring wrap with a ragged ran
  head        srwn_stream_score_head_slots / srwn_nll_rows_slots against one clock-form call per slot with n = ran(u)
  session     five streams in four slots, joining and leaving at their own times, against StreamScorer(max_batch=1).score
              of each alone: both dtypes, the fused head and its twin
  invariance  max_chunk, graph replay and a second session on the same pool change no bit
  model       the NumPy face, from_checkpoint, one face at a time; buffer_bytes
"""
import math

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DEV = "cuda"
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 1, 2, 5]      # both group kinds, and a history longer than a chunk
MAX_CHUNK, CAP = 128, 4
CASES = {"a": (64, 256, 256), "b": (32, 128, 100), "c": (32, 128, 256)}      # R, S, classes (100: padded columns)
LENGTHS = {"A": 300, "B": 1, "C": 131, "D": 517, "E": 64}
SPECIAL = [-1.0, 1.0, 0.0, -0.0, 1.5, -1.5, 1e-30]
_PARAMS, _AUDIO, _ALONE = {}, {}, {}


def _bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(t))
    return t.contiguous().view(torch.uint8)


def _params(name):
    if name not in _PARAMS:
        R, S, Cc = CASES[name]
        _PARAMS[name] = O.init_stack_params(11, DIL, 2, R, S, Cc, bias_scale=0.05)
    return _PARAMS[name]


def _streams():
    """The five streams' audio, made once and never changed; the special sample values lie in stream A's first piece and
    across the first ring wrap of stream D."""
    if not _AUDIO:
        for i, (k, n) in enumerate(LENGTHS.items()):
            _AUDIO[k] = O.synthetic_audio(1, n, seed=20 + i)[0].astype(np.float32)
        _AUDIO["A"][3:3 + len(SPECIAL)] = SPECIAL
        _AUDIO["D"][254:254 + len(SPECIAL)] = SPECIAL
        for a in _AUDIO.values():
            a.setflags(write=False)
    return _AUDIO


def _weights(name, dt):
    Sc = sub("scorer")
    R, S, Cc = CASES[name]
    w = Sc.ScorerWeights(DIL, R, S, Cc, 2, dt)
    w.load_oracle_params(_params(name))
    return w


def _scorer(name, dt, monkeypatch, fused=True, max_batch=CAP, max_chunk=MAX_CHUNK, graphs=True):
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1" if fused else "0")
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "1" if graphs else "0")
    s = sub("scorer").StreamScorer(_weights(name, dt), max_batch=max_batch, max_chunk=max_chunk)
    assert s.fused == fused and s.use_graphs == graphs
    return s


def _alone(name, dt, monkeypatch):
    """stream -> (nll [T], logits [T, C], best [T]) of StreamScorer(max_batch=1).score of that stream alone: once per case."""
    key = (name, dt)
    if key not in _ALONE:
        one = _scorer(name, dt, monkeypatch, max_batch=1)
        _ALONE[key] = {k: tuple(o[0].clone() for o in one.score(x[None], return_logits=True, return_best=True))
                       for k, x in _streams().items()}
    return _ALONE[key]


# ---- the table of the two kernel tests: t = 0; one tap before time 0; ran = 0; a ring wrap with 0 < ran < n, ran % 32 != 0
RING = 150                      # >= MAX_CHUNK + 2, and short enough that a chunk of 128 wraps
N = MAX_CHUNK
T0 = [0, 1, 77, 3 * RING + 5]
RAN = [N, N, 0, 45]


def _table():
    return torch.tensor([[a, a + r] for a, r in zip(T0, RAN)], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("R,Cc", [(64, 256), (32, 100)])
def test_entry_against_the_clock_form_and_mu_law(R, Cc, dt):
    K = sub("kernels"); L_ = sub("_lib")
    rng = np.random.default_rng(R + Cc)
    hist, mc, sentinel = 11, MAX_CHUNK, 7.0
    init_w = torch.tensor(rng.normal(0, 0.5, (2, R)), dtype=F32, device=DEV)
    init_b = torch.tensor(rng.normal(0, 0.1, R), dtype=F32, device=DEV)
    audio = []                  # per slot, its stream from time 0 to the end of the chunk
    for u in range(CAP):
        a = rng.uniform(-1.2, 1.2, T0[u] + max(RAN[u], 1)).astype(np.float32)
        at = T0[u] + (3 if RAN[u] > 20 else 0)
        a[at:at + len(SPECIAL)] = SPECIAL[:max(0, len(a) - at)]
        audio.append(a)
    ring = np.full((CAP, RING), np.nan, np.float32)      # what the kernel must not read is NaN
    for u in range(CAP):
        for s in range(max(T0[u] - 2, 0), T0[u] + RAN[u]):
            ring[u, s % RING] = audio[u][s]
    ring = torch.tensor(ring, device=DEV)
    out = torch.full((CAP, hist + mc, R), sentinel, dtype=dt, device=DEV)
    codes = torch.full((CAP, mc), -77, dtype=torch.int32, device=DEV)
    L_.call("srwn_score_stream_in_slots", ring.data_ptr(), RING, init_w.data_ptr(), init_b.data_ptr(), out.data_ptr(),
            hist + mc, hist, codes.data_ptr(), mc, CAP, N, mc, R, Cc, K.abi_dtype(dt), _table().data_ptr(), K._stream())
    torch.cuda.synchronize()
    for u in range(CAP):
        t, ran = T0[u], RAN[u]
        assert torch.all(out[u, :hist] == sentinel) and torch.all(out[u, hist + ran:] == sentinel), u
        assert torch.all(codes[u, ran:] == -77), u
        if ran == 0:
            continue
        a = np.concatenate([np.zeros(2, np.float32), audio[u]])      # a[s + 2] = sample s, zeros before time 0
        delayed = torch.zeros((1, mc), dtype=F32, device=DEV)
        delayed[0, :ran] = torch.tensor(a[t + 1:t + 1 + ran])         # x'[i] = sample t + i - 1
        carry = torch.tensor(a[t:t + 1], device=DEV)                  # sample t - 2
        out1 = torch.full((1, hist + mc, R), sentinel, dtype=dt, device=DEV)
        L_.call("srwn_recog_stream_in", delayed.data_ptr(), mc, carry.data_ptr(), init_w.data_ptr(), init_b.data_ptr(),
                out1.data_ptr(), hist + mc, hist, 1, ran, mc, R, K.abi_dtype(dt), K._stream())
        want_codes = K.mu_law_encode(torch.tensor(audio[u][t:t + ran], device=DEV), Cc)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[u, hist:hist + ran]), _bits(out1[0, hist:hist + ran])), u
        assert not torch.all(out1[0, hist:hist + ran] == sentinel) and not torch.isnan(out[u, hist:hist + ran].float()).any()
        assert torch.equal(codes[u, :ran], want_codes), u
        assert 0 <= int(want_codes.min()) and int(want_codes.max()) < Cc
    sp = torch.tensor(SPECIAL, device=DEV)      # the special targets were among them, with srwn_mu_law_encode's codes
    assert torch.equal(codes[0, 3:3 + len(SPECIAL)], K.mu_law_encode(sp, Cc))
    assert torch.equal(codes[3, 3:3 + len(SPECIAL)], K.mu_law_encode(sp, Cc))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_head_slot_forms_against_the_clock_forms(name, dt):
    K = sub("kernels"); L_ = sub("_lib")
    R, S, Cc = CASES[name]
    w = _weights(name, dt)
    rng = np.random.default_rng(len(name) + R)
    mc, L, es = MAX_CHUNK, len(DIL), torch.tensor([], dtype=dt).element_size()
    z = torch.tensor(rng.normal(0, 0.5, (L, CAP, mc, R)), dtype=dt, device=DEV)
    codes = torch.tensor(rng.integers(0, Cc, (CAP, mc)), dtype=torch.int32, device=DEV)
    logits32 = torch.tensor(rng.normal(0, 2.0, (CAP, mc, w.Cp)), dtype=F32, device=DEV)
    images = (L, w.wptr(w.o_skip), w.bs_sum.data_ptr(), w.wptr(w.o_w1), w.view("head_b1").data_ptr(), w.wptr(w.o_w2),
              w.view("head_b2").data_ptr())
    dti, st, table = K.abi_dtype(dt), K._stream(), _table()

    def outs(rows):
        return (torch.full((rows, mc), 7.0, dtype=F32, device=DEV), torch.full((rows, mc), -77, dtype=torch.int32, device=DEV),
                torch.full((rows, mc, Cc), 7.0, dtype=F32, device=DEV))

    def ptrs(o):
        return tuple(t.data_ptr() for t in o)

    for twin in (False, True):
        got = outs(CAP)
        if twin:
            L_.call("srwn_nll_rows_slots", logits32.data_ptr(), w.Cp, mc, codes.data_ptr(), *ptrs(got), mc, CAP, N, Cc,
                    table.data_ptr(), st)
        else:
            L_.call("srwn_stream_score_head_slots", z.data_ptr(), CAP * mc * R, mc, *images, codes.data_ptr(), *ptrs(got), mc,
                    CAP, N, mc, R, S, Cc, dti, table.data_ptr(), st)
        torch.cuda.synchronize()
        for u in range(CAP):
            ran = RAN[u]
            assert torch.all(got[0][u, ran:] == 7.0) and torch.all(got[1][u, ran:] == -77) and torch.all(got[2][u, ran:] == 7.0), u
            if ran == 0:
                continue
            one = outs(1)
            cu = codes.data_ptr() + u * mc * 4
            if twin:
                L_.call("srwn_nll_rows", logits32.data_ptr() + u * mc * w.Cp * 4, w.Cp, mc, cu, *ptrs(one), mc, 1, ran, Cc, st)
            else:
                L_.call("srwn_stream_score_head", z.data_ptr() + u * mc * R * es, CAP * mc * R, mc, *images, cu, *ptrs(one), mc,
                        1, ran, mc, R, S, Cc, dti, st)
            torch.cuda.synchronize()
            for i in range(3):
                assert torch.equal(_bits(got[i][u, :ran]), _bits(one[i][0, :ran])), (twin, u, i)
            assert torch.isfinite(one[0][0, :ran]).all() and 0 <= int(one[1][0, :ran].min()) and int(one[1][0, :ran].max()) < Cc


# ---- the pool ------------------------------------------------------------------------------------------------------------
def _session(pool):
    """The ragged session: A and B join first, C a step later, D into an explicit slot; pieces of 0, 1, 31, 33, 100, 235,
    256 samples; B (one sample long) sits idle in its slot from the first step on; C leaves mid-way, 31 of its samples
    pushed but never scored, and E joins its slot -- whose history rows, audio and clock are C's and must all start over.
    -> stream -> [(nll, logits, best)] pieces in order, and the running means read at the end."""
    x = _streams()
    got = {k: [] for k in x}
    owner = {}

    def step():
        out = pool.step(return_logits=True, return_best=True)
        assert isinstance(out, tuple) and len(out) == 3 and set(out[0]) == set(out[1]) == set(out[2])
        for u in out[0]:
            got[owner[u]].append(tuple(o[u] for o in out))
        return {owner[u]: int(v.shape[0]) for u, v in out[0].items()}

    assert pool.join(2) == [0, 1]
    owner.update({0: "A", 1: "B"})
    assert math.isnan(pool.bits_per_sample(0)) and pool.step() == {}
    pool.push([0, 1], [x["A"][:31], x["B"]])
    assert step() == {"A": 31, "B": 1}
    assert pool.join() == [2]
    owner[2] = "C"
    pool.push([0, 2], [x["A"][31:64], x["C"][:0]])
    assert step() == {"A": 33}
    assert pool.join(slots=[3]) == [3]
    owner[3] = "D"
    assert pool.audio_room(3) == pool.audio_ring - 2 >= 256
    pool.push([0, 2, 3], [x["A"][64:65], x["C"][:100], x["D"][:256]])
    assert step() == {"A": 1, "C": 100, "D": 256}
    pool.push([3, 0], [x["D"][256:512], x["A"][65:]])
    assert step() == {"A": 235, "D": 256}
    assert step() == {}                                        # nothing waits: nothing is launched
    pool.push(2, x["C"][100:])
    pool.leave(2)                                              # mid-way: its last 31 samples are never scored
    assert pool.join() == [2]
    owner[2] = "E"
    assert math.isnan(pool.bits_per_sample(2)) and pool.received[2] == 0 and pool.scored[2] == 0
    pool.push([2, 3], [x["E"], x["D"][512:]])
    assert step() == {"E": 64, "D": 5}
    assert pool.scored.tolist() == [300, 1, 64, 517] == pool.received.tolist()
    means = {owner[u]: pool.bits_per_sample(u) for u in range(CAP)}
    sums = dict(zip((owner[u] for u in range(CAP)), pool.nll_sum.tolist()))
    pool.leave(pool.active)
    assert pool.free == [0, 1, 2, 3]
    return got, means, sums


def _check_session(got, want, means=None, sums=None):
    scored = dict(LENGTHS, C=100)
    for k, pieces in got.items():
        for i in range(3):
            cat = torch.cat([p[i] for p in pieces], 0)
            assert cat.shape[0] == scored[k]
            assert torch.equal(_bits(cat), _bits(want[k][i][:scored[k]])), (k, i)
    if means is None:
        return
    for k in "ABDE":      # the slots' streams at the end: the running mean is the fp64 mean of what the slot returned, in bits;
        # the two sums add the same <= 1e4 fp32 values in fp64 in different orders: each step loses at most 2^-53 relative
        nll = torch.cat([p[0] for p in got[k]], 0).double().cpu().numpy()
        assert abs(means[k] - nll.mean() / math.log(2.0)) <= 1e-12 * abs(means[k]), k
        assert abs(sums[k] - nll.sum()) <= 1e-12 * abs(sums[k]), k


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twin"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_pool_streams_equal_score_alone(name, fused, dt, monkeypatch):
    want = _alone(name, dt, monkeypatch)
    s = _scorer(name, dt, monkeypatch, fused=fused)
    pool = s.pool()
    assert pool.capacity == CAP and pool.audio_ring == 2 * MAX_CHUNK + 2
    assert pool.launches_per_step == 2 + len(s.groups) + (1 if fused else 4)
    got, means, sums = _session(pool)
    _check_session(got, want, means, sums)
    assert set(pool._graphs) <= {(n, True, True) for n in (32, 64, 96, 128)} and pool._graphs


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_chunk_graphs_and_a_second_session_change_no_bit(dt, monkeypatch):
    name = "b"
    want = _alone(name, dt, monkeypatch)
    pool = _scorer(name, dt, monkeypatch).pool()
    _check_session(_session(pool)[0], want)
    assert pool._graphs
    _check_session(_session(pool)[0], want)                   # the same pool again: every step a replay, every slot stale
    small = _scorer(name, dt, monkeypatch, max_chunk=32).pool(audio_ring=2 * MAX_CHUNK + 2)
    _check_session(_session(small)[0], want)
    assert set(small._graphs) == {(32, True, True)}
    eager = _scorer(name, dt, monkeypatch, graphs=False).pool()
    _check_session(_session(eager)[0], want)
    assert not eager._graphs


def test_pool_state_and_serial_interplay(monkeypatch):
    s = _scorer("b", F32, monkeypatch)
    x = _streams()["E"]
    st = s.start(2)
    pool = s.pool()
    with pytest.raises(ValueError, match="current"):
        s.push(st, np.zeros((2, 4), np.float32))              # pool() ended the state
    u, = pool.join()
    pool.push(u, x[:10])
    second = s.pool()                                          # ... and an earlier pool
    with pytest.raises(ValueError, match="closed"):
        pool.step()
    v, = second.join()
    second.push(v, x)
    want = _alone("b", F32, monkeypatch)["E"]
    assert torch.equal(_bits(second.step()[v]), _bits(want[0]))
    nll = s.score(x[None])                                     # score() -> start(): the pool closes
    assert torch.equal(_bits(nll[0]), _bits(want[0]))
    for call in (lambda: second.join(), lambda: second.push(v, x[:1]), lambda: second.step(), lambda: second.leave(v)):
        with pytest.raises(ValueError, match="closed"):
            call()
    with pytest.raises(ValueError, match="audio_ring"):
        s.pool(audio_ring=MAX_CHUNK + 1)
    assert s.pool(audio_ring=MAX_CHUNK + 2).audio_ring == MAX_CHUNK + 2


def test_buffer_bytes(monkeypatch):
    s = _scorer("b", BF16, monkeypatch)
    pool = s.pool()
    bb, ring = pool.buffer_bytes(), 2 * MAX_CHUNK + 2
    assert bb["pool audio ring"] == CAP * ring * 4
    assert bb["pool stage + table"] == (4 * CAP + CAP * ring) * 4 + CAP * 2 * 8
    assert {k: v for k, v in bb.items() if not k.startswith("pool ")} == s.buffer_bytes()
    assert s.pool(audio_ring=500).buffer_bytes()["pool audio ring"] == CAP * 500 * 4
    twin = _scorer("b", BF16, monkeypatch, fused=False).pool().buffer_bytes()
    assert "twin r0/r1/logits" in twin and "pool audio ring" in twin


# ---- the model face --------------------------------------------------------------------------------------------------------
def test_model_face(tmp_path, monkeypatch):
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1")
    M = sub("model")
    dil, Tm, R, S, Cc = [1, 2, 4, 8, 1, 2], 200, 32, 128, 256
    m = M.WaveNetTeacher(Tm, 0, dil, dilation_channels=R, skip_channels=S, quantization_channels=Cc, dtype=F32, seed=3)
    rng = np.random.default_rng(8)
    xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (150, 70, 1)]
    sc = m.scorer(max_batch=4, max_chunk=64)
    want = [sc.score(x[None], return_best=True) for x in xs]
    pool = sc.pool()
    assert isinstance(pool, M.ScorerStreamPool) and pool.capacity == 4 and pool.audio_ring == 130
    us = pool.join(3)
    assert us == [0, 1, 2] and pool.free == [3] and np.isnan(pool.bits_per_sample(0))
    pool.push(us, [x[:40] for x in xs])
    first = pool.step(return_best=True)
    pool.push(us[:2], [x[40:] for x in xs[:2]])
    rest = pool.step(return_best=True)
    assert set(first[0]) == {0, 1, 2} and set(rest[0]) == {0, 1}
    for u, x in zip(us, xs):
        for i in range(2):
            cat = np.concatenate([d[i][u] for d in (first, rest) if u in d[i]])
            assert isinstance(cat, np.ndarray) and np.array_equal(cat, want[u][i][0]), (u, i)
    assert pool.received.tolist() == [150, 70, 1, 0] == pool.scored.tolist() and pool.audio_room(0) == 128
    nll0 = want[0][0][0].astype(np.float64)
    assert abs(pool.bits_per_sample(0) - nll0.mean() / math.log(2.0)) <= 1e-12 * pool.bits_per_sample(0)
    assert pool.step() == {}
    st = sc.stream(1)                                          # stream() closes the pool
    with pytest.raises(ValueError, match="closed"):
        pool.step()
    with pytest.raises(ValueError, match="closed"):
        pool.join()
    assert np.array_equal(st.push(xs[1][None]), want[1][0])
    again = sc.pool()
    with pytest.raises(ValueError, match="current"):
        st.push(xs[1][None])                                   # ... and pool() the stream
    assert again.join() == [0]
    # save -> from_checkpoint(...).pool()
    assert m.save(str(tmp_path), 5, force=True)
    p2 = M.StreamingScorer.from_checkpoint(str(tmp_path), dtype=F32, max_batch=2, max_chunk=64).pool(audio_ring=200)
    assert p2.capacity == 2 and p2.audio_ring == 200
    u, = p2.join(slots=[1])
    p2.push(u, xs[0])
    out = p2.step()
    assert set(out) == {1} and np.array_equal(out[1], want[0][0][0])
