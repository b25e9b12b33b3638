"""GPU tests of embedder pools (srwn_version() 120; embedder.EmbedderPool, model.StreamingEmbedder.pool).

The one claim is bit equality: a stream's ``EmbedResult`` from a pool is ``StreamEmbedder(max_batch=1).embed`` of that stream
alone under the same gallery -- embeddings, distances, nearest row and its distance -- in any slot, whenever it joined,
however its audio was cut, whatever k the steps had and whatever the other slots hold or held before.  There is no tolerance
in this file; the lockstep embedder is held to the fp64 oracle in tests/test_gpu_embedder.py.
"""
import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_embedder import CASES, MAX_GALLERY, MAX_HOPS, _bits, _oracle, _same, _weights

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
CAPACITY, N_GALLERY = 4, 70
_AUDIO = {}


def _streams(name):
    """Five streams of different lengths, the third shorter than the window (it emits nothing): computed once, read-only."""
    if name not in _AUDIO:
        hop, window = CASES[name][4:]
        mc = MAX_HOPS * hop
        lengths = [window + 5 * hop + 3, 6 * mc + 2 * hop + 7, window - 1, 2 * window + mc + hop // 2, window + 2 * mc + 1]
        audio = O.synthetic_audio(len(lengths), max(lengths), seed=6).astype(np.float32)
        audio.setflags(write=False)
        _AUDIO[name] = [audio[i, :n] for i, n in enumerate(lengths)]
    return _AUDIO[name]


def _embedder(name, dt, max_batch, n_gallery=N_GALLERY):
    hop, window = CASES[name][4:]
    e = sub("embedder").StreamEmbedder(_weights(name, dt), max_batch=max_batch, hop=hop, window=window, max_hops=MAX_HOPS,
                                       max_gallery=MAX_GALLERY)
    e.enroll(_oracle(name)[3][:n_gallery])
    return e


def _session(name, pool, between=None):
    """The ragged session of tests/test_gpu_recognizer_pool.py on five streams in four slots: joins at different steps, pieces
    of 0, fewer than hop and several max_chunk samples, slot 2 idle through several steps, stream 1 leaves mid-way and
    stream 4 takes its slot with stale rows in place.  between(): called once, between two steps in the middle.  Returns
    ({stream: [EmbedResult pieces]}, {stream: samples pushed}, the number of pieces each stream had when between ran)."""
    hop, window = CASES[name][4:]
    xs = _streams(name)
    got = {s: [] for s in range(len(xs))}
    slot_of, at = {}, {s: 0 for s in range(len(xs))}
    mc = MAX_HOPS * hop
    assert pool.audio_ring == 2 * mc + 1

    def join(s, slots=None):
        u, = pool.join(1, slots)
        slot_of[s] = u

    def push(pieces):      # {stream: samples}: one push for all of them
        ss = list(pieces)
        audio = []
        for s in ss:
            n = min(pieces[s], len(xs[s]) - at[s], pool.audio_room(slot_of[s]))
            audio.append(xs[s][at[s]:at[s] + n])
            at[s] += n
        pool.push([slot_of[s] for s in ss], audio)

    def step():
        out = pool.step()
        back = {u: s for s, u in slot_of.items()}
        assert set(out) <= set(back)                                  # an idle or free slot's rows never appear
        for u, r in out.items():
            e = r.embeddings.shape[0]
            assert e > 0 and r.nearest.shape == r.distance.shape == (e,) and r.distances.shape[0] == e
            got[back[u]].append(r)
        return out

    assert pool.step() == {}                                         # nothing joined: nothing launched
    join(0); join(1)
    push({0: 0, 1: hop - 1}); assert step() == {}                    # 0 samples, fewer than a hop: nothing due
    push({0: hop + 3, 1: 1}); step()
    join(2)                                                          # slot 2: joined, no audio yet -- idle through steps
    push({0: 2 * mc, 1: 2 * mc}); step()                             # several max_chunk: more than one pass
    join(3, slots=[3])
    push({0: 7, 1: mc + 5, 3: 3 * hop}); step()
    seen = {s: len(p) for s, p in got.items()}
    if between is not None:
        between()
    push({0: 2 * mc, 1: 2 * mc, 3: hop // 2}); step()
    push({2: len(xs[2])}); assert slot_of[2] not in step()          # shorter than the window: it emits nothing
    assert at[1] < len(xs[1])
    pool.leave(slot_of.pop(1))                                       # stream 1 leaves mid-way ...
    join(4)                                                          # ... and stream 4 takes its slot
    assert slot_of[4] == 1
    rng = np.random.default_rng(8)
    for rnd in range(64):
        live = [s for s in slot_of if at[s] < len(xs[s])]
        if not live:
            break
        push({s: int(rng.choice([0, 1, hop - 1, 2 * mc, mc + 1])) if rnd else 1 for s in live}); step()
    assert not [s for s in slot_of if at[s] < len(xs[s])]
    assert pool.step() == {}
    for s, u in slot_of.items():
        assert pool.received[u] == len(xs[s]) and pool.emitted[u] == max(0, len(xs[s]) // hop - window // hop + 1)
    return got, at, seen


def _cat(pieces):
    return [torch.cat(f, 0) for f in zip(*pieces)]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["a", "b"])
def test_pool_streams_equal_embed_alone(name, fused, dt, monkeypatch):
    monkeypatch.setenv("SRWN_EMBED_FUSED", "1" if fused else "0")
    hop, window = CASES[name][4:]
    alone = _embedder(name, dt, 1)
    e = _embedder(name, dt, CAPACITY)
    assert e.embed_fused == alone.embed_fused == fused
    pool = e.pool()
    assert pool.capacity == CAPACITY and pool.launches_per_step == e.launches_per_step
    got, at, _ = _session(name, pool)
    assert pool._graphs                                               # steps were replayed
    for s, x in enumerate(_streams(name)):
        n_emit = max(0, at[s] // hop - window // hop + 1)
        if n_emit == 0:
            assert not got[s], s
            continue
        want = [f[0, :n_emit] for f in alone.embed(np.array(x[None]))]      # (stream 1 left mid-way: the results up to there)
        assert want[0].shape[0] == n_emit and _same(_cat(got[s]), want), s
    with pytest.raises(ValueError, match="closed"):                   # start() ends the pool
        e.start(1)
        pool.step()


def test_enrolling_between_two_steps_reaches_the_later_steps_only(monkeypatch):
    """Two more templates enrolled in the middle of a session: every embedding is what it was, the results before are
    matched against 70 rows, those after against 72 -- and equal srwn_gallery_match on the emitted embeddings."""
    L_ = sub("_lib"); K = sub("kernels")
    name, dt = "a", F32
    D = CASES[name][2]
    extra = _oracle(name)[3][N_GALLERY:N_GALLERY + 2]
    base = _embedder(name, dt, CAPACITY)
    ref, _, _ = _session(name, base.pool())
    e = _embedder(name, dt, CAPACITY)
    got, _, seen = _session(name, e.pool(), between=lambda: e.enroll(extra))
    assert e.labels == list(range(N_GALLERY + 2))
    count = torch.tensor([N_GALLERY + 2], dtype=torch.int32, device=DEV)
    for s in got:
        assert len(got[s]) == len(ref[s])
        for i, (r, w) in enumerate(zip(got[s], ref[s])):
            assert torch.equal(_bits(r.embeddings), _bits(w.embeddings))
            if i < seen[s]:
                assert _same(r, w)
                continue
            rows = r.embeddings.shape[0]
            assert r.distances.shape == (rows, N_GALLERY + 2)
            assert torch.equal(_bits(r.distances[:, :N_GALLERY]), _bits(w.distances))
            dist = torch.zeros((rows, MAX_GALLERY), device=DEV)
            near = torch.zeros(rows, dtype=torch.int32, device=DEV)
            dmin = torch.zeros(rows, device=DEV)
            L_.call("srwn_gallery_match", r.embeddings.contiguous().data_ptr(), rows, D, e.gallery_buf.data_ptr(),
                    count.data_ptr(), MAX_GALLERY, dist.data_ptr(), near.data_ptr(), dmin.data_ptr(), K._stream())
            assert _same(r, (r.embeddings, near, dmin, dist[:, :N_GALLERY + 2]))
    assert sum(len(p) - seen[s] for s, p in got.items()) > 0 and sum(seen.values()) > 0


def test_numpy_face(monkeypatch):
    """model.StreamingEmbedder.pool(): NumPy in, NumPy out, the same bits; a threshold adds ``accepted``."""
    M = sub("model")
    name, dt = "c", BF16
    hop, window = CASES[name][4:]
    face = M.StreamingEmbedder(_weights(name, dt), max_batch=CAPACITY, hop=hop, window=window, max_hops=MAX_HOPS,
                               max_gallery=MAX_GALLERY)
    face.enroll_embeddings(_oracle(name)[3][:N_GALLERY])
    x = _streams(name)[0]
    want = face.embed(x[None])
    pool = face.pool()
    u, v = pool.join(2)
    pool.push([u, v], [x[:100], x[:200]])
    first = pool.step()
    pool.push([u, v], [x[100:], x[200:]])
    threshold = float(np.median(want.distance))
    second = pool.step(threshold=threshold)
    assert isinstance(first[v].embeddings, np.ndarray) and pool.received[v] == len(x) and pool.emitted[u] == want.nearest.shape[1]
    for slot in (u, v):
        res, ok = second[slot]
        for i, f in enumerate(want):
            assert np.array_equal(np.concatenate([first[slot][i], res[i]]), f[0]), (slot, i)
        assert ok.dtype == bool and np.array_equal(ok, res.distance <= np.float32(threshold))
    assert 0 < sum(int(second[s][1].sum()) for s in (u, v)) < sum(second[s][1].size for s in (u, v))
