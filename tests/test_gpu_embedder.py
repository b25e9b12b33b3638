"""GPU tests of the streaming embedder (srwn_version() 120; embedder.StreamEmbedder, model.SiameseWaveNet.embedder).

  oracle      embeddings against the fp64 oracle's sliding average of the last 1x1 (oracle.wavenet_np.stack_forward), both
              dtypes; distances against fp64 NumPy on the returned fp32 embeddings
  bits        embeddings are StreamClassifier's pooled logits; the fused head is its twin; eager is replayed; chunking,
              batch size and batch row change nothing; the gallery may change under a captured graph
  matching    nearest / dmin are the argmin / min of the kernel's own distances, lowest index on ties; N = 0, 1, 70, 96
  model       hop = window = input_size: SiameseWaveNet.get_embedding; from_checkpoint after save
"""
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, rel_err

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
# fp32: the project's parity bar.  bf16: twice the worst error measured on MI355X against the fp64 oracle over the cases
# below (SRWN_PRINT_ERR=1 pytest -s prints every figure), relative to the largest oracle value.  Measured:
#   case a: 1.68e-3        case b: 1.83e-3        case c: 2.36e-3        (fp32: 4.6e-7, 4.8e-7, 2.7e-7)
TOL_F32 = 1e-3
MEASURED_BF16_EMB = 2.36e-3
TOL_BF16_EMB = 2 * MEASURED_BF16_EMB
# Distances: a sum of D <= 256 non-negative fp32 squares, each with relative error <= 3 * 2^-24, accumulated in any order,
# is within (D + 3) * 2^-24 < 1.6e-5 of d^2; the square root halves that and adds one rounding.  (Measured: 1.5e-7.)
TOL_DIST = 2e-5

DIL, T, MAX_HOPS, MAX_GALLERY = [1, 2, 4, 8, 1, 2], 500, 3, 96
CASES = {      # name: R, S, D, B, hop, window
    "a": (32, 128, 40, 3, 32, 96),
    "b": (64, 256, 256, 1, 40, 80),
    "c": (32, 128, 2, 3, 40, 80),
}
N_EMIT = {"a": 13, "b": 11, "c": 11}
_ORACLE = {}


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    """Two EmbedResults agree bit for bit, field by field."""
    return all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _oracle(name):
    """(params, audio, embeddings [B, n_emit, D] fp64, gallery [MAX_GALLERY, D] fp32) of a case: computed once, shared,
    never changed.  The gallery: random rows of the embeddings' scale about their mean."""
    if name not in _ORACLE:
        R, S, D, B, hop, window = CASES[name]
        sp = O.init_stack_params(11, DIL, 2, R, S, D, bias_scale=0.05)
        audio = O.synthetic_audio(B, T, seed=4)
        out_t, _ = O.stack_forward(sp, audio.astype(np.float64))
        pos = [(j + 1) * hop - window for j in range(window // hop - 1, T // hop)]
        emb = np.stack([out_t[:, p:p + window].mean(1) for p in pos], 1)      # the mean commutes with the last 1x1
        rng = np.random.default_rng(5)
        gal = (emb.mean((0, 1)) + emb.std() * rng.standard_normal((MAX_GALLERY, D))).astype(np.float32)
        for a in (audio, emb, gal):
            a.setflags(write=False)
        _ORACLE[name] = (sp, audio, emb, gal)
    return _ORACLE[name]


def _weights(name, dt, cls=None):
    R, S, D = CASES[name][:3]
    w = (cls or sub("embedder").EmbedderWeights)(DIL, R, S, D, 2, dt)
    w.load_oracle_params(_oracle(name)[0])
    return w


def _embedder(name, dt, monkeypatch, fused=True, max_batch=None, n_gallery=0, graphs=True):
    _, _, _, B, hop, window = CASES[name]
    monkeypatch.setenv("SRWN_EMBED_FUSED", "1" if fused else "0")
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "1" if graphs else "0")
    e = sub("embedder").StreamEmbedder(_weights(name, dt), max_batch=max_batch or B, hop=hop, window=window, max_hops=MAX_HOPS,
                                       max_gallery=MAX_GALLERY)
    assert e.embed_fused == fused and e.use_graphs == graphs
    assert e.launches_per_step == len(e.groups) + (4 if fused else 5)
    if n_gallery:
        assert e.enroll(_oracle(name)[3][:n_gallery]) == list(range(n_gallery))
    return e


def _audio(name):
    return torch.tensor(_oracle(name)[1])


# ---- 1. the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_embeddings_against_the_oracle(name, dt, monkeypatch):
    e = _embedder(name, dt, monkeypatch)
    r = e.embed(_audio(name))
    want = _oracle(name)[2]
    B, D = CASES[name][3], CASES[name][2]
    assert tuple(r.embeddings.shape) == want.shape == (B, N_EMIT[name], D)
    assert e._state.emitted == N_EMIT[name] and e._state.t == T
    # an empty gallery: no column, no nearest row
    assert tuple(r.distances.shape) == (B, N_EMIT[name], 0)
    assert bool((r.nearest == -1).all()) and bool(torch.isinf(r.distance).all()) and bool((r.distance > 0).all())
    err = rel_err(r.embeddings.cpu().numpy(), want)
    _say("embeddings against the oracle, case %s %s: %.3g" % (name, dt, err))
    assert err < (TOL_F32 if dt == F32 else TOL_BF16_EMB)


# ---- 2. a tower is the classifier up to the last 1x1 -------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_embeddings_are_the_classifiers_logits(name, dt, monkeypatch):
    R_ = sub("recognizer")
    _, _, _, B, hop, window = CASES[name]
    c = R_.StreamClassifier(_weights(name, dt, R_.ClassifierWeights), max_batch=B, hop=hop, window=window, max_hops=MAX_HOPS)
    logits = c.classify(_audio(name), return_logits=True)[1]
    emb = _embedder(name, dt, monkeypatch).embed(_audio(name)).embeddings
    assert torch.equal(_bits(emb), _bits(logits))


# ---- 3. fused against the twin, eager and replayed; 4. distances against fp64 ---------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fused_is_the_twin_and_distances_hold(name, dt, monkeypatch):
    gal = _oracle(name)[3]
    runs = []
    for fused in (True, False):
        e = _embedder(name, dt, monkeypatch, fused, n_gallery=70)
        runs += [e.embed(_audio(name)) for _ in range(3)]      # eager, capture + replay, replay
        assert e._graphs
    for r in runs[1:]:
        assert _same(r, runs[0])
    r = runs[0]
    emb = r.embeddings.cpu().numpy().astype(np.float64)
    want = np.sqrt(1e-8 + ((emb[:, :, None, :] - gal[None, None, :70].astype(np.float64)) ** 2).sum(-1))
    got = r.distances.cpu().numpy()
    assert got.shape == want.shape == (CASES[name][3], N_EMIT[name], 70)
    err = float((np.abs(got - want) / want).max())
    _say("distances against fp64, case %s %s: %.3g" % (name, dt, err))
    assert err <= TOL_DIST
    # 5. (on the way) nearest and dmin are the argmin and min of the kernel's own row
    assert np.array_equal(r.nearest.cpu().numpy(), got.argmin(-1))
    assert np.array_equal(r.distance.cpu().numpy(), got.min(-1))


# ---- 5. nearest ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("N", [0, 1, 70, MAX_GALLERY])
def test_nearest_is_the_first_minimum_of_the_row(N, fused, monkeypatch):
    """Through the step, on a pre-poisoned ``dist`` buffer.  Rows 3 and 5 (N > 5) are one of the stream's own embeddings:
    two identical rows tie at the smallest distance there is, and the lower index wins."""
    e = _embedder("a", F32, monkeypatch, fused)
    own = e.embed(_audio("a")).embeddings[1, 4].clone()
    gal = torch.tensor(_oracle("a")[3][:N])
    if N > 5:
        gal[3] = gal[5] = own.cpu()
    e.enroll(gal)
    e.dist.fill_(float("nan"))
    r = e.embed(_audio("a"))
    assert tuple(r.distances.shape) == (3, N_EMIT["a"], N)
    assert bool(torch.isnan(e.dist[:, N:]).all())                 # columns >= N stay as they were
    if N == 0:
        assert bool((r.nearest == -1).all()) and bool(torch.isinf(r.distance).all())
        return
    d = r.distances.cpu().numpy()
    assert np.isfinite(d).all()
    assert np.array_equal(r.nearest.cpu().numpy(), d.argmin(-1))      # (NumPy's argmin: the first of equal minima)
    assert np.array_equal(r.distance.cpu().numpy(), d.min(-1))
    if N > 5:
        assert int(r.nearest[1, 4]) == 3 and d[1, 4, 3] == d[1, 4, 5] and abs(d[1, 4, 3] - 1e-4) <= TOL_DIST * 1e-4      # sqrt(1e-8 + 0)


@pytest.mark.parametrize("D", [2, 40, 256])
def test_gallery_match_alone(D):
    """srwn_gallery_match on stored embeddings: the bits of a distance do not depend on N or on the row, ties go to the
    lowest index whichever wave holds it, and columns >= N are left alone."""
    L_ = sub("_lib"); K = sub("kernels")
    rng = np.random.default_rng(D)
    rows, mg = 5, MAX_GALLERY
    emb = torch.tensor(rng.standard_normal((rows, D)), dtype=torch.float32, device=DEV)
    gal = torch.tensor(rng.standard_normal((mg, D)), dtype=torch.float32, device=DEV)
    gal[[2, 7, 9, 64]] = emb[0]      # (waves 2, 3, 1 and 0: the lowest index is not in the lowest wave)
    emb[4] = emb[1]
    outs = {}
    for N in (0, 1, 3, 70, mg):
        count = torch.tensor([N], dtype=torch.int32, device=DEV)
        dist = torch.full((rows, mg), float("nan"), device=DEV)
        near = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
        dmin = torch.full((rows,), float("nan"), device=DEV)
        L_.call("srwn_gallery_match", emb.data_ptr(), rows, D, gal.data_ptr(), count.data_ptr(), mg, dist.data_ptr(),
                near.data_ptr(), dmin.data_ptr(), K._stream())
        torch.cuda.synchronize()
        d = dist.cpu().numpy()
        assert np.isnan(d[:, N:]).all() and np.isfinite(d[:, :N]).all()
        if N == 0:
            assert near.tolist() == [-1] * rows and bool(torch.isinf(dmin).all())
            continue
        assert np.array_equal(near.cpu().numpy(), d[:, :N].argmin(-1)) and np.array_equal(dmin.cpu().numpy(), d[:, :N].min(-1))
        assert int(near[0]) == (2 if N >= 3 else 0)
        outs[N] = d
    for N in (1, 3, 70):
        assert np.array_equal(outs[N][:, :N], outs[mg][:, :N])      # ... not on N
    assert np.array_equal(outs[mg][4], outs[mg][1])                   # ... not on the row
    want = np.sqrt(1e-8 + ((emb.double().cpu().numpy()[:, None] - gal.double().cpu().numpy()[None]) ** 2).sum(-1))
    assert float((np.abs(outs[mg] - want) / want).max()) <= TOL_DIST


# ---- 6. the gallery may change under a captured graph --------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_gallery_changes_under_a_captured_graph(dt, fused, monkeypatch):
    gal, audio = _oracle("a")[3], _audio("a")
    third = []
    for graphs in (True, False):
        e = _embedder("a", dt, monkeypatch, fused, n_gallery=3, graphs=graphs)
        first, second = e.embed(audio), e.embed(audio)
        assert _same(first, second) and bool(e._graphs) == graphs
        captured = dict(e._graphs)
        assert e.enroll(gal[3:5], labels=["x", "y"]) == [3, 4] and e.labels == [0, 1, 2, "x", "y"]
        third.append(e.embed(audio))
        assert e._graphs == captured                              # nothing was captured anew
        assert tuple(third[-1].distances.shape) == (3, N_EMIT["a"], 5)
        assert torch.equal(_bits(third[-1].distances[..., :3]), _bits(first.distances))
    assert _same(third[0], third[1])
    e.clear()
    assert tuple(e.embed(audio).distances.shape) == (3, N_EMIT["a"], 0) and e.labels == []


# ---- 7. cutting, batch size, batch row -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("name", ["a", "c"])
def test_cutting_and_batch_rows_change_no_bit(name, dt, monkeypatch):
    hop = CASES[name][4]
    e = _embedder(name, dt, monkeypatch, n_gallery=70)
    audio = _audio(name)
    whole = e.embed(audio)
    st = e.start(audio.shape[0])
    rng = np.random.default_rng(3)
    parts, at = [], 0
    while at < T:
        n = min(int(rng.integers(0, 2 * hop + 8)), T - at)      # pieces of 0 .. 2 * hop + 7 samples
        parts.append(e.push(st, audio[:, at:at + n]))
        at += n
        assert st.t == at and st.pending == at % hop
    assert st.emitted == N_EMIT[name] and any(p.nearest.shape[1] == 0 for p in parts)
    assert _same([torch.cat(f, 1) for f in zip(*parts)], whole)
    alone = e.embed(audio[2:3])                                   # another batch size, another row
    assert _same([f[0] for f in alone], [f[2] for f in whole])


# ---- 8. the model's face ---------------------------------------------------------------------------------------------------
def test_single_window_is_get_embedding(tmp_path):
    """hop = window = input_size: the one embedding is SiameseWaveNet.get_embedding's (another summation order, so within
    twice the fp32 bound that each holds against the oracle, not bit for bit); from_checkpoint after save reproduces
    embedder()'s bits; enroll embeds with the object's own path."""
    M = sub("model")
    R, S, D, B = 32, 128, 40, 3
    Tm = 200
    sp = O.init_stack_params(11, DIL, 2, R, S, D, bias_scale=0.05)
    audio = O.synthetic_audio(B, Tm, seed=9)
    m = M.SiameseWaveNet(Tm, D, DIL, dilation_channels=R, skip_channels=S, dtype=F32)
    m._engine(B, Tm).load_oracle_params(sp)
    want = m.get_embedding(None, audio)
    emb = m.embedder(max_batch=B, max_gallery=8)
    assert (emb.hop, emb.window, emb.max_gallery, emb.output_dimensions) == (Tm, Tm, 8, D)
    r = emb.embed(audio)
    assert r.embeddings.shape == want.shape == (B, 1, D) and r.distances.shape == (B, 1, 0)
    oracle = O.stack_forward(sp, audio.astype(np.float64))[0].mean(1)[:, None]
    assert rel_err(want, oracle) < 1e-3 and rel_err(r.embeddings, oracle) < 1e-3
    assert rel_err(r.embeddings, want) < 2e-3
    # enroll the clips themselves: each is its own nearest template, at the distance of two equal vectors
    assert emb.enroll(audio, labels=["u", "v", "w"]) == [0, 1, 2] and emb.labels == ["u", "v", "w"]
    assert np.array_equal(emb.gallery, r.embeddings[:, 0])
    s = emb.stream(B)
    none = s.push(audio[:, :150])
    assert none.embeddings.shape == (B, 0, D) and (s.t, s.emitted) == (150, 0)
    got, ok = s.push(audio[:, 150:], threshold=1e-3)
    assert (s.t, s.emitted) == (Tm, 1) and np.array_equal(got.embeddings, r.embeddings)
    assert got.nearest[:, 0].tolist() == [0, 1, 2] and np.all(np.abs(got.distance - 1e-4) <= TOL_DIST * 1e-4) and ok.all()
    assert got.distances.shape == (B, 1, 3) and not s.push(np.zeros((B, 0), np.float32), threshold=0.0)[1].size
    with pytest.raises(ValueError, match="max_gallery"):
        emb.enroll_embeddings(np.zeros((6, D), np.float32))
    assert emb.enroll_embeddings(np.zeros((1, D), np.float32)) == [3]
    emb.clear()
    assert emb.gallery.shape == (0, D)
    with pytest.raises(ValueError, match="samples"):      # get_embedding keeps its length refusal
        m.get_embedding(None, audio[:, :150])
    # the checkpoint names SiameseWaveNet.save writes
    assert m.save(None, str(tmp_path), 3, force=True)
    long = O.synthetic_audio(B, 500, seed=2)
    a = m.embedder(max_batch=B, hop=40, window=80, max_hops=MAX_HOPS).embed(long)
    b = M.StreamingEmbedder.from_checkpoint(str(tmp_path), DIL, D, R, S, dtype=F32, max_batch=B, hop=40, window=80,
                                            max_hops=MAX_HOPS).embed(long)
    assert a.embeddings.shape == (B, 11, D) and np.array_equal(a.embeddings, b.embeddings)
