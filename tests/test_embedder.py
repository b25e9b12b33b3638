"""CPU tests of the streaming embedder (srwn_version() 120): the entry points declared, bound, generated and exported; their
argument errors without a GPU; every refusal of the host layers before any device work; and the launch list of a step, alone
and in a pool, with the fused head and with its twin (``_lib.call`` recorded, as tests/test_stream_stack.py does)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._pkg import ROOT, sub
from tests.test_recognizer import A, E_NULL, E_SHAPE, _bare, _lib
from tests.test_stream_stack import BM, NAMES, Weights, _names

NEW = ["srwn_window_embed_match", "srwn_window_embed_match_slots", "srwn_gallery_match"]


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
    assert L.SIGNATURES[NEW[0]] == L.SIGNATURES[NEW[1]]      # the table in the clock's place, capacity in B's
    block = raw[raw.index("streaming embedder (since srwn_version() 120"):]
    assert "model.py:660-797" in block and "model.py:736" in block
    B = sub("build")
    assert "srwn_embed.hip" in B.SOURCES
    assert B.NO_SPILL["srwn_embed.hip"] == ["window_embed_match_kernel", "gallery_match_kernel"]


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_version_and_exports(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 120
    for n in NEW:
        assert callable(getattr(lib, n))


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)

    def fused(name="srwn_window_embed_match", ring=A, rr=5, clock=A, B=2, k=2, hop=32, window=128, S=128, w2=A, b2=A, D=40,
              ldw=64, gallery=A, count=A, mg=96, emb=A, dist=A, nearest=A, dmin=A):
        return getattr(lib, name)(ring, rr, clock, B, k, hop, window, S, w2, b2, D, ldw, gallery, count, mg, emb, dist, nearest,
                                  dmin, None)

    for name in NEW[:2]:
        for arg in ("ring", "clock", "w2", "b2", "gallery", "count", "emb", "dist", "nearest", "dmin"):
            assert fused(name, **{arg: None}) == E_NULL, (name, arg)
        assert name[5:].encode() in lib.srwn_last_error()
        for bad in (dict(S=512), dict(S=0), dict(D=0), dict(D=257, ldw=288), dict(ldw=39), dict(mg=0), dict(mg=1025), dict(k=0),
                    dict(B=0), dict(hop=0), dict(window=100), dict(window=16), dict(rr=4)):
            assert fused(name, **bad) == E_SHAPE, (name, bad)
        assert name[5:].encode() in lib.srwn_last_error()

    def match(emb=A, rows=3, D=40, gallery=A, count=A, mg=96, dist=A, nearest=A, dmin=A):
        return lib.srwn_gallery_match(emb, rows, D, gallery, count, mg, dist, nearest, dmin, None)

    assert match(rows=0, emb=None) == 0      # empty work is done before anything is looked at
    for arg in ("emb", "gallery", "count", "dist", "nearest", "dmin"):
        assert match(**{arg: None}) == E_NULL, arg
    for bad in (dict(D=0), dict(D=257), dict(mg=0), dict(mg=1025), dict(rows=-1)):
        assert match(**bad) == E_SHAPE, bad
    assert b"gallery_match" in lib.srwn_last_error()


# ---- refusals, before any device work ----------------------------------------------------------------------------------
def test_weights_refuse_first():
    E = sub("embedder")
    for r, s in ((48, 256), (128, 256), (32, 192)):
        with pytest.raises(NotImplementedError, match="streaming embedder.*built for"):
            E.EmbedderWeights([1, 2], r, s, 12)
    with pytest.raises(NotImplementedError, match="output_channels"):
        E.EmbedderWeights([1, 2], 32, 128, 300)
    cfg = dict(head_mode="contrastive", gate_mode="reference", shift_input=False, cond_channels=0, dilations=[1, 2],
               dilation_channels=32, skip_channels=256, output_channels=12, filter_width=2, dtype=torch.float32)
    eng = lambda **kw: SimpleNamespace(cfg=SimpleNamespace(**dict(cfg, **kw)), dev="cpu")
    for mode in ("pooled", "per_timestep"):
        with pytest.raises(ValueError, match="contrastive"):
            E.EmbedderWeights.from_engine(eng(head_mode=mode))
    with pytest.raises(NotImplementedError, match="wavenet"):
        E.EmbedderWeights.from_engine(eng(gate_mode="wavenet"))
    with pytest.raises(ValueError, match="RightShift"):
        E.EmbedderWeights.from_engine(eng(shift_input=True))
    with pytest.raises(ValueError, match="conditioning"):
        E.EmbedderWeights.from_engine(eng(cond_channels=16))
    with pytest.raises(NotImplementedError, match="built for"):
        E.EmbedderWeights.from_engine(eng(dilation_channels=48))


def test_embedder_refuses_first():
    E = sub("embedder"); R = sub("recognizer")
    with pytest.raises(ValueError, match="multiple of hop"):
        E.StreamEmbedder(None, hop=48, window=100)
    with pytest.raises(ValueError, match="max_hops"):
        E.StreamEmbedder(None, hop=16, window=32, max_hops=0)
    for mg in (0, 1025):
        with pytest.raises(ValueError, match="max_gallery"):
            E.StreamEmbedder(None, hop=16, window=32, max_gallery=mg)
    e = _bare(E.StreamEmbedder, max_batch=2, _state=None, _serial=0, D=4, max_gallery=3, _n=2, _labels=["a", "b"], dev="cpu")
    with pytest.raises(ValueError, match="max_batch"):
        e.embed(np.zeros((3, 10), np.float32))
    with pytest.raises(ValueError, match=r"\[batch, samples\]"):
        e.embed(np.zeros(10, np.float32))
    with pytest.raises(TypeError, match="embed"):
        e.classify(np.zeros((1, 10), np.float32))
    st = R.RecogState(2, 1, None)
    e._state, e._serial = st, 1
    with pytest.raises(ValueError, match="streams"):
        e.push(st, np.zeros((1, 10), np.float32))
    with pytest.raises(ValueError, match="current"):
        e.push(R.RecogState(2, 0, None), np.zeros((2, 10), np.float32))
    assert (st.t, st.emitted) == (0, 0)
    # the gallery: a wrong width, labels of another length and one template too many leave it as it was
    for bad, labels, what in ((np.zeros((1, 5)), None, r"\[n, 4\]"), (np.zeros((1, 2, 4)), None, r"\[n, 4\]"),
                              (np.zeros((1, 4)), ["x", "y"], "labels"), (np.zeros((2, 4)), None, "max_gallery is 3")):
        with pytest.raises(ValueError, match=what):
            e.enroll(bad, labels)
        assert (e._n, e.labels) == (2, ["a", "b"])
    assert e.enroll(np.zeros((0, 4))) == [] and e._n == 2      # nothing to append: no device work


def test_models_refuse_first():
    M = sub("model")
    ok = dict(input_size=128, filter_width=2, dilation_channels=32, skip_channels=128, _primary=None)
    with pytest.raises(ValueError, match="multiple of hop"):
        _bare(M.SiameseWaveNet, **ok).embedder(hop=48)
    with pytest.raises(ValueError, match="multiple of hop"):
        _bare(M.SiameseWaveNet, **ok).embedder(window=100, hop=40)
    with pytest.raises(ValueError, match="hop"):
        _bare(M.SiameseWaveNet, **ok).embedder(hop=0)
    with pytest.raises(ValueError, match="max_gallery"):
        _bare(M.SiameseWaveNet, **ok).embedder(max_gallery=2000)
    with pytest.raises(NotImplementedError, match="filter_width"):
        _bare(M.SiameseWaveNet, **dict(ok, filter_width=3)).embedder()
    with pytest.raises(NotImplementedError, match="streaming embedder.*built for"):
        _bare(M.SiameseWaveNet, **dict(ok, dilation_channels=48, skip_channels=256)).embedder()
    with pytest.raises(NotImplementedError, match="built for"):
        M.StreamingEmbedder.from_checkpoint("/nonexistent", [1, 2], 12, dilation_channels=48)
    with pytest.raises(ValueError, match="multiple of hop"):
        M.StreamingEmbedder.from_checkpoint("/nonexistent", [1, 2], 12, hop=7, window=16)
    face = _bare(M.StreamingEmbedder, window=32, max_gallery=2, max_batch=1,
                 _eng=SimpleNamespace(labels=["a"]))
    with pytest.raises(ValueError, match=r"window = 32"):
        face.enroll(np.zeros((1, 31), np.float32))
    with pytest.raises(ValueError, match="labels"):
        face.enroll(np.zeros((1, 32), np.float32), ["x", "y"])
    with pytest.raises(ValueError, match="max_gallery is 2"):
        face.enroll(np.zeros((2, 32), np.float32))


# ---- the launch list -----------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """tests/test_stream_stack.py's recorder, with the embedder's own ``call`` recorded too."""
    rec = []
    for m in ("_lib", "kernels", "stream_stack", "recognizer", "embedder"):
        if hasattr(sub(m), "call"):
            monkeypatch.setattr(sub(m), "call", lambda name, *args: rec.append((name, args)))
    monkeypatch.setattr(sub("kernels"), "_need_gpu", lambda: None)
    monkeypatch.setattr(sub("kernels"), "_chk", lambda t, name, dtype=None, shape=None: t.data_ptr())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: SimpleNamespace(cuda_stream=0))
    monkeypatch.delenv("SRWN_GROUP_LAYERS", raising=False)
    return rec


@pytest.mark.parametrize("head", [True, False], ids=["head", "head-twin"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twin"])
@pytest.mark.parametrize("pooled", [False, True], ids=["alone", "pool"])
def test_embedder_step(calls, monkeypatch, fused, pooled, head):
    monkeypatch.setenv("SRWN_EMBED_FUSED", "1" if fused else "0")
    monkeypatch.setenv("SRWN_RECOG_FUSED", "1" if head else "0")
    e = sub("embedder").StreamEmbedder(Weights(classes=12), max_batch=BM, hop=8, window=32, max_hops=4, max_gallery=9)
    assert (e.embed_fused, e.fused, e.D, e.max_gallery) == (fused, head, 12, 9)
    pool = SimpleNamespace(table=torch.zeros((BM, 2), dtype=torch.int64), ring=torch.zeros((BM, 65)), audio_ring=65) if pooled else None
    e._launch_step(BM, 2, pool)
    sfx, G = "_slots" if pooled else "", len(e.groups)
    sums = ["srwn_pooled_stream_head" + sfx] if head else ["srwn_pw_linear"] * 2 + ["srwn_hop_sum" + sfx]
    tail = ["srwn_window_embed_match" + sfx] if fused else ["srwn_window_mean" + sfx, "srwn_gallery_match"]
    assert _names(calls) == ["srwn_recog_stream_in" + sfx] + [NAMES[True, pooled]] * G + sums + tail + ["srwn_recog_roll" + sfx]
    assert len(calls) == e.launches_per_step
    if fused and head:
        assert e.launches_per_step == 4 + G
    when = pool.table.data_ptr() if pooled else e.clock.data_ptr()
    w2, b2 = e.w.view("head_w2").data_ptr(), e.w.view("head_b2").data_ptr()
    gal = (e.gallery_buf.data_ptr(), e.count.data_ptr(), 9)
    out = (e.dist.data_ptr(), e.nearest.data_ptr(), e.dmin.data_ptr(), 0)
    args = dict(calls)
    if fused:
        assert args[tail[0]] == (e.ring.data_ptr(), e.ring_rows, when, BM, 2, 8, 32, e.w.S, w2, b2, 12, 32) + gal + (
            e.emb.data_ptr(),) + out
        assert e.mean is None
    else:      # the twin: the window means' pooled logits ARE the embeddings
        assert args[tail[0]] == (e.ring.data_ptr(), e.ring_rows, e.mean.data_ptr(), when, BM, 2, 8, 32, e.w.S, w2, b2,
                                 e.emb.data_ptr(), 12, 32, 0)
        assert args["srwn_gallery_match"] == (e.emb.data_ptr(), BM * 2, 12) + gal + out
    assert tuple(e.dist.shape) == (BM * 4, 9) and tuple(e.emb.shape) == (BM * 4, 12)
    assert set(e.buffer_bytes()) == {"boundary", "z", "ring", "audio", "emissions", "gallery", "images"} | (
        set() if head else {"twin r0/r1"})
    assert e.buffer_bytes()["gallery"] == 9 * 12 * 4 + 4


def test_classifier_step_is_what_it_was(calls, monkeypatch):
    """The classifier's tail went into an overridable method: it issues the launches it issued, on the buffers it had."""
    monkeypatch.setenv("SRWN_RECOG_FUSED", "1")
    c = sub("recognizer").StreamClassifier(Weights(classes=12), max_batch=BM, hop=8, window=32, max_hops=4)
    c._launch_step(BM, 2)
    w2, b2 = c.w.view("head_w2").data_ptr(), c.w.view("head_b2").data_ptr()
    args = dict(calls)
    assert [n for n, _ in calls][-3:] == ["srwn_window_mean", "srwn_pooled_head", "srwn_recog_roll"]
    assert args["srwn_window_mean"] == (c.ring.data_ptr(), c.ring_rows, c.mean.data_ptr(), c.clock.data_ptr(), BM, 2, 8, 32,
                                        c.w.S, w2, b2, c.logits.data_ptr(), 12, 32, 0)
    assert args["srwn_pooled_head"] == (c.mean.data_ptr(), w2, b2, None, c.probs.data_ptr(), None, None, None, None, BM * 2,
                                        c.w.S, 12, 32, 0)
    assert c.launches_per_step == 4 + len(c.groups) + 1


def test_gallery_on_the_host(calls):
    """enroll / clear / labels / gallery on host tensors: indices, labels and the device count follow each other."""
    e = sub("embedder").StreamEmbedder(Weights(classes=4), max_batch=1, hop=8, window=32, max_hops=2, max_gallery=5)
    assert e.enroll(np.arange(8, dtype=np.float32).reshape(2, 4)) == [0, 1]
    assert e.enroll(torch.full((4,), 7.0), labels=["seven"]) == [2]
    assert e.labels == [0, 1, "seven"] and int(e.count) == 3
    assert e.gallery.tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [7, 7, 7, 7]]
    with pytest.raises(ValueError, match="max_gallery is 5"):
        e.enroll(np.zeros((3, 4), np.float32))
    assert int(e.count) == 3 and e.labels == [0, 1, "seven"]
    e.clear()
    assert int(e.count) == 0 and e.labels == [] and tuple(e.gallery.shape) == (0, 4)
    assert e.enroll(np.ones((5, 4), np.float32)) == [0, 1, 2, 3, 4] and int(e.count) == 5
