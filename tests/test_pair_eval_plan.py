"""CPU tests of device-resident evaluation of an embedding model (srwn_version() 125): the NumPy restatement of
``srwn_pair_sweep``'s rules on hand cases, the host metrics of ``PairEvalResult`` on hand-made histograms, every refusal of
the sampler, of ``SiameseWaveNet.evaluate`` / ``fit(..., validate=...)`` and of ``ParallelWaveNet.evaluate`` before any
device work, and the two C entries declared, bound, generated and exported, with their argument errors without a GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests._pkg import ROOT, sub
from tests.pair_eval_reference import distance_matrix_fp64, pair_reference

E_SHAPE, E_NULL = -2, -3
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _lib(binding):
    L = sub("_lib")
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "sr-wavenet_amd", "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.build()
    return L.bind(binding)


def _bare(cls, **attrs):
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _matrix(points):
    """A stored fp32 matrix of hand points: any fp32 matrix serves, the rules are functions of the stored numbers."""
    p = np.asarray(points, np.float64).reshape(len(points), -1)
    return np.sqrt(1e-8 + ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)).astype(np.float32)


# ---- the kernel's rules, restated ---------------------------------------------------------------------------------------
def test_reference_on_points_on_a_line():
    #             0    1    2    3    4
    x = [0.0, 1.0, 3.0, 4.0, 10.0]
    lab = [0, 1, 0, 1, 0]
    d = _matrix(x)
    near, nd, same, sd, rank, hs, hd = pair_reference(d, lab, 4, np.float32(4 / 8.0))
    # record 1 lies at distance 1 of record 0 and at 2 of record 2: 0 first; record 2 at 1 of record 3
    assert near.tolist() == [1, 0, 3, 2, 3]
    assert same.tolist() == [2, 3, 0, 1, 2]
    assert nd.tolist() == [d[0, 1], d[1, 0], d[2, 3], d[3, 2], d[4, 3]] and sd.tolist() == [d[0, 2], d[1, 3], d[2, 0], d[3, 1], d[4, 2]]
    # record 0: record 1 (other label, 1) comes before record 2 (3); record 2: 3 (1) and 1 (2) before 0 (3);
    # record 3: 2 (1) before 1 (3); record 4: 3 (6) before 2 (7); record 1: 0 (1) and 2 (2) before 3 (3)
    assert rank.tolist() == [1, 2, 2, 1, 1]
    # pairs i < j: distances 1, 3, 4, 10 | 2, 3, 9 | 1, 7 | 6 and scale 1/2: bins 0, 1, 2, 3(5 -> last) | 1, 1, 3 | 0, 3 | 3
    same_pairs = {(0, 2): 1, (0, 4): 3, (2, 4): 3, (1, 3): 1}
    want_s, want_d = np.zeros(4, np.int64), np.zeros(4, np.int64)
    for i in range(5):
        for j in range(i + 1, 5):
            b = min(3, int(np.float32(d[i, j]) * np.float32(0.5)))
            (want_s if lab[i] == lab[j] else want_d)[b] += 1
            if lab[i] == lab[j]:
                assert same_pairs[i, j] == b
    assert np.array_equal(hs, want_s) and np.array_equal(hd, want_d)
    assert hs.sum() + hd.sum() == 10 and hs.tolist() == [0, 2, 0, 2]


def test_reference_on_duplicated_points():
    """Exact duplicates and equal distances: the lower index decides everywhere."""
    pts = [[0, 0], [0, 0], [1, 0], [0, 1], [0, 0], [-1, 0]]
    lab = [0, 1, 1, 0, 0, 1]
    d = _matrix(pts)
    near, nd, same, sd, rank, hs, hd = pair_reference(d, lab, 8, np.float32(8 / 4.0))
    assert d[0, 1] == d[0, 4] == d[1, 4] == np.float32(1e-4)
    assert near.tolist() == [1, 0, 0, 0, 0, 0]                    # ties at 1e-4 and at 1: the lowest index that is not i
    assert same.tolist() == [4, 2, 1, 0, 0, 1]                    # record 1: records 2 and 5 tie at 1, 2 comes first
    assert sd[0] == np.float32(1e-4) and sd[1] == d[1, 2]
    # record 0: record 1 (another label) ties with record 4 at a lower index: 1 in front.  record 1: 0 and 4 (1e-4), and
    # of the four records at distance 1 only record 3 has another label, at an index above 2: 2.  record 2: at distance 1
    # from 0, 1, 4; 0 comes before 1, 4 after: 1.  record 3: 0 is the first of all: 0.  record 4: 0 first: 0.
    # record 5: at distance 1 from 0, 1, 4; 0 before 1: 1
    assert rank.tolist() == [1, 2, 1, 0, 0, 1]
    assert hs.sum() + hd.sum() == 15


def test_reference_with_a_single_member_class_and_one_record():
    d = _matrix([0.0, 2.0, 5.0])
    near, nd, same, sd, rank, hs, hd = pair_reference(d, [0, 7, 0], 2, np.float32(2 / 4.0))
    assert near.tolist() == [1, 0, 1] and same.tolist() == [2, -1, 0] and rank.tolist() == [1, -1, 1]
    assert sd[1] == np.inf and np.isfinite(sd[[0, 2]]).all()
    assert hs.tolist() == [0, 1] and hd.tolist() == [0, 2]        # 5 * 0.5 = 2.5 is not below 2: the last bin; 2 * 0.5 = 1
    near, nd, same, sd, rank, hs, hd = pair_reference(_matrix([3.0]), [4], 3, np.float32(1.0))
    assert near.tolist() == [-1] and same.tolist() == [-1] and rank.tolist() == [-1]
    assert nd.tolist() == [np.inf] and sd.tolist() == [np.inf] and hs.sum() == 0 and hd.sum() == 0


def test_reference_bins_take_everything():
    d = np.array([[1e-4, np.nan, np.inf, 0.4999], [np.nan, 1e-4, 7.0, 0.5], [np.inf, 7.0, 1e-4, 3.9999],
                  [0.4999, 0.5, 3.9999, 1e-4]], np.float32)
    _, _, _, _, _, hs, hd = pair_reference(d, [0, 0, 0, 0], 8, np.float32(2.0))
    # NaN, inf and 14 go to the last bin; 0.9998 -> 0, 1.0 -> 1, 7.9998 -> 7
    assert hs.tolist() == [1, 1, 0, 0, 0, 0, 0, 4] and hd.sum() == 0


def test_fp64_distance_bound_is_a_few_ulps():
    e = np.random.default_rng(0).standard_normal((5, 130)).astype(np.float32)
    d, bound = distance_matrix_fp64(e)
    assert d.shape == (5, 5) and np.allclose(np.diag(d), 1e-4, rtol=1e-6)
    assert (bound > 0).all() and (bound[d > 1] <= 9.5 * 2.0 ** -24 * d[d > 1] + 1e-37).all()


# ---- the host metrics ---------------------------------------------------------------------------------------------------
def _result(hs, hd, rank=(0,), d_max=4.0):
    D = sub("dataset")
    n = len(rank)
    z = np.zeros(n, np.int32)
    return D.PairEvalResult(np.zeros((n, 2), np.float32), z, z.astype(np.float32), z, z.astype(np.float32),
                            np.asarray(rank, np.int32), hs, hd, n, z, len(hs), d_max)


def test_metrics_of_perfectly_separated_sets():
    r = _result([3, 2, 0, 0], [0, 0, 4, 1])
    assert r.eer == 0.0 and r.auc == 1.0 and r.eer_threshold == 2.0 and r.edge(-1) == 0.0 and r.edge(3) == 4.0
    assert r.far_frr(0.0) == (0.0, 1.0) and r.far_frr(4.0) == (1.0, 0.0)
    assert r.far_frr(1.0) == (0.0, 0.4) and r.far_frr(3.0) == (0.8, 0.0)
    with pytest.raises(ValueError, match="bin edges"):
        r.far_frr(1.5)
    with pytest.raises(ValueError, match="bin edges"):
        r.far_frr(5.0)
    far, frr = r.rates()
    assert far.dtype == np.float64 and far.tolist() == [0, 0, 0, 0.8, 1] and frr.tolist() == [1, 0.4, 0, 0, 0]


def test_metrics_of_identical_histograms():
    r = _result([1, 2, 3, 2], [1, 2, 3, 2])
    assert r.eer == 0.5 and abs(r.auc - 0.5) < 1e-15
    # |FAR - FRR| = |2 F - 1| over F = 0, 1/8, 3/8, 6/8, 1: least at F = 3/8, edge 1
    assert r.eer_threshold == 2.0


def test_metrics_of_overlapping_sets():
    r = _result([6, 2, 0, 0], [1, 1, 6, 0], d_max=2.0)
    far, frr = r.rates()
    assert far.tolist() == [0, 0.125, 0.25, 1, 1] and frr.tolist() == [1, 0.25, 0, 0, 0]
    assert r.eer == (0.125 + 0.25) / 2 and r.eer_threshold == 0.5          # |FAR - FRR| = 1, 1/8, 1/4, 1, 1
    tpr = [0, 0.75, 1, 1, 1]
    want = sum((far[k + 1] - far[k]) * (tpr[k + 1] + tpr[k]) / 2 for k in range(4))
    assert r.auc == want


def test_metrics_without_pairs_of_one_label():
    r = _result([0, 0, 0], [2, 1, 0], rank=(-1, -1, -1))
    assert np.isnan(r.eer) and np.isnan(r.auc) and np.isnan(r.eer_threshold)
    far, frr = r.far_frr(4.0 / 3.0)
    assert far == 2.0 / 3.0 and np.isnan(frr)
    assert r.nn_accuracy == 0.0 and r.recall_at(5) == 0.0
    assert "PairEvalResult" in repr(r)


def test_recall_counts_records_without_a_partner_as_misses():
    r = _result([1], [1], rank=(0, 2, -1, 1, 0, 5, -1, 0))
    assert r.nn_accuracy == 3 / 8 and r.recall_at(1) == 3 / 8 and r.recall_at(2) == 4 / 8 and r.recall_at(3) == 5 / 8
    assert r.recall_at(100) == 6 / 8


# ---- refusals before any device work ------------------------------------------------------------------------------------
def _bare_dataset(D, n=7, clip_len=80, labels=None, num_classes=0, host=None):
    d = _bare(D.DeviceDataset, audio=SimpleNamespace(shape=(n, clip_len)), labels=labels, num_classes=num_classes,
              device="cuda")
    if host is not None:
        d._labels_host = np.asarray(host, np.int32)
    return d


def test_embed_sampler_refusals_without_a_device():
    D = sub("dataset")
    with pytest.raises(ValueError, match="holds no labels"):
        _bare_dataset(D).embed_sampler(4, 64)
    ok = dict(labels=object(), num_classes=4, host=[0, 1, 2, 3, 0, 1, 2])
    with pytest.raises(ValueError, match="needs every rank's embeddings"):
        _bare_dataset(D, **ok).embed_sampler(4, 64, rank=1, world=2)
    for bins in (0, -1, 4097):
        with pytest.raises(ValueError, match="bins %d: at least 1, at most 4096" % bins):
            _bare_dataset(D, **ok).embed_sampler(4, 64, bins=bins)
    for d_max in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="d_max .*finite and above 0"):
            _bare_dataset(D, **ok).embed_sampler(4, 64, d_max=d_max)
    with pytest.raises(ValueError, match="sweep_capacity"):
        _bare_dataset(D, **ok).embed_sampler(4, 64, sweep_capacity=0)
    assert D.MAX_EMBED_RECORDS >= 4096
    with pytest.raises(ValueError, match="%d records: at most %d" % (D.MAX_EMBED_RECORDS + 1, D.MAX_EMBED_RECORDS)):
        _bare_dataset(D, n=D.MAX_EMBED_RECORDS + 1, labels=object(), num_classes=4,
                      host=[0] * (D.MAX_EMBED_RECORDS + 1)).embed_sampler(4, 64)
    for bad in ([0, 1, 2, 3, 4, 0, 1], [0, 1, -1, 3, 2, 0, 1]):
        with pytest.raises(ValueError, match=r"inside \[0, 4\)"):
            _bare_dataset(D, labels=object(), num_classes=4, host=bad).embed_sampler(4, 64)
    with pytest.raises(ValueError, match="num_samples 81 > clip length 80"):
        _bare_dataset(D, **ok).embed_sampler(4, 81)
    with pytest.raises(ValueError, match="rank 1 of 1"):
        _bare_dataset(D, **ok).embed_sampler(4, 64, rank=1)
    with pytest.raises(ValueError, match="batch_size 0"):
        _bare_dataset(D, **ok).embed_sampler(0, 64)


def test_bound_sampler_refusals_without_a_device():
    D = sub("dataset")
    es = _bare(D.EmbedSampler, dim=2, d_max=None, emb=object(), bins=8)
    with pytest.raises(ValueError, match="bound to 2 embedding dimensions, the model has 5"):
        es.bind(5, 10.0)
    with pytest.raises(ValueError, match="d_max is not set yet"):
        es.scale
    es.bind(2, 10.0)
    assert es.d_max == 10.0 and es.scale == np.float32(0.8) and es.scale.dtype == np.float32
    es.bind(2, 3.0)                                                # a d_max that is set stays
    assert es.d_max == 10.0
    for dim in (0, D.MAX_EMBED_DIM + 1):
        with pytest.raises(ValueError, match="embedding dimensions"):
            _bare(D.EmbedSampler, dim=None, d_max=1.0).bind(dim, 1.0)
    with pytest.raises(ValueError, match="finite and above 0"):
        _bare(D.EmbedSampler, dim=None, d_max=None).bind(2, 0.0)
    with pytest.raises(TypeError, match="logs no loss"):
        es.log_step(None)
    with pytest.raises(ValueError, match="not bound"):
        _bare(D.EmbedSampler, dim=None, emb=None, dataset=_bare_dataset(D), batch_size=2).collect(None)


def test_evaluate_and_validate_refusals_without_a_device():
    D, M = sub("dataset"), sub("model")
    ds = _bare_dataset(D, labels=object(), num_classes=4)
    plain = _bare(D.BatchSampler, dataset=ds, batch_size=3, num_samples=64, shuffle=False, world=1)
    pairs = _bare(D.PairSampler, dataset=ds, batch_size=3, pairs=3, num_samples=64)
    ev = _bare(D.EvalSampler, dataset=ds, batch_size=4, num_samples=64)
    es = _bare(D.EmbedSampler, dataset=ds, batch_size=4, num_samples=64, dim=3, d_max=1.0)
    net = _bare(M.SiameseWaveNet, input_size=64, output_dimensions=2, margin=5.0)
    for wrong in (plain, ev, pairs):
        with pytest.raises(TypeError, match="EmbedSampler"):
            net.evaluate(wrong)
        with pytest.raises(TypeError, match="EmbedSampler"):
            net.fit(pairs, 1, validate=(wrong, 2))
    for every in (0, -3):
        with pytest.raises(ValueError, match="every %d: at least 1" % every):
            net.fit(pairs, 1, validate=(es, every))
    with pytest.raises(ValueError, match=r"\(eval_sampler, every\)"):
        net.fit(pairs, 1, validate=es)
    with pytest.raises(NotImplementedError, match="pairs of clips"):
        net.fit(es, 1)
    with pytest.raises(ValueError, match="input_size=32"):
        _bare(M.SiameseWaveNet, input_size=32, output_dimensions=3, margin=5.0).evaluate(es)
    with pytest.raises(ValueError, match="bound to 3 embedding dimensions, the model has 2"):
        net.evaluate(es)
    with pytest.raises(ValueError, match="bound to 3 embedding dimensions, the model has 2"):
        net.fit(pairs, 1, validate=(es, 1))
    # the student's loss sweep: whole batches only, a DistillSampler in order
    student = _bare(M.ParallelWaveNet, condition_size=0)
    dist = lambda **kw: _bare(D.DistillSampler, dataset=ds, num_samples=64, **kw)
    with pytest.raises(ValueError, match="ParallelWaveNet.evaluate: 7 clips are no multiple of batch_size \\* world = 3"):
        student.evaluate(dist(batch_size=3, shuffle=False, world=1))
    with pytest.raises(ValueError, match="no multiple of batch_size \\* world = 14"):
        student.evaluate(dist(batch_size=7, shuffle=False, world=2))
    with pytest.raises(ValueError, match="ParallelWaveNet.evaluate: the sampler shuffles"):
        student.evaluate(dist(batch_size=7, shuffle=True, world=1))
    for wrong in (plain, ev, es):
        with pytest.raises(TypeError, match="ParallelWaveNet.evaluate takes a dataset.DistillSampler"):
            student.evaluate(wrong)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    raw = open(os.path.join(ROOT, "include", "srwn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    lib = _lib("ctypes")
    for n in ("srwn_embed_collect", "srwn_pair_sweep"):
        assert re.search(r"\b%s\s*\(" % n, hdr)
        assert n in L.SIGNATURES and 'm.def("%s"' % n in src
        assert hasattr(lib, n)
    assert lib.srwn_version() >= 125
    B = sub("build")
    assert "srwn_pair_eval.hip" in B.SOURCES
    assert set(B.NO_SPILL["srwn_pair_eval.hip"]) >= {"embed_collect_kernel", "pair_sweep_kernel"}
    assert "since srwn_version() 125" in raw


def _collect(lib, emb=A, indices=A, state=A, n=11, B=4, D=2, rank=0, world=1, cap=2, slots=A, seen=A):
    return lib.srwn_embed_collect(emb, indices, state, n, B, D, rank, world, cap, slots, seen, None)


def _sweep(lib, slots=A, labels=A, state=A, n=11, D=2, cap=2, bins=8, scale=1.0, near=A, same=A, rank=A, nd=A, sd=A, hs=A,
           hd=A, dist=None):
    return lib.srwn_pair_sweep(slots, labels, state, n, D, cap, bins, scale, near, same, rank, nd, sd, hs, hd, dist, None)


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    for name in ("emb", "indices", "state", "slots", "seen"):
        assert _collect(lib, **{name: None}) == E_NULL, name
    assert b"embed_collect: null pointer" in lib.srwn_last_error()
    for kw in (dict(D=0), dict(D=1025), dict(B=0), dict(n=0), dict(n=4097), dict(rank=1), dict(rank=-1),
               dict(rank=2, world=2), dict(world=0), dict(cap=0)):
        assert _collect(lib, **kw) == E_SHAPE, kw
    assert b"embed_collect" in lib.srwn_last_error()
    for name in ("slots", "labels", "state", "near", "same", "rank", "nd", "sd", "hs", "hd"):
        assert _sweep(lib, **{name: None}) == E_NULL, name
    assert b"pair_sweep: null pointer" in lib.srwn_last_error()
    for kw in (dict(D=0), dict(D=1025), dict(n=0), dict(n=4097), dict(cap=0), dict(bins=0), dict(bins=4097),
               dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan"))):
        assert _sweep(lib, **kw) == E_SHAPE, kw
    assert b"pair_sweep" in lib.srwn_last_error()
