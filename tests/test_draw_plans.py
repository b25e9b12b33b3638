"""CPU tests of device-resident training for the student and the twins (srwn_version() 123): the order functions
``dataset.noise_plan`` and ``dataset.pair_plan`` -- the specifications the draw kernels of csrc/srwn_draw.hip implement --,
every refusal of the samplers and of ``fit`` before any device work, and the five C entries declared, bound, generated and
exported, with their argument errors without a GPU."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests._pkg import ROOT, sub

NEW = ["srwn_distill_draw", "srwn_cond_scatter", "srwn_distill_log", "srwn_pair_draw", "srwn_pair_log"]
E_DTYPE, E_SHAPE, E_NULL = -1, -2, -3
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take
SEED = 3
LABELS9 = [0, 1, 0, 2, 1, 0, 3, 1, 0]      # classes of 4, 3, 1 and 1 records
CLIP, T = 70, 61


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


# ---- noise_plan ---------------------------------------------------------------------------------------------------------
def test_noise_plan_values_and_streams():
    D = sub("dataset")
    k = D.noise_plan(SEED, 0, 3, 500)
    assert k.dtype == np.uint32 and k.shape == (3, 500)
    assert k.max() < 1 << 23
    assert k.max() > 1 << 22 and k.min() < 1 << 20       # 1500 draws on [0, 2^23) reach into both ends
    rows = [tuple(r) for r in k.tolist()]
    rows += [tuple(r) for r in D.noise_plan(SEED, 1, 3, 500).tolist()]               # another step
    rows += [tuple(r) for r in D.noise_plan(SEED, 1, 3, 500, rank=1, world=2).tolist()]   # another rank (positions 9..11)
    rows += [tuple(r) for r in D.noise_plan(SEED + 1, 0, 3, 500).tolist()]           # another seed
    assert len(set(rows)) == len(rows) == 12
    # a row is a prefix of the longer row of the same position
    assert np.array_equal(D.noise_plan(SEED, 0, 3, 64), k[:, :64])


def test_noise_plan_ranks_interleave_as_positions_do():
    D = sub("dataset")
    for s in range(4):
        r0 = D.noise_plan(SEED, s, 3, 40, rank=0, world=2)
        r1 = D.noise_plan(SEED, s, 3, 40, rank=1, world=2)
        assert np.array_equal(np.concatenate([r0, r1]), D.noise_plan(SEED, s, 6, 40))
    with pytest.raises(ValueError, match="rank 2 of 2"):
        D.noise_plan(SEED, 0, 3, 40, rank=2, world=2)


def test_noise_plan_by_hand():
    """One entry's chain written out: step 2 of rank 1 of 2, B = 2, row b = 1, entry j = 4."""
    D = sub("dataset")
    M = (1 << 64) - 1

    def mix(x):
        x &= M
        x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M
        x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    golden, salt = 0x9E3779B97F4A7C15, 0x6E6F697365726F77
    assert D.NOISE_SALT == salt and D.NOISE_SALT != D._CROP_SALT
    p = (2 * 2 + 1) * 2 + 1
    sb = mix((SEED ^ salt) + golden * (p + 1))
    want = mix(sb + golden * (4 + 1)) >> 41
    assert want == 2966519                     # (the constants, pinned)
    assert int(D.noise_plan(SEED, 2, 2, 5, rank=1, world=2)[1, 4]) == want
    assert int(D.noise_rows(SEED, 2, 2, rank=1, world=2)[1]) == sb


# ---- pair_plan ----------------------------------------------------------------------------------------------------------
def _pairs(D, steps, P=3, labels=LABELS9, classes=4, **kw):
    """(left, right, off_left, off_right, y) of every pair of the first `steps` steps."""
    return [np.concatenate(c) for c in zip(*[D.pair_plan(SEED, s, P, labels, classes, CLIP, T, **kw) for s in range(steps)])]


def test_pair_plan_on_nine_records():
    D = sub("dataset")
    lab = np.array(LABELS9)
    left, right, ol, orr, y = _pairs(D, 400, crop="random")
    assert left.dtype == np.int32 and right.dtype == np.int32 and ol.dtype == np.int64 and orr.dtype == np.int64
    assert y.dtype == np.float32
    # the left side is draw_plan's
    for s in (0, 7):
        idx, off = D.draw_plan(SEED, s, 3, 9, CLIP, T, True, "random")
        got = D.pair_plan(SEED, s, 3, LABELS9, 4, CLIP, T, crop="random")
        assert got[0].tolist() == idx.tolist() and got[2].tolist() == off.tolist()
    assert np.array_equal(y, (lab[left] == lab[right]).astype(np.float32))
    m = np.bincount(lab)[lab[left]]
    assert (right != left)[m >= 2].all()
    assert (y[m == 1] == 0).all()                         # a singleton is forced to "different"
    assert ((orr >= 0) & (orr <= CLIP - T)).all() and len(set(orr.tolist())) == CLIP - T + 1
    assert (ol != orr).any()
    # all three branches occur in 1200 pairs, and every eligible right record of every left record
    assert (y[m >= 2] == 1).any() and (y[m >= 2] == 0).any() and (m == 1).any()
    seen = {(int(a), int(b)) for a, b in zip(left, right)}
    assert seen == {(a, b) for a in range(9) for b in range(9) if a != b}


def test_pair_plan_head_crop_and_ranks():
    D = sub("dataset")
    got = D.pair_plan(SEED, 5, 3, LABELS9, 4, CLIP, T)
    assert got[2].tolist() == [0, 0, 0] and got[3].tolist() == [0, 0, 0]
    for s in range(4):
        r0 = D.pair_plan(SEED, s, 3, LABELS9, 4, CLIP, T, crop="random", rank=0, world=2)
        r1 = D.pair_plan(SEED, s, 3, LABELS9, 4, CLIP, T, crop="random", rank=1, world=2)
        one = D.pair_plan(SEED, s, 6, LABELS9, 4, CLIP, T, crop="random")
        for a, b, c in zip(r0, r1, one):
            assert np.concatenate([a, b]).tolist() == c.tolist()


def test_pair_plan_at_the_ends_of_p_same():
    D = sub("dataset")
    lab = np.array(LABELS9)
    m = np.bincount(lab)
    left, right, _, _, y = _pairs(D, 100, p_same=0.0)
    assert (y == 0).all()
    left, right, _, _, y = _pairs(D, 100, p_same=1.0)
    assert np.array_equal(y, (m[lab[left]] >= 2).astype(np.float32))     # all "same" but the singletons
    # one class only: "same" whatever the coin says; one record only: itself, y = 1
    left, right, _, _, y = _pairs(D, 20, labels=[2, 2, 2], classes=3, p_same=0.0)
    assert (y == 1).all() and (left != right).all()
    left, right, _, _, y = _pairs(D, 5, labels=[1], classes=2, p_same=0.0)
    assert (y == 1).all() and (left == 0).all() and (right == 0).all()
    with pytest.raises(ValueError, match="p_same"):
        D.pair_plan(SEED, 0, 3, LABELS9, 4, CLIP, T, p_same=1.5)


@pytest.mark.parametrize("p_same", [0.5, 0.2])
def test_pair_plan_fraction_of_same(p_same):
    """Without singletons nothing is forced: over n = 3000 positions the fraction of "same" lies within four standard
    deviations of p_same.  (The plan is deterministic: this holds for SEED, as checked here.)"""
    D = sub("dataset")
    labels = [0, 1, 0, 2, 1, 0, 2, 1, 0]
    n = 3000
    y = _pairs(D, n // 3, labels=labels, classes=3, p_same=p_same)[4]
    assert y.size == n
    assert abs(float(y.mean()) - p_same) <= 4.0 * math.sqrt(p_same * (1.0 - p_same) / n), float(y.mean())


def test_class_index():
    D = sub("dataset")
    order, place, start = D.class_index(LABELS9, 4)
    assert order.tolist() == [0, 2, 5, 8, 1, 4, 7, 3, 6] and start.tolist() == [0, 4, 7, 8, 9]
    assert place[order].tolist() == list(range(9))
    assert D.class_index([1, 1], 3)[2].tolist() == [0, 0, 2, 2]          # an empty class
    assert D.same_threshold(0.0) == 0 and D.same_threshold(1.0) == 1 << 32 and D.same_threshold(0.5) == 1 << 31


# ---- the scalars tests/test_gpu_draw.py holds srwn_distill_log to --------------------------------------------------------
LOG_COEF = (0.3, 1.7, 1536)               # alpha, beta, N
# (ce, power, logs) as float32 bit patterns, loss_div 1: beta * ce - alpha * entropy + power lands on the midpoint of two
# float32 values when both products are rounded first, and one double ulp beside it when either product stays exact
LOG_TIES = [(0x457918CD, 0x2B800000, 0xC522431F), (0x44BD7B7E, 0x2B000000, 0xC545CB92),
            (0x451DB3CA, 0x2B000000, 0xC5123821), (0x43949978, 0x364CCCCD, 0xC53151AC)]


def distill_log_cases():
    """(ce, power, logs, loss_div): the ties at loss_div 1, then triples of the size a student step produces at 3."""
    rng = np.random.default_rng(5)
    out = [tuple(np.array(c, np.uint32).view(np.float32)) + (1.0,) for c in LOG_TIES]
    out += [(np.float32(1234.5678), np.float32(0.25), np.float32(-2000.125), 3.0)]
    out += [(np.float32(c), np.float32(p), np.float32(l), 3.0)
            for c, p, l in zip(rng.uniform(1, 5000, 12), rng.uniform(0, 3, 12), rng.uniform(-4000, -1000, 12))]
    return out


def distill_log_host(ce, power, logs, div):
    """``StudentEngine.losses()``: Python float arithmetic, then float32."""
    alpha, beta, N = LOG_COEF
    ce, power, logs = float(ce), float(power), float(logs)
    entropy = logs + 2.0 * N
    return np.float32((beta * ce - alpha * entropy + power) / div), np.float32(power), np.float32(entropy)


def test_distill_log_cases_tell_a_fused_multiply_add_apart():
    """The log kernel must round beta * ce and alpha * entropy before it subtracts them.  For every tie case, keeping one
    of the products exact inside the subtraction (what a contracted multiply-add computes) changes the float32 loss."""
    from fractions import Fraction
    alpha, beta, N = LOG_COEF
    for ce, power, logs, div in distill_log_cases()[:len(LOG_TIES)]:
        ce, power, logs = float(ce), float(power), float(logs)
        entropy = logs + 2.0 * N
        fused = (float(Fraction(beta) * Fraction(ce) - Fraction(alpha * entropy)),      # fma(beta, ce, -(alpha entropy))
                 float(Fraction(beta * ce) - Fraction(alpha) * Fraction(entropy)))      # fma(-alpha, entropy, beta ce)
        assert any(np.float32((f + power) / div) != distill_log_host(ce, power, logs, div)[0] for f in fused)


# ---- refusals before any device work ------------------------------------------------------------------------------------
def test_labels_outside_the_classes_are_refused():
    D = sub("dataset")
    for bad in ([0, 1, 4], [0, -1, 2]):
        with pytest.raises(ValueError, match=r"inside \[0, 4\)"):
            D.pair_plan(SEED, 0, 2, bad, 4, CLIP, T)
        with pytest.raises(ValueError, match=r"inside \[0, 4\)"):
            D.class_index(bad, 4)


def _bare_dataset(D, n=7, clip_len=70, labels=None, num_classes=0):
    return _bare(D.DeviceDataset, audio=SimpleNamespace(shape=(n, clip_len)), labels=labels, num_classes=num_classes,
                 device="cuda")


def test_sampler_refusals_without_a_device():
    D = sub("dataset")
    d = _bare_dataset(D)
    with pytest.raises(ValueError, match="holds no labels"):
        d.pair_sampler(3, 64)
    with pytest.raises(ValueError, match="num_samples 71 > clip length 70"):
        d.distill_sampler(3, 71)
    with pytest.raises(ValueError, match="temperature"):
        d.distill_sampler(3, 64, temperature=-1.0)
    with pytest.raises(ValueError, match="log_capacity"):
        d.distill_sampler(3, 64, log_capacity=0)
    labelled = _bare_dataset(D, labels=object(), num_classes=4)
    with pytest.raises(ValueError, match="p_same"):
        labelled.pair_sampler(3, 64, p_same=2.0)
    with pytest.raises(ValueError, match="rank 2 of 2"):
        labelled.pair_sampler(3, 64, rank=2, world=2)


def test_fit_keeps_its_refusals_for_other_samplers():
    D, M = sub("dataset"), sub("model")
    ds = _bare_dataset(D)
    plain = _bare(D.BatchSampler, dataset=ds, batch_size=3, num_samples=64)
    pairs = _bare(D.PairSampler, dataset=ds, batch_size=3, pairs=3, num_samples=64)
    distill = _bare(D.DistillSampler, dataset=ds, batch_size=3, num_samples=64)
    for s in (plain, pairs):
        with pytest.raises(NotImplementedError, match="noise and teacher passes beside the clips; feed it with train"):
            _bare(M.ParallelWaveNet).fit(s, 1)
    for s in (plain, distill):
        with pytest.raises(NotImplementedError, match="pairs of clips and their labels; feed it with train"):
            _bare(M.SiameseWaveNet).fit(s, 1)
    # a decoder-only teacher has no encoder to run inside the step
    with pytest.raises(NotImplementedError, match="decoder-only teacher has no encoder"):
        _bare(M.ParallelWaveNet, _teacher=_bare(M.WaveNetTeacher)).fit(distill, 1)
    # the conditions are the labels' one-hot rows; the twins' clip length is the model's
    with pytest.raises(ValueError, match="holds no labels"):
        _bare(M.ParallelWaveNet, _teacher=None, condition_size=4).fit(distill, 1)
    with pytest.raises(ValueError, match="input_size=32"):
        _bare(M.SiameseWaveNet, input_size=32).fit(pairs, 1)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    lib = _lib("ctypes")
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES and 'm.def("%s"' % n in src, n
        assert hasattr(lib, n), n
    assert lib.srwn_version() >= 123
    assert "srwn_draw.hip" in sub("build").SOURCES
    assert "since srwn_version() 123" in open(os.path.join(ROOT, "include", "srwn.h")).read()


def _distill(lib, clips=A, labels=A, n=7, clip_len=70, state=A, B=2, T=64, shuffle=1, crop=0, rank=0, world=1, a0=A, a1=None,
             a2=None, noise=A, temp=1.0, tables=None, nt=0, ld=16, rows=1, col0=8, classes=4, dt=0, indices=A):
    return lib.srwn_distill_draw(clips, labels, n, clip_len, state, B, T, shuffle, crop, rank, world, a0, a1, a2, noise, temp,
                                 tables, nt, ld, rows, col0, classes, dt, indices, None)


def _pair(lib, clips=A, labels=A, order=A, place=A, start=A, classes=4, n=9, clip_len=70, state=A, P=3, T=64, thr=1 << 31,
          shuffle=1, crop=0, rank=0, world=1, audio=A, y=A, left=A, right=A, ylog=A):
    return lib.srwn_pair_draw(clips, labels, order, place, start, classes, n, clip_len, state, P, T, thr, shuffle, crop, rank,
                              world, audio, y, left, right, ylog, None)


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    assert _distill(lib, B=0) == 0 and _distill(lib, T=0) == 0 and _pair(lib, P=0) == 0
    for kw in (dict(clips=None), dict(state=None), dict(a0=None), dict(indices=None), dict(nt=2, tables=None),
               dict(nt=2, tables=A, labels=None)):
        assert _distill(lib, **kw) == E_NULL, kw
    for kw in (dict(T=71), dict(n=0), dict(B=65536, clip_len=70), dict(rank=1), dict(crop=2), dict(nt=65, tables=A),
               dict(nt=-1), dict(nt=1, tables=A, ld=11), dict(nt=1, tables=A, rows=0), dict(a1=A + 2), dict(noise=A + 1)):
        assert _distill(lib, **kw) == E_SHAPE, kw
    assert _distill(lib, nt=1, tables=A, dt=7) == E_DTYPE
    assert b"distill_draw" in lib.srwn_last_error()
    for kw in (dict(labels=None), dict(order=None), dict(place=None), dict(start=None), dict(audio=None), dict(y=None),
               dict(left=None), dict(right=None), dict(ylog=None), dict(clips=None), dict(state=None)):
        assert _pair(lib, **kw) == E_NULL, kw
    for kw in (dict(T=71), dict(n=0), dict(P=32768), dict(rank=2, world=2), dict(crop=-1), dict(thr=-1),
               dict(thr=(1 << 32) + 1), dict(classes=0), dict(audio=A + 2)):
        assert _pair(lib, **kw) == E_SHAPE, kw
    assert lib.srwn_cond_scatter(A, 0, 8, A, 3, 16, 0, None) == 0
    assert lib.srwn_cond_scatter(None, 4, 8, A, 3, 16, 0, None) == E_NULL
    assert lib.srwn_cond_scatter(A, 4, 8, None, 3, 16, 0, None) == E_NULL
    assert lib.srwn_cond_scatter(A, 4, 17, A, 3, 16, 0, None) == E_SHAPE
    assert lib.srwn_cond_scatter(A, 4, 8, A, 65, 16, 0, None) == E_SHAPE
    assert lib.srwn_cond_scatter(A, 4, 8, A, 3, 16, 5, None) == E_DTYPE
    assert lib.srwn_distill_log(A, A, None, 1.0, 1.0, 1536, 2.0, A, A, A, 4, A, None) == E_NULL
    assert lib.srwn_distill_log(A, A, A, 1.0, 1.0, 1536, 2.0, A, A, A, 0, A, None) == E_SHAPE
    assert lib.srwn_distill_log(A, A, A, 1.0, 1.0, 1536, 0.0, A, A, A, 4, A, None) == E_SHAPE
    assert lib.srwn_distill_log(A, A, A, 1.0, 1.0, -1, 2.0, A, A, A, 4, A, None) == E_SHAPE
    assert lib.srwn_pair_log(A, None, 3, A, A, 4, A, None) == E_NULL
    assert lib.srwn_pair_log(A, A, 0, A, A, 4, A, None) == E_SHAPE
    assert lib.srwn_pair_log(A, A, 3, A, A, 0, A, None) == E_SHAPE
