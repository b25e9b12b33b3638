"""CPU tests of device-resident evaluation (srwn_version() 124): the order function ``dataset.sweep_plan`` -- the
specification of a sweep --, the NumPy restatement of ``srwn_eval_classes``'s rules on hand cases, every refusal of the
sampler, of ``evaluate`` and of ``fit(..., validate=...)`` before any device work, and the C entry declared, bound,
generated and exported, with its argument errors without a GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests._pkg import ROOT, sub
from tests.eval_reference import eval_reference, ulp_distance

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


# ---- sweep_plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3])
def test_a_sweep_visits_every_record_once(world):
    D = sub("dataset")
    n, B = 11, 4
    steps = D.sweep_steps(n, B, world)
    assert steps == -(-n // (B * world))
    seen, positions = [], []
    for rank in range(world):
        for s in range(steps):
            idx, valid = D.sweep_plan(s, B, n, rank, world)
            assert idx.dtype == np.int32 and idx.shape == (B,) and valid.dtype == bool and valid.shape == (B,)
            p = (s * world + rank) * B + np.arange(B)
            assert np.array_equal(valid, p < n)                       # the invalid rows are exactly the positions >= n
            want, _ = D.draw_plan(7, s, B, n, 80, 64, False, "head", rank, world)
            assert np.array_equal(idx, want)                          # every row: the draw's record without shuffling
            assert (idx >= 0).all() and (idx < n).all()               # (the ragged tail reads inside the set)
            seen += idx[valid].tolist()
            positions += p.tolist()
    assert sorted(seen) == list(range(n))
    assert sorted(positions) == list(range(steps * world * B))        # the ranks' steps tile the positions


def test_sweep_plan_edge_cases():
    D = sub("dataset")
    idx, valid = D.sweep_plan(0, 4, 1)                                # one record, B > n
    assert idx.tolist() == [0, 0, 0, 0] and valid.tolist() == [True, False, False, False]
    assert D.sweep_steps(1, 4) == 1 and D.sweep_steps(1, 1) == 1
    idx, valid = D.sweep_plan(0, 16, 11)                              # B > n: one ragged step, records wrap
    assert D.sweep_steps(11, 16) == 1 and valid.sum() == 11 and idx.tolist() == [p % 11 for p in range(16)]
    assert D.sweep_steps(12, 4) == 3                                  # n % B == 0: no ragged step
    for s in range(3):
        idx, valid = D.sweep_plan(s, 4, 12)
        assert valid.all() and idx.tolist() == list(range(4 * s, 4 * s + 4))
    assert D.sweep_steps(12, 4, world=3) == 1 and D.sweep_steps(13, 4, world=3) == 2
    idx, valid = D.sweep_plan(1, 4, 13, rank=2, world=3)              # a whole step past the end
    assert not valid.any() and (idx < 13).all()
    for bad in (dict(step=0, batch_size=0, n=5), dict(step=0, batch_size=4, n=0), dict(step=-1, batch_size=4, n=5),
                dict(step=0, batch_size=4, n=5, rank=2, world=2)):
        with pytest.raises(ValueError):
            D.sweep_plan(**bad)
    with pytest.raises(ValueError):
        D.sweep_steps(0, 4)


# ---- the kernel's rules, restated ---------------------------------------------------------------------------------------
def test_reference_on_hand_cases():
    probs = np.array([[0.25, 0.5, 0.5, 0.0],        # two maxima: the lower index wins
                      [0.25, 0.25, 0.25, 0.25],     # the label tied with every class
                      [0.0, 1.0, 0.0, 0.0],         # a probability of 0 at the label
                      [0.0, 1.0, 0.0, 0.0],         # ... and of 1
                      [0.125, 0.5, 0.125, 0.25]], np.float32)
    labels = np.array([2, 2, 3, 1, 0])
    pred, rank, nll, conf = eval_reference(probs, labels)
    assert pred.tolist() == [1, 0, 1, 1, 1]
    # row 0: class 1 ties with the label at a lower index; row 1: the equal-valued lower indices 0 and 1 only; row 2:
    # class 1 is greater, classes 0 and 2 tie at lower indices; row 4: classes 1 and 3 are greater, class 2 ties above
    assert rank.tolist() == [1, 2, 3, 0, 2]
    assert ((rank == 0) == (pred == labels)).all()
    assert nll[2] == np.inf and nll[3] == 0.0
    assert nll[0] == np.float32(np.log(2.0)) and nll[4] == np.float32(np.log(8.0))
    want = np.zeros((4, 4), np.int32)
    for l, p in zip(labels, pred):
        want[l, p] += 1
    assert np.array_equal(conf, want) and conf.sum() == 5
    pred1, rank1, nll1, conf1 = eval_reference(np.ones((2, 1), np.float32), [0, 0])      # one class
    assert pred1.tolist() == [0, 0] and rank1.tolist() == [0, 0] and conf1.tolist() == [[2]]
    assert ulp_distance(np.float32([1.0, -0.0, np.inf]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0,
                                                                       np.inf])).tolist() == [1, 0, 0]


# ---- refusals before any device work ------------------------------------------------------------------------------------
def _bare_dataset(D, n=7, clip_len=80, labels=None, num_classes=0, host=None):
    d = _bare(D.DeviceDataset, audio=SimpleNamespace(shape=(n, clip_len)), labels=labels, num_classes=num_classes,
              device="cuda")
    if host is not None:
        d._labels_host = np.asarray(host, np.int32)
    return d


def test_eval_sampler_refusals_without_a_device():
    D = sub("dataset")
    with pytest.raises(ValueError, match="holds no labels"):
        _bare_dataset(D).eval_sampler(4, 64)
    for bad in ([0, 1, 2, 3, 4, 0, 1], [0, 1, -1, 3, 2, 0, 1]):
        with pytest.raises(ValueError, match=r"inside \[0, 4\)"):
            _bare_dataset(D, labels=object(), num_classes=4, host=bad).eval_sampler(4, 64)
    with pytest.raises(ValueError, match="num_classes 257: at most 256"):
        _bare_dataset(D, labels=object(), num_classes=257, host=[0] * 7).eval_sampler(4, 64)
    ok = dict(labels=object(), num_classes=4, host=[0, 1, 2, 3, 0, 1, 2])
    with pytest.raises(ValueError, match="sweep_capacity"):
        _bare_dataset(D, **ok).eval_sampler(4, 64, sweep_capacity=0)
    with pytest.raises(ValueError, match="top_k"):
        _bare_dataset(D, **ok).eval_sampler(4, 64, top_k=0)
    with pytest.raises(ValueError, match="num_samples 81 > clip length 80"):
        _bare_dataset(D, **ok).eval_sampler(4, 81)
    with pytest.raises(ValueError, match="rank 2 of 2"):
        _bare_dataset(D, **ok).eval_sampler(4, 64, rank=2, world=2)


def test_evaluate_and_validate_refusals_without_a_device():
    D, M = sub("dataset"), sub("model")
    ds = _bare_dataset(D, labels=object(), num_classes=4)
    plain = _bare(D.BatchSampler, dataset=ds, batch_size=3, num_samples=64, shuffle=False, world=1)
    ev = _bare(D.EvalSampler, dataset=ds, batch_size=4, num_samples=64)
    net = _bare(M.WaveNet, input_size=64, output_size=4)
    with pytest.raises(TypeError, match="EvalSampler"):
        net.fit(plain, 1, validate=(plain, 2))
    for every in (0, -3):
        with pytest.raises(ValueError, match="every %d: at least 1" % every):
            net.fit(plain, 1, validate=(ev, every))
    with pytest.raises(ValueError, match=r"\(eval_sampler, every\)"):
        net.fit(plain, 1, validate=ev)
    with pytest.raises(TypeError, match="EvalSampler"):
        net.evaluate(plain)
    with pytest.raises(TypeError, match="sweeps a held-out set"):
        net.fit(ev, 1)
    with pytest.raises(ValueError, match="input_size=32"):
        _bare(M.WaveNet, input_size=32, output_size=4).evaluate(ev)
    with pytest.raises(ValueError, match="num_classes=4"):
        _bare(M.WaveNet, input_size=64, output_size=5).evaluate(ev)
    # the loss sweeps of the teacher and the auto-encoder: whole batches only, a plain sampler in order
    for model in (_bare(M.WaveNetTeacher, use_encoding=False), _bare(M.WaveNetAutoEncoder, condition_size=0)):
        with pytest.raises(ValueError, match="7 clips are no multiple of batch_size \\* world = 3"):
            model.evaluate(plain)
        with pytest.raises(ValueError, match="no multiple of batch_size \\* world = 14"):
            model.evaluate(_bare(D.BatchSampler, dataset=ds, batch_size=7, num_samples=64, shuffle=False, world=2))
        with pytest.raises(ValueError, match="shuffles"):
            model.evaluate(_bare(D.BatchSampler, dataset=ds, batch_size=7, num_samples=64, shuffle=True, world=1))
        with pytest.raises(TypeError, match="plain dataset.BatchSampler"):
            model.evaluate(ev)
    with pytest.raises(NotImplementedError, match="use_encoding=True"):
        _bare(M.WaveNetTeacher, use_encoding=True).evaluate(
            _bare(D.BatchSampler, dataset=ds, batch_size=7, num_samples=64, shuffle=False, world=1))


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    lib = _lib("ctypes")
    n = "srwn_eval_classes"
    assert re.search(r"\b%s\s*\(" % n, hdr)
    assert n in L.SIGNATURES and 'm.def("%s"' % n in src
    assert hasattr(lib, n)
    assert lib.srwn_version() >= 124
    assert "srwn_eval.hip" in sub("build").SOURCES
    assert "since srwn_version() 124" in open(os.path.join(ROOT, "include", "srwn.h")).read()


def _eval(lib, probs=A, indices=A, labels=A, state=A, n=11, B=4, C=5, rank=0, world=1, cap=2, pred=A, rk=A, nll=A, conf=A,
          seen=A):
    return lib.srwn_eval_classes(probs, indices, labels, state, n, B, C, rank, world, cap, pred, rk, nll, conf, seen, None)


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    for name in ("probs", "indices", "labels", "state", "pred", "rk", "nll", "conf", "seen"):
        assert _eval(lib, **{name: None}) == E_NULL, name
    assert b"eval_classes: null pointer" in lib.srwn_last_error()
    for kw in (dict(C=0), dict(C=257), dict(C=-1), dict(B=0), dict(B=-2), dict(n=0), dict(rank=1), dict(rank=-1),
               dict(rank=2, world=2), dict(world=0), dict(cap=0), dict(cap=-1)):
        assert _eval(lib, **kw) == E_SHAPE, kw
    assert b"eval_classes" in lib.srwn_last_error()
