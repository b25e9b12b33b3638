"""CPU tests of the device-resident datasets (srwn_version() 122): the order function ``dataset.draw_plan`` -- the
specification the draw kernel implements -- as a bijection per epoch, across epoch boundaries, per rank and per crop; every
refusal of the Python classes before any device work; the two C entries declared, bound, generated and exported, and their
argument errors without a GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests._pkg import ROOT, sub

NEW = ["srwn_batch_draw", "srwn_step_log"]
E_DTYPE, E_SHAPE, E_NULL = -1, -2, -3
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take
SEED = 3          # test_epochs_are_reshuffled checks that this seed shows what it is there to show


def _lib(binding):
    L = sub("_lib")
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "sr-wavenet_amd", "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.build()
    return L.bind(binding)


def _bare(cls, **attrs):
    """An object without its device state (constructing one needs a GPU): what the checks read first."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _epochs(D, n, B, count, seed=SEED, **kw):
    """The first `count` epochs of the sample sequence, cut out of whole batches."""
    steps = -(-count * n // B)
    seq = np.concatenate([D.draw_plan(seed, s, B, n, 70, 64, **kw)[0] for s in range(steps)])
    return seq[:count * n].reshape(count, n)


# ---- the order function -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 1000])
def test_every_epoch_is_a_permutation(n):
    D = sub("dataset")
    for ep in _epochs(D, n, 5, 3):
        assert sorted(ep.tolist()) == list(range(n))
    for e in (0, 1, 12345678901):         # the bijection itself, far epochs included
        assert sorted(D.permute(SEED, e, i, n) for i in range(n)) == list(range(n))


def test_a_batch_crosses_the_epoch_boundary():
    D = sub("dataset")
    n, B = 7, 3
    ep = _epochs(D, n, B, 3)
    idx2 = D.draw_plan(SEED, 2, B, n, 70, 64)[0]          # positions 6, 7, 8: the last of epoch 0, the first two of epoch 1
    assert idx2.tolist() == [ep[0, 6], ep[1, 0], ep[1, 1]]
    assert idx2.dtype == np.int32


def test_epochs_are_reshuffled():
    D = sub("dataset")
    ep = _epochs(D, 7, 3, 4)
    assert len({tuple(e) for e in ep.tolist()}) > 1, "the first four epochs of seed %d share one order" % SEED
    assert any(tuple(e) != tuple(range(7)) for e in ep.tolist())
    other = _epochs(D, 7, 3, 4, seed=SEED + 1)
    assert other.tolist() != ep.tolist()                  # the seed keys the order


def test_without_shuffle_the_order_is_sequential():
    D = sub("dataset")
    ep = _epochs(D, 7, 3, 3, shuffle=False)
    assert ep.tolist() == [list(range(7))] * 3


def test_ranks_are_disjoint_and_interleave_to_one_rank():
    D = sub("dataset")
    n, B = 7, 3
    for s in range(5):
        r0 = D.draw_plan(SEED, s, B, n, 70, 61, crop="random", rank=0, world=2)
        r1 = D.draw_plan(SEED, s, B, n, 70, 61, crop="random", rank=1, world=2)
        one = D.draw_plan(SEED, s, 2 * B, n, 70, 61, crop="random")
        assert np.concatenate([r0[0], r1[0]]).tolist() == one[0].tolist()
        assert np.concatenate([r0[1], r1[1]]).tolist() == one[1].tolist()
    # positions of the two ranks never coincide: over whole epochs each record is drawn once by exactly one of them
    n, B = 64, 4
    seqs = [np.concatenate([D.draw_plan(SEED, s, B, n, 70, 64, rank=r, world=2)[0] for s in range(n // (2 * B))])
            for r in (0, 1)]
    assert not set(seqs[0].tolist()) & set(seqs[1].tolist())
    assert sorted(seqs[0].tolist() + seqs[1].tolist()) == list(range(n))


def test_offsets():
    D = sub("dataset")
    offs = []
    for s in range(40):
        assert D.draw_plan(SEED, s, 3, 7, 70, 61, crop="head")[1].tolist() == [0, 0, 0]
        assert D.draw_plan(SEED, s, 3, 7, 70, 70, crop="random")[1].tolist() == [0, 0, 0]      # the whole clip: no room
        o = D.draw_plan(SEED, s, 3, 7, 70, 61, crop="random")[1]
        assert o.dtype == np.int64 and o.min() >= 0 and o.max() <= 9
        offs += o.tolist()
    assert set(offs) == set(range(10))                    # 120 draws on [0, 9]: both ends are reached


# ---- refusals before any device work -------------------------------------------------------------------------------------
def _bare_dataset(D, n=7, clip_len=70, labels=None, num_classes=0):
    return _bare(D.DeviceDataset, audio=SimpleNamespace(shape=(n, clip_len)), labels=labels, num_classes=num_classes,
                 device="cuda")


def test_sampler_refusals_without_a_device():
    D = sub("dataset")
    d = _bare_dataset(D)
    assert len(d) == 7 and d.clip_len == 70
    with pytest.raises(ValueError, match="num_samples 71 > clip length 70"):
        d.sampler(3, 71)
    with pytest.raises(ValueError, match="batch_size 0"):
        d.sampler(0, 64)
    with pytest.raises(ValueError, match="crop"):
        d.sampler(3, 64, crop="tail")
    with pytest.raises(ValueError, match="rank 2 of 2"):
        d.sampler(3, 64, rank=2, world=2)
    with pytest.raises(ValueError, match="log_capacity"):
        d.sampler(3, 64, log_capacity=0)


def test_dataset_refusals_without_a_device():
    D = sub("dataset")
    x = np.zeros((7, 70), np.float32)
    with pytest.raises(ValueError, match=r"audio must be \[clips, samples\]"):
        D.DeviceDataset(np.zeros(70, np.float32))
    with pytest.raises(ValueError, match=r"labels must be \[7\]"):
        D.DeviceDataset(x, labels=np.zeros(6, np.int64), num_classes=4)
    with pytest.raises(ValueError, match=r"labels must be \[7\]"):
        D.DeviceDataset(x, labels=np.zeros((7, 4), np.int64), num_classes=4)
    with pytest.raises(TypeError, match="integers"):
        D.DeviceDataset(x, labels=np.zeros(7, np.float32), num_classes=4)
    with pytest.raises(ValueError, match="labels need num_classes"):
        D.DeviceDataset(x, labels=np.zeros(7, np.int64))
    with pytest.raises(ValueError, match="num_classes without labels"):
        D.DeviceDataset(x, num_classes=4)


def test_fit_refusals_without_a_device():
    D, M = sub("dataset"), sub("model")
    s = _bare(D.BatchSampler, dataset=_bare_dataset(D), batch_size=3, num_samples=64)
    with pytest.raises(NotImplementedError, match="encoding comes from another model"):
        _bare(M.WaveNetTeacher, use_encoding=True).fit(s, 1)
    with pytest.raises(NotImplementedError, match="noise and teacher passes"):
        _bare(M.ParallelWaveNet).fit(s, 1)
    with pytest.raises(NotImplementedError, match="pairs"):
        _bare(M.SiameseWaveNet).fit(s, 1)
    # a fixed-shape auto-encoder refuses another shape with its existing message
    ae = _bare(M.WaveNetAutoEncoder, condition_size=0, _eng=SimpleNamespace(B=2, T=64))
    with pytest.raises(NotImplementedError, match=r"one \(batch, length\) per model object.*\(2, 64\), got \(3, 64\)"):
        ae.fit(s, 1)
    # models whose labels are inputs refuse a dataset without them, or with another width
    with pytest.raises(ValueError, match="holds no labels"):
        _bare(M.WaveNetAutoEncoder, condition_size=4, _eng=SimpleNamespace(B=3, T=64)).fit(s, 1)
    with pytest.raises(ValueError, match="holds no labels"):
        _bare(M.WaveNet, input_size=64, output_size=4).fit(s, 1)
    with pytest.raises(ValueError, match="input_size=32"):
        _bare(M.WaveNet, input_size=32, output_size=4).fit(s, 1)
    s5 = _bare(D.BatchSampler, dataset=_bare_dataset(D, labels=object(), num_classes=5), batch_size=3, num_samples=64)
    with pytest.raises(ValueError, match="num_classes=5"):
        _bare(M.WaveNet, input_size=64, output_size=4).fit(s5, 1)


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    lib = _lib("ctypes")
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES and 'm.def("%s"' % n in src, n
        assert hasattr(lib, n), n
    assert lib.srwn_version() >= 122
    assert "srwn_data.hip" in sub("build").SOURCES


def _draw(lib, clips=A, labels=A, n=7, clip_len=70, state=A, B=3, T=64, shuffle=1, crop=0, rank=0, world=1, audio0=A,
          audio1=None, codes=None, Q=256, onehot=None, ld=4, rows=1, col0=0, classes=4, odt=0, indices=A):
    return lib.srwn_batch_draw(clips, labels, n, clip_len, state, B, T, shuffle, crop, rank, world, audio0, audio1, codes, Q,
                               onehot, ld, rows, col0, classes, odt, indices, None)


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    assert _draw(lib, B=0) == 0 and _draw(lib, T=0) == 0                       # empty work: done before any launch
    for kw in (dict(clips=None), dict(state=None), dict(audio0=None), dict(indices=None),
               dict(onehot=A, labels=None)):
        assert _draw(lib, **kw) == E_NULL, kw
        assert b"batch_draw" in lib.srwn_last_error()
    for kw in (dict(n=0), dict(clip_len=0), dict(T=71), dict(B=-1), dict(B=65536), dict(rank=1), dict(rank=-1, world=2),
               dict(world=0), dict(crop=2), dict(codes=A, Q=1), dict(onehot=A, ld=3), dict(onehot=A, col0=1),
               dict(onehot=A, classes=0), dict(onehot=A, rows=0), dict(onehot=A, col0=-1), dict(audio0=A + 2),
               dict(audio1=A + 1), dict(codes=A + 2), dict(clips=A + 1)):
        assert _draw(lib, **kw) == E_SHAPE, kw
    assert _draw(lib, onehot=A, odt=7) == E_DTYPE
    assert lib.srwn_step_log(None, A, 4, A, None) == E_NULL
    assert lib.srwn_step_log(A, None, 4, A, None) == E_NULL
    assert lib.srwn_step_log(A, A, 4, None, None) == E_NULL and b"step_log" in lib.srwn_last_error()
    assert lib.srwn_step_log(A, A, 0, A, None) == E_SHAPE
