"""CPU tests of augmented draws (srwn_version() 127): ``dataset.Augment`` and what it refuses, the order function
``dataset.augment_plan`` and the sample rule ``dataset.augment_rows`` -- the specifications the kernels of
csrc/srwn_augment.hip implement --, the samplers' and ``evaluate``'s refusals before any device work, the two C entries
declared, bound, generated and exported with their argument errors without a GPU, and the samplers' dispatch: without an
``Augment`` a draw is the call it was."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests._pkg import ROOT, sub

NEW = ["srwn_batch_draw_aug", "srwn_pair_draw_aug"]
E_DTYPE, E_SHAPE, E_NULL = -1, -2, -3
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take
SEED = 3          # the coin count of test_plan_coin below is a property of this seed (checked here, on the CPU)
F = np.float32


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


def _ptr(v):
    return SimpleNamespace(data_ptr=lambda: v)


def _bare_dataset(D, n=7, clip_len=70, labels=None, num_classes=0, device="cuda", base=1000):
    return _bare(D.DeviceDataset, audio=SimpleNamespace(shape=(n, clip_len), data_ptr=lambda: base), labels=labels,
                 num_classes=num_classes, device=device)


# ---- Augment ------------------------------------------------------------------------------------------------------------
def test_augment_defaults_and_immutability():
    D = sub("dataset")
    a = D.Augment()
    assert (a.shift, a.gain, a.noise, a.noise_prob, a.noise_volume, a.noise_threshold) == (0, (1.0, 1.0), None, 0.0,
                                                                                          (0.0, 0.0), 0)
    nz = _bare_dataset(D, 2, 90)
    a = D.Augment(shift=5, gain=(0.5, 2), noise=nz, noise_prob=0.25, noise_volume=[0, 0.3])
    assert a.shift == 5 and a.gain == (0.5, 2.0) and a.noise is nz and a.noise_volume == (0.0, 0.3)
    assert a.noise_threshold == D.same_threshold(0.25) == 1 << 30
    with pytest.raises(AttributeError, match="immutable"):
        a.shift = 6
    with pytest.raises(AttributeError, match="immutable"):
        del a.gain
    assert "shift=5" in repr(a)


def test_augment_constructor_refusals():
    D = sub("dataset")
    nz = _bare_dataset(D, 2, 90)
    for kw in (dict(shift=-1), dict(shift=1.5), dict(shift=True), dict(shift=1 << 31)):
        with pytest.raises(ValueError, match="shift"):
            D.Augment(**kw)
    for bad in ((2.0, 1.0), (-0.5, 1.0), (0.0, float("inf")), (float("nan"), 1.0), (1.0, float("nan")), 1.0, (1.0,),
                (1.0, 2.0, 3.0), (0.0, 1e39)):                     # (1e39 is not finite in fp32)
        with pytest.raises(ValueError, match="gain"):
            D.Augment(gain=bad)
        with pytest.raises(ValueError, match="noise_volume"):
            D.Augment(noise=nz, noise_prob=1.0, noise_volume=bad)
    for p in (-0.1, 1.5, float("nan"), "often"):
        with pytest.raises(ValueError, match="noise_prob"):
            D.Augment(noise=nz, noise_prob=p)
    with pytest.raises(ValueError, match="without noise"):
        D.Augment(noise_prob=0.5)
    for wrong in (np.zeros((2, 90), F), "noise.npy", 3):
        with pytest.raises(TypeError, match="DeviceDataset"):
            D.Augment(noise=wrong)


def test_sampler_construction_refusals_without_a_device():
    D = sub("dataset")
    d = _bare_dataset(D)
    labelled = _bare_dataset(D, labels=object(), num_classes=4)
    makers = (lambda a: d.sampler(3, 64, augment=a), lambda a: labelled.pair_sampler(3, 64, augment=a),
              lambda a: D.BatchSampler(d, 3, 64, augment=a), lambda a: D.PairSampler(labelled, 3, 64, augment=a))
    for make in makers:
        with pytest.raises(ValueError, match="shift 64: below num_samples 64"):
            make(D.Augment(shift=64))
        with pytest.raises(ValueError, match="shorter than num_samples"):
            make(D.Augment(noise=_bare_dataset(D, 2, 63), noise_prob=1.0))
        with pytest.raises(ValueError, match="the noise is on cpu"):
            make(D.Augment(noise=_bare_dataset(D, 2, 90, device="cpu"), noise_prob=1.0))
        with pytest.raises(TypeError, match="must be an Augment"):
            make(dict(shift=3))
    # the samplers whose draws are not augmented take no such keyword
    a = D.Augment(shift=3)
    with pytest.raises(TypeError, match="augment"):
        labelled.distill_sampler(3, 64, augment=a)
    with pytest.raises(TypeError, match="augment"):
        labelled.eval_sampler(3, 64, augment=a)
    with pytest.raises(TypeError, match="augment"):
        labelled.embed_sampler(3, 64, augment=a)
    # a sampler without one has no plan to state
    with pytest.raises(ValueError, match="does not augment"):
        _bare(D.BatchSampler).augment_plan(0)


def test_evaluate_refuses_an_augmenting_sampler():
    """A held-out sweep is not augmented: every ``evaluate`` says so before any device work."""
    D, M = sub("dataset"), sub("model")
    ds = _bare_dataset(D, n=6, labels=object(), num_classes=4)
    a = D.Augment(shift=3)
    plain = _bare(D.BatchSampler, dataset=ds, batch_size=3, num_samples=64, shuffle=False, world=1, augment=a)
    with pytest.raises(ValueError, match="WaveNetTeacher.evaluate: the sampler augments"):
        _bare(M.WaveNetTeacher, use_encoding=False).evaluate(plain)
    with pytest.raises(ValueError, match="WaveNetAutoEncoder.evaluate: the sampler augments"):
        _bare(M.WaveNetAutoEncoder).evaluate(plain)
    distill = _bare(D.DistillSampler, dataset=ds, batch_size=3, num_samples=64, shuffle=False, world=1, augment=a)
    with pytest.raises(ValueError, match="ParallelWaveNet.evaluate: the sampler augments"):
        _bare(M.ParallelWaveNet).evaluate(distill)
    with pytest.raises(ValueError, match="WaveNet.evaluate: the sampler augments"):
        _bare(M.WaveNet).evaluate(_bare(D.EvalSampler, augment=a))
    with pytest.raises(ValueError, match="SiameseWaveNet.evaluate: the sampler augments"):
        _bare(M.SiameseWaveNet).evaluate(_bare(D.EmbedSampler, augment=a))
    # ... and the same bare samplers without one get past that check (to the next refusal: they shuffle)
    plain = _bare(D.BatchSampler, dataset=ds, batch_size=3, num_samples=64, shuffle=True, world=1)
    with pytest.raises(ValueError, match="the sampler shuffles"):
        _bare(M.WaveNetTeacher, use_encoding=False).evaluate(plain)


def test_driver_flags():
    """The flags of examples/classifier.py and examples/siamese.py: nothing asked is None, and without --device-data they
    are refused with a message, not ignored."""
    import argparse
    D = sub("dataset")
    p = argparse.ArgumentParser()
    D.add_augment_flags(p)
    assert D.augment_from_flags(p.parse_args([]), False) is None and D.augment_from_flags(p.parse_args([]), True) is None
    a = D.augment_from_flags(p.parse_args(["--shift", "100", "--gain", "0.5:2"]), True)
    assert (a.shift, a.gain, a.noise, a.noise_threshold) == (100, (0.5, 2.0), None, 0)
    for flags in (["--shift", "3"], ["--gain", "0.5:2"], ["--noise", "n.npy"], ["--noise-prob", "0.5"],
                  ["--noise-volume", "0:1"]):
        with pytest.raises(SystemExit, match="%s: augmentation happens where the batch is drawn on the device; add "
                                             "--device-data" % flags[0]):
            D.augment_from_flags(p.parse_args(flags), False)
    for flags, why in ((["--gain", "2:1"], "gain"), (["--gain", "1"], "LO:HI"), (["--noise-prob", "0.5"], "without noise"),
                       (["--shift", "-2"], "shift")):
        with pytest.raises(SystemExit, match=why):
            D.augment_from_flags(p.parse_args(flags), True)
    for name in ("classifier", "siamese"):
        src = open(os.path.join(ROOT, "examples", name + ".py")).read()
        assert "add_augment_flags(p)" in src and "augment_from_flags(a, a.device_data)" in src and "augment=a.augment" in src


# ---- augment_plan -------------------------------------------------------------------------------------------------------
def _noise(D, n=5, length=90):
    return _bare_dataset(D, n, length)


def test_plan_is_a_pure_function_with_the_stated_types():
    D = sub("dataset")
    a = D.Augment(shift=9, gain=(0.5, 1.5), noise=_noise(D), noise_prob=0.5, noise_volume=(0.1, 0.4))
    p = D.augment_plan(SEED, 2, 4, 64, a, 5, 90)
    q = D.augment_plan(SEED, 2, 4, 64, a, 5, 90)
    assert p._fields == ("shift", "gain", "mix", "noise_index", "noise_offset", "volume")
    assert [x.dtype for x in p] == [np.int32, np.float32, np.bool_, np.int32, np.int64, np.float32]
    for x, y in zip(p, q):
        assert x.shape == (4,) and np.array_equal(x, y)
    # the statement itself, for one row: position 2 * 4 + 1 = 9, side 0
    h = lambda salt: D._mix64((SEED ^ salt) + D._GOLDEN * (2 * 9 + 0 + 1))
    assert p.shift[1] == (((h(D.AUG_SHIFT_SALT) >> 32) * 19) >> 32) - 9
    u = F(h(D.AUG_GAIN_SALT) >> 40) * F(2.0 ** -24)
    assert p.gain[1] == F(F(0.5) + F(u * F(F(1.5) - F(0.5))))
    assert p.mix[1] == ((h(D.AUG_COIN_SALT) >> 32) < 1 << 31)
    assert p.noise_index[1] == ((h(D.AUG_PICK_SALT) >> 32) * 5) >> 32
    assert p.noise_offset[1] == ((h(D.AUG_OFFSET_SALT) >> 32) * 27) >> 32
    salts = [D.AUG_SHIFT_SALT, D.AUG_GAIN_SALT, D.AUG_COIN_SALT, D.AUG_PICK_SALT, D.AUG_OFFSET_SALT, D.AUG_VOLUME_SALT,
             D._CROP_SALT, D.NOISE_SALT, D.PAIR_SALT, D.PAIR_PICK_SALT, D.PAIR_CROP_SALT]
    assert len(set(salts)) == len(salts)


def test_plan_rows_of_other_positions_ranks_and_sides_differ():
    D = sub("dataset")
    a = D.Augment(shift=2000, gain=(0.25, 4.0))
    key = lambda p: list(zip(p.shift.tolist(), p.gain.tolist()))
    rows = key(D.augment_plan(SEED, 0, 4, 4096, a, 0, 0)) + key(D.augment_plan(SEED, 1, 4, 4096, a, 0, 0))
    rows += key(D.augment_plan(SEED, 0, 4, 4096, a, 0, 0, side=1))
    rows += key(D.augment_plan(SEED, 1, 4, 4096, a, 0, 0, rank=1, world=2))          # positions 12..15
    rows += key(D.augment_plan(SEED + 1, 0, 4, 4096, a, 0, 0))
    assert len(set(rows)) == len(rows) == 20
    # ranks interleave as positions do, on both sides
    for side in (0, 1):
        r0 = D.augment_plan(SEED, 3, 3, 4096, a, 0, 0, rank=0, world=2, side=side)
        r1 = D.augment_plan(SEED, 3, 3, 4096, a, 0, 0, rank=1, world=2, side=side)
        whole = D.augment_plan(SEED, 3, 6, 4096, a, 0, 0, side=side)
        assert key(r0) + key(r1) == key(whole)


def test_plan_shift_range_and_constant_gain():
    D = sub("dataset")
    p = D.augment_plan(SEED, 0, 4096, 64, D.Augment(shift=3, gain=(0.7, 0.7)), 0, 0)
    assert sorted(set(p.shift.tolist())) == [-3, -2, -1, 0, 1, 2, 3]
    assert (p.gain == F(0.7)).all()
    assert not p.mix.any() and not p.noise_index.any() and not p.noise_offset.any()
    p = D.augment_plan(SEED, 0, 64, 64, D.Augment(), 0, 0)
    assert not p.shift.any() and (p.gain == F(1.0)).all()
    g = D.augment_plan(SEED, 0, 4096, 64, D.Augment(gain=(0.5, 2.0)), 0, 0).gain
    assert g.min() >= F(0.5) and g.max() <= F(2.0) and g.min() < 0.51 and g.max() > 1.99


def test_plan_coin():
    D = sub("dataset")
    nz = _noise(D)
    mix = lambda prob: D.augment_plan(SEED, 0, 4096, 64, D.Augment(noise=nz, noise_prob=prob, noise_volume=(0.1, 0.2)), 5, 90).mix
    assert not mix(0.0).any() and mix(1.0).all()
    count = int(mix(0.5).sum())
    print("rows mixed at noise_prob 0.5, seed %d: %d of 4096" % (SEED, count))
    assert abs(count - 2048) <= 160          # five standard deviations (32) of a fair coin; one fixed number for this seed
    # without noise clips nothing mixes, whatever the Augment says
    a = D.Augment(noise=nz, noise_prob=1.0)
    assert not D.augment_plan(SEED, 0, 64, 64, a, 0, 0).mix.any()


def test_plan_noise_records_and_offsets_stay_inside():
    D = sub("dataset")
    a = D.Augment(noise=_noise(D), noise_prob=1.0, noise_volume=(0.25, 0.5))
    p = D.augment_plan(SEED, 0, 4096, 64, a, 5, 90)
    assert sorted(set(p.noise_index.tolist())) == [0, 1, 2, 3, 4]
    assert p.noise_offset.min() == 0 and p.noise_offset.max() == 26 and len(set(p.noise_offset.tolist())) == 27
    assert p.volume.min() >= F(0.25) and p.volume.max() <= F(0.5)
    p = D.augment_plan(SEED, 0, 4096, 64, a, 5, 64)               # noise_len == T: one window
    assert not p.noise_offset.any() and p.mix.all()
    with pytest.raises(ValueError, match="noise clips of 63 samples"):
        D.augment_plan(SEED, 0, 4, 64, a, 5, 63)
    with pytest.raises(ValueError, match="shift 64"):
        D.augment_plan(SEED, 0, 4, 64, D.Augment(shift=64), 0, 0)
    with pytest.raises(ValueError, match="side"):
        D.augment_plan(SEED, 0, 4, 64, a, 5, 90, side=2)


def test_sampler_states_its_plan():
    D = sub("dataset")
    nz = _noise(D)
    a = D.Augment(shift=5, noise=nz, noise_prob=0.5, noise_volume=(0.1, 0.2))
    s = _bare(D.BatchSampler, augment=a, seed=SEED, step=4, batch_size=3, num_samples=64, rank=1, world=2)
    for got, want in ((s.augment_plan(), D.augment_plan(SEED, 4, 3, 64, a, 5, 90, 1, 2)),
                      (s.augment_plan(7), D.augment_plan(SEED, 7, 3, 64, a, 5, 90, 1, 2))):
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    ps = _bare(D.PairSampler, augment=a, seed=SEED, step=4, batch_size=3, pairs=3, num_samples=64, rank=0, world=1)
    left, right = ps.augment_plan()
    assert all(np.array_equal(x, y) for x, y in zip(left, D.augment_plan(SEED, 4, 3, 64, a, 5, 90, side=0)))
    assert all(np.array_equal(x, y) for x, y in zip(right, D.augment_plan(SEED, 4, 3, 64, a, 5, 90, side=1)))


# ---- augment_rows -------------------------------------------------------------------------------------------------------
def _plan(D, shift=0, gain=1.0, mix=False, index=0, offset=0, volume=0.0, B=1):
    full = lambda v, dt: np.full(B, v, dt)
    return D.AugmentPlan(full(shift, np.int32), full(gain, F), full(mix, bool), full(index, np.int32),
                         full(offset, np.int64), full(volume, F))


def test_rows_identity():
    D = sub("dataset")
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (3, 37)).astype(F)
    x[0, :4] = [1.0, -1.0, 0.0, 1e-42]
    y = D.augment_rows(x, D.augment_plan(SEED, 0, 3, 37, D.Augment(), 0, 0))
    assert y.dtype == F and np.array_equal(y, x)
    # as values: -0.0 + +0.0 is +0.0, the one sign a zero has
    y = D.augment_rows(np.array([[-0.0, 0.0]], F), _plan(D))
    assert y.view(np.uint32).tolist() == [[0, 0]]


def test_rows_shift():
    D = sub("dataset")
    T = 9
    x = np.arange(1, T + 1, dtype=F)[None, :] / F(16)
    y = D.augment_rows(x, _plan(D, shift=T - 1))
    assert np.count_nonzero(y) == 1 and y[0, T - 1] == x[0, 0]
    y = D.augment_rows(x, _plan(D, shift=-(T - 1)))
    assert np.count_nonzero(y) == 1 and y[0, 0] == x[0, T - 1]
    assert D.augment_rows(x, _plan(D, shift=2))[0].tolist() == [0, 0] + x[0, :T - 2].tolist()
    assert D.augment_rows(x, _plan(D, shift=-2))[0].tolist() == x[0, 2:].tolist() + [0, 0]
    assert (D.augment_rows(x, _plan(D, shift=2)).view(np.uint32)[0, :2] == 0).all()      # the fill is +0.0


def test_rows_clamp_gain_and_noise():
    D = sub("dataset")
    up, down = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
    x = np.array([[up, down, 1.0, -1.0, 3.0, -3.0, np.nan, 0.5]], F)
    y = D.augment_rows(x, _plan(D))
    assert y[0, :6].tolist() == [1.0, -1.0, 1.0, -1.0, 1.0, -1.0] and np.isnan(y[0, 6]) and y[0, 7] == 0.5
    # gain, then noise at its offset and volume, each product and the sum rounded to fp32
    noise = np.arange(40, dtype=F).reshape(2, 20) / F(64)
    x = np.array([[0.3, -0.2, 0.1]], F)
    y = D.augment_rows(x, _plan(D, gain=0.7, mix=True, index=1, offset=5, volume=0.3), noise)
    want = [F(F(F(0.7) * x[0, j]) + F(F(0.3) * noise[1, 5 + j])) for j in range(3)]
    assert y[0].tolist() == want
    # a plan that does not mix ignores index, offset and volume
    assert np.array_equal(D.augment_rows(x, _plan(D, gain=0.7, index=1, offset=5, volume=0.3)),
                          D.augment_rows(x, _plan(D, gain=0.7)))
    with pytest.raises(ValueError, match="pass the noise clips"):
        D.augment_rows(x, _plan(D, mix=True))
    # a subnormal product is kept
    y = D.augment_rows(np.array([[2.0 ** -126]], F), _plan(D, gain=0.5))
    assert y[0, 0] == F(2.0 ** -127) and y[0, 0] != 0


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    raw = open(os.path.join(ROOT, "include", "srwn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    lib = _lib("ctypes")
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES and 'm.def("%s"' % n in src, n
        assert hasattr(lib, n), n
    assert len(L.SIGNATURES["srwn_batch_draw_aug"][1]) == len(L.SIGNATURES["srwn_batch_draw"][1]) + 9
    assert len(L.SIGNATURES["srwn_pair_draw_aug"][1]) == len(L.SIGNATURES["srwn_pair_draw"][1]) + 9
    assert lib.srwn_version() >= 127
    assert "srwn_augment.hip" in sub("build").SOURCES
    assert "since srwn_version() 127" in raw
    # the three draw units share one statement of the order function
    csrc = os.path.join(ROOT, "sr-wavenet_amd", "csrc")
    for unit in ("srwn_data.hip", "srwn_draw.hip", "srwn_augment.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "srwn_draw_common.h"' in text, unit
        assert "0xBF58476D1CE4E5B9" not in text, unit + " states mix64 itself"


def _batch(lib, clips=A, labels=A, n=7, clip_len=70, state=A, B=2, T=64, shuffle=1, crop=0, rank=0, world=1, a0=A, a1=None,
           codes=None, Q=256, onehot=None, ld=16, rows=1, col0=8, classes=4, dt=0, indices=A, shift=3, gain=(0.5, 2.0),
           noise=A, nn=2, nlen=90, thr=1 << 31, vol=(0.0, 0.5)):
    return lib.srwn_batch_draw_aug(clips, labels, n, clip_len, state, B, T, shuffle, crop, rank, world, a0, a1, codes, Q,
                                   onehot, ld, rows, col0, classes, dt, indices, shift, gain[0], gain[1], noise, nn, nlen,
                                   thr, vol[0], vol[1], None)


def _pair(lib, clips=A, labels=A, order=A, place=A, start=A, classes=4, n=9, clip_len=70, state=A, P=3, T=64, same=1 << 31,
          shuffle=1, crop=0, rank=0, world=1, audio=A, y=A, left=A, right=A, ylog=A, shift=3, gain=(0.5, 2.0), noise=A, nn=2,
          nlen=90, thr=1 << 31, vol=(0.0, 0.5)):
    return lib.srwn_pair_draw_aug(clips, labels, order, place, start, classes, n, clip_len, state, P, T, same, shuffle, crop,
                                  rank, world, audio, y, left, right, ylog, shift, gain[0], gain[1], noise, nn, nlen, thr,
                                  vol[0], vol[1], None)


AUG_SHAPE_ERRORS = (dict(shift=64), dict(shift=-1), dict(nlen=63), dict(gain=(2.0, 1.0)), dict(gain=(-0.5, 1.0)),
                    dict(gain=(0.0, float("inf"))), dict(gain=(float("nan"), 1.0)), dict(vol=(0.5, 0.25)),
                    dict(vol=(-1.0, -0.5)), dict(vol=(0.0, float("nan"))), dict(nn=-1), dict(thr=-1),
                    dict(thr=(1 << 32) + 1), dict(noise=A + 2))


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    assert _batch(lib, B=0) == 0 and _batch(lib, T=0) == 0 and _pair(lib, P=0) == 0 and _pair(lib, T=0) == 0
    for kw in (dict(clips=None), dict(state=None), dict(a0=None), dict(indices=None), dict(onehot=A, labels=None),
               dict(noise=None)):
        assert _batch(lib, **kw) == E_NULL, kw
    assert b"batch_draw_aug" in lib.srwn_last_error()
    for kw in (dict(T=71), dict(n=0), dict(B=65536), dict(rank=1), dict(crop=2), dict(codes=A, Q=1),
               dict(onehot=A, ld=11), dict(onehot=A, rows=0), dict(a1=A + 2), dict(codes=A + 1)) + AUG_SHAPE_ERRORS:
        assert _batch(lib, **kw) == E_SHAPE, kw
    assert _batch(lib, onehot=A, dt=7) == E_DTYPE
    for kw in (dict(labels=None), dict(order=None), dict(place=None), dict(start=None), dict(audio=None), dict(y=None),
               dict(left=None), dict(right=None), dict(ylog=None), dict(clips=None), dict(state=None), dict(noise=None)):
        assert _pair(lib, **kw) == E_NULL, kw
    assert b"pair_draw_aug" in lib.srwn_last_error()
    for kw in (dict(T=71), dict(n=0), dict(P=32768), dict(rank=2, world=2), dict(crop=-1), dict(same=-1),
               dict(same=(1 << 32) + 1), dict(classes=0), dict(audio=A + 2)) + AUG_SHAPE_ERRORS:
        assert _pair(lib, **kw) == E_SHAPE, kw


# ---- dispatch -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """``kernels.call`` recorded and not made; the tensors' checks answer with the stand-ins themselves."""
    K = sub("kernels")
    seen = []
    monkeypatch.setattr(K, "call", lambda name, *args: seen.append((name,) + args))
    monkeypatch.setattr(K, "_chk", lambda t, name, dtype=None, shape=None: t)
    monkeypatch.setattr(K, "_opt", lambda t, name, dtype=None, shape=None: t)
    monkeypatch.setattr(K, "_stream", lambda: 77)
    return seen


def test_a_plain_sampler_draws_as_before(calls):
    D = sub("dataset")
    ds = _bare_dataset(D, labels=_ptr(2000), num_classes=4)
    kw = dict(dataset=ds, batch_size=3, num_samples=64, shuffle=True, crop="random", rank=1, world=2, state=_ptr(3000),
              indices=_ptr(4000))
    codes = SimpleNamespace(numel=lambda: 192)
    _bare(D.BatchSampler, **kw).draw("a0", "a1", codes, 256)
    assert calls.pop() == ("srwn_batch_draw", 1000, 2000, 7, 70, 3000, 3, 64, 1, 1, 1, 2, "a0", "a1", codes, 256, None, 0, 1, 0,
                           4, 0, 4000, 77)
    _bare(D.BatchSampler, augment=None, **kw).draw("a0")
    assert calls.pop() == ("srwn_batch_draw", 1000, 2000, 7, 70, 3000, 3, 64, 1, 1, 1, 2, "a0", None, None, 0, None, 0, 1, 0,
                           4, 0, 4000, 77)
    # with an Augment: the other entry, the same arguments, then the augmentation block, then the stream
    nz = _bare_dataset(D, 5, 90, base=5000)
    a = D.Augment(shift=6, gain=(0.5, 2.0), noise=nz, noise_prob=0.25, noise_volume=(0.1, 0.4))
    _bare(D.BatchSampler, augment=a, **kw).draw("a0")
    assert calls.pop() == ("srwn_batch_draw_aug", 1000, 2000, 7, 70, 3000, 3, 64, 1, 1, 1, 2, "a0", None, None, 0, None, 0, 1,
                           0, 4, 0, 4000, 6, 0.5, 2.0, 5000, 5, 90, 1 << 30, 0.1, 0.4, 77)
    _bare(D.BatchSampler, augment=D.Augment(shift=2), **kw).draw("a0")
    assert calls.pop()[-10:] == (2, 1.0, 1.0, None, 0, 0, 0, 0.0, 0.0, 77)
    assert not calls


def test_a_plain_pair_sampler_draws_as_before(calls):
    D = sub("dataset")
    ds = _bare_dataset(D, n=9, labels=_ptr(2000), num_classes=4)
    kw = dict(dataset=ds, batch_size=3, pairs=3, num_samples=64, shuffle=False, crop="head", rank=0, world=1,
              state=_ptr(3000), indices=_ptr(4000), right=_ptr(4100), y=_ptr(4200), same_threshold=1 << 31,
              _index=(_ptr(11), _ptr(12), _ptr(13)))
    plain = (1000, 2000, 11, 12, 13, 4, 9, 70, 3000, 3, 64, 1 << 31, 0, 0, 0, 1, "audio", "labels", 4000, 4100, 4200)
    _bare(D.PairSampler, **kw).draw("audio", "labels")
    assert calls.pop() == ("srwn_pair_draw",) + plain + (77,)
    a = D.Augment(shift=6, gain=(0.5, 2.0))
    _bare(D.PairSampler, augment=a, **kw).draw("audio", "labels")
    assert calls.pop() == ("srwn_pair_draw_aug",) + plain + (6, 0.5, 2.0, None, 0, 0, 0, 0.0, 0.0, 77)
    assert not calls
