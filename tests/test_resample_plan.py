"""CPU tests of speed perturbation in the augmented draws (srwn_version() 128): ``Augment(speed=, taps=)`` and what it
refuses, the order function ``dataset.speed_plan``, the filter ``dataset.resample_table`` and the sample rule
``dataset.resample_rows`` -- the specifications the kernels of csrc/srwn_resample.hip implement --, the quality of that rule
on sines against a bound measured here on the CPU (tests/resample_design.py: worst error 4.75e-4, bound 9.5e-4), the two C
entries declared, bound, generated and exported with their argument errors without a GPU, the drivers' flags, and the
samplers' dispatch: an ``Augment`` whose speed is the default draws through the ``_aug`` entries as before."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import resample_design as R
from tests._pkg import ROOT, sub

NEW = ["srwn_batch_draw_warp", "srwn_pair_draw_warp"]
E_DTYPE, E_SHAPE, E_NULL = -1, -2, -3
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take
SEED = 3
F = np.float32
ONE = 1 << 24


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
def test_augment_speed_defaults_and_immutability():
    D = sub("dataset")
    a = D.Augment()
    assert (a.speed, a.taps, a.step_lo, a.step_hi, a.resamples, a.cutoff) == ((1.0, 1.0), 16, ONE, ONE, False, 1.0)
    assert "speed" not in repr(a)
    a = D.Augment(shift=5, speed=(0.9, 1.1), taps=32)
    assert a.speed == (0.9, 1.1) and a.taps == 32 and a.shift == 5 and a.resamples and a.cutoff == 1.0 / 1.1
    assert (a.step_lo, a.step_hi) == (round(0.9 * 2 ** 24), round(1.1 * 2 ** 24)) == (15099494, 18454938)
    assert "speed=(0.9, 1.1)" in repr(a) and "taps=32" in repr(a)
    assert D.Augment(speed=[0.5, 2]).speed == (0.5, 2.0) and D.Augment(speed=(0.5, 2.0)).cutoff == 0.5
    assert (D.Augment(speed=(0.5, 2.0)).step_lo, D.Augment(speed=(0.5, 2.0)).step_hi) == (1 << 23, 1 << 25)
    for name in ("speed", "taps", "step_lo", "step_hi"):
        with pytest.raises(AttributeError, match="immutable"):
            setattr(a, name, 1)
        with pytest.raises(AttributeError, match="immutable"):
            delattr(a, name)
    # the five arguments in front keep their places
    b = D.Augment(3, (0.5, 2.0), None, 0.0, (0.0, 0.0), (0.9, 1.0), 8)
    assert (b.shift, b.gain, b.speed, b.taps) == (3, (0.5, 2.0), (0.9, 1.0), 8)


def test_augment_speed_refusals():
    D = sub("dataset")
    for bad in ((1.1, 0.9), (0.49, 1.0), (1.0, 2.01), (float("nan"), 1.0), (1.0, float("nan")), (1.0, float("inf")),
                (-1.0, 1.0), 1.0, (1.0,), (0.9, 1.0, 1.1), "fast"):
        with pytest.raises(ValueError, match="speed"):
            D.Augment(speed=bad)
    for bad in (0, 1, 3, 15, 66, -2, 16.0, True, "16", None):
        with pytest.raises(ValueError, match="taps"):
            D.Augment(speed=(0.9, 1.1), taps=bad)
    for ok in (2, 4, 16, 64, np.int64(8)):
        assert D.Augment(taps=ok).taps == int(ok)


# ---- speed_plan ---------------------------------------------------------------------------------------------------------
def test_speed_plan_is_a_pure_function_with_the_stated_draw():
    D = sub("dataset")
    a = D.Augment(speed=(0.9, 1.1))
    p, q = D.speed_plan(SEED, 2, 4, a), D.speed_plan(SEED, 2, 4, a)
    assert p.dtype == np.int64 and p.shape == (4,) and np.array_equal(p, q)
    # the statement itself, for one row: position 2 * 4 + 1 = 9, both sides
    for side in (0, 1):
        h = D._mix64((SEED ^ D.AUG_SPEED_SALT) + D._GOLDEN * (2 * 9 + side + 1))
        want = a.step_lo + (((h >> 32) * (a.step_hi - a.step_lo + 1)) >> 32)
        assert D.speed_plan(SEED, 2, 4, a, side=side)[1] == want
    salts = [D.AUG_SPEED_SALT, D.AUG_SHIFT_SALT, D.AUG_GAIN_SALT, D.AUG_COIN_SALT, D.AUG_PICK_SALT, D.AUG_OFFSET_SALT,
             D.AUG_VOLUME_SALT, D._CROP_SALT, D.NOISE_SALT, D.PAIR_SALT, D.PAIR_PICK_SALT, D.PAIR_CROP_SALT]
    assert len(set(salts)) == len(salts)
    assert (D.speed_plan(SEED, 0, 64, D.Augment()) == ONE).all()
    assert (D.speed_plan(SEED, 0, 64, D.Augment(speed=(1.25, 1.25))) == 5 << 22).all()
    with pytest.raises(ValueError, match="side"):
        D.speed_plan(SEED, 0, 4, a, side=2)
    with pytest.raises(ValueError, match="rank"):
        D.speed_plan(SEED, 0, 4, a, rank=2, world=2)
    with pytest.raises(TypeError, match="Augment"):
        D.speed_plan(SEED, 0, 4, dict(speed=(0.9, 1.1)))


def test_speed_plan_reaches_both_ends():
    """A range of five steps over 4096 positions: every step occurs, none outside; and a wide range stays inside."""
    D = sub("dataset")
    lo = ONE - 2
    a = D.Augment(speed=(lo / 2.0 ** 24, (lo + 4) / 2.0 ** 24))
    assert (a.step_lo, a.step_hi) == (lo, lo + 4)
    p = D.speed_plan(SEED, 0, 4096, a)
    assert sorted(set(p.tolist())) == [lo, lo + 1, lo + 2, lo + 3, lo + 4]
    a = D.Augment(speed=(0.5, 2.0))
    p = D.speed_plan(SEED, 0, 4096, a)
    assert p.min() >= 1 << 23 and p.max() <= 1 << 25 and p.min() < 0.51 * ONE and p.max() > 1.99 * ONE


def test_speed_plan_rows_ranks_steps_and_sides_never_share_a_draw():
    D = sub("dataset")
    a = D.Augment(speed=(0.5, 2.0))
    rows = D.speed_plan(SEED, 0, 4, a).tolist() + D.speed_plan(SEED, 1, 4, a).tolist()
    rows += D.speed_plan(SEED, 0, 4, a, side=1).tolist()
    rows += D.speed_plan(SEED, 1, 4, a, rank=1, world=2).tolist()            # positions 12..15
    rows += D.speed_plan(SEED + 1, 0, 4, a).tolist()
    assert len(set(rows)) == len(rows) == 20
    for side in (0, 1):                       # ranks interleave as positions do, on both sides
        r0 = D.speed_plan(SEED, 3, 3, a, rank=0, world=2, side=side)
        r1 = D.speed_plan(SEED, 3, 3, a, rank=1, world=2, side=side)
        assert r0.tolist() + r1.tolist() == D.speed_plan(SEED, 3, 6, a, side=side).tolist()


def test_setting_speed_leaves_the_six_other_draws_alone():
    D = sub("dataset")
    nz = _bare_dataset(D, 5, 90)
    kw = dict(shift=9, gain=(0.5, 1.5), noise=nz, noise_prob=0.5, noise_volume=(0.1, 0.4))
    for side in (0, 1):
        p = D.augment_plan(SEED, 2, 64, 64, D.Augment(**kw), 5, 90, side=side)
        q = D.augment_plan(SEED, 2, 64, 64, D.Augment(speed=(0.9, 1.1), taps=8, **kw), 5, 90, side=side)
        assert p._fields == q._fields == ("shift", "gain", "mix", "noise_index", "noise_offset", "volume")
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(p, q))


def test_samplers_state_their_speed_plan():
    D = sub("dataset")
    a = D.Augment(speed=(0.9, 1.1))
    s = _bare(D.BatchSampler, augment=a, seed=SEED, step=4, batch_size=3, num_samples=64, rank=1, world=2)
    assert np.array_equal(s.speed_plan(), D.speed_plan(SEED, 4, 3, a, 1, 2))
    assert np.array_equal(s.speed_plan(7), D.speed_plan(SEED, 7, 3, a, 1, 2))
    ps = _bare(D.PairSampler, augment=a, seed=SEED, step=4, batch_size=3, pairs=3, num_samples=64, rank=0, world=1)
    left, right = ps.speed_plan()
    assert np.array_equal(left, D.speed_plan(SEED, 4, 3, a, side=0)) and np.array_equal(right, D.speed_plan(SEED, 4, 3, a, side=1))
    assert np.array_equal(ps.speed_plan(5, side=1), D.speed_plan(SEED, 5, 3, a, side=1))
    assert not np.array_equal(left, right)
    with pytest.raises(ValueError, match="does not augment"):
        _bare(D.BatchSampler).speed_plan(0)


# ---- resample_table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [2, 16, 64])
@pytest.mark.parametrize("cutoff", [1.0, 1 / 1.1, 0.5])
def test_table_rows_sum_to_one(cutoff, taps):
    """Every phase row was divided by its sum in float64 and rounded once, entry by entry: entry k moves by at most
    2^-24 |h_k| (fp32's unit roundoff), so the row's sum by at most 2^-24 sum |h_k| (the rows' absolute sums lie between
    1 and 2.1)."""
    D = sub("dataset")
    t = D.resample_table(cutoff, taps)
    assert t.dtype == F and t.shape == (D.RESAMPLE_PHASES, taps) and not t.flags.writeable
    t64 = t.astype(np.float64)
    absum = np.abs(t64).sum(axis=1)
    assert (np.abs(t64.sum(axis=1) - 1.0) <= 2.0 ** -24 * absum).all()
    assert D.resample_table(cutoff, taps) is t                          # one table per (cutoff, taps)


def test_table_layout():
    D = sub("dataset")
    P = D.RESAMPLE_PHASES
    assert P & (P - 1) == 0 and P <= ONE
    for taps in (2, 16, 64):
        t = D.resample_table(1.0, taps)
        impulse = np.zeros(taps, F)
        impulse[taps // 2 - 1] = 1.0
        assert np.array_equal(t[0].view(np.uint32), impulse.view(np.uint32))       # exact, every zero +0.0
        # the peak moves from tap taps/2 - 1 to tap taps/2 as the phase grows: the tap nearest the position
        assert t[1].argmax() == taps // 2 - 1 and t[P - 1].argmax() == taps // 2
        # phase f read forwards is phase P - f read backwards (the position seen from the other side)
        assert np.allclose(t[P // 4], t[P - P // 4][::-1], rtol=0, atol=2.0 ** -23)
    # the stated weights, for one entry: cutoff 0.5, tap 9 of phase 1000 of 16
    t = D.resample_table(0.5, 16)
    d = (np.arange(16) - 7) - 1000 / P
    h = 0.5 * np.sinc(0.5 * d) * np.i0(D.RESAMPLE_BETA * np.sqrt(1 - (d / 8) ** 2)) / np.i0(D.RESAMPLE_BETA)
    assert np.array_equal(t[1000], (h / h.sum()).astype(F))
    assert t[0, 7] != 1.0                                                   # (only cutoff 1 has the impulse)
    for bad in (0.0, 1.5, -0.5, float("nan")):
        with pytest.raises(ValueError, match="cutoff"):
            D.resample_table(bad, 16)
    for bad in (0, 3, 66):
        with pytest.raises(ValueError, match="taps"):
            D.resample_table(1.0, bad)


# ---- resample_rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [2, 16, 64])
def test_rows_at_speed_one_are_the_rows(taps):
    D = sub("dataset")
    rng = np.random.default_rng(0)
    x = rng.uniform(-1.5, 1.5, (3, 37)).astype(F)
    x[0, :6] = [1.0, -1.0, 0.0, 1e-42, -1e-42, 2.0 ** -126]
    x[1, 5] = -0.0
    y = D.resample_rows(x, [ONE] * 3, D.resample_table(1.0, taps))
    assert y.dtype == F
    want = x.copy()
    want[1, 5] = 0.0                                                       # +0.0 + -0.0
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))


def test_rows_statement_for_one_sample():
    """Row 1, output 11 at step 1.1: q = 11 * step, i = 12, the phase by floor, 16 products summed in tap order."""
    D = sub("dataset")
    a = D.Augment(speed=(1.1, 1.1))
    t = a.table()
    x = np.random.default_rng(1).uniform(-1, 1, (2, 20)).astype(F)
    y = D.resample_rows(x, [a.step_lo, a.step_hi], t)
    q = 11 * a.step_hi
    i, f = q >> 24, (q >> (24 - (D.RESAMPLE_PHASES.bit_length() - 1))) & (D.RESAMPLE_PHASES - 1)
    assert i == 12 and f == int((11 * a.step_hi / 2 ** 24 - 12) * D.RESAMPLE_PHASES)
    acc = F(0.0)
    for k in range(16):
        at = i - 7 + k
        acc = F(acc + F(t[f, k] * (x[1, at] if 0 <= at < 20 else F(0.0))))
    assert y[1, 11] == acc
    # faster: the content ends at T / s and zeros follow once the window has left the row
    z = D.resample_rows(x, [1 << 25, 1 << 25], D.resample_table(0.5, 16))
    assert z[0, 18:].view(np.uint32).tolist() == [0, 0]                   # positions 36, 38: the window starts at 29, 31
    assert z[0, :14].all()                                                # (position 26: the window still holds 19)
    for bad in ([1 << 22, ONE], [ONE, (1 << 25) + 1]):
        with pytest.raises(ValueError, match="steps"):
            D.resample_rows(x, bad, t)
    with pytest.raises(ValueError, match="rows"):
        D.resample_rows(x, [ONE], t)
    with pytest.raises(ValueError, match="table"):
        D.resample_rows(x, [ONE, ONE], t[:16])


def test_rows_quality_on_sines():
    """tests/resample_design.py: every case within twice the worst error measured there, on the CPU."""
    D = sub("dataset")
    errors = R.quality_errors(D)
    for s, f, e in errors:
        print("speed %.1f  tone %.2f of Nyquist  worst error %.3e" % (s, f, e))
    assert len(errors) == 11 and (2.0, 0.4) not in [(s, f) for s, f, _ in errors]
    worst = max(e for _, _, e in errors)
    print("worst %.4e  recorded %.4e  bound %.4e" % (worst, R.MEASURED_WORST, R.QUALITY_BOUND))
    assert worst <= R.QUALITY_BOUND
    assert R.QUALITY_BOUND == 2 * R.MEASURED_WORST and abs(worst - R.MEASURED_WORST) < 0.01 * R.MEASURED_WORST


# ---- the drivers --------------------------------------------------------------------------------------------------------
def test_driver_flags():
    import argparse
    D = sub("dataset")
    p = argparse.ArgumentParser()
    D.add_augment_flags(p)
    assert D.augment_from_flags(p.parse_args([]), True) is None
    a = D.augment_from_flags(p.parse_args(["--speed", "0.9:1.1"]), True)
    assert (a.speed, a.taps, a.shift, a.gain) == ((0.9, 1.1), 16, 0, (1.0, 1.0))
    a = D.augment_from_flags(p.parse_args(["--speed", "0.9:1.1", "--resample-taps", "32", "--shift", "7"]), True)
    assert (a.speed, a.taps, a.shift) == ((0.9, 1.1), 32, 7)
    for flags in (["--speed", "0.9:1.1"], ["--resample-taps", "32"]):
        with pytest.raises(SystemExit, match="%s: augmentation happens where the batch is drawn on the device; add "
                                             "--device-data" % flags[0]):
            D.augment_from_flags(p.parse_args(flags), False)
    for flags, why in ((["--speed", "1.1:0.9"], "speed"), (["--speed", "1"], "LO:HI"), (["--speed", "0.4:1"], "speed"),
                       (["--resample-taps", "7"], "taps")):
        with pytest.raises(SystemExit, match=why):
            D.augment_from_flags(p.parse_args(flags), True)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_generated():
    L, D = sub("_lib"), sub("dataset")
    raw = open(os.path.join(ROOT, "include", "srwn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    lib = _lib("ctypes")
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES and 'm.def("%s"' % n in src, n
        assert hasattr(lib, n), n
    assert len(L.SIGNATURES["srwn_batch_draw_warp"][1]) == len(L.SIGNATURES["srwn_batch_draw_aug"][1]) + 4
    assert len(L.SIGNATURES["srwn_pair_draw_warp"][1]) == len(L.SIGNATURES["srwn_pair_draw_aug"][1]) + 4
    assert lib.srwn_version() >= 128
    assert "srwn_resample.hip" in sub("build").SOURCES
    assert "since srwn_version() 128" in raw
    assert int(re.search(r"#define SRWN_RESAMPLE_PHASES (\d+)", hdr).group(1)) == D.RESAMPLE_PHASES
    # the augmenting units share one statement of a row's plan, and the order function with the other draws
    csrc = os.path.join(ROOT, "sr-wavenet_amd", "csrc")
    for unit in ("srwn_augment.hip", "srwn_resample.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "srwn_augment.h"' in text and '#include "srwn_draw_common.h"' in text, unit
        assert "0xBF58476D1CE4E5B9" not in text and "kAugShiftSalt =" not in text, unit
    assert "%X" % D.AUG_SPEED_SALT in open(os.path.join(csrc, "srwn_resample.hip")).read()


def _batch(lib, clips=A, labels=A, n=7, clip_len=70, state=A, B=2, T=64, shuffle=1, crop=0, rank=0, world=1, a0=A, a1=None,
           codes=None, Q=256, onehot=None, ld=16, rows=1, col0=8, classes=4, dt=0, indices=A, shift=3, gain=(0.5, 2.0),
           noise=A, nn=2, nlen=90, thr=1 << 31, vol=(0.0, 0.5), table=A, taps=16, steps=(15099494, 18454938)):
    return lib.srwn_batch_draw_warp(clips, labels, n, clip_len, state, B, T, shuffle, crop, rank, world, a0, a1, codes, Q,
                                    onehot, ld, rows, col0, classes, dt, indices, shift, gain[0], gain[1], noise, nn, nlen,
                                    thr, vol[0], vol[1], table, taps, steps[0], steps[1], None)


def _pair(lib, clips=A, labels=A, order=A, place=A, start=A, classes=4, n=9, clip_len=70, state=A, P=3, T=64, same=1 << 31,
          shuffle=1, crop=0, rank=0, world=1, audio=A, y=A, left=A, right=A, ylog=A, shift=3, gain=(0.5, 2.0), noise=A, nn=2,
          nlen=90, thr=1 << 31, vol=(0.0, 0.5), table=A, taps=16, steps=(15099494, 18454938)):
    return lib.srwn_pair_draw_warp(clips, labels, order, place, start, classes, n, clip_len, state, P, T, same, shuffle, crop,
                                   rank, world, audio, y, left, right, ylog, shift, gain[0], gain[1], noise, nn, nlen, thr,
                                   vol[0], vol[1], table, taps, steps[0], steps[1], None)


AUG_SHAPE_ERRORS = (dict(shift=64), dict(shift=-1), dict(nlen=63), dict(gain=(2.0, 1.0)), dict(gain=(-0.5, 1.0)),
                    dict(gain=(0.0, float("inf"))), dict(gain=(float("nan"), 1.0)), dict(vol=(0.5, 0.25)),
                    dict(vol=(-1.0, -0.5)), dict(vol=(0.0, float("nan"))), dict(nn=-1), dict(thr=-1),
                    dict(thr=(1 << 32) + 1), dict(noise=A + 2))
WARP_SHAPE_ERRORS = (dict(taps=0), dict(taps=1), dict(taps=15), dict(taps=66), dict(taps=-2),
                     dict(steps=(ONE + 1, ONE)), dict(steps=((1 << 23) - 1, ONE)), dict(steps=(ONE, (1 << 25) + 1)),
                     dict(steps=(0, 0)), dict(steps=(-ONE, ONE)), dict(table=A + 2))


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    assert _batch(lib, B=0) == 0 and _batch(lib, T=0) == 0 and _pair(lib, P=0) == 0 and _pair(lib, T=0) == 0
    for kw in (dict(clips=None), dict(state=None), dict(a0=None), dict(indices=None), dict(onehot=A, labels=None),
               dict(noise=None), dict(table=None)):
        assert _batch(lib, **kw) == E_NULL, kw
    assert b"batch_draw_warp" in lib.srwn_last_error()
    for kw in (dict(T=71), dict(n=0), dict(B=65536), dict(rank=1), dict(crop=2), dict(codes=A, Q=1),
               dict(onehot=A, ld=11), dict(onehot=A, rows=0), dict(a1=A + 2), dict(codes=A + 1)) + AUG_SHAPE_ERRORS + \
            WARP_SHAPE_ERRORS:
        assert _batch(lib, **kw) == E_SHAPE, kw
    assert _batch(lib, onehot=A, dt=7) == E_DTYPE
    for kw in (dict(labels=None), dict(order=None), dict(place=None), dict(start=None), dict(audio=None), dict(y=None),
               dict(left=None), dict(right=None), dict(ylog=None), dict(clips=None), dict(state=None), dict(noise=None),
               dict(table=None)):
        assert _pair(lib, **kw) == E_NULL, kw
    assert b"pair_draw_warp" in lib.srwn_last_error()
    for kw in (dict(T=71), dict(n=0), dict(P=32768), dict(rank=2, world=2), dict(crop=-1), dict(same=-1),
               dict(same=(1 << 32) + 1), dict(classes=0), dict(audio=A + 2)) + AUG_SHAPE_ERRORS + WARP_SHAPE_ERRORS:
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


def test_batch_sampler_dispatch(calls):
    D = sub("dataset")
    ds = _bare_dataset(D, labels=_ptr(2000), num_classes=4)
    kw = dict(dataset=ds, batch_size=3, num_samples=64, shuffle=True, crop="random", rank=1, world=2, state=_ptr(3000),
              indices=_ptr(4000))
    plain = (1000, 2000, 7, 70, 3000, 3, 64, 1, 1, 1, 2, "a0", None, None, 0, None, 0, 1, 0, 4, 0, 4000)
    nz = _bare_dataset(D, 5, 90, base=5000)
    aug = dict(shift=6, gain=(0.5, 2.0), noise=nz, noise_prob=0.25, noise_volume=(0.1, 0.4))
    block = (6, 0.5, 2.0, 5000, 5, 90, 1 << 30, 0.1, 0.4)
    # the default speed, spelled or not, with any taps: the _aug entry and its arguments, nothing behind them
    for a in (D.Augment(**aug), D.Augment(speed=(1.0, 1.0), **aug), D.Augment(taps=8, **aug)):
        _bare(D.BatchSampler, augment=a, **kw).draw("a0")
        assert calls.pop() == ("srwn_batch_draw_aug",) + plain + block + (77,)
    _bare(D.BatchSampler, **kw).draw("a0")
    assert calls.pop() == ("srwn_batch_draw",) + plain + (77,)
    # a speed: the new entry, the same arguments, then the resampling block, then the stream
    a = D.Augment(speed=(0.9, 1.1), taps=32, **aug)
    _bare(D.BatchSampler, augment=a, _resample_dev=_ptr(6000), **kw).draw("a0")
    assert calls.pop() == ("srwn_batch_draw_warp",) + plain + block + (6000, 32, 15099494, 18454938, 77)
    _bare(D.BatchSampler, augment=D.Augment(speed=(2.0, 2.0)), _resample_dev=_ptr(6000), **kw).draw("a0")
    assert calls.pop()[-14:] == (0, 1.0, 1.0, None, 0, 0, 0, 0.0, 0.0, 6000, 16, 1 << 25, 1 << 25, 77)
    assert not calls


def test_pair_sampler_dispatch(calls):
    D = sub("dataset")
    ds = _bare_dataset(D, n=9, labels=_ptr(2000), num_classes=4)
    kw = dict(dataset=ds, batch_size=3, pairs=3, num_samples=64, shuffle=False, crop="head", rank=0, world=1,
              state=_ptr(3000), indices=_ptr(4000), right=_ptr(4100), y=_ptr(4200), same_threshold=1 << 31,
              _index=(_ptr(11), _ptr(12), _ptr(13)))
    plain = (1000, 2000, 11, 12, 13, 4, 9, 70, 3000, 3, 64, 1 << 31, 0, 0, 0, 1, "audio", "labels", 4000, 4100, 4200)
    block = (6, 0.5, 2.0, None, 0, 0, 0, 0.0, 0.0)
    _bare(D.PairSampler, augment=D.Augment(shift=6, gain=(0.5, 2.0)), **kw).draw("audio", "labels")
    assert calls.pop() == ("srwn_pair_draw_aug",) + plain + block + (77,)
    a = D.Augment(shift=6, gain=(0.5, 2.0), speed=(0.5, 1.0), taps=2)
    _bare(D.PairSampler, augment=a, _resample_dev=_ptr(6000), **kw).draw("audio", "labels")
    assert calls.pop() == ("srwn_pair_draw_warp",) + plain + block + (6000, 2, 1 << 23, 1 << 24, 77)
    assert not calls


def test_evaluate_still_refuses_an_augmenting_sampler():
    D, M = sub("dataset"), sub("model")
    ds = _bare_dataset(D, n=6, labels=object(), num_classes=4)
    a = D.Augment(speed=(0.9, 1.1))
    plain = _bare(D.BatchSampler, dataset=ds, batch_size=3, num_samples=64, shuffle=False, world=1, augment=a)
    with pytest.raises(ValueError, match="WaveNetTeacher.evaluate: the sampler augments"):
        _bare(M.WaveNetTeacher, use_encoding=False).evaluate(plain)
    for name in ("distill_sampler", "eval_sampler", "embed_sampler"):
        with pytest.raises(TypeError, match="augment"):
            getattr(ds, name)(3, 64, augment=a)
