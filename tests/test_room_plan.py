"""CPU tests of room reverberation in the augmented draws: the two new keywords of ``dataset.Augment``, ``reverb_plan``,
``reverb_rows`` against ``np.convolve`` in float64 under the derived bound of tests/room_design.py, the planted operands,
the two host helpers, the drivers' flags, the C-ABI of ``srwn_batch_draw_room`` / ``srwn_pair_draw_room`` (every refusal
comes back before any launch, so none needs a GPU) and the calls the samplers make, recorded and not made: without
``reverb``, or at probability 0, exactly the calls of before."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import room_design as R
from tests._pkg import ROOT, sub

NEW = ["srwn_batch_draw_room", "srwn_pair_draw_room"]
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


def _host_dataset(D, array, device="cuda"):
    """A dataset whose clips are a host tensor: what ``Augment.check`` reduces."""
    import torch
    return _bare(D.DeviceDataset, audio=torch.as_tensor(np.asarray(array, F)), labels=None, num_classes=0, device=device)


# ---- Augment ------------------------------------------------------------------------------------------------------------
def test_augment_reverb_defaults_and_immutability():
    D = sub("dataset")
    a = D.Augment()
    assert (a.reverb, a.reverb_prob, a.reverb_threshold, a.reverberates) == (None, 0.0, 0, False)
    assert "reverb" not in repr(a)
    assert D.ROOM_MAX_TAPS == 8192
    rv = _bare_dataset(D, 5, 64)
    b = D.Augment(reverb=rv)
    assert not b.reverberates and repr(b) == repr(a)                # responses at probability 0 change nothing
    c = D.Augment(3, (0.5, 2.0), None, 0.0, (0.0, 0.0), (1.0, 1.0), 16, rv, 0.25)     # trailing, behind taps
    assert c.reverberates and c.reverb is rv and c.reverb_threshold == 1 << 30 and not c.resamples
    assert repr(c).endswith(", reverb=<5 responses of 64 taps>, reverb_prob=0.25)") and "speed" not in repr(c)
    assert D.Augment(reverb=rv, reverb_prob=1.0).reverb_threshold == 1 << 32
    for name in ("reverb", "reverb_prob", "reverb_threshold"):
        with pytest.raises(AttributeError):
            setattr(c, name, None)


def test_augment_reverb_refusals():
    D = sub("dataset")
    rv = _bare_dataset(D, 5, 64)
    with pytest.raises(TypeError, match="reverb must be a DeviceDataset"):
        D.Augment(reverb=np.zeros((2, 8), F))
    for p in (-0.1, 1.5, float("nan"), "x", None):
        with pytest.raises(ValueError, match="reverb_prob"):
            D.Augment(reverb=rv, reverb_prob=p)
    with pytest.raises(ValueError, match="reverb_prob 0.5 without reverb"):
        D.Augment(reverb_prob=0.5)


def test_check_refuses_what_only_a_sampler_knows():
    D = sub("dataset")
    ds = _bare_dataset(D)
    good = D.synthetic_rirs(3, 64)
    D.Augment(reverb=_host_dataset(D, good), reverb_prob=0.5).check(ds, 64)
    with pytest.raises(ValueError, match="the room responses are on cpu, the clips are on cuda"):
        D.Augment(reverb=_host_dataset(D, good, device="cpu"), reverb_prob=0.5).check(ds, 64)
    with pytest.raises(ValueError, match="room responses of 8193 taps: 1 to 8192"):
        D.Augment(reverb=_host_dataset(D, np.ones((1, 8193))), reverb_prob=0.5).check(ds, 64)
    D.Augment(reverb=_host_dataset(D, np.ones((1, 8192))), reverb_prob=0.5).check(ds, 64)
    for bad in (np.nan, np.inf, -np.inf):
        h = good.copy()
        h[2, 63] = bad
        with pytest.raises(ValueError, match="a tap that is not finite"):
            D.Augment(reverb=_host_dataset(D, h), reverb_prob=0.5).check(ds, 64)


# ---- reverb_plan --------------------------------------------------------------------------------------------------------
def test_reverb_plan_is_a_pure_function_with_the_stated_draws():
    D = sub("dataset")
    assert D.AUG_RIR_COIN_SALT == int.from_bytes(b"augrcoin", "big") == 0x61756772636F696E
    assert D.AUG_RIR_PICK_SALT == int.from_bytes(b"augrpick", "big") == 0x617567727069636B
    a = D.Augment(reverb=_bare_dataset(D, 5, 64), reverb_prob=0.3)
    p1, p2 = D.reverb_plan(SEED, 7, 6, a, 5, 1, 2, 1), D.reverb_plan(SEED, 7, 6, a, 5, 1, 2, 1)
    assert p1._fields == ("apply", "index") and p1.apply.dtype == bool and p1.index.dtype == np.int32
    assert all(np.array_equal(x, y) for x, y in zip(p1, p2))
    for b in range(6):
        p = (7 * 2 + 1) * 6 + b
        key = D._GOLDEN * (2 * p + 1 + 1)
        hc, hp = D._mix64((SEED ^ D.AUG_RIR_COIN_SALT) + key), D._mix64((SEED ^ D.AUG_RIR_PICK_SALT) + key)
        assert p1.apply[b] == ((hc >> 32) < a.reverb_threshold) and p1.index[b] == ((hp >> 32) * 5) >> 32
    for bad in (dict(batch_size=0), dict(rank=2, world=2), dict(side=2), dict(rir_n=-1)):
        kw = dict(seed=SEED, step=0, batch_size=4, augment=a, rir_n=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.reverb_plan(**kw)
    with pytest.raises(TypeError):
        D.reverb_plan(SEED, 0, 4, None, 5)


def test_reverb_plan_rows_ranks_steps_and_sides_never_share_a_draw():
    D = sub("dataset")
    a = D.Augment(reverb=_bare_dataset(D, 1 << 20, 64), reverb_prob=0.5)
    seen = {}
    for step in range(3):
        for rank in range(2):
            for side in (0, 1):
                pl = D.reverb_plan(SEED, step, 8, a, 1 << 20, rank, 2, side)
                for b in range(8):
                    seen[(step, rank, side, b)] = int(pl.index[b])
    assert len(set(seen.values())) == len(seen)                     # 96 draws on 2^20 values: none shared
    assert {bool(v) for st in range(3) for v in D.reverb_plan(SEED, st, 8, a, 1 << 20).apply} == {False, True}


def test_the_coin_and_the_indices():
    D = sub("dataset")
    rv = _bare_dataset(D, 5, 64)
    off, on = D.Augment(reverb=rv, reverb_prob=0.0), D.Augment(reverb=rv, reverb_prob=1.0)
    idx = []
    for step in range(20):
        assert not D.reverb_plan(SEED, step, 8, off, 5).apply.any()
        pl = D.reverb_plan(SEED, step, 8, on, 5)
        assert pl.apply.all()
        idx += pl.index.tolist()
    assert sorted(set(idx)) == [0, 1, 2, 3, 4]
    assert not D.reverb_plan(SEED, 0, 8, on, 0).apply.any()         # never without responses


def test_adding_reverb_leaves_the_seven_other_draws_alone():
    D = sub("dataset")
    nz = _bare_dataset(D, 5, 90)
    kw = dict(shift=6, gain=(0.5, 2.0), noise=nz, noise_prob=0.5, noise_volume=(0.1, 0.4), speed=(0.9, 1.1))
    a, b = D.Augment(**kw), D.Augment(reverb=_bare_dataset(D, 5, 64), reverb_prob=0.5, **kw)
    for step in range(4):
        for side in (0, 1):
            pa, pb = D.augment_plan(SEED, step, 6, 64, a, 5, 90, 1, 2, side), D.augment_plan(SEED, step, 6, 64, b, 5, 90, 1, 2, side)
            assert pa._fields == ("shift", "gain", "mix", "noise_index", "noise_offset", "volume")
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
            assert np.array_equal(D.speed_plan(SEED, step, 6, a, 1, 2, side), D.speed_plan(SEED, step, 6, b, 1, 2, side))


def test_samplers_state_their_reverb_plan():
    D = sub("dataset")
    rv = _bare_dataset(D, 5, 64)
    a = D.Augment(reverb=rv, reverb_prob=0.5)
    ds = _bare_dataset(D)
    s = _bare(D.BatchSampler, dataset=ds, batch_size=4, num_samples=64, seed=SEED, rank=1, world=2, step=9, augment=a)
    for got, want in ((s.reverb_plan(), D.reverb_plan(SEED, 9, 4, a, 5, 1, 2, 0)),
                      (s.reverb_plan(2, 1), D.reverb_plan(SEED, 2, 4, a, 5, 1, 2, 1))):
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    p = _bare(D.PairSampler, dataset=ds, batch_size=4, pairs=4, num_samples=64, seed=SEED, rank=0, world=1, step=5, augment=a)
    left, right = p.reverb_plan()
    assert all(np.array_equal(x, y) for x, y in zip(left, D.reverb_plan(SEED, 5, 4, a, 5, 0, 1, 0)))
    assert all(np.array_equal(x, y) for x, y in zip(right, D.reverb_plan(SEED, 5, 4, a, 5, 0, 1, 1)))
    assert all(np.array_equal(x, y) for x, y in zip(p.reverb_plan(3, 1), D.reverb_plan(SEED, 3, 4, a, 5, 0, 1, 1)))
    with pytest.raises(ValueError, match="does not augment"):
        _bare(D.BatchSampler, augment=None).reverb_plan()


# ---- reverb_rows --------------------------------------------------------------------------------------------------------
def _all(B, index=0):
    D = sub("dataset")
    return D.ReverbPlan(np.ones(B, bool), np.full(B, index, np.int32))


@pytest.mark.parametrize("T,K", [(4099, 4096), (5, 7), (300, 64), (64, 1)])
def test_rows_against_convolve_in_float64(T, K):
    D = sub("dataset")
    rng = np.random.default_rng(T + K)
    rows = rng.uniform(-1.0, 1.0, (2, T)).astype(F)
    h = D.synthetic_rirs(2, K, seed=K)
    plan = D.ReverbPlan(np.array([True, True]), np.array([1, 0], np.int32))
    e = D.reverb_rows(rows, plan, h)
    assert e.dtype == F and e.shape == rows.shape
    worst = 0.0
    for b in range(2):
        ref, bound = R.reference(rows[b], h[plan.index[b]])
        err = np.abs(e[b].astype(np.float64) - ref)
        assert (err <= bound).all(), (b, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print("T=%d K=%d: worst |e - ref| / bound = %.4f" % (T, K, worst))


def test_rows_statement_for_one_sample():
    """The rule spelled out for single outputs: tap order, separate roundings, +0 outside the row, the tail cut."""
    D = sub("dataset")
    rng = np.random.default_rng(5)
    row, h = rng.uniform(-1, 1, 40).astype(F), rng.uniform(-1, 1, (1, 9)).astype(F)
    e = D.reverb_rows(row[None], _all(1), h)[0]
    for j in (0, 3, 8, 39):
        acc = F(0.0)
        for k in range(9):
            r = row[j - k] if j - k >= 0 else F(0.0)
            acc = F(acc + F(h[0, k] * r))
        assert e[j].view(np.uint32) == acc.view(np.uint32), j
    assert e.shape == (40,)


def test_rows_pass_untouched_where_the_coin_is_off():
    D = sub("dataset")
    rows = np.array([[1.0, -0.0, 2.0 ** -126, np.nan, 1e30], [0.5, -0.0, 0.0, -1.0, 2.0]], F)
    plan = D.ReverbPlan(np.array([False, True]), np.array([0, 0], np.int32))
    e = D.reverb_rows(rows, plan, np.array([[2.0, 0.0]], F))
    assert np.array_equal(e[0].view(np.uint32), rows[0].view(np.uint32))
    assert e[1].tolist() == [1.0, 0.0, 0.0, -2.0, 4.0]
    none = D.ReverbPlan(np.zeros(2, bool), np.zeros(2, np.int32))
    assert np.array_equal(D.reverb_rows(rows, none, None).view(np.uint32), rows.view(np.uint32))
    with pytest.raises(ValueError, match="rows must be"):
        D.reverb_rows(rows[:1], plan, np.ones((1, 2), F))
    with pytest.raises(ValueError, match="rirs must be"):
        D.reverb_rows(rows, plan, np.ones((1, 8193), F))


def test_the_unit_impulse_returns_the_row_but_for_the_sign_of_a_zero():
    D = sub("dataset")
    rng = np.random.default_rng(2)
    row = rng.uniform(-1, 1, 64).astype(F)
    row[[3, 17, 40]] = -0.0
    row[[5, 9]] = [2.0 ** -126, -2.0 ** -140]
    h = np.zeros((1, 8), F)
    h[0, 0] = 1.0
    e = D.reverb_rows(row[None], _all(1), h)[0]
    assert np.array_equal(e, row)                                    # equal as floats
    differ = np.nonzero(e.view(np.uint32) != row.view(np.uint32))[0]
    assert differ.tolist() == [3, 17, 40]                            # +0 + -0 = +0: the bits differ exactly at the -0.0
    assert not np.signbit(e[differ]).any()


def test_the_order_plant():
    D = sub("dataset")
    ones = np.ones((1, 8), F)
    fwd = D.reverb_rows(ones, _all(1), R.ORDER_TAPS[None])[0]
    rev = D.reverb_rows(ones, _all(1), R.ORDER_TAPS[None, ::-1])[0]
    assert fwd[2] == F(1.0) and rev[2] == F(1.0 + 2.0 ** -23)
    h = R.plant_rirs(16)
    assert D.reverb_rows(ones, _all(1, 0), h)[0, 2:].tolist() == [1.0] * 6
    assert D.reverb_rows(ones, _all(1, 1), h)[0, 2:].tolist() == [1.0 + 2.0 ** -23] * 6
    pairwise = F(F(h[0, 0] * 1 + F(h[0, 1] * 1 + h[0, 2] * 1)))
    assert pairwise != F(1.0)                                        # (the plant tells another order apart)


def test_the_fusion_plant():
    D = sub("dataset")
    a, c = R.A_PLANT, R.C_PLANT
    assert np.float64(a) * np.float64(a) == 1.0 + 2.0 ** -11 + 2.0 ** -24 and F(np.float64(a) * np.float64(a)) == F(1.0 + 2.0 ** -11)
    rows = R.plant_rows(12)[1:]
    h = R.plant_rirs(4)
    e = D.reverb_rows(rows, _all(1, 2), h)[0]
    fused = R.reverb_rows_unrounded_products(D, rows, _all(1, 2), h)[0]
    at_c = np.arange(1, 12, 2)
    assert (e[at_c] == 0.0).all() and (fused[at_c] == F(2.0 ** -24)).all()
    # ... and on random operands a fused sum has other bits in most outputs
    rng = np.random.default_rng(0)
    rows = rng.uniform(-1, 1, (2, 300)).astype(F)
    h = D.synthetic_rirs(1, 64, seed=3)
    e, fused = D.reverb_rows(rows, _all(2), h), R.reverb_rows_unrounded_products(D, rows, _all(2), h)
    differ = int(np.count_nonzero(e.view(np.uint32) != fused.view(np.uint32)))
    print("outputs a fused tap sum would round otherwise:", differ, "of", e.size)
    assert differ > e.size // 4


def test_pairwise_summation_is_not_the_rule():
    D = sub("dataset")
    rng = np.random.default_rng(1)
    row, h = rng.uniform(-1, 1, 200).astype(F), rng.uniform(-1, 1, (1, 64)).astype(F)
    e = D.reverb_rows(row[None], _all(1), h)[0]
    padded = np.concatenate([np.zeros(63, F), row])
    prod = np.stack([(h[0, k] * padded[63 - k:63 - k + 200]).astype(F) for k in range(64)])
    while prod.shape[0] > 1:
        prod = (prod[0::2] + prod[1::2]).astype(F)
    assert np.count_nonzero(prod[0] != e) > 50


# ---- the host helpers ---------------------------------------------------------------------------------------------------
def test_prepare_rirs():
    D = sub("dataset")
    rng = np.random.default_rng(4)
    raw = rng.standard_normal((3, 500)) * np.exp(-np.arange(500) / 80.0)
    raw[:, :20] *= 0.01
    raw[0, 37], raw[1, 20], raw[2, 499] = 9.0, -7.0, 8.0             # the direct paths, one of them the last tap
    for length in (64, 500, 700):
        h = D.prepare_rirs(raw, length)
        assert h.dtype == F and h.shape == (3, length)
        assert np.abs((h.astype(np.float64) ** 2).sum(1) - 1.0).max() <= 1e-6
        assert (np.abs(h).argmax(1) == 0).all()
    h = D.prepare_rirs(raw, 700)
    assert np.allclose(h[0, :463] / h[0, 0], raw[0, 37:] / 9.0, rtol=1e-6, atol=1e-7) and not h[0, 463:].any()
    assert h[2, 0] == 1.0 and not h[2, 1:].any()
    assert D.prepare_rirs(raw[0], 8).shape == (1, 8)
    for bad in (np.zeros((2, 5)), np.array([[1.0, np.nan]]), np.array([[np.inf, 1.0]])):
        with pytest.raises(ValueError, match="all zero|not finite"):
            D.prepare_rirs(bad, 4)
    for length in (0, 8193):
        with pytest.raises(ValueError, match="length"):
            D.prepare_rirs(raw, length)


def test_synthetic_rirs_are_seeded():
    D = sub("dataset")
    a, b, c = D.synthetic_rirs(4, 256, seed=7), D.synthetic_rirs(4, 256, seed=7), D.synthetic_rirs(4, 256, seed=8)
    assert a.dtype == F and a.shape == (4, 256) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.isfinite(a).all() and (np.abs(a).argmax(1) == 0).all()
    assert np.abs((a.astype(np.float64) ** 2).sum(1) - 1.0).max() <= 1e-6
    fast, slow = D.synthetic_rirs(8, 4096, rt60=(0.05, 0.05), seed=1), D.synthetic_rirs(8, 4096, rt60=(0.5, 0.5), seed=1)
    tail = lambda h: float((h[:, 1600:].astype(np.float64) ** 2).sum())
    assert tail(fast) < 1e-6 * tail(slow)                            # 0.1 s in: 120 dB down against 12 dB
    for bad in (dict(n=0), dict(rt60=(0.0, 0.1)), dict(rt60=(0.3, 0.2)), dict(rt60=0.3), dict(length=8193), dict(sample_rate=0)):
        kw = dict(n=2, length=64)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.synthetic_rirs(**kw)


# ---- the drivers --------------------------------------------------------------------------------------------------------
def test_driver_flags(tmp_path, monkeypatch):
    import argparse
    D = sub("dataset")
    made = []

    class Uploaded(D.DeviceDataset):                                 # (a real one needs a GPU)
        def __init__(self, clips, device="cuda"):
            made.append(clips)
            self.audio, self.labels, self.num_classes, self.device = SimpleNamespace(shape=clips.shape), None, 0, device

    monkeypatch.setattr(D, "DeviceDataset", Uploaded)
    p = argparse.ArgumentParser()
    D.add_augment_flags(p)
    assert D.augment_from_flags(p.parse_args([]), True) is None
    path = str(tmp_path / "rirs.npy")
    np.save(path, D.synthetic_rirs(3, 64))
    a = D.augment_from_flags(p.parse_args(["--rir", path, "--rir-prob", "0.5", "--shift", "7"]), True)
    assert a.reverberates and (len(a.reverb), a.reverb.clip_len, a.reverb_prob, a.shift) == (3, 64, 0.5, 7)
    assert made[0].dtype == F and made[0].shape == (3, 64)
    assert not D.augment_from_flags(p.parse_args(["--rir", path]), True).reverberates
    for flags in (["--rir", path], ["--rir-prob", "0.5"]):
        with pytest.raises(SystemExit, match="%s: augmentation happens where the batch is drawn on the device; add "
                                             "--device-data" % flags[0]):
            D.augment_from_flags(p.parse_args(flags), False)
    with pytest.raises(SystemExit, match="reverb_prob 0.5 without reverb"):
        D.augment_from_flags(p.parse_args(["--rir-prob", "0.5"]), True)
    with pytest.raises(SystemExit, match="reverb_prob"):
        D.augment_from_flags(p.parse_args(["--rir", path, "--rir-prob", "1.5"]), True)
    flat = str(tmp_path / "flat.npy")
    np.save(flat, np.ones(8, F))
    with pytest.raises(SystemExit, match=r"an \[M, K\] array"):
        D.augment_from_flags(p.parse_args(["--rir", flat]), True)
    for driver in ("classifier.py", "siamese.py"):
        text = open(os.path.join(ROOT, "examples", driver)).read()
        assert "add_augment_flags" in text and "--rir" in text, driver


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
    assert len(L.SIGNATURES["srwn_batch_draw_room"][1]) == len(L.SIGNATURES["srwn_batch_draw_warp"][1]) + 4
    assert len(L.SIGNATURES["srwn_pair_draw_room"][1]) == len(L.SIGNATURES["srwn_pair_draw_warp"][1]) + 4
    assert lib.srwn_version() >= 129
    B = sub("build")
    assert "srwn_room.hip" in B.SOURCES
    assert B.NO_SPILL["srwn_room.hip"] == ["batch_draw_room_kernel", "pair_draw_room_kernel"]
    assert "since srwn_version() 129" in raw
    assert int(re.search(r"#define SRWN_ROOM_MAX_TAPS (\d+)", hdr).group(1)) == D.ROOM_MAX_TAPS
    # the three augmenting units share one statement of a row's plan and of its resampling
    csrc = os.path.join(ROOT, "sr-wavenet_amd", "csrc")
    for unit in ("srwn_resample.hip", "srwn_room.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "srwn_resample.h"' in text and "warp_samples(" not in text.replace("warp_samples<", ""), unit
        assert "long kAugSpeedSalt" not in text and "0xBF58476D1CE4E5B9" not in text, unit
    room = open(os.path.join(csrc, "srwn_room.hip")).read()
    assert "%X" % D.AUG_RIR_COIN_SALT in room and "%X" % D.AUG_RIR_PICK_SALT in room
    assert "__fmul_rn" in room and "__fadd_rn" in room and "fmaf" not in room
    span = int(re.search(r"constexpr int kRoomSpan = (\d+);", room).group(1))
    assert span >= 256 and span & (span - 1) == 0 and 4096 % span == 0
    assert (span + D.ROOM_MAX_TAPS) * 4 < 48 * 1024
    assert (16000 + span - 1) // span * 8 >= 256                     # a workgroup per compute unit at the flagship shape


def _batch(lib, clips=A, labels=A, n=7, clip_len=70, state=A, B=2, T=64, shuffle=1, crop=0, rank=0, world=1, a0=A, a1=None,
           codes=None, Q=256, onehot=None, ld=16, rows=1, col0=8, classes=4, dt=0, indices=A, shift=3, gain=(0.5, 2.0),
           noise=A, nn=2, nlen=90, thr=1 << 31, vol=(0.0, 0.5), table=A, taps=16, steps=(15099494, 18454938), rir=A, rn=3,
           rlen=64, rthr=1 << 31):
    return lib.srwn_batch_draw_room(clips, labels, n, clip_len, state, B, T, shuffle, crop, rank, world, a0, a1, codes, Q,
                                    onehot, ld, rows, col0, classes, dt, indices, shift, gain[0], gain[1], noise, nn, nlen,
                                    thr, vol[0], vol[1], table, taps, steps[0], steps[1], rir, rn, rlen, rthr, None)


def _pair(lib, clips=A, labels=A, order=A, place=A, start=A, classes=4, n=9, clip_len=70, state=A, P=3, T=64, same=1 << 31,
          shuffle=1, crop=0, rank=0, world=1, audio=A, y=A, left=A, right=A, ylog=A, shift=3, gain=(0.5, 2.0), noise=A, nn=2,
          nlen=90, thr=1 << 31, vol=(0.0, 0.5), table=A, taps=16, steps=(15099494, 18454938), rir=A, rn=3, rlen=64,
          rthr=1 << 31):
    return lib.srwn_pair_draw_room(clips, labels, order, place, start, classes, n, clip_len, state, P, T, same, shuffle, crop,
                                   rank, world, audio, y, left, right, ylog, shift, gain[0], gain[1], noise, nn, nlen, thr,
                                   vol[0], vol[1], table, taps, steps[0], steps[1], rir, rn, rlen, rthr, None)


AUG_SHAPE_ERRORS = (dict(shift=64), dict(shift=-1), dict(nlen=63), dict(gain=(2.0, 1.0)), dict(gain=(-0.5, 1.0)),
                    dict(gain=(0.0, float("inf"))), dict(gain=(float("nan"), 1.0)), dict(vol=(0.5, 0.25)),
                    dict(vol=(-1.0, -0.5)), dict(vol=(0.0, float("nan"))), dict(nn=-1), dict(thr=-1),
                    dict(thr=(1 << 32) + 1), dict(noise=A + 2))
WARP_SHAPE_ERRORS = (dict(taps=0), dict(taps=1), dict(taps=15), dict(taps=66), dict(taps=-2),
                     dict(steps=(ONE + 1, ONE)), dict(steps=((1 << 23) - 1, ONE)), dict(steps=(ONE, (1 << 25) + 1)),
                     dict(steps=(0, 0)), dict(steps=(-ONE, ONE)), dict(table=A + 2))
ROOM_SHAPE_ERRORS = (dict(rn=0), dict(rn=-1), dict(rlen=0), dict(rlen=-4), dict(rlen=8193), dict(rthr=-1),
                     dict(rthr=(1 << 32) + 1), dict(rir=A + 2))
# a null table is "no resampling" only with no taps at step 2^24 on both ends
NULL_TABLE_ERRORS = (dict(table=None), dict(table=None, taps=0), dict(table=None, taps=16, steps=(ONE, ONE)),
                     dict(table=None, taps=0, steps=(ONE, ONE + 1)), dict(table=None, taps=0, steps=(ONE - 1, ONE)),
                     dict(rir=None))


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    assert _batch(lib, B=0) == 0 and _batch(lib, T=0) == 0 and _pair(lib, P=0) == 0 and _pair(lib, T=0) == 0
    for kw in (dict(clips=None), dict(state=None), dict(a0=None), dict(indices=None), dict(onehot=A, labels=None),
               dict(noise=None)) + NULL_TABLE_ERRORS:
        assert _batch(lib, **kw) == E_NULL, kw
    assert b"batch_draw_room" in lib.srwn_last_error()
    for kw in (dict(T=71), dict(n=0), dict(B=65536), dict(rank=1), dict(crop=2), dict(codes=A, Q=1),
               dict(onehot=A, ld=11), dict(onehot=A, rows=0), dict(a1=A + 2), dict(codes=A + 1)) + AUG_SHAPE_ERRORS + \
            WARP_SHAPE_ERRORS + ROOM_SHAPE_ERRORS:
        assert _batch(lib, **kw) == E_SHAPE, kw
    assert _batch(lib, onehot=A, dt=7) == E_DTYPE
    for kw in (dict(labels=None), dict(order=None), dict(place=None), dict(start=None), dict(audio=None), dict(y=None),
               dict(left=None), dict(right=None), dict(ylog=None), dict(clips=None), dict(state=None), dict(noise=None)) + \
            NULL_TABLE_ERRORS:
        assert _pair(lib, **kw) == E_NULL, kw
    assert b"pair_draw_room" in lib.srwn_last_error()
    for kw in (dict(T=71), dict(n=0), dict(P=32768), dict(rank=2, world=2), dict(crop=-1), dict(same=-1),
               dict(same=(1 << 32) + 1), dict(classes=0), dict(audio=A + 2)) + AUG_SHAPE_ERRORS + WARP_SHAPE_ERRORS + \
            ROOM_SHAPE_ERRORS:
        assert _pair(lib, **kw) == E_SHAPE, kw
    # the blocks are checked in their order: the augmentation block's error comes back in front of the room block's
    assert _batch(lib, shift=64, rn=0) == E_SHAPE and b"shift bound" in lib.srwn_last_error()
    assert _batch(lib, taps=15, rn=0) == E_SHAPE and b"15 taps" in lib.srwn_last_error()


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
    nz, rv = _bare_dataset(D, 5, 90, base=5000), _bare_dataset(D, 3, 64, base=7000)
    aug = dict(shift=6, gain=(0.5, 2.0), noise=nz, noise_prob=0.25, noise_volume=(0.1, 0.4))
    block = (6, 0.5, 2.0, 5000, 5, 90, 1 << 30, 0.1, 0.4)
    # no responses, or responses at probability 0: the three older paths, their names and their tuples
    for extra in (dict(), dict(reverb=None), dict(reverb=rv), dict(reverb=rv, reverb_prob=0.0)):
        _bare(D.BatchSampler, augment=D.Augment(**aug, **extra), **kw).draw("a0")
        assert calls.pop() == ("srwn_batch_draw_aug",) + plain + block + (77,)
        a = D.Augment(speed=(0.9, 1.1), taps=32, **aug, **extra)
        _bare(D.BatchSampler, augment=a, _resample_dev=_ptr(6000), **kw).draw("a0")
        assert calls.pop() == ("srwn_batch_draw_warp",) + plain + block + (6000, 32, 15099494, 18454938, 77)
    _bare(D.BatchSampler, **kw).draw("a0")
    assert calls.pop() == ("srwn_batch_draw",) + plain + (77,)
    # responses: the new entry; a null table exactly when the speed is (1, 1)
    room = (7000, 3, 64, 1 << 31)
    for a in (D.Augment(reverb=rv, reverb_prob=0.5, **aug), D.Augment(reverb=rv, reverb_prob=0.5, taps=8, **aug)):
        s = _bare(D.BatchSampler, augment=a, **kw)
        s.draw("a0")
        assert calls.pop() == ("srwn_batch_draw_room",) + plain + block + (None, 0, ONE, ONE) + room + (77,)
        assert s._resample_dev is None                               # nothing uploaded
    a = D.Augment(speed=(0.9, 1.1), taps=32, reverb=rv, reverb_prob=0.5, **aug)
    _bare(D.BatchSampler, augment=a, _resample_dev=_ptr(6000), **kw).draw("a0")
    assert calls.pop() == ("srwn_batch_draw_room",) + plain + block + (6000, 32, 15099494, 18454938) + room + (77,)
    assert not calls


def test_pair_sampler_dispatch(calls):
    D = sub("dataset")
    ds = _bare_dataset(D, n=9, labels=_ptr(2000), num_classes=4)
    kw = dict(dataset=ds, batch_size=3, pairs=3, num_samples=64, shuffle=False, crop="head", rank=0, world=1,
              state=_ptr(3000), indices=_ptr(4000), right=_ptr(4100), y=_ptr(4200), same_threshold=1 << 31,
              _index=(_ptr(11), _ptr(12), _ptr(13)))
    plain = (1000, 2000, 11, 12, 13, 4, 9, 70, 3000, 3, 64, 1 << 31, 0, 0, 0, 1, "audio", "labels", 4000, 4100, 4200)
    block = (6, 0.5, 2.0, None, 0, 0, 0, 0.0, 0.0)
    rv = _bare_dataset(D, 3, 64, base=7000)
    for extra in (dict(), dict(reverb=rv), dict(reverb=rv, reverb_prob=0.0)):
        _bare(D.PairSampler, augment=D.Augment(shift=6, gain=(0.5, 2.0), **extra), **kw).draw("audio", "labels")
        assert calls.pop() == ("srwn_pair_draw_aug",) + plain + block + (77,)
        a = D.Augment(shift=6, gain=(0.5, 2.0), speed=(0.5, 1.0), taps=2, **extra)
        _bare(D.PairSampler, augment=a, _resample_dev=_ptr(6000), **kw).draw("audio", "labels")
        assert calls.pop() == ("srwn_pair_draw_warp",) + plain + block + (6000, 2, 1 << 23, 1 << 24, 77)
    _bare(D.PairSampler, **kw).draw("audio", "labels")
    assert calls.pop() == ("srwn_pair_draw",) + plain + (77,)
    _bare(D.PairSampler, augment=D.Augment(shift=6, gain=(0.5, 2.0), reverb=rv, reverb_prob=1.0), **kw).draw("audio", "labels")
    assert calls.pop() == ("srwn_pair_draw_room",) + plain + block + (None, 0, ONE, ONE, 7000, 3, 64, 1 << 32, 77)
    a = D.Augment(shift=6, gain=(0.5, 2.0), speed=(0.5, 1.0), taps=2, reverb=rv, reverb_prob=1.0)
    _bare(D.PairSampler, augment=a, _resample_dev=_ptr(6000), **kw).draw("audio", "labels")
    assert calls.pop() == ("srwn_pair_draw_room",) + plain + block + (6000, 2, 1 << 23, 1 << 24, 7000, 3, 64, 1 << 32, 77)
    assert not calls


def test_evaluate_still_refuses_an_augmenting_sampler():
    D, M = sub("dataset"), sub("model")
    ds = _bare_dataset(D, n=6, labels=object(), num_classes=4)
    a = D.Augment(reverb=_bare_dataset(D, 3, 64), reverb_prob=0.5)
    plain = _bare(D.BatchSampler, dataset=ds, batch_size=3, num_samples=64, shuffle=False, world=1, augment=a)
    with pytest.raises(ValueError, match="WaveNetTeacher.evaluate: the sampler augments"):
        _bare(M.WaveNetTeacher, use_encoding=False).evaluate(plain)
    for name in ("distill_sampler", "eval_sampler", "embed_sampler"):
        with pytest.raises(TypeError, match="augment"):
            getattr(ds, name)(3, 64, augment=a)
