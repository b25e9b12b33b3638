"""GPU tests of the student's and the twins' draw and log launches (csrc/srwn_draw.hip) against their specifications in
``dataset.py``, entry by entry and with no tolerance: ``srwn_distill_draw`` against ``draw_plan`` / ``noise_plan`` and
``srwn_logistic_noise``, ``srwn_cond_scatter`` against ``copy_``, ``srwn_distill_log`` against ``StudentEngine.losses()``'s
Python arithmetic, ``srwn_pair_draw`` against ``pair_plan`` and ``srwn_pair_log``'s rings."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._pkg import sub

pytestmark = pytest.mark.gpu

SEED = 3
NC = 4
LABELS7 = np.array([0, 3, -1, 1, 2, NC, 3], np.int64)        # labels 2 and 5 lie outside the classes: zero rows
LABELS9 = np.array([0, 1, 0, 2, 1, 0, 3, 1, 0], np.int64)    # classes of 4, 3, 1 and 1 records (tests/test_draw_plans.py)
DEV = "cuda"


def _clips(n, length, seed=11):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n, length)).astype(np.float32)


def _onehot(labels, C):
    out = np.zeros((len(labels), C), np.float32)
    ok = (labels >= 0) & (labels < C)
    out[np.nonzero(ok)[0], labels[ok]] = 1.0            # tf.one_hot: out of range -> zeros
    return out


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _noise_reference(K, rows, B, T, temperature):
    """srwn_logistic_noise for the plan's row seeds at clock 0."""
    seeds = torch.as_tensor(rows.astype(np.int64), device=DEV)          # (the same 64 bits)
    temp = torch.full((B,), temperature, device=DEV)
    clock = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.full((B, T), 9.0, device=DEV)
    K.call("srwn_logistic_noise", out.data_ptr(), T, temp.data_ptr(), seeds.data_ptr(), clock.data_ptr(), B, T, K._stream())
    return out


def _from_bits(K, k):
    bits = torch.as_tensor(k.astype(np.int64), device=DEV).to(torch.int32).contiguous()
    out = torch.empty(k.shape, device=DEV)
    K.call("srwn_logistic_from_bits", bits.data_ptr(), out.data_ptr(), bits.numel(), K._stream())
    return out


# ---- srwn_distill_draw ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_distill_draw_matches_the_plans(temperature, dtype):
    D, K = sub("dataset"), sub("kernels")
    n, clip, B, T = 7, 800, 2, 768
    clips = _clips(n, clip)
    ds = D.DeviceDataset(clips, LABELS7, NC)
    s = ds.distill_sampler(B, T, seed=SEED, crop="random", temperature=temperature, log_capacity=4)
    frames, lat, Ep, F = 12, 8, 16, 2
    dst = [torch.full((B, T), 9.0, device=DEV) for _ in range(3)]
    noise = torch.full((B, T), 9.0, device=DEV)
    tables = [torch.full((B * frames, Ep), 5.0, dtype=dtype, device=DEV) for _ in range(F + 1)]
    drawn = []
    for step in range(6):
        idx, off = D.draw_plan(SEED, step, B, n, clip, T, True, "random")
        assert (s.plan()[0].tolist(), s.plan()[1].tolist()) == (idx.tolist(), off.tolist())
        k = D.noise_plan(SEED, step, B, T)
        assert np.array_equal(s.noise_plan(), k)
        s.draw(dst[0], dst[1], dst[2], noise, tables, frames, lat)
        want = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
        assert s.indices.cpu().numpy().tolist() == idx.tolist(), step
        for d in dst:
            assert np.array_equal(_bits(d), want.view(np.uint32)), step
        ref = _noise_reference(K, D.noise_rows(SEED, step, B), B, T, temperature)
        assert np.array_equal(_bits(noise), _bits(ref)), step
        unit = _from_bits(K, k)                             # the plan's k through the kernel's own map
        assert np.array_equal(_bits(noise), _bits(unit * torch.tensor(temperature, device=DEV))), step
        oh = np.repeat(_onehot(LABELS7[idx], NC)[:, None, :], frames, 1)
        for t in tables:
            c = t.float().cpu().numpy().reshape(B, frames, Ep)
            assert np.array_equal(c[:, :, lat:lat + NC], oh), step
            assert (c[:, :, :lat] == 5.0).all() and (c[:, :, lat + NC:] == 5.0).all(), "columns outside the condition block"
        drawn += idx.tolist()
        s.step += 1
        s.state[1:].fill_(s.step)                           # (the log launch ticks it in a step; no engine here)
    assert {2, 5} <= set(drawn)                             # both out-of-range labels were drawn (their rows are zero)


def test_distill_draw_without_noise_tables_and_at_temperature_zero():
    D = sub("dataset")
    clips = _clips(7, 70)
    ds = D.DeviceDataset(clips)
    audio = torch.full((3, 61), 9.0, device=DEV)
    noise = torch.full((3, 61), 9.0, device=DEV)
    s = ds.distill_sampler(3, 61, seed=SEED, shuffle=False, rank=1, world=2)
    s.draw(audio)
    idx, off = s.plan()
    assert idx.tolist() == [3, 4, 5]
    assert np.array_equal(audio.cpu().numpy(), clips[idx, :61]) and (noise == 9.0).all()
    s = ds.distill_sampler(3, 61, seed=SEED, temperature=0.0)
    s.draw(audio, noise=noise)
    assert np.array_equal(_bits(noise), np.zeros((3, 61), np.uint32))      # +0, srwn_logistic_noise's rule


def test_distill_draw_rows_longer_than_a_workgroups_share():
    """Rows of 8197 samples are three workgroups each (4096 + 4096 + 5): the shares' own heads and tails, at offsets that
    leave source and destination aligned differently; the noise of a row runs across the shares."""
    D, K = sub("dataset"), sub("kernels")
    n, clip, T, B = 3, 9001, 8197, 2
    clips = _clips(n, clip, seed=4)
    s = D.DeviceDataset(clips).distill_sampler(B, T, seed=SEED, crop="random", temperature=0.7)
    dst = [torch.full((B, T), 9.0, device=DEV) for _ in range(3)]
    noise = torch.full((B, T), 9.0, device=DEV)
    for step in range(3):
        idx, off = s.plan()
        s.draw(dst[0], dst[1], dst[2], noise)
        want = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
        assert s.indices.cpu().numpy().tolist() == idx.tolist()
        for d in dst:
            assert np.array_equal(_bits(d), want.view(np.uint32)), step
        assert np.array_equal(_bits(noise), _bits(_noise_reference(K, s.noise_rows(), B, T, 0.7))), step
        s.step += 1
        s.state[1:].fill_(s.step)


# ---- srwn_cond_scatter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cond_scatter_is_copy(dtype):
    D = sub("dataset")
    rows, lat, Ep = 24, 8, 16
    s = D.DeviceDataset(_clips(2, 70)).distill_sampler(1, 64)
    rng = np.random.default_rng(2)
    e = rng.standard_normal((rows, lat)).astype(np.float32)
    # ties of the bf16 rounding, both ways, a value that rounds up into the next binade, tiny values and zeros of both signs
    e[0, :6] = np.array([0x3F808000, 0x3F818000, 0x3FFF8000, 0xBF808000, 0x00000001, 0x80000000], np.uint32).view(np.float32)
    enc = torch.as_tensor(e, device=DEV)
    tables = [torch.full((rows, Ep), 5.0, dtype=dtype, device=DEV) for _ in range(3)]
    want = torch.full((rows, Ep), 5.0, dtype=dtype, device=DEV)
    want[:, :lat].copy_(enc)
    s.scatter(enc, tables)
    for t in tables:
        assert torch.equal(t.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
        assert (t[:, lat:].float() == 5.0).all()


# ---- srwn_distill_log ----------------------------------------------------------------------------------------------------
def test_distill_log_is_the_host_arithmetic():
    """Hand-set scalars, among them values at which beta * ce - alpha * entropy with a product kept unrounded (a fused
    multiply-add) rounds differently from two rounded products (tests/test_draw_plans.py checks that they do); the ring of
    4 wraps and the counter ticks."""
    from tests.test_draw_plans import LOG_COEF, distill_log_cases, distill_log_host
    D = sub("dataset")
    s = D.DeviceDataset(_clips(2, 70)).distill_sampler(1, 64, seed=SEED, log_capacity=4)
    alpha, beta, N = LOG_COEF
    cases = distill_log_cases()
    eng = SimpleNamespace(ce=torch.zeros(1, device=DEV), power=torch.zeros(1, device=DEV), logs=torch.zeros(1, device=DEV),
                          alpha=alpha, beta=beta, N=N, loss_div=1.0)
    got, want = [], []
    for i, c in enumerate(cases):
        eng.ce.fill_(float(c[0])); eng.power.fill_(float(c[1])); eng.logs.fill_(float(c[2]))
        eng.loss_div = c[3]
        s.log_engine(eng)
        s.step += 1
        got.append((s.losses(i, 1)[0], s.power_losses(i, 1)[0], s.entropies(i, 1)[0]))
        want.append(distill_log_host(*c))
    got, want = np.array(got, np.float32), np.array(want, np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert s.state.cpu().tolist() == [SEED, len(cases)]
    last = len(cases) - 4                                   # the ring holds the last four steps
    assert np.array_equal(s.losses(last, 4).view(np.uint32), want[last:, 0].view(np.uint32))
    assert np.array_equal(s.entropies(last, 4).view(np.uint32), want[last:, 2].view(np.uint32))
    with pytest.raises(ValueError, match="ring holds 4"):
        s.entropies(0, 5)


# ---- srwn_pair_draw / srwn_pair_log --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(crop="head"), dict(crop="random"), dict(crop="random", rank=1, world=2)],
                         ids=["head", "random", "rank1of2"])
@pytest.mark.parametrize("T", [70, 61])
def test_pair_draw_matches_the_plan(T, kw):
    D = sub("dataset")
    n, clip, P = 9, 70, 3
    clips = _clips(n, clip)
    ds = D.DeviceDataset(clips, LABELS9, NC)
    s = ds.pair_sampler(P, T, seed=SEED, log_capacity=4, **kw)
    audio = torch.full((2 * P, T), 9.0, device=DEV)
    y = torch.full((P,), 9.0, device=DEV)
    loss = torch.zeros(1, device=DEV)
    dist = torch.zeros(P, device=DEV)
    ys = []
    for step in range(8):
        left, right, ol, orr, yy = D.pair_plan(SEED, step, P, LABELS9, NC, clip, T, 0.5, True, kw["crop"],
                                               kw.get("rank", 0), kw.get("world", 1))
        got = s.pair_plan()
        assert all(a.tolist() == b.tolist() for a, b in zip(got, (left, right, ol, orr, yy)))
        s.draw(audio, y)
        want = np.stack([clips[i, o:o + T] for i, o in zip(np.concatenate([left, right]), np.concatenate([ol, orr]))])
        assert s.indices.cpu().numpy().tolist() == left.tolist() and s.right.cpu().numpy().tolist() == right.tolist(), step
        assert np.array_equal(_bits(audio), want.view(np.uint32)), step
        assert np.array_equal(y.cpu().numpy(), yy) and np.array_equal(s.y.cpu().numpy(), yy), step
        loss.fill_(step + 0.5)
        dist.copy_(torch.arange(P, device=DEV) + 10.0 * step)
        s.log_engine(SimpleNamespace(loss=loss, dist=dist))
        s.step += 1
        ys += yy.tolist()
    assert 0.0 in ys and 1.0 in ys
    # the rings of 4 hold steps 4, 5, 6, 7; the device counter stands at 8
    assert s.state.cpu().tolist() == [SEED, 8]
    assert s.losses(4, 4).tolist() == [4.5, 5.5, 6.5, 7.5]
    assert s.distances(4, 4).tolist() == [[10.0 * st + i for i in range(P)] for st in range(4, 8)]


def test_pair_draw_rows_longer_than_a_workgroups_share():
    D = sub("dataset")
    n, clip, T, P = 4, 9001, 8197, 2
    clips = _clips(n, clip, seed=4)
    labels = np.array([0, 1, 0, 1])
    s = D.DeviceDataset(clips, labels, 2).pair_sampler(P, T, seed=SEED, crop="random")
    audio = torch.full((2 * P, T), 9.0, device=DEV)
    y = torch.zeros(P, device=DEV)
    left, right, ol, orr, yy = s.pair_plan()
    s.draw(audio, y)
    want = np.stack([clips[i, o:o + T] for i, o in zip(np.concatenate([left, right]), np.concatenate([ol, orr]))])
    assert np.array_equal(_bits(audio), want.view(np.uint32))
    assert np.array_equal(y.cpu().numpy(), yy)


def test_pair_sampler_refuses_labels_outside_the_classes():
    D = sub("dataset")
    ds = D.DeviceDataset(_clips(7, 70), LABELS7, NC)
    with pytest.raises(ValueError, match=r"inside \[0, 4\)"):
        ds.pair_sampler(3, 64)
