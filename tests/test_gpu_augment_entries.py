"""GPU tests of ``srwn_batch_draw_aug`` and ``srwn_pair_draw_aug`` on their own: every output of a draw against
``dataset.augment_rows`` over ``dataset.draw_plan`` / ``pair_plan`` and ``augment_plan``, bit for bit and without a tolerance
-- both audio buffers as ``uint32`` (so the sign of a zero counts), the codes, the one-hot rows in fp32 and bf16 at a
non-zero column, the indices.

Shapes: B = 3; T = 5 (shorter than one 16-byte vector) and T = 4099 (two workgroups per row, the second a ragged tail of
3); clips of T + 37 samples cropped at random and clips of T samples cropped at the head; shift bounds 0, 1 and T - 1;
no noise, noise clips of T samples (one window) and of T + 13 samples at noise_prob 0.5 (mixed and unmixed rows in one
launch).  SEED was searched on the CPU with ``augment_plan``: it is the first seed whose first six steps (18 positions)
hold both extreme shifts -(T - 1) and T - 1 for T = 5 and for T = 4099; ``test_the_seed_reaches_both_extremes`` says so.

A third of every clip is planted: 1, -1, the next float beyond each, -0.0 and 2^-126, whose product with a gain below one
is subnormal (the kernel must keep it, as NumPy does).  ``test_no_fused_multiply_add`` plants operands whose fused
multiply-add has other bits than the three separately rounded operations, in either order of contraction."""
import numpy as np
import pytest
import torch

from tests._pkg import sub

pytestmark = pytest.mark.gpu

SEED = 179349
B, N, NC, STEPS = 3, 7, 4, 6
LABELS = np.array([0, 3, -1, 1, 2, NC, 3], np.int64)       # labels 2 and 5 lie outside the classes
LABELS9 = np.array([0, 1, 0, 2, 1, 0, 3, 1, 0], np.int64)
F = np.float32
UP, DOWN = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
SPECIALS = np.array([1.0, -1.0, UP, DOWN, -0.0, 2.0 ** -126, -2.0 ** -126, 0.0], F)


def _clips(n, length, seed=11):
    """Random samples in [-1.2, 1.2]; every third one is a planted special, another one in every clip."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.2, 1.2, (n, length)).astype(F)
    j = np.arange(0, length, 3)
    for r in range(n):
        x[r, j] = SPECIALS[(j // 3 + r) % len(SPECIALS)]
    return x


def _onehot(labels, C):
    out = np.zeros((len(labels), C), F)
    ok = (labels >= 0) & (labels < C)
    out[np.nonzero(ok)[0], labels[ok]] = 1.0
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _augment(D, T, shift, noise):
    """(the Augment, the noise clips on the host or None)."""
    if noise == "none":
        return D.Augment(shift=shift, gain=(0.5, 0.96875)), None
    length, prob = (T, 1.0) if noise == "window" else (T + 13, 0.5)
    nz = _clips(4, length, seed=23)
    return D.Augment(shift=shift, gain=(0.5, 2.0), noise=D.DeviceDataset(nz), noise_prob=prob,
                     noise_volume=(0.125, 0.75)), nz


def test_the_seed_reaches_both_extremes():
    D = sub("dataset")
    for T in (5, 4099):
        sh = np.concatenate([D.augment_plan(SEED, st, B, T, D.Augment(shift=T - 1), 0, 0).shift for st in range(STEPS)])
        assert sh.min() == -(T - 1) and sh.max() == T - 1, T


@pytest.mark.parametrize("noise", ["none", "window", "longer"])
@pytest.mark.parametrize("bound", ["0", "1", "T-1"])
@pytest.mark.parametrize("crop", ["random", "head"])
@pytest.mark.parametrize("T", [5, 4099])
def test_batch_draw_aug_matches_the_restatement(T, crop, bound, noise):
    D, K = sub("dataset"), sub("kernels")
    clip_len = T + 37 if crop == "random" else T
    shift = {"0": 0, "1": 1, "T-1": T - 1}[bound]
    clips = _clips(N, clip_len)
    aug, nz = _augment(D, T, shift, noise)
    s = D.DeviceDataset(clips, LABELS, NC).sampler(B, T, seed=SEED, crop=crop, augment=aug)
    dev, frames, col0, ld = "cuda", 2, 8, 16
    audio = torch.full((B, T), 9.0, device=dev)
    audio2 = torch.full((B, T), 9.0, device=dev)
    codes = torch.full((B * T,), -7, dtype=torch.int32, device=dev)
    onehot = torch.full((B, col0 + NC + 1), 9.0, device=dev)
    cond = torch.full((B * frames, ld), 5.0, dtype=torch.bfloat16, device=dev)
    loss = torch.zeros(1, device=dev)
    shifts, mixed, subnormal, clamped = [], [], 0, 0
    for step in range(STEPS):
        idx, off = D.draw_plan(SEED, step, B, N, clip_len, T, True, crop)
        plan = s.augment_plan()
        want = D.augment_rows(np.stack([clips[i, o:o + T] for i, o in zip(idx, off)]), plan, nz)
        s.draw(audio, audio2, codes, 256, onehot, 1, col0)
        s.draw(audio, onehot=cond, onehot_rows=frames, onehot_col0=col0)
        s.log_step(loss)
        s.step += 1
        got = audio.cpu().numpy()
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, (step, bad[:4].tolist(), [(got[b, j], want[b, j]) for b, j in bad[:4]], plan)
        assert torch.equal(audio2.view(torch.int32), audio.view(torch.int32)), step
        assert torch.equal(codes.view(B, T), K.mu_law_encode(torch.as_tensor(want, device=dev), 256)), step
        assert s.indices.cpu().numpy().tolist() == idx.tolist(), step
        oh = _onehot(LABELS[idx], NC)
        o = onehot.cpu().numpy()
        assert np.array_equal(o[:, col0:col0 + NC], oh) and (o[:, :col0] == 9.0).all() and (o[:, col0 + NC:] == 9.0).all()
        c = cond.float().cpu().numpy().reshape(B, frames, ld)
        assert np.array_equal(c[:, :, col0:col0 + NC], np.repeat(oh[:, None, :], frames, 1)), step
        assert (c[:, :, :col0] == 5.0).all() and (c[:, :, col0 + NC:] == 5.0).all()
        shifts += plan.shift.tolist()
        mixed += plan.mix.tolist()
        subnormal += int(np.count_nonzero((want != 0) & (np.abs(want) < F(2.0 ** -126))))
        clamped += int(np.count_nonzero(np.abs(want) == 1.0))
    # what the case is there for did occur (all of it decided on the CPU, from the plans and the restatement)
    assert min(shifts) == -shift and max(shifts) == shift
    assert set(mixed) == {"none": {False}, "window": {True}, "longer": {False, True}}[noise]
    if noise == "none":
        assert subnormal > 0               # 2^-126 times a gain below one
    if noise != "none" or T > 5:
        assert clamped > 0                 # (gains up to 2; or enough samples beyond +-1 / 0.97)
    assert s.state.cpu().tolist() == [SEED, STEPS]


@pytest.mark.parametrize("T", [5, 4099])
def test_defaults_change_only_the_sign_of_a_zero(T):
    """``Augment()``: shift 0, gain 1, no noise -- the plain draw's values, with -0.0 drawn as +0.0 (the sum is formed)."""
    D = sub("dataset")
    clips = _clips(N, T + 37)
    ds = D.DeviceDataset(clips)
    plain, aug = torch.zeros((B, T), device="cuda"), torch.zeros((B, T), device="cuda")
    ds.sampler(B, T, seed=SEED, crop="random").draw(plain)
    ds.sampler(B, T, seed=SEED, crop="random", augment=D.Augment()).draw(aug)
    p, a = plain.cpu().numpy(), aug.cpu().numpy()
    assert np.array_equal(np.clip(p, -1, 1), a)
    assert np.signbit(p[p == 0]).any() and not np.signbit(a[a == 0]).any()


@pytest.mark.parametrize("T", [5, 4099])
def test_no_fused_multiply_add(T):
    """gain = volume = g = 1 + 2^-12.  Even samples: x = g, n = -1, so g * x = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11, g * n
    = -(1 + 2^-12) is exact and the sum is 2^-12, where fma(g, x, g * n) keeps the 2^-24.  Odd samples: x = -1, n = g, the
    same with the roles swapped, for a compiler that contracts the other product.  Both asserted here in exact arithmetic
    before the kernel runs."""
    D = sub("dataset")
    g = F(1 + 2.0 ** -12)
    x = np.where(np.arange(T) % 2 == 0, g, F(-1)).astype(F)
    n = np.where(np.arange(T) % 2 == 0, F(-1), g).astype(F)
    two_step = (g * x).astype(F) + (g * n).astype(F)
    fused_x = (np.float64(g) * x.astype(np.float64) + (g * n).astype(F).astype(np.float64)).astype(F)    # (exact in fp64)
    fused_n = (np.float64(g) * n.astype(np.float64) + (g * x).astype(F).astype(np.float64)).astype(F)
    assert (two_step[0::2] != fused_x[0::2]).all() and (two_step[1::2] != fused_n[1::2]).all()
    assert (two_step == F(2.0 ** -12)).all() and (fused_x[0::2] == F(2.0 ** -12 + 2.0 ** -24)).all()
    assert (fused_n[1::2] == F(2.0 ** -12 + 2.0 ** -24)).all()
    aug = D.Augment(gain=(float(g), float(g)), noise=D.DeviceDataset(np.stack([n, n])), noise_prob=1.0,
                    noise_volume=(float(g), float(g)))
    s = D.DeviceDataset(np.stack([x] * N)).sampler(B, T, seed=SEED, augment=aug)
    plan = s.augment_plan()
    assert (plan.gain == g).all() and (plan.volume == g).all() and plan.mix.all() and not plan.noise_offset.any()
    audio = torch.zeros((B, T), device="cuda")
    s.draw(audio)
    got = audio.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(np.stack([two_step] * B))), (got[0, :4], two_step[:4], fused_x[:4], fused_n[:4])


@pytest.mark.parametrize("T", [5, 4099])
def test_pair_draw_aug_matches_the_restatement(T):
    D = sub("dataset")
    P, clip_len = 3, T + 37
    clips = _clips(9, clip_len)
    aug, nz = _augment(D, T, T - 1, "longer")
    s = D.DeviceDataset(clips, LABELS9, NC).pair_sampler(P, T, seed=SEED, crop="random", augment=aug)
    audio = torch.full((2 * P, T), 9.0, device="cuda")
    y = torch.full((P,), 9.0, device="cuda")
    loss, dist = torch.zeros(1, device="cuda"), torch.zeros(P, device="cuda")
    mixed = []
    for step in range(STEPS):
        left, right, ol, orr, want_y = D.pair_plan(SEED, step, P, LABELS9, NC, clip_len, T, 0.5, True, "random")
        pl, pr = s.augment_plan()
        assert not all(np.array_equal(a, b) for a, b in zip(pl, pr))
        want = np.concatenate([D.augment_rows(np.stack([clips[i, o:o + T] for i, o in zip(left, ol)]), pl, nz),
                               D.augment_rows(np.stack([clips[i, o:o + T] for i, o in zip(right, orr)]), pr, nz)])
        s.draw(audio, y)
        s.log_pairs(loss, dist)
        s.step += 1
        got = audio.cpu().numpy()
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, (step, bad[:4].tolist(), pl, pr)
        assert y.cpu().tolist() == want_y.tolist() == s.y.cpu().tolist()
        assert s.indices.cpu().tolist() == left.tolist() and s.right.cpu().tolist() == right.tolist()
        mixed += pl.mix.tolist() + pr.mix.tolist()
    assert set(mixed) == {False, True}


def test_pair_draw_aug_two_views_of_one_record():
    """A one-record set: left and right are that record at the same crop, and the two sides' augmentations differ."""
    D = sub("dataset")
    T, P = 4099, 3
    clips = _clips(1, T)
    aug = D.Augment(shift=T - 1, gain=(0.5, 2.0))
    s = D.DeviceDataset(clips, np.array([0]), 1).pair_sampler(P, T, seed=SEED, augment=aug)
    audio = torch.full((2 * P, T), 9.0, device="cuda")
    y = torch.zeros(P, device="cuda")
    pl, pr = s.augment_plan()
    s.draw(audio, y)
    rows = np.repeat(clips, P, 0)
    want = np.concatenate([D.augment_rows(rows, pl), D.augment_rows(rows, pr)])
    got = audio.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert s.indices.cpu().tolist() == s.right.cpu().tolist() == [0] * P and y.cpu().tolist() == [1.0] * P
    for b in range(P):
        assert not np.array_equal(got[b], got[P + b]), b
