"""GPU tests of ``srwn_batch_draw_warp`` and ``srwn_pair_draw_warp`` on their own: every output of a draw against
``augment_rows(resample_rows(...))`` over ``draw_plan`` / ``pair_plan``, ``speed_plan`` and ``augment_plan``, bit for bit
and without a tolerance -- both audio buffers as ``uint32`` (so the sign of a zero counts), the codes, the one-hot rows in
fp32 and bf16 at a non-zero column, the indices; for pairs the audio, y, left and right.

Shapes: B = 3; T = 5 with 2, 16 and 64 taps (every tap window is cut by both ends of the row) and T = 4099 with 16 taps
(two workgroups per row, the second a ragged tail of 3, heads and tails unaligned in rows 1 and 2); clips of T + 37 samples
cropped at random.  Before every step the records are rewritten so that every sample outside the step's crop windows is the
sentinel 1e30: a tap that reads past its row -- into the record's neighbouring samples -- gives a huge sum that the clamp
turns into +-1, which the comparison sees.  Speeds: 0.5 and 2.0 (the ends of the range), 0.9 .. 1.1 (a step per row), 1.0
sent through the entry (the samplers would draw it through ``_aug``), and the one step 2^24 + 2^12, whose phase is j mod
4096 at output j -- T = 4099 visits every row of the table.  Shift bounds 0, 1 and T - 1 (SEED reaches both extremes within
the six steps, as tests/test_gpu_augment_entries.py says and checks), gains 0.5 .. 2, noise clips of T + 13 samples mixed
into every row.  The three destinations are also placed 0, 4 and 8 bytes behind a 16-byte boundary, so that each is written
in a pass of its own.

A third of every clip is planted: 1, -1, the next float beyond each, -0.0 and +-2^-126, whose products with a tap below one
are subnormal.  That the operands tell a fused multiply-add from the two separately rounded operations is shown on the CPU
(tests/resample_design.py: the tap sum with unrounded products differs from the rule's in thousands of outputs)."""
import numpy as np
import pytest
import torch

from tests import resample_design as R
from tests._pkg import sub

pytestmark = pytest.mark.gpu

SEED = 179349
B, N, NC, STEPS = 3, 7, 4, 6
LABELS = np.array([0, 3, -1, 1, 2, NC, 3], np.int64)       # labels 2 and 5 lie outside the classes
LABELS9 = np.array([0, 1, 0, 2, 1, 0, 3, 1, 0], np.int64)
F = np.float32
UP, DOWN = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
SPECIALS = np.array([1.0, -1.0, UP, DOWN, -0.0, 2.0 ** -126, -2.0 ** -126, 0.0], F)
SENTINEL = F(1e30)
PHASE_STEP = 1.0 + 1.0 / 4096            # 2^24 + 2^12 as a speed
SPEEDS = {"half": (0.5, 0.5), "double": (2.0, 2.0), "range": (0.9, 1.1), "one": (1.0, 1.0), "phases": (PHASE_STEP, PHASE_STEP)}


def _clips(n, length, seed=11):
    """Random samples in [-1.2, 1.2]; every third one is a planted special, another one in every clip."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.2, 1.2, (n, length)).astype(F)
    j = np.arange(0, length, 3)
    for r in range(n):
        x[r, j] = SPECIALS[(j // 3 + r) % len(SPECIALS)]
    return x


def _fenced(clips, windows, T):
    """`clips` with the sentinel on every sample outside the (record, offset) windows of T samples."""
    inside = np.zeros(clips.shape, bool)
    for rec, off in windows:
        inside[rec, off:off + T] = True
    return np.where(inside, clips, SENTINEL).astype(F)


def _onehot(labels, C):
    out = np.zeros((len(labels), C), F)
    ok = (labels >= 0) & (labels < C)
    out[np.nonzero(ok)[0], labels[ok]] = 1.0
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _augment(D, T, shift, speed, taps, prob=1.0):
    nz = _clips(4, T + 13, seed=23)
    return D.Augment(shift=shift, gain=(0.5, 2.0), noise=D.DeviceDataset(nz), noise_prob=prob, noise_volume=(0.125, 0.75),
                     speed=SPEEDS[speed], taps=taps), nz


def test_the_cases_are_what_they_say():
    """Decided on the CPU: the seed's shifts, the phase step, and operands that a fused multiply-add would round otherwise."""
    D = sub("dataset")
    assert D.RESAMPLE_PHASES == 4096
    a = D.Augment(speed=SPEEDS["phases"])
    assert a.step_lo == a.step_hi == (1 << 24) + (1 << 12)
    q = np.arange(4099, dtype=np.uint64) * np.uint64(a.step_lo)
    assert sorted(set(((q >> np.uint64(12)) & np.uint64(4095)).tolist())) == list(range(4096))
    for T in (5, 4099):
        sh = np.concatenate([D.augment_plan(SEED, st, B, T, D.Augment(shift=T - 1), 0, 0).shift for st in range(STEPS)])
        assert sh.min() == -(T - 1) and sh.max() == T - 1, T
    steps = np.concatenate([D.speed_plan(SEED, st, B, D.Augment(speed=SPEEDS["range"])) for st in range(STEPS)])
    assert len(set(steps.tolist())) == B * STEPS and steps.min() < 1 << 24 < steps.max()
    rows = _clips(B, 4099)
    for speed in ("half", "double", "range", "phases"):
        a = D.Augment(speed=SPEEDS[speed])
        st = D.speed_plan(SEED, 0, B, a)
        two_step = D.resample_rows(rows, st, a.table())
        fused = R.resample_rows_unrounded_products(D, rows, st, a.table())
        differ = int(np.count_nonzero(_bits(two_step) != _bits(fused)))
        print(speed, "outputs a fused tap sum would round otherwise:", differ, "of", two_step.size)
        assert differ > 1000, speed


@pytest.mark.parametrize("speed", sorted(SPEEDS))
@pytest.mark.parametrize("T,taps", [(5, 2), (5, 16), (5, 64), (4099, 16)])
def test_batch_draw_warp_matches_the_restatement(T, taps, speed, monkeypatch):
    D, K = sub("dataset"), sub("kernels")
    if speed == "one":
        monkeypatch.setattr(D.Augment, "resamples", True)          # through the entry, not through _aug
    clip_len = T + 37
    clips = _clips(N, clip_len)
    dev, frames, col0, ld = "cuda", 2, 8, 16
    audio = torch.full((B, T), 9.0, device=dev)
    audio2 = torch.full((B, T), 9.0, device=dev)
    codes = torch.full((B * T,), -7, dtype=torch.int32, device=dev)
    onehot = torch.full((B, col0 + NC + 1), 9.0, device=dev)
    cond = torch.full((B * frames, ld), 5.0, dtype=torch.bfloat16, device=dev)
    loss = torch.zeros(1, device=dev)
    for shift in (0, 1, T - 1):
        aug, nz = _augment(D, T, shift, speed, taps)
        ds = D.DeviceDataset(clips, LABELS, NC)
        s = ds.sampler(B, T, seed=SEED, crop="random", augment=aug)
        table = aug.table()
        assert table.shape == (4096, taps)
        shifts, steps_seen = [], []
        for step in range(STEPS):
            idx, off = D.draw_plan(SEED, step, B, N, clip_len, T, True, "random")
            fenced = _fenced(clips, zip(idx, off), T)
            ds.audio.copy_(torch.from_numpy(fenced))
            plan, steps = s.augment_plan(), s.speed_plan()
            assert plan.mix.all()
            want = R.warp_rows(D, np.stack([fenced[i, o:o + T] for i, o in zip(idx, off)]), steps, table, plan, nz)
            s.draw(audio, audio2, codes, 256, onehot, 1, col0)
            s.draw(audio, onehot=cond, onehot_rows=frames, onehot_col0=col0)
            s.log_step(loss)
            s.step += 1
            got = audio.cpu().numpy()
            bad = np.argwhere(_bits(got) != _bits(want))
            assert bad.size == 0, (shift, step, bad[:4].tolist(), [(got[b, j], want[b, j]) for b, j in bad[:4]], plan, steps)
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
            steps_seen += steps.tolist()
        assert min(shifts) == -shift and max(shifts) == shift
        assert min(steps_seen) >= aug.step_lo and max(steps_seen) <= aug.step_hi
        assert s.state.cpu().tolist() == [SEED, STEPS]


@pytest.mark.parametrize("T", [5, 4099])
def test_destinations_at_different_positions_against_the_16_byte_boundaries(T):
    """audio starts on a 16-byte boundary, the second buffer 4 bytes and the codes 8 bytes behind one: the kernel writes
    destinations that share the position in one pass and every other one in a pass of its own, each with its own head,
    body and tail.  The elements around the three buffers keep their fill."""
    D, K = sub("dataset"), sub("kernels")
    clips = _clips(N, T + 37)
    aug, nz = _augment(D, T, T - 1, "range", 16)
    s = D.DeviceDataset(clips, LABELS, NC).sampler(B, T, seed=SEED, crop="random", augment=aug)
    n = B * T
    big_a = torch.full((n + 8,), 9.0, device="cuda")
    big_b = torch.full((n + 8,), 9.0, device="cuda")
    big_c = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")
    audio, audio2, codes = big_a[4:4 + n].view(B, T), big_b[1:1 + n].view(B, T), big_c[2:2 + n]
    assert [t.data_ptr() % 16 for t in (audio, audio2, codes)] == [0, 4, 8]
    for step in range(2):
        idx, off = D.draw_plan(SEED, step, B, N, T + 37, T, True, "random")
        want = R.warp_rows(D, np.stack([clips[i, o:o + T] for i, o in zip(idx, off)]), s.speed_plan(), aug.table(),
                           s.augment_plan(), nz)
        s.draw(audio, audio2, codes, 256)
        s.step += 1
        s.state[1:].fill_(s.step)
        assert np.array_equal(_bits(audio.cpu().numpy()), _bits(want)), step
        assert torch.equal(audio2.view(torch.int32), audio.view(torch.int32)), step
        assert torch.equal(codes.view(B, T), K.mu_law_encode(torch.as_tensor(want, device="cuda"), 256)), step
    assert (big_a[:4] == 9.0).all() and (big_a[4 + n:] == 9.0).all() and big_b[0] == 9.0 and (big_b[1 + n:] == 9.0).all()
    assert (big_c[:2] == -7).all() and (big_c[2 + n:] == -7).all()


@pytest.mark.parametrize("T", [5, 4099])
def test_speed_one_through_the_entry_is_the_aug_draw(T, monkeypatch):
    """Step 2^24 reads phase 0, the unit impulse: the ``_warp`` entry's rows are the ``_aug`` entry's, bit for bit."""
    D = sub("dataset")
    clips = _clips(N, T + 37)
    aug, _ = _augment(D, T, T - 1, "one", 16)
    ds = D.DeviceDataset(clips)
    a, b = torch.zeros((B, T), device="cuda"), torch.zeros((B, T), device="cuda")
    ds.sampler(B, T, seed=SEED, crop="random", augment=aug).draw(a)
    monkeypatch.setattr(D.Augment, "resamples", True)
    ds.sampler(B, T, seed=SEED, crop="random", augment=aug).draw(b)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("T,taps", [(5, 2), (5, 64), (4099, 16)])
def test_pair_draw_warp_matches_the_restatement(T, taps):
    D = sub("dataset")
    P, clip_len = 3, T + 37
    clips = _clips(9, clip_len)
    aug, nz = _augment(D, T, T - 1, "range", taps, prob=0.5)
    ds = D.DeviceDataset(clips, LABELS9, NC)
    s = ds.pair_sampler(P, T, seed=SEED, crop="random", augment=aug)
    table = aug.table()
    audio = torch.full((2 * P, T), 9.0, device="cuda")
    y = torch.full((P,), 9.0, device="cuda")
    loss, dist = torch.zeros(1, device="cuda"), torch.zeros(P, device="cuda")
    mixed = []
    for step in range(STEPS):
        left, right, ol, orr, want_y = D.pair_plan(SEED, step, P, LABELS9, NC, clip_len, T, 0.5, True, "random")
        fenced = _fenced(clips, list(zip(left, ol)) + list(zip(right, orr)), T)
        ds.audio.copy_(torch.from_numpy(fenced))
        pl, pr = s.augment_plan()
        sl, sr = s.speed_plan()
        assert not np.array_equal(sl, sr)
        want = np.concatenate([
            R.warp_rows(D, np.stack([fenced[i, o:o + T] for i, o in zip(left, ol)]), sl, table, pl, nz),
            R.warp_rows(D, np.stack([fenced[i, o:o + T] for i, o in zip(right, orr)]), sr, table, pr, nz)])
        s.draw(audio, y)
        s.log_pairs(loss, dist)
        s.step += 1
        got = audio.cpu().numpy()
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, (step, bad[:4].tolist(), pl, pr, sl, sr)
        assert y.cpu().tolist() == want_y.tolist() == s.y.cpu().tolist()
        assert s.indices.cpu().tolist() == left.tolist() and s.right.cpu().tolist() == right.tolist()
        mixed += pl.mix.tolist() + pr.mix.tolist()
    assert set(mixed) == {False, True}


def test_pair_draw_warp_two_views_of_one_record():
    """A one-record set: left and right are that record at the same crop; nothing but the speed is drawn, and the two
    sides' steps differ, so the two views do."""
    D = sub("dataset")
    T, P = 4099, 3
    clips = _clips(1, T)
    aug = D.Augment(speed=(0.9, 1.1))
    s = D.DeviceDataset(clips, np.array([0]), 1).pair_sampler(P, T, seed=SEED, augment=aug)
    audio = torch.full((2 * P, T), 9.0, device="cuda")
    y = torch.zeros(P, device="cuda")
    pl, pr = s.augment_plan()
    sl, sr = s.speed_plan()
    assert all(a != b for a, b in zip(sl.tolist(), sr.tolist()))
    assert all(np.array_equal(a, b) for a, b in zip(pl, pr))               # shift 0, gain 1, no noise on both sides
    s.draw(audio, y)
    rows = np.repeat(clips, P, 0)
    want = np.concatenate([R.warp_rows(D, rows, sl, aug.table(), pl), R.warp_rows(D, rows, sr, aug.table(), pr)])
    got = audio.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert s.indices.cpu().tolist() == s.right.cpu().tolist() == [0] * P and y.cpu().tolist() == [1.0] * P
    for b in range(P):
        assert not np.array_equal(got[b], got[P + b]), b
