"""GPU tests of ``srwn_batch_draw_room`` and ``srwn_pair_draw_room`` on their own: every output of a draw against
``augment_rows(reverb_rows(resample_rows(...)))`` over ``draw_plan`` / ``pair_plan``, ``speed_plan``, ``reverb_plan`` and
``augment_plan``, bit for bit and without a tolerance -- both audio buffers as ``uint32`` (so the sign of a zero counts),
the codes, the one-hot rows, the indices; for pairs the audio, y, left and right.

Shapes: B = 3, clips of T + 37 samples cropped at random.  T = 5 with K = 1, 2 and 7 taps (at K = 7 > T every window is
cut by the row's start); T = 4099 with K = 64 and K = 8192 (for any span that is a power of two between 256 and 4096 there
are several workgroups per row, the last a ragged tail of 3, and at K = 8192 the halo is longer than a span and than the
row) and T = 4099 with K = 4096 under resampling through 16 taps.  Speeds: none (a null table), 0.9 .. 1.1, 0.5, 2.0.
Shift bounds 0, 1 and T - 1, gains 0.5 .. 2, noise mixed into every row.  ``reverb_prob`` 1.0 reverberates every row; at
0.5 SEED and the step count make both kinds of row occur (checked on the CPU below), and the rows whose coin is off also
equal what ``srwn_batch_draw_warp`` / ``srwn_batch_draw_aug`` write on the device from the same state.

Operands: the planted clips of tests/test_gpu_resample_entries.py (+-1, the next floats beyond, -0.0, +-2^-126) under
responses whose taps lie below one, so products are subnormal; the order plant and the fusion plant of
tests/room_design.py in a test of their own; before every step the records are rewritten so that every sample outside the
step's crop windows is the sentinel 1e30, and the responses sit between guard words of the same sentinel: a tap sum that
reads past its row or its response is huge, the clamp turns it into +-1, and the comparison sees it.  The three
destinations are also placed 0, 4 and 8 bytes behind a 16-byte boundary, so that each is written in a pass of its own.
That the operands tell a fused multiply-add from the two separately rounded operations is counted on the CPU.  The
entries' refusals come back before any launch and need no GPU: tests/test_room_plan.py goes through every one of them."""
import numpy as np
import pytest
import torch

from tests import room_design as R
from tests._pkg import sub

pytestmark = pytest.mark.gpu

SEED = 179349
B, N, NC, STEPS = 3, 7, 4, 3
LABELS = np.array([0, 3, -1, 1, 2, NC, 3], np.int64)       # labels 2 and 5 lie outside the classes
LABELS9 = np.array([0, 1, 0, 2, 1, 0, 3, 1, 0], np.int64)
F = np.float32
UP, DOWN = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
SPECIALS = np.array([1.0, -1.0, UP, DOWN, -0.0, 2.0 ** -126, -2.0 ** -126, 0.0], F)
SENTINEL = F(1e30)
SPEEDS = {"none": (1.0, 1.0), "range": (0.9, 1.1), "half": (0.5, 0.5), "double": (2.0, 2.0)}
M = 4                                                      # responses per set
_RULE = {}                                                 # (case) -> the rule's rows, computed once and left unchanged


def _clips(n, length, seed=11):
    """Random samples in [-1.2, 1.2]; every third one is a planted special, another one in every clip."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.2, 1.2, (n, length)).astype(F)
    j = np.arange(0, length, 3)
    for r in range(n):
        x[r, j] = SPECIALS[(j // 3 + r) % len(SPECIALS)]
    return x


def _rirs(K, seed=31):
    """M responses of K taps, every tap below one in size (a product with +-2^-126 is subnormal), a unit first tap in the
    first one only, signs mixed, a few exact zeros and a -0.0."""
    rng = np.random.default_rng(seed + K)
    h = (rng.uniform(-0.9, 0.9, (M, K)) * np.exp(-np.arange(K) / max(K / 3.0, 1.0))[None, :]).astype(F)
    h[0, 0] = 1.0
    if K > 4:
        h[1, 2], h[2, 3] = 0.0, -0.0
    return h


def _guarded(h):
    """The responses on the device between guard words of the sentinel: a view of the middle of one allocation."""
    K = h.shape[1]
    flat = torch.full((M * K + 8,), float(SENTINEL), device="cuda")
    flat[4:4 + M * K] = torch.from_numpy(h.reshape(-1)).cuda()
    return flat, flat[4:4 + M * K].view(M, K)


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


def _augment(D, T, K, shift, speed, prob, taps=16, noise_prob=1.0):
    nz = _clips(4, T + 13, seed=23)
    h = _rirs(K)
    flat, view = _guarded(h)
    rv = D.DeviceDataset(view)
    assert rv.audio.data_ptr() == view.data_ptr()                   # the dataset reads the guarded allocation itself
    aug = D.Augment(shift=shift, gain=(0.5, 2.0), noise=D.DeviceDataset(nz), noise_prob=noise_prob,
                    noise_volume=(0.125, 0.75), speed=SPEEDS[speed], taps=taps, reverb=rv, reverb_prob=prob)
    return aug, nz, h, flat


def _want(D, key, rows, steps, table, rplan, h, plan, nz):
    if key not in _RULE:
        _RULE[key] = R.room_rows(D, rows, steps, table, rplan, h, plan, nz)
        _RULE[key].setflags(write=False)
    return _RULE[key]


def test_the_cases_are_what_they_say():
    """Decided on the CPU: the seed's coins, the shifts, and operands a fused multiply-add would round otherwise."""
    D = sub("dataset")
    host = object.__new__(D.DeviceDataset)
    from types import SimpleNamespace
    host.audio, host.device = SimpleNamespace(shape=(M, 64)), "cuda"
    half = D.Augment(reverb=host, reverb_prob=0.5)
    coins = [D.reverb_plan(SEED, st, B, half, M).apply.tolist() for st in range(STEPS)]
    assert {False, True} == set(coins[0]) == set(coins[1])          # both kinds of row in one batch, twice
    picks = np.concatenate([D.reverb_plan(SEED, st, B, D.Augment(reverb=host, reverb_prob=1.0), M).index for st in range(STEPS)])
    assert len(set(picks.tolist())) >= 2
    for T in (5, 4099):
        sh = np.concatenate([D.augment_plan(SEED, st, B, T, D.Augment(shift=T - 1), 0, 0).shift for st in range(STEPS)])
        assert sh.min() <= -(T - 1) + 1 and sh.max() >= (T - 1) - 6, (T, sh)     # both ends of the row, to a few samples
    rows = _clips(B, 4099)
    every = D.ReverbPlan(np.ones(B, bool), np.arange(B, dtype=np.int32))
    for K in (2, 7, 64, 8192):
        h = _rirs(K)
        e, fused = D.reverb_rows(rows, every, h), R.reverb_rows_unrounded_products(D, rows, every, h)
        differ = int(np.count_nonzero(_bits(e) != _bits(fused)))
        print("K = %d: outputs a fused tap sum would round otherwise: %d of %d" % (K, differ, e.size))
        assert differ > 1000, K
        small = np.abs(h[None, :, :1] * rows[:, None, :]).astype(F)   # products of the first taps with the planted 2^-126
        assert ((small > 0) & (small < F(2.0 ** -126))).any(), K


CASES = [(5, 1, "none"), (5, 2, "range"), (5, 7, "none"), (5, 7, "half"), (4099, 64, "none"), (4099, 64, "double"),
         (4099, 8192, "none"), (4099, 4096, "range")]


@pytest.mark.parametrize("T,K,speed", CASES)
def test_batch_draw_room_matches_the_restatement(T, K, speed):
    D, Kn = sub("dataset"), sub("kernels")
    clip_len = T + 37
    clips = _clips(N, clip_len)
    dev, col0 = "cuda", 8
    audio = torch.full((B, T), 9.0, device=dev)
    audio2 = torch.full((B, T), 9.0, device=dev)
    codes = torch.full((B * T,), -7, dtype=torch.int32, device=dev)
    onehot = torch.full((B, col0 + NC + 1), 9.0, device=dev)
    loss = torch.zeros(1, device=dev)
    big = K >= 4096
    for shift, prob in ((T - 1, 1.0),) if big else ((0, 1.0), (1, 0.5), (T - 1, 1.0)):
        aug, nz, h, flat = _augment(D, T, K, shift, speed, prob)
        ds = D.DeviceDataset(clips, LABELS, NC)
        s = ds.sampler(B, T, seed=SEED, crop="random", augment=aug)
        table = aug.table() if aug.resamples else None
        applied = []
        for step in range(2 if big else STEPS):
            idx, off = D.draw_plan(SEED, step, B, N, clip_len, T, True, "random")
            fenced = _fenced(clips, zip(idx, off), T)
            ds.audio.copy_(torch.from_numpy(fenced))
            plan, steps, rplan = s.augment_plan(), s.speed_plan(), s.reverb_plan()
            assert plan.mix.all()
            rows = np.stack([fenced[i, o:o + T] for i, o in zip(idx, off)])
            want = _want(D, ("batch", T, K, speed, shift, prob, step), rows, steps, table, rplan, h, plan, nz)
            s.draw(audio, audio2, codes, 256, onehot, 1, col0)
            s.log_step(loss)
            s.step += 1
            got = audio.cpu().numpy()
            bad = np.argwhere(_bits(got) != _bits(want))
            assert bad.size == 0, (shift, prob, step, len(bad), bad[:4].tolist(),
                                   [(got[b, j], want[b, j]) for b, j in bad[:4]], plan, steps, rplan)
            assert torch.equal(audio2.view(torch.int32), audio.view(torch.int32)), step
            assert torch.equal(codes.view(B, T), Kn.mu_law_encode(torch.as_tensor(want.copy(), device=dev), 256)), step
            assert s.indices.cpu().numpy().tolist() == idx.tolist(), step
            o = onehot.cpu().numpy()
            assert np.array_equal(o[:, col0:col0 + NC], _onehot(LABELS[idx], NC))
            assert (o[:, :col0] == 9.0).all() and (o[:, col0 + NC:] == 9.0).all()
            applied += rplan.apply.tolist()
        assert set(applied) == ({True} if prob == 1.0 else {False, True})
        assert s.state.cpu().tolist() == [SEED, 2 if big else STEPS]
        assert (flat[:4] == float(SENTINEL)).all() and (flat[-4:] == float(SENTINEL)).all()


@pytest.mark.parametrize("T,K", [(5, 7), (4099, 64)])
@pytest.mark.parametrize("speed", ["none", "range"])
def test_rows_whose_coin_is_off_are_the_older_entries_rows(T, K, speed):
    """At probability 0.5, from the same state: the rows whose coin is off hold the bits ``srwn_batch_draw_aug`` (no
    speed) or ``srwn_batch_draw_warp`` writes, the others do not."""
    D = sub("dataset")
    clips = _clips(N, T + 37)
    aug, nz, h, flat = _augment(D, T, K, T - 1, speed, 0.5)
    older = D.Augment(shift=aug.shift, gain=aug.gain, noise=aug.noise, noise_prob=1.0, noise_volume=aug.noise_volume,
                      speed=aug.speed, taps=aug.taps)
    ds = D.DeviceDataset(clips, LABELS, NC)
    s, so = (ds.sampler(B, T, seed=SEED, crop="random", augment=a) for a in (aug, older))
    a, b = torch.zeros((B, T), device="cuda"), torch.zeros((B, T), device="cuda")
    for step in range(STEPS):
        for x in (s, so):
            x.seek(step)
        rplan = s.reverb_plan()
        s.draw(a)
        so.draw(b)
        same = (a.view(torch.int32) == b.view(torch.int32)).all(dim=1).cpu().tolist()
        assert same == [not v for v in rplan.apply.tolist()], (step, same, rplan)


@pytest.mark.parametrize("T", [5, 4099])
def test_destinations_at_different_positions_against_the_16_byte_boundaries(T):
    """audio starts on a 16-byte boundary, the second buffer 4 bytes and the codes 8 bytes behind one: destinations that
    share the position are written in one pass and every other one in a pass of its own, each with its own head, body and
    tail.  The elements around the three buffers keep their fill."""
    D, Kn = sub("dataset"), sub("kernels")
    clips = _clips(N, T + 37)
    aug, nz, h, flat = _augment(D, T, 7, T - 1, "range", 0.5)
    s = D.DeviceDataset(clips, LABELS, NC).sampler(B, T, seed=SEED, crop="random", augment=aug)
    n = B * T
    big_a = torch.full((n + 8,), 9.0, device="cuda")
    big_b = torch.full((n + 8,), 9.0, device="cuda")
    big_c = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")
    audio, audio2, codes = big_a[4:4 + n].view(B, T), big_b[1:1 + n].view(B, T), big_c[2:2 + n]
    assert [t.data_ptr() % 16 for t in (audio, audio2, codes)] == [0, 4, 8]
    for step in range(2):
        idx, off = D.draw_plan(SEED, step, B, N, T + 37, T, True, "random")
        want = R.room_rows(D, np.stack([clips[i, o:o + T] for i, o in zip(idx, off)]), s.speed_plan(), aug.table(),
                           s.reverb_plan(), h, s.augment_plan(), nz)
        s.draw(audio, audio2, codes, 256)
        s.seek(step + 1)
        assert np.array_equal(_bits(audio.cpu().numpy()), _bits(want)), step
        assert torch.equal(audio2.view(torch.int32), audio.view(torch.int32)), step
        assert torch.equal(codes.view(B, T), Kn.mu_law_encode(torch.as_tensor(want, device="cuda"), 256)), step
    assert (big_a[:4] == 9.0).all() and (big_a[4 + n:] == 9.0).all() and big_b[0] == 9.0 and (big_b[1 + n:] == 9.0).all()
    assert (big_c[:2] == -7).all() and (big_c[2 + n:] == -7).all()


@pytest.mark.parametrize("K", [3, 16, 4096])
def test_the_planted_orders_and_roundings(K):
    """Records of halves and of a / 2, c / 2 alternating (the plants of tests/room_design.py scaled by a power of two, so
    that no sum reaches the clamp) under the planted responses, nothing else drawn (shift 0, gain 1, no noise): the
    outputs are the tap sums themselves -- 0.5 against 0.5 + 2^-24 for the two tap orders, 0 where a fused multiply-add
    leaves 2^-25 -- and every row the rule's."""
    D = sub("dataset")
    T = 520                                                        # more than one workgroup per row at a span of 256 or 512
    clips = np.repeat(R.plant_rows(T, 0.5), 2, 0)                    # records 0, 1: halves; 2, 3: alternating
    h = R.plant_rirs(K)
    aug = D.Augment(reverb=D.DeviceDataset(h), reverb_prob=1.0)
    s = D.DeviceDataset(clips).sampler(4, T, seed=SEED, augment=aug)
    audio = torch.zeros((4, T), device="cuda")
    seen = set()
    for step in range(8):
        idx, off = s.plan()
        rplan, plan = s.reverb_plan(), s.augment_plan()
        want = R.room_rows(D, clips[idx], None, None, rplan, h, plan)
        s.draw(audio)
        s.seek(step + 1)
        got = audio.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), step
        for b in range(4):
            kind = (int(idx[b]) // 2, int(rplan.index[b]))
            seen.add(kind)
            if kind == (0, 0):
                assert (got[b, 2:] == F(0.5)).all()
            if kind == (0, 1):
                assert (got[b, 2:] == F(0.5 + 2.0 ** -24)).all()
            if kind == (1, 2):
                assert (got[b, 1::2] == 0.0).all()                   # fused: 2^-25
    assert {(0, 0), (0, 1), (1, 2)} <= seen


@pytest.mark.parametrize("T,K,speed", [(5, 7, "range"), (4099, 64, "none"), (4099, 64, "range")])
def test_pair_draw_room_matches_the_restatement(T, K, speed):
    D = sub("dataset")
    P, clip_len = 3, T + 37
    clips = _clips(9, clip_len)
    aug, nz, h, flat = _augment(D, T, K, T - 1, speed, 0.5, noise_prob=0.5)
    ds = D.DeviceDataset(clips, LABELS9, NC)
    s = ds.pair_sampler(P, T, seed=SEED, crop="random", augment=aug)
    table = aug.table() if aug.resamples else None
    audio = torch.full((2 * P, T), 9.0, device="cuda")
    y = torch.full((P,), 9.0, device="cuda")
    loss, dist = torch.zeros(1, device="cuda"), torch.zeros(P, device="cuda")
    applied, differ = [], 0
    for step in range(STEPS):
        left, right, ol, orr, want_y = D.pair_plan(SEED, step, P, LABELS9, NC, clip_len, T, 0.5, True, "random")
        fenced = _fenced(clips, list(zip(left, ol)) + list(zip(right, orr)), T)
        ds.audio.copy_(torch.from_numpy(fenced))
        pl, pr = s.augment_plan()
        sl, sr = s.speed_plan()
        rl, rr = s.reverb_plan()
        want = np.concatenate([
            R.room_rows(D, np.stack([fenced[i, o:o + T] for i, o in zip(left, ol)]), sl, table, rl, h, pl, nz),
            R.room_rows(D, np.stack([fenced[i, o:o + T] for i, o in zip(right, orr)]), sr, table, rr, h, pr, nz)])
        s.draw(audio, y)
        s.log_pairs(loss, dist)
        s.step += 1
        got = audio.cpu().numpy()
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, (step, len(bad), bad[:4].tolist(), pl, pr, sl, sr, rl, rr)
        assert y.cpu().tolist() == want_y.tolist() == s.y.cpu().tolist()
        assert s.indices.cpu().tolist() == left.tolist() and s.right.cpu().tolist() == right.tolist()
        applied += rl.apply.tolist() + rr.apply.tolist()
        differ += sum(1 for b in range(P) if rl.apply[b] and rr.apply[b] and rl.index[b] != rr.index[b])
    assert set(applied) == {False, True}
    assert differ > 0                                                # the two sides pick responses of their own
    assert (flat[:4] == float(SENTINEL)).all() and (flat[-4:] == float(SENTINEL)).all()
