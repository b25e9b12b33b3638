"""GPU tests of ``fit`` on samplers that resample: against the host loop ``train(augment_rows(resample_rows(clips[idx,
off:off + T], steps, table), plan))`` over ``draw_plan`` / ``pair_plan``, ``speed_plan`` and ``augment_plan``, bit for bit in
every loss (and distance) and every parameter tensor -- the classifier in fp32 and bf16 and the twin towers --, eager
launches and replays of the captured step, continuation by ``seek`` and by ``load_training_state``, and rank 1 of 2.

Shapes: 7 clips of 300 samples cropped at random to T = 256, B = 2 (the twins: 9 labelled records, P = 2), stacks of three
layers [1, 2, 4] at R = 32 and S = 128; speeds 0.9 .. 1.1 through 16 taps, shifts up to 40 samples, gains 0.5 .. 1.5, 3 noise
clips of 269 samples mixed into half of the rows."""
import numpy as np
import pytest
import torch

from tests import resample_design as R
from tests._pkg import sub

pytestmark = pytest.mark.gpu

SEED = 3
N, CLIP, T, B, DIL, RC, S, NC = 7, 300, 256, 2, [1, 2, 4], 32, 128, 4
LABELS = np.array([0, 3, -1, 1, 2, NC, 3], np.int64)       # labels 2 and 5 lie outside the classes: zero rows
LABELS9 = np.array([0, 1, 0, 2, 1, 0, 3, 1, 0], np.int64)
P = 2
NOISE_N, NOISE_LEN = 3, T + 13
AUG = dict(shift=40, gain=(0.5, 1.5), noise_prob=0.5, noise_volume=(0.05, 0.3), speed=(0.9, 1.1), taps=16)


def _clips(n=N, length=CLIP, seed=11):
    rng = np.random.default_rng(seed)
    return (0.9 * np.sin(np.arange(length)[None, :] * rng.uniform(0.05, 0.6, (n, 1))) *
            rng.uniform(0.2, 1.0, (n, 1)) + 0.02 * rng.standard_normal((n, length))).astype(np.float32)


def _noise():
    return (0.5 * np.random.default_rng(29).standard_normal((NOISE_N, NOISE_LEN))).astype(np.float32)


def _onehot(labels, C):
    out = np.zeros((len(labels), C), np.float32)
    ok = (labels >= 0) & (labels < C)
    out[np.nonzero(ok)[0], labels[ok]] = 1.0
    return out


def _params(m):
    return {k: v.detach().cpu().clone() for k, v in m.network_params.items()}


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _augment(host=False):
    """The Augment of these tests; `host`: without device memory (what the plans need is the noise set's shape)."""
    D = sub("dataset")
    if host:
        from types import SimpleNamespace
        nz = object.__new__(D.DeviceDataset)
        nz.audio, nz.device = SimpleNamespace(shape=(NOISE_N, NOISE_LEN)), "cuda"
    else:
        nz = D.DeviceDataset(_noise())
    return D.Augment(noise=nz, **AUG)


def _classifier(dtype):
    return sub("model").WaveNet(T, NC, DIL, dilation_channels=RC, skip_channels=S, output_channels=NC, learning_rate=1e-3,
                                dtype=dtype, seed=5)


def _twins():
    return sub("model").SiameseWaveNet(T, 2, DIL, dilation_channels=RC, skip_channels=S, learning_rate=1e-3,
                                       dtype=torch.float32, seed=5)


def _host_rows(st, rank=0, world=1):
    """The batch of step `st` as the host makes it: (rows [B, T], the records' labels)."""
    D = sub("dataset")
    a = _augment(host=True)
    clips = _clips()
    idx, off = D.draw_plan(SEED, st, B, N, CLIP, T, True, "random", rank, world)
    x = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
    x = R.warp_rows(D, x, D.speed_plan(SEED, st, B, a, rank, world), a.table(),
                    D.augment_plan(SEED, st, B, T, a, NOISE_N, NOISE_LEN, rank, world), _noise())
    return x, LABELS[idx]


def _host_loop(dtype, steps, rank=0, world=1):
    m = _classifier(dtype)
    losses = []
    for st in range(steps):
        x, lab = _host_rows(st, rank, world)
        losses.append(m.train(x, _onehot(lab, NC)))
    return m, np.array(losses, np.float32)


def _sampler(**kw):
    D = sub("dataset")
    return D.DeviceDataset(_clips(), LABELS, NC).sampler(B, T, seed=SEED, crop="random", augment=_augment(), **kw)


@pytest.fixture(scope="module")
def host():
    """Each dtype's host loop, once: the losses of six steps and the parameters behind them."""
    cache = {}

    def get(dtype):
        if dtype not in cache:
            m, losses = _host_loop(dtype, 6)
            cache[dtype] = dict(losses=losses, p6=_params(m))
        return cache[dtype]
    return get


def test_the_plans_do_something():
    """Decided on the CPU: the six steps play slower and faster, and the resampled rows are not the drawn ones."""
    D = sub("dataset")
    a = _augment(host=True)
    steps = np.concatenate([D.speed_plan(SEED, st, B, a) for st in range(6)])
    assert steps.min() < 1 << 24 < steps.max() and len(set(steps.tolist())) == 6 * B
    x = _clips()[:B, :T]
    assert not np.array_equal(D.resample_rows(x, steps[:B], a.table()), x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fit_equals_the_host_loop(host, dtype):
    """Six steps: two eager, the capture, replays."""
    h = host(dtype)
    m = _classifier(dtype)
    s = _sampler()
    got = m.fit(s, 6)
    print("fit", got.tolist(), "host loop", h["losses"].tolist())
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(h["losses"]))
    _same(_params(m), h["p6"])
    assert s.step == 6 and s.state.cpu().tolist()[1] == 6
    assert m._engine(B, T)._fit_state["graphs"] is not None


def test_fit_with_eager_launches(host, monkeypatch):
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    h = host(torch.float32)
    m = _classifier(torch.float32)
    got = m.fit(_sampler(), 6)
    assert m._engine(B, T)._fit_state["graphs"] is None
    assert np.array_equal(_bits(got), _bits(h["losses"]))
    _same(_params(m), h["p6"])


def test_fit_continues_after_seek(host):
    h = host(torch.float32)
    m = _classifier(torch.float32)
    first = m.fit(_sampler(), 3)
    s = _sampler()                            # another sampler object: fit captures for it again
    s.seek(3)
    rest = m.fit(s, 3)
    assert np.array_equal(_bits(np.concatenate([first, rest])), _bits(h["losses"]))
    _same(_params(m), h["p6"])


def test_fit_continues_from_a_training_state(host, tmp_path):
    h = host(torch.float32)
    d = str(tmp_path)
    m = _classifier(torch.float32)
    s = _sampler()
    first = m.fit(s, 3)
    m.save(d, 3, force=True)
    m.save_training_state(d, 3, sampler=s)
    m2 = _classifier(torch.float32)
    m2._engine(B, T)
    s2 = _sampler()
    assert m2.load(d) and m2.load_training_state(d, sampler=s2) is True and s2.step == 3
    rest = m2.fit(s2, 3)
    assert np.array_equal(_bits(np.concatenate([first, rest])), _bits(h["losses"]))
    _same(_params(m2), h["p6"])


def test_rank_one_of_two_equals_its_host_loop():
    D = sub("dataset")
    a = _augment(host=True)
    r0 = np.concatenate([D.speed_plan(SEED, st, B, a, 0, 2) for st in range(4)])
    r1 = np.concatenate([D.speed_plan(SEED, st, B, a, 1, 2) for st in range(4)])
    assert not set(r0.tolist()) & set(r1.tolist())
    ref, want = _host_loop(torch.float32, 4, rank=1, world=2)
    m = _classifier(torch.float32)
    got = m.fit(_sampler(rank=1, world=2), 4)
    assert np.array_equal(_bits(got), _bits(want))
    _same(_params(m), _params(ref))


def test_twins_fit_equals_the_host_loop():
    D = sub("dataset")
    clips = _clips(9)
    a = _augment(host=True)
    ref = _twins()
    loss, dist = [], []
    for st in range(6):
        left, right, ol, orr, y = D.pair_plan(SEED, st, P, LABELS9, NC, CLIP, T, 0.5, True, "random")
        sides = []
        for side, (rec, off) in enumerate(((left, ol), (right, orr))):
            rows = np.stack([clips[i, o:o + T] for i, o in zip(rec, off)])
            sides.append(R.warp_rows(D, rows, D.speed_plan(SEED, st, P, a, side=side), a.table(),
                                     D.augment_plan(SEED, st, P, T, a, NOISE_N, NOISE_LEN, side=side), _noise()))
        l, d = ref.train(None, sides[0], sides[1], y)
        loss.append(l); dist.append(d)
    want_loss, want_dist = np.array(loss, np.float32), np.array(dist, np.float32).reshape(6, P)
    m = _twins()
    s = D.DeviceDataset(clips, LABELS9, NC).pair_sampler(P, T, seed=SEED, crop="random", augment=_augment())
    got_loss, got_dist = m.fit(s, 6)
    print("fit", got_loss.tolist(), "host loop", want_loss.tolist())
    assert np.array_equal(_bits(got_loss), _bits(want_loss))
    assert np.array_equal(_bits(got_dist), _bits(want_dist))
    _same(_params(m), _params(ref))
    assert s.step == 6 and m._engine(2 * P, T)._fit_state["graphs"] is not None
