"""GPU tests of ``fit`` on samplers that reverberate: against the host loop ``train(augment_rows(reverb_rows(resample_rows(
clips[idx, off:off + T], steps, table), rplan, rirs), plan))`` over ``draw_plan`` / ``pair_plan``, ``speed_plan``,
``reverb_plan`` and ``augment_plan``, bit for bit in every loss (and distance) and every parameter tensor -- the classifier
in fp32 and bf16, the softmax teacher and the twin towers --, eager launches and replays of the captured step, continuation
by ``seek`` and by ``load_training_state``, and rank 1 of 2; and ``examples/classifier.py`` with ``--device-data --rir``.

Shapes, those of tests/test_gpu_fit_resample.py: 7 clips of 300 samples cropped at random to T = 256, B = 2 (the twins: 9
labelled records, P = 2), stacks of three layers [1, 2, 4] at R = 32 and S = 128; speeds 0.9 .. 1.1 through 16 taps, shifts
up to 40 samples, gains 0.5 .. 1.5, 3 noise clips of 269 samples mixed into half of the rows; and 3 synthetic room
responses of 64 taps convolved into half of the rows."""
import numpy as np
import pytest
import torch

from tests import room_design as R
from tests._pkg import sub

pytestmark = pytest.mark.gpu

SEED = 3
N, CLIP, T, B, DIL, RC, S, NC = 7, 300, 256, 2, [1, 2, 4], 32, 128, 4
LABELS = np.array([0, 3, -1, 1, 2, NC, 3], np.int64)       # labels 2 and 5 lie outside the classes: zero rows
LABELS9 = np.array([0, 1, 0, 2, 1, 0, 3, 1, 0], np.int64)
P = 2
NOISE_N, NOISE_LEN = 3, T + 13
RIR_N, RIR_K = 3, 64
AUG = dict(shift=40, gain=(0.5, 1.5), noise_prob=0.5, noise_volume=(0.05, 0.3), speed=(0.9, 1.1), taps=16, reverb_prob=0.5)


def _clips(n=N, length=CLIP, seed=11):
    rng = np.random.default_rng(seed)
    return (0.9 * np.sin(np.arange(length)[None, :] * rng.uniform(0.05, 0.6, (n, 1))) *
            rng.uniform(0.2, 1.0, (n, 1)) + 0.02 * rng.standard_normal((n, length))).astype(np.float32)


def _noise():
    return (0.5 * np.random.default_rng(29).standard_normal((NOISE_N, NOISE_LEN))).astype(np.float32)


def _rirs():
    return sub("dataset").synthetic_rirs(RIR_N, RIR_K, rt60=(0.002, 0.004), seed=41)     # (64 taps are 4 ms)


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
    """The Augment of these tests; `host`: without device memory (what the plans need is the sets' shapes)."""
    D = sub("dataset")
    if host:
        from types import SimpleNamespace
        nz, rv = object.__new__(D.DeviceDataset), object.__new__(D.DeviceDataset)
        nz.audio, nz.device = SimpleNamespace(shape=(NOISE_N, NOISE_LEN)), "cuda"
        rv.audio, rv.device = SimpleNamespace(shape=(RIR_N, RIR_K)), "cuda"
    else:
        nz, rv = D.DeviceDataset(_noise()), D.DeviceDataset(_rirs())
    return D.Augment(noise=nz, reverb=rv, **AUG)


def _classifier(dtype):
    return sub("model").WaveNet(T, NC, DIL, dilation_channels=RC, skip_channels=S, output_channels=NC, learning_rate=1e-3,
                                dtype=dtype, seed=5)


def _teacher():
    return sub("model").WaveNetTeacher(T, 0, DIL, dilation_channels=RC, skip_channels=S, quantization_channels=256,
                                       dtype=torch.float32, learning_rate=1e-3, head="softmax", seed=5)


def _twins():
    return sub("model").SiameseWaveNet(T, 2, DIL, dilation_channels=RC, skip_channels=S, learning_rate=1e-3,
                                       dtype=torch.float32, seed=5)


KINDS = {"classifier_fp32": (lambda: _classifier(torch.float32), True),
         "classifier_bf16": (lambda: _classifier(torch.bfloat16), True), "teacher": (_teacher, False)}
_ROWS = {}                   # (step, rank, world) -> the host's batch, made once and left unchanged


def _host_rows(st, rank=0, world=1):
    """The batch of step `st` as the host makes it: (rows [B, T], the records' labels)."""
    if (st, rank, world) not in _ROWS:
        D = sub("dataset")
        a = _augment(host=True)
        clips = _clips()
        idx, off = D.draw_plan(SEED, st, B, N, CLIP, T, True, "random", rank, world)
        x = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
        x = R.room_rows(D, x, D.speed_plan(SEED, st, B, a, rank, world), a.table(),
                        D.reverb_plan(SEED, st, B, a, RIR_N, rank, world), _rirs(),
                        D.augment_plan(SEED, st, B, T, a, NOISE_N, NOISE_LEN, rank, world), _noise())
        x.setflags(write=False)
        _ROWS[(st, rank, world)] = (x, LABELS[idx])
    return _ROWS[(st, rank, world)]


def _host_loop(kind, steps, rank=0, world=1):
    make, labelled = KINDS[kind]
    m = make()
    losses = []
    for st in range(steps):
        x, lab = _host_rows(st, rank, world)
        losses.append(m.train(x.copy(), _onehot(lab, NC)) if labelled else m.train(x.copy()))
    return m, np.array(losses, np.float32)


def _sampler(kind="classifier_fp32", **kw):
    D = sub("dataset")
    labelled = KINDS[kind][1]
    ds = D.DeviceDataset(_clips(), LABELS if labelled else None, NC if labelled else 0)
    return ds.sampler(B, T, seed=SEED, crop="random", augment=_augment(), **kw)


@pytest.fixture(scope="module")
def host():
    """Each kind's host loop, once: the losses of six steps and the parameters behind them."""
    cache = {}

    def get(kind):
        if kind not in cache:
            m, losses = _host_loop(kind, 6)
            cache[kind] = dict(losses=losses, p6=_params(m))
        return cache[kind]
    return get


def test_the_plans_do_something():
    """Decided on the CPU: the six steps hold reverberated and dry rows, and a reverberated row is not the drawn one."""
    D = sub("dataset")
    a = _augment(host=True)
    assert a.reverberates and a.resamples
    plans = [D.reverb_plan(SEED, st, B, a, RIR_N) for st in range(6)]
    assert set(np.concatenate([p.apply for p in plans]).tolist()) == {False, True}
    assert any(set(p.apply.tolist()) == {False, True} for p in plans)            # both kinds in one batch
    x = _clips()[:B, :T]
    every = D.ReverbPlan(np.ones(B, bool), np.zeros(B, np.int32))
    e = D.reverb_rows(x, every, _rirs())
    assert not np.array_equal(e, x) and np.isfinite(e).all()
    pairs = [D.reverb_plan(SEED, st, P, a, RIR_N, side=side).apply for st in range(6) for side in (0, 1)]
    assert set(np.concatenate(pairs).tolist()) == {False, True}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fit_equals_the_host_loop(host, kind):
    """Six steps: two eager, the capture, replays."""
    h = host(kind)
    m = KINDS[kind][0]()
    s = _sampler(kind)
    got = m.fit(s, 6)
    print(kind, "fit", got.tolist(), "host loop", h["losses"].tolist())
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(h["losses"]))
    _same(_params(m), h["p6"])
    assert s.step == 6 and s.state.cpu().tolist()[1] == 6
    assert m._engine(B, T)._fit_state["graphs"] is not None


def test_fit_with_eager_launches(host, monkeypatch):
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    h = host("classifier_fp32")
    m = _classifier(torch.float32)
    got = m.fit(_sampler(), 6)
    assert m._engine(B, T)._fit_state["graphs"] is None
    assert np.array_equal(_bits(got), _bits(h["losses"]))
    _same(_params(m), h["p6"])


def test_fit_continues_after_seek(host):
    h = host("teacher")
    m = _teacher()
    first = m.fit(_sampler("teacher"), 3)
    s = _sampler("teacher")                   # another sampler object: fit captures for it again
    s.seek(3)
    rest = m.fit(s, 3)
    assert np.array_equal(_bits(np.concatenate([first, rest])), _bits(h["losses"]))
    _same(_params(m), h["p6"])


def test_fit_continues_from_a_training_state(host, tmp_path):
    h = host("classifier_fp32")
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
    r0 = [D.reverb_plan(SEED, st, B, a, RIR_N, 0, 2).apply.tolist() for st in range(4)]
    r1 = [D.reverb_plan(SEED, st, B, a, RIR_N, 1, 2).apply.tolist() for st in range(4)]
    assert r0 != r1
    ref, want = _host_loop("classifier_fp32", 4, rank=1, world=2)
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
            sides.append(R.room_rows(D, rows, D.speed_plan(SEED, st, P, a, side=side), a.table(),
                                     D.reverb_plan(SEED, st, P, a, RIR_N, side=side), _rirs(),
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


# ---- the example driver -------------------------------------------------------------------------------------------------
def test_classifier_example_with_room_responses(tmp_path):
    """--device-data with --rir on a file written by ``synthetic_rirs`` trains; without --device-data it is refused."""
    import importlib.util
    import os
    import sys
    rir = str(tmp_path / "rirs.npy")
    np.save(rir, sub("dataset").synthetic_rirs(3, 256, rt60=(0.01, 0.02), seed=2))
    flags = ["--rir", rir, "--rir-prob", "0.5", "--shift", "50"]
    shape = ["--train", "--logdir", str(tmp_path / "run"), "--steps", "5", "--print-steps", "3", "--batch-size", "2",
             "--num-samples", "512", "--layers", "6", "--seed", "1"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_classifier", os.path.join(root, "examples", "classifier.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    try:
        with pytest.raises(SystemExit, match="add --device-data"):
            ex.main(shape + flags)
        assert not os.path.exists(str(tmp_path / "run"))
        ex.main(shape + flags + ["--device-data", "--device-clips", "12", "--validation-clips", "4", "--validate-every", "3"])
        assert os.path.exists(os.path.join(str(tmp_path / "run"), "checkpoint"))
    finally:
        for m in ("model", "ops", "nsynth", "simple_audio"):
            sys.modules.pop(m, None)
        d = os.path.join(root, "sr-wavenet_amd", "dropin")
        while d in sys.path:
            sys.path.remove(d)
