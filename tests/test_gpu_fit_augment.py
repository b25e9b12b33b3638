"""GPU tests of ``fit`` on augmenting samplers: against the host loop ``train(augment_rows(clips[idx, off:off + T], plan))``
over ``draw_plan`` / ``pair_plan`` and ``augment_plan``, bit for bit in every loss (and distance) and every parameter
tensor -- the classifier in fp32 and bf16, the softmax teacher (the codes come from the augmented rows), the auto-encoder
(both of its buffers hold the same augmented clip) and the twin towers --, eager launches, continuation by ``seek`` and by
``load_training_state``, two ranks' shares each run alone, validation inside ``fit``, and a sampler without an ``Augment``,
which still gives the plain host loop's bits.

Shapes: 7 clips of 300 samples cropped at random to T = 256, B = 2 (the twins: 9 labelled records, P = 2), stacks of three
layers [1, 2, 4] at R = 32 and S = 128; 3 noise clips of 269 samples mixed into half of the rows; shifts up to 40 samples."""
import numpy as np
import pytest
import torch

from tests._pkg import sub

pytestmark = pytest.mark.gpu

SEED = 3
N, CLIP, T, B, DIL, R, S, NC = 7, 300, 256, 2, [1, 2, 4], 32, 128, 4
LABELS = np.array([0, 3, -1, 1, 2, NC, 3], np.int64)       # labels 2 and 5 lie outside the classes: zero rows
LABELS9 = np.array([0, 1, 0, 2, 1, 0, 3, 1, 0], np.int64)
P = 2
NOISE_N, NOISE_LEN = 3, T + 13
AUG = dict(shift=40, gain=(0.5, 1.5), noise_prob=0.5, noise_volume=(0.05, 0.3))


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
    """The Augment of these tests; `host`: without device memory (what ``augment_plan`` needs is the noise set's shape)."""
    D = sub("dataset")
    if host:
        from types import SimpleNamespace
        nz = object.__new__(D.DeviceDataset)
        nz.audio, nz.device = SimpleNamespace(shape=(NOISE_N, NOISE_LEN)), "cuda"
    else:
        nz = D.DeviceDataset(_noise())
    return D.Augment(noise=nz, **AUG)


def _classifier(dtype):
    return sub("model").WaveNet(T, NC, DIL, dilation_channels=R, skip_channels=S, output_channels=NC, learning_rate=1e-3,
                                dtype=dtype, seed=5)


def _teacher():
    return sub("model").WaveNetTeacher(T, 0, DIL, dilation_channels=R, skip_channels=S, quantization_channels=256,
                                       dtype=torch.float32, learning_rate=1e-3, head="softmax", seed=5)


def _autoencoder():
    return sub("model").WaveNetAutoEncoder(T, NC, 5, DIL, dilation_channels=R, skip_channels=S, latent_channels=8,
                                           pool_stride=16, learning_rate=1e-3, dtype=torch.bfloat16, seed=5)


def _twins():
    return sub("model").SiameseWaveNet(T, 2, DIL, dilation_channels=R, skip_channels=S, learning_rate=1e-3,
                                       dtype=torch.float32, seed=5)


KINDS = {"classifier_fp32": (lambda: _classifier(torch.float32), True), "classifier_bf16": (lambda: _classifier(torch.bfloat16), True),
         "teacher": (_teacher, False), "autoencoder": (_autoencoder, True)}


def _host_rows(st, augment, rank=0, world=1):
    """The batch of step `st` as the host makes it: (rows [B, T], the records' labels)."""
    D = sub("dataset")
    clips = _clips()
    idx, off = D.draw_plan(SEED, st, B, N, CLIP, T, True, "random", rank, world)
    x = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
    if augment is not None:
        x = D.augment_rows(x, D.augment_plan(SEED, st, B, T, augment, NOISE_N, NOISE_LEN, rank, world), _noise())
    return x, LABELS[idx]


def _host_loop(kind, steps, first=0, model=None, augment="default", rank=0, world=1):
    make, labelled = KINDS[kind]
    augment = _augment(host=True) if augment == "default" else augment
    m = model or make()
    losses = []
    for st in range(first, first + steps):
        x, lab = _host_rows(st, augment, rank, world)
        losses.append(m.train(x, _onehot(lab, NC)) if labelled else m.train(x))
    return m, np.array(losses, np.float32)


def _sampler(kind, augment="default", **kw):
    D = sub("dataset")
    labelled = KINDS[kind][1]
    ds = D.DeviceDataset(_clips(), LABELS if labelled else None, NC if labelled else 0)
    return ds.sampler(B, T, seed=SEED, crop="random", augment=_augment() if augment == "default" else augment, **kw)


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
    """Decided on the CPU: the six steps shift both ways, scale, and hold mixed and unmixed rows."""
    D = sub("dataset")
    plans = [D.augment_plan(SEED, st, B, T, _augment(host=True), NOISE_N, NOISE_LEN) for st in range(6)]
    shift = np.concatenate([p.shift for p in plans])
    assert shift.min() < 0 < shift.max() and set(np.concatenate([p.mix for p in plans]).tolist()) == {False, True}
    assert len(set(np.concatenate([p.gain for p in plans]).tolist())) == 6 * B


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
    got = m.fit(_sampler("classifier_fp32"), 6)
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
    s = _sampler("classifier_fp32")
    first = m.fit(s, 3)
    m.save(d, 3, force=True)
    m.save_training_state(d, 3, sampler=s)
    m2 = _classifier(torch.float32)
    m2._engine(B, T)
    s2 = _sampler("classifier_fp32")
    assert m2.load(d) and m2.load_training_state(d, sampler=s2) is True and s2.step == 3
    rest = m2.fit(s2, 3)
    assert np.array_equal(_bits(np.concatenate([first, rest])), _bits(h["losses"]))
    _same(_params(m2), h["p6"])


def test_two_ranks_draw_disjoint_plans_and_each_equals_its_host_loop():
    D = sub("dataset")
    a = _augment(host=True)
    rows = []
    for rank in (0, 1):
        for st in range(4):
            p = D.augment_plan(SEED, st, B, T, a, NOISE_N, NOISE_LEN, rank, 2)
            rows += list(zip(p.shift.tolist(), p.gain.tolist(), p.volume.tolist()))
    assert len(set(rows)) == len(rows) == 2 * 4 * B
    for rank in (0, 1):
        ref, want = _host_loop("classifier_fp32", 4, rank=rank, world=2)
        m = _classifier(torch.float32)
        got = m.fit(_sampler("classifier_fp32", rank=rank, world=2), 4)
        assert np.array_equal(_bits(got), _bits(want)), rank
        _same(_params(m), _params(ref))


def test_fit_with_validation_keeps_the_bits(host):
    D = sub("dataset")
    h = host("classifier_fp32")
    m = _classifier(torch.float32)
    ev = D.DeviceDataset(_clips()[:, :T], np.abs(LABELS) % NC, NC).eval_sampler(B, T)
    losses, results = m.fit(_sampler("classifier_fp32"), 6, validate=(ev, 3))
    assert np.array_equal(_bits(losses), _bits(h["losses"])) and [r.step for r in results] == [3, 6]
    _same(_params(m), h["p6"])
    with pytest.raises(ValueError, match="the sampler augments"):
        _teacher().evaluate(_sampler("teacher", shuffle=False))


def test_fit_under_training_controls_equals_the_host_loop():
    """Clipping, a schedule and EMA weights act behind the draw: the augmented ``fit`` is still the host loop."""
    O = sub("optim")
    ctl = dict(schedule=O.cosine(2e-3, 6), horizon=6, clip_norm=0.5, ema_decay=0.9)
    ref = _classifier(torch.float32)
    ref.set_training_controls(**ctl)
    _, want = _host_loop("classifier_fp32", 6, model=ref)
    m = _classifier(torch.float32)
    m.set_training_controls(**ctl)
    got = m.fit(_sampler("classifier_fp32"), 6)
    assert np.array_equal(_bits(got), _bits(want))
    _same(_params(m), _params(ref))
    with m.ema_weights(), ref.ema_weights():
        _same(_params(m), _params(ref))


def test_a_sampler_without_an_augment_is_the_plain_host_loop():
    ref, want = _host_loop("classifier_fp32", 4, augment=None)
    m = _classifier(torch.float32)
    s = _sampler("classifier_fp32", augment=None)
    assert s.augment is None
    got = m.fit(s, 4)
    assert np.array_equal(_bits(got), _bits(want))
    _same(_params(m), _params(ref))


# ---- the twins ---------------------------------------------------------------------------------------------------------
def test_twins_fit_equals_the_host_loop():
    D = sub("dataset")
    clips = _clips(9)
    a = _augment(host=True)
    ref = _twins()
    loss, dist = [], []
    for st in range(6):
        left, right, ol, orr, y = D.pair_plan(SEED, st, P, LABELS9, NC, CLIP, T, 0.5, True, "random")
        pl = D.augment_plan(SEED, st, P, T, a, NOISE_N, NOISE_LEN, side=0)
        pr = D.augment_plan(SEED, st, P, T, a, NOISE_N, NOISE_LEN, side=1)
        xl = D.augment_rows(np.stack([clips[i, o:o + T] for i, o in zip(left, ol)]), pl, _noise())
        xr = D.augment_rows(np.stack([clips[i, o:o + T] for i, o in zip(right, orr)]), pr, _noise())
        l, d = ref.train(None, xl, xr, y)
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


# ---- the example drivers -----------------------------------------------------------------------------------------------
def _example(name):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_" + name, os.path.join(root, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    return ex, root


def _forget_dropin(root):
    import os
    import sys
    for m in ("model", "ops", "nsynth", "simple_audio"):
        sys.modules.pop(m, None)
    d = os.path.join(root, "sr-wavenet_amd", "dropin")
    while d in sys.path:
        sys.path.remove(d)


@pytest.mark.parametrize("name", ["classifier", "siamese"])
def test_example_with_augmentation_flags(tmp_path, name):
    """--device-data with all five flags trains; the flags without --device-data are refused with a message."""
    import os
    noise = str(tmp_path / "noise.npy")
    np.save(noise, (0.3 * np.random.default_rng(2).standard_normal((3, 600))).astype(np.float32))
    flags = ["--shift", "50", "--gain", "0.7:1.3", "--noise", noise, "--noise-prob", "0.5", "--noise-volume", "0.1:0.4"]
    shape = ["--train", "--logdir", str(tmp_path / "run"), "--steps", "5", "--print-steps", "3", "--batch-size", "2",
             "--num-samples", "512", "--layers", "6", "--seed", "1"]
    ex, root = _example(name)
    try:
        with pytest.raises(SystemExit, match="add --device-data"):
            ex.main(shape + flags)
        assert not os.path.exists(str(tmp_path / "run"))
        ex.main(shape + flags + ["--device-data", "--device-clips", "12"] +
                (["--validation-clips", "4", "--validate-every", "3"] if name == "classifier" else []))
        assert os.path.exists(os.path.join(str(tmp_path / "run"), "checkpoint"))
    finally:
        _forget_dropin(root)
