"""GPU tests of the device-resident datasets: the draw kernel against ``dataset.draw_plan`` entry by entry, ``fit`` against
the host loop ``train(x)`` over the plan's batches bit for bit (losses and every parameter tensor), continuation, eager
launches, a loss ring shorter than the run, ``train(x)`` and ``fit`` mixed on one model, and TFRecord loading.

Shapes: 7 clips of 70 samples, batches of 3, stacks of three layers [1, 2, 4] at R = 32 and S = 128."""
import os
import sys

import numpy as np
import pytest
import torch

from tests._pkg import sub

pytestmark = pytest.mark.gpu

N, CLIP, B, DIL, R, S = 7, 70, 3, [1, 2, 4], 32, 128
NC = 4                                                  # classes; labels 2 and 5 of LABELS lie outside them
LABELS = np.array([0, 3, -1, 1, 2, NC, 3], np.int64)
SEED = 3


def _clips():
    rng = np.random.default_rng(11)
    return (0.9 * np.sin(np.arange(CLIP)[None, :] * rng.uniform(0.05, 0.6, (N, 1))) *
            rng.uniform(0.2, 1.0, (N, 1)) + 0.02 * rng.standard_normal((N, CLIP))).astype(np.float32)


def _onehot(labels, C):
    out = np.zeros((len(labels), C), np.float32)
    ok = (labels >= 0) & (labels < C)
    out[np.nonzero(ok)[0], labels[ok]] = 1.0            # tf.one_hot: out of range -> zeros
    return out


def _dataset(labels=True):
    D = sub("dataset")
    return D.DeviceDataset(_clips(), LABELS if labels else None, NC if labels else 0)


def _params(m):
    return {k: v.detach().cpu().clone() for k, v in m.network_params.items()}


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- the kernel against the plan ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", ["head", "random"])
@pytest.mark.parametrize("T", [70, 64, 61])
def test_draw_matches_the_plan(crop, T):
    D, K = sub("dataset"), sub("kernels")
    clips = _clips()
    ds = _dataset()
    assert len(ds) == N and ds.clip_len == CLIP and ds.nbytes == N * CLIP * 4 + N * 4
    s = ds.sampler(B, T, seed=SEED, crop=crop, log_capacity=4)
    frames, lat, Ep = 2, 8, 16                           # the auto-encoder form: NC condition columns behind 8 latent ones
    dev = "cuda"
    audio = torch.full((B, T), 9.0, device=dev)
    audio2 = torch.full((B, T), 9.0, device=dev)
    codes = torch.full((B * T,), -7, dtype=torch.int32, device=dev)
    onehot = torch.full((B, NC), 9.0, device=dev)
    cond = torch.full((B * frames, Ep), 5.0, dtype=torch.bfloat16, device=dev)
    loss = torch.zeros(1, device=dev)
    seen_offsets = set()
    for step in range(6):
        idx, off = D.draw_plan(SEED, step, B, N, CLIP, T, True, crop)
        assert (s.plan()[0].tolist(), s.plan()[1].tolist()) == (idx.tolist(), off.tolist())
        s.draw(audio, audio2, codes, 256, onehot)
        s.draw(audio, onehot=cond, onehot_rows=frames, onehot_col0=lat)
        loss.fill_(step + 0.5)
        s.log_step(loss)
        s.step += 1
        want = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
        assert s.indices.cpu().numpy().tolist() == idx.tolist(), step
        assert np.array_equal(audio.cpu().numpy().view(np.uint32), want.view(np.uint32)), step
        assert torch.equal(audio2, audio)
        assert torch.equal(codes.view(B, T), K.mu_law_encode(torch.as_tensor(want, device=dev), 256)), step
        oh = _onehot(LABELS[idx], NC)
        assert np.array_equal(onehot.cpu().numpy(), oh), step
        c = cond.float().cpu().numpy().reshape(B, frames, Ep)
        assert np.array_equal(c[:, :, lat:lat + NC], np.repeat(oh[:, None, :], frames, 1)), step
        assert (c[:, :, :lat] == 5.0).all() and (c[:, :, lat + NC:] == 5.0).all(), "columns outside the condition block"
        seen_offsets |= set(off.tolist())
    # both out-of-range labels were drawn (their rows are zero), and the random crop moved
    drawn = np.concatenate([D.draw_plan(SEED, st, B, N, CLIP, T, True, crop)[0] for st in range(6)])
    assert {2, 5} <= set(drawn.tolist())
    assert seen_offsets == {0} if (crop == "head" or T == CLIP) else len(seen_offsets) > 1
    # the ring of 4 holds steps 4, 5, 2, 3; the device counter stands at 6
    assert s.state.cpu().tolist() == [SEED, 6]
    assert s.log.cpu().tolist() == [4.5, 5.5, 2.5, 3.5]
    assert s.losses(2, 4).tolist() == [2.5, 3.5, 4.5, 5.5]


def test_draw_without_shuffle_and_per_rank():
    D = sub("dataset")
    clips = _clips()
    ds = _dataset(labels=False)
    audio = torch.zeros((B, 61), device="cuda")
    loss = torch.zeros(1, device="cuda")
    for kw in (dict(shuffle=False), dict(rank=1, world=2, crop="random")):
        s = ds.sampler(B, 61, seed=SEED, **kw)
        for step in range(4):
            idx, off = s.plan()
            s.draw(audio)
            s.log_step(loss)
            s.step += 1
            assert s.indices.cpu().numpy().tolist() == idx.tolist()
            assert np.array_equal(audio.cpu().numpy(), np.stack([clips[i, o:o + 61] for i, o in zip(idx, off)]))
        if not kw.get("world"):
            assert s.plan(0)[0].tolist() == [0, 1, 2] and s.plan(2)[0].tolist() == [6, 0, 1]


def test_draw_rows_longer_than_a_workgroups_share():
    """Rows of 8197 samples are three workgroups each (4096 + 4096 + 5): the shares' own heads and tails, at offsets that
    leave source and destination aligned differently."""
    D, K = sub("dataset"), sub("kernels")
    n, clip, T, batch = 3, 9001, 8197, 2
    clips = np.random.default_rng(4).uniform(-1, 1, (n, clip)).astype(np.float32)
    s = D.DeviceDataset(clips).sampler(batch, T, seed=SEED, crop="random")
    audio = torch.full((batch, T), 9.0, device="cuda")
    audio2 = torch.full((batch, T), 9.0, device="cuda")
    codes = torch.full((batch * T,), -7, dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    for step in range(3):
        idx, off = s.plan()
        s.draw(audio, audio2, codes, 256)
        s.log_step(loss)
        s.step += 1
        want = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
        assert s.indices.cpu().numpy().tolist() == idx.tolist()
        assert np.array_equal(audio.cpu().numpy(), want) and torch.equal(audio2, audio), step
        assert torch.equal(codes.view(batch, T), K.mu_law_encode(torch.as_tensor(want, device="cuda"), 256)), step


# ---- fit == the host loop ----------------------------------------------------------------------------------------------
def _teacher(dtype, head="softmax", T=64):
    M = sub("model")
    return M.WaveNetTeacher(T, 0, DIL, dilation_channels=R, skip_channels=S, quantization_channels=256, dtype=dtype,
                            learning_rate=1e-3, head=head, seed=5)


def _classifier():
    M = sub("model")
    return M.WaveNet(64, NC, DIL, dilation_channels=R, skip_channels=S, output_channels=NC, learning_rate=1e-3,
                     dtype=torch.float32, seed=5)


def _autoencoder():
    M = sub("model")
    return M.WaveNetAutoEncoder(64, NC, 5, DIL, dilation_channels=R, skip_channels=S, latent_channels=8, pool_stride=16,
                                learning_rate=1e-3, dtype=torch.bfloat16, seed=5)


def _host_step(kind, m, x, labels):
    if kind == "classifier":
        return m.train(x, _onehot(labels, NC))
    if kind == "autoencoder":
        return m.train(x, _onehot(labels, NC))
    return m.train(x)


KINDS = {
    "teacher_fp32": (lambda: _teacher(torch.float32), B, "random", False),
    "teacher_bf16": (lambda: _teacher(torch.bfloat16), B, "random", False),
    "teacher_mol": (lambda: _teacher(torch.float32, head="mol"), B, "head", False),
    "classifier": (_classifier, B, "random", True),
    "autoencoder": (_autoencoder, 2, "random", True),
}


def _host_loop(kind, steps, first=0, model=None):
    """`steps` steps of train(x) over the plan's batches from step `first`: (model, losses)."""
    D = sub("dataset")
    make, batch, crop, _ = KINDS[kind]
    clips = _clips()
    m = model or make()
    losses = []
    for st in range(first, first + steps):
        idx, off = D.draw_plan(SEED, st, batch, N, CLIP, 64, True, crop)
        x = np.stack([clips[i, o:o + 64] for i, o in zip(idx, off)])
        losses.append(_host_step(kind, m, x, LABELS[idx]))
    return m, np.array(losses, np.float32)


def _sampler(kind, **kw):
    _, batch, crop, labels = KINDS[kind]
    return _dataset(labels).sampler(batch, 64, seed=SEED, crop=crop, **kw)


@pytest.mark.parametrize("kind", ["teacher_bf16", "teacher_mol", "classifier", "autoencoder"])
def test_fit_equals_the_host_loop(kind):
    """Six steps: two eager, the capture, replays -- against train(x) over the same batches on an identically seeded
    model.  No tolerance: the draw writes the bits set_inputs writes, and the step between is the same launches."""
    ref, want = _host_loop(kind, 6)
    m = KINDS[kind][0]()
    s = _sampler(kind)
    got = m.fit(s, 6)
    assert got.dtype == np.float32 and got.shape == (6,)
    print(kind, "fit", got.tolist(), "host loop", want.tolist())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _same(_params(m), _params(ref))
    assert s.step == 6 and s.state.cpu().tolist()[1] == 6


@pytest.fixture(scope="module")
def host_fp32():
    """The fp32 softmax teacher's host loop, once: the losses of 10 steps, the parameters after 6 and after 10."""
    m, l6 = _host_loop("teacher_fp32", 6)
    p6 = _params(m)
    _, l4 = _host_loop("teacher_fp32", 4, first=6, model=m)
    return dict(losses=np.concatenate([l6, l4]), p6=p6, p10=_params(m))


def test_fit_equals_the_host_loop_fp32(host_fp32):
    m = _teacher(torch.float32)
    got = m.fit(_sampler("teacher_fp32"), 6)
    assert np.array_equal(got.view(np.uint32), host_fp32["losses"][:6].view(np.uint32))
    _same(_params(m), host_fp32["p6"])


def test_fit_continues(host_fp32):
    m = _teacher(torch.float32)
    s = _sampler("teacher_fp32")
    got = np.concatenate([m.fit(s, 3), m.fit(s, 3), m.fit(s, 0)])
    assert np.array_equal(got.view(np.uint32), host_fp32["losses"][:6].view(np.uint32))
    _same(_params(m), host_fp32["p6"])


def test_fit_with_eager_launches(host_fp32, monkeypatch):
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    m = _teacher(torch.float32)
    got = m.fit(_sampler("teacher_fp32"), 6)
    assert m._engine(B, 64)._fit_state["graphs"] is None
    assert np.array_equal(got.view(np.uint32), host_fp32["losses"][:6].view(np.uint32))
    _same(_params(m), host_fp32["p6"])


def test_fit_with_the_step_cut_at_the_all_reduce(host_fp32, monkeypatch):
    """SRWN_FORCE_DIST=1 (one rank): {draw, forward, backward} and {Adam, re-pack, log} as two graphs with the all-reduce's
    place between them, the form a data-parallel engine replays."""
    monkeypatch.setenv("SRWN_FORCE_DIST", "1")
    m = _teacher(torch.float32)
    got = m.fit(_sampler("teacher_fp32"), 6)
    assert len(m._engine(B, 64)._fit_state["graphs"]) == 2
    assert np.array_equal(got.view(np.uint32), host_fp32["losses"][:6].view(np.uint32))
    _same(_params(m), host_fp32["p6"])


def test_fit_drains_a_short_ring(host_fp32):
    m = _teacher(torch.float32)
    s = _sampler("teacher_fp32", log_capacity=4)
    got = m.fit(s, 10)
    assert m._engine(B, 64)._fit_state["graphs"] is not None
    assert np.array_equal(got.view(np.uint32), host_fp32["losses"].view(np.uint32))
    _same(_params(m), host_fp32["p10"])


def test_train_and_fit_mix_on_one_model(host_fp32):
    # fit, then train(x): the host loop takes over at step 3
    m = _teacher(torch.float32)
    got = m.fit(_sampler("teacher_fp32"), 3)
    _, rest = _host_loop("teacher_fp32", 3, first=3, model=m)
    assert np.array_equal(np.concatenate([got, rest]).view(np.uint32), host_fp32["losses"][:6].view(np.uint32))
    _same(_params(m), host_fp32["p6"])
    # train(x) (its two eager steps, its own capture, a replay), then fit from step 3, then train(x) replays again
    m, first = _host_loop("teacher_fp32", 3)
    s = _sampler("teacher_fp32")
    s.seek(3)
    got = m.fit(s, 3)
    assert np.array_equal(np.concatenate([first, got]).view(np.uint32), host_fp32["losses"][:6].view(np.uint32))
    _same(_params(m), host_fp32["p6"])
    _, rest = _host_loop("teacher_fp32", 4, first=6, model=m)
    assert np.array_equal(rest.view(np.uint32), host_fp32["losses"][6:].view(np.uint32))
    _same(_params(m), host_fp32["p10"])


def _three_ways(rounds=4):
    """`rounds` rounds of {train(x) on a host batch, fit(sampler, 1), evaluate(eval_sampler)} on one classifier, all three
    on its engine of shape (B, 64): (model, engine, train losses, fit losses, the EvalResults' arrays, parameters)."""
    D = sub("dataset")
    m, clips = _classifier(), _clips()
    s = _sampler("classifier")
    ev = D.DeviceDataset(clips, np.abs(LABELS) % NC, NC).eval_sampler(B, 64)
    trained, fitted, swept = [], [], []
    for r in range(rounds):
        idx = (np.arange(B) + r) % N
        trained.append(m.train(clips[idx, :64], _onehot(LABELS[idx], NC)))
        fitted.append(m.fit(s, 1))
        res = m.evaluate(ev)
        swept.append([np.asarray(a) for a in (res.pred, res.rank, res.nll, res.confusion, res.owned)])
    return (m, m._engine(B, 64), np.array(trained, np.float32), np.concatenate(fitted), swept, _params(m))


def test_train_fit_and_evaluate_capture_each_their_own(monkeypatch):
    """train(x), fit and evaluate interleaved on one engine: each counts its own two eager steps and captures graphs of its
    own behind them, and every loss, every sweep's arrays and the final parameters are those of the same rounds under
    SRWN_MODEL_GRAPHS=0, bit for bit."""
    m, eng, trained, fitted, swept, params = _three_ways()
    assert eng._graph_ready is True
    assert eng._fit_state["graphs"] is not None and len(eng._fit_state["graphs"]) == 1
    assert eng._eval_state["graph"] is not None
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    m0, eng0, trained0, fitted0, swept0, params0 = _three_ways()
    assert not getattr(eng0, "_graph_ready", False)
    assert eng0._fit_state["graphs"] is None and eng0._eval_state["graph"] is None
    print("train", trained.tolist(), trained0.tolist(), "fit", fitted.tolist(), fitted0.tolist())
    assert np.array_equal(trained.view(np.uint32), trained0.view(np.uint32))
    assert fitted.shape == (4,) and np.array_equal(fitted.view(np.uint32), fitted0.view(np.uint32))
    for got, want in zip(swept, swept0):
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    _same(params, params0)


def test_fit_refuses_what_the_model_does_not_accept():
    m = _classifier()
    with pytest.raises(ValueError, match="holds no labels"):
        m.fit(_dataset(labels=False).sampler(B, 64), 1)
    with pytest.raises(ValueError, match="input_size=64"):
        m.fit(_dataset().sampler(B, 61), 1)
    ae = _autoencoder()
    ae.fit(_sampler("autoencoder"), 1)
    with pytest.raises(NotImplementedError, match=r"one \(batch, length\) per model object"):
        ae.fit(_dataset().sampler(3, 64), 1)


# ---- TFRecord loading --------------------------------------------------------------------------------------------------
def test_from_tfrecord(tmp_path):
    from tests.test_tfrecord import example, nsynth_example, record
    D, NS = sub("dataset"), sub("nsynth")
    rng = np.random.default_rng(0)
    path = str(tmp_path / "clips.tfrecord")
    with open(path, "wb") as f:
        for i in range(5):
            f.write(record(example(nsynth_example(i, CLIP, rng))))
    tf = NS.TFRecordFile(path)
    audio, pitch = tf.batch(np.arange(5), CLIP, CLIP, "pitch")
    ds = D.DeviceDataset.from_tfrecord(path, CLIP, piece=2)
    assert len(ds) == 5 and ds.clip_len == CLIP and ds.num_classes == 128
    assert np.array_equal(ds.audio.cpu().numpy().view(np.uint32), audio.view(np.uint32))
    assert ds.labels.dtype == torch.int32 and ds.labels.cpu().numpy().tolist() == pitch.tolist()
    short = D.DeviceDataset.from_tfrecord(path, CLIP, label_key=None, limit=3)
    assert len(short) == 3 and short.labels is None and short.num_classes == 0
    assert np.array_equal(short.audio.cpu().numpy(), audio[:3])


# ---- the example driver ------------------------------------------------------------------------------------------------
def test_teacher_example_with_device_data(tmp_path):
    """examples/teacher.py --device-data on a block of synthetic waves: fit between the prints, checkpoints written."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_teacher", os.path.join(root, "examples", "teacher.py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    tdir = str(tmp_path / "t")
    try:
        loss = ex.main(["--teacher", tdir, "--steps", "5", "--batch-size", "2", "--num-samples", "1024", "--pool-stride", "64",
                        "--latent-channels", "8", "--layers", "6", "--print-steps", "3", "--device-data", "--device-clips", "5"])
        assert np.isfinite(loss) and os.path.exists(os.path.join(tdir, "checkpoint"))
    finally:
        for m in ("model", "ops", "nsynth", "simple_audio"):
            sys.modules.pop(m, None)
        d = os.path.join(root, "sr-wavenet_amd", "dropin")
        while d in sys.path:
            sys.path.remove(d)
