"""GPU tests of ``fit`` on the student and on the twin towers: against the host loops of examples/student.py
(``encode``, logistic noise, ``train_fast``) and examples/siamese.py (``train`` on pairs) over the plans' batches, bit for
bit -- losses, power losses / distances and every parameter tensor --, continuation, eager launches, rings shorter than the
run, ``train_fast`` and ``fit`` mixed on one model, the frozen teacher, and the two ``--device-data`` drivers.

Student: 7 clips of 800 samples, B = 2, T = 768 (two STFT frames), two flows of three layers [1, 2, 4] at R = 32, S = 128,
latent 8, pool_stride 64, on a WaveNetAutoEncoder of the same stack saved to and loaded from a directory.  Twins: the 9
labelled records of tests/test_draw_plans.py, P = 3, T = 64, D = 2."""
import os
import sys

import numpy as np
import pytest
import torch

from tests._pkg import sub

pytestmark = pytest.mark.gpu

SEED = 3
DIL, R, S = [1, 2, 4], 32, 128
N, CLIP, B, T, LAT, POOL, NC = 7, 800, 2, 768, 8, 64, 4
LABELS7 = np.array([0, 3, -1, 1, 2, NC, 3], np.int64)          # labels 2 and 5 lie outside the classes: zero conditions
LABELS9 = np.array([0, 1, 0, 2, 1, 0, 3, 1, 0], np.int64)
P, TP, CLIP9 = 3, 64, 70


def _clips(n, length):
    rng = np.random.default_rng(11)
    return (0.9 * np.sin(np.arange(length)[None, :] * rng.uniform(0.05, 0.6, (n, 1))) *
            rng.uniform(0.2, 1.0, (n, 1)) + 0.02 * rng.standard_normal((n, length))).astype(np.float32)


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


# ---- the student -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teacher_dirs(tmp_path_factory):
    """One saved WaveNetAutoEncoder per (dtype, condition_size)."""
    M = sub("model")
    out = {}
    for dtype in (torch.float32, torch.bfloat16):
        for cs in (0, NC):
            d = str(tmp_path_factory.mktemp("teacher"))
            t = M.WaveNetAutoEncoder(T, cs, 5, DIL, dilation_channels=R, skip_channels=S, latent_channels=LAT,
                                     pool_stride=POOL, learning_rate=1e-3, dtype=dtype, seed=5)
            t._engine(B, T)
            t.save(d, 0, force=True)
            out[dtype, cs] = d
            del t
    return out


def _student(teacher_dirs, dtype, cs):
    M = sub("model")
    return M.ParallelWaveNet(T, cs, DIL, teacher_dirs[dtype, cs], num_flows=2, dilation_channels=R, skip_channels=S,
                             latent_channels=LAT, pool_stride=POOL, learning_rate=1e-3, dtype=dtype, seed=7)


def _student_sampler(cs, **kw):
    D = sub("dataset")
    ds = D.DeviceDataset(_clips(N, CLIP), LABELS7 if cs else None, NC if cs else 0)
    return ds.distill_sampler(B, T, seed=SEED, crop="random", **kw)


def _noise(step):
    """The step's noise as the host loop gets it: the plan's bits through the device's own logistic map."""
    D, K = sub("dataset"), sub("kernels")
    k = D.noise_plan(SEED, step, B, T)
    bits = torch.as_tensor(k.astype(np.int64), device="cuda").to(torch.int32).contiguous()
    out = torch.empty((B, T), device="cuda")
    K.call("srwn_logistic_from_bits", bits.data_ptr(), out.data_ptr(), bits.numel(), K._stream())
    return out.cpu().numpy()


def _student_host_loop(teacher_dirs, dtype, cs, steps, first=0, model=None):
    """examples/student.py's loop over the plans' batches from step `first`: (model, losses, power losses)."""
    D = sub("dataset")
    clips = _clips(N, CLIP)
    m = model or _student(teacher_dirs, dtype, cs)
    loss, power = [], []
    for st in range(first, first + steps):
        idx, off = D.draw_plan(SEED, st, B, N, CLIP, T, True, "random")
        x = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
        c = _onehot(LABELS7[idx], NC) if cs else None
        enc = m.encode(None, x, c)
        l, p = m.train_fast(None, _noise(st), x, enc, c)
        loss.append(l); power.append(p)
    return m, np.array(loss, np.float32), np.array(power, np.float32)


@pytest.fixture(scope="module")
def student_host(teacher_dirs):
    """Host loops, once per (dtype, condition_size): losses and parameters after 6 steps, and the same from a second,
    identically seeded run (the precondition of every comparison below)."""
    cache = {}

    def get(dtype, cs):
        if (dtype, cs) not in cache:
            m, l, p = _student_host_loop(teacher_dirs, dtype, cs, 6)
            m2, l2, p2 = _student_host_loop(teacher_dirs, dtype, cs, 6)
            cache[dtype, cs] = dict(loss=l, power=p, p6=_params(m), again=(l2, p2, _params(m2)), model=m)
        return cache[dtype, cs]
    return get


def _reproducible(h):
    """Two identically seeded host loops agree bit for bit: without that no fit can be held to one of them."""
    l2, p2, params2 = h["again"]
    assert np.array_equal(_bits(h["loss"]), _bits(l2)) and np.array_equal(_bits(h["power"]), _bits(p2)), \
        "the student step is not reproducible: %s vs %s" % (h["loss"].tolist(), l2.tolist())
    _same(h["p6"], params2)


@pytest.mark.parametrize("cs", [0, NC], ids=["plain", "conditioned"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_student_fit_equals_the_host_loop(teacher_dirs, student_host, dtype, cs):
    """Six steps: two eager, the capture, replays."""
    h = student_host(dtype, cs)
    _reproducible(h)
    m = _student(teacher_dirs, dtype, cs)
    m._engine(B, T)
    frozen = _params(m._teacher)
    s = _student_sampler(cs)
    loss, power = m.fit(s, 6)
    assert loss.dtype == np.float32 and loss.shape == (6,) and power.dtype == np.float32 and power.shape == (6,)
    print("fit", loss.tolist(), power.tolist(), "host loop", h["loss"].tolist(), h["power"].tolist())
    assert np.array_equal(_bits(loss), _bits(h["loss"]))
    assert np.array_equal(_bits(power), _bits(h["power"]))
    _same(_params(m), h["p6"])
    _same(_params(m._teacher), frozen)                   # the teacher's parameters have not moved
    assert s.step == 6 and s.state.cpu().tolist()[1] == 6
    assert m._engine(B, T)._fit_state["graphs"] is not None
    # the entropy ring: losses()'s entropy of the last step, which the loss is made of
    ent = s.entropies(0, 6)
    assert ent.dtype == np.float32 and np.isfinite(ent).all()
    eng = m._engine(B, T)
    assert ent[5] == np.float32(float(eng.logs.item()) + 2.0 * eng.N)


def test_student_fit_continues(teacher_dirs, student_host):
    h = student_host(torch.float32, 0)
    _reproducible(h)
    m = _student(teacher_dirs, torch.float32, 0)
    s = _student_sampler(0)
    parts = [m.fit(s, 3), m.fit(s, 3), m.fit(s, 0)]
    assert parts[2][0].shape == (0,) and parts[2][1].shape == (0,)
    assert np.array_equal(_bits(np.concatenate([p[0] for p in parts])), _bits(h["loss"]))
    assert np.array_equal(_bits(np.concatenate([p[1] for p in parts])), _bits(h["power"]))
    _same(_params(m), h["p6"])


def test_student_fit_with_eager_launches(teacher_dirs, student_host, monkeypatch):
    h = student_host(torch.float32, 0)
    _reproducible(h)
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    m = _student(teacher_dirs, torch.float32, 0)
    loss, power = m.fit(_student_sampler(0), 6)
    assert m._engine(B, T)._fit_state["graphs"] is None
    assert np.array_equal(_bits(loss), _bits(h["loss"])) and np.array_equal(_bits(power), _bits(h["power"]))
    _same(_params(m), h["p6"])


def test_student_fit_drains_a_short_ring(teacher_dirs, student_host):
    h = student_host(torch.float32, 0)
    _reproducible(h)
    m = _student(teacher_dirs, torch.float32, 0)
    loss, power = m.fit(_student_sampler(0, log_capacity=4), 6)
    assert np.array_equal(_bits(loss), _bits(h["loss"])) and np.array_equal(_bits(power), _bits(h["power"]))
    _same(_params(m), h["p6"])


def test_student_train_fast_and_fit_mix_on_one_model(teacher_dirs, student_host):
    h = student_host(torch.float32, 0)
    _reproducible(h)
    # fit, then the host loop takes over at step 3
    m = _student(teacher_dirs, torch.float32, 0)
    loss, power = m.fit(_student_sampler(0), 3)
    _, l2, p2 = _student_host_loop(teacher_dirs, torch.float32, 0, 3, first=3, model=m)
    assert np.array_equal(_bits(np.concatenate([loss, l2])), _bits(h["loss"]))
    assert np.array_equal(_bits(np.concatenate([power, p2])), _bits(h["power"]))
    _same(_params(m), h["p6"])
    # the host loop (its two eager steps, its own capture, a replay), then fit from step 3
    m, l1, p1 = _student_host_loop(teacher_dirs, torch.float32, 0, 3)
    s = _student_sampler(0)
    s.seek(3)
    loss, power = m.fit(s, 3)
    assert np.array_equal(_bits(np.concatenate([l1, loss])), _bits(h["loss"]))
    assert np.array_equal(_bits(np.concatenate([p1, power])), _bits(h["power"]))
    _same(_params(m), h["p6"])


def test_student_fit_refusals(teacher_dirs):
    D, M = sub("dataset"), sub("model")
    m = _student(teacher_dirs, torch.float32, NC)
    with pytest.raises(ValueError, match="holds no labels"):
        m.fit(_student_sampler(0), 1)
    plain = D.DeviceDataset(_clips(N, CLIP)).sampler(B, T)
    with pytest.raises(NotImplementedError, match="noise and teacher passes"):
        m.fit(plain, 1)
    # a decoder-only mixture-of-logistics teacher has no encoder
    t = M.WaveNetTeacher(T, 0, DIL, dilation_channels=R, skip_channels=S, head="mol", use_encoding=True,
                         latent_channels=LAT, pool_stride=POOL, dtype=torch.float32, seed=5)
    st = M.ParallelWaveNet(T, 0, DIL, t, num_flows=2, dilation_channels=R, skip_channels=S, latent_channels=LAT,
                           pool_stride=POOL, dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="decoder-only teacher has no encoder"):
        st.fit(_student_sampler(0), 1)


# ---- the twins ---------------------------------------------------------------------------------------------------------
def _twins(dtype):
    M = sub("model")
    return M.SiameseWaveNet(TP, 2, DIL, dilation_channels=R, skip_channels=S, learning_rate=1e-3, dtype=dtype, seed=5)


def _pair_sampler(**kw):
    D = sub("dataset")
    return D.DeviceDataset(_clips(9, CLIP9), LABELS9, NC).pair_sampler(P, TP, seed=SEED, crop="random", **kw)


def _twins_host_loop(dtype, steps, first=0, model=None):
    D = sub("dataset")
    clips = _clips(9, CLIP9)
    m = model or _twins(dtype)
    loss, dist = [], []
    for st in range(first, first + steps):
        left, right, ol, orr, y = D.pair_plan(SEED, st, P, LABELS9, NC, CLIP9, TP, 0.5, True, "random")
        xl = np.stack([clips[i, o:o + TP] for i, o in zip(left, ol)])
        xr = np.stack([clips[i, o:o + TP] for i, o in zip(right, orr)])
        l, d = m.train(None, xl, xr, y)
        loss.append(l); dist.append(d)
    return m, np.array(loss, np.float32), np.array(dist, np.float32).reshape(steps, P)


@pytest.fixture(scope="module")
def twins_host():
    cache = {}

    def get(dtype):
        if dtype not in cache:
            m, l, d = _twins_host_loop(dtype, 6)
            cache[dtype] = dict(loss=l, dist=d, p6=_params(m))
        return cache[dtype]
    return get


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_twins_fit_equals_the_host_loop(twins_host, dtype):
    h = twins_host(dtype)
    m = _twins(dtype)
    s = _pair_sampler()
    loss, dist = m.fit(s, 6)
    assert loss.dtype == np.float32 and loss.shape == (6,) and dist.dtype == np.float32 and dist.shape == (6, P)
    print("fit", loss.tolist(), "host loop", h["loss"].tolist())
    assert np.array_equal(_bits(loss), _bits(h["loss"]))
    assert np.array_equal(_bits(dist), _bits(h["dist"]))
    _same(_params(m), h["p6"])
    assert s.step == 6 and s.state.cpu().tolist()[1] == 6
    assert m._engine(2 * P, TP)._fit_state["graphs"] is not None
    left, right, _, _, y = s.pair_plan(5)                 # the sampler's buffers hold the last draw
    assert s.indices.cpu().tolist() == left.tolist() and s.right.cpu().tolist() == right.tolist()
    assert s.y.cpu().tolist() == y.tolist()


def test_twins_fit_continues_through_a_short_ring(twins_host):
    h = twins_host(torch.float32)
    m = _twins(torch.float32)
    s = _pair_sampler(log_capacity=2)
    parts = [m.fit(s, 3), m.fit(s, 3), m.fit(s, 0)]
    assert parts[2][0].shape == (0,) and parts[2][1].shape == (0, P)
    assert np.array_equal(_bits(np.concatenate([p[0] for p in parts])), _bits(h["loss"]))
    assert np.array_equal(_bits(np.concatenate([p[1] for p in parts])), _bits(h["dist"]))
    _same(_params(m), h["p6"])


def test_twins_fit_with_eager_launches_then_train(twins_host, monkeypatch):
    h = twins_host(torch.float32)
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    m = _twins(torch.float32)
    loss, dist = m.fit(_pair_sampler(), 3)
    assert m._engine(2 * P, TP)._fit_state["graphs"] is None
    _, l2, d2 = _twins_host_loop(torch.float32, 3, first=3, model=m)      # train() takes over at step 3
    assert np.array_equal(_bits(np.concatenate([loss, l2])), _bits(h["loss"]))
    assert np.array_equal(_bits(np.concatenate([dist, d2])), _bits(h["dist"]))
    _same(_params(m), h["p6"])


def test_twins_fit_refusals():
    D = sub("dataset")
    m = _twins(torch.float32)
    ds = D.DeviceDataset(_clips(9, CLIP9), LABELS9, NC)
    with pytest.raises(NotImplementedError, match="pairs of clips and their labels"):
        m.fit(ds.sampler(P, TP), 1)
    with pytest.raises(ValueError, match="input_size=64"):
        m.fit(ds.pair_sampler(P, 61), 1)


# ---- the example drivers -----------------------------------------------------------------------------------------------
def _example(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_" + name, os.path.join(root, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    return ex, root


def _forget_dropin(root):
    for m in ("model", "ops", "nsynth", "simple_audio"):
        sys.modules.pop(m, None)
    d = os.path.join(root, "sr-wavenet_amd", "dropin")
    while d in sys.path:
        sys.path.remove(d)


def test_student_example_with_device_data(tmp_path):
    """examples/teacher.py writes a small teacher; examples/student.py --device-data distils against it."""
    tdir, sdir = str(tmp_path / "t"), str(tmp_path / "s")
    shape = ["--batch-size", "2", "--num-samples", "1024", "--pool-stride", "64", "--latent-channels", "8", "--layers", "6"]
    ex, root = _example("teacher")
    try:
        ex.main(["--teacher", tdir, "--steps", "2", "--print-steps", "2"] + shape)
        ex, root = _example("student")
        loss = ex.main(["--teacher", tdir, "--student", sdir, "--steps", "5", "--print-steps", "3", "--flows", "2",
                        "--device-data", "--device-clips", "5"] + shape)
        assert np.isfinite(loss) and os.path.exists(os.path.join(sdir, "checkpoint"))
    finally:
        _forget_dropin(root)


def test_siamese_example_with_device_data(tmp_path):
    ex, root = _example("siamese")
    try:
        loss = ex.main(["--train", "--device-data", "--logdir", str(tmp_path / "tw"), "--steps", "5", "--print-steps", "3",
                        "--batch-size", "2", "--num-samples", "512", "--layers", "6", "--device-clips", "12", "--seed", "1"])
        assert np.isfinite(loss) and os.path.exists(os.path.join(str(tmp_path / "tw"), "checkpoint"))
    finally:
        _forget_dropin(root)
