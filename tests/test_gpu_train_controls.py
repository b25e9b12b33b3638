"""GPU tests of the training controls end to end, for the five trainable models: with no controls nothing changes (bits and
launch lists); ``fit`` under a piecewise schedule + clipping + EMA equals a host loop built only from entry points older
than the controls; ``ema_weights()`` serves the averaged weights and leaves no trace; ``validate_ema``; resuming from
``save`` + ``save_training_state``; the table rewritten in place under a captured graph.

Shapes: stacks of three layers [1, 2, 4] at R = 32, S = 128; B = 2, T = 256; 5 classes for the classifier; the auto-encoder
at encoder channels 128, latent 8, pool stride 64; the student with two flows at T = 768 (its loss needs a 512-sample STFT
frame); the twins with 2 pairs and D = 2.  8 steps -- two eager, the capture, replays -- on a table of 6 rows, so the last
steps keep its last row, with rings of 4 losses, so a drain falls inside the run."""
import contextlib

import numpy as np
import pytest
import torch

from tests._pkg import sub
from tests.opt_reference import ctl_row

pytestmark = pytest.mark.gpu

SEED = 3
DIL, R, S = [1, 2, 4], 32, 128
B, T, C = 2, 256, 5
N, CLIP = 7, 300
LAT, POOL, EC = 8, 64, 128
ST, SCLIP = 768, 800
P, D2 = 2, 2
LABELS = np.arange(N) % C
STEPS, HORIZON, RING = 8, 6, 4
DECAY = 0.9
KINDS = ["classifier", "teacher", "autoencoder", "student", "twins"]
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def _clips(n, length, seed=11):
    rng = np.random.default_rng(seed)
    return (0.9 * np.sin(np.arange(length)[None, :] * rng.uniform(0.05, 0.6, (n, 1))) *
            rng.uniform(0.2, 1.0, (n, 1)) + 0.02 * rng.standard_normal((n, length))).astype(np.float32)


def _onehot(labels, width):
    out = np.zeros((len(labels), width), np.float32)
    out[np.arange(len(labels)), labels] = 1.0
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _schedule():
    return sub("optim").piecewise([1, 3], [3e-3, 1e-3, 3e-4])


# ---- one harness per model: how to build it, feed ``fit`` and make the same step from the host -------------------------------
class Harness:
    def __init__(self, kind, dtype, tmp):
        self.kind, self.dtype, self.tmp = kind, dtype, tmp
        self._teacher_dir = None

    def model(self):
        M = sub("model")
        kw = dict(dilation_channels=R, skip_channels=S, learning_rate=1e-3, dtype=self.dtype)
        if self.kind == "classifier":
            return M.WaveNet(T, C, DIL, output_channels=C, seed=5, **kw)
        if self.kind == "teacher":
            return M.WaveNetTeacher(T, 0, DIL, seed=5, **kw)
        if self.kind == "autoencoder":
            return M.WaveNetAutoEncoder(T, 0, 5, DIL, encoder_channels=EC, latent_channels=LAT, pool_stride=POOL, seed=5, **kw)
        if self.kind == "twins":
            return M.SiameseWaveNet(T, D2, DIL, margin=1.0, seed=5, **kw)
        if self._teacher_dir is None:
            t = M.WaveNetAutoEncoder(ST, 0, 5, DIL, encoder_channels=EC, latent_channels=LAT, pool_stride=POOL, seed=5, **kw)
            t._engine(B, ST)
            self._teacher_dir = str(self.tmp.mktemp("teacher"))
            t.save(self._teacher_dir, 0, force=True)
        return M.ParallelWaveNet(ST, 0, DIL, self._teacher_dir, num_flows=2, latent_channels=LAT, pool_stride=POOL, seed=7, **kw)

    def sampler(self, **kw):
        D = sub("dataset")
        if self.kind == "student":
            return D.DeviceDataset(_clips(N, SCLIP)).distill_sampler(B, ST, seed=SEED, crop="random", **kw)
        ds = D.DeviceDataset(_clips(N, CLIP), LABELS, C)
        if self.kind == "twins":
            return ds.pair_sampler(P, T, seed=SEED, crop="random", **kw)
        return ds.sampler(B, T, seed=SEED, crop="random", **kw)

    def fit(self, m, s, steps):
        out = m.fit(s, steps)
        return out if isinstance(out, np.ndarray) else out[0]

    def engine(self, m):
        if self.kind == "student":
            return m._engine(B, ST)
        return m._engine(2 * P if self.kind == "twins" else B, T)

    def train(self, m, step):
        """``train`` on the batch ``fit`` draws at `step` (the samplers' plans): the loss, float32."""
        D = sub("dataset")
        if self.kind == "twins":
            clips = _clips(N, CLIP)
            left, right, ol, orr, y = D.pair_plan(SEED, step, P, LABELS, C, CLIP, T, 0.5, True, "random")
            xl = np.stack([clips[i, o:o + T] for i, o in zip(left, ol)])
            xr = np.stack([clips[i, o:o + T] for i, o in zip(right, orr)])
            return m.train(None, xl, xr, y)[0]
        if self.kind == "student":
            clips = _clips(N, SCLIP)
            idx, off = D.draw_plan(SEED, step, B, N, SCLIP, ST, True, "random")
            x = np.stack([clips[i, o:o + ST] for i, o in zip(idx, off)])
            K = sub("kernels")
            k = D.noise_plan(SEED, step, B, ST)
            bits = torch.as_tensor(k.astype(np.int64), device="cuda").to(torch.int32).contiguous()
            noise = torch.empty((B, ST), device="cuda")
            K.call("srwn_logistic_from_bits", bits.data_ptr(), noise.data_ptr(), bits.numel(), K._stream())
            return m.train_fast(None, noise.cpu().numpy(), x, m.encode(None, x), None)[0]
        clips = _clips(N, CLIP)
        idx, off = D.draw_plan(SEED, step, B, N, CLIP, T, True, "random")
        x = np.stack([clips[i, o:o + T] for i, o in zip(idx, off)])
        if self.kind == "classifier":
            return m.train(x, _onehot(LABELS[idx], C))
        return m.train(x)

    def state(self, m):
        """Every optimizer's params, m, v, step -- and the shadow where there is one --, cloned."""
        out = {}
        for name, (eng, params, am, av, step, ctl) in m._optimizers().items():
            out[name] = dict(params=params.clone(), m=am.clone(), v=av.clone(), step=step.clone())
            if ctl.ema is not None:
                out[name]["ema"] = ctl.ema.clone()
        return out


def _same_state(a, b, keys=None):
    assert set(a) == set(b)
    for name in a:
        for k in (keys or a[name]):
            assert torch.equal(a[name][k].view(torch.uint8), b[name][k].view(torch.uint8)), (name, k)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cache = {}

    def get(kind, dtype):
        if (kind, dtype) not in cache:
            cache[kind, dtype] = Harness(kind, dtype, tmp_path_factory)
        return cache[kind, dtype]
    return get


@contextlib.contextmanager
def _recorded():
    """The names of the C entry points called, in order, through every module of the package that calls them."""
    import sys
    names, undo = [], []
    L = sub("_lib")
    real = L.call

    def rec(name, *args):
        names.append(name)
        return real(name, *args)
    for mod in list(sys.modules.values()):
        if getattr(mod, "__name__", "").startswith("sr-wavenet_amd") and getattr(mod, "call", None) is real:
            undo.append(mod)
            mod.call = rec
    try:
        yield names
    finally:
        for mod in undo:
            mod.call = real


# ---- no controls: nothing changes -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_runs(harness):
    """``fit`` for STEPS steps on a model that never heard of controls: losses, final state, the launch list of an eager
    step.  Once per (model, dtype)."""
    cache = {}

    def get(kind, dtype):
        if (kind, dtype) not in cache:
            h = harness(kind, dtype)
            m = h.model()
            h.engine(m)                                  # (built outside the recording: the step's launches only)
            s = h.sampler(log_capacity=RING)
            with _recorded() as names:
                first = h.fit(m, s, 1)
            losses = np.concatenate([first, h.fit(m, s, STEPS - 1)])
            cache[kind, dtype] = dict(losses=losses, state=h.state(m), launches=list(names))
        return cache[kind, dtype]
    return get


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_without_controls_nothing_changes(harness, plain_runs, kind, dtype):
    """A model on which controls were set and removed again runs the launches, and computes the bits, of one on which
    they never were: ``fit``, and ``train`` on the same batches."""
    h, ref = harness(kind, dtype), plain_runs(kind, dtype)
    m = h.model()
    m.set_training_controls(schedule=_schedule(), horizon=HORIZON, clip_norm=1.0, ema_decay=DECAY)
    h.engine(m)
    m.set_training_controls()
    s = h.sampler(log_capacity=RING)
    with _recorded() as names:
        first = h.fit(m, s, 1)
    losses = np.concatenate([first, h.fit(m, s, STEPS - 1)])
    assert names == ref["launches"] and "srwn_adam_step_ctl" not in names
    assert any(n in ("srwn_adam_step", "srwn_adam_step_scaled") for n in names)
    assert np.array_equal(_bits(losses), _bits(ref["losses"]))
    _same_state(h.state(m), ref["state"])
    t = h.model()                                                       # train(x) on the plans' batches
    tl = np.array([h.train(t, k) for k in range(STEPS)], np.float32)
    assert np.array_equal(_bits(tl), _bits(ref["losses"]))
    _same_state(h.state(t), ref["state"])


# ---- controls: fit == a host loop of the older entry points ---------------------------------------------------------------
def _host_loop(h, clip_norm, steps=STEPS, monkeypatch=None):
    """The twin: a model without controls whose update is made here from srwn_sumsq, srwn_clip_scale,
    srwn_adam_step_scaled at ``lr = table[row]`` and the re-pack, the EMA by three separate torch float32 operations in
    the rule's order.  Returns (losses, state with the shadows, norms [steps])."""
    K, O = sub("kernels"), sub("optim")
    table = O.control_table(_schedule(), HORIZON, DECAY)
    m = h.model()
    eng = h.engine(m)
    opts = m._optimizers()
    shadows = {name: o[1].clone() for name, o in opts.items()}
    clip = torch.zeros(2, dtype=torch.float32, device="cuda")
    parts = [torch.zeros(K.sumsq_partials(o[1].numel()), dtype=torch.float32, device="cuda") for o in opts.values()]
    allparts = torch.cat(parts)
    count = [0]
    norms = []

    def update():
        row = ctl_row(count[0] + 1, HORIZON)
        lr, d = float(table[row, 0]), table[row, 1]
        at = 0
        for (name, (e, params, am, av, step, _)), p in zip(opts.items(), parts):      # partials in consecutive slices
            K.sumsq(e.storage.grads if h.kind == "student" else e.grads, allparts[at:at + p.numel()])
            at += p.numel()
        K.clip_scale(allparts, clip_norm, 1.0, clip)
        for name, (e, params, am, av, step, _) in opts.items():
            grads = e.storage.grads if h.kind == "student" else e.grads
            K.adam_step_scaled(params, grads, am, av, step, lr, clip, True)
            s = torch.tensor(float(np.float32(1.0) - np.float32(d)), dtype=torch.float32, device="cuda")
            diff = shadows[name] - params
            prod = diff * s
            shadows[name] = shadows[name] - prod
            for f in (e.flows if h.kind == "student" else [e]):
                f.repack()
        norms.append(float(clip[1].item()))
        count[0] += 1

    eng.optimizer_step = update
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")            # (the twin's learning rate is a host scalar: no capture)
    losses = np.array([h.train(m, k) for k in range(steps)], np.float32)
    monkeypatch.delenv("SRWN_MODEL_GRAPHS")
    state = h.state(m)
    for name in state:
        state[name]["ema"] = shadows[name]
    return losses, state, np.array(norms, np.float32)


@pytest.fixture(scope="module")
def clip_norms():
    return {}


def _clip_norm(h, clip_norms, monkeypatch):
    """From a dry run without clipping (a bound no norm reaches): the median of its norms, so that some steps of the
    real run clip and some do not."""
    key = (h.kind, h.dtype)
    if key not in clip_norms:
        _, _, norms = _host_loop(h, 1e30, monkeypatch=monkeypatch)
        clip_norms[key] = float(np.median(norms.astype(np.float64)))
    return clip_norms[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_fit_under_controls_equals_the_host_loop(harness, clip_norms, kind, dtype, monkeypatch):
    h = harness(kind, dtype)
    cn = _clip_norm(h, clip_norms, monkeypatch)
    want_losses, want, norms = _host_loop(h, cn, monkeypatch=monkeypatch)
    print(kind, "clip_norm", cn, "norms", norms.tolist())
    assert (norms > cn).any() and (norms <= cn).any(), "the run must hold clipped and unclipped steps"
    m = h.model()
    m.set_training_controls(schedule=_schedule(), horizon=HORIZON, clip_norm=cn, ema_decay=DECAY)
    s = h.sampler(log_capacity=RING)
    with _recorded() as names:
        first = h.fit(m, s, 1)
    assert "srwn_adam_step_ctl" in names and "srwn_adam_step" not in names and "srwn_adam_step_scaled" not in names
    losses = np.concatenate([first, h.fit(m, s, STEPS - 1)])
    eng = h.engine(m)
    assert eng._fit_state["graphs"] is not None
    print("fit", losses.tolist(), "host loop", want_losses.tolist())
    assert np.array_equal(_bits(losses), _bits(want_losses))
    _same_state(h.state(m), want)
    assert np.float32(eng.clip[1].item()) == norms[-1]                      # the logged norm of the last step
    assert int(next(iter(m._optimizers().values()))[4].item()) == STEPS


# ---- ema_weights() ----------------------------------------------------------------------------------------------------------
def _trained(h, steps=4, **controls):
    m = h.model()
    m.set_training_controls(schedule=_schedule(), horizon=HORIZON, ema_decay=DECAY, **controls)
    s = h.sampler(log_capacity=RING)
    h.fit(m, s, steps)
    return m, s


def _with_params_of_ema(h, m):
    """A second model object whose parameters are a copy of `m`'s EMA buffers."""
    other = h.model()
    h.engine(other)
    src, dst = m._optimizers(), other._optimizers()
    for name in src:
        dst[name][1].copy_(src[name][5].ema)
    for e in ([h.engine(other)] if h.kind in ("classifier", "teacher", "twins") else []):
        e.repack(); e._repack_generation()
    if h.kind == "autoencoder":
        other._eng.dec.repack(); other._eng.dec._repack_generation(); other._eng.enc.repack()
    if h.kind == "student":
        for f in other._primary.flows:
            f.repack()
    return other


def _outputs(h, m):
    """What the model serves from its current parameters, as arrays."""
    x = _clips(B, ST if h.kind == "student" else T, seed=23)
    if h.kind == "classifier":
        ev = sub("dataset").DeviceDataset(_clips(N, CLIP, seed=29), LABELS, C).eval_sampler(3, T, seed=SEED)
        r = m.evaluate(ev)
        return [m.predict(x), r.nll, r.pred.astype(np.float32), r.confusion.astype(np.float32)]
    if h.kind == "teacher":
        return [m.get_logits(x), m.generate(2, 24, mode="argmax", seed=1).astype(np.float32), np.float32([m.loss(x)])]
    if h.kind == "autoencoder":
        return [m.encode(x), m.reconstruct(x, seed=4)]
    if h.kind == "twins":
        es = sub("dataset").DeviceDataset(_clips(N, CLIP, seed=29), LABELS, C).embed_sampler(3, T, seed=SEED)
        r = m.evaluate(es)
        return [m.get_embedding(None, x), r.emb, r.nearest.astype(np.float32)]
    enc = m.encode(None, x)
    rng = np.random.default_rng(5)
    return [m.generate(None, rng.logistic(size=(B, ST)).astype(np.float32), enc)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_ema_weights_serves_the_average_and_leaves_no_trace(harness, kind, dtype):
    h = harness(kind, dtype)
    m, s = _trained(h)
    eng = h.engine(m)
    before = h.state(m)
    for e in _image_engines(h, eng):                  # (the generation-only images follow the parameters lazily: current now)
        getattr(e, "_repack_generation", lambda: None)()
    images = [e.packed.clone() for e in _image_engines(h, eng)]
    raw = _outputs(h, m)
    other = _with_params_of_ema(h, m)
    want = _outputs(h, other)
    with m.ema_weights() as inside:
        assert inside is m
        got = _outputs(h, m)
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            h.fit(m, s, 1)
        with pytest.raises(RuntimeError):
            eng.optimizer_step()
        for name, o in m._optimizers().items():                                  # the contents moved, the pointers did not
            assert torch.equal(o[1], before[name]["ema"]) and torch.equal(o[5].ema, before[name]["params"])
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w))
    assert any(not np.array_equal(_bits(g), _bits(r)) for g, r in zip(got, raw)), "the averaged weights must serve something else"
    _same_state(h.state(m), before)
    for e, img in zip(_image_engines(h, eng), images):
        assert torch.equal(e.packed.view(torch.uint8), img.view(torch.uint8))
    for g, r in zip(_outputs(h, m), raw):
        assert np.array_equal(_bits(g), _bits(r))
    never, s2 = _trained(h)                                                        # a run that never entered the context
    l1, l2 = h.fit(m, s, 2), h.fit(never, s2, 2)
    assert np.array_equal(_bits(l1), _bits(l2))
    _same_state(h.state(m), h.state(never))


def _image_engines(h, eng):
    if h.kind == "autoencoder":
        return [eng.dec, eng.enc]
    if h.kind == "student":
        return list(eng.flows)
    return [eng]


def test_ema_weights_without_an_ema(harness):
    m = harness("classifier", torch.float32).model()
    with pytest.raises(ValueError, match="no EMA"):
        m.ema_weights()
    m.set_training_controls(schedule=1e-3, clip_norm=1.0)
    with pytest.raises(ValueError, match="no EMA"):
        m.ema_weights()
    with pytest.raises(ValueError):
        harness("classifier", torch.float32).engine(m).swap_ema()


# ---- validate_ema ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["classifier", "twins"])
def test_validation_on_the_averaged_weights(harness, kind, dtype):
    """Sweeps every 2 steps inside ``fit`` under validate_ema equal ``with ema_weights(): evaluate(...)`` from a host loop
    stopped at the same steps; the training run keeps the bits of the run without validation."""
    h = harness(kind, dtype)
    D = sub("dataset")
    held = D.DeviceDataset(_clips(N, CLIP, seed=29), LABELS, C)
    mk = (lambda: held.eval_sampler(3, T, seed=SEED, sweep_capacity=2)) if kind == "classifier" else \
        (lambda: held.embed_sampler(3, T, seed=SEED, sweep_capacity=2))
    ctl = dict(schedule=_schedule(), horizon=HORIZON, clip_norm=0.5, ema_decay=DECAY)
    m = h.model()
    m.set_training_controls(validate_ema=True, **ctl)
    out = m.fit(h.sampler(log_capacity=RING), STEPS, validate=(mk(), 2))
    losses, results = out[0], out[-1]
    assert [r.step for r in results] == [2, 4, 6, 8]
    plain = h.model()
    plain.set_training_controls(**ctl)
    sp = h.sampler(log_capacity=RING)
    ev = mk()
    want_losses, want = [], []
    for k in range(4):
        want_losses.append(h.fit(plain, sp, 2))
        with plain.ema_weights():
            want.append(plain.evaluate(ev, step=sp.step))
    assert np.array_equal(_bits(losses), _bits(np.concatenate(want_losses)))
    _same_state(h.state(m), h.state(plain))
    for a, b in zip(results, want):
        assert a.step == b.step and a.seen == b.seen
        if kind == "classifier":
            assert np.array_equal(a.pred, b.pred) and np.array_equal(a.rank, b.rank) and np.array_equal(a.confusion, b.confusion)
            assert np.array_equal(_bits(a.nll), _bits(b.nll))
        else:
            assert np.array_equal(_bits(a.emb), _bits(b.emb)) and np.array_equal(a.nearest, b.nearest)
            assert np.array_equal(_bits(a.nearest_dist), _bits(b.nearest_dist))
            assert np.array_equal(a.hist_same, b.hist_same) and np.array_equal(a.hist_diff, b.hist_diff)
    raw = h.model()                                                      # the sweeps judged the average, not the raw weights
    raw.set_training_controls(**ctl)
    r_raw = raw.fit(h.sampler(log_capacity=RING), STEPS, validate=(mk(), 2))[-1]
    key = (lambda r: r.nll) if kind == "classifier" else (lambda r: r.emb)
    assert any(not np.array_equal(_bits(key(a)), _bits(key(b))) for a, b in zip(results, r_raw))


# ---- resume ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_resume_continues_the_run_exactly(harness, kind, dtype, tmp_path):
    h = harness(kind, dtype)
    ctl = dict(schedule=_schedule(), horizon=HORIZON, clip_norm=0.5, ema_decay=DECAY)
    whole = h.model()
    whole.set_training_controls(**ctl)
    sw = h.sampler(log_capacity=RING)
    want = h.fit(whole, sw, 6)

    first = h.model()
    first.set_training_controls(**ctl)
    s1 = h.sampler(log_capacity=RING)
    h.fit(first, s1, 3)
    d = str(tmp_path)
    save = (lambda m, *a, **k: m.save(None, *a, **k)) if kind in ("student", "twins") else (lambda m, *a, **k: m.save(*a, **k))
    load = (lambda m, x: m.load(None, x)) if kind in ("student", "twins") else (lambda m, x: m.load(x))
    save(first, d, 3, force=True)
    first.save_training_state(d, 3, sampler=s1)

    second = h.model()
    second.set_training_controls(**ctl)
    h.engine(second)
    s2 = h.sampler(log_capacity=RING)
    assert load(second, d)
    assert second.load_training_state(d, sampler=s2) is True
    assert s2.step == 3
    got = h.fit(second, s2, 3)
    assert np.array_equal(_bits(got), _bits(want[3:]))
    _same_state(h.state(second), h.state(whole))
    assert torch.equal(s2.state, sw.state)

    cold = h.model()                                                        # without the training state: not the same run
    cold.set_training_controls(**ctl)
    h.engine(cold)
    s3 = h.sampler(log_capacity=RING)
    assert load(cold, d)
    s3.seek(3)
    h.fit(cold, s3, 1)
    whole4 = h.model()
    whole4.set_training_controls(**ctl)
    h.fit(whole4, h.sampler(log_capacity=RING), 4)
    a, b = h.state(cold), h.state(whole4)
    assert any(not torch.equal(a[n]["params"], b[n]["params"]) for n in a)

    other = h.model()                                                       # mismatches are refused
    with pytest.raises(ValueError, match="controls"):
        other.load_training_state(d)


def test_a_training_state_of_other_shapes_is_refused(harness, tmp_path):
    M = sub("model")
    h = harness("classifier", torch.float32)
    m = h.model()
    m.set_training_controls(schedule=1e-3, ema_decay=DECAY)
    h.engine(m)
    m.save_training_state(str(tmp_path), 0)
    wide = M.WaveNet(T, C, DIL, dilation_channels=64, skip_channels=S, output_channels=C, dtype=torch.float32)
    wide.set_training_controls(schedule=1e-3, ema_decay=DECAY)
    with pytest.raises(ValueError, match="shape"):
        wide.load_training_state(str(tmp_path))


# ---- the table under a captured graph -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["classifier", "autoencoder", "student"])
def test_a_table_replaced_in_place_steers_the_replays(harness, kind):
    """Four steps capture ``fit``'s graph; then the table is replaced by one of the same features whose rows 4 and 6 have
    lr = 0 (in place: the graph object stays): the replays of steps 5 and 7 leave the parameters alone, 6 and 8 move them."""
    h = harness(kind, torch.float32)
    O = sub("optim")
    m = h.model()
    m.set_training_controls(schedule=1e-3, horizon=8, ema_decay=DECAY)
    s = h.sampler(log_capacity=RING)
    h.fit(m, s, 4)
    eng = h.engine(m)
    graphs = eng._fit_state["graphs"]
    assert graphs is not None
    m.set_training_controls(schedule=O.piecewise([3, 4, 5, 6], [1e-3, 0.0, 1e-3, 0.0, 1e-3]), horizon=8, ema_decay=DECAY)
    assert eng._fit_state is not None and eng._fit_state["graphs"] is graphs
    for step in range(5, 9):
        before = h.state(m)
        h.fit(m, s, 1)
        after = h.state(m)
        for name in after:
            same = torch.equal(before[name]["params"], after[name]["params"])
            assert same == (step in (5, 7)), (step, name)
            assert not torch.equal(before[name]["m"], after[name]["m"])
    assert eng._fit_state["graphs"] is graphs


def test_enabling_the_ema_after_capture_drops_the_graphs(harness):
    h = harness("classifier", torch.float32)
    m = h.model()
    m.set_training_controls(schedule=_schedule(), horizon=HORIZON)
    s = h.sampler(log_capacity=RING)
    first = h.fit(m, s, 4)
    eng = h.engine(m)
    assert eng._fit_state["graphs"] is not None
    m.set_training_controls(schedule=_schedule(), horizon=HORIZON, ema_decay=DECAY)
    assert eng._fit_state is None and not getattr(eng, "_graph_ready", False)
    shadow0 = eng.params.clone()
    assert torch.equal(eng.ema, shadow0)                                     # the shadow starts at the parameters
    rest = h.fit(m, s, 4)
    assert eng._fit_state["graphs"] is not None                              # captured again by the usual rule
    ref = h.model()                                                          # the parameters: the run without a shadow
    ref.set_training_controls(schedule=_schedule(), horizon=HORIZON)
    want = h.fit(ref, h.sampler(log_capacity=RING), STEPS)
    assert np.array_equal(_bits(np.concatenate([first, rest])), _bits(want))
    _same_state(h.state(m), h.state(ref), keys=["params", "m", "v", "step"])
    assert not torch.equal(eng.ema, shadow0) and not torch.equal(eng.ema, eng.params)
