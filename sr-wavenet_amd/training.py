"""The training machinery the five trainable models of ``model.py`` share, host-side only: the capture rule
(``_captured_step``) and its three callers -- ``_train_step`` (``train(x)``), ``_fit`` / ``_fit_validated`` (``fit`` on a
device-resident sampler of dataset.py) and ``_sweep_steps`` (the forward-only sweeps of ``evaluate``: ``_eval_sweep``,
``_evaluate_losses``) --, what a sampler must be for a model to take it, the checkpoint files (``_write_state`` /
``_read_state``), and ``_TrainingControls``, the base of every trainable model: training controls and EMA weights
(optim.py), the optimizer state beside the checkpoint, ``save`` / ``load`` with the reference's cadence.
Nothing here imports ``model.py`` or ``serving.py``."""
from __future__ import annotations

import gc
import json
import os
import time

import numpy as np
import torch

from .engine import WaveNetEngine


def _captured_step(st, slot, eager, capture, replay):
    """The capture rule, once.  `st` counts the eager steps of one launch sequence (``st["eager"]``), remembers a failed
    capture (``st["failed"]``) and holds what was captured (``st[slot]``, None before).  Captured: ``replay(st[slot])``.
    Otherwise ``eager()`` runs the launches, and behind the second eager step ``capture()`` records them -- it launches
    nothing and returns what is to be replayed -- unless SRWN_MODEL_GRAPHS=0 or an earlier capture failed; a capture
    that raises is reported once and the steps stay eager.  Returns what the step returned."""
    if st[slot] is not None:
        return replay(st[slot])
    out = eager()
    st["eager"] += 1
    if st["eager"] >= 2 and os.environ.get("SRWN_MODEL_GRAPHS", "1") != "0" and not st["failed"]:
        try:
            torch.cuda.synchronize()
            gc.collect()        # (a collection inside a capture may destroy hipGraphs mid-capture: kernels.run_cached_graph)
            st[slot] = capture()
            torch.cuda.synchronize()
        except Exception as e:   # keep going with eager launches, say why once
            st["failed"] = True
            print("hipGraph capture failed (%s); continuing with eager launches" % e)
    return out


def _sampler_state(eng, attr, sampler, slot):
    """The capture state of an (engine, sampler) pair, kept on the engine as `attr`: it starts again at zero when another
    sampler object is passed (and after ``OptControls.drop_graphs`` has cleared it)."""
    st = getattr(eng, attr, None)
    if st is None or st["sampler"] is not sampler:
        st = {"sampler": sampler, "eager": 0, slot: None, "failed": False}
        setattr(eng, attr, st)
    return st


def _train_step(eng):
    """One training step of an engine: the first two run as eager launches, then the step is captured as hipGraphs
    (inputs live in persistent device buffers, so replays see each new batch) -- at the reference scripts' small
    shapes the ~100-400 launches of a step cost more than the kernels.  SRWN_MODEL_GRAPHS=0 keeps eager launches.
    The state is the engine's ``_graph_ready`` (``OptControls.drop_graphs`` clears it, not the count: one eager step
    precedes the next capture), ``_eager_steps`` and ``_graph_failed``."""
    st = {"eager": getattr(eng, "_eager_steps", 0), "failed": getattr(eng, "_graph_failed", False),
          "ready": getattr(eng, "_graph_ready", False) or None}
    out = _captured_step(st, "ready", eng.train_step, lambda: eng.capture_graphs() or True,
                         lambda ready: eng.train_step_graphed())
    eng._eager_steps, eng._graph_failed, eng._graph_ready = st["eager"], st["failed"], bool(st["ready"])
    return out


def _fit_part(eng, sampler, dest, part, between=None):
    """The launches of one ``fit`` step on either side of the gradient all-reduce: 0 = {draw, forward, backward},
    1 = {Adam, re-pack, log}.  Between the sampler's two launches this is ``train_step``'s own sequence; `between`
    (the student: the teacher encoder's forward pass and the scatter of its encoding) runs right behind the draw."""
    if part == 0:
        sampler.draw(**dest)
        if between is not None:
            between()
        if isinstance(eng, WaveNetEngine):
            eng.forward(defer_loss=True)
        else:                            # the auto-encoder pair (encoder.AutoEncoderEngine), the student (StudentEngine)
            eng.forward()
        eng.backward()
    else:
        eng.optimizer_step()
        sampler.log_engine(eng)


def _fit(eng, sampler, steps, dest, between=None, after_step=None):
    """``steps`` training steps of an engine fed by a sampler of dataset.py: every batch is drawn on the device by the
    step's first launch (``dest``: where the sampler's ``draw`` writes what ``set_inputs`` would) and the step is logged
    by its last (the sampler's ``log_engine``), so a run of steps needs no upload and no host wait -- the host waits once
    per ``log_capacity`` steps to drain the rings.  Capture follows the rule of ``_captured_step``: two eager steps of this
    (engine, sampler) pair, then hipGraphs of its own (the graphs of ``train(x)`` are not touched); SRWN_MODEL_GRAPHS=0
    keeps eager launches.  Returns what the sampler's ``results`` gives for every step, one array per logged quantity:
    the loss, float32 [steps], first.  `after_step` (validation) is called behind every step, once the sampler's count has
    ticked; what it enqueues runs between this step's launches and the next one's."""
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps %d" % steps)
    st = _sampler_state(eng, "_fit_state", sampler, "graphs")

    def eager():
        _fit_part(eng, sampler, dest, 0, between)
        eng.allreduce_grads()
        _fit_part(eng, sampler, dest, 1, between)

    def replay(graphs):
        graphs[0].replay()
        if len(graphs) > 1:
            eng.allreduce_grads()
            graphs[1].replay()
    capture = lambda: _fit_capture(eng, sampler, dest, between)
    pieces, done = [], 0
    while done < steps:
        n = min(steps - done, sampler.log_capacity)
        step0 = sampler.step
        for _ in range(n):
            _captured_step(st, "graphs", eager, capture, replay)
            sampler.step += 1
            if after_step is not None:       # (validation: a sweep of another sampler enqueued behind this step)
                after_step()
        pieces.append(sampler.results(step0, n))               # the host waits here
        done += n
    if not pieces:
        pieces.append(sampler.results(sampler.step, 0))
    return tuple(np.concatenate([p[i] for p in pieces], axis=0) for i in range(len(pieces[0])))


def _fit_capture(eng, sampler, dest, between=None):
    """The ``fit`` step as one hipGraph, or with several ranks as two with the all-reduce left between them (see
    ``WaveNetEngine.capture_graphs``).  Capturing launches nothing: the device step does not tick."""
    g0 = torch.cuda.CUDAGraph()
    if eng.world == 1 and os.environ.get("SRWN_FORCE_DIST") != "1":
        with torch.cuda.graph(g0):
            _fit_part(eng, sampler, dest, 0, between)
            _fit_part(eng, sampler, dest, 1, between)
        return [g0]
    with torch.cuda.graph(g0):
        _fit_part(eng, sampler, dest, 0, between)
    g1 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1, pool=g0.pool()):
        _fit_part(eng, sampler, dest, 1, between)
    return [g0, g1]


def _fit_validated(eng, sampler, steps, dest, ev, every, sweep, ema):
    """``_fit`` with `sweep()` -- one sweep of the held-out sampler `ev` -- enqueued behind every `every`-th step
    (``sampler.step`` after the step); with `ema` it judges the averaged weights, swapped in and out on its stream.  The
    host reads `ev`'s result slots when ``sweep_capacity`` sweeps are pending and at the end.  Returns (``_fit``'s, results)."""
    results, pending = [], []            # pending: (sweep number, training step) of the sweeps still in their slots

    def drain():                         # the host waits here
        results.extend(ev.result(k, s) for k, s in pending)
        del pending[:]

    def after_step():
        if sampler.step % every == 0:
            if len(pending) >= ev.sweep_capacity:
                drain()
            if ema:
                eng.swap_ema()
            sweep()
            if ema:
                eng.swap_ema()
            pending.append((ev.sweep - 1, sampler.step))

    out = _fit(eng, sampler, steps, dest, after_step=after_step)
    drain()
    return out, results


def _fit_labels(sampler, width, who, what, method="fit"):
    """The dataset of `sampler` must hold labels of `width` classes (their one-hot rows are `who`'s `what`); `method`: the
    method that refuses."""
    d = sampler.dataset
    if d.labels is None:
        raise ValueError("%s.%s: the dataset holds no labels; their one-hot rows are the %s" % (who, method, what))
    if d.num_classes != int(width):
        raise ValueError("%s.%s: the dataset has num_classes=%d, the model's %s are %d wide"
                         % (who, method, d.num_classes, what, int(width)))


def _sweep_steps(eng, sampler, step, count, tick):
    """`count` forward-only steps of an engine fed by a sampler, enqueued without a host wait: `step()` is the launch
    sequence {draw, forward, the sampler's last launch} and `tick()` the host's copy of what that last launch does to the
    device state.  Capture follows the rule of ``_captured_step`` with a state of its own: two eager steps of this (engine,
    sampler) pair, then one hipGraph that is replayed (the graphs of ``fit`` and ``train`` are not touched);
    SRWN_MODEL_GRAPHS=0 keeps eager launches."""
    st = _sampler_state(eng, "_eval_state", sampler, "graph")

    def capture():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):       # capturing launches nothing: the device state does not tick
            step()
        return g
    for _ in range(count):
        _captured_step(st, "graph", step, capture, lambda g: g.replay())
        tick()


def _eval_sweep(eng, ev):
    """One sweep of an ``EvalSampler`` through a pooled-head engine, enqueued: ``sweep_steps`` steps of {srwn_batch_draw
    into the engine's audio, the forward pass without loss or weight-gradient tiles, srwn_eval_classes}.  The sweep lands
    in slot ``(ev.sweep - 1) % sweep_capacity`` once this returns; nothing waits for it here."""
    def step():
        ev.draw(audio=eng.audio)
        eng.forward(with_loss=False, train=False)
        ev.classify(eng.probs)
    ev.seek(0)
    _sweep_steps(eng, ev, step, ev.sweep_steps, ev.stepped)


def _evaluate_losses(eng, sampler, dest, steps, between=None, read=None):
    """What a sampler logs of every step of one forward-only sweep of `steps` steps (``_loss_sweep_steps``), one float32
    [steps] array per quantity `read(first, count)` gives (default: the loss): the launches of ``loss(batch)`` between
    the sampler's draw -- with `between` behind it, as in ``_fit_part`` -- and its log.  The host waits once per
    ``log_capacity`` steps."""
    def step():
        sampler.draw(**dest)
        if between is not None:
            between()
        eng.forward()
        sampler.log_engine(eng)

    def tick():
        sampler.step += 1
    read = read or (lambda first, count: (sampler.losses(first, count),))
    sampler.seek(0)
    pieces, done = [], 0
    while done < steps:
        n = min(steps - done, sampler.log_capacity)
        _sweep_steps(eng, sampler, step, n, tick)
        pieces.append(read(done, n))                            # the host waits here
        done += n
    return tuple(np.concatenate(q) for q in zip(*pieces))


def _loss_sweep_steps(sampler, who, kind=None, how="a plain dataset.BatchSampler (dataset.sampler(..., shuffle=False))"):
    """The steps of ``_evaluate_losses``, or the reason why `sampler` cannot drive it.  `kind`: the sampler class the
    model's step is fed by (default: a plain ``BatchSampler``), `how` its name in the refusal."""
    from .dataset import BatchSampler
    if type(sampler) is not (kind or BatchSampler):
        raise TypeError("%s.evaluate takes %s, got %s" % (who, how, type(sampler).__name__))
    _refuse_augment(sampler, who)
    if sampler.shuffle:
        raise ValueError("%s.evaluate: the sampler shuffles; a sweep visits the records in order (shuffle=False)" % who)
    n, per = len(sampler.dataset), sampler.batch_size * sampler.world
    if n % per:
        raise ValueError("%s.evaluate: %d clips are no multiple of batch_size * world = %d; this model's loss kernel gives "
                         "one number per batch, so a ragged last step would count wrapped-around clips twice (the "
                         "streaming scorers give per-sample likelihoods of any clip)" % (who, n, per))
    return n // per


def _refuse_augment(sampler, who):
    """A held-out sweep is not augmented: ``evaluate`` refuses a sampler that carries an ``Augment``."""
    if getattr(sampler, "augment", None) is not None:
        raise ValueError("%s.evaluate: the sampler augments its rows; a held-out sweep is not augmented (build it with "
                         "augment=None)" % who)


def _check_validate(validate, kind=None, how="a dataset.EvalSampler (dataset.eval_sampler(...))"):
    """``validate=(eval_sampler, every)`` of ``WaveNet.fit`` (`kind`, `how`: the sampler class of another model's
    sweeps and its name in the refusal), checked before any device work."""
    from .dataset import EvalSampler
    try:
        ev, every = validate
    except (TypeError, ValueError):
        raise ValueError("validate must be (eval_sampler, every), got %r" % (validate,))
    if not isinstance(ev, kind or EvalSampler):
        raise TypeError("validate: the first entry must be %s, got %s" % (how, type(ev).__name__))
    if int(every) < 1:
        raise ValueError("validate: every %d: at least 1" % int(every))
    return ev, int(every)


# --- checkpoint files --------------------------------------------------------------------------------------------
# Two on-disk forms behind the reference's `checkpoint` state file (model.py:217-235): this package's own
# `model.ckpt-N.pt` (a torch state dict keyed by the reference's variable names) and TensorFlow's V2 bundle
# `model.ckpt-N.index` + `.data-00000-of-00001` as tf.train.Saver writes it (tf_checkpoint.py; SRWN_CKPT_FORMAT=tf or
# save(..., fmt="tf")), so weights trained with the reference load by name and vice versa.
def _write_state(logdir, global_step, params, fmt=None):
    fmt = fmt or os.environ.get("SRWN_CKPT_FORMAT", "pt")
    os.makedirs(logdir, exist_ok=True)
    if fmt == "tf":
        from . import tf_checkpoint as tfc
        name = "model.ckpt-%d" % int(global_step)
        tfc.write_bundle(os.path.join(logdir, name), {k: v.detach().float().cpu().numpy() for k, v in params.items()})
        tfc.write_checkpoint_state(logdir, name)
        return
    if fmt != "pt":
        raise ValueError("checkpoint format %r (pt, tf)" % (fmt,))
    state = {k: v.detach().cpu().clone() for k, v in params.items()}
    torch.save(state, os.path.join(logdir, "model.ckpt-%d.pt" % int(global_step)))
    with open(os.path.join(logdir, "checkpoint"), "w") as f:
        f.write('model_checkpoint_path: "model.ckpt-%d.pt"\n' % int(global_step))


def _read_state(logdir, params_fn):
    """None: no checkpoint state file; False: the file it names is missing; True: the tensors of `params_fn()` filled
    (it is only called once a file is there: building the name map instantiates the model's first engine)."""
    if logdir is None or not os.path.exists(os.path.join(logdir, "checkpoint")):
        return None
    from . import tf_checkpoint as tfc
    path = tfc.latest_checkpoint(logdir)
    if path is None or not (os.path.exists(path) or tfc.is_bundle(path)):
        print("Could not find checkpoint at %s" % path)
        return False
    params = params_fn()
    if tfc.is_bundle(path):
        arrays = tfc.read_bundle(path, names=list(params))       # Adam slots and counters in a TF bundle are ignored
        #                                                            (this package's own: save_/load_training_state)
        get = lambda k: torch.from_numpy(arrays[k])
    else:
        state = torch.load(path, weights_only=True)
        get = lambda k: state[k]
    for k, dst in params.items():
        src = get(k)
        if tuple(src.shape) != tuple(dst.shape):     # same element count in another layout would load scrambled weights
            raise ValueError("checkpoint variable %s has shape %s, the model's is %s" % (k, tuple(src.shape), tuple(dst.shape)))
        dst.copy_(src.to(dst.device))
    return True


# --- training controls (optim.py) ----------------------------------------------------------------------------------
class _TrainingControls:
    """What the five trainable models share: ``set_training_controls``, ``ema_weights``, ``save_training_state`` /
    ``load_training_state``, and ``save`` / ``load`` of the variables ``network_params`` names.  A model says where its
    optimizers live: ``_control_engine()`` -- the engine whose ``set_controls`` / ``swap_ema`` reach every parameter buffer
    of the model (built on first use) -- and ``_optimizers()``, name -> (engine, params, m, v, step, controls holder);
    and what follows loaded weights: ``_after_load()`` resets its EMA shadows and re-packs its weight images."""
    _controls = None          # the optim.TrainControls in force (class defaults: objects made without __init__ have none)
    _in_ema = False

    def set_training_controls(self, schedule=None, horizon=None, clip_norm=None, ema_decay=None, ema_warmup=True,
                              validate_ema=False):
        """Learning-rate schedule, gradient clipping and EMA weights for ``train`` and ``fit``, for every engine of the model,
        present and future.  `schedule`: a schedule of ``optim`` (or any ``f(step) -> lr`` of the 0-based step, or a
        number); None keeps the constructor's learning_rate, constant.  `horizon`: the steps the device table holds (later
        steps keep its last row; default 1).  `clip_norm`: tf.clip_by_global_norm's bound.  `ema_decay` in [0, 1): keep an
        exponential moving average of the weights (`ema_warmup`: tf's ``min(decay, (1 + t) / (10 + t))``), which
        ``ema_weights()`` serves and, with `validate_ema`, the sweeps of ``fit(..., validate=...)`` judge.  Calling it with
        no argument removes the controls.  The same features within the allocated horizon rewrite the device table in
        place and captured graphs follow; anything else captures ``train`` and ``fit`` again."""
        from .optim import TrainControls
        if self._in_ema:
            raise RuntimeError("set_training_controls inside ema_weights()")
        if schedule is None and horizon is None and clip_norm is None and ema_decay is None:
            controls = None
            if validate_ema:
                raise ValueError("validate_ema needs ema_decay")
        else:
            controls = TrainControls(self._learning_rate() if schedule is None else schedule,
                                     1 if horizon is None else horizon, clip_norm, ema_decay, ema_warmup, validate_ema)
        self._controls = controls
        eng = self._control_engine(build=False)
        if eng is not None:
            eng.set_controls(controls)
        return controls

    def _learning_rate(self):
        return self._cfg.learning_rate

    def _apply_controls(self, eng):
        """A model's first engine, just built: the controls set before it existed."""
        if self._controls is not None:
            eng.set_controls(self._controls)

    def _refuse_in_ema(self, what):
        if self._in_ema:
            raise RuntimeError("%s inside ema_weights(): the parameters hold the averaged weights; leave the context to "
                               "train" % what)

    def _validate_ema(self):
        return self._controls is not None and self._controls.validate_ema

    def ema_weights(self):
        """A context in which the model's parameters ARE the averaged weights: ``swap_ema()`` on entry and again on exit.
        Everything that reads the parameters inside it -- predict, evaluate, generate, stream, generation_pool, encode,
        reconstruct, get_embedding, save, and the snapshots recognizer(), embedder(), synthesizer(), inverter(), scorer()
        take -- serves the average; ``train`` / ``fit`` raise RuntimeError.  ValueError without an EMA."""
        if self._controls is None or self._controls.ema_decay is None:
            raise ValueError("ema_weights: this model keeps no EMA weights (set_training_controls(ema_decay=...))")
        if self._in_ema:
            raise RuntimeError("ema_weights: already inside the context")
        return _EmaContext(self)

    def training_step(self) -> int:
        """Adam's step count (of the model's first optimizer): the steps trained so far, where a resumed run goes on."""
        return int(next(iter(self._optimizers().values()))[4].item())

    # --- checkpointing with the reference's cadence semantics (model.py:217-239) -------------------------------
    def save(self, logdir, global_step, force=False, fmt=None):
        """Writes ``network_params`` (and ``_config()`` as config.json) when forced or 60 s after the last time."""
        if force or time.time() - self.last_checkpoint_time > 60:
            _write_state(logdir, global_step, self.network_params, fmt)
            cfg = self._config()
            if cfg is not None:
                with open(os.path.join(logdir, "config.json"), "w") as f:
                    json.dump(cfg, f)
            self.last_checkpoint_time = time.time()
            return True
        return False

    def _config(self):      # the constructor arguments beside a checkpoint (the reference: its meta graph, model.py:318)
        return None

    def load(self, logdir):
        ok = _read_state(logdir, lambda: self.network_params)
        if ok:
            self._after_load()      # (an EMA shadow restarts from the loaded weights: load_training_state has the saved one)
            print("Restoring previous session")
        return ok

    # --- optimizer state next to the checkpoint ------------------------------------------------------------
    def save_training_state(self, logdir, global_step, sampler=None):
        """What ``save`` leaves out and a resumed run needs: Adam's m, v and step of every optimizer of the model, the EMA
        shadow, the controls' scalar settings and -- given a sampler -- its {seed, step}, as ``train_state-N.pt`` named in
        a ``train_state`` file the way ``checkpoint`` names the weights.  ``save`` and its files do not change."""
        self._refuse_in_ema("save_training_state")
        opts = {}
        for name, (eng, params, m, v, step, ctl) in self._optimizers().items():
            opts[name] = {"m": m.detach().cpu().clone(), "v": v.detach().cpu().clone(), "step": int(step.item()),
                          "ema": None if ctl.ema is None else ctl.ema.detach().cpu().clone()}
        state = {"optimizers": opts, "controls": None if self._controls is None else self._controls.scalars(),
                 "sampler": None if sampler is None else {"seed": int(sampler.seed), "step": int(sampler.step)}}
        os.makedirs(logdir, exist_ok=True)
        name = "train_state-%d.pt" % int(global_step)
        torch.save(state, os.path.join(logdir, name))
        with open(os.path.join(logdir, "train_state"), "w") as f:
            f.write('train_state_path: "%s"\n' % name)

    def load_training_state(self, logdir, sampler=None):
        """Restores what ``save_training_state`` wrote; after ``load`` it resumes the run exactly -- call
        ``set_training_controls`` first as the saved run did (a schedule is code: the file holds the scalar settings and
        checks clip_norm, ema_decay and ema_warmup; the horizon may grow).  Given a sampler built like the saved one, it continues its sequence at the saved step.  Returns
        False without a state file; ValueError where shapes or settings do not match."""
        self._refuse_in_ema("load_training_state")
        idx = os.path.join(logdir, "train_state")
        if not os.path.exists(idx):
            return False
        import re
        m_ = re.search(r'train_state_path: "([^"]+)"', open(idx).read())
        path = os.path.join(logdir, m_.group(1)) if m_ else None
        if path is None or not os.path.exists(path):
            print("Could not find training state at %s" % path)
            return False
        state = torch.load(path, weights_only=True)
        have = None if self._controls is None else self._controls.scalars()
        # (what shapes the state: clipping and the shadow.  A resumed run may extend its horizon or judge other weights.)
        drop = lambda c: None if c is None else {k: v for k, v in c.items() if k not in ("validate_ema", "horizon")}
        if drop(state["controls"]) != drop(have):
            raise ValueError("the training state was saved under controls %r, this model has %r: call "
                             "set_training_controls as the saved run did" % (state["controls"], have))
        opts = self._optimizers()
        if set(opts) != set(state["optimizers"]):
            raise ValueError("the training state holds optimizers %s, the model has %s"
                             % (sorted(state["optimizers"]), sorted(opts)))
        for name, (eng, params, m, v, step, ctl) in opts.items():       # check everything before anything is written
            o = state["optimizers"][name]
            for k, dst in (("m", m), ("v", v), ("ema", ctl.ema)):
                if (o[k] is None) != (dst is None) or (dst is not None and tuple(o[k].shape) != tuple(dst.shape)):
                    raise ValueError("training state %s.%s has shape %s, the model's is %s"
                                     % (name, k, None if o[k] is None else tuple(o[k].shape),
                                        None if dst is None else tuple(dst.shape)))
        if sampler is not None:
            if state["sampler"] is None:
                raise ValueError("the training state holds no sampler state")
            if int(state["sampler"]["seed"]) != int(sampler.seed):
                raise ValueError("the training state's sampler was seeded %d, this one %d"
                                 % (state["sampler"]["seed"], sampler.seed))
        for name, (eng, params, m, v, step, ctl) in opts.items():
            o = state["optimizers"][name]
            m.copy_(o["m"]); v.copy_(o["v"]); step.fill_(int(o["step"]))
            if ctl.ema is not None:
                ctl.ema.copy_(o["ema"])
        if sampler is not None:
            sampler.seek(int(state["sampler"]["step"]))
        return True


class _EmaContext:
    def __init__(self, model):
        self.model = model

    def __enter__(self):
        m = self.model
        m._control_engine().swap_ema()
        m._in_ema = True
        return m

    def __exit__(self, *exc):
        m = self.model
        m._control_engine().swap_ema()
        m._in_ema = False
        return False
