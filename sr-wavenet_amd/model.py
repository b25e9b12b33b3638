"""Host-side mirror of the reference's model classes (``/root/reference/model.py``) on the MI355X engine.

Same constructor and method signatures, NumPy in / NumPy out like the reference's ``sess.run``
wrappers, but no TensorFlow: the graph body is the fixed kernel sequence of ``engine.WaveNetEngine``.

* ``WaveNet``            -- model.py:8-72 (clip-level softmax classifier), complete.
* ``WaveNetTeacher``     -- the 30-layer mu-law softmax teacher BASELINE.json names (decoder stack of
                            model.py:158-196 with the 256-way softmax head the reference carries at
                            model.py:100-112); this is the benchmark path.
* ``WaveNetAutoEncoder`` -- model.py:75-285: non-causal encoder + conditioned mixture-of-logistics decoder
                            (encoder.AutoEncoderEngine), the teacher teacher.py trains.
* ``StreamingScorer``    -- the softmax teacher's per-sample likelihood on its own (scorer.StreamScorer): any batch, any
                            length, whole recordings or streams.
* ``AudioEncoder``       -- that auto-encoder's encoder on its own (encoder.FrameEncoder): any batch, any length,
                            whole clips or streams.
* ``ParallelWaveNet``    -- model.py:290-656: the IAF student distilled against that frozen teacher
                            (student.StudentEngine).
* ``SiameseWaveNet``     -- model.py:660-797: two weight-sharing WaveNet towers trained on pairs with the contrastive
                            loss (engine head_mode "contrastive": both towers run as one batch).
* ``StreamingEmbedder``  -- one such tower on its own (embedder.StreamEmbedder): any batch, any length, whole recordings or
                            streams, every window matched against a gallery of enrolled templates.
"""
from __future__ import annotations

import os
import time
from typing import Dict, Optional

import numpy as np
import torch

from . import kernels as K
from .dataset import EvalResult, PairEvalResult  # noqa: F401  (what the evaluate() methods return)
from .engine import StackConfig, WaveNetEngine
from .slots import SlotTable, per_stream, slot_list


def _train_step(eng):
    """One training step of an engine: the first two run as eager launches, then the step is captured as hipGraphs
    (inputs live in persistent device buffers, so replays see each new batch) -- at the reference scripts' small
    shapes the ~100-400 launches of a step cost more than the kernels.  SRWN_MODEL_GRAPHS=0 keeps eager launches."""
    if getattr(eng, "_graph_ready", False):
        return eng.train_step_graphed()
    out = eng.train_step()
    eng._eager_steps = getattr(eng, "_eager_steps", 0) + 1
    if eng._eager_steps >= 2 and os.environ.get("SRWN_MODEL_GRAPHS", "1") != "0" and not getattr(eng, "_graph_failed", False):
        try:
            eng.capture_graphs()
            eng._graph_ready = True
        except Exception as e:   # keep training with eager launches, say why once
            eng._graph_failed = True
            print("hipGraph capture failed (%s); continuing with eager launches" % e)
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
    per ``log_capacity`` steps to drain the rings.  Capture follows ``_train_step``'s rule: two eager steps of this
    (engine, sampler) pair, then hipGraphs of its own (the graphs of ``train(x)`` are not touched); SRWN_MODEL_GRAPHS=0
    keeps eager launches.  Returns what the sampler's ``results`` gives for every step, one array per logged quantity:
    the loss, float32 [steps], first.  `after_step` (validation) is called behind every step, once the sampler's count has
    ticked; what it enqueues runs between this step's launches and the next one's."""
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps %d" % steps)
    st = getattr(eng, "_fit_state", None)
    if st is None or st["sampler"] is not sampler:
        st = eng._fit_state = {"sampler": sampler, "eager": 0, "graphs": None, "failed": False}
    world = eng.dec.world if hasattr(eng, "dec") else eng.world
    pieces = []
    done = 0
    while done < steps:
        n = min(steps - done, sampler.log_capacity)
        step0 = sampler.step
        for _ in range(n):
            if st["graphs"] is not None:
                st["graphs"][0].replay()
                if len(st["graphs"]) > 1:
                    eng.allreduce_grads()
                    st["graphs"][1].replay()
            else:
                _fit_part(eng, sampler, dest, 0, between)
                eng.allreduce_grads()
                _fit_part(eng, sampler, dest, 1, between)
                st["eager"] += 1
                if st["eager"] >= 2 and os.environ.get("SRWN_MODEL_GRAPHS", "1") != "0" and not st["failed"]:
                    try:
                        st["graphs"] = _fit_capture(eng, sampler, dest, world, between)
                    except Exception as e:   # keep training with eager launches, say why once
                        st["failed"] = True
                        print("hipGraph capture failed (%s); continuing with eager launches" % e)
            sampler.step += 1
            if after_step is not None:       # (validation: a sweep of another sampler enqueued behind this step)
                after_step()
        pieces.append(sampler.results(step0, n))               # the host waits here
        done += n
    if not pieces:
        pieces.append(sampler.results(sampler.step, 0))
    return tuple(np.concatenate([p[i] for p in pieces], axis=0) for i in range(len(pieces[0])))


def _fit_capture(eng, sampler, dest, world, between=None):
    """The ``fit`` step as one hipGraph, or with several ranks as two with the all-reduce left between them (see
    ``WaveNetEngine.capture_graphs``).  Capturing launches nothing: the device step does not tick."""
    import gc
    torch.cuda.synchronize()
    gc.collect()        # (a collection inside a capture may destroy hipGraphs mid-capture: kernels.run_cached_graph)
    g0 = torch.cuda.CUDAGraph()
    if world == 1 and os.environ.get("SRWN_FORCE_DIST") != "1":
        with torch.cuda.graph(g0):
            _fit_part(eng, sampler, dest, 0, between)
            _fit_part(eng, sampler, dest, 1, between)
        graphs = [g0]
    else:
        with torch.cuda.graph(g0):
            _fit_part(eng, sampler, dest, 0, between)
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, pool=g0.pool()):
            _fit_part(eng, sampler, dest, 1, between)
        graphs = [g0, g1]
    torch.cuda.synchronize()
    return graphs


def _fit_labels(sampler, width, who, what):
    """The dataset of `sampler` must hold labels of `width` classes (their one-hot rows are `who`'s `what`)."""
    d = sampler.dataset
    if d.labels is None:
        raise ValueError("%s.fit: the dataset holds no labels; their one-hot rows are the %s" % (who, what))
    if d.num_classes != int(width):
        raise ValueError("%s.fit: the dataset has num_classes=%d, the model's %s are %d wide"
                         % (who, d.num_classes, what, int(width)))


def _sweep_steps(eng, sampler, step, count, tick):
    """`count` forward-only steps of an engine fed by a sampler, enqueued without a host wait: `step()` is the launch
    sequence {draw, forward, the sampler's last launch} and `tick()` the host's copy of what that last launch does to the
    device state.  Capture follows ``_fit``'s rule with a state of its own: two eager steps of this (engine, sampler) pair,
    then one hipGraph that is replayed (the graphs of ``fit`` and ``train`` are not touched); SRWN_MODEL_GRAPHS=0 keeps
    eager launches."""
    st = getattr(eng, "_eval_state", None)
    if st is None or st["sampler"] is not sampler:
        st = eng._eval_state = {"sampler": sampler, "eager": 0, "graph": None, "failed": False}
    for _ in range(count):
        if st["graph"] is not None:
            st["graph"].replay()
        else:
            step()
            st["eager"] += 1
            if st["eager"] >= 2 and os.environ.get("SRWN_MODEL_GRAPHS", "1") != "0" and not st["failed"]:
                try:
                    import gc
                    torch.cuda.synchronize()
                    gc.collect()    # (a collection inside a capture may destroy hipGraphs mid-capture: see _fit_capture)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):       # capturing launches nothing: the device state does not tick
                        step()
                    torch.cuda.synchronize()
                    st["graph"] = g
                except Exception as e:   # keep sweeping with eager launches, say why once
                    st["failed"] = True
                    print("hipGraph capture failed (%s); continuing with eager launches" % e)
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


def _evaluate_losses(eng, sampler, dest, who):
    """The forward-only loss of every step of one sweep of a plain, non-shuffled ``BatchSampler``, float32 [steps]: the
    launches of ``loss(batch)`` between the sampler's draw and its ``srwn_step_log``.  The host waits once per
    ``log_capacity`` steps."""
    def step():
        sampler.draw(**dest)
        eng.forward()
        sampler.log_engine(eng)

    def tick():
        sampler.step += 1
    steps = _loss_sweep_steps(sampler, who)
    sampler.seek(0)
    pieces, done = [], 0
    while done < steps:
        n = min(steps - done, sampler.log_capacity)
        _sweep_steps(eng, sampler, step, n, tick)
        pieces.append(sampler.losses(done, n))                  # the host waits here
        done += n
    return np.concatenate(pieces)


def _loss_sweep_steps(sampler, who, kind=None, how="a plain dataset.BatchSampler (dataset.sampler(..., shuffle=False))"):
    """The steps of ``_evaluate_losses``, or the reason why `sampler` cannot drive it.  `kind`: the sampler class the
    model's step is fed by (default: a plain ``BatchSampler``), `how` its name in the refusal."""
    from .dataset import BatchSampler
    if type(sampler) is not (kind or BatchSampler):
        raise TypeError("%s.evaluate takes %s, got %s" % (who, how, type(sampler).__name__))
    if sampler.shuffle:
        raise ValueError("%s.evaluate: the sampler shuffles; a sweep visits the records in order (shuffle=False)" % who)
    n, per = len(sampler.dataset), sampler.batch_size * sampler.world
    if n % per:
        raise ValueError("%s.evaluate: %d clips are no multiple of batch_size * world = %d; this model's loss kernel gives "
                         "one number per batch, so a ragged last step would count wrapped-around clips twice (the "
                         "streaming scorers give per-sample likelihoods of any clip)" % (who, n, per))
    return n // per


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


def _default_dtype():
    return torch.float32 if os.environ.get("SRWN_DTYPE", "bf16").lower() in ("f32", "fp32", "float32") else torch.bfloat16


# --- conditions ---------------------------------------------------------------------------------------------------
# The reference concatenates a clip's conditions onto every frame of its encoding (encoding_w_condition: model.py:161-167
# for the decoder, model.py:496-499 for the student's flows).
def _tile_conditions(frames, cond):
    """frames [B, k, latent] and conditions [B, condition_size] (torch, one device) -> [B, k, latent + condition_size]."""
    return torch.cat([frames, cond[:, None, :].expand(-1, frames.shape[1], -1)], dim=2)


def _tile_conditions_np(frames, cond):
    """One stream in NumPy: frames [k, latent] and conditions [1, condition_size] -> [k, latent + condition_size]."""
    return np.concatenate([frames, np.repeat(cond, frames.shape[0], 0)], 1)


def _check_conditions(batch, conditions, condition_size, who):
    """conditions as float32 NumPy [batch, condition_size] (None when the model `who` has none); no device work."""
    if condition_size <= 0:
        return None
    if conditions is None:
        raise ValueError("this %s was built with condition_size > 0; pass conditions [%d, %d]" % (who, batch, condition_size))
    c = np.asarray(conditions, dtype=np.float32)
    if c.shape != (batch, condition_size):
        raise ValueError("conditions must be [%d, %d]" % (batch, condition_size))
    return c


def _to_device(c):
    return None if c is None else torch.as_tensor(c).to("cuda")


def _device_conditions(batch, conditions, condition_size, who):
    """The same, checked and then on the device (the caller has asked for the GPU)."""
    return _to_device(_check_conditions(batch, conditions, condition_size, who))


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
    ``load_training_state``.  A model says where its optimizers live: ``_control_engine()`` -- the engine whose
    ``set_controls`` / ``swap_ema`` reach every parameter buffer of the model (built on first use) -- and
    ``_optimizers()``, name -> (engine, params, m, v, step, controls holder)."""
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


class _EngineOwner(_TrainingControls):
    """Builds one engine per (batch, length) seen, all sharing the same parameters."""

    def _setup(self, cfg: StackConfig, seed: int):
        K._need_gpu()
        self._cfg = cfg
        self._seed = seed
        self._engines: Dict[tuple, WaveNetEngine] = {}
        self._primary: Optional[WaveNetEngine] = None
        self.last_checkpoint_time = time.time()

    def _engine(self, B: int, T: int) -> WaveNetEngine:
        key = (int(B), int(T))
        eng = self._engines.get(key)
        if eng is None:
            eng = WaveNetEngine(self._cfg, B, T, "cuda", seed=self._seed, share_from=self._primary)
            if self._primary is None:
                self._primary = eng
                self._apply_controls(eng)
            self._engines[key] = eng
        return eng

    def _learning_rate(self):
        return self._cfg.learning_rate

    def _control_engine(self, build=True):
        """The first engine: its controls, EMA shadow and weight images are shared by every other (``share_from``)."""
        if self._primary is None and build:
            self._engine(1, self._default_length)
        return self._primary

    def _optimizers(self):
        e = self._control_engine()
        return {"stack": (e, e.params, e.adam_m, e.adam_v, e.adam_step, e.ctl)}

    @property
    def network_params(self):
        """Reference name -> tensor (the analogue of tf.get_collection(TRAINABLE_VARIABLES, scope))."""
        if self._primary is None:
            self._engine(1, self._default_length)
        return self._primary.tf_variables(self._scope, decoder=self._decoder_names)

    # --- checkpointing with the reference's cadence semantics (model.py:217-239) -------------------
    def save(self, logdir, global_step, force=False, fmt=None):
        if force or time.time() - self.last_checkpoint_time > 60:
            _write_state(logdir, global_step, self.network_params, fmt)
            self.last_checkpoint_time = time.time()
            return True
        return False

    def load(self, logdir):
        ok = _read_state(logdir, lambda: self.network_params)
        if ok:
            self._primary._reset_ema()      # (an EMA shadow restarts from the loaded weights: load_training_state has the saved one)
            self._primary.repack()
            print("Restoring previous session")
        return ok


class WaveNet(_EngineOwner):
    """model.py:8-72.  ``train(inputs[B,T], targets[B,output_size]) -> loss``; ``predict -> [B,1,C]``."""

    def __init__(self, input_size, output_size, dilations, filter_width=2, dilation_channels=32, skip_channels=256,
                 output_channels=256, name="WaveNet", learning_rate=0.001, dtype=None, seed=0, *, gate_mode="reference"):
        self.input_size = input_size
        self.output_size = output_size
        self.dilations = dilations
        self.filter_width = filter_width
        self.dilation_channels = dilation_channels
        self.skip_channels = skip_channels
        self.output_channels = output_channels
        if output_size != output_channels:
            # the reference's softmax CE (model.py:29) needs logits and labels of equal width
            raise ValueError("output_size (%d) must equal output_channels (%d)" % (output_size, output_channels))
        self._scope, self._decoder_names, self._default_length = name, False, int(input_size)
        self._setup(StackConfig(dilations=list(dilations), filter_width=filter_width,
                                dilation_channels=dilation_channels, skip_channels=skip_channels,
                                output_channels=output_channels, shift_input=False, head_mode="pooled",
                                dtype=dtype or _default_dtype(), learning_rate=learning_rate, gate_mode=gate_mode), seed)
        self.gate_mode = gate_mode

    def _stage(self, inputs, targets=None):
        x = np.asarray(inputs, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("inputs must be [batch, samples]")
        if x.shape[1] != self.input_size:
            # tf.nn.pool window = input_size, VALID (model.py:58): other lengths would pool differently
            raise ValueError("inputs have %d samples, the model was built for input_size=%d" % (x.shape[1], self.input_size))
        eng = self._engine(x.shape[0], x.shape[1])
        t = None
        if targets is not None:
            t = torch.as_tensor(np.asarray(targets, dtype=np.float32), device="cuda")
            if tuple(t.shape) != (x.shape[0], self.output_size):
                raise ValueError("targets must be [batch, %d]" % self.output_size)
        eng.set_inputs(torch.as_tensor(x, device="cuda"), t)
        return eng

    def train(self, inputs, targets):
        self._refuse_in_ema("train")
        eng = self._stage(inputs, targets)
        _train_step(eng)
        return np.float32(eng.loss.item())

    def fit(self, sampler, steps, validate=None):
        """``steps`` training steps on batches a ``dataset.BatchSampler`` draws on the device (the labels' one-hot rows
        are the targets); returns every step's loss, float32 [steps].  See ``_fit``.

        ``validate=(eval_sampler, every)``: one sweep of a ``dataset.EvalSampler`` (``evaluate``'s) is enqueued behind
        every training step whose count -- ``sampler.step`` after the step -- is a multiple of `every`, as replays of a
        graph of its own between the training graph's.  Each sweep lands in the next of the sampler's result slots, so
        the host does not wait per sweep: the slots are read when ``sweep_capacity`` of them are full and at the end.
        Returns ``(losses, [EvalResult, ...])`` then, every result with the ``step`` it was taken at.  The training run's
        bits are the ones without validation.  Under ``set_training_controls(..., validate_ema=True)`` every sweep runs on
        the EMA weights (``swap_ema`` in front of it and behind it, enqueued like the sweep itself)."""
        from .dataset import EvalSampler
        self._refuse_in_ema("fit")
        if isinstance(sampler, EvalSampler):
            raise TypeError("WaveNet.fit: an EvalSampler sweeps a held-out set; train on dataset.sampler(...)")
        if sampler.num_samples != self.input_size:
            raise ValueError("inputs have %d samples, the model was built for input_size=%d"
                             % (sampler.num_samples, self.input_size))
        _fit_labels(sampler, self.output_size, "WaveNet", "targets")
        if validate is None:
            eng = self._engine(sampler.batch_size, sampler.num_samples)
            return _fit(eng, sampler, steps, dict(audio=eng.audio, onehot=eng.labels))[0]
        ev, every = _check_validate(validate)
        self._check_eval(ev)
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        eng_v = self._engine(ev.batch_size, ev.num_samples)
        results, pending = [], []            # pending: (sweep number, training step) of the sweeps still in their slots

        def drain():                         # the host waits here
            results.extend(ev.result(k, s) for k, s in pending)
            del pending[:]

        def after_step():
            if sampler.step % every == 0:
                if len(pending) >= ev.sweep_capacity:
                    drain()
                if self._validate_ema():         # the sweep judges the averaged weights: swapped in and out on its stream
                    eng.swap_ema()
                _eval_sweep(eng_v, ev)
                if self._validate_ema():
                    eng.swap_ema()
                pending.append((ev.sweep - 1, sampler.step))

        losses = _fit(eng, sampler, steps, dict(audio=eng.audio, onehot=eng.labels), after_step=after_step)[0]
        drain()
        return losses, results

    def _check_eval(self, ev):
        from .dataset import EvalSampler
        if not isinstance(ev, EvalSampler):
            raise TypeError("WaveNet.evaluate takes a dataset.EvalSampler (dataset.eval_sampler(...)), got %s"
                            % type(ev).__name__)
        if ev.num_samples != self.input_size:
            raise ValueError("inputs have %d samples, the model was built for input_size=%d"
                             % (ev.num_samples, self.input_size))
        if ev.dataset.num_classes != int(self.output_size):
            raise ValueError("WaveNet.evaluate: the dataset has num_classes=%d, the model's posteriors are %d wide"
                             % (ev.dataset.num_classes, int(self.output_size)))

    def evaluate(self, eval_sampler, step=None):
        """One sweep of a labelled held-out set on the device -- the reference driver's test mode (train.py:90-120)
        without its loop of uploads and downloads: ``sweep_steps`` steps of {draw, forward pass, ``srwn_eval_classes``},
        the host waits once at the end.  Returns an ``EvalResult`` (dataset.py): per record the predicted class, the rank
        of the label's class and -log p(label); the confusion matrix, accuracy, top-k accuracy, mean NLL and per-class
        (correct, total).  The sampler's batch size may differ from the training one: the engine of that shape runs on
        the model's current parameters, as ``predict`` does.  Nothing else changes: the parameters, the Adam moments,
        the optimizer's step and a training sampler's state keep their bits.  With world > 1 this rank sweeps and returns
        its own share (``EvalResult.owned``); merging -- adding ``confusion``, taking each record from the rank that saw
        it -- is the caller's."""
        self._check_eval(eval_sampler)
        eng = self._engine(eval_sampler.batch_size, eval_sampler.num_samples)
        _eval_sweep(eng, eval_sampler)
        return eval_sampler.result(eval_sampler.sweep - 1, step)          # the host waits here

    def predict(self, inputs):
        eng = self._stage(inputs)
        eng.forward(with_loss=False)
        return eng.probs.cpu().numpy()[:, None, :]

    def recognizer(self, max_batch=1, hop=None, window=None, max_hops=8):
        """A ``StreamingClassifier`` on a copy of this model's current weights: audio of any length in, the pooled
        posteriors of a window of `window` samples (default input_size) sliding by `hop` (default: the window) out.  With
        hop = window = input_size its single emission on a clip of input_size samples is ``predict``'s."""
        window = int(self.input_size if window is None else window)
        hop = window if hop is None else int(hop)
        from .recognizer import ClassifierWeights, check_classifier_widths, check_hop_window
        check_hop_window(hop, window)
        if self.gate_mode != "reference":
            raise NotImplementedError("gate_mode %r is not built for the streaming classifier" % (self.gate_mode,))
        check_classifier_widths(self.filter_width, self.dilation_channels, self.skip_channels)
        if self._primary is None:
            self._engine(1, self._default_length)
        return StreamingClassifier(ClassifierWeights.from_engine(self._primary), max_batch=max_batch, hop=hop,
                                   window=window, max_hops=max_hops)


class StreamingClassifier(object):
    """The deployable form of the ``WaveNet`` classifier (createNetwork, model.py:33-62) with a NumPy face: no training
    engine, no clip length.  ``classify(audio [B, T])`` -> probabilities [B, n_emit, C] of every window position
    (j + 1) * hop - window, j >= window / hop - 1, of a recording of any length; ``stream(batch)`` -> a
    ``ClassifierStream`` to ``push`` audio into as it arrives.  An emission does not depend on how the audio was cut."""

    def __init__(self, weights, max_batch=1, hop=160, window=16000, max_hops=8):
        from .recognizer import StreamClassifier
        self._w = weights
        self._eng = StreamClassifier(weights, max_batch=max_batch, hop=hop, window=window, max_hops=max_hops)
        self.max_batch, self.hop, self.window = self._eng.max_batch, self._eng.hop, self._eng.window

    @classmethod
    def from_checkpoint(cls, logdir, dilations, output_channels, dilation_channels=32, skip_channels=256, filter_width=2,
                        name="WaveNet", dtype=None, max_batch=1, hop=160, window=16000, max_hops=8):
        """A classifier on the variables saved in `logdir` (``WaveNet.save``'s .pt form or a TensorFlow bundle, by the
        reference's variable names under `name`)."""
        from .recognizer import ClassifierWeights, check_classifier_widths, check_hop_window
        check_hop_window(hop, window)
        check_classifier_widths(filter_width, dilation_channels, skip_channels)
        w = ClassifierWeights(dilations, dilation_channels, skip_channels, output_channels, filter_width,
                              dtype or _default_dtype())
        if not w.load(logdir, name):
            raise FileNotFoundError("%s: no checkpoint to restore (WaveNet.save writes one)" % logdir)
        return cls(w, max_batch=max_batch, hop=hop, window=window, max_hops=max_hops)

    def classify(self, inputs, return_logits=False):
        """inputs [B, T] -> probabilities [B, n_emit, C] (NumPy), n_emit = max(0, T // hop - window / hop + 1)."""
        out = self._eng.classify(self._eng._check_audio(inputs), return_logits)
        return tuple(o.cpu().numpy() for o in out) if return_logits else out.cpu().numpy()

    def stream(self, batch_size=1):
        return ClassifierStream(self, self._eng.start(batch_size))

    def pool(self, audio_ring=None):
        """A ``ClassifierPool``: this classifier's ``max_batch`` rows as slots that streams join and leave, each pushing
        audio of any length at a clock of its own (``recognizer.ClassifierPool``).  audio_ring: samples a slot can hold
        (default 2 * max_hops * hop + 1).  Ends the current ``ClassifierStream``; ``stream`` and ``classify`` end the pool."""
        return ClassifierPool(self._eng.pool(audio_ring))


class ClassifierStream(object):
    """NumPy face of one running batch of classifier streams (``StreamingClassifier.stream``).  ``t``: samples received
    per stream; ``emitted``: emissions returned so far."""

    def __init__(self, owner, state):
        self._owner, self._st, self.batch_size = owner, state, state.B

    @property
    def t(self):
        return self._st.t

    @property
    def emitted(self):
        return self._st.emitted

    def push(self, audio, return_logits=False):
        """audio [B, n], any n >= 0 -> probabilities [B, k, C] of the k window positions it completed (k may be 0)."""
        out = self._owner._eng.push(self._st, audio, return_logits)
        return tuple(o.cpu().numpy() for o in out) if return_logits else out.cpu().numpy()


class StreamingScorer(object):
    """The deployable likelihood scorer of the softmax ``WaveNetTeacher`` with a NumPy face: no training engine, no clip
    length.  ``score(audio [B, T])`` -> nll [B, T] in nats, nll[b, t] = -log p(mu_law_encode(audio)[b, t] | audio[b, < t]),
    for recordings of any length; ``stream(batch)`` -> a ``ScorerStream`` to ``push`` audio into as it arrives.  A value
    does not depend on how the audio was cut."""

    def __init__(self, weights, max_batch=1, max_chunk=1600):
        from .scorer import StreamScorer
        self._w = weights
        self._eng = StreamScorer(weights, max_batch=max_batch, max_chunk=max_chunk)
        self.max_batch, self.max_chunk = self._eng.max_batch, self._eng.max_chunk

    @classmethod
    def from_checkpoint(cls, logdir, dtype=None, max_batch=1, max_chunk=1600):
        """A scorer on the variables ``WaveNetTeacher.save`` left in `logdir` (its config.json names the stack; the
        checkpoint is this package's .pt form or a TensorFlow bundle, read by the reference's variable names)."""
        import json
        from types import SimpleNamespace
        from .recognizer import check_classifier_widths
        from .scorer import ScorerWeights
        path = os.path.join(logdir, "config.json")
        if not os.path.exists(path):
            raise FileNotFoundError("%s: no config.json (save the teacher with WaveNetTeacher.save)" % logdir)
        c = json.load(open(path))
        ScorerWeights.check_config(SimpleNamespace(
            head_mode="per_timestep" if c.get("head", "softmax") == "softmax" else "mol", gate_mode=c.get("gate_mode", "reference"),
            cond_channels=(c["latent_channels"] + c["condition_size"]) if c.get("use_encoding") else 0, shift_input=True))
        check_classifier_widths(c["filter_width"], c["dilation_channels"], c["skip_channels"], "streaming scorer")
        w = ScorerWeights(c["dilations"], c["dilation_channels"], c["skip_channels"], c["quantization_channels"],
                          c["filter_width"], dtype or _default_dtype())
        if not w.load(logdir, c.get("name", "WaveNetTeacher")):
            raise FileNotFoundError("%s: no checkpoint to restore (WaveNetTeacher.save writes one)" % logdir)
        return cls(w, max_batch=max_batch, max_chunk=max_chunk)

    @staticmethod
    def _numpy(out):
        return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()

    def score(self, inputs, return_logits=False, return_best=False):
        """inputs [B, T] -> nll [B, T] (NumPy, nats); with return_logits also the logits [B, T, C], with return_best also
        the most likely code [B, T]."""
        return self._numpy(self._eng.score(self._eng._check_audio(inputs), return_logits, return_best))

    def stream(self, batch_size=1):
        return ScorerStream(self, self._eng.start(batch_size))

    def pool(self, audio_ring=None):
        """A ``ScorerStreamPool``: this scorer's ``max_batch`` rows as slots that streams join and leave, each pushing audio
        of any length at a clock of its own (``scorer.ScorerPool``).  audio_ring: samples a slot can hold (default 2 *
        max_chunk + 2).  Ends the current ``ScorerStream``; ``stream`` and ``score`` end the pool."""
        return ScorerStreamPool(self._eng.pool(audio_ring))


class ScorerStream(object):
    """NumPy face of one running batch of scorer streams (``StreamingScorer.stream``).  ``t``: samples scored per
    stream."""

    def __init__(self, owner, state):
        self._owner, self._st, self.batch_size = owner, state, state.B

    @property
    def t(self):
        return self._st.t

    def push(self, audio, return_logits=False, return_best=False):
        """audio [B, n], any n >= 0 -> nll [B, n] of exactly those samples."""
        return self._owner._numpy(self._owner._eng.push(self._st, audio, return_logits, return_best))

    def bits_per_sample(self):
        """Mean nll of everything pushed so far, in bits, per stream [B] (NaN before the first sample)."""
        from .scorer import bits_per_sample
        return np.array([bits_per_sample(v, self._st.t) for v in self._st.nll_sum.cpu().numpy()])


class _MolScorerFace(object):
    """What ``StreamingMolScorer`` and ``AutoEncoderScorer`` share: a ``scorer.MolStreamScorer`` ``_eng`` on a snapshot of
    decoder weights ``_w``, and the tiling of clip-level conditions onto encoding frames (``with_conditions``)."""

    def _setup(self, weights, latent_channels, condition_size, max_batch, max_chunk, max_frames):
        from .scorer import MolStreamScorer
        self._w = weights
        self.latent_channels, self.condition_size = int(latent_channels), int(condition_size)
        self._eng = MolStreamScorer(weights, max_batch=max_batch, max_chunk=max_chunk, max_frames=max_frames)
        self.max_batch, self.max_chunk, self.max_frames = self._eng.max_batch, self._eng.max_chunk, self._eng.max_frames
        self.pool_stride, self.conditioned = int(self._eng.pool), bool(self._eng.E)

    def _conditions(self, batch, conditions):
        """conditions [B, condition_size] on the device, or None (no device work before the refusals)."""
        if not self.conditioned:
            if conditions is not None:
                raise ValueError("this decoder is not conditioned")
            return None
        c = _check_conditions(batch, conditions, self.condition_size, "scorer")
        return None if c is None else torch.as_tensor(c, device="cuda")

    def _frames(self, encoding, cond):
        """encoding [B, k, latent] (NumPy or device) -> the conditioning frames [B, k, latent + condition_size] (device)."""
        e = torch.as_tensor(encoding, dtype=torch.float32)
        if e.dim() != 3 or e.shape[2] != self.latent_channels:
            raise ValueError("encoding must be [batch, frames, latent_channels=%d], got %s"
                             % (self.latent_channels, tuple(e.shape)))
        e = e.to("cuda")
        return e if cond is None else _tile_conditions(e, cond)

    def _score(self, inputs, encoding, conditions, return_logits):
        x = self._eng._check_audio(inputs)
        enc = None
        if self.conditioned:
            if encoding is None:
                raise ValueError("this decoder is conditioned: pass encoding [batch, samples / pool_stride, %d]"
                                 % self.latent_channels)
            enc = self._frames(encoding, self._conditions(int(x.shape[0]), conditions))
        elif encoding is not None or conditions is not None:
            raise ValueError("this decoder is not conditioned")
        out = self._eng.score(x, enc, return_logits)
        return tuple(o.cpu().numpy() for o in out) if return_logits else out.cpu().numpy()


class _MolScoreStreamBase(object):
    """NumPy face of one running batch of mixture-of-logistics scorer streams.  ``t``: samples scored per stream."""

    def __init__(self, owner, batch_size, conditions):
        self._owner, self.batch_size = owner, int(batch_size)
        self._cond = owner._conditions(self.batch_size, conditions)      # (its refusals come before any device work)
        self._st = owner._eng.start(self.batch_size)

    t = property(lambda self: self._st.t)
    fed = property(lambda self: self._st.fed)

    def bits_per_sample(self):
        """Mean nll of everything scored so far, in bits, per stream [B] (NaN before the first sample)."""
        from .scorer import bits_per_sample
        return np.array([bits_per_sample(v, self._st.t) for v in self._st.nll_sum.cpu().numpy()])


class StreamingMolScorer(_MolScorerFace):
    """The deployable likelihood scorer of the mixture-of-logistics ``WaveNetTeacher`` (the model the student distils
    from), conditioned or not, with a NumPy face: ``score(inputs [B, T], encoding, conditions)`` -> nll [B, T] in nats,
    nll[b, t] = -log p(inputs[b, t] | inputs[b, < t], encoding); ``stream(batch, conditions)`` -> a ``MolScorerStream`` to
    ``feed`` frames and ``push`` audio into as they arrive.  A value does not depend on how audio and frames were cut."""

    def __init__(self, weights, latent_channels=0, condition_size=0, max_batch=1, max_chunk=1600, max_frames=32):
        self._setup(weights, latent_channels, condition_size, max_batch, max_chunk, max_frames)

    def score(self, inputs, encoding=None, conditions=None, return_logits=False):
        """inputs [B, T] (T = frames * pool_stride for a conditioned teacher) -> nll [B, T] (NumPy, nats); with
        return_logits also the logits [B, T, 4 * num_mixtures]."""
        return self._score(inputs, encoding, conditions, return_logits)

    def stream(self, batch_size=1, conditions=None):
        return MolScorerStream(self, batch_size, conditions)

    def pool(self, audio_ring=None):
        """A ``MolScorerStreamPool``: this scorer's ``max_batch`` rows as slots that streams join and leave, each pushing
        audio and being fed frames at a clock of its own (``scorer.MolScorerPool``).  audio_ring: samples a slot can hold
        (default 2 * max_chunk + 2).  Ends the current ``MolScorerStream``; ``stream`` and ``score`` end the pool."""
        return MolScorerStreamPool(self, self._eng.pool(audio_ring))


class MolScorerStream(_MolScoreStreamBase):
    """``StreamingMolScorer.stream``: ``feed(encoding [B, k, latent])`` hands every stream its next k <= ``room`` frames,
    ``push(audio [B, n])`` scores the next n <= ``available`` samples (an unconditioned teacher: any n, nothing to feed)."""

    room = property(lambda self: self._owner._eng.room(self._st))
    available = property(lambda self: self._owner._eng.available(self._st))

    def feed(self, encoding):
        if not self._owner.conditioned:
            raise ValueError("feed: this teacher is not conditioned")
        self._owner._eng.feed(self._st, self._owner._frames(encoding, self._cond))

    def push(self, audio, return_logits=False):
        out = self._owner._eng.push(self._st, audio, return_logits)
        return tuple(o.cpu().numpy() for o in out) if return_logits else out.cpu().numpy()


class AutoEncoderScorer(_MolScorerFace):
    """The whole ``WaveNetAutoEncoder`` as a likelihood meter: an ``AudioEncoder`` (a snapshot of the encoder) feeding a
    ``scorer.MolStreamScorer`` on a snapshot of the decoder -- audio in, nll[b, t] = -log p(audio[b, t] | audio[b, < t],
    encode(audio)) in nats out, the number the auto-encoder is trained on, for recordings of any length.  ``score`` scores
    the (T // pool_stride) * pool_stride samples whose frames exist; ``stream`` does so as the audio arrives, a sample as
    soon as the encoder has completed its frame, with the same bits however the audio was cut."""

    def __init__(self, encoder, weights, condition_size=0, max_batch=1, max_chunk=1600, max_frames=32):
        if not isinstance(encoder, AudioEncoder):
            raise TypeError("AutoEncoderScorer(encoder: AudioEncoder, weights: scorer.MolScorerWeights)")
        if int(encoder.pool_stride) != int(weights.pool) or weights.E != encoder.latent_channels + int(condition_size):
            raise ValueError("the encoder gives %d-channel frames per %d samples, the decoder takes %d channels (%d of "
                             "them conditions) per %d" % (encoder.latent_channels, encoder.pool_stride, weights.E,
                                                          int(condition_size), weights.pool))
        self.encoder = encoder
        self._setup(weights, encoder.latent_channels, condition_size, max_batch, max_chunk, max_frames)

    @classmethod
    def from_checkpoint(cls, logdir, dtype=None, max_batch=1, max_chunk=1600, max_frames=32):
        """A scorer on the variables ``WaveNetAutoEncoder.save`` left in `logdir` (its config.json names both halves)."""
        import json
        from .scorer import MolScorerWeights
        path = os.path.join(logdir, "config.json")
        if not os.path.exists(path):
            raise FileNotFoundError("%s: no config.json (save the model with WaveNetAutoEncoder.save)" % logdir)
        c = json.load(open(path))
        dt = dtype or _default_dtype()
        enc = AudioEncoder.from_checkpoint(logdir, dtype=dt, max_batch=max_batch, max_frames=max_frames)
        w = MolScorerWeights(c["dilations"], c["dilation_channels"], c["skip_channels"], c["num_mixtures"],
                             c["latent_channels"] + c["condition_size"], c["pool_stride"], c["filter_width"], dt)
        if not w.load(logdir, c.get("name", "WaveNetAutoEncoder") + "/Decoder"):
            raise FileNotFoundError("%s: no checkpoint to restore (WaveNetAutoEncoder.save writes one)" % logdir)
        return cls(enc, w, c["condition_size"], max_batch=max_batch, max_chunk=max_chunk, max_frames=max_frames)

    def score_with_encoding(self, inputs, encoding, conditions=None, return_logits=False):
        """inputs [B, frames * pool_stride], encoding [B, frames, latent_channels] -> nll (NumPy, nats)."""
        return self._score(inputs, encoding, conditions, return_logits)

    def score(self, inputs, conditions=None, return_logits=False):
        """inputs [B, T] of any T -> nll [B, (T // pool_stride) * pool_stride] under the encoding of the inputs."""
        x = self.encoder._check(inputs)
        enc = self.encoder._eng.encode(torch.as_tensor(x))
        return self._score(x[:, :int(enc.shape[1]) * self.pool_stride], enc, conditions, return_logits)

    def stream(self, batch_size=1, conditions=None):
        if not 1 <= int(batch_size) <= min(self.max_batch, self.encoder.max_batch):
            raise ValueError("batch_size %r: this scorer holds %d streams" % (batch_size, min(self.max_batch, self.encoder.max_batch)))
        return AutoEncoderScoreStream(self, int(batch_size), conditions)

    def pool(self, audio_ring=None):
        """An ``AutoEncoderScorerPool``: an encoder pool feeding a scorer pool, slot by slot, each stream at a clock of its
        own.  audio_ring: samples a slot of the SCORER half can hold (default: the encoder pool's ring plus max_chunk + 2;
        at least ``scorer.ae_pool_min_audio_ring``).  Ends the current stream of either half."""
        return AutoEncoderScorerPool(self, audio_ring)


class AutoEncoderScoreStream(_MolScoreStreamBase):
    """``AutoEncoderScorer.stream``: ``push(audio [B, n])``, any n, returns the nll of every sample whose frame the encoder
    has completed by now ([B, m], m >= 0); audio that cannot be scored yet waits on the device.  ``finish()`` returns the
    rest (the encoder's last whole frames, with its clip-end padding) and closes the stream.  ``received``: samples
    pushed; ``t``: samples scored."""

    def __init__(self, owner, batch_size, conditions):
        super().__init__(owner, batch_size, conditions)
        self._enc = owner.encoder._eng.start(self.batch_size)
        self._backlog = torch.zeros((self.batch_size, 0), dtype=torch.float32, device="cuda")

    received = property(lambda self: self._enc.received)

    def _drain(self, frames):
        """frames [B, k, latent] (device) into the ring and every sample they allow: feed -> push -> feed while the ring
        has less room than the frames that are due."""
        o, st, outs = self._owner, self._st, []
        eng, k, f0 = o._eng, int(frames.shape[1]), 0
        while True:
            if f0 < k:
                r = min(eng.room(st), k - f0)
                if r > 0:
                    eng.feed(st, o._frames(frames[:, f0:f0 + r], self._cond))
                    f0 += r
            n = int(eng.available(st))
            if n <= 0:
                if f0 < k:      # (cannot happen: max_frames >= live_min_frames leaves room once every sample is scored)
                    raise RuntimeError("the conditioning ring has no room and no sample to score")
                break
            outs.append(eng.push(st, self._backlog[:, :n]))
            self._backlog = self._backlog[:, n:]
        if not outs:
            return np.zeros((self.batch_size, 0), np.float32)
        return torch.cat(outs, dim=1).cpu().numpy()

    def push(self, audio):
        if self._enc.closed:
            raise ValueError("this stream is closed (finish was called)")
        x = torch.as_tensor(self._owner.encoder._check(audio, self.batch_size))
        frames = self._owner.encoder._eng.push(self._enc, x)
        self._backlog = torch.cat([self._backlog, x.to("cuda")], dim=1)
        return self._drain(frames)

    def finish(self):
        out = self._drain(self._owner.encoder._eng.finish(self._enc))
        self._backlog = self._backlog[:, :0]
        return out


class WaveNetTeacher(_EngineOwner):
    """The mu-law softmax teacher of BASELINE.json configs[1-2]: ``createDecoder``'s stack
    (model.py:158-196: RightShift teacher forcing, per-layer conditioning add) with a
    ``quantization_channels``-way softmax over mu-law codes per sample (model.py:100-112).

    ``train(inputs[B,T], encoding=None, conditions=None) -> loss`` (mean CE over B*T);
    ``get_logits`` / ``predict_codes`` for evaluation.  ``encoding`` is [B, T/pool_stride, latent];
    ``conditions`` [B, condition_size] is tiled over frames and concatenated (model.py:161-167).
    """

    def __init__(self, input_size, condition_size, dilations, filter_width=2, dilation_channels=32,
                 skip_channels=256, quantization_channels=256, latent_channels=16, pool_stride=512,
                 name="WaveNetTeacher", learning_rate=0.001, use_encoding=False, dtype=None, seed=0,
                 head="softmax", num_mixtures=5, *, gate_mode="reference"):
        """gate_mode: "reference" (default) = the gate the reference runs, c = z*sigmoid(z) (ops.py:33); "wavenet" = the
        canonical tanh(Wf*x) * sigmoid(Wg*x), which also trains the `_gate` variables (generation is not built for it)."""
        if gate_mode not in ("reference", "wavenet"):
            raise ValueError("gate_mode %r: 'reference' or 'wavenet'" % (gate_mode,))
        self._ctor = dict(input_size=int(input_size), condition_size=int(condition_size),
                          dilations=[int(d) for d in dilations], filter_width=int(filter_width),
                          dilation_channels=int(dilation_channels), skip_channels=int(skip_channels),
                          quantization_channels=int(quantization_channels), latent_channels=int(latent_channels),
                          pool_stride=int(pool_stride), name=name, learning_rate=float(learning_rate),
                          use_encoding=bool(use_encoding), seed=int(seed), head=head, num_mixtures=int(num_mixtures),
                          gate_mode=gate_mode)
        self.gate_mode = gate_mode
        self.input_size = input_size
        self.condition_size = condition_size
        self.dilations = dilations
        self.quantization_channels = quantization_channels
        self.latent_channels = latent_channels
        self.pool_stride = pool_stride
        self.use_encoding = bool(use_encoding)
        self.head = head
        self.num_mixtures = num_mixtures
        if head not in ("softmax", "mol"):
            raise ValueError("head must be 'softmax' (mu-law classes) or 'mol' (mixture of logistics, model.py:114)")
        cond_ch = (latent_channels + condition_size) if self.use_encoding else 0
        self._scope, self._decoder_names, self._default_length = name, bool(cond_ch), int(input_size)
        self._setup(StackConfig(dilations=list(dilations), filter_width=filter_width,
                                dilation_channels=dilation_channels, skip_channels=skip_channels,
                                output_channels=quantization_channels if head == "softmax" else 4 * num_mixtures,
                                cond_channels=cond_ch, pool_stride=pool_stride if cond_ch else 1, shift_input=True,
                                head_mode="per_timestep" if head == "softmax" else "mol",
                                dtype=dtype or _default_dtype(),
                                learning_rate=learning_rate, gate_mode=gate_mode), seed)

    def save(self, logdir, global_step, force=False, fmt=None):
        """Checkpoint + ``config.json`` (the constructor arguments; the reference gets them from the meta graph
        it imports at model.py:318)."""
        done = super().save(logdir, global_step, force, fmt)
        if done:
            import json
            with open(os.path.join(logdir, "config.json"), "w") as f:
                json.dump(self._ctor, f)
        return done

    @classmethod
    def from_checkpoint(cls, logdir, dtype=None):
        import json
        path = os.path.join(logdir, "config.json")
        if not os.path.exists(path):
            raise FileNotFoundError("%s: no config.json (save the teacher with WaveNetTeacher.save)" % logdir)
        m = cls(dtype=dtype, **json.load(open(path)))
        if not m.load(logdir):
            raise FileNotFoundError("%s: no checkpoint to restore" % logdir)
        return m

    def _stage(self, inputs, encoding=None, conditions=None):
        x = torch.as_tensor(np.asarray(inputs, dtype=np.float32), device="cuda")
        B, T = x.shape
        eng = self._engine(B, T)
        cond = None
        if self.use_encoding:
            if encoding is None:
                raise ValueError("this teacher was built with use_encoding=True; pass encoding [B, T/pool, latent]")
            e = torch.as_tensor(np.asarray(encoding, dtype=np.float32), device="cuda")
            if self.condition_size > 0:
                c = torch.as_tensor(np.asarray(conditions, dtype=np.float32), device="cuda")
                e = _tile_conditions(e, c)
            cond = e.contiguous()
        codes = None
        if self.head == "softmax":
            codes = K.mu_law_encode(x.contiguous(), self.quantization_channels)        # ops.py:82-93
        eng.set_inputs(x, codes, cond)
        return eng

    def train(self, inputs, encoding=None, conditions=None):
        self._refuse_in_ema("train")
        eng = self._stage(inputs, encoding, conditions)
        _train_step(eng)
        return np.float32(eng.loss.item())

    def fit(self, sampler, steps):
        """``steps`` training steps on batches a ``dataset.BatchSampler`` draws on the device (with the softmax head the
        draw writes the mu-law targets too); returns every step's loss, float32 [steps].  See ``_fit``.  The unconditioned
        teacher only: a conditioned teacher's encoding comes from another model."""
        self._refuse_in_ema("fit")
        if self.use_encoding:
            raise NotImplementedError("WaveNetTeacher.fit: this teacher was built with use_encoding=True and its encoding "
                                      "comes from another model; feed it with train(inputs, encoding, conditions)")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        dest = dict(audio=eng.audio)
        if self.head == "softmax":
            dest.update(codes=eng.targets, quantization_channels=self.quantization_channels)
        return _fit(eng, sampler, steps, dest)[0]

    def evaluate(self, sampler):
        """The forward-only loss -- ``loss(batch)`` -- of every step of one sweep over the sampler's dataset, float32
        [len(dataset) / (batch_size * world)] in the steps' order, with one host wait per ``log_capacity`` steps.  The loss
        kernel gives a batch mean (softmax) or sum (mixture of logistics), not per-clip values, so `sampler` is a plain
        ``dataset.sampler(..., shuffle=False)`` whose batches divide the set.  Per-sample held-out likelihoods of any
        clip exist already: the streaming scorers (``scorer()``, ``mol_scorer()``).  No parameter changes.  The
        unconditioned teacher only, as ``fit``."""
        if self.use_encoding:
            raise NotImplementedError("WaveNetTeacher.evaluate: this teacher was built with use_encoding=True and its "
                                      "encoding comes from another model; use loss(inputs, encoding, conditions)")
        _loss_sweep_steps(sampler, "WaveNetTeacher")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        dest = dict(audio=eng.audio)
        if self.head == "softmax":
            dest.update(codes=eng.targets, quantization_channels=self.quantization_channels)
        return _evaluate_losses(eng, sampler, dest, "WaveNetTeacher")

    def get_logits(self, inputs, encoding=None, conditions=None):
        eng = self._stage(inputs, encoding, conditions)
        return eng.forward(want_logits=True).cpu().numpy()

    def loss(self, inputs, encoding=None, conditions=None):
        eng = self._stage(inputs, encoding, conditions)
        eng.forward()
        return np.float32(eng.loss.item())

    def scorer(self, max_batch=1, max_chunk=1600):
        """A ``StreamingScorer`` on a copy of this teacher's current weights: audio of any length in, nll[b, t] = -log
        p(code[b, t] | audio[b, < t]) in nats out, one number per sample -- the quantity ``loss`` averages, without the
        training engine.  The unconditioned softmax teacher with the reference gate only."""
        from .recognizer import check_classifier_widths
        from .scorer import ScorerWeights
        ScorerWeights.check_config(self._cfg)
        check_classifier_widths(self._cfg.filter_width, self._cfg.dilation_channels, self._cfg.skip_channels,
                                "streaming scorer")
        if self._primary is None:
            self._engine(1, self._default_length)
        return StreamingScorer(ScorerWeights.from_engine(self._primary), max_batch=max_batch, max_chunk=max_chunk)

    def mol_scorer(self, max_batch=1, max_chunk=1600, max_frames=32):
        """A ``StreamingMolScorer`` on a copy of this teacher's current weights, for head="mol" teachers, conditioned
        (``score(inputs, encoding, conditions)``, frames fed through a ring of ``max_frames``) or not: nll[b, t] = -log
        p(inputs[b, t] | inputs[b, < t], encoding) in nats -- the quantity ``loss`` sums, without the training engine."""
        from .recognizer import check_classifier_widths
        from .scorer import MolScorerWeights
        MolScorerWeights.check_config(self._cfg)
        check_classifier_widths(self._cfg.filter_width, self._cfg.dilation_channels, self._cfg.skip_channels,
                                "streaming scorer")
        if self._primary is None:
            self._engine(1, self._default_length)
        return StreamingMolScorer(MolScorerWeights.from_engine(self._primary),
                                  self.latent_channels if self.use_encoding else 0,
                                  self.condition_size if self.use_encoding else 0, max_batch=max_batch,
                                  max_chunk=max_chunk, max_frames=max_frames)

    def generate(self, batch_size, num_samples, mode="sample", seed=0, forced=None, return_logits=False,
                 encoding=None, conditions=None, prompt=None, *, temperature=1.0, top_k=0, top_p=1.0):
        """Queue-cached autoregressive generation (the O(T L) replacement of the reference's O(T^2 L)
        loop, teacher.py:140-171): returns audio [B, num_samples] float32, or (audio, codes, logits) when
        return_logits.  `forced` [B, num_samples] = teacher forcing.  The softmax teacher emits mu-law decoded
        samples; the mixture-of-logistics teacher (optionally conditioned on `encoding`) emits logistic samples.
        `prompt` [B, P]: the num_samples that FOLLOW the prompt (one parallel pass over it primes the generator).
        temperature / top_k / top_p (mode "sample"; each a scalar or one entry per utterance): divide the logits by the
        temperature, keep the top_k most likely classes, keep the smallest set of classes holding top_p of the mass, then
        draw with the step's usual uniform; the mixture-of-logistics head takes the temperature only (on the mixture
        choice and the logistic noise).  The defaults are the plain draw."""
        ctl = dict(temperature=temperature, top_k=top_k, top_p=top_p)
        if prompt is not None:
            p = self._check_generation(batch_size, prompt)
            self._check_sampling(batch_size, ctl, "generate")
            eng = self._primary or self._engine(1, self._default_length)
            st = eng.generation_state(int(batch_size), self._generation_cond(encoding, conditions), seed, **ctl)
            eng.prime(st, p)
            f = None if forced is None else torch.as_tensor(np.asarray(forced, dtype=np.float32), device="cuda")
            a, c, lg = eng.generate_chunk(st, int(num_samples), mode=mode, forced=f, want_logits=return_logits)
            if return_logits:
                return a.cpu().numpy(), c.cpu().numpy(), lg.cpu().numpy()
            return a.cpu().numpy()
        if self.head == "softmax" and self.use_encoding:
            raise NotImplementedError("generation: the conditioned softmax teacher is not built")
        if self.gate_mode == "wavenet":
            raise NotImplementedError("generation: gate_mode 'wavenet' is trained only (the generation kernels implement "
                                      "the reference gate)")
        self._check_sampling(batch_size, ctl, "generate")
        eng = self._primary or self._engine(1, self._default_length)
        f = None if forced is None else torch.as_tensor(np.asarray(forced, dtype=np.float32), device="cuda")
        cond = self._generation_cond(encoding, conditions)
        a, c, lg = eng.generate(int(num_samples), mode=mode, seed=seed, forced=f, want_logits=return_logits,
                                batch=int(batch_size), cond=cond, **ctl)
        if return_logits:
            return a.cpu().numpy(), c.cpu().numpy(), lg.cpu().numpy()
        return a.cpu().numpy()

    def stream(self, batch_size, chunk_size, mode="sample", seed=0, prompt=None, encoding=None, conditions=None,
               max_samples=None, *, temperature=1.0, top_k=0, top_p=1.0):
        """Real-time generation: an iterator of NumPy [B, chunk_size] blocks (the last one shorter where max_samples or
        the encoding ends), each back as soon as its samples exist.  The blocks put together are generate(..., seed) bit
        for bit.  prompt [B, P]: continue from it.  A conditioned decoder stops where the encoding's frames run out
        (frames * pool_stride samples in all, the prompt included); otherwise the stream ends only at max_samples.
        temperature / top_k / top_p: the sampling controls of `generate`, for the whole stream."""
        p = self._check_generation(batch_size, prompt)
        if int(chunk_size) < 1:
            raise ValueError("chunk_size must be >= 1")
        ctl = dict(temperature=temperature, top_k=top_k, top_p=top_p)
        self._check_sampling(batch_size, ctl, "stream")
        eng = self._primary or self._engine(1, self._default_length)
        st = eng.generation_state(int(batch_size), self._generation_cond(encoding, conditions), seed, **ctl)
        if p is not None:
            eng.prime(st, p)
        return _stream_chunks(eng, st, int(chunk_size), mode, max_samples)

    def generation_pool(self, capacity, frames=None, mode="sample"):
        """A pool of `capacity` generation slots that streams join and leave while it runs (GenerationPool).  A conditioned
        (mixture-of-logistics) teacher takes `frames`, the most encoding frames a stream brings; each join then takes one
        encoding [frames_i, latent] (and conditions [condition_size]) per stream."""
        self._check_generation(1, None)
        if int(capacity) < 1:
            raise ValueError("generation_pool: capacity %d" % int(capacity))
        if self.use_encoding and (frames is None or int(frames) < 1):
            raise ValueError("this teacher was built with use_encoding=True; pass frames")
        eng = self._primary or self._engine(1, self._default_length)
        return GenerationPool(eng.generation_pool(int(capacity), frames if self.use_encoding else None),
                              self._pool_cond, mode)

    def _pool_cond(self, n, encoding, conditions):
        if not self.use_encoding:
            if encoding is not None:
                raise ValueError("this teacher is not conditioned: no encoding")
            return None
        return _pool_encodings(n, encoding, conditions, self.latent_channels, self.condition_size)

    def _check_sampling(self, n, ctl, who):
        """The sampling controls' ranges, before any device work (engine.sampling_table)."""
        from .engine import sampling_table
        mol = self.head == "mol"
        sampling_table(int(n), ctl["temperature"], ctl["top_k"], ctl["top_p"],
                       64 if mol else int(self.quantization_channels), mol, who)      # (a mixture head refuses top_k)

    def _check_generation(self, batch_size, prompt):
        """What generation refuses before any device work; returns the prompt as float32 [B, P] (or None)."""
        if self.head == "softmax" and self.use_encoding:
            raise NotImplementedError("generation: the conditioned softmax teacher is not built")
        if self.gate_mode == "wavenet":
            raise NotImplementedError("generation: gate_mode 'wavenet' is trained only (the generation kernels implement "
                                      "the reference gate)")
        return _check_prompt(batch_size, prompt)

    def _generation_cond(self, encoding, conditions):
        if not self.use_encoding:
            return None
        if encoding is None:
            raise ValueError("this teacher was built with use_encoding=True; pass encoding [B, frames, latent]")
        cond = torch.as_tensor(np.asarray(encoding, dtype=np.float32), device="cuda")
        if self.condition_size > 0:
            c = torch.as_tensor(np.asarray(conditions, dtype=np.float32), device="cuda")
            cond = _tile_conditions(cond, c)
        return cond.contiguous()


def _pool_encodings(n, encoding, conditions, latent, condition_size):
    """The per-stream encodings of a pool join: n of [frames_i, latent] (+ conditions [condition_size] tiled over the
    frames) -> n float32 arrays [frames_i, latent + condition_size]."""
    if encoding is None:
        raise ValueError("this decoder is conditioned: pass encoding, one [frames, latent] per stream")
    encs = per_stream(encoding, n, "encodings")
    conds = per_stream(conditions, n, "conditions")
    out = []
    for e, c in zip(encs, conds):
        e = np.asarray(e, dtype=np.float32)
        if e.ndim != 2 or e.shape[1] != latent:
            raise ValueError("join: each encoding is [frames, %d], got shape %s" % (latent, e.shape))
        if condition_size > 0:
            if c is None:
                raise ValueError("built with condition_size > 0: pass conditions, one [%d] per stream" % condition_size)
            e = _tile_conditions_np(e, np.asarray(c, dtype=np.float32).reshape(1, condition_size))
        out.append(e)
    return out


def _check_prompt(batch_size, prompt):
    if prompt is None:
        return None
    p = np.asarray(prompt, dtype=np.float32)
    if p.ndim != 2 or p.shape[0] != int(batch_size):
        raise ValueError("prompt must be [batch=%d, P], got shape %s" % (int(batch_size), p.shape))
    return p


def _stream_chunks(eng, st, chunk, mode, max_samples):
    """The blocks of a primed generation state (WaveNetEngine.generate_chunk) until max_samples or the encoding ends."""
    made = 0
    while True:
        n = chunk
        if max_samples is not None:
            n = min(n, int(max_samples) - made)
        if st.limit is not None:
            n = min(n, st.limit - st.t)
        if n <= 0:
            return
        a, _, _ = eng.generate_chunk(st, n, mode=mode)
        made += n
        yield a.cpu().numpy()


def _ran_dict(a, ran, slots):
    """A pool step's device rows a [capacity, n] as {slot: its ran[slot] samples} (NumPy) for the `slots` that made some."""
    a = a.cpu().numpy()
    return {u: a[u, :int(ran[u])] for u in slots if ran[u] > 0}


def _host_dict(d):
    """A pool step's {slot: device rows} as {slot: NumPy rows}, with ONE device-to-host copy however many slots."""
    us = list(d)
    if len(us) < 2:
        return {u: d[u].cpu().numpy() for u in us}
    flat = torch.cat([d[u] for u in us], dim=0).cpu().numpy()
    return dict(zip(us, np.split(flat, np.cumsum([d[u].shape[0] for u in us])[:-1])))


def _audio_pieces(slots, audio):
    """What a pool's ``push`` was given as one array per slot: one slot, or one 1-D array, is a single piece."""
    one = np.isscalar(slots) or (isinstance(audio, np.ndarray) and audio.dtype != object and audio.ndim == 1)
    return [np.asarray(a) for a in ([audio] if one else audio)]


class _PoolFace(object):
    """What the NumPy faces of the pools share: ``self._pool``'s slot view, forwarded."""

    capacity = property(lambda self: self._pool.capacity)
    active = property(lambda self: self._pool.active)
    free = property(lambda self: self._pool.free)

    def leave(self, slots):
        self._pool.leave(slots)


class GenerationPool(_PoolFace):
    """NumPy face of a generation pool (engine.GenerationPool): a fixed number of slots over one set of rings that streams
    join and leave while it runs.  ``join(seed=[...], prompt=[...], ...)`` takes one entry per stream and returns their
    slots; ``step(n)`` runs n pool steps in one launch and returns ``{slot: samples}`` of every slot that produced some; a
    stream that reaches its end frees its slot; ``leave(slots)`` ends streams early.  A stream's samples put together are
    what a batch-of-one ``generate`` with its seed and prompt returns.  On a live pool
    (``WaveNetAutoEncoder.generation_pool(..., live=True)``) ``join(..., live=True)`` / ``feed`` / ``room`` / ``close``
    mirror ``SynthesisPool``: the stream is fed while it runs and waits, with no samples, while it has none to make."""

    def __init__(self, pool, cond_fn, mode, latent=None, condition_size=0):
        self._pool, self._cond_fn, self.mode = pool, cond_fn, mode
        self._latent, self._cs = latent, int(condition_size)
        self._live_cond = {}      # slot -> the conditions of the live stream joined there last

    t = property(lambda self: self._pool.t)

    def join(self, seed, prompt=None, encoding=None, conditions=None, max_samples=None, *, temperature=None, top_k=None,
             top_p=None, live=False):
        """temperature / top_k / top_p: the joining streams' sampling controls (a scalar or one entry per stream; None = the
        default), as `generate` takes them.  encoding: one [frames_i, latent] per stream.
        live=True (a live pool): a single 2-D array is one stream; an encoding holds a stream's first frames ([0, latent]: none yet), its conditions are kept
        and tiled onto every frame fed later (``feed``); a live stream that has used up its frames waits (no samples)
        until it is fed, closed or left."""
        if live:
            K._need_gpu()
        if live and isinstance(encoding, np.ndarray) and encoding.ndim == 2:
            encoding = [encoding]
            conditions = None if conditions is None else [conditions]
        seeds = [int(s) for s in (seed if np.ndim(seed) else [seed])]
        n = len(seeds)
        prompts = per_stream(prompt, n, "prompts")
        for p in prompts:
            if p is not None and np.ndim(p) != 1:
                raise ValueError("join: each prompt is 1-D [P], got shape %s" % (np.shape(p),))
        prompts = [None if p is None else np.asarray(p, dtype=np.float32) for p in prompts]
        mx = per_stream(max_samples, n, "max_samples")
        cond = self._cond_fn(n, encoding, conditions)
        if live:
            slots = self._pool.join(seeds, prompts, cond, mx, temperature=temperature, top_k=top_k, top_p=top_p, live=True)
            if self._cs > 0:
                for u, c in zip(slots, per_stream(conditions, n, "conditions")):
                    self._live_cond[u] = np.asarray(c, dtype=np.float32).reshape(1, self._cs)
            return slots
        if temperature is None and top_k is None and top_p is None:
            return self._pool.join(seeds, prompts, cond, mx)
        return self._pool.join(seeds, prompts, cond, mx, temperature=temperature, top_k=top_k, top_p=top_p)

    def feed(self, slots, encoding):
        """The next frames of live slots: encoding[i] [k_i, latent] for slots[i] (k_i <= ``room``)."""
        slots = slot_list(slots, self.capacity, "feed")
        if isinstance(encoding, np.ndarray) and encoding.ndim == 2:
            encoding = [encoding]
        encs = [np.asarray(e, dtype=np.float32) for e in encoding]
        if len(encs) != len(slots):
            raise ValueError("feed: %d slots but %d encodings" % (len(slots), len(encs)))
        for e in encs:
            if e.ndim != 2 or e.shape[1] != self._latent:
                raise ValueError("feed: each encoding is [k, %s], got shape %s" % (self._latent, e.shape))
        if self._cs > 0:
            if any(u not in self._live_cond for u in slots):
                raise ValueError("feed: slots %s are not all live streams of this pool" % (slots,))
            encs = [_tile_conditions_np(e, self._live_cond[u]) for u, e in zip(slots, encs)]
        self._pool.feed(slots, encs)

    def room(self, slot):
        return self._pool.room(int(slot))

    def close(self, slots):
        """No more frames will come for these live streams: each frees its slot at the end of what it was fed."""
        self._pool.close(slots)

    def step(self, n, mode=None, forced=None):
        a, _, _, ran = self._pool.step(int(n), mode=mode or self.mode, forced=forced)
        return _ran_dict(a, ran, range(self._pool.capacity))


class WaveNetAutoEncoder(_TrainingControls):
    """model.py:75-285 on ``encoder.AutoEncoderEngine``: the non-causal encoder (ResidualDilationLayerNC chain,
    skip sum -> latent 1x1 -> average pool) and the conditioned mixture-of-logistics decoder, trained jointly on
    ``discretized_mix_logistic_loss(inputs, logits)`` (model.py:103,114,116).

    NumPy in / NumPy out like the reference's ``sess.run`` wrappers; there is no session.  One (batch, length) per
    model object.  ``reconstruct*`` draw the sampler's uniforms on the device (``seed`` makes them repeatable)."""

    def __init__(self, input_size, condition_size, num_mixtures, dilations, filter_width=2, encoder_channels=128,
                 dilation_channels=32, skip_channels=256, latent_channels=16, pool_stride=512,
                 name="WaveNetAutoEncoder", learning_rate=0.001, dtype=None, seed=0):
        K._need_gpu()
        self._ctor = dict(input_size=int(input_size), condition_size=int(condition_size),
                          num_mixtures=int(num_mixtures), dilations=[int(d) for d in dilations],
                          filter_width=int(filter_width), encoder_channels=int(encoder_channels),
                          dilation_channels=int(dilation_channels), skip_channels=int(skip_channels),
                          latent_channels=int(latent_channels), pool_stride=int(pool_stride), name=name,
                          learning_rate=float(learning_rate), seed=int(seed))
        self.input_size = input_size
        self.condition_size = condition_size
        self.num_mixtures = num_mixtures
        self.dilations = dilations
        self.filter_width = filter_width
        self.encoder_channels = encoder_channels
        self.dilation_channels = dilation_channels
        self.skip_channels = skip_channels
        self.latent_channels = latent_channels
        self.pool_stride = pool_stride
        self._name, self._seed = name, seed
        self._cfg = StackConfig(dilations=list(dilations), filter_width=filter_width,
                                dilation_channels=dilation_channels, skip_channels=skip_channels,
                                output_channels=4 * num_mixtures, cond_channels=latent_channels + condition_size,
                                pool_stride=pool_stride, shift_input=True, head_mode="mol",
                                dtype=dtype or _default_dtype(), learning_rate=learning_rate)
        self._eng = None
        self._gen = None
        self.last_checkpoint_time = time.time()

    # ------------------------------------------------------------------------------------------------
    def _engine(self, B: int, T: int):
        from .encoder import AutoEncoderEngine
        if self._eng is None:
            self._eng = AutoEncoderEngine(self._cfg, B, T, self.encoder_channels, self.latent_channels,
                                          self.condition_size, "cuda", seed=self._seed)
            self._apply_controls(self._eng)
        elif (self._eng.B, self._eng.T) != (int(B), int(T)):
            raise NotImplementedError("WaveNetAutoEncoder: one (batch, length) per model object for now; built for "
                                      "%s, got %s" % ((self._eng.B, self._eng.T), (B, T)))
        return self._eng

    def _stage(self, inputs, conditions):
        x = torch.as_tensor(np.asarray(inputs, dtype=np.float32), device="cuda")
        if x.ndim != 2:
            raise ValueError("inputs must be [batch, samples]")
        eng = self._engine(*x.shape)
        c = None
        if self.condition_size > 0:
            if conditions is None:
                raise ValueError("this auto-encoder was built with condition_size > 0; pass conditions")
            c = torch.as_tensor(np.asarray(conditions, dtype=np.float32), device="cuda")
        eng.set_inputs(x, c)
        return eng

    def _put_encoding(self, eng, encoding):
        e = torch.as_tensor(np.asarray(encoding, dtype=np.float32), device="cuda")
        d = eng.dec
        if tuple(e.shape) != (eng.B, d.frames, self.latent_channels):
            raise ValueError("encoding must be [batch, samples/pool_stride, latent_channels]")
        d.cond_in.view(eng.B, d.frames, d.Ep)[:, :, :self.latent_channels].copy_(e)

    def _sample(self, eng, seed=None):
        """``sample_from_discretized_mix_logistic`` on the decoder's logits (model.py:198; ops.py:178-201)."""
        d = eng.dec
        M = self.num_mixtures
        if self._gen is None:
            self._gen = torch.Generator(device="cuda")
            self._gen.manual_seed(self._seed)
        if seed is not None:
            self._gen.manual_seed(int(seed))
        u1 = torch.empty((d.N, M), dtype=torch.float32, device="cuda").uniform_(1e-5, 1.0 - 1e-5, generator=self._gen)
        u2 = torch.empty((d.N,), dtype=torch.float32, device="cuda").uniform_(1e-5, 1.0 - 1e-5, generator=self._gen)
        out = torch.empty((d.N,), dtype=torch.float32, device="cuda")
        from ._lib import call
        call("srwn_mol_sample", d.logits32.data_ptr(), d.logits32.stride(0), M, u1.data_ptr(), u2.data_ptr(),
             out.data_ptr(), d.N, torch.cuda.current_stream().cuda_stream)
        return out.view(eng.B, eng.T).cpu().numpy()

    def _learning_rate(self):
        return self._cfg.learning_rate

    def _control_engine(self, build=True):
        if self._eng is None and build:
            self._engine(1, self.input_size)
        return self._eng

    def _optimizers(self):
        """The decoder's and the encoder's: two buffers, two step counters, two shadows."""
        eng = self._control_engine()
        return {k: (e, e.params, e.adam_m, e.adam_v, e.adam_step, e.ctl) for k, e in (("decoder", eng.dec), ("encoder", eng.enc))}

    @property
    def network_params(self):
        eng = self._eng or self._engine(1, self.input_size)
        out = dict(eng.enc.tf_variables(self._name + "/Encoder"))
        out.update(eng.dec.tf_variables(self._name + "/Decoder", decoder=True))
        return out

    # --- the reference's methods (model.py:217-285) ---------------------------------------------------
    def save(self, logdir, global_step, force=False, fmt=None):
        if force or time.time() - self.last_checkpoint_time > 60:
            import json
            _write_state(logdir, global_step, self.network_params, fmt)
            with open(os.path.join(logdir, "config.json"), "w") as f:
                json.dump(dict(self._ctor, **{"class": "WaveNetAutoEncoder"}), f)
            self.last_checkpoint_time = time.time()
            return True
        return False

    def load(self, logdir):
        ok = _read_state(logdir, lambda: self.network_params)
        if ok:
            self._eng.enc.ctl.reset_ema(self._eng.enc.params); self._eng.dec._reset_ema()
            self._eng.enc.repack(); self._eng.dec.repack()
            print("Restoring previous session")
        return ok

    @classmethod
    def from_checkpoint(cls, logdir, batch, length, dtype=None):
        import json
        cfg = json.load(open(os.path.join(logdir, "config.json")))
        cfg.pop("class", None)
        m = cls(dtype=dtype, **cfg)
        m._engine(batch, length)
        if not m.load(logdir):
            raise FileNotFoundError("%s: no checkpoint to restore" % logdir)
        return m

    def train(self, inputs, conditions=None):
        self._refuse_in_ema("train")
        eng = self._stage(inputs, conditions)
        _train_step(eng)
        return np.float32(eng.loss.item())

    def fit(self, sampler, steps):
        """``steps`` training steps on batches a ``dataset.BatchSampler`` draws on the device; with condition_size > 0
        the labels' one-hot rows are the conditions.  Returns every step's loss, float32 [steps].  See ``_fit``."""
        self._refuse_in_ema("fit")
        if self.condition_size > 0:
            _fit_labels(sampler, self.condition_size, "WaveNetAutoEncoder", "conditions")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        d = eng.dec
        dest = dict(audio=eng.enc.x, audio2=d.audio)
        if self.condition_size > 0:
            dest.update(onehot=d.cond_in, onehot_rows=d.frames, onehot_col0=self.latent_channels)
        return _fit(eng, sampler, steps, dest)[0]

    def evaluate(self, sampler):
        """The forward-only loss of every step of one sweep over the sampler's dataset, float32 [len(dataset) /
        (batch_size * world)] in the steps' order; with condition_size > 0 the labels' one-hot rows are the conditions.
        The mixture-of-logistics loss kernel gives one number per batch, so `sampler` is a plain ``dataset.sampler(...,
        shuffle=False)`` whose batches divide the set.  Per-sample held-out likelihoods of any clip exist already: the
        streaming scorer (``scorer()``).  No parameter changes."""
        _loss_sweep_steps(sampler, "WaveNetAutoEncoder")
        if self.condition_size > 0:
            _fit_labels(sampler, self.condition_size, "WaveNetAutoEncoder", "conditions")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        d = eng.dec
        dest = dict(audio=eng.enc.x, audio2=d.audio)
        if self.condition_size > 0:
            dest.update(onehot=d.cond_in, onehot_rows=d.frames, onehot_col0=self.latent_channels)
        return _evaluate_losses(eng, sampler, dest, "WaveNetAutoEncoder")

    def encode(self, inputs, conditions=None):
        eng = self._stage(inputs, conditions)
        return eng.encode().view(eng.B, -1, self.latent_channels).cpu().numpy()

    def encoder(self, max_batch=1, max_frames=32):
        """An ``AudioEncoder`` with this model's hyper-parameters and a COPY of its current encoder parameters (a
        snapshot: call it again after more training).  It takes any batch <= max_batch and any length."""
        eng = self._eng or self._engine(1, self.input_size)
        enc = AudioEncoder(len(self.dilations), skip_channels=self.skip_channels, latent_channels=self.latent_channels,
                           pool_stride=self.pool_stride, encoder_channels=self.encoder_channels,
                           filter_width=self.filter_width, name=self._name, dtype=self._cfg.dtype, max_batch=max_batch,
                           max_frames=max_frames)
        enc._w.params.copy_(eng.enc.params)
        for k, t in eng.enc.dead.items():
            enc._w.dead[k].copy_(t)
        enc._w.repack()
        return enc

    def scorer(self, max_batch=1, max_chunk=1600, max_frames=32):
        """An ``AutoEncoderScorer`` on snapshots of this model's encoder (``encoder``) and decoder weights: audio in,
        nll[b, t] = -log p(audio[b, t] | audio[b, < t], encoding) in nats out, the number ``train`` descends on, for any
        batch <= max_batch and any length.  Call it again after more training."""
        from .recognizer import check_classifier_widths
        from .scorer import MolScorerWeights
        MolScorerWeights.check_config(self._cfg)
        check_classifier_widths(self.filter_width, self.dilation_channels, self.skip_channels, "streaming scorer")
        eng = self._eng or self._engine(1, self.input_size)
        return AutoEncoderScorer(self.encoder(max_batch, max_frames), MolScorerWeights.from_engine(eng.dec),
                                 self.condition_size, max_batch=max_batch, max_chunk=max_chunk, max_frames=max_frames)

    def reconstruct(self, inputs, conditions=None, seed=None):
        """``self.out`` (model.py:268-273): encode, run the decoder teacher-forced on the same clip, sample."""
        eng = self._stage(inputs, conditions)
        eng.forward()
        return self._sample(eng, seed)

    def reconstruct_with_encoding(self, inputs, encoding, conditions=None, seed=None):
        eng = self._stage(inputs, conditions)
        self._put_encoding(eng, encoding)
        eng.dec.forward(with_loss=False)
        return self._sample(eng, seed)

    def get_logits(self, inputs, encoding, conditions=None):
        eng = self._stage(inputs, conditions)
        self._put_encoding(eng, encoding)
        return eng.dec.forward(want_logits=True, with_loss=False).cpu().numpy()

    def generate(self, encoding, conditions=None, num_samples=None, mode="sample", seed=0, prompt=None, *,
                 temperature=1.0, top_k=0, top_p=1.0):
        """Queue-cached autoregressive sampling from the decoder given an encoding (the O(T L) replacement of the
        reference's sample-by-sample loop over ``reconstruct_with_encoding``, generator.py:150-170 /
        teacher.py:140-171): audio [B, num_samples] in [-1, 1].  prompt [B, P]: the num_samples (default: the rest of
        the encoding) that follow the prompt's P samples.  temperature (mode "sample"; a scalar or one entry per
        utterance): on the mixture choice and the logistic noise; top_k / top_p do not apply to a mixture head."""
        ctl = dict(temperature=temperature, top_k=top_k, top_p=top_p)
        self._check_sampling(np.shape(encoding)[0] if np.ndim(encoding) == 3 else 1, ctl, "generate")
        if prompt is not None:
            eng, st, p = self._prompted_state(encoding, conditions, seed, prompt, ctl)
            rest = st.limit - p.shape[1]
            T = int(num_samples) if num_samples is not None else rest
            if T > rest:
                raise ValueError("prompt %d + num_samples %d exceeds frames * pool_stride = %d" % (p.shape[1], T, st.limit))
            a, _, _ = eng.dec.generate_chunk(st, T, mode=mode)
            return a.cpu().numpy()
        e = torch.as_tensor(np.asarray(encoding, dtype=np.float32), device="cuda")
        if e.ndim != 3 or e.shape[2] != self.latent_channels:
            raise ValueError("encoding must be [batch, frames, latent_channels]")
        B, frames = int(e.shape[0]), int(e.shape[1])
        T = int(num_samples) if num_samples is not None else frames * self.pool_stride
        if T > frames * self.pool_stride:
            raise ValueError("num_samples %d exceeds frames * pool_stride = %d" % (T, frames * self.pool_stride))
        if self.condition_size > 0:
            if conditions is None:
                raise ValueError("this auto-encoder was built with condition_size > 0; pass conditions")
            c = torch.as_tensor(np.asarray(conditions, dtype=np.float32), device="cuda")
            e = _tile_conditions(e, c)
        eng = self._eng or self._engine(B, frames * self.pool_stride)
        a, _, _ = eng.dec.generate(T, mode=mode, seed=seed, batch=B, cond=e.contiguous(), **ctl)
        return a.cpu().numpy()

    def stream(self, encoding, conditions=None, chunk_size=160, mode="sample", seed=0, prompt=None, max_samples=None, *,
               temperature=1.0, top_k=0, top_p=1.0):
        """Real-time decoding: an iterator of NumPy [B, chunk_size] blocks that ends where the encoding's frames run out
        (or at max_samples); put together they are generate(encoding, ..., seed=seed) bit for bit.  prompt [B, P]: the
        samples after it.  temperature: as `generate`, for the whole stream."""
        if int(chunk_size) < 1:
            raise ValueError("chunk_size must be >= 1")
        ctl = dict(temperature=temperature, top_k=top_k, top_p=top_p)
        self._check_sampling(np.shape(encoding)[0] if np.ndim(encoding) == 3 else 1, ctl, "stream")
        eng, st, _ = self._prompted_state(encoding, conditions, seed, prompt, ctl)
        return _stream_chunks(eng.dec, st, int(chunk_size), mode, max_samples)

    def generation_pool(self, capacity, frames, mode="sample", *, live=False):
        """A pool of `capacity` decoder slots that streams join and leave while it runs (GenerationPool): `frames` = the
        most encoding frames a stream brings; each join takes one encoding [frames_i, latent_channels] (and conditions
        [condition_size]) per stream, which ends at frames_i * pool_stride.
        live=True: `frames` is the length of every slot's conditioning ring, and streams that ``join(..., live=True)`` are
        fed while they run (``feed`` / ``room`` / ``close``), with no bound on their length; bounded streams still join."""
        if int(capacity) < 1:
            raise ValueError("generation_pool: capacity %d" % int(capacity))
        if frames is None or int(frames) < 1:
            raise ValueError("generation_pool: frames %r (the most encoding frames of a stream)" % (frames,))
        if live:
            K._need_gpu()
        eng = self._eng or self._engine(1, int(frames) * self.pool_stride)
        pool = eng.dec.generation_pool(int(capacity), int(frames), live=True) if live else \
            eng.dec.generation_pool(int(capacity), int(frames))
        return GenerationPool(pool, self._pool_cond, mode, self.latent_channels, self.condition_size)

    def _pool_cond(self, n, encoding, conditions):
        return _pool_encodings(n, encoding, conditions, self.latent_channels, self.condition_size)

    def _check_sampling(self, n, ctl, who):
        """The sampling controls' ranges, before any device work (engine.sampling_table): a mixture head."""
        from .engine import sampling_table
        sampling_table(int(n), ctl["temperature"], ctl["top_k"], ctl["top_p"], 64, True, who)      # (top_k is refused: C unused)

    def _prompted_state(self, encoding, conditions, seed, prompt, ctl=None):
        enc = np.asarray(encoding, dtype=np.float32)
        if enc.ndim != 3 or enc.shape[2] != self.latent_channels:
            raise ValueError("encoding must be [batch, frames, latent_channels]")
        B, frames = int(enc.shape[0]), int(enc.shape[1])
        p = _check_prompt(B, prompt)
        if p is not None and p.shape[1] > frames * self.pool_stride:
            raise ValueError("prompt of %d samples exceeds frames * pool_stride = %d" % (p.shape[1], frames * self.pool_stride))
        e = torch.as_tensor(enc, device="cuda")
        if self.condition_size > 0:
            if conditions is None:
                raise ValueError("this auto-encoder was built with condition_size > 0; pass conditions")
            c = torch.as_tensor(np.asarray(conditions, dtype=np.float32), device="cuda")
            e = _tile_conditions(e, c)
        eng = self._eng or self._engine(B, frames * self.pool_stride)
        st = eng.dec.generation_state(B, e.contiguous(), seed, **(ctl or {}))
        if p is not None:
            eng.dec.prime(st, p)
        return eng, st, p

    def live(self, batch, conditions=None, max_frames=32, mode="sample", seed=0, prompt_frames=None, prompt=None, *,
             temperature=1.0):
        """Live decoding: a ``LiveDecoding`` of `batch` streams in lockstep whose encoding is FED while the decoder runs
        (``feed`` / ``step``), on a conditioning ring of `max_frames` frames -- a stream has no bound on its length.  The
        samples put together are ``generate(encoding, conditions, seed=seed, ...)`` of the whole encoding bit for bit.
        conditions [B, condition_size] are tiled onto every frame fed.  prompt [B, P] with prompt_frames [B, k, latent]
        (P <= k * pool_stride, k <= max_frames): the frames are fed and the run starts after the prompt."""
        batch, max_frames = int(batch), int(max_frames)
        if batch < 1 or max_frames < 1:
            raise ValueError("live: batch %d, max_frames %d" % (batch, max_frames))
        self._check_sampling(batch, dict(temperature=temperature, top_k=0, top_p=1.0), "live")
        p = _check_prompt(batch, prompt)
        pf = None
        if p is not None or prompt_frames is not None:
            if p is None or prompt_frames is None:
                raise ValueError("live: prompt [B, P] and prompt_frames [B, k, latent] come together")
            pf = prompt_frames if isinstance(prompt_frames, torch.Tensor) else np.asarray(prompt_frames, dtype=np.float32)
            if pf.ndim != 3 or pf.shape[0] != batch or pf.shape[2] != self.latent_channels or pf.shape[1] > max_frames:
                raise ValueError("prompt_frames must be [%d, k <= max_frames = %d, latent_channels=%d], got %s"
                                 % (batch, max_frames, self.latent_channels, tuple(pf.shape)))
            if p.shape[1] > pf.shape[1] * self.pool_stride:
                raise ValueError("prompt of %d samples exceeds frames * pool_stride = %d"
                                 % (p.shape[1], pf.shape[1] * self.pool_stride))
        c = _check_conditions(batch, conditions, self.condition_size, "auto-encoder")
        K._need_gpu()
        eng = self._eng or self._engine(batch, max_frames * self.pool_stride)
        cond = _to_device(c)
        st = eng.dec.live_generation_state(batch, max_frames, seed, temperature=temperature)
        live = LiveDecoding(self, eng.dec, st, cond, mode)
        if pf is not None:
            live.feed(pf)
            eng.dec.prime(st, p)
        return live

    def resynthesizer(self, max_batch=1, max_frames=32):
        """A ``TeacherResynthesizer``: ``self.encoder(max_batch, max_frames)`` (a snapshot of the encoder's parameters)
        feeding this model's decoder on conditioning rings of `max_frames` frames."""
        return TeacherResynthesizer(self.encoder(max_batch, max_frames), self, max_frames=max_frames)

    def mu_law(self, inputs, conditions=None):
        raise AttributeError("WaveNetAutoEncoder.mu_law reads self.targets, which the reference never defines "
                             "(model.py:100,276): it raises there too")


class _LiveStream(object):
    """What ``LiveDecoding`` and ``LiveSynthesis`` share: a running batch of ``batch_size`` streams of ``_owner`` on the
    engine state ``_st``, fed through a conditioning ring of ``_ring`` frames, with the conditions ``_cond`` (device, or
    None) tiled onto every frame fed.  A subclass gives ``room``, ``_take`` (the engine call the frames go to) and
    ``step`` / ``_step_device``."""

    def __init__(self, owner, state, cond, batch, ring):
        self._owner, self._st, self._cond, self.batch_size, self._ring = owner, state, cond, batch, ring

    t = property(lambda self: self._st.t)
    fed = property(lambda self: self._st.fed)

    @property
    def available(self):
        """Samples that can be made now: fed * pool_stride - t."""
        return self._st.limit - self._st.t

    def _feed_device(self, enc):
        """enc [B, k, latent] on the device (or NumPy): + the tiled conditions, into the ring."""
        o = self._owner
        e = torch.as_tensor(enc, dtype=torch.float32)
        if e.dim() != 3 or e.shape[0] != self.batch_size or e.shape[2] != o.latent_channels:
            raise ValueError("encoding must be [%d, k, latent_channels=%d], got %s"
                             % (self.batch_size, o.latent_channels, tuple(e.shape)))
        if e.shape[1] > self.room:
            raise ValueError("feed: %d frames, but the ring of %d has room for %d at t = %d with %d fed"
                             % (e.shape[1], self._ring, self.room, self.t, self.fed))
        if self._cond is not None:
            e = _tile_conditions(e.to("cuda"), self._cond)
        self._take(e)

    def feed(self, encoding):
        self._feed_device(encoding if isinstance(encoding, torch.Tensor) else np.asarray(encoding, dtype=np.float32))


class LiveDecoding(_LiveStream):
    """One running batch of live decoder streams (``WaveNetAutoEncoder.live``).  ``feed(encoding [B, k, latent])`` hands
    every stream its next k frames (k <= ``room``), ``step(n)`` returns the next n <= ``available`` samples [B, n]; ``t``:
    samples made so far (a prompt's included), ``fed``: frames fed.  The samples are those ``generate`` gives the whole
    encoding with the same seed and temperature, however the frames and chunks were cut."""

    def __init__(self, owner, dec, state, cond, mode):
        super().__init__(owner, state, cond, state.batch, state.max_frames)
        self._dec, self._mode = dec, mode

    @property
    def room(self):
        from .engine import live_decode_room
        return live_decode_room(self._st.max_frames, self._st.fed, self._st.t, self._owner.pool_stride)

    def _take(self, e):
        self._dec.feed(self._st, e)

    def _step_device(self, n, forced=None, want_logits=False):
        """(audio [B, n] f32, selected mixture [B, n] i32, logits [B, n, 4M] f32 or None) on the device."""
        return self._dec.generate_chunk(self._st, int(n), mode=self._mode, forced=forced, want_logits=want_logits)

    def step(self, n, forced=None, return_logits=False):
        """The next n samples [B, n] (NumPy); forced [B, n]: teacher forcing for this chunk; return_logits: (samples, logits
        [B, n, 4 * num_mixtures])."""
        a, _, lg = self._step_device(n, forced, return_logits)
        return (a.cpu().numpy(), lg.cpu().numpy()) if return_logits else a.cpu().numpy()


def _check_resynthesis_halves(who, encoder, other, other_type, arg, half):
    """What both resynthesizers ask of their halves -- an ``AudioEncoder`` and `other` (the argument `arg`, of
    `other_type`, whose `half` reads the frames) with one pool_stride and one latent width.  Returns ``lookahead``: the
    samples of audio a sample of output waits for beyond itself, the rest of its frame and the encoder's look-ahead."""
    if not isinstance(encoder, AudioEncoder) or not isinstance(other, other_type):
        raise TypeError("%s(encoder: AudioEncoder, %s: %s)" % (who, arg, other_type.__name__))
    if int(encoder.pool_stride) != int(other.pool_stride):
        raise ValueError("pool_stride: the encoder makes a frame per %d samples, the %s reads one per %d"
                         % (encoder.pool_stride, half, other.pool_stride))
    if int(encoder.latent_channels) != int(other.latent_channels):
        raise ValueError("latent_channels: the encoder gives %d, the %s takes %d"
                         % (encoder.latent_channels, half, other.latent_channels))
    return int(encoder.pool_stride) + encoder.num_layers + 1


class _ResynthesisStream(object):
    """One running batch of a resynthesizer's ``stream``: an encoder stream state ``_enc`` whose frames go, on the device,
    into the live half ``_live`` (a ``_LiveStream``).  ``t``: samples returned so far per stream; ``received``: samples
    pushed.  ``push`` may return no sample while the first frame's look-ahead is incomplete.  A subclass gives
    ``_start_live``, ``_audio`` (the audio of what its live half's ``_step_device`` returns) and ``_tail``, the axes its
    results have after [B, m]."""

    _tail = ()

    def __init__(self, owner, batch, conditions, seed, temperature, chunk_size):
        self._owner, self.batch_size, self._chunk = owner, batch, chunk_size
        self._live = self._start_live(batch, conditions, seed, temperature)      # (its refusals come before any device work)
        self._enc = owner.encoder._eng.start(batch)

    t = property(lambda self: self._live.t)
    received = property(lambda self: self._enc.received)

    def _audio(self, chunk):
        return chunk

    def _drain(self, frames, outs):
        """frames [B, k, latent] (device) into the ring and every sample they allow: feed -> step -> feed while the ring
        has less room than the frames that are due."""
        live, k, f0 = self._live, int(frames.shape[1]), 0
        while True:
            if f0 < k:
                r = min(live.room, k - f0)
                if r > 0:
                    live._feed_device(frames[:, f0:f0 + r])
                    f0 += r
            n = min(live.available, self._chunk)
            if n <= 0:
                if f0 < k:      # (cannot happen on a ring that starts a live stream: room > 0 once every sample is made)
                    raise RuntimeError("the conditioning ring has no room and no sample to make")
                return
            outs.append(self._audio(live._step_device(n)))

    def _result(self, outs):
        B = self.batch_size
        if not outs:
            return np.zeros((B, 0) + self._tail, np.float32)
        return torch.cat(outs, dim=1).view(B, -1, *self._tail).cpu().numpy()

    def push(self, audio):
        if self._enc.closed:
            raise ValueError("this stream is closed (finish was called)")
        x = self._owner.encoder._check(audio, self.batch_size)
        outs = []
        self._drain(self._owner.encoder._eng.push(self._enc, torch.as_tensor(x)), outs)
        return self._result(outs)

    def finish(self):
        """The encoder's remaining whole frames (clip-end padding) and the samples they allow; closes the stream."""
        outs = []
        self._drain(self._owner.encoder._eng.finish(self._enc), outs)
        return self._result(outs)


class TeacherResynthesizer(object):
    """The live auto-encoder loop at teacher quality: an ``AudioEncoder`` feeding the autoregressive decoder of a
    ``WaveNetAutoEncoder`` (``Resynthesizer`` is the same pipeline on the student).  Audio chunks in, decoded audio chunks
    out, with no bound on the length; the latent frames go from the encoder into the decoder's conditioning ring as device
    tensors.  The audio of a stream put together equals ``autoencoder.generate(encoder.encode(audio), conditions,
    seed=seed, ...)`` however the audio and the chunks were cut."""

    def __init__(self, encoder, autoencoder, max_frames=None):
        self.lookahead = _check_resynthesis_halves("TeacherResynthesizer", encoder, autoencoder, WaveNetAutoEncoder,
                                                   "autoencoder", "decoder")
        K._need_gpu()
        self.encoder, self.autoencoder = encoder, autoencoder
        self.pool_stride = int(encoder.pool_stride)
        self.max_frames = int(max_frames if max_frames is not None else encoder.max_frames)

    def stream(self, batch=1, conditions=None, seed=0, temperature=1.0, chunk_size=160):
        """A ``TeacherResynthesisStream`` of `batch` streams in lockstep: ``push(audio [B, m])`` returns every sample that
        can be made by now, [B, m']; ``finish()`` the rest.  conditions [B, condition_size] are tiled onto every frame on
        the device; chunk_size: the most samples of one decoder launch."""
        batch, chunk_size = int(batch), int(chunk_size)
        if not 1 <= batch <= self.encoder.max_batch:
            raise ValueError("batch %d: the encoder holds %d streams" % (batch, self.encoder.max_batch))
        if chunk_size < 1:
            raise ValueError("chunk_size %d: at least 1" % chunk_size)
        return TeacherResynthesisStream(self, batch, conditions, seed, temperature, chunk_size)

    def pool(self, chunk_size=160, audio_ring=None):
        """A ``TeacherResynthesisPool``: independent callers on one encoder and one decoder.  Streams join and leave while
        the batch runs, audio arrives ragged, and each caller receives what it would have received alone.  chunk_size: the
        samples a ``step`` makes per stream at most; audio_ring: samples of audio a slot can hold (``AudioEncoder.pool``)."""
        K._need_gpu()
        return TeacherResynthesisPool(self, int(chunk_size), audio_ring)


class TeacherResynthesisStream(_ResynthesisStream):
    """One running batch of ``TeacherResynthesizer.stream``: ``push`` / ``finish`` return samples [B, m]."""

    def _start_live(self, batch, conditions, seed, temperature):
        o = self._owner
        return o.autoencoder.live(batch, conditions, o.max_frames, seed=seed, temperature=temperature)

    def _audio(self, chunk):
        return chunk[0]      # of (audio, selected mixture, logits)


class AudioEncoder(object):
    """The deployable form of the auto-encoder's encoder (createEncoder, model.py:136-156): audio in, latent frames out
    (``encoder.FrameEncoder``), with no decoder and no training state anywhere.  One object serves any batch <=
    ``max_batch`` and any length, whole clips (``encode``) or chunk by chunk (``stream``); a frame's value does not
    depend on how the audio was cut.  ``load`` reads what ``WaveNetAutoEncoder.save`` wrote, by the reference's
    variable names; the decoder's variables in the file are ignored."""

    def __init__(self, num_layers, skip_channels=256, latent_channels=16, pool_stride=512, encoder_channels=128,
                 filter_width=2, name="WaveNetAutoEncoder", dtype=None, max_batch=1, max_frames=32):
        from .encoder import EncoderWeights, FrameEncoder, _check_encoder_widths
        _check_encoder_widths(encoder_channels, filter_width, skip_channels)
        K._need_gpu()
        self.num_layers, self.skip_channels, self.latent_channels = int(num_layers), skip_channels, latent_channels
        self.pool_stride, self.encoder_channels, self.filter_width = int(pool_stride), encoder_channels, filter_width
        self._name = name
        self.max_batch, self.max_frames = int(max_batch), int(max_frames)
        self._w = EncoderWeights(self.num_layers, encoder_channels, skip_channels, latent_channels, filter_width,
                                 dtype or _default_dtype())
        self._eng = FrameEncoder(self._w, self.pool_stride, max_batch=max_batch, max_frames=max_frames)

    @property
    def network_params(self):
        return self._w.tf_variables(self._name + "/Encoder")

    def load(self, logdir):
        ok = _read_state(logdir, lambda: self.network_params)
        if ok:
            self._w.repack()
        return ok

    @classmethod
    def from_checkpoint(cls, logdir, **kwargs):
        """An encoder on the variables saved in `logdir`, with the hyper-parameters of the ``config.json`` that
        ``WaveNetAutoEncoder.save`` writes beside them; kwargs: dtype, max_batch, max_frames."""
        import json
        with open(os.path.join(logdir, "config.json")) as f:
            cfg = json.load(f)
        enc = cls(len(cfg["dilations"]), skip_channels=cfg["skip_channels"], latent_channels=cfg["latent_channels"],
                  pool_stride=cfg["pool_stride"], encoder_channels=cfg["encoder_channels"],
                  filter_width=cfg["filter_width"], name=cfg.get("name", "WaveNetAutoEncoder"), **kwargs)
        if not enc.load(logdir):
            raise FileNotFoundError("%s: no checkpoint to restore (WaveNetAutoEncoder.save writes one)" % logdir)
        return enc

    def _check(self, inputs, batch=None):
        """Shape refusals, before anything touches the device."""
        x = np.asarray(inputs, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("inputs must be [batch, samples], got shape %s" % (x.shape,))
        if not 1 <= x.shape[0] <= self.max_batch:
            raise ValueError("batch %d: this encoder was built for max_batch=%d" % (x.shape[0], self.max_batch))
        if batch is not None and x.shape[0] != batch:
            raise ValueError("audio of %d streams pushed into a stream of %d" % (x.shape[0], batch))
        return x

    def encode(self, inputs):
        """inputs [B, T] -> encoding [B, T // pool_stride, latent_channels] (NumPy), for any T."""
        x = self._check(inputs)
        return self._eng.encode(torch.as_tensor(x)).cpu().numpy()

    def stream(self, batch_size=1):
        """An ``EncoderStream`` of `batch_size` streams in lockstep: ``push(audio [B, n])`` returns the frames whose
        look-ahead is complete, ``finish()`` the rest with the clip-end padding."""
        if not 1 <= int(batch_size) <= self.max_batch:
            raise ValueError("batch_size %r: this encoder was built for max_batch=%d" % (batch_size, self.max_batch))
        return EncoderStream(self, int(batch_size))

    def pool(self, audio_ring=None, max_rows=None):
        """An ``AudioEncoderPool``: this encoder's ``max_batch`` rows as slots that streams join and leave, each pushing
        audio of any length at a clock of its own (``encoder.EncoderPool``).  audio_ring: samples a slot can hold
        (default max_frames * pool_stride + num_layers + 1 + pool_stride); max_rows: frames per launch."""
        K._need_gpu()
        return AudioEncoderPool(self._eng.pool(audio_ring, max_rows))


class EncoderStream(object):
    """NumPy face of one running batch of encoder streams (``AudioEncoder.stream``).  ``t``: samples received per
    stream; ``frames``: frames emitted.  Everything ``push`` returned followed by what ``finish`` returns equals
    ``AudioEncoder.encode`` of the concatenated audio."""

    def __init__(self, owner, batch_size):
        self._owner, self.batch_size = owner, batch_size
        self._st = owner._eng.start(batch_size)

    @property
    def t(self):
        return self._st.received

    @property
    def frames(self):
        return self._st.emitted

    def push(self, audio):
        if self._st.closed:
            raise ValueError("this stream is closed (finish was called)")
        x = self._owner._check(audio, self.batch_size)
        return self._owner._eng.push(self._st, torch.as_tensor(x)).cpu().numpy()

    def finish(self):
        return self._owner._eng.finish(self._st).cpu().numpy()


class _AudioPoolFace(_PoolFace):
    """What the NumPy faces of the pools that take audio share (``self._pool``: an ``audio_ring.AudioRingSlots``)."""

    def __init__(self, pool):
        self._pool = pool

    received = property(lambda self: self._pool.received)
    emitted = property(lambda self: self._pool.emitted)

    def audio_room(self, slot):
        return self._pool.audio_room(int(slot))

    def join(self, n=1, slots=None):
        return self._pool.join(n, slots)

    def push(self, slots, audio):
        self._pool.push([int(slots)] if np.isscalar(slots) else slots, _audio_pieces(slots, audio))


class AudioEncoderPool(_AudioPoolFace):
    """NumPy face of an encoder pool (``AudioEncoder.pool``; encoder.EncoderPool).  ``join`` returns slots,
    ``push(slots, audio)`` takes one 1-D array per slot, of any length, ``finish(slots)`` ends streams, ``step()`` returns
    ``{slot: frames [k, latent]}`` for every slot with new frames and frees the finished slots whose frames are all out.
    A stream's frames put together are ``AudioEncoder.encode`` of its audio alone."""

    def finish(self, slots):
        self._pool.finish(slots)

    def step(self, limit=None):
        return {u: f.cpu().numpy() for u, f in self._pool.step(limit).items()}


class ClassifierPool(_AudioPoolFace):
    """NumPy face of a classifier pool (``StreamingClassifier.pool``; recognizer.ClassifierPool).  ``join`` returns slots,
    ``push(slots, audio)`` takes one 1-D array per slot, of any length, ``step()`` returns ``{slot: probabilities [e, C]}``
    for every slot whose stream completed window positions (with return_logits a second dict with the pooled logits).  A
    stream's emissions put together are ``StreamingClassifier.classify`` of its audio alone."""

    audio_ring = property(lambda self: self._pool.audio_ring)
    consumed = property(lambda self: self._pool.consumed)

    def step(self, return_logits=False):
        out = self._pool.step(return_logits)
        host = lambda d: {u: f.cpu().numpy() for u, f in d.items()}
        return (host(out[0]), host(out[1])) if return_logits else host(out)


class ScorerStreamPool(_AudioPoolFace):
    """NumPy face of a scorer pool (``StreamingScorer.pool``; scorer.ScorerPool).  ``join`` returns slots, ``push(slots,
    audio)`` takes one 1-D array per slot, of any length, ``step()`` returns ``{slot: nll [m]}`` (nats) for every slot whose
    stream scored m > 0 samples (with return_logits / return_best further dicts, in that order).  A stream's nll put
    together is ``StreamingScorer.score`` of its audio alone."""

    audio_ring = property(lambda self: self._pool.audio_ring)
    scored = property(lambda self: self._pool.scored)
    nll_sum = property(lambda self: self._pool.nll_sum)

    def bits_per_sample(self, slot):
        """The running mean nll of the stream in `slot`, in bits (NaN before its first sample)."""
        return self._pool.bits_per_sample(int(slot))

    def step(self, return_logits=False, return_best=False):
        out = self._pool.step(return_logits, return_best)
        host = lambda d: {u: f.cpu().numpy() for u, f in d.items()}
        return tuple(host(d) for d in out) if isinstance(out, tuple) else host(out)


class MolScorerStreamPool(_AudioPoolFace):
    """NumPy face of a mixture-of-logistics scorer pool (``StreamingMolScorer.pool``; scorer.MolScorerPool).
    ``join(conditions, n)`` returns slots (conditions [n, condition_size], one row per stream, tiled onto every frame the
    stream is fed), ``push(slots, audio)`` takes one 1-D array per slot, of any length, ``feed(slots, encoding)`` one
    [k, latent_channels] array per slot with k <= ``room(slot)``, ``step()`` returns ``{slot: nll [m]}`` (nats) for every slot
    whose stream scored m > 0 samples (with return_logits a second dict).  A stream's nll put together is
    ``StreamingMolScorer.score`` of its audio and encoding alone."""

    def __init__(self, owner, pool):
        super().__init__(pool)
        self._owner, self._cond = owner, {}      # slot -> its stream's conditions [1, condition_size] on the device, or None

    audio_ring = property(lambda self: self._pool.audio_ring)
    scored = property(lambda self: self._pool.scored)
    fed = property(lambda self: self._pool.fed)
    nll_sum = property(lambda self: self._pool.nll_sum)

    def join(self, conditions=None, n=1, slots=None):
        n = int(n) if slots is None else len(slot_list(slots, self.capacity, "join"))
        c = self._owner._conditions(n, conditions)           # (its refusals come before any device work)
        slots = self._pool.join(n, slots)
        for i, u in enumerate(slots):
            self._cond[u] = None if c is None else c[i:i + 1]
        return slots

    def leave(self, slots):
        self._pool.leave(slots)
        for u in slot_list(slots, self.capacity, "leave"):
            self._cond.pop(u, None)

    def room(self, slot):
        return self._pool.room(int(slot))

    def available(self, slot):
        return self._pool.available(int(slot))

    def bits_per_sample(self, slot):
        """The running mean nll of the stream in `slot`, in bits (NaN before its first sample)."""
        return self._pool.bits_per_sample(int(slot))

    def feed(self, slots, encoding):
        """encoding: one [k, latent_channels] array per slot (one slot: the array itself)."""
        if not self._owner.conditioned:
            raise ValueError("feed: this teacher is not conditioned")
        one = np.isscalar(slots) or (isinstance(encoding, (np.ndarray, torch.Tensor)) and encoding.ndim == 2)
        us = slot_list(slots, self.capacity, "feed")
        pieces = [encoding] if one else list(encoding)
        if len(pieces) != len(us):
            raise ValueError("feed: %d slots but %d pieces of encoding" % (len(us), len(pieces)))
        if any(u not in self._cond for u in us):
            raise ValueError("feed: slots %s do not all hold a stream of this pool" % (us,))
        self._pool.feed(us, [self._owner._frames(torch.as_tensor(e, dtype=torch.float32)[None], self._cond[u])[0]
                             for u, e in zip(us, pieces)])

    def step(self, return_logits=False):
        out = self._pool.step(return_logits)
        return tuple(_host_dict(d) for d in out) if isinstance(out, tuple) else _host_dict(out)


class ParallelWaveNet(_TrainingControls):
    """model.py:290-656 on ``student.StudentEngine``: ``num_flows`` inverse-autoregressive flows distilled against a
    frozen mixture-of-logistics teacher.

    ``teacher`` is a ``WaveNetAutoEncoder`` (or a decoder-only ``WaveNetTeacher(head="mol", use_encoding=True)``), or
    the directory one was saved to (the reference takes the checkpoint directory and imports its meta graph,
    model.py:313-324).  The ``sess`` argument of
    every method is accepted for call compatibility with student.py and ignored (there is no session).
    ``encode`` / ``reconstruct`` run the teacher auto-encoder (model.py:644-656); ``train`` is the per-row-clipped
    slow path (model.py:599-632), ``train_fast`` the one student.py:107 uses."""

    def __init__(self, input_size, condition_size, dilations, teacher, num_flows=2, filter_width=2,
                 dilation_channels=32, skip_channels=256, latent_channels=16, pool_stride=512,
                 name="ParallelWaveNet", alpha=1.0, beta=1.0, gamma=1.0, learning_rate=0.001, dtype=None, seed=0):
        K._need_gpu()
        self.input_size = input_size
        self.condition_size = condition_size
        self.dilations = dilations
        self.teacher = teacher
        self.num_flows = num_flows
        self.filter_width = filter_width
        self.dilation_channels = dilation_channels
        self.skip_channels = skip_channels
        self.latent_channels = latent_channels
        self.pool_stride = pool_stride
        self._name = name
        self._abg = (float(alpha), float(beta), float(gamma))
        self._lr, self._seed = learning_rate, seed
        self._teacher_dir = None
        self._dtype = dtype
        if isinstance(teacher, (str, os.PathLike)):
            self._teacher_dir = os.fspath(teacher)
            import json
            cfgp = os.path.join(self._teacher_dir, "config.json")
            if not os.path.exists(cfgp):
                raise FileNotFoundError("%s: no config.json (save the teacher with its save() method)" % self._teacher_dir)
            if json.load(open(cfgp)).get("class") == "WaveNetAutoEncoder":
                self._teacher = None      # built on first use: the auto-encoder is tied to one (batch, length)
                self._teacher_cfg = {k: v for k, v in json.load(open(cfgp)).items() if k != "class"}
            else:
                self._teacher = WaveNetTeacher.from_checkpoint(self._teacher_dir, dtype=dtype)
        else:
            self._teacher = teacher
        t = self._teacher
        if isinstance(t, WaveNetTeacher) and t.gate_mode != "reference":
            raise ValueError("ParallelWaveNet: the teacher was built with gate_mode=%r; distillation runs the reference "
                             "gate only (the teacher's generation and the flows implement it)" % t.gate_mode)
        if t is None:
            tc = self._teacher_cfg
            tl, tcs, tp, tdt = tc["latent_channels"], tc["condition_size"], tc["pool_stride"], None
        elif isinstance(t, WaveNetAutoEncoder):
            tl, tcs, tp, tdt = t.latent_channels, t.condition_size, t.pool_stride, t._cfg.dtype
        elif isinstance(t, WaveNetTeacher) and t.head == "mol" and t.use_encoding:
            tl, tcs, tp, tdt = t.latent_channels, t.condition_size, t.pool_stride, t._cfg.dtype
        else:
            raise ValueError("teacher must be a WaveNetAutoEncoder, or a mixture-of-logistics WaveNetTeacher built "
                             "with use_encoding=True, or a directory one of them was saved to")
        if (tl, tcs, tp) != (latent_channels, condition_size, pool_stride):
            raise ValueError("student and teacher must agree on latent_channels, condition_size and pool_stride "
                             "(they share the encoding placeholders, model.py:318-324)")
        self._flow_cfg = StackConfig(dilations=list(dilations), filter_width=filter_width,
                                     dilation_channels=dilation_channels, skip_channels=skip_channels,
                                     cond_channels=latent_channels + condition_size, pool_stride=pool_stride,
                                     dtype=dtype or tdt or _default_dtype(), learning_rate=learning_rate)
        self._engines: Dict[tuple, object] = {}
        self._primary = None
        self.last_checkpoint_time = time.time()

    # ------------------------------------------------------------------------------------------------
    def _engine(self, B: int, T: int):
        from .student import StudentEngine
        key = (int(B), int(T))
        eng = self._engines.get(key)
        if eng is None:
            if self._primary is not None:
                raise NotImplementedError("ParallelWaveNet: one (batch, length) per model object for now; got %s "
                                          "after %s" % (key, next(iter(self._engines))))
            a, b, g = self._abg
            if self._teacher is None:
                self._teacher = WaveNetAutoEncoder.from_checkpoint(self._teacher_dir, B, T, dtype=self._dtype)
            teng = self._teacher._engine(B, T)
            eng = StudentEngine(teng.dec if isinstance(self._teacher, WaveNetAutoEncoder) else teng, self._flow_cfg,
                                self.num_flows, alpha=a, beta=b, gamma=g, learning_rate=self._lr, seed=self._seed)
            self._primary = eng
            self._engines[key] = eng
            self._apply_controls(eng)
        return eng

    def _learning_rate(self):
        return self._lr

    def _control_engine(self, build=True):
        if self._primary is None and build:
            self._engine(1, self.input_size)
        return self._primary

    def _optimizers(self):
        st = self._control_engine().storage
        return {"flows": (self._primary, st.params, st.adam_m, st.adam_v, st.adam_step, self._primary.ctl)}

    def _stage(self, inputs, truth, encoding, conditions):
        z = torch.as_tensor(np.asarray(inputs, dtype=np.float32), device="cuda")
        B, T = z.shape
        eng = self._engine(B, T)
        e = torch.as_tensor(np.asarray(encoding, dtype=np.float32), device="cuda")
        if self.condition_size > 0:
            if conditions is None:
                raise ValueError("this student was built with condition_size > 0; pass conditions [B, condition_size]")
            c = torch.as_tensor(np.asarray(conditions, dtype=np.float32), device="cuda")
            e = _tile_conditions(e, c)
        if tuple(e.shape) != (B, T // self.pool_stride, self.latent_channels + self.condition_size):
            raise ValueError("encoding must be [batch, samples/pool_stride, latent_channels]")
        tr = None if truth is None else torch.as_tensor(np.asarray(truth, dtype=np.float32), device="cuda")
        eng.set_inputs(z, tr, e.contiguous())
        return eng

    @property
    def network_params(self):
        if self._primary is None:
            self._engine(1, self.input_size)
        out = {}
        for i, f in enumerate(self._primary.flows):
            out.update(f.tf_variables("%s/Flow%d/Flow%d" % (self._name, i, i)))           # model.py:417,468,510
        return out

    def synthesizer(self, max_batch=1, max_chunk=1600, max_frames=None):
        """A ``StudentSynthesizer`` with this model's hyper-parameters and a COPY of its current flow parameters (a
        snapshot: call it again after more training).  max_frames defaults to input_size // pool_stride."""
        if self._primary is None:
            self._engine(1, self.input_size)
        syn = StudentSynthesizer(self.dilations, self.num_flows, filter_width=self.filter_width,
                                 dilation_channels=self.dilation_channels, latent_channels=self.latent_channels,
                                 condition_size=self.condition_size, pool_stride=self.pool_stride, name=self._name,
                                 dtype=self._flow_cfg.dtype, max_batch=max_batch, max_chunk=max_chunk,
                                 max_frames=max_frames or max(1, self.input_size // self.pool_stride))
        for w, f in zip(syn._eng.weights, self._primary.flows):
            w.params.copy_(f.params)
        syn._eng.repack()
        return syn

    def inverter(self, max_batch=1):
        """A ``StudentInverter`` with this model's hyper-parameters and a COPY of its current flow parameters (a
        snapshot, as ``synthesizer``): audio -> noise and the student's exact log-likelihood of held-out audio."""
        inv = StudentInverter(self.dilations, self.num_flows, filter_width=self.filter_width,
                              dilation_channels=self.dilation_channels, latent_channels=self.latent_channels,
                              condition_size=self.condition_size, pool_stride=self.pool_stride, name=self._name,
                              dtype=self._flow_cfg.dtype, max_batch=max_batch)
        if self._primary is None:
            self._engine(1, self.input_size)
        for w, f in zip(inv._eng.weights, self._primary.flows):
            w.params.copy_(f.params)
            w.repack()
        inv._eng.repack()
        return inv

    # --- checkpointing (model.py:540-567) ---------------------------------------------------------------
    def load(self, sess, logdir):
        if self._teacher_dir is not None and self._teacher is not None:
            self._teacher.load(self._teacher_dir)                                         # model.py:543-544
        ok = _read_state(logdir, lambda: self.network_params)
        if ok:
            self._primary.ctl.reset_ema(self._primary.storage.params)
            for f in self._primary.flows:
                f.repack()
            print("Restoring previous session")
        return ok

    def save(self, sess, logdir, global_step, force=False, fmt=None):
        if force or time.time() - self.last_checkpoint_time > 60:
            _write_state(logdir, global_step, self.network_params, fmt)
            self.last_checkpoint_time = time.time()
            return True
        return False

    # --- graph outputs (model.py:570-597) ---------------------------------------------------------------
    def generate(self, sess, inputs, encoding, conditions=None):
        """noise [B,T] -> audio [B,T,1] in [-1,1] in ONE parallel pass (``self.out``, model.py:535)."""
        eng = self._stage(inputs, None, encoding, conditions)
        eng.forward_flows()
        return eng.out.view(eng.B, eng.T, 1).cpu().numpy()

    def getEntropy_fast(self, sess, inputs, encoding, conditions=None):
        """sum(log s_tot + 2) over the batch (model.py:356)."""
        eng = self._stage(inputs, None, encoding, conditions)
        eng.forward_flows()
        return np.float32(float(eng.logs.item()) + 2.0 * eng.N)

    def getEntropy(self, sess, inputs, encoding, conditions=None):
        """Per-sample entropies [B].  (The reference feeds one noise row against the whole batch of encodings,
        model.py:584-590; here every row is paired with its own encoding.)"""
        eng = self._stage(inputs, None, encoding, conditions)
        eng.forward_flows()
        logs = sum(f.prm[:, 0].view(eng.B, eng.T).sum(1) for f in eng.flows)
        return (logs + 2.0 * eng.T).double().cpu().numpy()

    def fit(self, sampler, steps):
        """``steps`` distillation steps (``train_fast``'s) on batches a ``dataset.DistillSampler`` draws on the device:
        clips, logistic noise and -- with condition_size > 0 -- the labels' one-hot rows; the frozen teacher's encoder
        runs inside the step and its encoding goes straight into the conditioning inputs.  The teacher must be a
        ``WaveNetAutoEncoder`` (object or directory).  Returns (loss [steps], power_loss [steps]), float32; the entropies
        are in the sampler's ring (``sampler.entropies``).  See ``_fit``."""
        from .dataset import DistillSampler
        self._refuse_in_ema("fit")
        if not isinstance(sampler, DistillSampler):
            raise NotImplementedError("ParallelWaveNet.fit: a student step needs noise and teacher passes beside the clips; "
                                      "feed it with train(sess, inputs, truth, encoding, conditions)")
        if self._teacher is not None and not isinstance(self._teacher, WaveNetAutoEncoder):
            raise NotImplementedError("ParallelWaveNet.fit runs the teacher's encoder inside the step: build the student "
                                      "on a WaveNetAutoEncoder teacher (a decoder-only teacher has no encoder)")
        if self.condition_size > 0:
            _fit_labels(sampler, self.condition_size, "ParallelWaveNet", "conditions")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        enc, tch = self._teacher._engine(eng.B, eng.T).enc, eng.teacher
        tables = [tch.cond_in] + [f.cond_in for f in eng.flows]
        dest = dict(audio=enc.x, audio2=eng.truth, audio3=tch.audio, noise=eng.noise)
        if self.condition_size > 0:
            dest.update(tables=tables, rows=tch.frames, col0=self.latent_channels)

        def between():      # the teacher's encoding of the clips, into the latent columns of every conditioning input
            enc.forward()
            sampler.scatter(enc.enc, tables)
        return _fit(eng, sampler, steps, dest, between)

    def evaluate(self, sampler):
        """The forward-only ``(loss, power_loss, entropy)`` of every batch of one sweep of a held-out set, float32
        [steps] each: a step is ``fit``'s without the backward pass and the update -- {``srwn_distill_draw``, the teacher
        encoder's forward pass and ``srwn_cond_scatter``, the student's forward pass, ``srwn_distill_log``} -- replayed
        from a graph of its own; the noise is the sampler's ``noise_plan`` and the conditions are as in ``fit``.  Takes a
        ``dataset.DistillSampler`` built with ``shuffle=False`` whose set is a multiple of batch_size * world (the losses
        are one number per batch).  The host waits once per ``log_capacity`` steps.  Nothing else changes: the flows'
        parameters, their Adam moments, the optimizer's step, the frozen teacher and a training sampler's state keep their
        bits."""
        from .dataset import DistillSampler
        steps = _loss_sweep_steps(sampler, "ParallelWaveNet", DistillSampler,
                                  "a dataset.DistillSampler (dataset.distill_sampler(..., shuffle=False))")
        if self._teacher is not None and not isinstance(self._teacher, WaveNetAutoEncoder):
            raise NotImplementedError("ParallelWaveNet.evaluate runs the teacher's encoder inside the step: build the "
                                      "student on a WaveNetAutoEncoder teacher (a decoder-only teacher has no encoder)")
        if self.condition_size > 0:
            d = sampler.dataset
            if d.labels is None:
                raise ValueError("ParallelWaveNet.evaluate: the dataset holds no labels; their one-hot rows are the "
                                 "conditions")
            if d.num_classes != int(self.condition_size):
                raise ValueError("ParallelWaveNet.evaluate: the dataset has num_classes=%d, the model's conditions are %d "
                                 "wide" % (d.num_classes, int(self.condition_size)))
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        enc, tch = self._teacher._engine(eng.B, eng.T).enc, eng.teacher
        tables = [tch.cond_in] + [f.cond_in for f in eng.flows]
        dest = dict(audio=enc.x, audio2=eng.truth, audio3=tch.audio, noise=eng.noise)
        if self.condition_size > 0:
            dest.update(tables=tables, rows=tch.frames, col0=self.latent_channels)

        def step():
            sampler.draw(**dest)
            enc.forward()
            sampler.scatter(enc.enc, tables)
            eng.forward()
            sampler.log_engine(eng)

        def tick():
            sampler.step += 1
        sampler.seek(0)
        pieces, done = [], 0
        while done < steps:
            n = min(steps - done, sampler.log_capacity)
            _sweep_steps(eng, sampler, step, n, tick)
            pieces.append((sampler.losses(done, n), sampler.power_losses(done, n), sampler.entropies(done, n)))   # waits
            done += n
        return tuple(np.concatenate([p[i] for p in pieces]) for i in range(3))

    def train_fast(self, sess, inputs, truth, encoding, conditions=None):
        """One distillation step (model.py:634-642): returns (loss, power_loss)."""
        self._refuse_in_ema("train_fast")
        eng = self._stage(inputs, truth, encoding, conditions)
        _train_step(eng)
        l = eng.losses()
        return np.float32(l["loss"]), np.float32(l["power_loss"])

    def train(self, sess, inputs, truth, encoding, conditions=None):
        """The slow path (model.py:599-632): per-noise-row gradients, each clipped to norm 1, then averaged and
        applied; returns (mean loss, mean power loss).  student.py:107 trains with ``train_fast``."""
        self._refuse_in_ema("train")
        eng = self._stage(inputs, truth, encoding, conditions)
        l, p = eng.train_per_sample()
        return np.float32(l), np.float32(p)

    def _ae_teacher(self, inputs):
        if self._teacher is None:
            x = np.asarray(inputs)
            self._teacher = WaveNetAutoEncoder.from_checkpoint(self._teacher_dir, x.shape[0], x.shape[1], dtype=self._dtype)
        if not isinstance(self._teacher, WaveNetAutoEncoder):
            raise NotImplementedError("encode/reconstruct run the teacher's encoder (model.py:644-656): build the "
                                      "student on a WaveNetAutoEncoder teacher")
        return self._teacher

    def encode(self, sess, inputs, conditions=None):
        """The teacher's encoding of a clip (``teacher_encoding``, model.py:644-649)."""
        return self._ae_teacher(inputs).encode(inputs, conditions)

    def reconstruct(self, sess, inputs, conditions=None):
        """The teacher's own reconstruction (``teacher_out``, model.py:651-656)."""
        return self._ae_teacher(inputs).reconstruct(inputs, conditions)


class StudentSynthesizer(object):
    """The deployable form of the student: the flows of a trained ``ParallelWaveNet`` (model.py:415-535) as a streaming
    synthesizer (``student.FlowSynthesizer``), with no teacher anywhere.  It serves any batch <= ``max_batch`` and any
    length = frames * pool_stride with frames <= ``max_frames``, in one call (``synthesize``) or chunk by chunk
    (``stream``), and streams of any length whose encoding arrives while they run (``live``); the noise is drawn on the
    device from per-stream seeds (or given).  ``load`` reads what
    ``ParallelWaveNet.save`` wrote, by the reference's variable names; the gate and skip variables a flow never reads are
    ignored."""

    def __init__(self, dilations, num_flows, filter_width=2, dilation_channels=32, latent_channels=16, condition_size=0,
                 pool_stride=512, name="ParallelWaveNet", dtype=None, max_batch=1, max_chunk=1600, max_frames=32):
        K._need_gpu()
        from .student import FlowSynthesizer
        self.dilations, self.num_flows = list(dilations), int(num_flows)
        self.filter_width, self.dilation_channels = filter_width, dilation_channels
        self.latent_channels, self.condition_size, self.pool_stride = latent_channels, condition_size, pool_stride
        self._name = name
        self.max_batch, self.max_chunk, self.max_frames = int(max_batch), int(max_chunk), int(max_frames)
        cfg = StackConfig(dilations=list(dilations), filter_width=filter_width, dilation_channels=dilation_channels,
                          cond_channels=latent_channels + condition_size, pool_stride=pool_stride,
                          dtype=dtype or _default_dtype())
        self._eng = FlowSynthesizer(cfg, num_flows, max_batch=max_batch, max_chunk=max_chunk, max_frames=max_frames)

    @property
    def network_params(self):
        out = {}
        for i, w in enumerate(self._eng.weights):
            out.update(w.tf_variables("%s/Flow%d/Flow%d" % (self._name, i, i)))           # model.py:417,468,510
        return out

    def load(self, logdir):
        ok = _read_state(logdir, lambda: self.network_params)
        if ok:
            self._eng.repack()
        return ok

    @classmethod
    def from_checkpoint(cls, logdir, dilations, num_flows, **kwargs):
        """A synthesizer on the flows saved in `logdir` (``ParallelWaveNet.save``); the hyper-parameters are the
        constructor's (the student's checkpoint holds variables only)."""
        syn = cls(dilations, num_flows, **kwargs)
        if not syn.load(logdir):
            raise FileNotFoundError("%s: no student checkpoint (ParallelWaveNet.save writes one)" % logdir)
        return syn

    # ------------------------------------------------------------------------------------------------
    def _begin(self, encoding, conditions, seed, temperature, noise):
        enc = np.asarray(encoding, dtype=np.float32)
        if enc.ndim != 3 or enc.shape[2] != self.latent_channels:
            raise ValueError("encoding must be [batch, frames, latent_channels=%d]" % self.latent_channels)
        B, frames = int(enc.shape[0]), int(enc.shape[1])
        if not 1 <= B <= self.max_batch or not 1 <= frames <= self.max_frames:
            raise ValueError("encoding of %d streams x %d frames: this synthesizer was built for max_batch=%d, max_frames=%d"
                             % (B, frames, self.max_batch, self.max_frames))
        e = torch.as_tensor(enc)
        if self.condition_size > 0:
            if conditions is None:
                raise ValueError("this student was built with condition_size > 0; pass conditions [B, condition_size]")
            c = np.asarray(conditions, dtype=np.float32)
            if c.shape != (B, self.condition_size):
                raise ValueError("conditions must be [%d, %d]" % (B, self.condition_size))
            e = _tile_conditions(e, torch.as_tensor(c))
        T = frames * self.pool_stride
        nz = None
        if noise is not None:
            nz = torch.as_tensor(np.asarray(noise, dtype=np.float32))
            if tuple(nz.shape) == (B, T, 1):      # (what StudentInverter.invert returns)
                nz = nz[:, :, 0]
            if tuple(nz.shape) != (B, T):
                raise ValueError("noise must be [%d, %d] (= frames * pool_stride)" % (B, T))
            nz = nz.to("cuda")
        st = self._eng.start(e.contiguous(), seed, temperature)
        return st, nz, B, T

    def _chunks(self, st, nz, T, size):
        t = 0
        while t < T:
            n = min(size, T - t)
            yield self._eng.step(st, n, None if nz is None else nz[:, t:t + n])
            t += n

    def synthesize(self, encoding, conditions=None, seed=0, temperature=1.0, noise=None):
        """encoding [B, frames, latent_channels] -> audio [B, frames * pool_stride, 1] in [-1, 1] (model.py:535), made in
        chunks of max_chunk.  seed / temperature: scalars or one per stream (a scalar seed s: stream b draws with s + b);
        noise [B, T] (or [B, T, 1], as ``StudentInverter.invert`` returns it): the logistic noise itself
        (``ParallelWaveNet.generate``'s `inputs`)."""
        st, nz, B, T = self._begin(encoding, conditions, seed, temperature, noise)
        out = torch.cat(list(self._chunks(st, nz, T, self.max_chunk)), dim=1)
        return out.view(B, T, 1).cpu().numpy()

    def stream(self, encoding, conditions=None, chunk_size=160, seed=0, temperature=1.0, noise=None):
        """The same audio as an iterator of NumPy [B, chunk, 1] blocks (the last one shorter when chunk_size does not
        divide the length); chunking never changes a sample."""
        chunk_size = int(chunk_size)
        if not 1 <= chunk_size <= self.max_chunk:
            raise ValueError("chunk_size %d: 1..max_chunk = %d" % (chunk_size, self.max_chunk))
        st, nz, B, T = self._begin(encoding, conditions, seed, temperature, noise)
        return (c.view(B, -1, 1).cpu().numpy() for c in self._chunks(st, nz, T, chunk_size))

    def pool(self):
        """A ``SynthesisPool`` on this synthesizer's buffers: ``max_batch`` slots that streams join and leave while it
        runs.  It ends a running ``stream``; the next ``synthesize`` / ``stream`` closes the pool."""
        K._need_gpu()
        return SynthesisPool(self._eng.pool(), self.latent_channels, self.condition_size)

    def live(self, batch, conditions=None, seed=0, temperature=1.0):
        """A ``LiveSynthesis`` of `batch` streams whose encoding arrives while they run: ``feed`` frames, ``step`` samples,
        with no bound on the length (the conditioning tables are rings of ``max_frames`` frames).  conditions
        [batch, condition_size] are tiled onto every fed frame.  It ends a running ``stream`` or pool, like ``synthesize``."""
        K._need_gpu()
        return LiveSynthesis(self, int(batch), conditions, seed, temperature)

    def inverter(self, max_batch=None):
        """A ``StudentInverter`` on this synthesizer's own flow weights (one snapshot serves both directions):
        ``synth.synthesize(encoding, conditions, noise=inv.invert(x, encoding, conditions))`` is the round trip."""
        return StudentInverter(self.dilations, self.num_flows, filter_width=self.filter_width,
                               dilation_channels=self.dilation_channels, latent_channels=self.latent_channels,
                               condition_size=self.condition_size, pool_stride=self.pool_stride, name=self._name,
                               dtype=self._eng.dt, max_batch=self.max_batch if max_batch is None else max_batch,
                               _share=self._eng)


class StudentInverter(object):
    """The reverse direction of the student (``student.FlowInverter``): audio in, out the logistic noise that the flows of
    a trained ``ParallelWaveNet`` (model.py:456-535) turn into it, and its exact log-likelihood under the student,
    nll[b, t] = -log logistic(z[b, t]; 0, 1) + sum over the flows of their log scales at t (nats).  The inverse of an
    autoregressive flow is sequential: one persistent launch per flow and chunk steps through the samples.

    The audio is taken as the flows' UNCLIPPED output: samples that the student clipped at +-1 (model.py:535) do not
    invert to the noise that made them.  ``load`` reads what ``ParallelWaveNet.save`` wrote."""

    def __init__(self, dilations, num_flows, filter_width=2, dilation_channels=32, latent_channels=16, condition_size=0,
                 pool_stride=512, name="ParallelWaveNet", dtype=None, max_batch=1, gate_mode="reference", _share=None):
        from .student import FlowInverter
        self.dilations, self.num_flows = list(dilations), int(num_flows)
        self.filter_width, self.dilation_channels = filter_width, dilation_channels
        self.latent_channels, self.condition_size, self.pool_stride = latent_channels, condition_size, pool_stride
        self._name, self.max_batch = name, int(max_batch)
        cfg = StackConfig(dilations=list(dilations), filter_width=filter_width, dilation_channels=dilation_channels,
                          cond_channels=latent_channels + condition_size, pool_stride=pool_stride,
                          dtype=dtype or _default_dtype(), gate_mode=gate_mode)
        if _share is None:
            self._eng = FlowInverter(cfg, num_flows, max_batch=max_batch)
        else:      # a FlowSynthesizer: its weights
            self._eng = FlowInverter(cfg, num_flows, max_batch=max_batch, device=_share.dev, weights=_share.weights)

    @property
    def network_params(self):
        out = {}
        for i, w in enumerate(self._eng.weights):
            out.update(w.tf_variables("%s/Flow%d/Flow%d" % (self._name, i, i)))           # model.py:417,468,510
        return out

    def load(self, logdir):
        ok = _read_state(logdir, lambda: self.network_params)
        if ok:
            for w in self._eng.weights:
                w.repack()
            self._eng.repack()
        return ok

    @classmethod
    def from_checkpoint(cls, logdir, dilations, num_flows, **kwargs):
        """An inverter on the flows saved in `logdir` (``ParallelWaveNet.save``); the hyper-parameters are the
        constructor's (the student's checkpoint holds variables only)."""
        inv = cls(dilations, num_flows, **kwargs)
        if not inv.load(logdir):
            raise FileNotFoundError("%s: no student checkpoint (ParallelWaveNet.save writes one)" % logdir)
        return inv

    # ------------------------------------------------------------------------------------------------
    def _cond(self, encoding, conditions):
        """encoding [B, frames, latent] (+ conditions [B, condition_size]) -> encoding_w_condition as a host tensor; every
        refusal, no device work."""
        enc = np.asarray(encoding, dtype=np.float32)
        if enc.ndim != 3 or enc.shape[2] != self.latent_channels:
            raise ValueError("encoding must be [batch, frames, latent_channels=%d]" % self.latent_channels)
        B = int(enc.shape[0])
        if not 1 <= B <= self.max_batch or enc.shape[1] < 1:
            raise ValueError("encoding of %d streams x %d frames: this inverter was built for max_batch=%d"
                             % (B, enc.shape[1], self.max_batch))
        c = _check_conditions(B, conditions, self.condition_size, "student")
        e = torch.as_tensor(enc)
        return e if c is None else _tile_conditions(e, torch.as_tensor(c))

    def _audio(self, audio, batch, length=None):
        x = np.asarray(audio, dtype=np.float32)
        if x.ndim == 3 and x.shape[2] == 1:
            x = x[:, :, 0]
        if x.ndim != 2 or x.shape[0] != batch or (length is not None and x.shape[1] != length):
            raise ValueError("audio must be [%d, %s], got %s" % (batch, "n" if length is None else length, np.shape(audio)))
        return x

    def _invert(self, audio, encoding, conditions):
        from .student import logistic_nll
        e = self._cond(encoding, conditions)
        x = self._audio(audio, e.shape[0], e.shape[1] * self.pool_stride)
        z, ls = self._eng.invert(torch.as_tensor(x), e.contiguous())
        return z, logistic_nll(z, ls)

    def invert(self, audio, encoding, conditions=None):
        """audio [B, T = frames * pool_stride] (or [B, T, 1]) -> noise [B, T, 1], ``ParallelWaveNet.generate``'s `inputs`."""
        z, _ = self._invert(audio, encoding, conditions)
        return z.view(z.shape[0], -1, 1).cpu().numpy()

    def log_likelihood(self, audio, encoding, conditions=None):
        """-log p(audio[b, t] | audio[b, < t], encoding) under the student, [B, T] in nats."""
        return self._invert(audio, encoding, conditions)[1].cpu().numpy()

    def stream(self, encoding, conditions=None):
        """An ``InversionStream`` over the encoding: ``push`` audio chunk by chunk; chunking never changes a bit."""
        e = self._cond(encoding, conditions)
        return InversionStream(self, self._eng.start(e.contiguous()))


class InversionStream(object):
    """NumPy face of one running batch of inversion streams (``StudentInverter.stream``).  ``t``: samples inverted per
    stream."""

    def __init__(self, owner, state):
        self._owner, self._st, self.batch_size = owner, state, state.B
        self._nll_sum = np.zeros(state.B, np.float64)

    @property
    def t(self):
        return self._st.t

    def push(self, audio):
        """audio [B, n] -> (noise [B, n], nll [B, n]) of exactly those samples.  A push past frames * pool_stride is
        refused (ValueError) and leaves the stream where it was."""
        from .student import logistic_nll
        x = self._owner._audio(audio, self._st.B)
        z, ls = self._owner._eng.step(self._st, torch.as_tensor(x))
        nll = logistic_nll(z, ls).cpu().numpy()
        self._nll_sum += nll.sum(1, dtype=np.float64)
        return z.cpu().numpy(), nll

    def bits_per_sample(self):
        """Mean nll of everything pushed so far, in bits, per stream [B] (NaN before the first sample)."""
        from .scorer import bits_per_sample
        return np.array([bits_per_sample(v, self._st.t) for v in self._nll_sum])


class LiveSynthesis(_LiveStream):
    """One running batch of live streams (``StudentSynthesizer.live``).  ``feed(encoding [B, k, latent])`` hands every
    stream its next k frames (k <= ``room``), ``step(n)`` returns the next n <= ``available`` samples [B, n, 1]; ``t``:
    samples made so far.  The samples are those ``synthesize`` gives the whole encoding with the same seed and
    temperature, however the frames and chunks were cut."""

    def __init__(self, owner, batch, conditions, seed, temperature):
        if not 1 <= batch <= owner.max_batch:
            raise ValueError("batch %d: this synthesizer was built for max_batch=%d" % (batch, owner.max_batch))
        cond = _device_conditions(batch, conditions, owner.condition_size, "student")
        super().__init__(owner, owner._eng.start(None, seed, temperature, live=True, batch=batch), cond, batch,
                         owner.max_frames)

    @property
    def room(self):
        return self._owner._eng.room(self._st)

    def _take(self, e):
        self._owner._eng.feed(self._st, e)

    def _step_device(self, n):
        return self._owner._eng.step(self._st, n)

    def step(self, n):
        n = int(n)
        return self._step_device(n).view(self.batch_size, n, 1).cpu().numpy()


class SynthesisPool(_PoolFace):
    """NumPy face of a student synthesis pool (student.SynthPool): ``join(encoding=[...], ...)`` takes one
    [frames_i, latent] per stream and returns their slots; ``step(n)`` advances every live slot by n samples with the
    launches of one synthesizer chunk and returns ``{slot: samples}`` of every slot that produced some; a stream that
    reaches its end frees its slot; ``leave(slots)`` ends streams early.  A stream's samples put together are what
    ``StudentSynthesizer.synthesize`` of that stream alone returns with its seed and temperature."""

    def __init__(self, pool, latent, condition_size):
        self._pool, self._latent, self._cs = pool, latent, condition_size
        self._live_cond = {}      # slot -> the conditions of the live stream joined there last

    t = property(lambda self: self._pool.t)

    def join(self, encoding, conditions=None, seed=0, temperature=None, max_samples=None, live=False):
        """encoding: one [frames_i, latent] per stream (a single 2-D array: one stream); conditions: one [condition_size]
        per stream, tiled over its frames; seed: one per stream or a scalar s (stream i draws with s + i).
        live=True: the streams are fed while they run (``feed``); an encoding holds a stream's first frames ([0, latent]:
        none yet), its conditions are kept and tiled onto every frame fed later; a live stream that has used up its frames
        waits (no samples) until it is fed, closed or left."""
        if live:
            K._need_gpu()
        if isinstance(encoding, np.ndarray) and encoding.ndim == 2:
            encoding = [encoding]
            conditions = None if conditions is None else [conditions]
        encoding = list(encoding)
        cond = _pool_encodings(len(encoding), encoding, conditions, self._latent, self._cs)
        slots = self._pool.join(cond, seed, temperature, max_samples, live=live)
        if live and self._cs > 0:
            for u, c in zip(slots, per_stream(conditions, len(slots), "conditions")):
                self._live_cond[u] = np.asarray(c, dtype=np.float32).reshape(1, self._cs)
        return slots

    def feed(self, slots, encoding):
        """The next frames of live slots: encoding[i] [k_i, latent] for slots[i] (k_i <= ``room``)."""
        slots = slot_list(slots, self.capacity, "feed")
        if isinstance(encoding, np.ndarray) and encoding.ndim == 2:
            encoding = [encoding]
        encs = [np.asarray(e, dtype=np.float32) for e in encoding]
        if len(encs) != len(slots):
            raise ValueError("feed: %d slots but %d encodings" % (len(slots), len(encs)))
        for e in encs:
            if e.ndim != 2 or e.shape[1] != self._latent:
                raise ValueError("feed: each encoding is [k, %d], got shape %s" % (self._latent, e.shape))
        if self._cs > 0:
            if any(u not in self._live_cond for u in slots):
                raise ValueError("feed: slots %s are not all live streams of this pool" % (slots,))
            encs = [_tile_conditions_np(e, self._live_cond[u]) for u, e in zip(slots, encs)]
        self._pool.feed(slots, encs)

    def room(self, slot):
        return self._pool.room(int(slot))

    def close(self, slots):
        """No more frames will come for these live streams: each frees its slot at the end of what it was fed."""
        self._pool.close(slots)

    def step(self, n):
        a, ran = self._pool.step(int(n))
        return _ran_dict(a, ran, range(self._pool.capacity))


class Resynthesizer(object):
    """The live pipeline: an ``AudioEncoder`` feeding a ``StudentSynthesizer``.  Audio chunks in, resynthesized audio
    chunks out, with no bound on the length; the latent frames go from the encoder into the synthesizer's conditioning
    rings as device tensors and never visit the host.  Both halves keep their own contracts, so the audio of a stream put
    together equals ``synthesizer.synthesize(encoder.encode(audio), ...)`` however the audio was cut."""

    def __init__(self, encoder, synthesizer):
        K._need_gpu()
        self.lookahead = _check_resynthesis_halves("Resynthesizer", encoder, synthesizer, StudentSynthesizer, "synthesizer",
                                                   "synthesizer")
        cs = synthesizer.condition_size
        if synthesizer._eng.E != encoder.latent_channels + cs:
            raise ValueError("condition_size %d: the synthesizer's flows read %d channels, not %d + %d"
                             % (cs, synthesizer._eng.E, encoder.latent_channels, cs))
        self.encoder, self.synthesizer = encoder, synthesizer
        self.pool_stride = int(encoder.pool_stride)

    def stream(self, batch=1, conditions=None, seed=0, temperature=1.0, chunk_size=160):
        """A ``ResynthesisStream`` of `batch` streams in lockstep: ``push(audio [B, m])`` returns every sample that can be
        made by now, [B, m', 1]; ``finish()`` the rest.  conditions [B, condition_size] are tiled onto every frame on the
        device (model.py:496-499); chunk_size: the largest synthesizer chunk."""
        batch, chunk_size = int(batch), int(chunk_size)
        if not 1 <= batch <= min(self.encoder.max_batch, self.synthesizer.max_batch):
            raise ValueError("batch %d: the encoder holds %d streams, the synthesizer %d"
                             % (batch, self.encoder.max_batch, self.synthesizer.max_batch))
        if not 1 <= chunk_size <= self.synthesizer.max_chunk:
            raise ValueError("chunk_size %d: 1..max_chunk = %d" % (chunk_size, self.synthesizer.max_chunk))
        return ResynthesisStream(self, batch, conditions, seed, temperature, chunk_size)

    def pool(self, chunk_size=160, audio_ring=None):
        """A ``ResynthesisPool``: independent callers on one encoder and one synthesizer.  Streams join and leave while the
        batch runs, audio arrives ragged, and each caller receives what it would have received alone.  chunk_size: the
        samples a ``step`` makes per stream at most; audio_ring: samples of audio a slot can hold (``AudioEncoder.pool``)."""
        K._need_gpu()
        return ResynthesisPool(self, int(chunk_size), audio_ring)


class ResynthesisStream(_ResynthesisStream):
    """One running batch of ``Resynthesizer.stream``: ``push`` / ``finish`` return samples [B, m, 1]."""

    _tail = (1,)

    def _start_live(self, batch, conditions, seed, temperature):
        return self._owner.synthesizer.live(batch, conditions, seed, temperature)


class _ResynthesisPool(SlotTable):
    """What ``ResynthesisPool`` and ``TeacherResynthesisPool`` share: an encoder pool ``_enc`` and a live decoding half
    ``_half`` (a pool with ``room`` / ``feed`` / ``close`` / ``leave`` / ``t`` and ``_active``) sharing slot ids, the
    streams' conditions ``_cond`` (slot -> [1, condition_size] on the device, None without: a slot is taken while it has an
    entry), ``_cs`` and ``_chunk``.  A subclass gives ``_half``, ``_half_join`` and ``_half_step``.
    One ``step``: the encoder emits for each slot at most the frames the decoding half's conditioning ring has room for
    (the rest stays audio in the slot's audio ring: there is no second queue), the new frames are fed as device tensors
    with the slot's conditions tiled on, the slots whose audio is finished and fully encoded are closed, and the
    decoding half makes up to ``chunk_size`` samples per slot.  A stream that reaches its end frees its slot in both
    halves."""

    _who = "student"

    @property
    def _active(self):      # (what SlotTable reads: a slot is taken while it has an entry in _cond)
        return np.array([u in self._cond for u in range(self.capacity)], bool)

    @property
    def t(self):
        """Samples returned so far, per slot."""
        return self._half.t[:self.capacity]

    @property
    def received(self):
        return self._enc.received[:self.capacity]

    def audio_room(self, slot):
        return self._enc.audio_room(int(slot))

    def _slots(self, slots, who):
        slots = self._slot_list(slots, who)
        if any(u not in self._cond for u in slots):
            raise ValueError("%s: slots %s do not all hold a stream of this pool" % (who, slots))
        return slots

    def join(self, conditions=None, seed=0, temperature=None, n=1):
        """n streams into the lowest free slots; conditions [n, condition_size] (one row per stream), seed a scalar s
        (stream i draws with s + i) or one per stream, temperature None, a scalar or one per stream.  Returns the slots."""
        n = int(n)
        slots = self._take_slots(n, None)
        c = _device_conditions(n, conditions, self._cs, self._who)
        conds = [None if c is None else c[i:i + 1] for i in range(n)]
        self._half_join(n, seed, temperature, slots)
        self._enc.join(slots=slots)
        for u, c in zip(slots, conds):
            self._cond[u] = c
        return slots

    def push(self, slots, audio):
        self._enc.push(self._slots(slots, "push"), _audio_pieces(slots, audio))

    def finish(self, slots):
        """No more audio comes for these streams; each frees its slot once its last sample has been returned."""
        self._enc.finish(self._slots(slots, "finish"))

    def leave(self, slots):
        """Ends these streams where they are and frees their slots in both halves."""
        slots = self._slots(slots, "leave")
        self._enc.leave(slots)
        self._half.leave(slots)
        for u in slots:
            del self._cond[u]

    def step(self):
        if not self._cond:
            return {}
        enc, half = self._enc, self._half
        frames = enc.step({u: half.room(u) for u in enc.active})
        if frames:
            us = sorted(frames)
            fr = [frames[u] if self._cond[u] is None else _tile_conditions(frames[u][None], self._cond[u])[0] for u in us]
            half.feed(us, fr)
        done = [u for u in self._cond if not enc._active[u]]          # finished and fully encoded: the stream's end is known
        if done:
            half.close(done)
        a, ran = self._half_step(self._chunk)
        out = _ran_dict(a, ran, self._cond) if ran.any() else {}
        for u in [u for u in self._cond if not half._active[u]]:
            del self._cond[u]
        return out


class ResynthesisPool(_ResynthesisPool):
    """``Resynthesizer.pool()``: an encoder pool and a live synthesis pool sharing slot ids; capacity is the smaller
    ``max_batch``.  ``join`` returns slots, ``push(slots, audio)`` takes one 1-D array per slot of any length (at most
    ``audio_room(slot)``), ``finish(slots)`` ends streams, ``step()`` returns ``{slot: samples}`` (``_ResynthesisPool``:
    frames the synthesizer's ring has room for, fed as device tensors; up to ``chunk_size`` samples per slot).  A stream's
    samples put together are ``synthesizer.synthesize(encoder.encode(audio), conditions, seed, temperature)`` of it
    alone."""

    def __init__(self, owner, chunk_size, audio_ring):
        from .student import live_min_frames
        enc, syn = owner.encoder, owner.synthesizer
        if not 1 <= chunk_size <= syn.max_chunk:
            raise ValueError("chunk_size %d: 1..max_chunk = %d" % (chunk_size, syn.max_chunk))
        need = live_min_frames(max(syn._eng.hist), owner.pool_stride)
        if syn.max_frames < need:
            raise ValueError("pool: live streams need a synthesizer ring of max_frames >= %d frames, this one holds %d"
                             % (need, syn.max_frames))
        self._owner, self._chunk = owner, chunk_size
        self.capacity = min(enc.max_batch, syn.max_batch)
        self._cs = syn.condition_size
        self._enc = enc._eng.pool(audio_ring)
        self._syn = syn._eng.pool()
        self._cond = {}        # slot -> its stream's conditions [1, condition_size] on the device (None without)

    _half = property(lambda self: self._syn)

    def _half_join(self, n, seed, temperature, slots):
        self._syn.join([None] * n, seed, temperature, slots=slots, live=True)

    def _half_step(self, chunk):
        return self._syn.step(chunk)


class TeacherResynthesisPool(_ResynthesisPool):
    """``TeacherResynthesizer.pool()``: an encoder pool and a LIVE generation pool of the decoder sharing slot ids;
    capacity is the encoder's ``max_batch``, the decoder's conditioning rings hold ``max_frames`` frames.  The contract of
    ``ResynthesisPool`` at teacher quality: ``join`` returns slots, ``push(slots, audio)`` takes one 1-D array per slot of
    any length (at most ``audio_room(slot)``), ``finish(slots)`` ends streams, ``step()`` returns ``{slot: samples}``.  A
    stream's samples put together are ``autoencoder.generate(encoder.encode(audio), conditions, seed=seed,
    temperature=temperature)`` of it alone."""

    _who = "auto-encoder"

    def __init__(self, owner, chunk_size, audio_ring):
        if chunk_size < 1:
            raise ValueError("chunk_size %d: at least 1" % chunk_size)
        enc, ae = owner.encoder, owner.autoencoder
        self._owner, self._chunk = owner, chunk_size
        self.capacity = int(enc.max_batch)
        self._cs = int(ae.condition_size)
        self._enc = enc._eng.pool(audio_ring)
        eng = ae._eng or ae._engine(1, owner.max_frames * owner.pool_stride)
        self._dec = eng.dec.generation_pool(self.capacity, owner.max_frames, live=True)
        self._cond = {}        # slot -> its stream's conditions [1, condition_size] on the device (None without)

    _half = property(lambda self: self._dec)

    def _half_join(self, n, seed, temperature, slots):
        sd = np.asarray(seed)
        seeds = [int(sd) + i for i in range(n)] if sd.ndim == 0 else [int(v) for v in per_stream(seed, n, "seeds", default=0)]
        self._dec.join(seeds, None, [None] * n, None, slots, temperature=temperature, live=True)

    def _half_step(self, chunk):
        dec = self._dec
        if not dec.any_runnable:      # every stream waits for frames: nothing is launched
            return None, np.zeros(self.capacity, np.int64)
        a, _, _, ran = dec.step(chunk, mode="sample")
        return a, ran


class SiameseWaveNet(_EngineOwner):
    """model.py:660-797: two towers of class ``WaveNet``'s network (input conv, residual stack, skip sum, relu -> 1x1
    -> relu -> 1x1, average pool over the whole clip) that share one set of weights, trained on pairs with the
    Hadsell-Chopra-LeCun contrastive loss under the reference's label convention (y = 1: "same", model.py:747-749).

    The towers share their weights, so a pair batch runs as ONE engine batch of 2P clips (the left clips, then the
    right ones) and the weight gradients come out summed over both towers.  The ``sess`` argument of every method is
    accepted for call compatibility with siamese.py and ignored (there is no session).
    ``train(sess, left[P,T], right[P,T], labels[P]) -> (loss, distance[P])``; ``get_embedding -> [B,1,D]``;
    ``get_distance -> [P]``.  Checkpoint names are those of the left tower, ``{name}/siamese/...`` (model.py:689)."""

    def __init__(self, input_size, output_dimensions, dilations, margin=5.0, filter_width=2, dilation_channels=32,
                 skip_channels=256, name="SiameseWaveNet", learning_rate=0.001, dtype=None, seed=0):
        self.input_size = input_size
        self.output_dimensions = output_dimensions
        self.dilations = dilations
        self.margin = margin
        self.filter_width = filter_width
        self.dilation_channels = dilation_channels
        self.skip_channels = skip_channels
        self._scope, self._decoder_names, self._default_length = name + "/siamese", False, int(input_size)
        self._setup(StackConfig(dilations=list(dilations), filter_width=filter_width,
                                dilation_channels=dilation_channels, skip_channels=skip_channels,
                                output_channels=output_dimensions, shift_input=False, head_mode="contrastive",
                                margin=float(margin), dtype=dtype or _default_dtype(), learning_rate=learning_rate),
                    seed)

    def _clips(self, inputs, what="inputs"):
        x = np.asarray(inputs, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("%s must be [batch, samples]" % what)
        if x.shape[1] != self.input_size:
            # tf.nn.pool window = input_size, VALID, then squeezed (model.py:710, 731): other lengths do not embed
            raise ValueError("%s have %d samples, the model was built for input_size=%d" % (what, x.shape[1], self.input_size))
        return x

    def _pair(self, inputs_left, inputs_right):
        left, right = self._clips(inputs_left, "inputs_left"), self._clips(inputs_right, "inputs_right")
        if left.shape[0] != right.shape[0]:
            raise ValueError("inputs_left and inputs_right must hold the same number of clips (%d vs %d)"
                             % (left.shape[0], right.shape[0]))
        return np.concatenate([left, right], axis=0)

    def _stage(self, x, labels=None):
        eng = self._engine(x.shape[0], x.shape[1])
        eng.set_inputs(torch.as_tensor(x, device="cuda"),
                       None if labels is None else torch.as_tensor(labels, device="cuda"))
        return eng

    def load(self, sess, logdir):
        return super().load(logdir)

    def save(self, sess, logdir, global_step, force=False, fmt=None):
        return super().save(logdir, global_step, force, fmt)

    def fit(self, sampler, steps, validate=None):
        """``steps`` training steps (``train``'s) on the pairs a ``dataset.PairSampler`` draws on the device from a
        labelled set of recordings.  Returns (loss [steps], distance [steps, P]), float32.  See ``_fit``.

        ``validate=(embed_sampler, every)``: one sweep of a ``dataset.EmbedSampler`` (``evaluate``'s) is enqueued behind
        every training step whose count -- ``sampler.step`` after the step -- is a multiple of `every`, with the contract
        of ``WaveNet.fit``'s ``validate``: each sweep lands in the next of the sampler's result slots, the slots are read
        when ``sweep_capacity`` of them are full and at the end, and the training run's bits are the ones without
        validation.  Returns ``(loss, distance, [PairEvalResult, ...])`` then, every result with the ``step`` it was
        taken at."""
        from .dataset import EmbedSampler, PairSampler
        self._refuse_in_ema("fit")
        if not isinstance(sampler, PairSampler):
            raise NotImplementedError("SiameseWaveNet.fit: a step needs pairs of clips and their labels; feed it with "
                                      "train(sess, inputs_left, inputs_right, labels)")
        if sampler.num_samples != self.input_size:
            raise ValueError("SiameseWaveNet.fit: the sampler draws %d samples, the model was built for input_size=%d"
                             % (sampler.num_samples, self.input_size))
        if validate is None:
            eng = self._engine(2 * sampler.pairs, sampler.num_samples)
            return _fit(eng, sampler, steps, dict(audio=eng.audio, labels=eng.labels))
        es, every = _check_validate(validate, EmbedSampler, "a dataset.EmbedSampler (dataset.embed_sampler(...))")
        self._check_embed(es)
        eng = self._engine(2 * sampler.pairs, sampler.num_samples)
        eng_v = self._engine(es.batch_size, es.num_samples)
        results, pending = [], []            # pending: (sweep number, training step) of the sweeps still in their slots

        def drain():                         # the host waits here
            results.extend(es.result(k, s) for k, s in pending)
            del pending[:]

        def after_step():
            if sampler.step % every == 0:
                if len(pending) >= es.sweep_capacity:
                    drain()
                if self._validate_ema():         # as WaveNet.fit: the sweep judges the averaged weights
                    eng.swap_ema()
                self._embed_sweep(eng_v, es)
                if self._validate_ema():
                    eng.swap_ema()
                pending.append((es.sweep - 1, sampler.step))

        loss, dist = _fit(eng, sampler, steps, dict(audio=eng.audio, labels=eng.labels), after_step=after_step)
        drain()
        return loss, dist, results

    def _check_embed(self, es):
        """An ``EmbedSampler`` this model can sweep; binds it to the embedding's width and, without a d_max of its own, to
        a histogram range of twice the margin (beyond the margin a pair of two labels costs nothing)."""
        from .dataset import EmbedSampler
        if not isinstance(es, EmbedSampler):
            raise TypeError("SiameseWaveNet.evaluate takes a dataset.EmbedSampler (dataset.embed_sampler(...)), got %s"
                            % type(es).__name__)
        if es.num_samples != self.input_size:
            raise ValueError("SiameseWaveNet.evaluate: the sampler draws %d samples, the model was built for input_size=%d"
                             % (es.num_samples, self.input_size))
        es.bind(self.output_dimensions, 2.0 * float(self.margin))

    @staticmethod
    def _embed_sweep(eng, es, distances=False):
        """One sweep of an ``EmbedSampler`` through a tower, enqueued: ``sweep_steps`` steps of {srwn_batch_draw into the
        engine's audio, ``get_embedding``'s forward pass -- no pairs, no loss --, srwn_embed_collect}, then srwn_pair_sweep
        over the slot ``(es.sweep - 1) % sweep_capacity``.  Nothing waits for it here."""
        def step():
            es.draw(audio=eng.audio)
            eng.forward(with_loss=False)
            es.collect(eng.emb)
        es.seek(0)
        _sweep_steps(eng, es, step, es.sweep_steps, es.stepped)
        es.pair_sweep(distances)

    def evaluate(self, embed_sampler, step=None, distances=False):
        """One sweep of a labelled held-out set on the device and one launch over all its pairs: ``sweep_steps`` replays of
        {draw, the tower's forward pass, ``srwn_embed_collect``}, ``srwn_pair_sweep``, then the host waits once.  Returns a
        ``PairEvalResult`` (dataset.py): the embeddings, per record the nearest record, the nearest one of its label and
        the rank of that one among the records of other labels, the distance histograms of the pairs of one label and of
        two, and from them nearest-neighbour accuracy, recall@k, FAR / FRR at the bin edges, EER and AUC; with
        `distances` the [N, N] matrix too.  The sampler's batch size is any (the engine of that shape runs on the model's
        current parameters, as ``get_embedding`` does).  Nothing else changes: the parameters, the Adam moments, the
        optimizer's step and a training sampler's state keep their bits."""
        self._check_embed(embed_sampler)
        eng = self._engine(embed_sampler.batch_size, embed_sampler.num_samples)
        self._embed_sweep(eng, embed_sampler, bool(distances))
        return embed_sampler.result(embed_sampler.sweep - 1, step, bool(distances))      # the host waits here

    def train(self, sess, inputs_left, inputs_right, labels):
        self._refuse_in_ema("train")
        x = self._pair(inputs_left, inputs_right)
        y = np.asarray(labels, dtype=np.float32).reshape(-1)
        if y.shape[0] != x.shape[0] // 2:
            raise ValueError("labels must hold one value per pair (%d), got %d" % (x.shape[0] // 2, y.shape[0]))
        eng = self._stage(x, y)
        _train_step(eng)
        return np.float32(eng.loss.item()), eng.dist.cpu().numpy()

    def get_embedding(self, sess, inputs):
        eng = self._stage(self._clips(inputs))
        eng.forward(with_loss=False)
        return eng.emb.cpu().numpy()[:, None, :]

    def get_distance(self, sess, inputs_left, inputs_right):
        eng = self._stage(self._pair(inputs_left, inputs_right))
        eng.forward(with_loss=False)
        return eng.dist.cpu().numpy()

    def embedder(self, max_batch=1, hop=None, window=None, max_hops=8, max_gallery=64):
        """A ``StreamingEmbedder`` on a copy of this model's current weights: audio of any length in, the embedding of a
        window of `window` samples (default input_size) sliding by `hop` (default: the window) out, matched against the
        templates enrolled with it.  With hop = window = input_size its single embedding of a clip of input_size samples is
        ``get_embedding``'s."""
        window = int(self.input_size if window is None else window)
        hop = window if hop is None else int(hop)
        from .embedder import EmbedderWeights, check_gallery_size
        from .recognizer import check_classifier_widths, check_hop_window
        check_hop_window(hop, window)
        check_gallery_size(max_gallery)
        check_classifier_widths(self.filter_width, self.dilation_channels, self.skip_channels, "streaming embedder")
        if self._primary is None:
            self._engine(1, self._default_length)
        return StreamingEmbedder(EmbedderWeights.from_engine(self._primary), max_batch=max_batch, hop=hop, window=window,
                                 max_hops=max_hops, max_gallery=max_gallery)


def _embed_host(r, threshold=None):
    """An ``embedder.EmbedResult`` of device tensors -> one of NumPy arrays; with a threshold (result, accepted)."""
    out = type(r)(*(t.cpu().numpy() for t in r))
    return out if threshold is None else (out, out.distance <= np.float32(threshold))


class StreamingEmbedder(object):
    """The deployable form of a ``SiameseWaveNet`` tower (model.py:689-731) with a NumPy face: no training engine, no clip
    length, and a gallery of enrolled templates on the device.  ``embed(audio [B, T])`` -> an ``EmbedResult`` (embeddings
    [B, n_emit, D], nearest [B, n_emit], distance [B, n_emit], distances [B, n_emit, N]) of every window position (j + 1) *
    hop - window, j >= window / hop - 1, of a recording of any length: the reference's distance (model.py:736) to each of
    the N enrolled templates, the nearest one's index (-1 with none enrolled) and its distance.  ``enroll(clips [n,
    window])`` embeds clips with this object's own path and adds them; ``stream(batch)`` -> an ``EmbedderStream`` to
    ``push`` audio into as it arrives.  A result does not depend on how the audio was cut."""

    def __init__(self, weights, max_batch=1, hop=160, window=16000, max_hops=8, max_gallery=64):
        from .embedder import StreamEmbedder
        self._w = weights
        self._eng = StreamEmbedder(weights, max_batch=max_batch, hop=hop, window=window, max_hops=max_hops,
                                   max_gallery=max_gallery)
        e = self._eng
        self.max_batch, self.hop, self.window, self.max_gallery, self.output_dimensions = (e.max_batch, e.hop, e.window,
                                                                                           e.max_gallery, e.D)

    @classmethod
    def from_checkpoint(cls, logdir, dilations, output_dimensions, dilation_channels=32, skip_channels=256, filter_width=2,
                        name="SiameseWaveNet", dtype=None, max_batch=1, hop=160, window=16000, max_hops=8, max_gallery=64):
        """An embedder on the variables saved in `logdir` (``SiameseWaveNet.save``'s .pt form or a TensorFlow bundle, by the
        reference's variable names under `name`/siamese)."""
        from .embedder import EmbedderWeights, check_gallery_size
        from .recognizer import check_classifier_widths, check_hop_window
        check_hop_window(hop, window)
        check_gallery_size(max_gallery)
        check_classifier_widths(filter_width, dilation_channels, skip_channels, "streaming embedder")
        w = EmbedderWeights(dilations, dilation_channels, skip_channels, output_dimensions, filter_width,
                            dtype or _default_dtype())
        if not w.load(logdir, name + "/siamese"):
            raise FileNotFoundError("%s: no checkpoint to restore (SiameseWaveNet.save writes one)" % logdir)
        return cls(w, max_batch=max_batch, hop=hop, window=window, max_hops=max_hops, max_gallery=max_gallery)

    gallery = property(lambda self: self._eng.gallery.cpu().numpy(), doc="The enrolled templates [N, D].")
    labels = property(lambda self: self._eng.labels, doc="One label per enrolled template.")

    def embed(self, inputs):
        """inputs [B, T] -> ``EmbedResult`` (NumPy) of the n_emit = max(0, T // hop - window / hop + 1) window positions."""
        return _embed_host(self._eng.embed(self._eng._check_audio(inputs)))

    def enroll(self, inputs, labels=None):
        """Embeds the clips inputs [n, window] (any n, in batches of max_batch) with this object's own path and enrolls
        the single window of each -> their gallery indices.  Ends the current stream or pool."""
        x = np.asarray(inputs, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.window:
            raise ValueError("enroll: inputs must be [n, window = %d], got shape %s" % (self.window, x.shape))
        labels = None if labels is None else list(labels)
        if labels is not None and len(labels) != x.shape[0]:
            raise ValueError("enroll: %d clips but %d labels" % (x.shape[0], len(labels)))
        if len(self._eng.labels) + x.shape[0] > self.max_gallery:
            raise ValueError("enroll: %d clips behind the %d enrolled, max_gallery is %d"
                             % (x.shape[0], len(self._eng.labels), self.max_gallery))
        if not x.shape[0]:
            return []
        e = torch.cat([self._eng.embed(x[i:i + self.max_batch]).embeddings[:, 0]
                       for i in range(0, x.shape[0], self.max_batch)], 0)
        return self._eng.enroll(e, labels)

    def enroll_embeddings(self, templates, labels=None):
        """Enrolls templates [n, D] that are embeddings already -> their gallery indices."""
        return self._eng.enroll(np.asarray(templates, dtype=np.float32), labels)

    def clear(self):
        self._eng.clear()

    def stream(self, batch_size=1):
        return EmbedderStream(self, self._eng.start(batch_size))

    def pool(self, audio_ring=None):
        """An ``EmbedderStreamPool``: this embedder's ``max_batch`` rows as slots that streams join and leave, each pushing
        audio of any length at a clock of its own, all matched against this embedder's gallery (``embedder.EmbedderPool``).
        Ends the current ``EmbedderStream``; ``stream``, ``embed`` and ``enroll`` end the pool."""
        return EmbedderStreamPool(self._eng.pool(audio_ring))


class EmbedderStream(object):
    """NumPy face of one running batch of embedder streams (``StreamingEmbedder.stream``).  ``t``: samples received per
    stream; ``emitted``: window positions returned so far."""

    def __init__(self, owner, state):
        self._owner, self._st, self.batch_size = owner, state, state.B

    t = property(lambda self: self._st.t)
    emitted = property(lambda self: self._st.emitted)

    def push(self, audio, threshold=None):
        """audio [B, n], any n >= 0 -> the ``EmbedResult`` [B, e, ..] of the e window positions it completed (e may be 0);
        with a threshold (result, accepted [B, e] = distance <= threshold)."""
        return _embed_host(self._owner._eng.push(self._st, audio), threshold)


class EmbedderStreamPool(_AudioPoolFace):
    """NumPy face of an embedder pool (``StreamingEmbedder.pool``; embedder.EmbedderPool).  ``join`` returns slots,
    ``push(slots, audio)`` takes one 1-D array per slot, of any length, ``step()`` returns ``{slot: EmbedResult [e, ..]}`` for
    every slot whose stream completed window positions.  A stream's results put together are ``StreamingEmbedder.embed`` of
    its audio alone under the same gallery."""

    audio_ring = property(lambda self: self._pool.audio_ring)
    consumed = property(lambda self: self._pool.consumed)

    def step(self, threshold=None):
        return {u: _embed_host(r, threshold) for u, r in self._pool.step().items()}


class AutoEncoderScorerPool(_ResynthesisPool):
    """``AutoEncoderScorer.pool()``: an encoder pool ``_enc`` and a ``scorer.MolScorerPool`` ``_mol`` sharing slot ids, with
    the contract of the resynthesis pools; capacity is the smaller ``max_batch``.  ``join(conditions, n)`` returns slots,
    ``push(slots, audio)`` takes one 1-D array per slot of any length (at most ``audio_room(slot)``) and writes it into BOTH
    halves' audio rings (two uploads: the halves keep separate rings), ``finish(slots)`` ends streams, ``leave(slots)``
    drops them, ``step()`` returns ``{slot: nll [m]}`` (NumPy, nats).  One ``step``: the encoder emits for each slot at most
    the frames the scorer's conditioning ring has room for (the rest stays audio), the new frames are fed as device
    tensors with the slot's conditions tiled on, the scorer scores every sample that has its frame, and a slot whose
    encoder half is finished and fully emitted and whose scorer half has scored all it was fed is freed in both halves.
    A stream's values put together are ``AutoEncoderScorer(max_batch=1).score(audio)`` of it alone: its first (T //
    pool_stride) * pool_stride samples; a stream shorter than one frame ends with nothing.
    The scorer half's audio ring must hold what the ENCODER still needs before it can emit the next frame -- with every
    fed sample scored that is pool_stride + L + 1 samples beyond emitted * pool_stride, plus the two samples the entry
    conv carries -- or neither half could move: ``scorer.ae_pool_min_audio_ring``, refused below."""

    _who = "scorer"

    def __init__(self, owner, audio_ring):
        from .scorer import ae_pool_min_audio_ring
        enc, mol = owner.encoder._eng, owner._eng
        need = ae_pool_min_audio_ring(mol.max_chunk, enc.P, enc.L)
        enc_ring = enc.max_frames * enc.P + enc.L + 1 + enc.P            # (the encoder pool's default)
        ring = enc_ring + mol.max_chunk + 2 if audio_ring is None else int(audio_ring)
        if ring < need:
            raise ValueError("pool: audio_ring %d: the scorer half needs at least %d samples (a step of max_chunk + 2 = %d, "
                             "and pool_stride + encoder layers + 3 = %d so that the encoder can complete its next frame)"
                             % (ring, need, mol.max_chunk + 2, enc.P + enc.L + 3))
        self._owner = owner
        self.capacity = min(enc.max_batch, mol.max_batch)
        self._cs = owner.condition_size
        self._enc = enc.pool()
        self._mol = mol.pool(ring)
        self._cond = {}        # slot -> its stream's conditions [1, condition_size] on the device (None without)

    _half = property(lambda self: self._mol)
    t = property(lambda self: self._mol.scored[:self.capacity], doc="Samples scored so far, per slot.")
    scored = t

    def audio_room(self, slot):
        """Samples a slot can take now: the smaller of the two halves' rooms."""
        return min(self._enc.audio_room(int(slot)), self._mol.audio_room(int(slot)))

    def bits_per_sample(self, slot):
        """The running mean nll of the stream in `slot`, in bits (NaN before its first sample)."""
        return self._mol.bits_per_sample(int(slot))

    def join(self, conditions=None, n=1):
        """n streams into the lowest free slots; conditions [n, condition_size] (one row per stream).  Returns the slots."""
        n = int(n)
        self._mol._check_open()
        slots = self._take_slots(n, None)
        c = _device_conditions(n, conditions, self._cs, self._who)
        self._mol.join(slots=slots)
        self._enc.join(slots=slots)
        for i, u in enumerate(slots):
            self._cond[u] = None if c is None else c[i:i + 1]
        return slots

    def push(self, slots, audio):
        """Each piece into both halves' rings.  A piece that fits one half only is refused before either is written, as
        is everything either half refuses."""
        pieces = _audio_pieces(slots, audio)
        slots = self._slots(slots, "push")
        self._mol._check_open()
        if len(pieces) != len(slots):
            raise ValueError("push: %d slots but %d pieces of audio" % (len(slots), len(pieces)))
        for u, x in zip(slots, pieces):
            if x.ndim == 1 and x.shape[0] > self.audio_room(u):
                raise ValueError("push: %d samples for slot %d, but its rings have room for %d (encoder half %d, scorer half "
                                 "%d)" % (x.shape[0], u, self.audio_room(u), self._enc.audio_room(u), self._mol.audio_room(u)))
        self._enc.push(slots, pieces)      # (its refusals -- a finished stream, a wrong dtype or rank -- come before it writes)
        self._mol.push(slots, pieces)

    def leave(self, slots):
        """Ends these streams where they are and frees their slots in both halves."""
        self._mol._check_open()
        super().leave(slots)

    def step(self):
        self._mol._check_open()
        if not self._cond:
            return {}
        enc, mol, P = self._enc, self._mol, self._owner.pool_stride
        frames = enc.step({u: mol.room(u) for u in enc.active})      # frames that do not fit stay audio
        if frames:
            us = sorted(frames)
            mol.feed(us, [frames[u] if self._cond[u] is None else _tile_conditions(frames[u][None], self._cond[u])[0]
                          for u in us])
        out = mol.step()
        done = [u for u in self._cond if not enc._active[u] and mol._scored[u] == mol._fed[u] * P]
        if done:                                                     # finished, fully encoded and fully scored
            mol.leave(done)
            for u in done:
                del self._cond[u]
        return _host_dict(out)
