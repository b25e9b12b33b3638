"""Host-side mirror of the reference's model classes (its ``model.py``) on the MI355X engine.

Same constructor and method signatures, NumPy in / NumPy out like the reference's ``sess.run``
wrappers, but no TensorFlow: the graph body is the fixed kernel sequence of ``engine.WaveNetEngine``.

* ``WaveNet``            -- model.py:8-72 (clip-level softmax classifier), complete.
* ``WaveNetTeacher``     -- the 30-layer mu-law softmax teacher BASELINE.json names (decoder stack of
                            model.py:158-196 with the 256-way softmax head the reference carries at
                            model.py:100-112); this is the benchmark path.
* ``WaveNetAutoEncoder`` -- model.py:75-285: non-causal encoder + conditioned mixture-of-logistics decoder
                            (encoder.AutoEncoderEngine), the teacher teacher.py trains.
* ``ParallelWaveNet``    -- model.py:290-656: the IAF student distilled against that frozen teacher
                            (student.StudentEngine).
* ``SiameseWaveNet``     -- model.py:660-797: two weight-sharing WaveNet towers trained on pairs with the contrastive
                            loss (engine head_mode "contrastive": both towers run as one batch).

What they train with (capture rule, ``fit`` / ``evaluate``, controls, checkpoints) is ``training.py``; the faces they hand
out for deployment (streams, pools, live streams) are ``serving.py``.  Every name of both is a name of this module too.
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
from .serving import (  # noqa: F401
    _default_dtype, _tile_conditions, _tile_conditions_np, _check_conditions, _to_device, _device_conditions,
    StreamingClassifier, ClassifierStream, StreamingScorer, ScorerStream, _MolScorerFace, _MolScoreStreamBase,
    StreamingMolScorer, MolScorerStream, AutoEncoderScorer, AutoEncoderScoreStream, _pool_encodings, _check_prompt,
    _stream_chunks, _ran_dict, _host_dict, _audio_pieces, _PoolFace, GenerationPool, _LiveStream, LiveDecoding,
    _check_resynthesis_halves, _ResynthesisStream, TeacherResynthesizer, TeacherResynthesisStream, AudioEncoder,
    EncoderStream, _AudioPoolFace, AudioEncoderPool, ClassifierPool, ScorerStreamPool, MolScorerStreamPool,
    _flow_variables, _FlowFace, StudentSynthesizer, StudentInverter, InversionStream, LiveSynthesis, SynthesisPool,
    Resynthesizer, ResynthesisStream, _ResynthesisPool, ResynthesisPool, TeacherResynthesisPool, _embed_host,
    StreamingEmbedder, EmbedderStream, EmbedderStreamPool, AutoEncoderScorerPool,
)
from .training import (  # noqa: F401
    _captured_step, _sampler_state, _train_step, _fit_part, _fit, _fit_capture, _fit_validated, _fit_labels,
    _sweep_steps, _eval_sweep, _evaluate_losses, _loss_sweep_steps, _refuse_augment, _check_validate, _write_state, _read_state,
    _TrainingControls, _EmaContext,
)


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
        return self._control_engine().tf_variables(self._scope, decoder=self._decoder_names)

    def _after_load(self):
        self._primary._reset_ema()
        self._primary.repack()


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
        are the targets); returns every step's loss, float32 [steps].  See ``training._fit``.

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
        if validate is not None:
            ev, every = _check_validate(validate)
            self._check_eval(ev)
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        dest = dict(audio=eng.audio, onehot=eng.labels)
        if validate is None:
            return _fit(eng, sampler, steps, dest)[0]
        eng_v = self._engine(ev.batch_size, ev.num_samples)
        (losses,), results = _fit_validated(eng, sampler, steps, dest, ev, every, lambda: _eval_sweep(eng_v, ev),
                                            self._validate_ema())
        return losses, results

    def _check_eval(self, ev):
        from .dataset import EvalSampler
        if not isinstance(ev, EvalSampler):
            raise TypeError("WaveNet.evaluate takes a dataset.EvalSampler (dataset.eval_sampler(...)), got %s"
                            % type(ev).__name__)
        _refuse_augment(ev, "WaveNet")
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
        return StreamingClassifier(ClassifierWeights.from_engine(self._control_engine()), max_batch=max_batch, hop=hop,
                                   window=window, max_hops=max_hops)


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

    def _config(self):
        return self._ctor

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
        draw writes the mu-law targets too); returns every step's loss, float32 [steps].  See ``training._fit``.  The unconditioned
        teacher only: a conditioned teacher's encoding comes from another model."""
        self._refuse_in_ema("fit")
        if self.use_encoding:
            raise NotImplementedError("WaveNetTeacher.fit: this teacher was built with use_encoding=True and its encoding "
                                      "comes from another model; feed it with train(inputs, encoding, conditions)")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        return _fit(eng, sampler, steps, self._dest(eng))[0]

    def _dest(self, eng):
        """Where a ``BatchSampler``'s draw writes what ``set_inputs`` would: the clips, with the softmax head their codes."""
        dest = dict(audio=eng.audio)
        if self.head == "softmax":
            dest.update(codes=eng.targets, quantization_channels=self.quantization_channels)
        return dest

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
        steps = _loss_sweep_steps(sampler, "WaveNetTeacher")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        return _evaluate_losses(eng, sampler, self._dest(eng), steps)[0]

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
        return StreamingScorer(ScorerWeights.from_engine(self._control_engine()), max_batch=max_batch, max_chunk=max_chunk)

    def mol_scorer(self, max_batch=1, max_chunk=1600, max_frames=32):
        """A ``StreamingMolScorer`` on a copy of this teacher's current weights, for head="mol" teachers, conditioned
        (``score(inputs, encoding, conditions)``, frames fed through a ring of ``max_frames``) or not: nll[b, t] = -log
        p(inputs[b, t] | inputs[b, < t], encoding) in nats -- the quantity ``loss`` sums, without the training engine."""
        from .recognizer import check_classifier_widths
        from .scorer import MolScorerWeights
        MolScorerWeights.check_config(self._cfg)
        check_classifier_widths(self._cfg.filter_width, self._cfg.dilation_channels, self._cfg.skip_channels,
                                "streaming scorer")
        return StreamingMolScorer(MolScorerWeights.from_engine(self._control_engine()),
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
            eng = self._control_engine()
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
        eng = self._control_engine()
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
        eng = self._control_engine()
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
        eng = self._control_engine()
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
        eng = self._control_engine()
        out = dict(eng.enc.tf_variables(self._name + "/Encoder"))
        out.update(eng.dec.tf_variables(self._name + "/Decoder", decoder=True))
        return out

    # --- the reference's methods (model.py:217-285) ---------------------------------------------------
    def _config(self):
        return dict(self._ctor, **{"class": "WaveNetAutoEncoder"})

    def _after_load(self):
        self._eng.enc.ctl.reset_ema(self._eng.enc.params); self._eng.dec._reset_ema()
        self._eng.enc.repack(); self._eng.dec.repack()

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
        the labels' one-hot rows are the conditions.  Returns every step's loss, float32 [steps].  See ``training._fit``."""
        self._refuse_in_ema("fit")
        if self.condition_size > 0:
            _fit_labels(sampler, self.condition_size, "WaveNetAutoEncoder", "conditions")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        return _fit(eng, sampler, steps, self._dest(eng))[0]

    def _dest(self, eng):
        """Where a ``BatchSampler``'s draw writes what ``set_inputs`` would: the clips for both halves, the labels' one-hot
        rows into the condition columns of every frame."""
        d = eng.dec
        dest = dict(audio=eng.enc.x, audio2=d.audio)
        if self.condition_size > 0:
            dest.update(onehot=d.cond_in, onehot_rows=d.frames, onehot_col0=self.latent_channels)
        return dest

    def evaluate(self, sampler):
        """The forward-only loss of every step of one sweep over the sampler's dataset, float32 [len(dataset) /
        (batch_size * world)] in the steps' order; with condition_size > 0 the labels' one-hot rows are the conditions.
        The mixture-of-logistics loss kernel gives one number per batch, so `sampler` is a plain ``dataset.sampler(...,
        shuffle=False)`` whose batches divide the set.  Per-sample held-out likelihoods of any clip exist already: the
        streaming scorer (``scorer()``).  No parameter changes."""
        steps = _loss_sweep_steps(sampler, "WaveNetAutoEncoder")
        if self.condition_size > 0:
            _fit_labels(sampler, self.condition_size, "WaveNetAutoEncoder", "conditions")      # (it says ".fit:")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        return _evaluate_losses(eng, sampler, self._dest(eng), steps)[0]

    def encode(self, inputs, conditions=None):
        eng = self._stage(inputs, conditions)
        return eng.encode().view(eng.B, -1, self.latent_channels).cpu().numpy()

    def encoder(self, max_batch=1, max_frames=32):
        """An ``AudioEncoder`` with this model's hyper-parameters and a COPY of its current encoder parameters (a
        snapshot: call it again after more training).  It takes any batch <= max_batch and any length."""
        eng = self._control_engine()
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
        eng = self._control_engine()
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
        return _flow_variables(self._name, self._control_engine().flows)

    def synthesizer(self, max_batch=1, max_chunk=1600, max_frames=None):
        """A ``StudentSynthesizer`` with this model's hyper-parameters and a COPY of its current flow parameters (a
        snapshot: call it again after more training).  max_frames defaults to input_size // pool_stride."""
        flows = self._control_engine().flows
        syn = StudentSynthesizer(self.dilations, self.num_flows, filter_width=self.filter_width,
                                 dilation_channels=self.dilation_channels, latent_channels=self.latent_channels,
                                 condition_size=self.condition_size, pool_stride=self.pool_stride, name=self._name,
                                 dtype=self._flow_cfg.dtype, max_batch=max_batch, max_chunk=max_chunk,
                                 max_frames=max_frames or max(1, self.input_size // self.pool_stride))
        for w, f in zip(syn._eng.weights, flows):
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
        for w, f in zip(inv._eng.weights, self._control_engine().flows):
            w.params.copy_(f.params)
            w.repack()
        inv._eng.repack()
        return inv

    # --- checkpointing (model.py:540-567) ---------------------------------------------------------------
    def load(self, sess, logdir):
        if self._teacher_dir is not None and self._teacher is not None:
            self._teacher.load(self._teacher_dir)                                         # model.py:543-544
        return super().load(logdir)

    def _after_load(self):
        self._primary.ctl.reset_ema(self._primary.storage.params)
        for f in self._primary.flows:
            f.repack()

    def save(self, sess, logdir, global_step, force=False, fmt=None):
        return super().save(logdir, global_step, force, fmt)

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
        are in the sampler's ring (``sampler.entropies``).  See ``training._fit``."""
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
        return _fit(eng, sampler, steps, *self._dest(eng, sampler))

    def _dest(self, eng, sampler):
        """(where a ``DistillSampler``'s draw writes what ``set_inputs`` would, the step's `between`: the teacher's encoding
        of the clips just drawn, into the latent columns of every conditioning input)."""
        enc, tch = self._teacher._engine(eng.B, eng.T).enc, eng.teacher
        tables = [tch.cond_in] + [f.cond_in for f in eng.flows]
        dest = dict(audio=enc.x, audio2=eng.truth, audio3=tch.audio, noise=eng.noise)
        if self.condition_size > 0:
            dest.update(tables=tables, rows=tch.frames, col0=self.latent_channels)

        def between():
            enc.forward()
            sampler.scatter(enc.enc, tables)
        return dest, between

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
            _fit_labels(sampler, self.condition_size, "ParallelWaveNet", "conditions", "evaluate")
        eng = self._engine(sampler.batch_size, sampler.num_samples)
        dest, between = self._dest(eng, sampler)
        return _evaluate_losses(eng, sampler, dest, steps, between, lambda first, count: (
            sampler.losses(first, count), sampler.power_losses(first, count), sampler.entropies(first, count)))

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
        labelled set of recordings.  Returns (loss [steps], distance [steps, P]), float32.  See ``training._fit``.

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
        if validate is not None:
            es, every = _check_validate(validate, EmbedSampler, "a dataset.EmbedSampler (dataset.embed_sampler(...))")
            self._check_embed(es)
        eng = self._engine(2 * sampler.pairs, sampler.num_samples)
        dest = dict(audio=eng.audio, labels=eng.labels)
        if validate is None:
            return _fit(eng, sampler, steps, dest)
        eng_v = self._engine(es.batch_size, es.num_samples)
        (loss, dist), results = _fit_validated(eng, sampler, steps, dest, es, every, lambda: self._embed_sweep(eng_v, es),
                                               self._validate_ema())
        return loss, dist, results

    def _check_embed(self, es):
        """An ``EmbedSampler`` this model can sweep; binds it to the embedding's width and, without a d_max of its own, to
        a histogram range of twice the margin (beyond the margin a pair of two labels costs nothing)."""
        from .dataset import EmbedSampler
        if not isinstance(es, EmbedSampler):
            raise TypeError("SiameseWaveNet.evaluate takes a dataset.EmbedSampler (dataset.embed_sampler(...)), got %s"
                            % type(es).__name__)
        _refuse_augment(es, "SiameseWaveNet")
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
        return StreamingEmbedder(EmbedderWeights.from_engine(self._control_engine()), max_batch=max_batch, hop=hop,
                                 window=window, max_hops=max_hops, max_gallery=max_gallery)
