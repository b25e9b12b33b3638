"""Training/inference engine for the WaveNet residual stack on one MI355X (one process per GPU).

Mirrors the graph bodies of the reference's model classes -- ``WaveNet.createNetwork``
(model.py:33-62) and ``WaveNetAutoEncoder.createDecoder`` (model.py:158-200) -- as a fixed
sequence of libsrwn.so kernel launches over pre-allocated HBM buffers:

  forward   input conv -> L x fused residual layer (h, z saved) -> skip sum as ONE K = L*R
            contraction over the saved z -> relu -> 1x1 -> relu -> last 1x1 + softmax-CE (fused)
  backward  head data gradients -> L x fused layer data gradient (top down) -> batched weight
            gradients (time-contraction MFMA GEMMs + deterministic slab reduction)
  update    [RCCL all-reduce of the flat fp32 gradient buffer] -> TF-Adam -> re-pack bf16 weights

HBM layout (channels-last, compute dtype): xs [L+1,B,T,R] layer inputs, zs [L,B,T,R] tanh
outputs, dfs [L,B,T,R], gs [L+1,B,T,R] residual-stream gradients (gs[L] stays zero), r0/r1/da1/
dtotal [B*T,S], dlogits [B*T,Cp].  Parameters, gradients and Adam moments are single flat fp32
buffers laid out struct-of-arrays across layers so every batched kernel sees a constant stride.
"""
from __future__ import annotations

import ctypes
import math
import os as _os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dp
from . import kernels as K
from . import packing as P
from .slots import SlotTable, per_stream

SQRT_HALF = 0.7071067811865476


@dataclass
class StackConfig:
    dilations: Sequence[int]
    filter_width: int = 2
    dilation_channels: int = 32   # R
    skip_channels: int = 256      # S
    output_channels: int = 256    # C (softmax classes / head width)
    cond_channels: int = 0        # channels of encoding_w_condition (model.py:161-167); 0 = no conditioning
    pool_stride: int = 1
    shift_input: bool = False     # RightShift(truth) teacher forcing (model.py:172)
    head_mode: str = "per_timestep"  # "per_timestep": mu-law softmax CE per sample (model.py:100-112);
    #                                  "pooled": class WaveNet's clip-level softmax (model.py:56-60, 24-29);
    #                                  "mol": discretised mixture of logistics, the live teacher's loss
    #                                         (model.py:114,196; ops.py:124-175): output_channels = 4*mixtures,
    #                                         loss SUMMED over batch and time
    #                                  "flow": no skip path, head relu -> 1x1 R->2 + affine transform: one flow of
    #                                         ParallelWaveNet (model.py:415-487), see student.FlowStack
    #                                  "contrastive": class SiameseWaveNet's twin towers (model.py:660-797) as ONE
    #                                         batch of B = 2P clips (left rows, then right): time-mean -> last 1x1 =
    #                                         embedding [B, output_channels], contrastive loss over the P pairs
    dtype: torch.dtype = torch.bfloat16
    learning_rate: float = 1e-3
    margin: float = 5.0           # contrastive head: the margin m of the loss (model.py:660, 747-749)
    gate_mode: str = "reference"  # "reference": c = z*sigmoid(z), the graph the reference runs (ops.py:33 discards the gate
    #                               conv); "wavenet": the canonical c = tanh(Wf*x + bf) * sigmoid(Wg*x + bg), trained with
    #                               one launch per layer (csrc/srwn_wngate.hip); the `_gate` variables are then trained too


class Section:
    __slots__ = ("name", "offset", "shape", "numel")

    def __init__(self, name, offset, shape):
        self.name, self.offset, self.shape = name, offset, tuple(shape)
        self.numel = int(np.prod(shape))


class OptControls:
    """The device side of ``optim.TrainControls`` for one flat parameter buffer, shared by every engine that shares the
    buffer (``share_from``): the control table float32 [capacity, 2] = {lr, ema_decay} and its length int32 [1] that
    ``srwn_adam_step_ctl`` reads, the EMA shadow (flat fp32 like ``params``) with the scratch buffer of its swap, the
    partials of the gradient norm and ``clip`` float32 [2] = {last clip factor, last norm}.  ``controls is None``: no
    controls, the optimizer runs the launches it ran before there were any."""

    def __init__(self):
        import weakref
        self.controls = None
        self.table = self.length = self.ema = self.scratch = self.sq_parts = self.clip = None
        self.swapped = False
        self.engines = weakref.WeakSet()      # whose captured graphs hold the launch list these controls decide

    def set(self, controls, params: torch.Tensor) -> bool:
        """Installs `controls` (or None).  The same features and bound within the allocated table: the table and its length are
        rewritten in place, captured graphs follow them, returns False.  Anything else re-allocates and returns True:
        the launch list has changed.  The shadow is set to the parameters when the EMA is switched on and kept while it
        stays on."""
        if self.swapped:
            raise RuntimeError("set_controls inside ema_weights(): the parameters and the EMA shadow are swapped")
        old = self.controls
        if controls is None:
            self.controls = None
            self.table = self.length = self.ema = self.scratch = self.sq_parts = self.clip = None
            return old is not None
        tab = torch.from_numpy(controls.table())
        if old is not None and old.features == controls.features and old.clip_norm == controls.clip_norm and \
                controls.horizon <= self.table.shape[0]:      # (clip_norm is a host scalar of srwn_clip_scale)
            self.table[:controls.horizon].copy_(tab)
            self.length.fill_(controls.horizon)
            self.controls = controls
            return False
        dev = params.device
        self.table, self.length = tab.to(dev), torch.full((1,), controls.horizon, dtype=torch.int32, device=dev)
        clip, ema = controls.features
        self.clip = torch.zeros(2, dtype=torch.float32, device=dev) if clip else None
        self.sq_parts = torch.zeros(K.sumsq_partials(params.numel()), dtype=torch.float32, device=dev) if clip else None
        if ema and self.ema is None:
            self.ema, self.scratch = params.clone(), torch.empty_like(params)
        elif not ema:
            self.ema = self.scratch = None
        self.controls = controls
        return True

    def reset_ema(self, params: torch.Tensor):
        """The shadow follows parameters that were set from outside (load, init_parameters)."""
        if self.ema is not None:
            if self.swapped:
                raise RuntimeError("the parameters were replaced inside ema_weights()")
            self.ema.copy_(params)

    def drop_graphs(self):
        for e in list(self.engines):
            e._graph_ready, e._fit_state = False, None


def adam_update(ctl: OptControls, params, grads, m, v, step, lr: float, grad_scale: float = 1.0, scale_dev=None):
    """The one update launch every optimizer of the package goes through.  No controls: srwn_adam_step at the fixed rate
    `lr` (srwn_adam_step_scaled where the gradient scale `scale_dev` is on the device), the launches from before there
    were controls.  Controls: srwn_adam_step_ctl -- the step's learning rate and EMA decay from the device table, the
    gradient scale ``grad_scale * scale_dev[0]``, the EMA shadow in the same pass."""
    if ctl.controls is None:
        if scale_dev is None:
            K.adam_step(params, grads, m, v, step, lr, grad_scale=grad_scale)
        else:
            K.adam_step_scaled(params, grads, m, v, step, lr, scale_dev, True)
        return
    if ctl.swapped:
        raise RuntimeError("optimizer_step inside ema_weights(): the parameters and the EMA shadow are swapped")
    K.adam_step_ctl(params, grads, m, v, step, ctl.table, ctl.length, ema=ctl.ema, scale_dev=scale_dev, tick=True,
                    grad_scale=grad_scale)


def swap_with_ema(ctl: OptControls, params):
    """Exchanges the CONTENTS of `params` and the shadow through the scratch buffer: three copies on the current stream."""
    if ctl.ema is None:
        raise ValueError("swap_ema: no EMA weights (set_controls with an ema_decay)")
    ctl.scratch.copy_(params)
    params.copy_(ctl.ema)
    ctl.ema.copy_(ctl.scratch)
    ctl.swapped = not ctl.swapped


def _os_environ_flag(name: str, default: bool) -> bool:
    import os
    return os.environ.get(name, "1" if default else "0") != "0"


class _Span:
    """Optional HIP-event bracket around a group of launches on the current stream (bench.py roofline)."""

    def __init__(self, eng, name):
        self.eng, self.name = eng, name

    def __enter__(self):
        if self.eng.timing or self.eng.timing_overlap:
            self.s = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if self.eng.timing or self.eng.timing_overlap:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.eng.spans.setdefault(self.name, []).append((self.s, e))
        return False


class GenerationState:
    """One resumable generation run (WaveNetEngine.generation_state): the per-layer rings of the queue-cached generator,
    the carry [B, 2] fp32 = (a[t-1], a[t-2]) the next step's input conv reads, the absolute step t of the next sample, the
    seed of the samplers' counters, and for a conditioned decoder the encoding `cond`, its per-layer conditioning
    `cond_all` [B*frames, L*R] and `limit` = frames * pool_stride (the last step it covers).  `sampling`: the run's
    sampling controls as a device array of SrwnGenSampling [B] (None: every utterance at the defaults)."""

    def __init__(self, batch, ring, carry, seed, cond=None, cond_all=None, frames=0, limit=None, sampling=None):
        self.batch, self.ring, self.carry, self.seed = int(batch), ring, carry, int(seed)
        self.cond, self.cond_all, self.frames, self.limit = cond, cond_all, int(frames), limit
        self.sampling = sampling
        self.t = 0

    live = False      # (LiveGenerationState: the conditioning table is a ring that `feed` fills while the run goes on)


class LiveGenerationState(GenerationState):
    """A generation run whose encoding arrives while it runs (WaveNetEngine.live_generation_state / feed): `cond_all`
    [B * max_frames, L*R] is a RING -- frame q of a stream in row q mod max_frames -- `fed` the frames written so far and
    `limit` = fed * pool_stride.  `cond` keeps the raw frames fed while t == 0 (what `prime` runs its forward pass on) and
    is dropped at the first step.  `stage_in` / `stage_out`: the feed's projection operands, [B * max_frames, Ep] (its
    padding columns stay zero) and [B * max_frames, L*R]."""

    live = True

    def __init__(self, batch, ring, carry, seed, cond_all, max_frames, sampling=None, stage_in=None, stage_out=None):
        super().__init__(batch, ring, carry, seed, None, cond_all, max_frames, 0, sampling)
        self.max_frames, self.fed = int(max_frames), 0
        self.stage_in, self.stage_out = stage_in, stage_out


def live_decode_room(max_frames: int, fed: int, t: int, pool_stride: int) -> int:
    """How many frames a live DECODER run may be fed now: max_frames - fed + t // pool_stride.  Its conditioning table is
    a ring of ``max_frames`` frames (frame q in row q mod max_frames) and step t reads the row of its own frame t //
    pool_stride only -- the layer rings carry everything older -- so every frame before the current one may be
    overwritten: unlike ``student.live_room`` there is no history term.  Pure Python."""
    max_frames, fed, t, pool_stride = int(max_frames), int(fed), int(t), int(pool_stride)
    if max_frames < 1 or fed < 0 or t < 0 or pool_stride < 1 or t > fed * pool_stride:
        raise ValueError("live_decode_room: max_frames=%d fed=%d t=%d pool_stride=%d" % (max_frames, fed, t, pool_stride))
    return max_frames - fed + t // pool_stride


def live_slot_shift(clock: int, stopped_at: int) -> int:
    """By how many positions the layer-ring columns of a pool slot are rotated before it runs again: clock - stopped_at,
    where ``stopped_at`` is the pool clock at which the slot's last own step ended (a join: the join's clock) and
    ``clock`` the one at which its next own step runs.  The rings follow the pool's clock -- step c of a layer of dilation
    d writes position c mod (d + 1) and reads the delayed tap at (c + 1) mod (d + 1) -- and a slot that waits for frames
    stores nothing meanwhile, so what it would have read at ``stopped_at`` must sit where ``clock`` reads:
    new[(p + shift) mod (d + 1)] = old[p] (srwn_generate_ring_rotate_slots).  0: the slot never paused.  Pure Python."""
    clock, stopped_at = int(clock), int(stopped_at)
    if stopped_at < 0 or clock < stopped_at or clock > INT32_MAX:
        raise ValueError("live_slot_shift: clock=%d stopped_at=%d" % (clock, stopped_at))
    return clock - stopped_at


def sampling_table(n, temperature, top_k, top_p, C, mol, who="generate"):
    """The sampling controls of n streams as srwn.h's SrwnGenSampling rows (a NumPy structured array [n]), or None when
    every stream is at the defaults (temperature 1, top_k 0, top_p 1: the calls without controls).  Each argument is a
    scalar, a sequence of n, or None (the default).  Ranges: temperature finite and > 0 (as float32), top_k 0 (off) or
    1..C, 0 < top_p <= 1; a mixture-of-logistics head (`mol`) takes the temperature only.  ValueError otherwise, naming
    the argument and the value.  No device work."""
    from . import _lib
    n = int(n)
    taus, ks, ps = (per_stream(x, n, name, who, default)
                    for x, name, default in ((temperature, "temperature", 1.0), (top_k, "top_k", 0), (top_p, "top_p", 1.0)))
    tab = np.zeros(n, dtype=np.dtype(_lib.SrwnGenSampling))
    for i, (t, k, p) in enumerate(zip(taus, ks, ps)):
        try:
            t32, p32 = np.float32(t), np.float32(p)
        except (TypeError, ValueError):
            raise ValueError("%s: temperature %r / top_p %r are not numbers" % (who, t, p))
        if not (np.isfinite(t32) and t32 > 0):
            raise ValueError("%s: temperature %r: finite and > 0" % (who, t))
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError("%s: top_k %r: an integer, 0 (off) or 1..%d" % (who, k, C))
        if mol and int(k) != 0:
            raise ValueError("%s: top_k %r: the mixture-of-logistics head takes temperature only" % (who, k))
        if mol and not p32 == 1:
            raise ValueError("%s: top_p %r: the mixture-of-logistics head takes temperature only" % (who, p))
        if not 0 <= int(k) <= C:
            raise ValueError("%s: top_k %r: 0 (off) or 1..%d classes" % (who, k, C))
        if not (p32 > 0 and p32 <= 1):
            raise ValueError("%s: top_p %r: 0 < top_p <= 1" % (who, p))
        tab[i] = (t32, p32, int(k), 0)
    if np.all(tab["temperature"] == 1) and np.all(tab["top_p"] == 1) and np.all(tab["top_k"] == 0):
        return None
    return tab


def _sampling_to_device(tab, dev):
    """A SrwnGenSampling table as the device array the *_sampled entry points read ([n, 4] 32-bit words)."""
    return torch.from_numpy(tab.view(np.int32).reshape(len(tab), 4).copy()).to(dev)


INT32_MAX = 2 ** 31 - 1   # the generation kernels' steps, clock and limits are int32: 2^31 steps is about 37 h at 16 kHz


def _pow2_at_least(n: int) -> int:
    return 1 << max(0, int(n) - 1).bit_length()


class GenerationPool(SlotTable):
    """A fixed-capacity generation pool (WaveNetEngine.generation_pool): `capacity` slots over ONE set of layer rings, each
    slot holding its own stream at its own step.  Streams `join` free slots (from prompts of any lengths and, for a
    conditioned decoder, with their own encodings), `step` runs every live slot with one launch per chunk, and a stream
    that reaches its end or `leave`s frees its slot for the next one.  The rings follow the pool's clock; what depends on
    a stream's own position -- the samplers' counters, the conditioning frame, whether it still emits -- comes from the
    per-slot table (srwn.h, SrwnGenSlot), so a slot produces the bits of a batch-of-one run with its seed.
    Joins are ordered between steps.  Steps, clock and limits are int32 (2^31 steps is about 37 h at 16 kHz).
    A LIVE pool (``generation_pool(..., live=True)``, the conditioned mixture-of-logistics decoder): `frames` is the length
    of every slot's conditioning RING, and ``join(..., live=True)`` starts streams that are fed while they run (``feed`` /
    ``room`` / ``close``).  A live slot that has used up its frames is starved, not ended: it stays taken with ran = 0, its
    columns store nothing into the layer rings, and before the launch in which it runs again they are rotated by the
    clock ticks it missed (``live_slot_shift``)."""

    live = False      # (a pool made with live=True: the live slot form's launches, per-slot feed state)

    def __init__(self, eng: "WaveNetEngine", capacity: int, frames: int = 0, live: bool = False):
        self.eng, self.capacity, self.frames = eng, int(capacity), int(frames)
        self.live = bool(live)
        self._live = np.zeros(self.capacity, bool)           # live slots: fed while they run; t_end = fed * pool_stride
        self._closed = np.zeros(self.capacity, bool)         # ... until closed: no more frames will come
        self._fed = np.zeros(self.capacity, np.int64)
        self._cap = np.full(self.capacity, INT32_MAX, np.int64)      # ... capped by prompt + max_samples
        self._stopped = np.zeros(self.capacity, np.int64)    # the clock at which each slot's last own step ended
        self.conditioned = bool(eng.mol and eng.E)
        self.E, self.pool_stride = int(eng.E), int(eng.cfg.pool_stride)
        self.clock = 0
        self._t = np.zeros(self.capacity, np.int64)          # host mirror of the device table (the kernel advances both alike)
        self._end = np.zeros(self.capacity, np.int64)
        self._seed = [0] * self.capacity
        self._active = np.zeros(self.capacity, bool)
        self._view = None
        eng._repack_generation()
        self.ring = eng._gen_ring(self.capacity)
        self.carry = torch.zeros((self.capacity, 2), dtype=torch.float32, device=eng.dev)
        self.slots = torch.zeros((self.capacity, 4), dtype=torch.int32, device=eng.dev)   # [t, t_end, seed lo, seed hi]
        self.C, self.mol = int(eng.C), bool(eng.mol)
        self._samp = None        # the slots' sampling controls (host SrwnGenSampling [capacity]) once a join brought some
        self.sampling = None     # ... and the device array the *_slots_sampled launches read
        self.cond_all = None
        if self.conditioned:
            self.cond_all = torch.zeros((self.capacity * self.frames, eng.L * eng.R), dtype=eng.dt, device=eng.dev)

    # ---- inspection
    @property
    def t(self) -> np.ndarray:
        """Each slot's own step of its next sample."""
        return self._t.copy()

    def _upload(self):
        from . import _lib
        tab = np.zeros(self.capacity, dtype=np.dtype(_lib.SrwnGenSlot))      # (srwn.h's layout, 16 bytes a slot)
        tab["t"], tab["t_end"], tab["seed"] = self._t, self._end, np.array(self._seed, dtype=np.uint64)
        self.slots.copy_(torch.from_numpy(tab.view(np.int32).reshape(self.capacity, 4)))
        if getattr(self, "_samp", None) is not None:
            if self.sampling is None:
                self.sampling = torch.zeros((self.capacity, 4), dtype=torch.int32, device=self.eng.dev)
            self.sampling.copy_(torch.from_numpy(self._samp.view(np.int32).reshape(self.capacity, 4)))

    def _check_join(self, seeds, prompts, cond, max_samples, slots, temperature=None, top_k=None, top_p=None, live=False):
        """Everything join refuses, before any device work: returns (seeds, prompts as float32 1-D arrays, the chosen
        slots, t_end per stream, the streams' sampling controls or None).  live: a stream brings 0..frames first frames
        (an entry None: none yet)."""
        if live and not self.live:
            raise ValueError("join: live streams need a pool made with generation_pool(..., live=True)")
        seeds = [int(s) for s in seeds]
        n = len(seeds)
        if n < 1:
            raise ValueError("join: no streams")
        if any(s < 0 or s >= 2 ** 64 for s in seeds):
            raise ValueError("join: seeds are unsigned 64-bit")
        samp = None
        if temperature is not None or top_k is not None or top_p is not None:
            samp = sampling_table(n, temperature, top_k, top_p, self.C, self.mol, "join")
        ps = []
        for p in per_stream(prompts, n, "prompts"):
            if p is None:
                ps.append(np.zeros(0, np.float32))
                continue
            p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
            if p.ndim != 1:
                raise ValueError("join: each prompt is 1-D [P], got shape %s" % (p.shape,))
            ps.append(p.astype(np.float32))
        mx = per_stream(max_samples, n, "max_samples")
        limits = [INT32_MAX] * n
        if self.conditioned:
            if cond is None:
                raise ValueError("this decoder is conditioned: pass cond, one [frames, %d] per stream" % self.E)
            cond = per_stream(list(cond), n, "encodings")
            if live:
                cond = [np.zeros((0, self.E), np.float32) if c is None else c for c in cond]
            for i, c in enumerate(cond):
                shp = tuple(c.shape) if hasattr(c, "shape") else np.shape(c)
                if len(shp) != 2 or shp[1] != self.E or not (0 if live else 1) <= shp[0] <= self.frames:
                    raise ValueError("join: cond %d must be [%d..%d frames, %d], got %s"
                                     % (i, 0 if live else 1, self.frames, self.E, shp))
                limits[i] = shp[0] * self.pool_stride
        elif cond is not None:
            raise ValueError("this decoder is not conditioned")
        slots = self._take_slots(n, slots)
        ends = []
        for p, m, lim in zip(ps, mx, limits):
            if len(p) > lim:
                raise ValueError("join: prompt of %d samples exceeds frames * pool_stride = %d" % (len(p), lim))
            if m is not None and int(m) < 0:
                raise ValueError("join: max_samples %d" % int(m))
            ends.append(min(lim, INT32_MAX if m is None else len(p) + int(m)))
        return seeds, ps, cond, slots, ends, samp

    def _prime_view(self, n: int, T: int) -> "WaveNetEngine":
        """The forward-only view the joins' prompt passes run in, its shape rounded up (powers of two; whole conditioning
        frames) so that it is reused across joins rather than built per join."""
        pool = self.pool_stride if self.eng.E else 1
        B, Tp = _pow2_at_least(n), _pow2_at_least(T)
        Tp = -(-Tp // pool) * pool
        if self._view is None or (self._view.B, self._view.T) != (B, Tp):
            self._view = None
            self._view = WaveNetEngine(self.eng.cfg, B, Tp, self.eng.dev, share_from=self.eng, frozen=True)
        return self._view

    def join(self, seeds, prompts=None, cond=None, max_samples=None, slots=None, *, temperature=None, top_k=None,
             top_p=None, live=False) -> List[int]:
        """n streams into free slots (the lowest ones, or `slots`): seeds [n]; prompts None or n entries of 1-D [P_i] (any
        lengths, none included); cond (conditioned decoder) n encodings [frames_i <= frames, cond_channels]; max_samples
        None, one int, or n entries: samples after the prompt (a conditioned stream ends at frames_i * pool_stride too).
        temperature / top_k / top_p: the streams' sampling controls (sampling_table: a scalar or one entry per stream; None
        = the default), written into their slots' entries of the pool's SrwnGenSampling array as the carry is.
        One stack-only forward over all prompts (padded to the longest) and one srwn_generate_ring_fill_slots; returns the
        slots.
        live=True (a live pool): the streams are fed while they run (``feed``): cond[i] holds a stream's first frames
        [k_i >= 0, cond_channels] (None: none yet), a prompt fits inside them (len <= k_i * pool_stride), and the stream
        ends where ``close`` finds it or at prompt + max_samples; until then a slot that has used up its frames waits."""
        from . import _lib
        seeds, ps, cond, slots, ends, samp = self._check_join(seeds, prompts, cond, max_samples, slots, temperature, top_k,
                                                              top_p, live)
        eng, n, dev = self.eng, len(seeds), self.eng.dev
        lens = [len(p) for p in ps]
        dst = torch.tensor(slots, dtype=torch.int32, device=dev)
        plen = torch.tensor(lens, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        if self.conditioned:
            LR, F = eng.L * eng.R, self.frames
            enc = torch.zeros((n, F, self.E), dtype=torch.float32, device=dev)      # (frames a stream lacks: zero rows)
            for i, c in enumerate(cond):
                c = torch.as_tensor(c).to(device=dev, dtype=torch.float32)
                enc[i, :c.shape[0]].copy_(c)
            self.cond_all.view(self.capacity, F, LR)[dst.long()] = eng._project_cond(enc.view(n * F, self.E)).view(n, F, LR)
        P = max(lens)
        xs, stride, T_src = None, 0, 0
        if P > 0:
            view = self._prime_view(n, P)
            audio = torch.zeros((view.B, view.T), dtype=torch.float32, device=dev)
            for i, p in enumerate(ps):
                if len(p):
                    audio[i, :len(p)].copy_(torch.from_numpy(p))
            vc = None
            if eng.E:
                fv = view.T // self.pool_stride
                vc = torch.zeros((view.B, fv, self.E), dtype=torch.float32, device=dev)
                for i, c in enumerate(cond):
                    c = torch.as_tensor(c).to(device=dev, dtype=torch.float32)[:fv]
                    vc[i, :c.shape[0]].copy_(c)
            view.set_inputs(audio, None, vc)
            view.forward(want_logits=False, with_loss=False, train=False, stack_only=True)
            xs, stride, T_src = view.xs.data_ptr(), view.B * view.T * eng.R, view.T
        _lib.call("srwn_generate_ring_fill_slots", xs, stride, T_src, n, dst.data_ptr(), plen.data_ptr(), self.clock,
                  eng._gen_dilations(), eng.L, self.capacity, eng.R, self.ring.data_ptr(), K.abi_dtype(eng.dt), st)
        carry = np.zeros((n, 2), np.float32)
        for i, p in enumerate(ps):
            carry[i, :min(2, len(p))] = p[::-1][:2]
        self.carry[dst.long()] = torch.from_numpy(carry).to(dev)
        for i, u in enumerate(slots):
            self._t[u], self._end[u], self._seed[u] = lens[i], ends[i], seeds[i]
            self._active[u] = True
        if self.live:
            mx = per_stream(max_samples, n, "max_samples")
            for i, u in enumerate(slots):
                self._live[u], self._closed[u], self._stopped[u] = live, False, self.clock
                self._fed[u] = int(np.shape(cond[i])[0]) if live else 0
                self._cap[u] = INT32_MAX if mx[i] is None else lens[i] + int(mx[i])
        if samp is not None and self._samp is None:
            self._samp = np.zeros(self.capacity, dtype=np.dtype(_lib.SrwnGenSampling))
            self._samp["temperature"], self._samp["top_p"] = 1.0, 1.0
        if self._samp is not None:      # (a join without controls puts its slots back at the defaults)
            for i, u in enumerate(slots):
                self._samp[u] = samp[i] if samp is not None else (1.0, 1.0, 0, 0)
        self._upload()
        return list(slots)

    def leave(self, slots) -> None:
        """Ends the streams in `slots` (a slot already free stays free) and frees their slots."""
        for u in self._slot_list(slots, "leave"):
            self._active[u] = False
            self._end[u] = self._t[u]
            if self.live:
                self._live[u] = False
        self._upload()

    @property
    def any_runnable(self) -> bool:
        """Whether a step would make a sample now: some slot is before its end (a starved live slot is not)."""
        return bool((self._t < self._end).any())

    # ---- live slots
    def _open_live(self, u: int) -> bool:
        return bool(self.live and self._active[u] and self._live[u] and not self._closed[u])

    def room(self, slot: int) -> int:
        """Frames a live slot may be fed now (``live_decode_room`` of its own fed and t); 0 for every other slot."""
        u, = self._slot_list(slot, "room")
        if not self._open_live(u):
            return 0
        return live_decode_room(self.frames, int(self._fed[u]), int(self._t[u]), self.pool_stride)

    def _check_feed(self, slots, frames):
        """Everything feed refuses, before any device work: (slots, frames as tensors [k_i, E])."""
        slots = self._slot_list(slots, "feed")
        if isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 2:
            frames = [frames]
        frames = [f if isinstance(f, torch.Tensor) else torch.as_tensor(np.asarray(f, dtype=np.float32)) for f in frames]
        if len(frames) != len(slots) or len(set(slots)) != len(slots):
            raise ValueError("feed: %d distinct slots need one [k, %d] each, got %d" % (len(slots), self.E, len(frames)))
        for u, f in zip(slots, frames):
            if not self._open_live(u):
                raise ValueError("feed: slot %d holds no live, open stream" % u)
            if f.dim() != 2 or f.shape[1] != self.E:
                raise ValueError("feed: frames of slot %d must be [k, %d], got %s" % (u, self.E, tuple(f.shape)))
            if f.shape[0] > self.room(u):
                raise ValueError("feed: %d frames for slot %d, but its ring of %d has room for %d at t = %d with %d fed"
                                 % (f.shape[0], u, self.frames, self.room(u), self._t[u], self._fed[u]))
        return slots, frames

    def feed(self, slots, frames) -> None:
        """The next frames of live slots: frames[i] [k_i, cond_channels] for slots[i], NumPy or device tensors (device
        tensors are taken as they are).  Refuses (ValueError, before any device work, nothing changed) k_i > ``room``, a
        slot that holds no live, open stream, and lists of different lengths.  The rows are ``_project_cond``'s -- the same
        srwn_pw_linear over the same image, so the bits of the one-shot table -- scattered into the slots' rings by ONE
        srwn_cond_ring_scatter_slots however many slots and frames; each slot's t_end grows to fed * pool_stride on the
        host mirror and the device table together."""
        from . import _lib
        slots, frames = self._check_feed(slots, frames)
        pairs = [(u, f) for u, f in zip(slots, frames) if f.shape[0] > 0]
        if not pairs:
            return
        eng, F = self.eng, self.frames
        rows = torch.cat([f.to(device=eng.dev, dtype=torch.float32) for _, f in pairs], dim=0)
        dst = np.concatenate([u * F + (int(self._fed[u]) + np.arange(f.shape[0])) % F for u, f in pairs]).astype(np.int32)
        LR = eng.L * eng.R
        out = eng._project_cond(rows)
        dst_dev = torch.from_numpy(dst).to(eng.dev)
        _lib.call("srwn_cond_ring_scatter_slots", out.data_ptr(), LR, self.cond_all.data_ptr(), LR, int(rows.shape[0]),
                  dst_dev.data_ptr(), self.capacity * F, LR, K.abi_dtype(eng.dt), torch.cuda.current_stream().cuda_stream)
        for u, f in pairs:
            self._fed[u] += int(f.shape[0])
            self._end[u] = min(int(self._fed[u]) * self.pool_stride, int(self._cap[u]))
        self._upload()

    def close(self, slots) -> None:
        """No more frames will come for the live streams in `slots`: each frees its slot at the end of what it was fed,
        like a bounded stream (at once when it is already there)."""
        for u in self._slot_list(slots, "close"):
            if self.live and self._active[u] and self._live[u]:
                self._closed[u] = True
                self._active[u] = self._t[u] < self._end[u]

    def step(self, nsteps: int, mode: str = "sample", forced: Optional[torch.Tensor] = None, want_logits: bool = False):
        """One launch of `nsteps` pool steps: (audio [capacity, nsteps] f32, codes [capacity, nsteps] i32, logits
        [capacity, nsteps, C] f32 or None, ran [capacity] int64 numpy).  Slot u's samples are row u's first ran[u]
        entries; the rest of every row stays zero.  `forced` [capacity, nsteps]: teacher forcing for this launch (every
        slot).  Slots whose stream reached its end become free."""
        eng, nsteps = self.eng, int(nsteps)
        if nsteps < 0:
            raise ValueError("step: nsteps %d" % nsteps)
        if self.clock + nsteps > INT32_MAX:
            raise ValueError("step: the pool's clock %d + %d steps passes int32" % (self.clock, nsteps))
        audio, codes, logits, forced = eng._gen_outputs(self.capacity, nsteps, want_logits, forced, "capacity")
        ran = np.clip(self._end - self._t, 0, nsteps)
        if nsteps == 0:
            return audio, codes, logits, ran
        if self.live:
            self._realign(ran)
        eng._launch_generation(self.ring, audio, codes, logits, forced, self.capacity, nsteps, mode, 0, self.clock,
                               self.carry, self.sampling, self.cond_all, self.frames, self.slots, live=self.live)
        self._t += ran
        if self.live:
            self._stopped[ran > 0] = self.clock + ran[ran > 0]
        self.clock += nsteps
        if self.live:      # (a starved live slot stays taken until it is closed, left or at prompt + max_samples)
            self._active &= (self._t < self._end) | (self._live & ~self._closed & (self._t < self._cap))
        else:
            self._active &= self._t < self._end
        return audio, codes, logits, ran

    def _realign(self, ran) -> None:
        """Before a launch of a live pool: every slot that will run and whose last own step did not end at this clock has
        the columns of its layer rings rotated by ``live_slot_shift``, all of them in one srwn_generate_ring_rotate_slots."""
        eng = self.eng
        us = [int(u) for u in np.flatnonzero(ran > 0)]
        sh = [live_slot_shift(self.clock, self._stopped[u]) for u in us]
        lag = [(u, s) for u, s in zip(us, sh) if s != 0]
        if not lag:
            return
        tab = torch.tensor(lag, dtype=torch.int32).t().contiguous().to(eng.dev)      # [2, n]: the slots, their shifts
        K.ring_rotate_slots(self.ring, eng._gen_dilations(), eng.L, self.capacity, eng.R, tab[0], tab[1])


CONTRASTIVE_LDS_FLOATS = 65536 // 4   # srwn_contrastive_head: rows*D + 2P floats in one workgroup (csrc/srwn_siamese.hip)


class WaveNetEngine:
    def __init__(self, cfg: StackConfig, batch: int, length: int, device="cuda", seed: int = 0,
                 process_group=None, share_from: Optional["WaveNetEngine"] = None, frozen: bool = False):
        if cfg.gate_mode not in ("reference", "wavenet"):
            raise ValueError("gate_mode %r: 'reference' or 'wavenet'" % (cfg.gate_mode,))
        if cfg.gate_mode == "wavenet" and cfg.head_mode == "flow":
            raise NotImplementedError("gate_mode 'wavenet' is not built for the flows of ParallelWaveNet")
        if cfg.filter_width != 2:
            raise NotImplementedError("filter_width %d: only 2 is built (reference default, model.py:9)" % cfg.filter_width)
        if cfg.dilation_channels not in (32, 64):
            raise NotImplementedError("dilation_channels %d: built for 32 and 64" % cfg.dilation_channels)
        if cfg.skip_channels % 32 or cfg.skip_channels < 32:
            raise NotImplementedError("skip_channels must be a multiple of 32")
        if cfg.output_channels < 1 or cfg.output_channels > 256:
            raise NotImplementedError("output_channels must be in [1, 256]")
        if cfg.head_mode == "mol" and (cfg.output_channels % 4 or not 4 <= cfg.output_channels <= 64):
            raise ValueError("mol head: output_channels = 4 * num_mixtures (<= 16 mixtures)")
        if cfg.head_mode not in ("per_timestep", "pooled", "mol", "flow", "contrastive"):
            raise ValueError("head_mode %r" % cfg.head_mode)
        if cfg.head_mode == "contrastive":
            # srwn_contrastive_head is one workgroup: the embeddings of all rows (and two floats per pair) live in its
            # 64 KiB of LDS.  Refused here, not on the first forward (the engine scores pairs when B is even)
            need = batch * cfg.output_channels + (batch if batch % 2 == 0 else 0)
            if need > CONTRASTIVE_LDS_FLOATS:
                raise ValueError("contrastive head: B=%d clips x D=%d dimensions (+ 2 per pair) need %d floats, over the "
                                 "head kernel's limit of %d (64 KiB of LDS)"
                                 % (batch, cfg.output_channels, need, CONTRASTIVE_LDS_FLOATS))
        if cfg.cond_channels and (length % cfg.pool_stride):
            raise ValueError("length %d is not a multiple of pool_stride %d" % (length, cfg.pool_stride))
        self.cfg = cfg
        # canonical gate: always the per-layer path (the group kernels, their weight-gradient tiles and the layer
        # weight-gradient kernel srwn_wgrad_layers all build c = z*sigmoid(z))
        self.wavenet = cfg.gate_mode == "wavenet"
        self.timing = False           # HIP-event spans with every launch alone on the chip (no side stream)
        self.timing_overlap = False   # the same spans inside the real schedule (side-stream work left running)
        self.spans: Dict[str, list] = {}
        import os as _os
        # multi-layer kernels (csrc/srwn_group.hip): SRWN_FUSE=0 keeps one launch per layer (the parity twin)
        fuse = _os.environ.get("SRWN_FUSE", "1")
        self.fuse_fwd = fuse not in ("0", "bwd") and not self.wavenet
        self.fuse_bwd = fuse not in ("0", "fwd") and not self.wavenet
        # SRWN_FUSE_WT=1 (default): layer weight gradients inside the 8-wave backward group kernel, split by output over
        # the waves; the forward group kernel writes the transposed operands ("weight-gradient tiles") they need
        # (csrc/srwn_group.hip, _wt entry points).  0: chain kernel + separate weight-gradient pass (the parity twin)
        self.fuse_wt = _os.environ.get("SRWN_FUSE_WT", "1") != "0"
        self.wt_store_x = _os.environ.get("SRWN_WT_STORE_X", "0") != "0"
        # SRWN_FUSE_IC (default on): the input conv inside the first layer group's forward kernel (unconditioned stacks)
        self.fuse_ic = _os.environ.get("SRWN_FUSE_IC", "1") != "0"
        # frozen: a stack that is never trained (a distillation teacher, model.py:334): fixed before allocation, so no
        # weight-gradient tiles / per-workgroup partial slabs are allocated for it and backward() refuses to run.  A
        # trainable stack can still be run forward-only (forward(train=False): the student does that to its teacher).
        self.frozen = bool(frozen)
        self._tiles_valid = False
        # weight-gradient passes on a side stream beside the data-gradient chain: worth 11 % with one launch per layer
        # (short latency-bound chain kernels), but with the group kernels every kernel of the backward phase is
        # bandwidth-bound and running two at once is slower than one after the other (2.15 vs 2.13 ms; the skip data
        # gradient beside the skip weight gradient: 446 us together, 347 us in turn) -> off by default there.
        # (decided on whether the grouped backward actually RUNS for this stack -- a 64/128 stack, say, keeps the per-layer
        # chain even with SRWN_FUSE=1 and wants the overlap)
        will_group = (self.fuse_bwd and cfg.dilation_channels in (32, 64) and cfg.filter_width == 2 and
                      ((cfg.dilation_channels, cfg.skip_channels) in ((64, 256), (32, 128)) or cfg.head_mode == "flow"))
        self.overlap = _os.environ.get("SRWN_OVERLAP", "0" if will_group else "1") != "0"
        self.seg_rows = int(_os.environ.get("SRWN_SEG_ROWS", "0"))
        # head 1x1 + softmax-CE + head data gradients as one launch (SRWN_HEAD_CHAIN=0: the four separate ones)
        self.head_chain = (_os.environ.get("SRWN_HEAD_CHAIN", "1") != "0" and cfg.head_mode == "per_timestep"
                           and cfg.dtype == torch.bfloat16 and cfg.skip_channels == 256)
        self._head_bwd_done = False
        self._ic_job = None
        self._loss_job = None
        self.defer_loss = _os.environ.get("SRWN_DEFER_LOSS", "1") != "0"      # (0: the loss sum keeps a launch of its own)
        self.side = None
        if torch.cuda.is_available() and self.overlap:
            # weight-gradient passes are throughput work: lowest priority, so the latency-critical dgrad
            # chain on the main stream gets CU slots first
            self.side = torch.cuda.Stream(priority=0)
        self.B, self.T = int(batch), int(length)
        self.N = self.B * self.T
        self.L = len(cfg.dilations)
        self.dil = [int(d) for d in cfg.dilations]
        self.R, self.S, self.C = cfg.dilation_channels, cfg.skip_channels, cfg.output_channels
        self.Kw = cfg.filter_width
        self.Cp = (self.C + 31) // 32 * 32
        self.E = cfg.cond_channels
        self.Ep = (self.E + 15) // 16 * 16
        self.frames = self.T // cfg.pool_stride if self.E else 0
        self.dev = torch.device(device)
        self.dt = cfg.dtype
        gl = int(_os.environ.get("SRWN_GROUP_LAYERS", "8"))
        # longest runs with a halo of at most one tile.  (SRWN_GROUP_PLAN=auto: the cost-model cut of
        # srwn_group_plan_auto -- measured slower on the benchmark shape: every extra launch costs ~14 us of launch,
        # segment prologue and store drain, more than the fuller tile rounds of shorter groups give back.)
        if _os.environ.get("SRWN_GROUP_PLAN", "greedy") == "auto" and self.R in (32, 64):
            self.groups = K.group_plan_auto(self.dil, self.B, self.T, self.R, self.dt, gl)
        else:
            self.groups = K.group_plan(self.dil, 31, gl)
        self.pg = process_group
        self.world = dp.world_size(process_group)
        if share_from is None:
            self._build_params(seed)
            self._build_packing()
        else:   # another (batch, length) view of the same model: parameters, moments, images are shared
            for a in ("sections", "nparams", "params", "grads", "adam_m", "adam_v", "adam_step", "bs_sum", "dead_gate",
                      "packer", "packed", "pack_train_elems", "o_conv", "o_res", "o_convT", "o_resT", "o_skipT", "o_skipT_all", "o_skip", "o_gen", "o_skip_gen",
                      "o_w1", "o_w2",
                      "o_w1T", "o_w2T", "o_w2p", "o_w2Tp", "o_w1Tp"):
                setattr(self, a, getattr(share_from, a))
            if self.E:
                self.o_wc = share_from.o_wc
        # training controls (optim.TrainControls): one holder per parameter buffer, shared like the Adam state
        self.ctl = share_from.ctl if share_from is not None else OptControls()
        self.ctl.engines.add(self)
        self._alloc_buffers()
        self.repack()

    # ------------------------------------------------------------------------------------------
    # parameters
    # ------------------------------------------------------------------------------------------
    def _build_params(self, seed):
        L, R, S, Kw, Cp, E = self.L, self.R, self.S, self.Kw, self.Cp, self.E
        secs: Dict[str, Section] = {}
        off = 0

        def add(name, shape):
            nonlocal off
            secs[name] = Section(name, off, shape)
            off += secs[name].numel

        add("init_w", (Kw, 1, R)); add("init_b", (R,))
        add("WF", (L, Kw, R, R)); add("BF", (L, R))
        if self.wavenet:      # (before WS: the gate's gradients join the second all-reduce bucket with the other layer ones)
            add("WG", (L, Kw, R, R)); add("BG", (L, R))
        add("WR", (L, R, R)); add("BR", (L, R))
        if E:
            add("WC", (L, E, R)); add("BC", (L, R))
        # the skip and head kernels come last: their gradients are final early in the backward pass and form the
        # first all-reduce bucket (everything from WS to the end), the per-layer gradients above form the second
        add("WS", (L, R, S)); add("BS", (L, S))
        add("head_w1", (S, S)); add("head_b1", (S,))
        add("head_w2", (S, Cp)); add("head_b2", (Cp,))   # padded to Cp columns (pad stays exactly zero)
        self.sections = secs
        self.nparams = off
        self.params = torch.zeros(off, dtype=torch.float32, device=self.dev)
        self.grads = torch.zeros(off, dtype=torch.float32, device=self.dev)
        self.adam_m = torch.zeros(off, dtype=torch.float32, device=self.dev)
        self.adam_v = torch.zeros(off, dtype=torch.float32, device=self.dev)
        self.adam_step = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.bs_sum = torch.zeros(S, dtype=torch.float32, device=self.dev)      # sum_l BS[l] (kept current by repack())
        # the dead gate conv variables of ops.py:31-33 exist in reference checkpoints; they take no
        # part in the graph (TF reports None gradients) so they live outside the trained buffer.
        # (gate_mode "wavenet": they are the trained sections WG / BG)
        self.dead_gate = None if self.wavenet else {
            "WG": torch.zeros((L, Kw, R, R), dtype=torch.float32, device=self.dev),
            "BG": torch.zeros((L, R), dtype=torch.float32, device=self.dev)}
        self.init_parameters(seed)

    def view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        s = self.sections[name]
        buf = self.params if buf is None else buf
        return buf[s.offset:s.offset + s.numel].view(s.shape)

    def init_parameters(self, seed: int):
        """Xavier-uniform kernels, zero biases (ops.py:15,18; tf.layers.conv1d defaults)."""
        rng = np.random.default_rng(seed)

        def xav(shape, fan_in, fan_out):
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            return torch.tensor(rng.uniform(-lim, lim, size=shape), dtype=torch.float32)

        L, R, S, Kw, C, E = self.L, self.R, self.S, self.Kw, self.C, self.E
        host = torch.zeros(self.nparams, dtype=torch.float32)

        def put(name, t):
            s = self.sections[name]
            host[s.offset:s.offset + s.numel] = t.reshape(-1)

        put("init_w", xav((Kw, 1, R), Kw * 1, Kw * R))
        put("WF", xav((L, Kw, R, R), Kw * R, Kw * R))
        put("WR", xav((L, R, R), R, R))
        put("WS", xav((L, R, S), R, S))
        if E:
            put("WC", xav((L, E, R), E, R))
        put("head_w1", xav((S, S), S, S))
        w2 = torch.zeros((S, self.Cp))
        w2[:, :C] = xav((S, C), S, C)
        put("head_w2", w2)
        wg = xav((L, Kw, R, R), Kw * R, Kw * R)      # (last in the RNG stream: every other draw is the same in both modes)
        if self.wavenet:
            put("WG", wg)
        self.params.copy_(host)
        if not self.wavenet:
            self.dead_gate["WG"].copy_(wg)
        self.adam_m.zero_(); self.adam_v.zero_(); self.adam_step.zero_()
        self._reset_ema()

    def load_oracle_params(self, sp):
        """Copies an oracle ``StackParams`` (tests) into the flat buffer."""
        host = torch.zeros(self.nparams, dtype=torch.float32)

        def put(name, arr):
            s = self.sections[name]
            host[s.offset:s.offset + s.numel] = torch.tensor(np.asarray(arr), dtype=torch.float32).reshape(-1)

        put("init_w", sp.init_w); put("init_b", sp.init_b)
        put("WF", np.stack([l.wf for l in sp.layers])); put("BF", np.stack([l.bf for l in sp.layers]))
        if self.wavenet:
            put("WG", np.stack([l.wg for l in sp.layers])); put("BG", np.stack([l.bg for l in sp.layers]))
        put("WR", np.stack([l.wr for l in sp.layers])); put("BR", np.stack([l.br for l in sp.layers]))
        put("WS", np.stack([l.ws for l in sp.layers])); put("BS", np.stack([l.bs for l in sp.layers]))
        if self.E:
            put("WC", np.stack([l.wc for l in sp.layers])); put("BC", np.stack([l.bc for l in sp.layers]))
        put("head_w1", sp.head_w1); put("head_b1", sp.head_b1)
        w2 = np.zeros((self.S, self.Cp)); w2[:, :self.C] = sp.head_w2
        b2 = np.zeros(self.Cp); b2[:self.C] = sp.head_b2
        put("head_w2", w2); put("head_b2", b2)
        self.params.copy_(host)
        self.adam_m.zero_(); self.adam_v.zero_(); self.adam_step.zero_()
        self._reset_ema()
        self.repack()

    def named_tensors(self, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Oracle-style names (l{i}.wf ...) -> views of `buf` (params by default)."""
        out = {"init_w": self.view("init_w", buf), "init_b": self.view("init_b", buf)}
        for i in range(self.L):
            out[f"l{i}.wf"] = self.view("WF", buf)[i]; out[f"l{i}.bf"] = self.view("BF", buf)[i]
            if self.wavenet:
                out[f"l{i}.wg"] = self.view("WG", buf)[i]; out[f"l{i}.bg"] = self.view("BG", buf)[i]
            out[f"l{i}.wr"] = self.view("WR", buf)[i]; out[f"l{i}.br"] = self.view("BR", buf)[i]
            out[f"l{i}.ws"] = self.view("WS", buf)[i]; out[f"l{i}.bs"] = self.view("BS", buf)[i]
            if self.E:
                out[f"l{i}.wc"] = self.view("WC", buf)[i]; out[f"l{i}.bc"] = self.view("BC", buf)[i]
        out["head_w1"] = self.view("head_w1", buf); out["head_b1"] = self.view("head_b1", buf)
        out["head_w2"] = self.view("head_w2", buf)[:, :self.C]; out["head_b2"] = self.view("head_b2", buf)[:self.C]
        return out

    def tf_variables(self, scope: str, decoder: bool) -> Dict[str, torch.Tensor]:
        """Reference variable names -> tensors in TF shapes, for checkpoint interchange."""
        per = 3 if decoder else 2

        def cname(j):
            return "conv1d" if j == 0 else "conv1d_%d" % j

        n = self.named_tensors()
        out = {f"{scope}/causal_conv_Kernel": n["init_w"], f"{scope}/causal_conv_Bias": n["init_b"].view(1, 1, -1)}
        for i in range(self.L):
            nm = f"dilated_conv_{i}"
            out[f"{scope}/{nm}_filter/{nm}_Kernel"] = n[f"l{i}.wf"]
            out[f"{scope}/{nm}_filter/{nm}_Bias"] = n[f"l{i}.bf"].view(1, 1, -1)
            gate = self.dead_gate if not self.wavenet else {"WG": self.view("WG"), "BG": self.view("BG")}
            out[f"{scope}/{nm}_gate/{nm}_Kernel"] = gate["WG"][i]
            out[f"{scope}/{nm}_gate/{nm}_Bias"] = gate["BG"][i].view(1, 1, -1)
            j = per * i
            if decoder:
                out[f"{scope}/{cname(j)}/kernel"] = n[f"l{i}.wc"].unsqueeze(0)
                out[f"{scope}/{cname(j)}/bias"] = n[f"l{i}.bc"]
                j += 1
            out[f"{scope}/{cname(j)}/kernel"] = n[f"l{i}.wr"].unsqueeze(0)
            out[f"{scope}/{cname(j)}/bias"] = n[f"l{i}.br"]
            out[f"{scope}/{cname(j + 1)}/kernel"] = n[f"l{i}.ws"].unsqueeze(0)
            out[f"{scope}/{cname(j + 1)}/bias"] = n[f"l{i}.bs"]
        out[f"{scope}/{cname(per * self.L)}/kernel"] = n["head_w1"].unsqueeze(0)
        out[f"{scope}/{cname(per * self.L)}/bias"] = n["head_b1"]
        out[f"{scope}/{cname(per * self.L + 1)}/kernel"] = n["head_w2"].unsqueeze(0)
        out[f"{scope}/{cname(per * self.L + 1)}/bias"] = n["head_b2"]
        return out

    # ------------------------------------------------------------------------------------------
    # MFMA weight images
    # ------------------------------------------------------------------------------------------
    def _build_packing(self):
        L, R, S, Kw, Cp, E, Ep = self.L, self.R, self.S, self.Kw, self.Cp, self.E, self.Ep
        sec = self.sections
        pk = K.Packer(self.dev)
        self._pack_stack(pk)
        self.pack_train_elems = None
        self._pack_head(pk)
        if self.pack_train_elems is None:      # (a head without generation-only images)
            self.pack_train_elems = pk.total
        pk.finalize()
        self.packer = pk
        self.packed = torch.zeros(max(pk.total, 1), dtype=self.dt, device=self.dev)

    def _pack_stack(self, pk):
        """Per-layer images of the residual stack: conv, 1x1 residual, their transposes, conditioning 1x1s."""
        L, R, Kw, E, Ep = self.L, self.R, self.Kw, self.E, self.Ep
        sec = self.sections
        self.o_conv, self.o_res, self.o_convT, self.o_resT = [], [], [], []
        for l in range(L):
            self.o_conv.append(P.pack_conv(pk, sec["WF"].offset + l * Kw * R * R, Kw, R))
            if self.wavenet:      # [Wf | Wg]: the gate conv's image right behind the filter's (one 2R-row product)
                o = P.pack_conv(pk, sec["WG"].offset + l * Kw * R * R, Kw, R)
                assert o == self.o_conv[l] + Kw * R * R
            self.o_res.append(P.pack_res(pk, sec["WR"].offset + l * R * R, R))
            self.o_convT.append(P.pack_conv_T(pk, sec["WF"].offset + l * Kw * R * R, Kw, R))
            if self.wavenet:      # [WfT | WgT] likewise (the data gradient contracts over both halves of D)
                o = P.pack_conv_T(pk, sec["WG"].offset + l * Kw * R * R, Kw, R)
                assert o == self.o_convT[l] + Kw * R * R
            self.o_resT.append(P.pack_linear_T(pk, sec["WR"].offset + l * R * R, R, R, R, perm=True))
        if E:
            # conditioning 1x1 of every layer as one [Ep] -> [L*R] product (model.py:180)
            self.o_wc = pk.reserve(L * R // 32, Ep // 16)
            for l in range(L):
                P.fill_linear(pk, self.o_wc + l * (R // 32) * (Ep // 16) * 512, sec["WC"].offset + l * E * R, E, R,
                              R // 32, Ep // 16)

    def _pack_head(self, pk):
        L, R, S, Kw, Cp = self.L, self.R, self.S, self.Kw, self.Cp
        sec = self.sections
        self.o_skipT = []
        # transposed skip kernels of all layers back to back (srwn_skip_dgrad_all streams them in order)
        per = (R // 32) * (S // 16) * 512
        self.o_skipT_all = pk.reserve(L * (R // 32), S // 16)
        for l in range(L):
            P.fill_linear_T(pk, self.o_skipT_all + l * per, sec["WS"].offset + l * R * S, R, S, R // 32, S // 16)
            self.o_skipT.append(self.o_skipT_all + l * per)
        # all skip 1x1s as one image: rows = skip channel, k = layer*R + n
        self.o_skip = pk.reserve(S // 32, L * R // 16)
        for l in range(L):
            P.fill_linear(pk, self.o_skip, sec["WS"].offset + l * R * S, R, S, S // 32, L * R // 16,
                          ks_offset=l * R // 16, ks_count=R // 16)
        self.o_w1 = P.pack_linear(pk, sec["head_w1"].offset, S, S, S)
        self.o_w2 = P.pack_linear(pk, sec["head_w2"].offset, S, Cp, Cp)
        self.o_w1T = P.pack_linear_T(pk, sec["head_w1"].offset, S, S, S)
        self.o_w2T = P.pack_linear_T(pk, sec["head_w2"].offset, S, Cp, S)
        # the same three in the accumulator's k order, for the one-launch head (csrc/srwn_head.hip)
        self.o_w2p = self.o_w2Tp = self.o_w1Tp = None
        if S == 256 and Cp == 256:
            self.o_w2p = P.pack_linear(pk, sec["head_w2"].offset, S, Cp, Cp, perm=True)
            self.o_w2Tp = P.pack_linear_T(pk, sec["head_w2"].offset, S, Cp, S, perm=True)
            self.o_w1Tp = P.pack_linear_T(pk, sec["head_w1"].offset, S, S, S, perm=True)
        # ---- everything above is read by the training step and re-gathered after every optimizer step; the images below
        # serve generate() only and are re-gathered there (they are 45 % of the image: 3.7 of 8.1 MB for config 2)
        self.pack_train_elems = pk.total
        # generation images: per layer [conv (last tap permuted) | residual], back to back (srwn_generate)
        self.o_gen = self.o_skip_gen = None
        if R in (32, 64) and S in (128, 256) and Kw == 2:
            for l in range(L):
                o = P.pack_conv_gen(pk, sec["WF"].offset + l * Kw * R * R, Kw, R)
                P.pack_res(pk, sec["WR"].offset + l * R * R, R)
                if l == 0:
                    self.o_gen = o
            # skip kernels for generation: B operand is the gate tile in registers -> permuted k order
            self.o_skip_gen = pk.reserve(S // 32, L * R // 16)
            for l in range(L):
                P.fill_linear(pk, self.o_skip_gen, sec["WS"].offset + l * R * S, R, S, S // 32, L * R // 16,
                              ks_offset=l * R // 16, ks_count=R // 16, perm=True)
        # the latency-optimised generator's fragment images (csrc/srwn_gen16.hip)
        self.o_g16 = None
        if (self.o_gen is not None and R in (32, 64) and S in (128, 256) and self.dt == torch.bfloat16 and L <= 64
                and ((self.cfg.head_mode == "per_timestep" and not self.E) or self.cfg.head_mode == "mol")):
            self.o_g16 = pk.reserve_raw(np.concatenate([P.gen16_layer_index(sec["WF"].offset, sec["WR"].offset,
                                                                            sec["WS"].offset, l, R, S) for l in range(L)]))
            self.o_g16_h1 = pk.reserve_raw(P.gen16_head_index(sec["head_w1"].offset, S, S, S))
            self.o_g16_h2 = pk.reserve_raw(P.gen16_head_index(sec["head_w2"].offset, S, Cp, Cp, interleave=True))

    def wptr(self, off: int) -> int:
        return self.packed.data_ptr() + off * self.packed.element_size()

    def repack(self):
        """Rebuilds what the kernels derive from the parameters: the weight images the training / forward kernels read (the
        generation-only tail: `_repack_generation`) and, in the same launch, the sum of the layers' skip biases (the bias of
        the skip sum, model.py:50: it was a reduction launch in front of every forward pass)."""
        bs = getattr(self, "bs_sum", None)      # (the flows of the student carry no skip path)
        rs = (self.view("BS"), bs) if (bs is not None and "BS" in self.sections) else None
        self.packer.gather(self.params, self.packed, 0, getattr(self, "pack_train_elems", None), rowsum=rs)

    def _repack_generation(self):
        n = getattr(self, "pack_train_elems", None)
        if n is not None and n < self.packer.total:
            self.packer.gather(self.params, self.packed, n, None)

    # ------------------------------------------------------------------------------------------
    # buffers
    # ------------------------------------------------------------------------------------------
    def _alloc_buffers(self):
        self._alloc_stack_buffers()
        self._alloc_head_buffers()

    def _alloc_stack_buffers(self):
        """Saved activations / gradients of the residual stack and its weight-gradient scratch."""
        B, T, N, L, R = self.B, self.T, self.N, self.L, self.R
        z = lambda *s, dt=self.dt: torch.zeros(s, dtype=dt, device=self.dev)
        self.audio = z(B, T, dt=torch.float32)
        self.xs = z(L + 1, B, T, R)
        self.zs = z(L, B, T, R)
        self.dfs = z(L, B, T, 2 * R if self.wavenet else R)   # (wavenet: D = [d f | d g] of both convs)
        if self.wavenet:
            self.ss = z(L, B, T, R)      # sigmoid(Wg*x + bg)
            self.cs = z(L, B, T, R)      # c = z*s: the skip sum and the 1x1 weight gradients read it as it is
            # both convs' weight / bias gradients as srwn_wgrad leaves them ([in, 2R] per tap), split into WF|WG, BF|BG
            self.wn_wgrad = z(L, self.Kw, R, 2 * R, dt=torch.float32)
            self.wn_bgrad = z(L, 2 * R, dt=torch.float32)
        self.gs = z(L + 1, B, T, R)   # gs[L] is never written by the teacher: its last dense output is unused
        self.nslabs = K.wgrad_slabs(N)
        self.use_wl = (R in (32, 64) and self.Kw == 2) and not self.wavenet
        self.use_dcs = (R, self.S) in ((64, 256), (32, 128))
        import os as _os
        # decided ONCE, before anything is sized (the tiles, the partial slabs and the skip weight-gradient path follow it)
        self._fused_wt = (self.fuse_wt and self.fuse_fwd and self.fused_bwd and self.cfg.head_mode != "flow"
                          and not self.frozen)
        if self.fused_wt:
            # weight-gradient tiles of every layer (written by the forward group kernels, read by the backward ones) and one
            # partial slab per workgroup of the backward kernels (slabs a group does not reach stay zero)
            geo = [K.group_wt_geometry(self.dil[l0:l1], B, T, R, self.dt, self.seg_rows) for l0, l1 in self.groups]
            self.wt_seg_rows = [g[0] for g in geo]
            wt_elems = max(g[2] for g in geo)
            self.xTs = z(L, wt_elems)
            self.cTs = z(L, wt_elems)
            self.nslabs = max(g[3] for g in geo)
            self.wt_segs = [(g[2] // (g[1] * R * 32), g[3]) for g in geo]      # per group: (segments, workgroups)
            # per layer: the stride and segment length of its group (what fixes the positions its tiles hold)
            self.wt_layer_st = [math.gcd(*self.dil[l0:l1]) for l0, l1 in self.groups for _ in range(l0, l1)]
            self.wt_layer_seg = [self.wt_seg_rows[i] for i, (l0, l1) in enumerate(self.groups) for _ in range(l0, l1)]
        elif self.use_wl and self.fuse_bwd and "SRWN_WG_SLAB_ROWS" not in _os.environ and self.groups:
            # the layer weight-gradient pass is launched per layer group with one workgroup per (layer, slab): cut the
            # rows so that the widest group's launch is one workgroup per CU (5-layer groups at 3072 rows per slab left
            # 46 of 256 CUs idle: 578 -> 503 us per step), slabs of at least 256 rows
            cus = torch.cuda.get_device_properties(self.dev).multi_processor_count if torch.cuda.is_available() else 256
            widest = max(l1 - l0 for l0, l1 in self.groups)
            self.nslabs = int(max(1, min(cus // widest, (N + 255) // 256, 256)))
        # SRWN_PART16 (default on; bf16 weight-gradient-tile mode only): the per-workgroup partial sums of the conv-tap and
        # residual 1x1 weight gradients are stored in the compute type (16 x 16 blocks in lane order) instead of fp32 --
        # 256 workgroups x 30 layers x 48 KB = 0.38 GB per step written by the backward group kernels and read back by the
        # reduction, halved, for one more bf16 rounding per partial (measured: +1.3e-4 .. 5.7e-4 relative L2 on those
        # gradients, whose bf16-mode error against the exact-fp32 mode is 7e-3: DESIGN.md 4c).
        # ... but only in the groups whose workgroups run ONE segment each: on every later segment a workgroup re-reads its
        # bf16 block, adds the segment's fp32 sum and rounds again (k segments per workgroup: k roundings of the running
        # sum; measured 1.9e-3 at k = 1 growing to 3.9e-3 at 8 and 7.0e-3 at 32).  A group with more segments than
        # workgroups (e.g. 16 x 16000 clips per GPU) keeps fp32 slabs.  SRWN_PART16=2: bf16 blocks in every group
        # (measurement: tests/test_gpu_multiseg.py)
        p16env = _os.environ.get("SRWN_PART16", "1")
        self.part16 = (self.fused_wt and self.dt == torch.bfloat16 and p16env != "0")
        self.group_p16 = [self.part16 and (nseg <= nwg or p16env == "2") for nseg, nwg in self.wt_segs] if self.fused_wt else []
        if self.use_wl:
            ns = self.nslabs
            mk = lambda dt: (z(L * ns * 2 * R * R, dt=dt), z(L * ns * R * R, dt=dt))
            pl16 = mk(torch.bfloat16) if any(self.group_p16) else None
            pl32 = mk(torch.float32) if not (self.group_p16 and all(self.group_p16)) else None
            self.pl_f, self.pl_r = pl16 or pl32      # the partials of the engine's mode; fp32 slabs where no group keeps blocks
            self.pl_f32, self.pl_r32 = pl32 or (None, None)      # (fp32 slabs of the groups that fall back)
            self.pl_bf = z(L * ns * R, dt=torch.float32); self.pl_br = z(L * ns * R, dt=torch.float32)
        from . import _lib
        # the input conv's weight-gradient partials: srwn_init_conv_wgrad's stage-1 slabs, or -- default path, unconditioned
        # stacks with a skip path -- one slab per workgroup of the FIRST group's backward launch, which forms them from its
        # bottom gradient while it is on the chip (no launch of its own)
        self.fuse_icg = (self.fused_wt and self.fuse_ic and not self.E and self.Kw == 2 and self.use_dcs
                         and (self.part16 or self.dt == torch.float32))
        self.ic_ws = z(max(int(_lib.load().srwn_init_conv_wgrad_partials(B, T, R, self.Kw)),
                           self.nslabs * (8 // (R // 16)) * (self.Kw + 1) * R if self.fuse_icg else 0), dt=torch.float32)
        if self.E:
            self.cond_in = z(B * self.frames, self.Ep)
            self.cond_all = z(L, B * self.frames, R)      # cb of every layer, layer by layer: a layer's frame rows are dense
            self.dcb = z(L, B * self.frames, R)
            # (few rows: one slab would be L workgroups walking B*frames rows in 32-row steps -- 69 us for 31 MFLOP at
            # 1 024 rows; 128-row slabs fill the chip)
            rows_c = B * self.frames
            self.nslabs_c = max(K.wgrad_slabs(rows_c), min(max(1, 256 // L), max(1, rows_c // 128)))
            self.wgc_parts = z(self.nslabs_c * L * self.Ep * R, dt=torch.float32)
            self.wgc_bparts = z(self.nslabs_c * L * R, dt=torch.float32)
            self.wc_grad_pad = z(L, self.Ep, R, dt=torch.float32)

    def _alloc_head_buffers(self):
        B, T, N, L, R, S, Cp = self.B, self.T, self.N, self.L, self.R, self.S, self.Cp
        z = lambda *s, dt=self.dt: torch.zeros(s, dtype=dt, device=self.dev)
        self.targets = torch.zeros(N, dtype=torch.int32, device=self.dev)
        if self.use_dcs:
            self.dcs = z(L, B, T, R)  # Ws_l . dtotal of every layer (one output-streaming GEMM)
        self.r0 = z(N, S); self.r1 = z(N, S); self.da1 = z(N, S); self.dtotal = z(N, S)
        self.dlogits = z(N, Cp)
        self.loss_parts = z((N + 31) // 32, dt=torch.float32)
        self.loss = z(1, dt=torch.float32)
        self.pooled = self.cfg.head_mode == "pooled"
        self.mol = self.cfg.head_mode == "mol"
        if self.mol:
            self.logits32 = z(N, Cp, dt=torch.float32)
        if self.pooled:
            self.labels = z(B, self.C, dt=torch.float32)
            self.probs = z(B, self.C, dt=torch.float32)
        if self.contrastive:      # B = 2P rows: the left clips, then the right ones
            self.labels = z(B // 2, dt=torch.float32)
            self.emb = z(B, self.C, dt=torch.float32)
            self.dist = z(B // 2, dt=torch.float32)
        if self.clip_head:
            from . import _lib as _l
            self.mean_r1 = z(B, S, dt=torch.float32)
            self.dmean = z(B, S, dt=torch.float32)
            self.tm_parts = z(B * int(_l.load().srwn_time_mean_slabs(T)) * S, dt=torch.float32)
        big = max(L * R * S, S * S, S * Cp, L * self.Kw * R * R)
        self.use_w256 = (S in (128, 256) and R in (32, 64) and (L * R) % 64 == 0)
        if self.use_w256:
            self.ns_skip = K.wgrad256_slabs(N, L, R)
            self.ns_head = K.wgrad256_slabs(N, S // 64)
            big = max(big, -(-max(self.ns_skip * L * R * S, self.ns_head * S * 256) // self.nslabs))
        # skip weight gradients from the forward's transposed gate outputs (csrc/srwn_wgradt.hip)
        self.skip_wt = (self.use_w256 and self.fused_wt and self.dt == torch.bfloat16 and (R, S) == (64, 256)
                        and _os_environ_flag("SRWN_WGRAD_WT", True))
        self.skip_parts16 = None
        if self.skip_wt:
            self.ns_skip_wt = K.wgrad_skip_wt_slabs(self.wt_layer_st, self.wt_layer_seg, T)
            if self.part16:      # its partial slabs in the compute type too (a buffer of their own: wg_parts is fp32)
                self.skip_parts16 = z(self.ns_skip_wt * L * R * S)
            else:
                big = max(big, -(-self.ns_skip_wt * L * R * S // self.nslabs))
        self.wg_parts = z(self.nslabs * big, dt=torch.float32)
        self.wg_bparts = z(max(self.nslabs * max(L * S, Cp, 2 * L * R if self.wavenet else 0), 256 * 256), dt=torch.float32)
        # the two head products keep partials of their own, so that skip + head finish in ONE reduction launch
        self.batch_reduce = self.use_w256 and not self.clip_head and Cp == 256 and _os_environ_flag("SRWN_BATCH_REDUCE", True)
        if self.batch_reduce:
            self.hd_parts = [z(self.ns_head * S * 256, dt=torch.float32) for _ in range(2)]
            self.hd_bparts = [z(self.ns_head * 256, dt=torch.float32) for _ in range(2)]

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def set_inputs(self, audio: torch.Tensor, targets: Optional[torch.Tensor] = None,
                   cond: Optional[torch.Tensor] = None):
        self.audio.copy_(audio.reshape(self.B, self.T))
        if targets is not None:
            if self.pooled:
                self.labels.copy_(targets.reshape(self.B, self.C))
            elif self.contrastive:
                if self.B % 2:
                    raise ValueError("contrastive head: labels need B = 2P rows (left clips, then right), got B=%d" % self.B)
                self.labels.copy_(targets.reshape(self.B // 2))
            else:
                self.targets.copy_(targets.reshape(self.N))
        if self.E:
            if cond is None:
                raise ValueError("this stack was built with conditioning; pass cond [B, frames, cond_channels]")
            self.cond_in.zero_()
            self.cond_in[:, :self.E].copy_(cond.reshape(self.B * self.frames, self.E))

    def forward(self, want_logits: bool = False, with_loss: bool = True, train: bool = True,
                defer_loss: bool = False, stack_only: bool = False) -> Optional[torch.Tensor]:
        """Runs the stack on the staged inputs; leaves loss in self.loss and dlogits for backward.
        Returns fp32 per-time-step logits [B,T,C] when want_logits.  train=False: forward only (no weight-gradient tiles
        are written; backward() refuses to follow such a pass).  defer_loss (the training step): the final sum of the loss
        partials is left to the backward pass, where it is one more job of the skip / head reduction launch.
        stack_only (internal: priming a generation state): the input conv and the residual layers only -- xs holds every
        layer's input afterwards -- no skip sum, no head, no loss."""
        B, T, N, L, R, S = self.B, self.T, self.N, self.L, self.R, self.S
        es = self.packed.element_size()
        v = self.view
        # input conv (model.py:40 / 172-173); RightShift folded into the tap offset.  Where the first layer group runs as a
        # group kernel on an unconditioned stack, the conv is computed inside it (its output never reaches HBM: nothing else
        # reads xs[0] unless the inner layer inputs are kept for inspection)
        self._tiles_valid = bool(train) and self.fused_wt
        self._ic_fused = (self.fuse_ic and self._tiles_valid and not self.E and self.Kw == 2 and not self.wt_store_x
                          and bool(self.groups))
        if not self._ic_fused:
            K.causal_conv1d_fwd(self.audio.view(B, T, 1), v("init_w"), v("init_b"), 1,
                                1 if self.cfg.shift_input else 0, out=self.xs[0])
        if self.E:
            self._cond_bias_to_input()
        with _Span(self, "fwd_layers"):
            self._stack_fwd(self.cond_all if self.E else None, wt=self._tiles_valid)
        if stack_only:
            return None
        with _Span(self, "skip_sum"):      # model.py:50-51 (bs_sum = the sum of the layers' skip biases: formed by repack())
            K.pw_linear(self._gate_out.data_ptr(), R, N * R, R, L * R, self.wptr(self.o_skip), self.bs_sum, self.r0, S, S,
                        N, pro=self._gate_pro, epi=K.EPI_RELU)
        self._head_bwd_done = False
        if self.head_chain and self.o_w2p is not None and not want_logits and with_loss:
            # model.py:53-56 + softmax CE + the two head data gradients: rows never leave the registers in between
            with _Span(self, "head_chain"):
                K.head_chain(self.r0, self.wptr(self.o_w1), self.wptr(self.o_w2p), self.wptr(self.o_w2Tp),
                             self.wptr(self.o_w1Tp), v("head_b1"), v("head_b2"), self.targets, self.loss_parts,
                             self.r1, self.dlogits, self.da1, self.dtotal, self.C, 1.0 / N)
            self._head_bwd_done = True
            if defer_loss and train and self.batch_reduce and not self.frozen and self.defer_loss:
                self._loss_job = (self.loss_parts, self.loss_parts.numel(), 1, 1, True, 1.0 / N, self.loss.data_ptr(), 0, "sum")
            else:
                K.reduce_loss(self.loss_parts, self.loss_parts.numel(), 1.0 / N, self.loss)
            return None
        with _Span(self, "head_1x1"):
            K.pw_linear(self.r0.data_ptr(), S, 0, S, S, self.wptr(self.o_w1), v("head_b1"), self.r1, S, S, N,
                        epi=K.EPI_RELU)                                               # model.py:53-54
        if self.clip_head:
            return self._forward_pooled_head(with_loss)
        if self.mol:
            # last 1x1 in fp32 (the mixture parameters need it), then the mixture-of-logistics NLL on the
            # UNshifted clip (labels = inputs, model.py:103,114) and its gradient
            with _Span(self, "head_mol"):
                K.pw_linear(self.r1.data_ptr(), S, 0, S, S, self.wptr(self.o_w2), v("head_b2"), self.logits32,
                            self.Cp, self.C, N, epi=K.EPI_F32, compute_dtype=self.dt)
                K.mol_loss(self.logits32, self.audio.view(N), self.C // 4, self.loss_parts, self.dlogits, 1.0)
            if with_loss:
                K.reduce_loss(self.loss_parts, (N + 255) // 256, 1.0, self.loss)
            return self.logits32[:, :self.C].reshape(B, T, self.C).clone() if want_logits else None
        logits = None
        if want_logits:
            logits = torch.empty((N, self.C), dtype=torch.float32, device=self.dev)
        with _Span(self, "head_softmax_ce"):
            K.head_softmax_ce(self.r1, self.wptr(self.o_w2), v("head_b2"), self.targets, self.loss_parts,
                              self.dlogits, logits, self.Cp, self.C, 1.0 / N)          # model.py:56 + softmax CE
        if with_loss:
            K.reduce_loss(self.loss_parts, self.loss_parts.numel(), 1.0 / N, self.loss)
        return None if logits is None else logits.view(B, T, self.C)

    def _forward_pooled_head(self, with_labels: bool):
        """model.py:56-60: last 1x1, average pool over the clip, softmax -- computed as the 1x1 of the
        time-mean (the pool commutes with it); leaves probs [B,C], loss, and dmean for backward.
        Contrastive head (model.py:708-750): the same pooled 1x1 is the embedding; leaves emb [B,C], dist [P] (B even),
        loss and dmean.  Either head writes the head_w2 / head_b2 gradients itself when it has labels."""
        from ._lib import call
        st = torch.cuda.current_stream().cuda_stream
        B, T, S, C, Cp = self.B, self.T, self.S, self.C, self.Cp
        g = self.grads
        call("srwn_time_mean", self.r1.data_ptr(), self.tm_parts.data_ptr(), self.mean_r1.data_ptr(), B, T, S,
             K.abi_dtype(self.dt), st)
        if self.contrastive:
            call("srwn_contrastive_head", self.mean_r1.data_ptr(), self.view("head_w2").data_ptr(),
                 self.view("head_b2").data_ptr(), self.labels.data_ptr() if with_labels else None, float(self.cfg.margin),
                 self.emb.data_ptr(), None if B % 2 else self.dist.data_ptr(), self.loss.data_ptr(),
                 self.view("head_w2", g).data_ptr(), self.view("head_b2", g).data_ptr(), self.dmean.data_ptr(), B, S,
                 C, Cp, st)
            return None
        call("srwn_pooled_head", self.mean_r1.data_ptr(), self.view("head_w2").data_ptr(),
             self.view("head_b2").data_ptr(), self.labels.data_ptr() if with_labels else None, self.probs.data_ptr(),
             self.loss.data_ptr(), self.view("head_w2", g).data_ptr(), self.view("head_b2", g).data_ptr(),
             self.dmean.data_ptr(), B, S, C, Cp, st)
        return None

    def _cond_bias_to_input(self):
        """cb_l = 1x1(encoding_w_condition) of every layer as one product (model.py:180), and the first layer's bias
        onto the input conv's output (model.py:181-183).  Every later layer receives its bias from the layer below:
        xs[l] always holds layer l's complete input, so taps, residual base and weight gradients never re-add it."""
        from ._lib import call
        L, R = self.L, self.R
        rows_c = self.B * self.frames
        st = torch.cuda.current_stream().cuda_stream
        call("srwn_pw_linear_ychunks", self.cond_in.data_ptr(), self.Ep, self.Ep, self.wptr(self.o_wc),
             self.view("BC").reshape(-1).data_ptr(), self.cond_all.data_ptr(), R, R, rows_c * R, L * R, L * R, rows_c,
             K.abi_dtype(self.dt), st)
        call("srwn_add_frame_bias", self.xs[0].data_ptr(), self.cond_all.data_ptr(), R, self.B, self.T, R,
             self.frames, self.cfg.pool_stride, K.abi_dtype(self.dt), st)

    def _stack_fwd(self, cond_all: Optional[torch.Tensor], wt: Optional[bool] = None):
        """The residual layers (model.py:42-47 / 176-189 / 428-453): xs[0] -> xs[1..L], zs[0..L-1].
        wt: also write the weight-gradient tiles (default: whenever the backward pass reads them)."""
        wt = self.fused_wt if wt is None else (wt and self.fused_wt)
        if self.fuse_fwd:
            for l0, l1 in self.groups:      # runs of layers whose outputs travel between layers in LDS
                if l1 - l0 >= 2 or wt:
                    self._group_fwd(l0, l1, cond_all, wt)
                else:
                    self._layer_fwd(l0, cond_all)
        else:
            for l in range(self.L):
                self._layer_fwd(l, cond_all)

    def _group_fwd(self, l0: int, l1: int, cond_all: Optional[torch.Tensor], use_wt: bool = True):
        """Layers [l0, l1) in one launch (srwn_residual_group_fwd); same stored xs / zs as the per-layer path."""
        v = self.view
        cond3 = None
        if cond_all is not None:      # layer l adds the bias of layer l + 1 onto its output
            cond3 = [cond_all[l + 1].view(self.B, self.frames, self.R) if l + 1 < self.L else None for l in range(l0, l1)]
        wt = {}
        use_wt = use_wt and self.fused_wt
        if l0 == 0 and getattr(self, "_ic_fused", False):
            if use_wt:
                wt = dict(xT=self.xTs[l0:l1], cT=self.cTs[l0:l1], store_inner_x=self.wt_store_x)
            K.residual_group_fwd_ic(self.audio, v("init_w"), v("init_b"), 1 if self.cfg.shift_input else 0,
                                    self.xs[l0 + 1:l1 + 1], self.zs[l0:l1],
                                    [self.wptr(self.o_conv[l]) for l in range(l0, l1)],
                                    [self.wptr(self.o_res[l]) for l in range(l0, l1)],
                                    [v("BF")[l] for l in range(l0, l1)], [v("BR")[l] for l in range(l0, l1)],
                                    self.dil[l0:l1], self.Kw,
                                    seg_rows=self.wt_seg_rows[self.groups.index((l0, l1))] if use_wt else self.seg_rows, **wt)
            return
        if use_wt:
            # (xs of the layers inside a group is NOT written in this mode: only the weight gradients would read it, and they
            # take the transposed tiles; SRWN_WT_STORE_X=1 keeps it for inspection)
            wt = dict(xT=self.xTs[l0:l1], cT=self.cTs[l0:l1], store_inner_x=self.wt_store_x)
        K.residual_group_fwd(self.xs[l0], self.xs[l0 + 1:l1 + 1], self.zs[l0:l1],
                             [self.wptr(self.o_conv[l]) for l in range(l0, l1)],
                             [self.wptr(self.o_res[l]) for l in range(l0, l1)],
                             [v("BF")[l] for l in range(l0, l1)], [v("BR")[l] for l in range(l0, l1)],
                             self.dil[l0:l1], self.Kw, cond=cond3,
                             pool_stride=self.cfg.pool_stride,
                             seg_rows=self.wt_seg_rows[self.groups.index((l0, l1))] if use_wt else self.seg_rows, **wt)

    def _layer_fwd(self, l: int, cond_all: Optional[torch.Tensor]):
        v = self.view
        nxt = cond_all is not None and l + 1 < self.L      # the NEXT layer's conditioning bias goes onto the output
        cond3 = cond_all[l + 1].view(self.B, self.frames, self.R) if nxt else None
        if self.wavenet:
            K.wavenet_layer_fwd(self.xs[l], cond3, self.wptr(self.o_conv[l]), self.wptr(self.o_res[l]), v("BF")[l],
                                v("BG")[l], v("BR")[l], self.xs[l + 1], self.zs[l], self.ss[l], self.cs[l], self.Kw,
                                self.dil[l], self.cfg.pool_stride)
            return
        K.residual_layer_fwd(self.xs[l], cond3, self.wptr(self.o_conv[l]), self.wptr(self.o_res[l]), v("BF")[l],
                             v("BR")[l], self.xs[l + 1], self.zs[l], self.Kw, self.dil[l], self.cfg.pool_stride)

    # ------------------------------------------------------------------------------------------
    # backward
    # ------------------------------------------------------------------------------------------
    def backward(self, join: bool = True, part: int = 0):
        """join=False leaves the weight-gradient passes running on ``self.side`` (the caller joins it before the
        optimizer): work that only needs the data gradients can start right away.
        part: 0 = the whole pass; 1 = head + dgrad chain down to layer ``self.split_layer`` and, on return, the skip /
        head gradients are FINAL (first all-reduce bucket, ``grads[bucket_off:]``); 2 = the rest.  Splitting lets the
        data-parallel step all-reduce the first bucket while part 2 runs.
        Data gradients top-down on the current stream; weight gradients on a side stream as soon as their
        operands exist (skip/head kernels right after the head data gradients, per-layer kernels in groups
        behind the dgrad chain), so the bandwidth-bound wgrad passes fill the ramp/tail bubbles of the
        short per-layer dgrad kernels.  Joined before the optimizer.  SRWN_OVERLAP=0 serialises everything."""
        B, T, N, L, R, S, Kw = self.B, self.T, self.N, self.L, self.R, self.S, self.Kw
        dt = self.dt
        if self.frozen:
            raise RuntimeError("backward: this stack was built frozen (forward only)")
        if self.fused_wt and not self._tiles_valid:
            raise RuntimeError("backward: the last forward pass ran with train=False and wrote no weight-gradient tiles")
        main = torch.cuda.current_stream()
        overlap = self.overlap and not self.timing
        side = self.side if overlap else main
        if part in (0, 1):
            self._bwd_head()
            if overlap:
                side.wait_stream(main)
            with torch.cuda.stream(side):
                self._wgrad_skip_and_head()
            if self.use_dcs:
                with _Span(self, "skip_dgrad_all"):
                    K.skip_dgrad_all(self.dtotal, self.wptr(self.o_skipT_all), self.dcs.view(L, N, R), R, S)
        # ---- residual stack, top down
        groups = self._wl_groups() if self.use_wl else []
        group_lo = {g[0]: g for g in groups}
        l_hi = self.split_layer - 1 if part == 2 else L - 1
        l_lo = self.split_layer if part == 1 else 0
        span = _Span(self, "bwd_layers" if part == 0 else "bwd_layers_part%d" % part).__enter__()
        if self.fused_bwd:
            # one launch per group of layers (srwn_residual_group_bwd), top group first; each group's weight-gradient
            # pass follows it on the side stream.  The bottom group writes gs[0]: no UP-only launch below layer 0.
            for l0, l1 in reversed(self.groups):
                if l0 > l_hi or l0 < l_lo:
                    continue
                if self.fused_wt:
                    self._group_bwd_wt(l0, l1)
                    continue
                self._group_bwd(l0, l1)
                if not self.timing:
                    if overlap:
                        ev = torch.cuda.Event()
                        ev.record(main)
                        side.wait_event(ev)
                    with torch.cuda.stream(side):
                        self._wgrad_layers_group(l0, l1)
            span.__exit__()
            if part == 1:
                if overlap:
                    main.wait_stream(side)
                return
            if self.timing and not self.fused_wt:
                for g in groups:
                    self._wgrad_layers_group(*g)
            merged = self.use_wl      # the input conv's slab sum joins the final reduction launch
            if merged and overlap:
                side.wait_stream(main)      # (gs[0], which the input conv's gradient reads, is complete on the main stream)
            with torch.cuda.stream(side):
                if merged and self._ic_job is None:      # (not already left by the first group's backward launch)
                    self._wgrad_input_conv_partials()
                self._wgrad_layers_finish()
            self._wgrad_input_and_cond(input_conv=not merged)
            if overlap and join:
                main.wait_stream(side)
            return
        for l in range(l_hi, l_lo - 1, -1):
            has_up = l < L - 1
            g_in = self.gs[l + 2] if (has_up and l + 2 < L) else None
            if self.wavenet:
                self._wavenet_layer_bwd(l, g_in, has_up)
            else:
                K.residual_layer_bwd(g_in, self.dfs[l + 1] if has_up else None,
                                     self.wptr(self.o_convT[l + 1]) if has_up else None,
                                     self.gs[l + 1] if has_up else None,
                                     self.wptr(self.o_resT[l]) if has_up else None,
                                     None if self.use_dcs else self.wptr(self.o_skipT[l]),
                                     None if self.use_dcs else self.dtotal, self.zs[l], self.dfs[l], B, T, R, S, Kw,
                                     self.dil[l + 1] if has_up else 1, has_up, True, dt,
                                     dcs=self.dcs[l] if self.use_dcs else None)
            if l in group_lo and not self.timing:   # df_l.. and G_{l+1}.. of this group are complete
                if overlap:
                    ev = torch.cuda.Event()
                    ev.record(main)
                    side.wait_event(ev)
                with torch.cuda.stream(side):
                    self._wgrad_layers_group(*group_lo[l])
        if part == 1:
            span.__exit__()
            if overlap:
                main.wait_stream(side)   # skip/head gradients (and the layer groups launched so far) are in
            return
        if self.wavenet:
            K.wavenet_layer_bwd(self.gs[1] if L > 1 else None, self.dfs[0], self.wptr(self.o_convT[0]), self.gs[0],
                                None, None, None, None, None, None, None, B, T, R, S, Kw, self.dil[0], True, False, dt)
        else:
            K.residual_layer_bwd(self.gs[1] if L > 1 else None, self.dfs[0], self.wptr(self.o_convT[0]), self.gs[0],
                                 None, None, None, None, None, B, T, R, S, Kw, self.dil[0], True, False, dt)
        span.__exit__()
        if self.timing:   # (timed runs keep the dgrad chain's span free of the weight-gradient passes)
            for g in groups:
                self._wgrad_layers_group(*g)
        merged = self.use_wl      # (as in the grouped path: the same sums in the same order)
        if overlap:       # (the canonical gate's conv weight gradients read every D_l of the chain: no group events)
            side.wait_stream(main)
        with torch.cuda.stream(side):
            if merged:
                self._wgrad_input_conv_partials()
            self._wgrad_layers_finish()
        self._wgrad_input_and_cond(input_conv=not merged)
        if overlap and join:
            main.wait_stream(side)

    def _wavenet_layer_bwd(self, l: int, g_in: Optional[torch.Tensor], has_up: bool):
        """Canonical gate: G_{l+1} from D_{l+1} (has_up) and D_l = [d f | d g] of layer l (csrc/srwn_wngate.hip)."""
        B, T, R, S = self.B, self.T, self.R, self.S
        K.wavenet_layer_bwd(g_in, self.dfs[l + 1] if has_up else None,
                            self.wptr(self.o_convT[l + 1]) if has_up else None, self.gs[l + 1] if has_up else None,
                            self.wptr(self.o_resT[l]) if has_up else None,
                            None if self.use_dcs else self.wptr(self.o_skipT[l]), None if self.use_dcs else self.dtotal,
                            self.dcs[l] if self.use_dcs else None, self.zs[l], self.ss[l], self.dfs[l], B, T, R, S,
                            self.Kw, self.dil[l + 1] if has_up else 1, has_up, True, self.dt)

    @property
    def _gate_out(self) -> torch.Tensor:
        """What the skip sum and the 1x1 weight gradients read: z (c rebuilt as z*sigmoid(z) on load), or c (wavenet)."""
        return self.cs if self.wavenet else self.zs

    @property
    def _gate_pro(self) -> int:
        return K.PRO_NONE if self.wavenet else K.PRO_GATE

    def join_side(self):
        if self.side is not None and self.overlap and not self.timing:
            torch.cuda.current_stream().wait_stream(self.side)

    @property
    def fused_bwd(self) -> bool:
        """The data-gradient chain runs as one launch per layer group (needs the precomputed skip gradients `dcs`, or a
        stack without a skip path)."""
        return self.fuse_bwd and self.use_wl and (getattr(self, "use_dcs", False) or self.cfg.head_mode == "flow")

    @property
    def fused_wt(self) -> bool:
        """The layer weight gradients are summed inside the backward group kernel from the forward kernel's weight-gradient
        tiles (no df / G round trip through HBM, no separate weight-gradient pass)."""
        # (not for the flows of the student: they carry no skip path and write every layer's input gradient for the
        # conditioning 1x1 anyway -- measured: their backward gains nothing and their forward pays for the tiles,
        # 7.09 vs 6.77 ms per distillation step -- and not for a stack that is never trained: StudentEngine's teacher)
        return self._fused_wt

    def _group_bwd_wt(self, l0: int, l1: int):
        """Chain + weight-gradient partials of layers [l0, l1) in one launch (srwn_residual_group_bwd_wt)."""
        flow = self.cfg.head_mode == "flow"
        R, ns = self.R, self.nslabs
        g_top = self.gs[l1] if (flow or l1 < self.L) else None
        ic = None
        if l0 == 0 and self.fuse_icg:      # the stack's first group: the input conv's weight-gradient partials ride along
            ic = (self.audio, self.ic_ws, 1 if self.cfg.shift_input else 0)
            sec = self.sections
            self._ic_job = (self.ic_ws, ns * (8 // (R // 16)), (self.Kw + 1) * R, 1, True, 1.0,
                            self.grads.data_ptr() + 4 * sec["init_w"].offset, 0)
        p16 = self.group_p16[self.groups.index((l0, l1))]
        pl_f, pl_r = (self.pl_f, self.pl_r) if p16 or not self.part16 else (self.pl_f32, self.pl_r32)
        with _Span(self, "group_bwd_wt"):
            K.residual_group_bwd_wt(g_top, self.gs[l0:l1], self.zs[l0:l1], None if flow else self.dcs[l0:l1],
                                    self.xTs[l0:l1], self.cTs[l0:l1],
                                    [self.wptr(self.o_convT[l]) for l in range(l0, l1)],
                                    [self.wptr(self.o_resT[l]) for l in range(l0, l1)], self.dil[l0:l1],
                                    pl_f[l0 * ns * 2 * R * R:], pl_r[l0 * ns * R * R:],
                                    self.pl_bf[l0 * ns * R:], self.pl_br[l0 * ns * R:], ns,
                                    self.wt_seg_rows[self.groups.index((l0, l1))], self.Kw, write_all_g=bool(self.E), ic=ic)

    def _group_bwd(self, l0: int, l1: int):
        flow = self.cfg.head_mode == "flow"
        g_top = self.gs[l1] if (flow or l1 < self.L) else None    # the teacher's last dense output is unused: G_L = 0
        K.residual_group_bwd(g_top, self.gs[l0:l1], self.dfs[l0:l1], self.zs[l0:l1],
                             None if flow else self.dcs[l0:l1],
                             [self.wptr(self.o_convT[l]) for l in range(l0, l1)],
                             [self.wptr(self.o_resT[l]) for l in range(l0, l1)], self.dil[l0:l1], self.Kw,
                             seg_rows=self.seg_rows)

    def _wl_groups(self):
        import os as _os
        if self.fused_bwd:
            return list(self.groups)
        per = int(_os.environ.get("SRWN_WL_GROUP", "6"))
        return [(l0, min(l0 + per, self.L)) for l0 in range(0, self.L, per)]

    @property
    def split_layer(self) -> int:
        """Where the two-part backward is cut: the layer-group boundary nearest 40 % of the depth (the part above it
        outlasts the skip/head weight-gradient kernels running beside it)."""
        los = [g[0] for g in self._wl_groups() if 0 < g[0] < self.L]
        return min(los, key=lambda v: abs(v - 0.4 * self.L)) if los else 0

    @property
    def contrastive(self) -> bool:
        return self.cfg.head_mode == "contrastive"

    @property
    def clip_head(self) -> bool:
        """One output row per clip (the pooled softmax or the contrastive embedding): the head runs on the time-mean of
        r1, writes the last 1x1's gradients itself, and its backward broadcasts one row over time."""
        return self.cfg.head_mode in ("pooled", "contrastive")

    @property
    def bucket_off(self) -> int:
        return self.sections["WS"].offset

    @property
    def bucketed(self) -> bool:
        """Two all-reduce buckets, the first overlapped with the lower part of the backward pass (needs the grouped
        weight-gradient path and a deep enough stack)."""
        import os as _os
        forced = _os.environ.get("SRWN_FORCE_DIST") == "1"
        mode = _os.environ.get("SRWN_BUCKETS", "auto")   # "0" off, "1" on, "auto": on for RCCL only (gloo's
        if mode == "0" or not ((self.world > 1 or forced) and self.use_wl and self.split_layer > 0 and not self.clip_head):
            return False                                 # asynchronous CUDA all-reduce stalls for tens of ms)
        if mode == "1":
            return True
        import torch.distributed as dist
        return dist.is_initialized() and dist.get_backend(self.pg) == "nccl"

    def _bwd_head(self):
        B, T, N, S, Cp = self.B, self.T, self.N, self.S, self.Cp
        if self._head_bwd_done:     # da1, dtotal came out of the forward's head launch
            return
        with _Span(self, "bwd_head"):   # relu masks against the saved activations
            if self.clip_head:
                from ._lib import call
                call("srwn_bcast_mask", self.dmean.data_ptr(), self.r1.data_ptr(), self.da1.data_ptr(), B, T, S,
                     1.0 / T, K.abi_dtype(self.dt), torch.cuda.current_stream().cuda_stream)
            else:
                K.pw_linear(self.dlogits.data_ptr(), Cp, 0, Cp, Cp, self.wptr(self.o_w2T), None, self.da1, S, S, N,
                            aux=self.r1, epi=K.EPI_MASK)
            K.pw_linear(self.da1.data_ptr(), S, 0, S, S, self.wptr(self.o_w1T), None, self.dtotal, S, S, N,
                        aux=self.r0, epi=K.EPI_MASK)

    def _wgrad_layers_group(self, l0: int, l1: int):
        """conv taps + 1x1 residual of layers [l0, l1) in one pass over x, z, df, G."""
        N, L, R, T, ns = self.N, self.L, self.R, self.T, self.nslabs
        es = self.xs.element_size()
        NR = N * R
        ckw = {}   # (xs already holds the conditioned inputs)
        with _Span(self, "wgrad_layers"):
            K.wgrad_layers(self.xs.view(L + 1, N, R)[l0:l1], self.zs.view(L, N, R)[l0:l1],
                           self.dfs.view(L, N, R)[l0:l1], self.gs.data_ptr() + (l0 + 1) * NR * es, self.dil[l0:l1],
                           self.pl_f[l0 * ns * 2 * R * R:], self.pl_r[l0 * ns * R * R:], self.pl_bf[l0 * ns * R:],
                           self.pl_br[l0 * ns * R:], T, ns, **ckw)

    def _wgrad_layers_finish(self):
        L, R, S, Kw, N, T = self.L, self.R, self.S, self.Kw, self.N, self.T
        gp, sec, ns, dt = self.grads.data_ptr(), self.sections, self.nslabs, self.dt
        es = self.xs.element_size()
        NR = N * R
        xs_p, dfs_p, gs_p = self.xs.data_ptr(), self.dfs.data_ptr(), self.gs.data_ptr()
        if self.use_wl:
            # runs of layers whose groups keep their partials in one format (one run unless a group fell back to fp32)
            runs = []
            for (l0, l1), p16 in zip(self.groups, self.group_p16) if self.group_p16 else [((0, L), False)]:
                if runs and runs[-1][2] == p16:
                    runs[-1][1] = l1
                else:
                    runs.append([l0, l1, p16])
            jf, jr = [], []
            for l0, l1, p16 in runs:
                pl_f, pl_r = (self.pl_f, self.pl_r) if p16 or not self.part16 else (self.pl_f32, self.pl_r32)
                blk = (R,) if p16 else ()      # (bf16 partial blocks in lane order: SRWN_PARTIALS_BLK16, R columns)
                jf.append((pl_f[l0 * ns * Kw * R * R:], ns, Kw * R * R, l1 - l0, True, 1.0,
                           gp + 4 * (sec["WF"].offset + l0 * Kw * R * R), Kw * R * R) + blk)
                jr.append((pl_r[l0 * ns * R * R:], ns, R * R, l1 - l0, True, SQRT_HALF,
                           gp + 4 * (sec["WR"].offset + l0 * R * R), R * R) + blk)
            jobs = jf + [(self.pl_bf, ns, R, L, True, 1.0, gp + 4 * sec["BF"].offset, R)] + jr + [
                (self.pl_br, ns, R, L, True, SQRT_HALF, gp + 4 * sec["BR"].offset, R)]
            if self._ic_job is not None:      # the input conv's kernel + bias gradient (init_w | init_b are adjacent)
                jobs.append(self._ic_job)
                self._ic_job = None
            K.reduce_partials_multi(jobs)
            return
        if self.wavenet:
            self._wgrad_wavenet_convs()
        else:
            for k in range(Kw):                              # dilated conv taps (legacy)
                shifts = [(Kw - 1 - k) * d for d in self.dil]
                last = k == Kw - 1
                K.wgrad(xs_p, NR, R, dfs_p, NR, R, shifts, L, self.wg_parts, self.wg_bparts if last else None, N, T, ns,
                        dt)                                  # (xs holds the conditioned conv inputs, model.py:183)
                K.reduce_partials(self.wg_parts, ns, R * R, L, True, 1.0, gp + 4 * (sec["WF"].offset + k * R * R),
                                  Kw * R * R)
                if last:
                    K.reduce_partials(self.wg_bparts, ns, R, L, True, 1.0, gp + 4 * sec["BF"].offset, R)
        K.wgrad(self._gate_out.data_ptr(), NR, R, gs_p + NR * es, NR, R, None, L, self.wg_parts, self.wg_bparts, N, T,
                ns, dt, pro=self._gate_pro)                                           # 1x1 residual
        K.reduce_partials(self.wg_parts, ns, R * R, L, True, SQRT_HALF, gp + 4 * sec["WR"].offset, R * R)
        K.reduce_partials(self.wg_bparts, ns, R, L, True, SQRT_HALF, gp + 4 * sec["BR"].offset, R)

    def _wgrad_wavenet_convs(self):
        """Both dilated convs of every layer (canonical gate): per tap one srwn_wgrad over (x_l, D_l) with cin = R,
        cout = 2R, reduced into [L, K, R, 2R] / [L, 2R] and split into the WF | WG and BF | BG sections."""
        L, R, Kw, N, T, ns = self.L, self.R, self.Kw, self.N, self.T, self.nslabs
        NR = N * R
        for k in range(Kw):
            last = k == Kw - 1
            K.wgrad(self.xs.data_ptr(), NR, R, self.dfs.data_ptr(), 2 * NR, 2 * R, [(Kw - 1 - k) * d for d in self.dil], L,
                    self.wg_parts, self.wg_bparts if last else None, N, T, ns, self.dt)
            K.reduce_partials(self.wg_parts, ns, R * 2 * R, L, True, 1.0,
                              self.wn_wgrad.data_ptr() + 4 * k * R * 2 * R, Kw * R * 2 * R)
            if last:
                K.reduce_partials(self.wg_bparts, ns, 2 * R, L, True, 1.0, self.wn_bgrad.data_ptr(), 2 * R)
        g = self.grads
        self.view("WF", g).copy_(self.wn_wgrad[..., :R]); self.view("WG", g).copy_(self.wn_wgrad[..., R:])
        self.view("BF", g).copy_(self.wn_bgrad[:, :R]); self.view("BG", g).copy_(self.wn_bgrad[:, R:])

    def _wgrad_skip_and_head(self):
        """Gradients of the skip 1x1s and the two head 1x1s: need only z, r0, r1, da1, dtotal, dlogits."""
        N, T, L, R, S, Cp = self.N, self.T, self.L, self.R, self.S, self.Cp
        gp, sec, ns, dt = self.grads.data_ptr(), self.sections, self.nslabs, self.dt
        NR = N * R
        zs_p = self._gate_out.data_ptr()      # (z, gated on load, or the canonical gate's c)
        if self.batch_reduce:
            ns_skip = self.ns_skip
            with _Span(self, "wgrad_skip"):
                if self.skip_wt and self.fused_wt:
                    ns_skip = self.ns_skip_wt
                    K.wgrad_skip_wt(self.cTs, self.wt_layer_st, self.wt_layer_seg, self.dtotal,
                                    self.wg_parts if self.skip_parts16 is None else self.skip_parts16,
                                    self.wg_bparts, ns_skip, self.B, T, R)
                else:
                    K.wgrad256(zs_p, NR, R, L, self.dtotal, self.wg_parts, self.wg_bparts, N, self.ns_skip,
                               pro=self._gate_pro, chunk_width=R)
            if S == Cp:   # both head 1x1s (S->S, S->C) as one launch
                K.wgrad256_pair(self.r0.data_ptr(), self.da1, self.hd_parts[0], self.hd_bparts[0],
                                self.r1.data_ptr(), self.dlogits, self.hd_parts[1], self.hd_bparts[1], 64, S, S // 64, N,
                                self.ns_head)
            else:
                K.wgrad256(self.r0.data_ptr(), 64, S, S // 64, self.da1, self.hd_parts[0], self.hd_bparts[0], N, self.ns_head)
                K.wgrad256(self.r1.data_ptr(), 64, S, S // 64, self.dlogits, self.hd_parts[1], self.hd_bparts[1], N,
                           self.ns_head)
            skip16 = self.skip_wt and self.fused_wt and self.skip_parts16 is not None
            jobs = [
                (self.skip_parts16, ns_skip, L * R * S, 1, True, 1.0, gp + 4 * sec["WS"].offset, 0, S) if skip16 else
                (self.wg_parts, ns_skip, L * R * S, 1, True, 1.0, gp + 4 * sec["WS"].offset, 0),
                (self.wg_bparts, ns_skip, S, L, False, 1.0, gp + 4 * sec["BS"].offset, S),
                (self.hd_parts[0], self.ns_head, S * S, 1, True, 1.0, gp + 4 * sec["head_w1"].offset, 0),
                (self.hd_bparts[0], self.ns_head, S, 1, True, 1.0, gp + 4 * sec["head_b1"].offset, 0),
                (self.hd_parts[1], self.ns_head, S * Cp, 1, True, 1.0, gp + 4 * sec["head_w2"].offset, 0),
                (self.hd_bparts[1], self.ns_head, Cp, 1, True, 1.0, gp + 4 * sec["head_b2"].offset, 0)]
            if self._loss_job is not None:      # the loss the forward pass deferred: one more (one-output) reduction
                jobs.append(self._loss_job)
                self._loss_job = None
            K.reduce_partials_multi(jobs)
            return
        if self.use_w256:
            # every skip 1x1 at once: out[L*R, S] = c_all^T . dtotal (dtotal re-read once per 4 layers)
            ns_skip = self.ns_skip
            with _Span(self, "wgrad_skip"):
                if self.skip_wt and self.fused_wt:
                    ns_skip = self.ns_skip_wt
                    K.wgrad_skip_wt(self.cTs, self.wt_layer_st, self.wt_layer_seg, self.dtotal,
                                    self.wg_parts if self.skip_parts16 is None else self.skip_parts16,
                                    self.wg_bparts, ns_skip, self.B, T, R)
                else:
                    K.wgrad256(zs_p, NR, R, L, self.dtotal, self.wg_parts, self.wg_bparts, N, self.ns_skip,
                               pro=self._gate_pro, chunk_width=R)
            if self.skip_wt and self.fused_wt and self.skip_parts16 is not None:
                K.reduce_partials_multi([(self.skip_parts16, ns_skip, L * R * S, 1, True, 1.0, gp + 4 * sec["WS"].offset, 0, S)])
            else:
                K.reduce_partials(self.wg_parts, ns_skip, L * R * S, 1, True, 1.0, gp + 4 * sec["WS"].offset, 0)
            K.reduce_partials(self.wg_bparts, ns_skip, S, L, False, 1.0, gp + 4 * sec["BS"].offset, S)
            K.wgrad256(self.r0.data_ptr(), 64, S, S // 64, self.da1, self.wg_parts, self.wg_bparts, N, self.ns_head)
            K.reduce_partials(self.wg_parts, self.ns_head, S * S, 1, True, 1.0, gp + 4 * sec["head_w1"].offset, 0)
            K.reduce_partials(self.wg_bparts, self.ns_head, S, 1, True, 1.0, gp + 4 * sec["head_b1"].offset, 0)
        else:
            with _Span(self, "wgrad_skip"):
                K.wgrad(zs_p, NR, R, self.dtotal.data_ptr(), 0, S, None, L, self.wg_parts, self.wg_bparts, N, T, ns,
                        dt, pro=self._gate_pro)                                       # 1x1 skip
            K.reduce_partials(self.wg_parts, ns, R * S, L, True, 1.0, gp + 4 * sec["WS"].offset, R * S)
            K.reduce_partials(self.wg_bparts, ns, S, L, True, 1.0, gp + 4 * sec["BS"].offset, S)
            K.wgrad(self.r0.data_ptr(), 0, S, self.da1.data_ptr(), 0, S, None, 1, self.wg_parts, self.wg_bparts, N, T,
                    ns, dt)                                                           # head 1x1 (S->S)
            K.reduce_partials(self.wg_parts, ns, S * S, 1, True, 1.0, gp + 4 * sec["head_w1"].offset, 0)
            K.reduce_partials(self.wg_bparts, ns, S, 1, True, 1.0, gp + 4 * sec["head_b1"].offset, 0)
        if self.use_w256 and not self.clip_head and Cp == 256:
            K.wgrad256(self.r1.data_ptr(), 64, S, S // 64, self.dlogits, self.wg_parts, self.wg_bparts, N,
                       self.ns_head)                                                  # last 1x1 (S->C)
            K.reduce_partials(self.wg_parts, self.ns_head, S * Cp, 1, True, 1.0, gp + 4 * sec["head_w2"].offset, 0)
            K.reduce_partials(self.wg_bparts, self.ns_head, Cp, 1, True, 1.0, gp + 4 * sec["head_b2"].offset, 0)
        elif not self.clip_head:   # (the pooled and contrastive heads wrote their own kernel/bias gradients in forward)
            K.wgrad(self.r1.data_ptr(), 0, S, self.dlogits.data_ptr(), 0, Cp, None, 1, self.wg_parts, self.wg_bparts,
                    N, T, ns, dt)                                                     # last 1x1 (S->C)
            K.reduce_partials(self.wg_parts, ns, S * Cp, 1, True, 1.0, gp + 4 * sec["head_w2"].offset, 0)
            K.reduce_partials(self.wg_bparts, ns, Cp, 1, True, 1.0, gp + 4 * sec["head_b2"].offset, 0)

    def _wgrad_input_conv_partials(self):
        """Stage 1 of the input conv's weight gradient (model.py:40): per-slab partial sums from gs[0]; its slab
        reduction rides in the final srwn_reduce_partials_multi launch (it was a launch of its own)."""
        sec = self.sections
        assert sec["init_b"].offset == sec["init_w"].offset + sec["init_w"].numel
        nsl = K.init_conv_wgrad(self.audio, self.gs[0], None, None, self.Kw, 1 if self.cfg.shift_input else 0, self.ic_ws)
        self._ic_job = (self.ic_ws, nsl, (self.Kw + 1) * self.R, 1, True, 1.0,
                        self.grads.data_ptr() + 4 * sec["init_w"].offset, 0)

    def _wgrad_input_and_cond(self, input_conv: bool = True):
        B, T, L, R, Kw = self.B, self.T, self.L, self.R, self.Kw
        g = self.grads
        gp, sec, dt = g.data_ptr(), self.sections, self.dt
        if input_conv:
            K.init_conv_wgrad(self.audio, self.gs[0], self.view("init_w", g).reshape(-1), self.view("init_b", g), Kw,
                              1 if self.cfg.shift_input else 0, self.ic_ws)
        if self.E:
            # conditioning 1x1 (model.py:180): dcb_l = adjoint of the NN upsample applied to G_l
            rows_c, Ep, E = B * self.frames, self.Ep, self.E
            from ._lib import call
            call("srwn_frame_sum_batched", self.gs.data_ptr(), B * T * R, self.dcb.data_ptr(), rows_c * R, L, B, T, R,
                 self.frames, self.cfg.pool_stride, 1.0, K.abi_dtype(dt), torch.cuda.current_stream().cuda_stream)
            K.wgrad(self.cond_in.data_ptr(), 0, Ep, self.dcb.data_ptr(), rows_c * R, R, None, L, self.wgc_parts,
                    self.wgc_bparts, rows_c, self.frames, self.nslabs_c, dt)
            if Ep == E:
                K.reduce_partials(self.wgc_parts, self.nslabs_c, Ep * R, L, True, 1.0, gp + 4 * sec["WC"].offset, E * R)
            else:
                K.reduce_partials(self.wgc_parts, self.nslabs_c, Ep * R, L, True, 1.0, self.wc_grad_pad.data_ptr(),
                                  Ep * R)
                self.view("WC", g).copy_(self.wc_grad_pad[:, :E, :])
            K.reduce_partials(self.wgc_bparts, self.nslabs_c, R, L, True, 1.0, gp + 4 * sec["BC"].offset, R)

    # ------------------------------------------------------------------------------------------
    # update
    # ------------------------------------------------------------------------------------------
    def allreduce_grads(self):
        """Data parallel: sum the flat gradient over ranks (RCCL over xGMI); Adam divides by world."""
        dp.allreduce_sum_(self.grads, self.pg)

    def optimizer_step(self):
        self._adam_update()
        self.repack()

    def _adam_update(self, joint_clip: bool = False):
        """The update launches.  No controls: srwn_adam_step at the configured rate.  Controls (``set_controls``):
        [srwn_sumsq -> srwn_clip_scale ->] srwn_adam_step_ctl.  `joint_clip`: the owner of several buffers has left the
        clip factor of their joint norm in ``self.clip`` already (encoder.AutoEncoderEngine)."""
        # mean losses: mean of shard gradients; the mixture-of-logistics loss is a SUM over batch and time
        # (ops.py:173-174), so shard gradients simply add
        grad_scale = 1.0 if self.mol else 1.0 / self.world
        c = self.ctl
        if c.controls is not None and c.clip is not None:
            if not joint_clip:      # the norm of the gradient Adam would use: behind the 1 / world of a mean loss
                K.sumsq(self.grads, c.sq_parts)
                K.clip_scale(c.sq_parts, c.controls.clip_norm, grad_scale, c.clip)
            grad_scale = 1.0
        adam_update(c, self.params, self.grads, self.adam_m, self.adam_v, self.adam_step, self.cfg.learning_rate,
                    grad_scale, c.clip)

    # ------------------------------------------------------------------------------------------
    # training controls: learning-rate table, gradient clipping, EMA weights (optim.py)
    # ------------------------------------------------------------------------------------------
    @property
    def clip(self) -> Optional[torch.Tensor]:
        """float32 [2] on the device: the last step's clip factor (times the loss's 1 / world) and gradient norm; None
        without clipping."""
        return self.ctl.clip

    @property
    def ema(self) -> Optional[torch.Tensor]:
        """The EMA shadow, flat fp32 like ``params`` (None without one).  Inside ``swap_ema`` it holds the raw weights."""
        return self.ctl.ema

    def set_controls(self, controls):
        """Installs an ``optim.TrainControls`` (None: back to the fixed rate) for this engine and every engine sharing its
        parameters.  The same features (clipping on / off and its bound, EMA on / off), a horizon inside the allocated table:
        the table and its length are rewritten in place and captured graphs follow.  Any other change drops the captured graphs
        of ``train`` and ``fit``; the usual rule captures them again."""
        if self.ctl.set(controls, self.params):
            self.ctl.drop_graphs()

    def _reset_ema(self):
        ctl = getattr(self, "ctl", None)      # (init_parameters runs before the holder exists)
        if ctl is not None:
            ctl.reset_ema(self.params)

    def swap_ema(self):
        """Exchanges the CONTENTS of ``params`` and the EMA shadow (the kernels read biases through views of ``params``,
        so the pointers stay) through one scratch buffer, then rebuilds the weight images.  Three copies and two gathers
        on the current stream: capturable.  Twice is the identity."""
        swap_with_ema(self.ctl, self.params)
        self.repack()
        self._repack_generation()

    def _allreduce_bucket_a(self):
        """Skip + head gradients: issued while the lower part of the backward pass runs."""
        return dp.allreduce_sum_(self.grads[self.bucket_off:], self.pg, async_op=True)

    def _allreduce_bucket_b(self, pending):
        dp.allreduce_sum_(self.grads[:self.bucket_off], self.pg)
        if pending is not None:
            pending.wait()

    def train_step(self) -> torch.Tensor:
        """fwd + bwd + (all-reduce) + Adam on the staged inputs; returns the device loss scalar.
        With several ranks the gradient all-reduce runs in two buckets, the first (skip + head kernels, 65 % of the
        bytes) overlapped with the lower part of the backward pass."""
        self.forward(defer_loss=True)
        if self.bucketed and not self.timing:
            self.backward(part=1)
            h = self._allreduce_bucket_a()
            self.backward(part=2)
            self._allreduce_bucket_b(h)
        else:
            self.backward()
            self.allreduce_grads()
        self.optimizer_step()
        return self.loss

    # ------------------------------------------------------------------------------------------
    # generation: what generate, generation_state / generate_chunk and the pools share
    # ------------------------------------------------------------------------------------------
    def _check_generates(self):
        """What every way into generation refuses first (reads wavenet, o_gen and cfg.head_mode only)."""
        if self.wavenet:
            raise NotImplementedError("generate: gate_mode 'wavenet' is trained only; the generation kernels implement "
                                      "the reference gate (canonical generation is not built)")
        if self.o_gen is None or self.clip_head:
            raise NotImplementedError("generate: built for R=64 or 32, S=256 or 128, K=2 stacks with a per-time-step head")

    def _refuse_conditioned_softmax(self, cond=None):
        """The softmax teacher with conditioning channels, or handed an encoding (reads mol and E only)."""
        if not self.mol and (self.E or cond is not None):
            raise NotImplementedError("generate: the conditioned softmax teacher is not built (the conditioned "
                                      "decoder of the reference has the mixture-of-logistics head)")

    def _gen16(self) -> bool:
        """Whether a launch runs the latency body (csrc/srwn_gen16.hip) rather than the throughput body (csrc/srwn_gen.hip):
        where its images were built, unless SRWN_GEN16=0.  Read at every launch (the parity tests flip it on one engine)."""
        return self.o_g16 is not None and _os.environ.get("SRWN_GEN16", "1") != "0"

    def _gen_dilations(self):
        """The dilations as the int32 array the generators' entry points take."""
        return (ctypes.c_int32 * self.L)(*self.dil)

    def _gen_ring(self, n: int) -> torch.Tensor:
        """The zeroed layer rings of n streams (one set per group of 32)."""
        from . import _lib
        relems = int(_lib.load().srwn_generate_ring_elems(self._gen_dilations(), self.L, self.R))
        return torch.zeros(relems * ((n + 31) // 32), dtype=self.dt, device=self.dev)

    def _gen_outputs(self, rows: int, nsteps: int, want_logits: bool, forced, rows_name: str = "batch"):
        """One launch's zeroed outputs -- audio [rows, nsteps] f32, codes [rows, nsteps] i32, logits [rows, nsteps, C] f32 or
        None -- and `forced` as the [rows, nsteps] f32 device tensor the kernels read (None: free running)."""
        audio = torch.zeros((rows, nsteps), dtype=torch.float32, device=self.dev)
        codes = torch.zeros((rows, nsteps), dtype=torch.int32, device=self.dev)
        logits = torch.zeros((rows, nsteps, self.C), dtype=torch.float32, device=self.dev) if want_logits else None
        if forced is not None:
            forced = torch.as_tensor(forced).to(device=self.dev, dtype=torch.float32).contiguous()
            if tuple(forced.shape) != (rows, nsteps):
                raise ValueError("forced must be [%s, nsteps]" % rows_name)
        return audio, codes, logits, forced

    def _project_cond(self, enc: torch.Tensor) -> torch.Tensor:
        """Encoding rows [rows, cond_channels] -> the conditioning biases of every layer [rows, L*R] (model.py:180): the
        rows padded to the Ep columns of the packed kernel, one pw_linear."""
        rows, LR = enc.shape[0], self.L * self.R
        cin = torch.zeros((rows, self.Ep), dtype=self.dt, device=self.dev)
        cin[:, :self.E].copy_(enc)
        out = torch.empty((rows, LR), dtype=self.dt, device=self.dev)
        K.pw_linear(cin.data_ptr(), self.Ep, 0, self.Ep, self.Ep, self.wptr(self.o_wc), self.view("BC").reshape(-1), out,
                    LR, LR, rows)
        return out

    # the general forms of the C ABI, [latency body][mixture-of-logistics head][slot form]: with t0 = 0, a NULL carry and
    # NULL sampling they run the kernels of the plain calls, so every launch goes through one of these eight
    _GEN_ENTRY = ((("srwn_generate_resume_sampled", "srwn_generate_slots_sampled"),
                   ("srwn_generate_mol_resume_sampled", "srwn_generate_mol_slots_sampled")),
                  (("srwn_generate16_resume_sampled", "srwn_generate16_slots_sampled"),
                   ("srwn_generate16_mol_resume_sampled", "srwn_generate16_mol_slots_sampled")))

    def _launch_generation(self, ring, audio, codes, logits, forced, batch, nsteps, mode, seed, t0, carry, sampling,
                           cond_all, frames, slots=None, live=False):
        """THE launch of the queue-cached generators: `nsteps` steps from absolute step t0 for `batch` streams over `ring`
        into audio / codes / logits (None: not kept), teacher-forced where `forced` is given.  carry [batch, 2] (None with
        t0 = 0: none read, none written), sampling: the SrwnGenSampling device array or None, cond_all [batch * frames,
        L*R] or None.  `slots` (a pool's SrwnGenSlot table) selects the slot form: t0 is then the pool's clock and the
        seeds are the slots'.  `live` (a LiveGenerationState's launch): cond_all is a ring of `frames` frames per stream and
        the live entry point runs.  The argument list is srwn.h's, built once from its blocks."""
        from . import _lib
        ptr = lambda t: None if t is None else t.data_ptr()
        v, g16 = self.view, self._gen16()
        if g16:
            weights = (self.wptr(self.o_g16), self.wptr(self.o_g16_h1), self.wptr(self.o_g16_h2))
        else:
            weights = (self.wptr(self.o_gen), self.wptr(self.o_skip_gen), self.wptr(self.o_w1), self.wptr(self.o_w2))
        shared = (v("BF").data_ptr(), v("BR").data_ptr(), self.bs_sum.data_ptr(), v("head_b1").data_ptr(),
                  v("head_b2").data_ptr(), v("init_w").data_ptr(), v("init_b").data_ptr(), ring.data_ptr(),
                  audio.data_ptr(), codes.data_ptr(), ptr(logits), ptr(forced), self._gen_dilations(), self.L, batch,
                  nsteps, nsteps, self.R, self.S)
        # the throughput body alone takes the filter width (after C, before num_mixtures) and the dtype (before the stream)
        kw, dtype = ((), ()) if g16 else ((self.Kw,), (K.abi_dtype(self.dt),))
        if self.mol:
            head = kw + (self.C // 4, ptr(cond_all), frames if cond_all is not None else 1, self.cfg.pool_stride,
                         self.L * self.R)
        else:
            head = (self.C,) + kw
        md = {"argmax": 0, "mean": 0, "sample": 1}[mode]
        st = torch.cuda.current_stream().cuda_stream
        if slots is None:
            tail = (md, int(seed)) + dtype + (st, t0, ptr(carry))
        else:
            tail = (md,) + dtype + (st, t0, carry.data_ptr(), slots.data_ptr())
        entry = self._GEN_ENTRY[g16][bool(self.mol)][slots is not None]
        if live:      # the live forms (srwn_version() 112, 114) are named after their *_mol_{resume,slots}_sampled twins
            entry = entry.replace("_resume_", "_live_").replace("_slots_", "_live_slots_")
        _lib.call(entry, *weights, *shared, *head, *tail, ptr(sampling))

    def generate(self, nsteps: int, mode: str = "sample", seed: int = 0, forced: Optional[torch.Tensor] = None,
                 want_logits: bool = False, batch: Optional[int] = None, cond: Optional[torch.Tensor] = None, *,
                 temperature=1.0, top_k=0, top_p=1.0):
        """Queue-cached autoregressive generation of `nsteps` samples for `batch` utterances.
        temperature / top_k / top_p (mode "sample"): the sampling controls of srwn.h's SrwnGenSampling, each a scalar or one
        entry per utterance (sampling_table); the defaults are the plain draw.
        Softmax teacher: returns (audio [B,nsteps] f32, mu-law codes [B,nsteps] i32, logits [B,nsteps,C] f32 or None).
        Mixture-of-logistics decoder (head_mode "mol"; `cond` = encoding_w_condition [B, frames, cond_channels] when the
        stack is conditioned): returns (audio, selected mixture, logits [B,nsteps,4M])."""
        self._check_generates()
        B = int(batch or self.B)
        samp = None
        if self.mol or not (self.E or cond is not None):      # (the conditioned softmax teacher is refused below)
            samp = sampling_table(B, temperature, top_k, top_p, self.C, self.mol, "generate")
        self._repack_generation()      # (the generation-only images follow the parameters lazily: not part of a training step)
        ring = self._gen_ring(B)
        audio, codes, logits, forced = self._gen_outputs(B, nsteps, want_logits, forced)
        self._refuse_conditioned_softmax(cond)
        cond_all, frames = None, 1
        if self.E:
            if cond is None:
                raise ValueError("this decoder is conditioned: pass cond [batch, frames, cond_channels]")
            cond = cond.to(device=self.dev, dtype=torch.float32)
            frames = cond.shape[1]
            if tuple(cond.shape) != (B, frames, self.E) or frames * self.cfg.pool_stride < nsteps:
                raise ValueError("cond must be [batch, frames >= nsteps/pool_stride, %d]" % self.E)
            cond_all = self._project_cond(cond.reshape(B * frames, self.E))
        elif cond is not None:
            raise ValueError("this decoder is not conditioned")
        # one launch from step 0: no carry to read (t0 = 0) and none written (NULL); the state of a run is generation_state's
        self._launch_generation(ring, audio, codes, logits, forced, B, nsteps, mode, seed, 0, None,
                                None if samp is None else _sampling_to_device(samp, self.dev), cond_all, frames)
        return audio, codes, logits

    # ------------------------------------------------------------------------------------------
    # resumable generation: streaming, chunks, prompts
    # ------------------------------------------------------------------------------------------
    def generation_state(self, batch: int, cond: Optional[torch.Tensor] = None, seed: int = 0, *, temperature=1.0,
                         top_k=0, top_p=1.0) -> "GenerationState":
        """A generation run of `batch` utterances that `generate_chunk` advances chunk by chunk and `prime` can start from a
        prompt: the layer rings, the carry (the last two input samples, [B, 2] fp32), the absolute step t, the seed and,
        for a conditioned decoder, the per-layer conditioning (`cond` = encoding_w_condition [B, frames, cond_channels]).
        temperature / top_k / top_p: the run's sampling controls (as `generate`), kept in the state for every chunk.
        The generation weight images are gathered here: train between chunks and the run keeps the weights it started
        with (make a new state to pick up new ones)."""
        self._check_generates()
        B = int(batch)
        if B < 1:
            raise ValueError("generation_state: batch %d" % B)
        samp = None
        if self.mol or not (self.E or cond is not None):      # (the conditioned softmax teacher is refused below)
            samp = sampling_table(B, temperature, top_k, top_p, self.C, self.mol, "generation_state")
        self._refuse_conditioned_softmax(cond)
        cond_all, frames = None, 0
        if self.E:
            if cond is None:
                raise ValueError("this decoder is conditioned: pass cond [batch, frames, cond_channels]")
            cond = cond.to(device=self.dev, dtype=torch.float32).contiguous()
            frames = int(cond.shape[1]) if cond.dim() == 3 else 0
            if cond.dim() != 3 or tuple(cond.shape) != (B, frames, self.E) or frames < 1:
                raise ValueError("cond must be [batch, frames, %d]" % self.E)
            cond_all = self._project_cond(cond.reshape(B * frames, self.E))
        elif cond is not None:
            raise ValueError("this decoder is not conditioned")
        self._repack_generation()
        ring = self._gen_ring(B)
        carry = torch.zeros((B, 2), dtype=torch.float32, device=self.dev)
        return GenerationState(B, ring, carry, int(seed), cond if frames else None, cond_all, frames,
                               frames * self.cfg.pool_stride if frames else None,
                               None if samp is None else _sampling_to_device(samp, self.dev))

    def live_generation_state(self, batch: int, max_frames: int, seed: int = 0, *, temperature=1.0) -> "LiveGenerationState":
        """A generation run of the conditioned mixture-of-logistics decoder whose encoding is FED while it runs (`feed`):
        the state of `generation_state` with a zeroed conditioning ring of `max_frames` frames per stream and fed = 0.
        `generate_chunk` advances it up to fed * pool_stride, `prime` starts it (at t = 0) from a prompt over the frames fed
        by then; the samples are those of `generate` over the whole encoding with the same seed and temperature."""
        self._check_generates()
        self._refuse_conditioned_softmax()
        if not self.E:
            raise ValueError("this decoder is not conditioned")
        B, F = int(batch), int(max_frames)
        if B < 1 or F < 1:
            raise ValueError("live_generation_state: batch %d, max_frames %d" % (B, F))
        samp = sampling_table(B, temperature, 0, 1.0, self.C, True, "live_generation_state")
        self._repack_generation()
        LR = self.L * self.R
        return LiveGenerationState(B, self._gen_ring(B), torch.zeros((B, 2), dtype=torch.float32, device=self.dev),
                                   int(seed), torch.zeros((B * F, LR), dtype=self.dt, device=self.dev), F,
                                   None if samp is None else _sampling_to_device(samp, self.dev),
                                   torch.zeros((B * F, self.Ep), dtype=self.dt, device=self.dev),
                                   torch.empty((B * F, LR), dtype=self.dt, device=self.dev))

    def feed(self, state: "LiveGenerationState", frames: torch.Tensor) -> None:
        """The next k frames of every stream of a live state: frames [B, k, cond_channels] (encoding_w_condition), a device
        tensor taken as it is.  Refuses (ValueError, before any device work, state untouched) k > `live_decode_room`.  The
        rows are `_project_cond`'s (the same srwn_pw_linear over the same image, so the bits of the one-shot table) in a
        staging buffer, scattered into the ring by ONE srwn_cond_ring_scatter however many streams; afterwards
        `generate_chunk` may run up to fed * pool_stride."""
        from . import _lib
        if not state.live:
            raise ValueError("feed: this state got its whole encoding at generation_state (live_generation_state begins "
                             "a live one)")
        fr = torch.as_tensor(frames)
        B, pool = state.batch, self.cfg.pool_stride
        if fr.dim() != 3 or fr.shape[0] != B or fr.shape[2] != self.E:
            raise ValueError("feed: frames must be [%d, k, %d], got %s" % (B, self.E, tuple(fr.shape)))
        k = int(fr.shape[1])
        if k == 0:
            return
        room = live_decode_room(state.max_frames, state.fed, state.t, pool)
        if k > room:
            raise ValueError("feed: %d frames, but the ring of %d has room for %d at t = %d with %d fed"
                             % (k, state.max_frames, room, state.t, state.fed))
        fr = fr.to(device=self.dev, dtype=torch.float32)
        LR, rows = self.L * self.R, B * k
        state.stage_in[:rows, :self.E].copy_(fr.reshape(rows, self.E))
        K.pw_linear(state.stage_in.data_ptr(), self.Ep, 0, self.Ep, self.Ep, self.wptr(self.o_wc),
                    self.view("BC").reshape(-1), state.stage_out[:rows], LR, LR, rows)
        _lib.call("srwn_cond_ring_scatter", state.stage_out.data_ptr(), LR, state.cond_all.data_ptr(), LR, B, k,
                  state.fed, state.max_frames, LR, K.abi_dtype(self.dt), torch.cuda.current_stream().cuda_stream)
        if state.t == 0:      # (what `prime` needs: the raw frames of a run that has not started)
            state.cond = fr.contiguous() if state.cond is None else torch.cat([state.cond, fr], dim=1)
        state.fed += k
        state.limit = state.fed * pool

    def generation_pool(self, capacity: int, frames: Optional[int] = None, *, live: bool = False) -> "GenerationPool":
        """A pool of `capacity` generation slots that streams join and leave while it runs (GenerationPool); `frames` = the
        most conditioning frames a stream of a conditioned decoder brings.  Refuses, before any device work, what
        `generate` refuses.  The generation weight images are gathered here: the pool keeps the weights it started with.
        live=True (the conditioned mixture-of-logistics decoder only, refused otherwise as `live_generation_state` does):
        `frames` is the length of every slot's conditioning ring and streams may ``join(..., live=True)`` to be fed while
        they run; bounded streams still join such a pool.  A pool made without it runs the launches it always ran."""
        self._check_generates()
        self._refuse_conditioned_softmax()
        if live and not (self.mol and self.E):
            raise ValueError("this decoder is not conditioned: a live pool feeds the conditioned mixture-of-logistics "
                             "decoder")
        if int(capacity) < 1:
            raise ValueError("generation_pool: capacity %d" % int(capacity))
        if self.mol and self.E:
            if frames is None or int(frames) < 1:
                raise ValueError("this decoder is conditioned: pass frames, the most encoding frames of a stream")
        elif frames is not None:
            raise ValueError("this decoder is not conditioned: no frames")
        return GenerationPool(self, int(capacity), int(frames or 0), bool(live))

    def _prime_view(self, B: int, T: int) -> "WaveNetEngine":
        """A forward-only (frozen) view of this stack at (B, T), kept for the next prompt of the same shape."""
        v = getattr(self, "_gen_prime_view", None)
        if v is None or (v.B, v.T) != (B, T):
            self._gen_prime_view = None
            v = WaveNetEngine(self.cfg, B, T, self.dev, share_from=self, frozen=True)
            self._gen_prime_view = v
        return v

    def prime(self, state: "GenerationState", prompt: torch.Tensor) -> None:
        """Continues `state` (at t = 0) from a prompt [B, P]: ONE parallel forward pass of the stack over the prompt
        (rounded up to a whole conditioning frame; the causal convs keep the padding out of every x_l[t < P]), its stored
        layer inputs into the rings (srwn_generate_ring_fill), the carry from the prompt's last two samples, t = P.  The
        next chunk's first sample is the one after the prompt."""
        from . import _lib
        prompt = torch.as_tensor(prompt).to(device=self.dev, dtype=torch.float32)
        if prompt.dim() != 2 or prompt.shape[0] != state.batch:
            raise ValueError("prompt must be [batch=%d, P], got %s" % (state.batch, tuple(prompt.shape)))
        if state.t != 0:
            raise ValueError("prime: the state is at step %d; a prompt starts a run (t = 0)" % state.t)
        B, P = state.batch, int(prompt.shape[1])
        if state.limit is not None and P > state.limit:
            raise ValueError("prompt of %d samples exceeds frames * pool_stride = %d" % (P, state.limit))
        if P == 0:
            return
        pool = self.cfg.pool_stride if self.E else 1
        P_pad = -(-P // pool) * pool
        view = self._prime_view(B, P_pad)
        audio = torch.zeros((B, P_pad), dtype=torch.float32, device=self.dev)
        audio[:, :P].copy_(prompt)
        view.set_inputs(audio, None, state.cond[:, :P_pad // pool] if self.E else None)
        view.forward(want_logits=False, with_loss=False, train=False, stack_only=True)
        _lib.call("srwn_generate_ring_fill", view.xs.data_ptr(), B * P_pad * self.R, P_pad, P, self._gen_dilations(), self.L,
                  B, self.R, state.ring.data_ptr(), K.abi_dtype(self.dt), torch.cuda.current_stream().cuda_stream)
        state.carry[:, 0].copy_(prompt[:, P - 1])
        if P >= 2:
            state.carry[:, 1].copy_(prompt[:, P - 2])
        state.t = P

    def generate_chunk(self, state: "GenerationState", nsteps: int, mode: str = "sample",
                       forced: Optional[torch.Tensor] = None, want_logits: bool = False):
        """The next `nsteps` samples of the run `state` (see `generate`: the same kernels, chosen by the same rule, and the
        same outputs): (audio [B, nsteps] f32, codes [B, nsteps] i32, logits [B, nsteps, C] f32 or None); advances
        state.t.  Chunks of any lengths give the bits of one `generate` call over their sum.  `forced` [B, nsteps]:
        teacher forcing for this chunk only."""
        B, nsteps = state.batch, int(nsteps)
        if nsteps < 0:
            raise ValueError("generate_chunk: nsteps %d" % nsteps)
        if state.limit is not None and state.t + nsteps > state.limit:
            raise ValueError("generate_chunk: steps %d..%d run past the encoding's frames * pool_stride = %d"
                             % (state.t, state.t + nsteps, state.limit))
        audio, codes, logits, forced = self._gen_outputs(B, nsteps, want_logits, forced)
        if nsteps == 0:
            return audio, codes, logits
        self._launch_generation(state.ring, audio, codes, logits, forced, B, nsteps, mode, state.seed, state.t, state.carry,
                                state.sampling, state.cond_all, state.frames, live=state.live)
        state.t += nsteps
        if state.live:
            state.cond = None      # (the raw frames served `prime`, which only starts a run)
        return audio, codes, logits

    def capture_graphs(self):
        """Captures the step as two hipGraphs -- {forward, backward} and {Adam, re-pack} -- with the
        gradient all-reduce left between them as an ordinary RCCL call, so one and many GPUs replay the
        same launch-free kernel sequence.  Call after at least one eager train_step (warm-up)."""
        import os as _os
        torch.cuda.synchronize()
        self._g_fb = torch.cuda.CUDAGraph()
        self._g_b2 = None
        if self.world == 1 and _os.environ.get("SRWN_FORCE_DIST") != "1":
            # no collective to leave between the graphs: the whole step is one replay
            with torch.cuda.graph(self._g_fb):
                self.forward(defer_loss=True)
                self.backward()
                self.optimizer_step()
            self._g_opt = None
            torch.cuda.synchronize()
            return
        with torch.cuda.graph(self._g_fb):
            self.forward(defer_loss=True)
            self.backward(part=1 if self.bucketed else 0)
        if self.bucketed:   # {forward, upper backward} | bucket A in flight | {lower backward} | bucket B | {Adam}
            self._g_b2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._g_b2, pool=self._g_fb.pool()):
                self.backward(part=2)
        self._g_opt = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g_opt, pool=self._g_fb.pool()):
            self.optimizer_step()
        torch.cuda.synchronize()

    def train_step_graphed(self) -> torch.Tensor:
        self._g_fb.replay()
        if self._g_opt is None:
            return self.loss
        if self._g_b2 is not None:
            h = self._allreduce_bucket_a()
            self._g_b2.replay()
            self._allreduce_bucket_b(h)
        else:
            self.allreduce_grads()
        self._g_opt.replay()
        return self.loss
