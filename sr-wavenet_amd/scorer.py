"""The softmax teacher (class ``WaveNetTeacher``: createDecoder's stack, model.py:158-196, with the per-sample softmax over
mu-law codes of model.py:100-112) as a standalone streaming likelihood scorer: audio of any length in, one number per
sample out,

  nll[b, t] = -log p(code[b, t] | audio[b, < t])            nats, code = mu_law_encode(audio)

which is what the teacher is trained on, without the training engine: no fixed (B, T), no saved activations, no
[B, T, 256] logits on their way to the host.

Per step of n <= max_chunk samples the launches are the streaming classifier's with another head: the stream entry
(``srwn_recog_stream_in``), one launch per layer group (``StreamStack.launch_groups``), ``srwn_stream_score_head`` (skip sum,
both head 1x1s, log-softmax and the gather of the target's column in one launch; ``SRWN_SCORE_FUSED=0``: the parity twin,
three ``srwn_pw_linear`` calls into chunk-sized buffers and ``srwn_nll_rows``) and the roll -- one hipGraph per (B, n).

The teacher's RightShift (model.py:172) costs no kernel: the stack's input stream is the audio delayed by one sample, so a
step stages x'[0] = the sample before the chunk (0 at the stream's start) and x'[1:n] = chunk[:n-1], and the entry conv's
two taps then read a[t-2] and a[t-1] for row t -- the generator's input conv.  A row depends on absolute time only: a
stream has the same bits however its audio was cut, at any batch size and in any row of the batch.

``StreamScorer.pool()`` turns the scorer's ``max_batch`` rows into SLOTS (``ScorerPool``): streams join and leave, each
pushes audio of any length at a clock of its own, and one step scores every sample that waits with the same launches in
their slot forms (srwn.h, srwn_version() 118) on a table the host writes before every step.  There is ONE launch list,
``StreamScorer._launch_step(B, n, ..., pool=None)``: with a pool it picks the ``_slots`` entry points and the pool's table in
the clock's place, and the pool's entry ``srwn_score_stream_in_slots`` reads a[t-2], a[t-1] and the target a[t] straight
from the pool's audio ring -- no staged delayed copy, no carry, no separate mu-law launch.

``MolStreamScorer`` is the same stream for the conditioned mixture-of-logistics decoder (the ``WaveNetAutoEncoder``'s, and the
mixture-of-logistics ``WaveNetTeacher``): nll[b, t] = -log p(audio[b, t] | audio[b, < t], encoding) with the audio itself
as the target.  Its entry is ``srwn_flow_stream_in`` on the chunk as it is (RightShift, entry conv and the first layer's
conditioning bias at the device clock; its carry, the two samples before the chunk, is staged from the state), its group
launches carry ``cond_next``, its head is ``srwn_stream_mol_score_head`` (twin: ``srwn_mol_score_rows``), and the encoding
frames are FED into a conditioning ring while the stream runs (``feed`` / ``room`` / ``available``).  The stack, the staged
chunk, the clock, the graph cache and the checks of a push are ``stream_stack.StreamHost``'s, shared with the classifier;
``_ScorerBase`` adds what only the scorers have: the nll and logits buffers, ``start``, the pool bookkeeping and the head's
common arguments.

``MolStreamScorer.pool()`` is the same pool for the conditioned decoder (``MolScorerPool``, a ``ScorerPool`` with a
conditioning ring and a ``fed`` count per slot; srwn.h, srwn_version() 119): ``feed(slots, frames)`` is ragged -- one copy,
one projection, one ``srwn_cond_ring_scatter_slots`` --, a step scores what has both arrived and got its frame, and
``MolStreamScorer._launch_step(B, n, want_logits, pool=None)`` is again ONE launch list: with a pool its entry is
``srwn_mol_score_stream_in_slots`` (a[t-2], a[t-1] and the target a[t] from the pool's audio ring, the first layer's bias
from the slot's conditioning ring: no staged chunk, no carry), the group launches carry ``cond_next`` in their slot form,
and the head and the roll are the slot forms.  ``model.AutoEncoderScorerPool`` couples it to an encoder pool;
``ae_pool_min_audio_ring`` is the smallest scorer-half ring that cannot deadlock that pair.
"""
from __future__ import annotations

import math
import os
import weakref
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import kernels as K
from . import packing as P
from ._lib import call
from .audio_ring import AudioRingSlots
from .engine import WaveNetEngine
from .recognizer import StackWeights
from .stream_stack import StreamHost, StreamStack, nbytes
from .student import live_min_frames, live_room

# What SRWN_SCORE_FUSED means when it is not set: "1" the one-launch head, "0" the parity twin.
SCORE_FUSED_DEFAULT = "1"


def plan_score_pool_step(received, scored, active, max_chunk: int) -> Tuple[int, np.ndarray]:
    """One step of a scorer pool: (n, rows [capacity]).  rows[u] = min(received[u] - scored[u], max_chunk) samples for an
    active slot and 0 for any other; n = 0 when nothing waits, else rows.max() rounded up to a multiple of 32 and capped at
    max_chunk: the rows of the step's launches, so a pool captures at most ceil(max_chunk / 32) graphs.  The device reads
    each slot's true row count from the table: n changes no bit.  Pure NumPy: the CPU tests hold it to brute force."""
    received, scored = np.asarray(received, np.int64), np.asarray(scored, np.int64)
    active = np.asarray(active, bool)
    max_chunk = int(max_chunk)
    if max_chunk < 1:
        raise ValueError("plan_score_pool_step: max_chunk=%d" % max_chunk)
    if received.ndim != 1 or received.shape != scored.shape or received.shape != active.shape:
        raise ValueError("plan_score_pool_step: received, scored and active are [capacity] each")
    if np.any(active & ((scored < 0) | (scored > received))):
        raise ValueError("plan_score_pool_step: a slot has scored more than it received")
    rows = np.where(active, np.minimum(max_chunk, received - scored), 0).astype(np.int64)
    most = int(rows.max()) if rows.size else 0
    return min((most + 31) // 32 * 32, max_chunk), rows


def cut_push(n: int, max_chunk: int) -> List[Tuple[int, int]]:
    """How a push of n samples is cut into steps: [(offset, rows)] in order, every step max_chunk rows but the last,
    none empty (n = 0: no step).  Pure Python: the CPU tests hold it to brute force."""
    n, max_chunk = int(n), int(max_chunk)
    if n < 0 or max_chunk < 1:
        raise ValueError("cut_push: n=%d max_chunk=%d" % (n, max_chunk))
    return [(a, min(max_chunk, n - a)) for a in range(0, n, max_chunk)]


class ScorerWeights(StackWeights):
    """The parameters and forward MFMA images of a per-time-step softmax stack without the training engine around it:
    ``ClassifierWeights``' layout and reference variable names plus the packed image of the last 1x1 (Cp = 32 *
    ceil(C / 32) rows, zero behind C).  Built from a softmax ``WaveNetTeacher``'s engine (``from_engine``: a copy of its
    parameters) or filled from a checkpoint directory by the reference's variable names (``load``)."""

    _who = "streaming scorer"

    def _pack_head(self, pk, secs):
        self.o_w2 = P.pack_linear(pk, secs["head_w2"].offset, self.S, self.Cp, self.Cp)

    @staticmethod
    def check_config(cfg) -> None:
        """What the scorer is built for, on an engine's ``StackConfig``: refused before anything touches the device."""
        if cfg.head_mode == "mol":
            raise NotImplementedError("the streaming scorer is built for the softmax teacher; the mixture-of-logistics "
                                      "head is scored by MolStreamScorer (WaveNetTeacher.mol_scorer, "
                                      "WaveNetAutoEncoder.scorer)")
        if cfg.head_mode != "per_timestep":
            raise ValueError("a streaming scorer needs the per-sample softmax head of WaveNetTeacher (head_mode "
                             "'per_timestep'), this engine has %r" % (cfg.head_mode,))
        if cfg.gate_mode != "reference":
            raise NotImplementedError("gate_mode %r is not built for the streaming scorer" % (cfg.gate_mode,))
        if cfg.cond_channels:
            raise NotImplementedError("the streaming scorer is not built for the conditioned softmax teacher (the "
                                      "conditioned mixture-of-logistics decoder: MolStreamScorer)")
        if not cfg.shift_input:
            raise ValueError("the scorer's stack predicts sample t from the samples before it: it needs the teacher's "
                             "RightShift (shift_input)")

    @classmethod
    def from_engine(cls, eng: WaveNetEngine) -> "ScorerWeights":
        """A copy of a softmax teacher engine's parameters (``WaveNetTeacher._engine``); later training does not reach
        it."""
        cfg = eng.cfg
        cls.check_config(cfg)
        return cls(cfg.dilations, cfg.dilation_channels, cfg.skip_channels, cfg.output_channels, cfg.filter_width, cfg.dtype,
                   eng.dev)._copy_engine(eng)

    def load(self, logdir, scope: str = "WaveNetTeacher") -> bool:
        """``StackWeights.load`` under the teacher's scope (``WaveNetTeacher.save`` or the reference's tf.train.Saver wrote
        the checkpoint)."""
        return super().load(logdir, scope)


class ScoreState:
    """One batch of streams of a ``StreamScorer`` (which holds the device side: a scorer serves one state at a time).
    ``t``: samples scored per stream; ``nll_sum``: the sum of every nll returned so far, fp64 [B] on the device."""

    def __init__(self, batch: int, serial: int, dev):
        self.B, self._serial, self.t = batch, serial, 0
        self._last = torch.zeros(batch, dtype=torch.float32, device=dev)      # the sample before the next chunk
        self.nll_sum = torch.zeros(batch, dtype=torch.float64, device=dev)


class _ScorerBase(StreamHost):
    """What ``StreamScorer`` and ``MolStreamScorer`` add to ``StreamHost``: the nll and logits a step leaves, the twin's fp32
    logits, ``start`` and the head's common arguments.  A subclass allocates the buffers of its own entry and head, and
    gives ``_new_state`` and ``_reset``."""

    _noun = "scorer"
    _pool = None      # the open pool, if any (``pool()``)

    def __init__(self, weights, max_batch: int = 1, max_chunk: int = 1600):
        if min(int(max_batch), int(max_chunk)) < 1:
            raise ValueError("max_batch and max_chunk must be >= 1")
        super().__init__(weights, max_batch, max_chunk, os.environ.get("SRWN_SCORE_FUSED", SCORE_FUSED_DEFAULT) != "0")
        Bm, C = self.max_batch, self.max_chunk
        self.nll = self._zeros(Bm, C, dt=torch.float32)
        self.logits_out: Optional[torch.Tensor] = None        # [Bm, C, classes] fp32, on the first return_logits
        if not self.fused:
            self.logits32 = self._zeros(Bm * C, self.w.Cp, dt=torch.float32)
        self.launches_per_step = 2 + len(self.groups) + (1 if self.fused else 4)

    def _bytes(self, audio, scores, **more) -> Dict[str, int]:
        """``buffer_bytes`` of a scorer: its audio and score buffers, and further families between those and the images."""
        out = dict(self.stack.nbytes(), audio=nbytes(audio), scores=nbytes(scores), **more, images=nbytes([self.w.packed]))
        if not self.fused:
            out["twin r0/r1/logits"] = nbytes([self.r0, self.r1, self.logits32])
        return out

    # ------------------------------------------------------------------------------------------------
    def start(self, batch: int = 1):
        """`batch` streams at clock 0: zero history (the conv's zero padding), zero carry, and 0 for the sample before
        the first one (the RightShift's padding).  The pool, if one is open, ends."""
        B = self._begin(batch)
        self._reset()
        self._state = self._new_state(B)
        self._close_pool()
        return self._state

    def _close_pool(self):
        if self._pool is not None:
            self._pool._open = False
            self._pool = None

    def _open_pool(self, pool):
        """`pool` (already built: a refused pool ends nothing) becomes the scorer's one open pool; the current state ends,
        and an earlier pool."""
        self._close_pool()
        self._serial += 1
        self._state = None
        self._pool = pool
        return pool

    def _reset(self):
        """What else a new state finds zeroed."""

    def _head_args(self):
        """The head's arguments up to the targets: z, the three images and their biases."""
        w = self.w
        return (self.stack.zs.data_ptr(), self.max_batch * self.max_chunk * w.R, self.max_chunk, w.L, w.wptr(w.o_skip),
                w.bs_sum.data_ptr(), w.wptr(w.o_w1), w.view("head_b1").data_ptr(), w.wptr(w.o_w2),
                w.view("head_b2").data_ptr())

    def _launch_twin_products(self, B: int, n: int):
        """``StreamHost``'s two products and the training forward's third, the last 1x1 in fp32."""
        w, S = self.w, self.w.S
        rows = super()._launch_twin_products(B, n)
        K.pw_linear(self.r1.data_ptr(), S, 0, S, S, w.wptr(w.o_w2), w.view("head_b2"), self.logits32[:rows], w.Cp, w.Cp,
                    rows, epi=K.EPI_F32, compute_dtype=self.dt)

    def _run_step(self, key: tuple, launch):
        K.run_cached_graph(self._graphs, self._seen, key, self.use_graphs, launch)


class StreamScorer(_ScorerBase):
    """``start`` a batch of streams, then ``push`` audio of any length: nll [B, n] fp32 of exactly the samples pushed,
    ``score`` for whole recordings.  A step of n rows is one hipGraph per (batch, n, outputs wanted), captured when it is
    used a second time (SRWN_MODEL_GRAPHS=0: eager launches)."""

    def __init__(self, weights: ScorerWeights, max_batch: int = 1, max_chunk: int = 1600):
        super().__init__(weights, max_batch, max_chunk)
        self.codes = self._zeros(self.max_batch, self.max_chunk, dt=torch.int32)
        self.best = self._zeros(self.max_batch, self.max_chunk, dt=torch.int32)

    def pool(self, audio_ring: Optional[int] = None) -> "ScorerPool":
        """A ``ScorerPool`` on this scorer's buffers: its ``max_batch`` rows as slots, each a stream at a clock of its own.
        audio_ring: samples a slot's audio ring holds (default 2 * max_chunk + 2, at least max_chunk + 2).  The current
        ``ScoreState`` ends, and an earlier pool; ``start`` and ``score`` end the pool."""
        return self._open_pool(ScorerPool(self, audio_ring))

    def _want_logits(self):
        if self.logits_out is None:
            self.logits_out = torch.zeros((self.max_batch, self.max_chunk, self.w.C), dtype=torch.float32, device=self.dev)

    def buffer_bytes(self) -> Dict[str, int]:
        """Device bytes by buffer family (DESIGN's table)."""
        return self._bytes([self.xbuf, self.carry, self.codes], [self.nll, self.best, self.logits_out])

    def _new_state(self, B: int) -> ScoreState:
        return ScoreState(B, self._serial, self.dev)

    def _launch_step(self, B: int, n: int, want_logits: bool = False, want_best: bool = False,
                     pool: Optional["ScorerPool"] = None):
        """The launches of a step of n rows: on the delayed audio staged in ``xbuf`` and the targets in ``codes`` at the
        clock, or, with `pool`, the same launches in their slot forms on ``pool.table`` -- B is then the pool's capacity,
        and the pool's entry reads the audio ring (the two samples before the chunk too: no staged delayed copy, no carry)
        and writes ``codes`` itself."""
        w = self.w
        st, dt, R, S, C = K._stream(), K.abi_dtype(self.dt), w.R, w.S, self.max_chunk
        v = w.view
        slots = pool is not None
        sfx = "_slots" if slots else ""
        when = pool.table.data_ptr() if slots else self.clock.data_ptr()      # the clock, or the table in its place
        table = (when,) if slots else ()
        entry = (v("init_w").data_ptr(), v("init_b").data_ptr(), self.bufs[0].data_ptr(), self.hist[0] + C, self.hist[0])
        if slots:
            call("srwn_score_stream_in_slots", pool.ring.data_ptr(), pool.audio_ring, *entry, self.codes.data_ptr(), C, B, n, C,
                 R, w.C, dt, when, st)
        else:
            call("srwn_recog_stream_in", self.xbuf.data_ptr(), C, self.carry.data_ptr(), *entry, B, n, C, R, dt, st)
        self.stack.launch_groups(B, n, when, slots)
        outs = (self.nll.data_ptr(), self.best.data_ptr() if want_best else None,
                self.logits_out.data_ptr() if want_logits else None, C, B, n)
        if self.fused:
            call("srwn_stream_score_head" + sfx, *self._head_args(), self.codes.data_ptr(), *outs, C, R, S, w.C, dt, *table, st)
        else:
            self._launch_twin_products(B, n)
            call("srwn_nll_rows" + sfx, self.logits32.data_ptr(), w.Cp, C, self.codes.data_ptr(), *outs, w.C, *table, st)
        self._launch_roll(B, n, when, slots)

    def push(self, state: ScoreState, audio, return_logits: bool = False, return_best: bool = False):
        """The next samples of every stream, audio [B, n] with any n >= 0 -> nll [B, n] fp32 (nats) of exactly those
        samples; with return_logits also the logits [B, n, C] fp32, with return_best also the most likely code [B, n]
        int32 (the lowest one on ties), in that order.  A device tensor is taken as it is.  Refuses (ValueError, state
        untouched) a wrong rank or batch."""
        self._check_state(state)
        x = self._check_audio(audio, state.B).to(device=self.dev, dtype=torch.float32).contiguous()
        B, n_all, Cc = state.B, int(x.shape[1]), self.w.C
        want_logits, want_best = bool(return_logits), bool(return_best)
        if want_logits:
            self._want_logits()
        nll = torch.empty((B, n_all), dtype=torch.float32, device=self.dev)
        logits = torch.empty((B, n_all, Cc), dtype=torch.float32, device=self.dev) if want_logits else None
        best = torch.empty((B, n_all), dtype=torch.int32, device=self.dev) if want_best else None
        codes = K.mu_law_encode(x, Cc) if n_all else None                 # ops.py:82-93: the targets
        for a, n in cut_push(n_all, self.max_chunk):
            self.xbuf[:B, 0].copy_(state._last)
            self.xbuf[:B, 1:n].copy_(x[:, a:a + n - 1])
            self.codes[:B, :n].copy_(codes[:, a:a + n])
            state._last = x[:, a + n - 1].clone()
            self._run_step((B, n, want_logits, want_best), lambda: self._launch_step(B, n, want_logits, want_best))
            nll[:, a:a + n] = self.nll[:B, :n]
            if want_logits:
                logits[:, a:a + n] = self.logits_out[:B, :n]
            if want_best:
                best[:, a:a + n] = self.best[:B, :n]
        state.t += n_all
        state.nll_sum += nll.sum(1, dtype=torch.float64)
        out = (nll,) + ((logits,) if want_logits else ()) + ((best,) if want_best else ())
        return out if len(out) > 1 else nll

    def score(self, audio, return_logits: bool = False, return_best: bool = False):
        """Whole recordings audio [B, T] of any T -> nll [B, T] (``push``'s returns).  Starts a new state (the current
        one ends)."""
        x = self._check_audio(audio)
        return self.push(self.start(int(x.shape[0])), x, return_logits, return_best)


class ScorerPool(AudioRingSlots):
    """``StreamScorer.pool()``: the scorer's ``max_batch`` rows as SLOTS, each holding a stream with its own samples
    ``received`` and samples ``scored``.  Streams ``join`` free slots (history rows zeroed by srwn_flow_stream_reset_slots),
    ``push`` audio of any length whenever it arrives (``AudioRingSlots.push``: one upload and one srwn_audio_ring_put
    however many slots are written) and ``step`` scores every sample that waits: per pass ``plan_score_pool_step``, the table
    [t = scored, t_end = t + rows] uploaded whole, and the launches of one scorer step in their slot forms
    (``StreamScorer._launch_step`` with this pool) -- one hipGraph per (n, outputs wanted), captured at second use.  A step
    runs no mu-law launch and makes no delayed copy: the pool's entry reads a[t-2], a[t-1] and the target a[t] from the
    ring.  The device never advances the table.  A stream's nll put together equals ``StreamScorer(max_batch=1).score`` of its
    audio alone, bit for bit: in any slot, whenever it joined, however its audio was cut, whatever n the steps had and
    whatever the other slots hold or held before."""

    def __init__(self, owner: StreamScorer, audio_ring: Optional[int] = None):
        c = self.c = owner
        self.capacity, self.max_chunk = c.max_batch, c.max_chunk
        self.audio_ring = 2 * c.max_chunk + 2 if audio_ring is None else int(audio_ring)
        if self.audio_ring < c.max_chunk + 2:
            raise ValueError("pool: audio_ring %d holds less than max_chunk + 2 = %d samples (a whole step and the two "
                             "samples before it)" % (self.audio_ring, c.max_chunk + 2))
        self._alloc_audio_ring()
        cap = self.capacity
        self._received = np.zeros(cap, np.int64)
        self._scored = np.zeros(cap, np.int64)
        self._active = np.zeros(cap, bool)
        self.table = torch.zeros((cap, 2), dtype=torch.int64, device=self.dev)      # SrwnSynthSlot [t, t_end] per slot
        self._nll_sum = torch.zeros(cap, dtype=torch.float64, device=self.dev)      # per slot, on the device: no step waits for it
        self._cols = torch.arange(c.max_chunk, dtype=torch.int64, device=self.dev).unsqueeze(0)
        self._graphs: Dict[tuple, object] = {}
        self._seen: set = set()
        self._open = True
        self.launches_per_step = c.launches_per_step      # the same launches in their slot forms (+ the table's upload)

    def buffer_bytes(self) -> Dict[str, int]:
        """The scorer's device bytes by buffer family with the pool's additions."""
        out = self.c.buffer_bytes()
        out["pool audio ring"] = nbytes([self.ring])
        out["pool stage + table"] = nbytes([self.stage, self.table])
        return out

    # ---- inspection
    dev = property(lambda self: self.c.dev, doc="The scorer's device.")
    received = property(lambda self: self._received.copy(), doc="Samples pushed into each slot's stream so far.")
    scored = property(lambda self: self._scored.copy(), doc="Samples of each slot's stream scored so far.")
    nll_sum = property(lambda self: self._nll_sum.cpu().numpy().copy(),
                       doc="The sum of every nll each slot's stream has returned (nats, fp64 [capacity]; 0 at its join).")

    def bits_per_sample(self, slot: int) -> float:
        """The running mean nll of the stream in `slot`, in bits (NaN before its first sample)."""
        u, = self._slot_list(slot, "bits_per_sample")
        return bits_per_sample(float(self._nll_sum[u]), int(self._scored[u]))

    def _check_open(self):
        if not self._open:
            raise ValueError("this pool is closed (the scorer started a batch or opened another pool)")

    def audio_room(self, slot: int) -> int:
        """Samples a slot can take now: audio_ring - 2 minus what waits to be scored (the - 2 keeps the samples scored - 1
        and scored - 2, the entry conv's taps before the next chunk, alive)."""
        u, = self._slot_list(slot, "audio_room")
        return int(self.audio_ring - 2 - (self._received[u] - self._scored[u]))

    # ---- streams come and go
    def join(self, n: int = 1, slots=None) -> List[int]:
        """n streams into free slots (the lowest ones, or `slots`); returns the slots.  A slot starts at sample 0 with
        zeroed history rows and a zero ``nll_sum``."""
        self._check_open()
        slots = self._take_slots(int(n) if slots is None else None, slots)
        c = self.c
        ids = torch.tensor(slots, dtype=torch.int32, device=c.dev)
        call("srwn_flow_stream_reset_slots", c.roll.data_ptr(), c.roll.shape[0], None, 0, 0, ids.data_ptr(), len(slots),
             self.capacity, c.w.R, K.abi_dtype(c.dt), K._stream())
        self._nll_sum.index_fill_(0, ids.long(), 0.0)
        for u in slots:
            self._received[u] = self._scored[u] = 0
            self._active[u] = True
        return list(slots)

    def leave(self, slots) -> None:
        """Ends the streams in `slots` where they are (a slot already free stays free) and frees their slots."""
        self._check_open()
        for u in self._slot_list(slots, "leave", distinct=True):
            self._active[u] = False

    def push(self, slots, audio) -> None:
        """``AudioRingSlots.push`` into an open pool: audio[i], 1-D of any length (0 too), behind what slots[i] received."""
        self._check_open()
        super().push(slots, audio)

    def _room_tail(self, u):
        return "scored %d" % self._scored[u]

    # ---- one step: every sample that waits
    def _plan(self) -> Tuple[int, np.ndarray]:
        """(n, rows per slot) of the next pass."""
        return plan_score_pool_step(self._received, self._scored, self._active, self.max_chunk)

    def _step(self, wants: tuple):
        """``step`` for the outputs `wants` = (logits[, best]) beside nll, bools: the passes while anything waits -> one
        dict {slot: rows} for nll and one per entry of `wants` that is set."""
        self._check_open()
        c, cap = self.c, self.capacity
        parts = [{} for _ in range(1 + len(wants))]
        while True:
            n, rows = self._plan()
            if n == 0:
                break
            if wants[0]:
                c._want_logits()
            self.table.copy_(torch.from_numpy(np.stack([self._scored, self._scored + rows], 1)))
            K.run_cached_graph(self._graphs, self._seen, (n,) + wants, c.use_graphs,
                               lambda: c._launch_step(cap, n, *wants, pool=self))
            # one copy per pass: the next pass writes the same buffers
            bufs = (c.nll, c.logits_out, getattr(c, "best", None))
            outs = [buf[:cap, :n].clone() if want else None for want, buf in zip((True,) + wants, bufs)]
            live = self._cols[:, :n] < (self.table[:, 1] - self.table[:, 0]).unsqueeze(1)      # [cap, n]: the slots' own rows
            self._nll_sum += torch.where(live, outs[0], 0.0).sum(1, dtype=torch.float64)
            for u in np.flatnonzero(rows):
                m = int(rows[u])
                for part, out in zip(parts, outs):
                    if out is not None:
                        part.setdefault(int(u), []).append(out[u, :m])
            self._scored += rows
        cat = lambda p: p[0] if len(p) == 1 else torch.cat(p, dim=0)
        res = tuple({u: cat(p) for u, p in part.items()} for part, want in zip(parts, (True,) + wants) if want)
        return res if len(res) > 1 else res[0]

    def step(self, return_logits: bool = False, return_best: bool = False):
        """Runs while any active slot has a sample waiting -> {slot: nll [m] fp32 on the device} for the slots whose
        streams scored m > 0 samples; with return_logits also {slot: logits [m, C]}, with return_best also {slot: the most
        likely code [m] int32}, in that order (a tuple of dicts).  With nothing waiting nothing is launched."""
        return self._step((bool(return_logits), bool(return_best)))


# ---- the conditioned mixture-of-logistics decoder ------------------------------------------------------------------------
MAX_MIXTURES = 16      # 4M <= 64 logits: the head keeps them in two 32-column tiles, two mixtures per lane of a row


def plan_score_pieces(frames: int, pool_stride: int, max_frames: int, hist_max: int) -> List[Tuple[int, int]]:
    """How ``MolStreamScorer.score`` walks a recording of `frames` encoding frames through a ring of `max_frames`:
    [(k, n)] in order -- feed k frames (as many as ``student.live_room`` allows, k >= 1), then push the n = fed *
    pool_stride - t samples they make scorable.  Ends with every frame fed and every sample pushed.  Pure Python: the
    CPU tests hold it to brute force on a ring model."""
    frames, pool_stride, max_frames, hist_max = int(frames), int(pool_stride), int(max_frames), int(hist_max)
    if frames < 0 or pool_stride < 1 or max_frames < live_min_frames(hist_max, pool_stride):
        raise ValueError("plan_score_pieces: frames=%d pool_stride=%d max_frames=%d (at least %d for a history of %d)"
                         % (frames, pool_stride, max_frames, live_min_frames(hist_max, pool_stride), hist_max))
    out, fed, t = [], 0, 0
    while fed < frames:
        k = min(live_room(fed, t, hist_max, pool_stride, max_frames), frames - fed)
        fed += k
        out.append((k, fed * pool_stride - t))
        t = fed * pool_stride
    return out


class MolScorerWeights(StackWeights):
    """The parameters and forward MFMA images of the mixture-of-logistics decoder (createDecoder, model.py:158-196) without
    the training engine around it: ``ScorerWeights``' layout with output_channels = 4 * num_mixtures (Cp = 32 or 64 rows in
    the packed last 1x1) and, for cond_channels > 0, the sections WC [L, E, R] / BC [L, R] and the conditioning image of all
    layers as one [Ep] -> [L * R] product, as the engine packs it.  Built from a decoder engine (``from_engine``: a copy
    of its parameters: ``WaveNetAutoEncoder``'s decoder, a mixture-of-logistics ``WaveNetTeacher``) or filled from a
    checkpoint directory by the reference's variable names (``load``)."""

    _who = "streaming scorer"

    def __init__(self, dilations, dilation_channels: int = 32, skip_channels: int = 256, num_mixtures: int = 10,
                 cond_channels: int = 0, pool_stride: int = 1, filter_width: int = 2, dtype: torch.dtype = torch.bfloat16,
                 device="cuda"):
        M, E, pool = int(num_mixtures), int(cond_channels), int(pool_stride)
        if not 1 <= M <= MAX_MIXTURES:
            raise NotImplementedError("num_mixtures %d: the streaming scorer's head is built for 1..%d" % (M, MAX_MIXTURES))
        if E < 0 or pool < 1:
            raise ValueError("cond_channels %d, pool_stride %d" % (E, pool))
        self.M, self.E, self.Ep, self.pool = M, E, (E + 15) // 16 * 16, pool if E else 1
        super().__init__(dilations, dilation_channels, skip_channels, 4 * M, filter_width, dtype, device)

    def _more_sections(self):
        return (("WC", (self.L, self.E, self.R)), ("BC", (self.L, self.R))) if self.E else ()

    def _pack_head(self, pk, secs):
        L, R, E, Ep = self.L, self.R, self.E, self.Ep
        self.o_w2 = P.pack_linear(pk, secs["head_w2"].offset, self.S, self.Cp, self.Cp)
        self.o_wc = None
        if E:      # (engine._pack_stack's image: rows = l * R + channel)
            self.o_wc = pk.reserve(L * R // 32, Ep // 16)
            for l in range(L):
                P.fill_linear(pk, self.o_wc + l * (R // 32) * (Ep // 16) * 512, secs["WC"].offset + l * E * R, E, R,
                              R // 32, Ep // 16)

    def tf_variables(self, scope: str) -> Dict[str, torch.Tensor]:
        """Reference name -> tensor by the decoder's naming (a conditioning 1x1 in front of every layer's two) when the
        stack is conditioned; the dead gate variables are left out."""
        return {k: v for k, v in WaveNetEngine.tf_variables(self, scope, decoder=bool(self.E)).items() if v.is_cuda}

    @staticmethod
    def check_config(cfg) -> None:
        """What the mixture-of-logistics scorer is built for, on an engine's ``StackConfig``: refused before anything
        touches the device."""
        if cfg.head_mode != "mol":
            raise ValueError("MolStreamScorer scores the mixture-of-logistics decoder (head_mode 'mol'), this engine has "
                             "%r (the softmax teacher: StreamScorer)" % (cfg.head_mode,))
        if cfg.gate_mode != "reference":
            raise NotImplementedError("gate_mode %r is not built for the streaming scorer" % (cfg.gate_mode,))
        if not cfg.shift_input:
            raise ValueError("the scorer's stack predicts sample t from the samples before it: it needs the decoder's "
                             "RightShift (shift_input)")
        if cfg.output_channels % 4 or not 1 <= cfg.output_channels // 4 <= MAX_MIXTURES:
            raise NotImplementedError("output_channels %d: 4 * num_mixtures with 1..%d mixtures"
                                      % (cfg.output_channels, MAX_MIXTURES))

    @classmethod
    def from_engine(cls, eng: WaveNetEngine) -> "MolScorerWeights":
        """A copy of a mixture-of-logistics decoder engine's parameters; later training does not reach it."""
        cfg = eng.cfg
        cls.check_config(cfg)
        return cls(cfg.dilations, cfg.dilation_channels, cfg.skip_channels, cfg.output_channels // 4, cfg.cond_channels,
                   cfg.pool_stride, cfg.filter_width, cfg.dtype, eng.dev)._copy_engine(eng)

    def load(self, logdir, scope: str = "WaveNetAutoEncoder/Decoder") -> bool:
        """``StackWeights.load`` under the decoder's scope (``WaveNetAutoEncoder.save`` / ``WaveNetTeacher.save`` or the
        reference's tf.train.Saver wrote the checkpoint)."""
        return super().load(logdir, scope)


class MolScoreState:
    """One batch of streams of a ``MolStreamScorer``.  ``t``: samples scored per stream; ``fed``: conditioning frames fed;
    ``nll_sum``: the sum of every nll returned so far, fp64 [B] on the device."""

    def __init__(self, batch: int, serial: int, dev):
        self.B, self._serial, self.t, self.fed = batch, serial, 0, 0
        self._carry = torch.zeros((batch, 2), dtype=torch.float32, device=dev)      # the samples t - 1 and t - 2
        self.nll_sum = torch.zeros(batch, dtype=torch.float64, device=dev)


class _PoolStride(int):
    """What the instance attribute ``MolStreamScorer.pool`` holds.  It has always been the decoder's pool stride, an int, and
    stays one wherever it is read; called, it is the method ``MolStreamScorer.pool`` that it shadows on the instance:
    ``scorer.pool(audio_ring)`` opens the scorer's pool, as ``StreamScorer.pool`` does."""

    def __new__(cls, stride, owner):
        o = super().__new__(cls, stride)
        o._owner = weakref.ref(owner)
        return o

    def __call__(self, audio_ring: Optional[int] = None) -> "MolScorerPool":
        owner = self._owner()
        return type(owner).pool(owner, audio_ring)


class MolStreamScorer(_ScorerBase):
    """``start`` a batch of streams, ``feed`` them encoding frames (a conditioned decoder) and ``push`` audio: nll [B, n]
    fp32 in nats of exactly the samples pushed, nll[b, t] = -log p(audio[b, t] | audio[b, < t], encoding); ``score`` for
    whole recordings.  The conditioning table is a ring of ``max_frames`` frames per stream: frame q in row q mod
    max_frames.  The group launches recompute their halo rows WITH their conditioning, so a chunk at time t still reads the
    frame of time t - hist_max (hist_max: the largest history of the plan's groups) and the room rule is
    ``student.live_room``; a ring shorter than ``student.live_min_frames`` would stall and is refused."""

    def __init__(self, weights: MolScorerWeights, max_batch: int = 1, max_chunk: int = 1600, max_frames: int = 32):
        if min(int(max_batch), int(max_chunk)) < 1:
            raise ValueError("max_batch and max_chunk must be >= 1")
        w = weights
        self.E, self.pool = w.E, _PoolStride(w.pool, self)
        self.hist_max = max(StreamStack.plan(w.dil)[1]) if w.E else 0
        self.max_frames = int(max_frames) if w.E else 1
        if w.E and self.max_frames < live_min_frames(self.hist_max, self.pool):
            raise ValueError("max_frames %d: a chunk still reads the conditioning of its groups' halo rows, %d samples back; "
                             "at pool_stride %d the ring needs at least %d frames"
                             % (self.max_frames, self.hist_max, self.pool, live_min_frames(self.hist_max, self.pool)))
        super().__init__(w, max_batch, max_chunk)
        Bm, F, LR = self.max_batch, self.max_frames, (w.L * w.R if w.E else w.R)
        self.LR = LR
        self.carry2 = self._zeros(Bm, 2, dt=torch.float32)          # srwn_flow_stream_in's carry, staged before every step
        self.ring = self._zeros(Bm * F, LR)                          # (unconditioned: one zero row per stream)
        if w.E:
            self.stage_in = self._zeros(Bm * F, w.Ep)
            self.stage_out = self._zeros(Bm * F, LR)

    _plan = staticmethod(lambda w: StreamStack.plan(w.dil)[0])      # the groups `w`'s stack will have (the tests size rings by it)

    def buffer_bytes(self) -> Dict[str, int]:
        """Device bytes by buffer family (DESIGN's table)."""
        return self._bytes([self.xbuf, self.carry, self.carry2], [self.nll, self.logits_out],
                           conditioning=nbytes([self.ring] + ([self.stage_in, self.stage_out] if self.E else [])))

    def _new_state(self, B: int) -> MolScoreState:
        return MolScoreState(B, self._serial, self.dev)

    def _reset(self):
        self.ring.zero_()

    def _want_logits(self):
        if self.logits_out is None:
            self.logits_out = torch.zeros((self.max_batch, self.max_chunk, self.w.C), dtype=torch.float32, device=self.dev)

    def pool(self, audio_ring: Optional[int] = None) -> "MolScorerPool":
        """A ``MolScorerPool`` on this scorer's buffers: its ``max_batch`` rows as slots, each a stream at a clock of its own
        with a conditioning ring of its own.  audio_ring: samples a slot's audio ring holds (default 2 * max_chunk + 2, at
        least max_chunk + 2).  The current ``MolScoreState`` ends, and an earlier pool; ``start`` and ``score`` end the
        pool.  (On an instance the name is also the decoder's pool stride, the int it has always been: ``_PoolStride``.)"""
        return self._open_pool(MolScorerPool(self, audio_ring))

    # ------------------------------------------------------------------------------------------------
    def room(self, state: MolScoreState) -> int:
        """Frames that may be fed now (0 for an unconditioned decoder)."""
        self._check_state(state)
        return live_room(state.fed, state.t, self.hist_max, self.pool, self.max_frames) if self.E else 0

    def available(self, state: MolScoreState):
        """Samples that may be pushed now: fed * pool_stride - t; unbounded (inf) without conditioning."""
        self._check_state(state)
        return state.fed * self.pool - state.t if self.E else float("inf")

    def feed(self, state: MolScoreState, frames) -> None:
        """The next k frames of every stream: frames [B, k, cond_channels], a device tensor taken as it is.  Refuses
        (ValueError, before any device work, state untouched) k > ``room``.  One projection through the conditioning
        image and ONE srwn_cond_ring_scatter however many streams."""
        self._check_state(state)
        if not self.E:
            raise ValueError("feed: this decoder is not conditioned")
        fr = torch.as_tensor(frames)
        B = state.B
        if fr.dim() != 3 or fr.shape[0] != B or fr.shape[2] != self.E:
            raise ValueError("feed: frames must be [%d, k, %d], got %s" % (B, self.E, tuple(fr.shape)))
        k = int(fr.shape[1])
        room = self.room(state)
        if k > room:
            raise ValueError("feed: %d frames, but the ring of %d has room for %d at t = %d with %d fed"
                             % (k, self.max_frames, room, state.t, state.fed))
        if k == 0:
            return
        w, rows, LR = self.w, B * k, self.LR
        self.stage_in[:rows, :self.E].copy_(fr.to(device=self.dev, dtype=torch.float32).reshape(rows, self.E))
        K.pw_linear(self.stage_in.data_ptr(), w.Ep, 0, w.Ep, w.Ep, w.wptr(w.o_wc), w.view("BC").reshape(-1),
                    self.stage_out[:rows], LR, LR, rows)
        call("srwn_cond_ring_scatter", self.stage_out.data_ptr(), LR, self.ring.data_ptr(), LR, B, k, state.fed,
             self.max_frames, LR, K.abi_dtype(self.dt), K._stream())
        state.fed += k

    def _launch_step(self, B: int, n: int, want_logits: bool = False, pool: Optional["MolScorerPool"] = None):
        """The launches of a step of n rows: on the chunk staged in ``xbuf`` (entry input and target) and the two samples
        before it in ``carry2`` at the clock, or, with `pool`, the same launches in their slot forms on ``pool.table`` -- B
        is then the pool's capacity, and the pool's entry reads the audio ring (the two samples before the chunk too: no
        staged chunk, no carry) and writes the targets into ``xbuf`` itself."""
        w = self.w
        st, dt, R, S, C = K._stream(), K.abi_dtype(self.dt), w.R, w.S, self.max_chunk
        v, F, LR = w.view, self.max_frames, self.LR
        slots = pool is not None
        sfx = "_slots" if slots else ""
        when = pool.table.data_ptr() if slots else self.clock.data_ptr()      # the clock, or the table in its place
        table = (when,) if slots else ()
        entry = (v("init_w").data_ptr(), v("init_b").data_ptr(), self.ring.data_ptr(), F, self.pool, LR,
                 self.bufs[0].data_ptr(), self.hist[0] + C, self.hist[0])
        if slots:
            call("srwn_mol_score_stream_in_slots", pool.ring.data_ptr(), pool.audio_ring, *entry, self.xbuf.data_ptr(), C, B,
                 n, C, R, dt, when, st)
        else:
            call("srwn_flow_stream_in", self.xbuf.data_ptr(), C, self.carry2.data_ptr(), *entry, B, n, C, R, dt, when, st)
        # layer l adds the bias of layer l + 1: its R columns of the ring's rows [L * R]
        above = [self.ring.data_ptr() + (l + 1) * R * self.ring.element_size() if l + 1 < w.L else None for l in range(w.L)]
        self.stack.launch_groups(B, n, when, slots, cond=(above, F, self.pool, LR) if self.E else None)
        lo = self.logits_out.data_ptr() if want_logits else None
        if self.fused:
            call("srwn_stream_mol_score_head" + sfx, *self._head_args(), self.xbuf.data_ptr(), C, self.nll.data_ptr(), lo, C,
                 B, n, C, R, S, w.M, dt, *table, st)
        else:
            self._launch_twin_products(B, n)
            call("srwn_mol_score_rows" + sfx, self.logits32.data_ptr(), w.Cp, C, self.xbuf.data_ptr(), C, self.nll.data_ptr(),
                 lo, C, B, n, w.M, *table, st)
        self._launch_roll(B, n, when, slots)

    def push(self, state: MolScoreState, audio, return_logits: bool = False):
        """The next samples of every stream, audio [B, n] with any n >= 0 -> nll [B, n] fp32 (nats) of exactly those
        samples (the targets are the audio itself: no mu-law); with return_logits also the logits [B, n, 4M] fp32.  A
        device tensor is taken as it is.  Refuses (ValueError, state untouched) a wrong rank or batch, and n >
        ``available``."""
        self._check_state(state)
        x = self._check_audio(audio, state.B)
        B, n_all = state.B, int(x.shape[1])
        if n_all > self.available(state):
            raise ValueError("push: %d samples, but the %d frames fed cover %d more at t = %d"
                             % (n_all, state.fed, self.available(state), state.t))
        C4 = self.w.C
        x = x.to(device=self.dev, dtype=torch.float32).contiguous()
        want_logits = bool(return_logits)
        if want_logits:
            self._want_logits()
        nll = torch.empty((B, n_all), dtype=torch.float32, device=self.dev)
        logits = torch.empty((B, n_all, C4), dtype=torch.float32, device=self.dev) if want_logits else None
        for a, n in cut_push(n_all, self.max_chunk):
            self.xbuf[:B, :n].copy_(x[:, a:a + n])
            self.carry2[:B].copy_(state._carry)
            # the next chunk's carry: its samples t - 1 and t - 2
            before = x[:, a + n - 2] if n >= 2 else state._carry[:, 0]
            state._carry = torch.stack([x[:, a + n - 1], before], dim=1)
            self._run_step((B, n, want_logits), lambda: self._launch_step(B, n, want_logits))
            nll[:, a:a + n] = self.nll[:B, :n]
            if want_logits:
                logits[:, a:a + n] = self.logits_out[:B, :n]
        state.t += n_all
        state.nll_sum += nll.sum(1, dtype=torch.float64)
        return (nll, logits) if want_logits else nll

    def score(self, audio, encoding=None, return_logits: bool = False):
        """Whole recordings audio [B, T] -> nll [B, T] (``push``'s returns).  A conditioned decoder takes encoding [B,
        frames, cond_channels] with T = frames * pool_stride, fed and pushed in the pieces of ``plan_score_pieces``.
        Starts a new state (the current one ends)."""
        x = self._check_audio(audio)
        B, T = int(x.shape[0]), int(x.shape[1])
        if not self.E:
            if encoding is not None:
                raise ValueError("score: this decoder is not conditioned")
            return self.push(self.start(B), x, return_logits)
        if encoding is None:
            raise ValueError("score: this decoder is conditioned: pass encoding [batch, frames, %d]" % self.E)
        enc = torch.as_tensor(encoding)
        if enc.dim() != 3 or enc.shape[0] != B or enc.shape[2] != self.E or int(enc.shape[1]) * self.pool != T:
            raise ValueError("score: encoding must be [%d, samples / pool_stride = %s, %d], got %s"
                             % (B, "%d / %d" % (T, self.pool), self.E, tuple(enc.shape)))
        st = self.start(B)
        outs, f0, t0 = [], 0, 0
        for k, n in plan_score_pieces(int(enc.shape[1]), self.pool, self.max_frames, self.hist_max):
            self.feed(st, enc[:, f0:f0 + k])
            outs.append(self.push(st, x[:, t0:t0 + n], return_logits))
            f0, t0 = f0 + k, t0 + n
        if not outs:
            outs = [self.push(st, x, return_logits)]
        if return_logits:
            return torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)
        return torch.cat(outs, 1)


class MolScorerPool(ScorerPool):
    """``MolStreamScorer.pool()``: ``ScorerPool`` for the conditioned mixture-of-logistics decoder -- the same slots, audio
    ring, table, pass loop and graph cache (an ``AudioRingSlots`` like it), plus a CONDITIONING RING per slot: the scorer's
    ring [max_batch * max_frames] read as ``max_frames`` rows per slot, frame q of slot u in row u * max_frames + q mod
    max_frames.  Each slot has its own ``fed`` beside ``received`` and ``scored``.  ``feed(slots, frames)`` hands slots
    their next frames, ragged: one copy into the stage, one srwn_pw_linear over all new rows and one
    srwn_cond_ring_scatter_slots however many slots and frames, under the room rule ``student.live_room`` on the slot's own
    fed and scored.  ``step`` scores, per slot, the samples that have both arrived and got their frame: the plan runs on
    min(received, fed * pool_stride) (an unconditioned decoder: on received alone, it has no feed and room 0).  The
    launches are ``MolStreamScorer._launch_step`` with this pool: the entry srwn_mol_score_stream_in_slots reads a[t-2],
    a[t-1] and the target a[t] from the audio ring and the first layer's bias from the slot's conditioning ring, the group
    launches carry ``cond_next`` in their slot form, then the slot head (or the twin) and the slot roll -- as many launches
    as a lockstep step.  A stream's nll put together equals ``MolStreamScorer(max_batch=1).score`` of its audio and frames
    alone, bit for bit: in any slot, whenever it joined, however its audio and frames were cut, whatever n the steps had
    and whatever the other slots hold or held before."""

    def __init__(self, owner: "MolStreamScorer", audio_ring: Optional[int] = None):
        super().__init__(owner, audio_ring)
        self._fed = np.zeros(self.capacity, np.int64)
        # the feed's destination rows, one upload per feed
        self._dst = torch.zeros(self.capacity * owner.max_frames, dtype=torch.int32, device=self.dev)

    def buffer_bytes(self) -> Dict[str, int]:
        """The scorer's device bytes by buffer family with the pool's additions."""
        out = super().buffer_bytes()
        out["pool feed rows"] = nbytes([self._dst])
        return out

    fed = property(lambda self: self._fed.copy(), doc="Conditioning frames fed into each slot's stream so far.")

    def room(self, slot: int) -> int:
        """Frames slot `slot` may be fed now: ``student.live_room`` on its own fed and scored (0 for an unconditioned
        decoder)."""
        u, = self._slot_list(slot, "room")
        c = self.c
        return live_room(self._fed[u], self._scored[u], c.hist_max, c.pool, c.max_frames) if c.E else 0

    def available(self, slot: int) -> int:
        """Samples of slot `slot` the next ``step`` scores: those that have arrived and whose frame was fed."""
        u, = self._slot_list(slot, "available")
        return int(self._ready()[u] - self._scored[u])

    def _ready(self) -> np.ndarray:
        """Per slot, the samples that have arrived and have their conditioning frame."""
        return np.minimum(self._received, self._fed * self.c.pool) if self.c.E else self._received

    def _plan(self) -> Tuple[int, np.ndarray]:
        return plan_score_pool_step(self._ready(), self._scored, self._active, self.max_chunk)

    def join(self, n: int = 1, slots=None) -> List[int]:
        """``ScorerPool.join``; a slot also starts with no frame fed.  The rows of its conditioning ring are NOT zeroed: a
        stream only reads frames it was fed (a chunk's rows lie below fed * pool_stride, its halo rows before time 0 are
        the conv's zero padding), so what an earlier stream left there is never read."""
        slots = super().join(n, slots)
        self._fed[slots] = 0
        return slots

    def feed(self, slots, frames) -> None:
        """The next frames of slots: frames[i] [k_i, cond_channels] for slots[i], ragged (k_i = 0 too); device tensors are
        taken as they are.  Refuses (ValueError, before any device work, nothing changed) an unconditioned decoder, a slot
        that holds no stream, a wrong shape and k_i > ``room(slots[i])``.  One copy into the stage, one projection through
        the conditioning image and ONE srwn_cond_ring_scatter_slots however many slots and frames: row j of slot u goes to
        ring row u * max_frames + (fed_u + j) mod max_frames."""
        self._check_open()
        c = self.c
        if not c.E:
            raise ValueError("feed: this decoder is not conditioned")
        slots = self._slot_list(slots, "feed", distinct=True)
        if isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 2:
            frames = [frames]
        frames = [f if isinstance(f, torch.Tensor) else torch.as_tensor(np.asarray(f, dtype=np.float32)) for f in frames]
        if len(frames) != len(slots):
            raise ValueError("feed: %d slots but %d pieces of frames" % (len(slots), len(frames)))
        for u, f in zip(slots, frames):
            if not self._active[u]:
                raise ValueError("feed: slot %d holds no stream" % u)
            if f.dim() != 2 or f.shape[1] != c.E:
                raise ValueError("feed: frames of slot %d must be [k, %d], got %s" % (u, c.E, tuple(f.shape)))
            if f.shape[0] > self.room(u):
                raise ValueError("feed: %d frames for slot %d, but its ring of %d has room for %d at t = %d with %d fed"
                                 % (f.shape[0], u, c.max_frames, self.room(u), self._scored[u], self._fed[u]))
        pairs = [(u, f) for u, f in zip(slots, frames) if f.shape[0] > 0]
        if not pairs:
            return
        w, F, LR = c.w, c.max_frames, c.LR
        dst = np.concatenate([u * F + (int(self._fed[u]) + np.arange(f.shape[0])) % F for u, f in pairs]).astype(np.int32)
        rows = int(dst.shape[0])
        c.stage_in[:rows, :c.E].copy_(torch.cat([f.to(device=self.dev, dtype=torch.float32) for _, f in pairs], dim=0))
        K.pw_linear(c.stage_in.data_ptr(), w.Ep, 0, w.Ep, w.Ep, w.wptr(w.o_wc), w.view("BC").reshape(-1),
                    c.stage_out[:rows], LR, LR, rows)
        self._dst[:rows].copy_(torch.from_numpy(dst))
        call("srwn_cond_ring_scatter_slots", c.stage_out.data_ptr(), LR, c.ring.data_ptr(), LR, rows, self._dst.data_ptr(),
             self.capacity * F, LR, K.abi_dtype(c.dt), K._stream())
        for u, f in pairs:
            self._fed[u] += int(f.shape[0])

    def step(self, return_logits: bool = False):
        """Runs while any active slot has a sample waiting that has its frame -> {slot: nll [m] fp32 on the device} for
        the slots whose streams scored m > 0 samples; with return_logits a second dict {slot: logits [m, 4M]}.  With
        nothing to score nothing is launched."""
        return self._step((bool(return_logits),))


def ae_pool_min_audio_ring(max_chunk: int, pool_stride: int, enc_layers: int) -> int:
    """The smallest audio ring of the scorer half of an encoder + scorer pool pair (``model.AutoEncoderScorerPool``) that
    cannot deadlock it.  The scorer's ring keeps the samples [scored - 2, received) and a push must fit BOTH halves.  The
    encoder emits frame e once received >= (e + 1) * pool_stride + enc_layers + 1 (``encoder.plan_frames``); until then no
    frame is fed and the scorer stands at scored = e * pool_stride at best, so its ring has to take pool_stride +
    enc_layers + 1 samples beyond that point beside the two carried ones: pool_stride + enc_layers + 3.  And a step reads
    max_chunk + 2 (``MolScorerPool``).  The larger of the two.  Pure Python: the CPU tests hold it to a ring model."""
    return max(int(max_chunk) + 2, int(pool_stride) + int(enc_layers) + 3)


def bits_per_sample(nll_sum: float, samples: int) -> float:
    """Mean nll in bits: nll_sum (nats) / samples / ln 2 (NaN before any sample)."""
    return float(nll_sum) / samples / math.log(2.0) if samples > 0 else float("nan")
