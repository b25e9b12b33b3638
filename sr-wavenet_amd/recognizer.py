"""The classifier of class ``WaveNet`` (createNetwork, model.py:33-62) as a standalone streaming recognizer: audio of any
length in, the pooled posteriors of a sliding window out.

The reference graph's input placeholder is [None, None]: on T > input_size samples its VALID average pool (model.py:58)
yields T - input_size + 1 pooled rows, one per window position.  A stream emits the row of every ``hop``-th position:

  H_j = sum of r1[t] over t in [j * hop, (j + 1) * hop)                fp32 [S], r1 = relu(W1 relu(sum_l skip_l + bs) + b1)
  e_j = softmax(((H_{j-nW+1} + ... + H_j) / window) @ W2 + b2)         nW = window / hop, j >= nW - 1, oldest block first

(the pool commutes with the last 1x1, as ``srwn_pooled_head`` already relies on).  Audio that does not fill a hop waits
in the state, so the stack only ever advances by whole hops at hop-aligned absolute times: every H_j depends on absolute
time only, and a stream has the same bits however its audio was cut, at any batch size and in any row of the batch.

Per step of k hops: the stream entry (input conv), one launch per layer group (``StreamStack.launch_groups`` with stored z:
the stream form of the group kernels that also stores every layer's z of the chunk's rows), ``srwn_pooled_stream_head``
(skip sum, head 1x1 and hop sums in one launch; ``SRWN_RECOG_FUSED=0``: the parity twin, two ``srwn_pw_linear`` calls into
chunk-sized buffers and ``srwn_hop_sum``), ``srwn_window_mean``, ``srwn_pooled_head`` and the roll.  The stack, the staged
chunk, the clock, the graph cache and a push's checks are ``stream_stack.StreamHost``'s, shared with the scorers.

``StreamClassifier.pool()`` turns the classifier's ``max_batch`` rows into SLOTS (``ClassifierPool``): streams join and
leave, each pushes audio of any length at a clock of its own, and one step serves every slot that has a whole hop waiting
with the same launches in their slot forms (srwn.h, srwn_version() 115), on a table the host writes before every step.
There is ONE launch list, ``StreamClassifier._launch_step(B, h, pool=None)``: with a pool it picks the ``_slots`` entry
points, the pool's table in the clock's place and the pool's audio ring in the place of the staged chunk and its carry.
The pool's audio ring and its ``push`` are ``audio_ring.AudioRingSlots``, which the encoder pool shares.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import kernels as K
from . import packing as P
from ._lib import call
from .engine import Section, WaveNetEngine
from .audio_ring import AudioRingSlots
from .stream_stack import StreamHost, nbytes

# What SRWN_RECOG_FUSED means when it is not set: "1" the one-launch head, "0" the parity twin.
RECOG_FUSED_DEFAULT = "1"


def emissions_due(t_before: int, t_after: int, hop: int, window: int) -> Tuple[int, int]:
    """Which emissions a stream owes once it holds ``t_after`` samples, having held ``t_before``: (first hop index j,
    count).  Emission e_j covers the samples [(j + 1) * hop - window, (j + 1) * hop): it is due once (j + 1) * hop
    samples are in, and exists only from j = window / hop - 1 on (VALID: no window reaches before the stream's start).
    Pure Python: the CPU tests hold it to brute force."""
    t_before, t_after, hop, window = int(t_before), int(t_after), int(hop), int(window)
    check_hop_window(hop, window)
    if t_before < 0 or t_after < t_before:
        raise ValueError("emissions_due: t_before=%d t_after=%d" % (t_before, t_after))
    nW = window // hop
    lo = max(t_before // hop, nW - 1)
    hi = t_after // hop
    return lo, max(0, hi - lo)


def plan_pool_step(received, consumed, active, hop: int, max_hops: int) -> Tuple[int, np.ndarray]:
    """One step of a classifier pool: (k, hops [capacity]).  hops[u] = min(max_hops, (received[u] - consumed[u]) // hop)
    whole hops for an active slot and 0 for any other, k = hops.max() the hops of the step's launches (0: nothing to
    launch).  Pure NumPy: the CPU tests hold it to brute force."""
    received, consumed = np.asarray(received, np.int64), np.asarray(consumed, np.int64)
    active = np.asarray(active, bool)
    hop, max_hops = int(hop), int(max_hops)
    if hop < 1 or max_hops < 1:
        raise ValueError("plan_pool_step: hop=%d max_hops=%d" % (hop, max_hops))
    if received.ndim != 1 or received.shape != consumed.shape or received.shape != active.shape:
        raise ValueError("plan_pool_step: received, consumed and active are [capacity] each")
    if np.any(active & ((consumed < 0) | (consumed > received))):
        raise ValueError("plan_pool_step: a slot has consumed more than it received")
    hops = np.where(active, np.minimum(max_hops, (received - consumed) // hop), 0).astype(np.int64)
    return (int(hops.max()) if hops.size else 0), hops


def check_hop_window(hop, window):
    if int(hop) < 1:
        raise ValueError("hop %r: at least 1" % (hop,))
    if int(window) < int(hop) or int(window) % int(hop):
        raise ValueError("window %r must be a multiple of hop %r" % (window, hop))


def check_classifier_widths(filter_width, dilation_channels, skip_channels, who="streaming classifier"):
    """What the streaming classifier's kernels are built for: refused before anything touches the device."""
    if filter_width != 2:
        raise NotImplementedError("filter_width %d: only 2 is built (reference default, model.py:9)" % filter_width)
    if dilation_channels not in (32, 64) or skip_channels not in (128, 256):
        raise NotImplementedError("%s: dilation_channels %d x skip_channels %d; built for {32, 64} x "
                                  "{128, 256}" % (who, dilation_channels, skip_channels))


class StackWeights:
    """The parameters and forward MFMA images of a reference-gate stack with its two head 1x1s, without the training
    engine around it: the engine's section layout and reference variable names, no activations, gradients or Adam state.
    ``ClassifierWeights`` (below), ``scorer.ScorerWeights`` and ``scorer.MolScorerWeights`` are its users; a subclass adds
    the images its own head needs in ``_pack_head`` and, for a conditioned stack (``E`` > 0), the conditioning sections in
    ``_more_sections``."""

    view = WaveNetEngine.view
    wptr = WaveNetEngine.wptr
    named_tensors = WaveNetEngine.named_tensors
    wavenet, E = False, 0
    _who = "streaming classifier"

    def _pack_head(self, pk, secs):
        """Further images behind the ones every user needs (registered on `pk` before it is finalized)."""

    def _more_sections(self):
        """Further parameter sections (name, shape) behind the ones every user has (a conditioned stack's WC / BC)."""
        return ()

    def _copy_engine(self, eng: WaveNetEngine):
        for name in self.sections:
            self.view(name).copy_(eng.view(name))
        self.repack()
        return self

    def __init__(self, dilations, dilation_channels: int = 32, skip_channels: int = 256, output_channels: int = 256,
                 filter_width: int = 2, dtype: torch.dtype = torch.bfloat16, device="cuda"):
        check_classifier_widths(filter_width, dilation_channels, skip_channels, self._who)
        if not 1 <= int(output_channels) <= 256:
            raise NotImplementedError("output_channels must be in [1, 256]")
        if len(dilations) < 1 or min(int(d) for d in dilations) < 1:
            raise ValueError("dilations %r" % (list(dilations),))
        K._need_gpu()
        self.dil = [int(d) for d in dilations]
        self.L, self.R, self.S, self.C, self.Kw = len(self.dil), int(dilation_channels), int(skip_channels), int(output_channels), 2
        self.Cp = (self.C + 31) // 32 * 32
        self.dt, self.dev = dtype, torch.device(device)
        L, R, S, Kw, Cp = self.L, self.R, self.S, self.Kw, self.Cp
        secs: Dict[str, Section] = {}
        off = 0
        for name, shape in (("init_w", (Kw, 1, R)), ("init_b", (R,)), ("WF", (L, Kw, R, R)), ("BF", (L, R)),
                            ("WR", (L, R, R)), ("BR", (L, R)), ("WS", (L, R, S)), ("BS", (L, S)),
                            ("head_w1", (S, S)), ("head_b1", (S,)), ("head_w2", (S, Cp)), ("head_b2", (Cp,))) \
                + tuple(self._more_sections()):
            secs[name] = Section(name, off, shape)
            off += secs[name].numel
        self.sections, self.nparams = secs, off
        self.params = torch.zeros(off, dtype=torch.float32, device=self.dev)
        self.bs_sum = torch.zeros(S, dtype=torch.float32, device=self.dev)
        ph = torch.zeros(1)      # the dead gate variables (ops.py:31-33) exist in checkpoints only: stride-0 host placeholders
        self.dead_gate = {"WG": ph.expand(L, Kw, R, R), "BG": ph.expand(L, R)}
        pk = K.Packer(self.dev)
        self.o_conv = [P.pack_conv(pk, secs["WF"].offset + l * Kw * R * R, Kw, R) for l in range(L)]
        self.o_res = [P.pack_res(pk, secs["WR"].offset + l * R * R, R) for l in range(L)]
        self.o_skip = pk.reserve(S // 32, L * R // 16)      # all skip 1x1s as one image: rows = skip channel, k = l * R + n
        for l in range(L):
            P.fill_linear(pk, self.o_skip, secs["WS"].offset + l * R * S, R, S, S // 32, L * R // 16,
                          ks_offset=l * R // 16, ks_count=R // 16)
        self.o_w1 = P.pack_linear(pk, secs["head_w1"].offset, S, S, S)
        self._pack_head(pk, secs)
        pk.finalize()
        self.packer = pk
        self.packed = torch.zeros(max(pk.total, 1), dtype=self.dt, device=self.dev)
        self.repack()

    def repack(self):
        """The images and the sum of the skip biases from the current parameters (call after changing ``params``)."""
        self.packer.gather(self.params, self.packed, rowsum=(self.view("BS"), self.bs_sum))

    def tf_variables(self, scope: str) -> Dict[str, torch.Tensor]:
        """Reference name -> tensor for the variables the classifier reads (the dead gate variables are left out)."""
        return {k: v for k, v in WaveNetEngine.tf_variables(self, scope, decoder=False).items() if v.is_cuda}

    def load_oracle_params(self, sp):
        """Copies an oracle ``StackParams`` (tests) into the flat buffer."""
        host = torch.zeros(self.nparams, dtype=torch.float32)

        def put(name, arr):
            s = self.sections[name]
            host[s.offset:s.offset + s.numel] = torch.tensor(np.asarray(arr), dtype=torch.float32).reshape(-1)

        put("init_w", sp.init_w); put("init_b", sp.init_b)
        for nm, f in (("WF", "wf"), ("BF", "bf"), ("WR", "wr"), ("BR", "br"), ("WS", "ws"), ("BS", "bs")):
            put(nm, np.stack([getattr(l, f) for l in sp.layers]))
        if self.E:
            put("WC", np.stack([l.wc for l in sp.layers])); put("BC", np.stack([l.bc for l in sp.layers]))
        put("head_w1", sp.head_w1); put("head_b1", sp.head_b1)
        w2 = np.zeros((self.S, self.Cp)); w2[:, :self.C] = sp.head_w2
        b2 = np.zeros(self.Cp); b2[:self.C] = sp.head_b2
        put("head_w2", w2); put("head_b2", b2)
        self.params.copy_(host)
        self.repack()

    def load(self, logdir, scope: str = "WaveNet") -> bool:
        """Fills the parameters from the checkpoint that `logdir`'s state file names (``WaveNet.save`` or the reference's
        tf.train.Saver wrote it), by the reference's variable names under `scope`."""
        from .training import _read_state
        ok = _read_state(logdir, lambda: self.tf_variables(scope))
        if ok:
            self.repack()
        return bool(ok)


class ClassifierWeights(StackWeights):
    """The parameters and forward MFMA images of a ``WaveNet`` classifier without the training engine around it: the
    engine's section layout and reference variable names, no activations, gradients or Adam state.  Built from a
    ``WaveNet``'s engine (``from_engine``: a copy of its parameters) or filled from a checkpoint directory by the
    reference's variable names (``load``: this package's .pt form or a TensorFlow bundle)."""

    @classmethod
    def from_engine(cls, eng: WaveNetEngine) -> "ClassifierWeights":
        """A copy of a pooled-head engine's parameters (``WaveNet._engine``); later training does not reach it."""
        cfg = eng.cfg
        if cfg.head_mode != "pooled":
            raise ValueError("a streaming classifier needs the time-pooled head of class WaveNet (head_mode 'pooled'), "
                             "this engine has %r" % (cfg.head_mode,))
        if cfg.gate_mode != "reference":
            raise NotImplementedError("gate_mode %r is not built for the streaming classifier" % (cfg.gate_mode,))
        if cfg.shift_input or cfg.cond_channels:
            raise ValueError("the classifier's stack has no RightShift and no conditioning (model.py:33-62)")
        return cls(cfg.dilations, cfg.dilation_channels, cfg.skip_channels, cfg.output_channels, cfg.filter_width, cfg.dtype,
                   eng.dev)._copy_engine(eng)


class RecogState:
    """One batch of streams of a ``StreamClassifier`` (which holds the device side: a classifier serves one state at a
    time).  ``t``: samples received per stream; ``emitted``: emissions returned so far; ``pending``: samples waiting for
    their hop to fill (< hop)."""

    def __init__(self, batch: int, serial: int, rem: torch.Tensor):
        self.B, self._serial, self.t, self.emitted, self._rem = batch, serial, 0, 0, rem

    @property
    def pending(self) -> int:
        return int(self._rem.shape[1])


class StreamClassifier(StreamHost):
    """``start`` a batch of streams, then ``push`` audio of any length: the probabilities [B, k, C] of the k window
    positions that audio completed (k >= 0), ``classify`` for whole recordings.  A step of h hops is one hipGraph per
    (batch, h), captured when it is used a second time (SRWN_MODEL_GRAPHS=0: eager launches)."""

    _noun = "classifier"

    def __init__(self, weights: ClassifierWeights, max_batch: int = 1, hop: int = 160, window: int = 16000,
                 max_hops: int = 8):
        check_hop_window(hop, window)
        if min(int(max_batch), int(max_hops)) < 1:
            raise ValueError("max_batch and max_hops must be >= 1")
        self.hop, self.window, self.max_hops = int(hop), int(window), int(max_hops)
        self.nW = self.window // self.hop
        self.ring_rows = self.nW + self.max_hops - 1      # a step writes max_hops rows before the oldest window is read
        super().__init__(weights, max_batch, self.max_hops * self.hop,
                         os.environ.get("SRWN_RECOG_FUSED", RECOG_FUSED_DEFAULT) != "0")
        self.ring = self._zeros(self.max_batch, self.ring_rows, self.w.S, dt=torch.float32)
        self._pool: Optional["ClassifierPool"] = None
        self._alloc_emissions()

    def _alloc_emissions(self):
        """The buffers ``_launch_emit`` writes, for max_batch * max_hops rows, and the step's launch count."""
        w, rows, z = self.w, self.max_batch * self.max_hops, self._zeros
        self.mean = z(rows, w.S, dt=torch.float32)
        self.logits = z(rows, w.C, dt=torch.float32)
        self.probs = z(rows, w.C, dt=torch.float32)
        self.launches_per_step = 4 + len(self.groups) + (1 if self.fused else 3)

    def buffer_bytes(self) -> Dict[str, int]:
        """Device bytes by buffer family (DESIGN's table)."""
        out = dict(self.stack.nbytes(), ring=nbytes([self.ring]), audio=nbytes([self.xbuf, self.carry]),
                   emissions=nbytes([self.mean, self.logits, self.probs]), images=nbytes([self.w.packed]))
        if not self.fused:
            out["twin r0/r1"] = nbytes([self.r0, self.r1])
        return out

    # ------------------------------------------------------------------------------------------------
    def start(self, batch: int = 1) -> RecogState:
        """`batch` streams at clock 0: zero history (the conv's zero padding), zero carry, empty ring."""
        B = self._begin(batch)
        self.ring.zero_()
        self._close_pool()
        self._state = RecogState(B, self._serial, torch.zeros((B, 0), dtype=torch.float32, device=self.dev))
        return self._state

    def _close_pool(self):
        if self._pool is not None:
            self._pool._open = False
            self._pool = None

    def pool(self, audio_ring: Optional[int] = None) -> "ClassifierPool":
        """A ``ClassifierPool`` on this classifier's buffers: its ``max_batch`` rows as slots, each a stream at a clock of
        its own.  audio_ring: samples a slot's audio ring holds (default 2 * max_chunk + 1, at least max_chunk + 1).  The
        current ``RecogState`` ends, and an earlier pool; ``start`` ends the pool."""
        pool = self._new_pool(audio_ring)
        self._close_pool()
        self._serial += 1
        self._state = None
        self._pool = pool
        return pool

    def _new_pool(self, audio_ring):
        return ClassifierPool(self, audio_ring)

    def _launch_step(self, B: int, h: int, pool: Optional["ClassifierPool"] = None):
        """The launches of a step of h hops (n = h * hop rows): on the audio staged in ``xbuf`` at the clock, or, with
        `pool`, the same launches in their slot forms on ``pool.table`` -- B is then the pool's capacity and the audio
        comes from the pool's ring, which holds the sample before the chunk too (no carry)."""
        w = self.w
        st, dt, R, S, C, L = K._stream(), K.abi_dtype(self.dt), w.R, w.S, self.max_chunk, w.L
        slots = pool is not None
        sfx = "_slots" if slots else ""
        n, v = h * self.hop, w.view
        when = pool.table.data_ptr() if slots else self.clock.data_ptr()      # the clock, or the table in its place
        entry = (self.bufs[0].data_ptr(), self.hist[0] + C, self.hist[0], B, n, C, R, dt)
        if slots:
            call("srwn_recog_stream_in_slots", pool.ring.data_ptr(), pool.audio_ring, v("init_w").data_ptr(),
                 v("init_b").data_ptr(), *entry, when, st)
        else:
            call("srwn_recog_stream_in", self.xbuf.data_ptr(), C, self.carry.data_ptr(), v("init_w").data_ptr(),
                 v("init_b").data_ptr(), *entry, st)
        self.stack.launch_groups(B, n, when, slots)
        if self.fused:
            call("srwn_pooled_stream_head" + sfx, self.stack.zs.data_ptr(), self.max_batch * C * R, C, L, w.wptr(w.o_skip),
                 w.bs_sum.data_ptr(), w.wptr(w.o_w1), v("head_b1").data_ptr(), self.ring.data_ptr(), self.ring_rows, when, B,
                 h, self.hop, C, R, S, dt, st)
        else:      # the hop sum never reads the stale rows that ride along in the two products
            self._launch_twin_products(B, n)
            call("srwn_hop_sum" + sfx, self.r1.data_ptr(), C, self.ring.data_ptr(), self.ring_rows, when, B, h, self.hop, C, S,
                 dt, st)
        self._launch_emit(B, h, when, sfx)
        self._launch_roll(B, n, when, slots)

    def _launch_emit(self, B: int, h: int, when: int, sfx: str):
        """What a step makes of the hop sums (between the head and the roll): the window means with their pooled logits,
        then the probabilities.  when, sfx: the clock and "", or a pool's table and "_slots"."""
        w, st = self.w, K._stream()
        w2, b2 = w.view("head_w2").data_ptr(), w.view("head_b2").data_ptr()
        call("srwn_window_mean" + sfx, self.ring.data_ptr(), self.ring_rows, self.mean.data_ptr(), when, B, h, self.hop,
             self.window, w.S, w2, b2, self.logits.data_ptr(), w.C, w.Cp, st)
        call("srwn_pooled_head", self.mean.data_ptr(), w2, b2, None, self.probs.data_ptr(), None, None, None, None, B * h,
             w.S, w.C, w.Cp, st)

    def push(self, state: RecogState, audio, return_logits: bool = False):
        """The next samples of every stream, audio [B, n] with any n >= 0 -> probabilities [B, k, C] fp32 of the k window
        positions they completed (k may be 0); with return_logits also the pooled logits [B, k, C].  A device tensor is
        taken as it is.  Refuses (ValueError, state untouched) a wrong rank or batch."""
        self._check_state(state)
        x = self._check_audio(audio, state.B).to(device=self.dev, dtype=torch.float32)
        B, Cc = state.B, self.w.C
        x = torch.cat([state._rem, x], 1) if state._rem.shape[1] else x
        hops = int(x.shape[1]) // self.hop
        done = state.t - state._rem.shape[1]                  # samples the stack has consumed (hop-aligned)
        first, count = emissions_due(done, done + hops * self.hop, self.hop, self.window)
        probs = torch.empty((B, count, Cc), dtype=torch.float32, device=self.dev)
        logits = torch.empty((B, count, Cc), dtype=torch.float32, device=self.dev) if return_logits else None
        at, j = 0, done // self.hop
        for h0 in range(0, hops, self.max_hops):
            h = min(self.max_hops, hops - h0)
            n = h * self.hop
            self.xbuf[:B, :n].copy_(x[:, h0 * self.hop:h0 * self.hop + n])
            K.run_cached_graph(self._graphs, self._seen, (B, h), self.use_graphs, lambda: self._launch_step(B, h))
            skip = min(max(first - j, 0), h)                  # hops of this step before the first full window
            if h > skip:
                sl = slice(at, at + h - skip)
                probs[:, sl] = self.probs[:B * h].view(B, h, Cc)[:, skip:]
                if return_logits:
                    logits[:, sl] = self.logits[:B * h].view(B, h, Cc)[:, skip:]
                at += h - skip
            j += h
        state._rem = x[:, hops * self.hop:].clone()
        state.t = done + int(x.shape[1])
        state.emitted += count
        return (probs, logits) if return_logits else probs

    def classify(self, audio, return_logits: bool = False):
        """Whole recordings audio [B, T] of any T -> probabilities [B, n_emit, C], n_emit = max(0, T // hop - window /
        hop + 1); a trailing part that does not fill a hop is not heard.  Starts a new state (the current one ends)."""
        x = self._check_audio(audio)
        return self.push(self.start(int(x.shape[0])), x, return_logits)


class ClassifierPool(AudioRingSlots):
    """``StreamClassifier.pool()``: the classifier's ``max_batch`` rows as SLOTS, each holding a stream with its own
    samples ``received``, samples ``consumed`` by the stack (a multiple of hop) and emissions ``emitted``.  Streams ``join``
    free slots (history rows zeroed by srwn_flow_stream_reset_slots; the hop-sum ring needs no reset, srwn.h), ``push``
    audio of any length whenever it arrives (one upload and one srwn_audio_ring_put however many slots are written: a
    slot's audio lives in its row of a device ring, sample s in column s mod audio_ring), and ``step`` serves every slot
    that has a whole hop waiting: per pass ``plan_pool_step``, the table [t = consumed, t_end = t + hops * hop] uploaded
    whole, and the launches of one classifier step in their slot forms (``StreamClassifier._launch_step`` with this pool)
    -- one hipGraph per k, captured at second use.  The
    device never advances the table.  A stream's emissions put together equal ``StreamClassifier(max_batch=1).classify``
    of its audio alone, bit for bit: in any slot, whenever it joined, however its audio was cut, whatever k the steps
    had and whatever the other slots hold or held before."""

    def __init__(self, owner: StreamClassifier, audio_ring: Optional[int] = None):
        c = self.c = owner
        self.capacity, self.hop, self.window, self.max_hops = c.max_batch, c.hop, c.window, c.max_hops
        self.audio_ring = 2 * c.max_chunk + 1 if audio_ring is None else int(audio_ring)
        if self.audio_ring < c.max_chunk + 1:
            raise ValueError("pool: audio_ring %d holds less than max_chunk + 1 = %d samples (a whole step and the sample "
                             "before it)" % (self.audio_ring, c.max_chunk + 1))
        self._alloc_audio_ring()
        cap = self.capacity
        self._received = np.zeros(cap, np.int64)
        self._consumed = np.zeros(cap, np.int64)
        self._emitted = np.zeros(cap, np.int64)
        self._active = np.zeros(cap, bool)
        self.table = torch.zeros((cap, 2), dtype=torch.int64, device=self.dev)      # SrwnSynthSlot [t, t_end] per slot
        self._graphs: Dict[int, object] = {}
        self._seen: set = set()
        self._open = True
        self.launches_per_step = c.launches_per_step      # the same launches in their slot forms (+ the table's upload)

    def buffer_bytes(self) -> Dict[str, int]:
        """The classifier's device bytes by buffer family with the pool's additions."""
        out = self.c.buffer_bytes()
        out["pool audio ring"] = nbytes([self.ring])
        out["pool stage + table"] = nbytes([self.stage, self.table])
        return out

    # ---- inspection
    dev = property(lambda self: self.c.dev, doc="The classifier's device.")
    received = property(lambda self: self._received.copy(), doc="Samples pushed into each slot's stream so far.")
    consumed = property(lambda self: self._consumed.copy(), doc="Samples each slot's stack has run (whole hops).")
    emitted = property(lambda self: self._emitted.copy(), doc="Emissions each slot's stream has returned so far.")

    def _check_open(self):
        if not self._open:
            raise ValueError("this pool is closed (the classifier started a batch or opened another pool)")

    def audio_room(self, slot: int) -> int:
        """Samples a slot can take now: audio_ring - 1 minus what waits for its hop (the - 1 keeps sample consumed - 1, the
        input conv's tap before the next chunk, alive)."""
        u, = self._slot_list(slot, "audio_room")
        return int(self.audio_ring - 1 - (self._received[u] - self._consumed[u]))

    # ---- streams come and go
    def join(self, n: int = 1, slots=None) -> List[int]:
        """n streams into free slots (the lowest ones, or `slots`); returns the slots.  A slot starts at sample 0 with
        zeroed history rows."""
        self._check_open()
        slots = self._take_slots(int(n) if slots is None else None, slots)
        c = self.c
        ids = torch.tensor(slots, dtype=torch.int32, device=c.dev)
        call("srwn_flow_stream_reset_slots", c.roll.data_ptr(), c.roll.shape[0], None, 0, 0, ids.data_ptr(), len(slots),
             self.capacity, c.w.R, K.abi_dtype(c.dt), K._stream())
        for u in slots:
            self._received[u] = self._consumed[u] = self._emitted[u] = 0
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
        return "consumed %d" % self._consumed[u]

    # ---- one step: every whole hop that waits
    def _passes(self):
        """The passes of a ``step``, while any active slot has a whole hop waiting: per pass ``plan_pool_step``, the table
        uploaded whole and the launches of one classifier step of k hops in their slot forms; yields (k, [(slot, lo, hi)])
        -- the emission rows [lo, hi) of the pass's k that each slot's stream completed (``emissions_due`` on the slot's own
        clock; slots with none are left out) -- and moves the slots' clocks on once the caller has taken them."""
        self._check_open()
        c, cap, hop = self.c, self.capacity, self.hop
        while True:
            k, hops = plan_pool_step(self._received, self._consumed, self._active, hop, self.max_hops)
            if k == 0:
                return
            self.table.copy_(torch.from_numpy(np.stack([self._consumed, self._consumed + hops * hop], 1)))
            K.run_cached_graph(self._graphs, self._seen, k, c.use_graphs, lambda: c._launch_step(cap, k, self))
            due = []
            for u in np.flatnonzero(hops):
                t0, h = int(self._consumed[u]), int(hops[u])
                first, count = emissions_due(t0, t0 + h * hop, hop, self.window)
                if count:      # (first - t0 // hop: hops of this step before the stream's first full window)
                    due.append((int(u), first - t0 // hop, h))
                    self._emitted[u] += count
            yield k, due
            self._consumed += hops * hop

    def step(self, return_logits: bool = False):
        """Runs while any active slot has a whole hop waiting -> {slot: probabilities [e, C] fp32 on the device} for the
        slots whose streams completed e > 0 window positions (``emissions_due`` on the slot's own clock); with
        return_logits (probabilities, logits): a second dict with the pooled logits [e, C] of the same slots.  With nothing
        due nothing is launched."""
        pp, pl = {}, {}
        for k, due in self._passes():
            if due:      # one copy per pass: the next pass writes the same buffers
                c, cap, Cc = self.c, self.capacity, self.c.w.C
                probs = c.probs[:cap * k].view(cap, k, Cc).clone()
                logits = c.logits[:cap * k].view(cap, k, Cc).clone() if return_logits else None
            for u, lo, hi in due:
                pp.setdefault(u, []).append(probs[u, lo:hi])
                if return_logits:
                    pl.setdefault(u, []).append(logits[u, lo:hi])
        cat = lambda p: p[0] if len(p) == 1 else torch.cat(p, dim=0)
        out = {u: cat(p) for u, p in pp.items()}
        return (out, {u: cat(p) for u, p in pl.items()}) if return_logits else out
