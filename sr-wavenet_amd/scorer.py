"""The softmax teacher (class ``WaveNetTeacher``: createDecoder's stack, model.py:158-196, with the per-sample softmax over
mu-law codes of model.py:100-112) as a standalone streaming likelihood scorer: audio of any length in, one number per
sample out,

  nll[b, t] = -log p(code[b, t] | audio[b, < t])            nats, code = mu_law_encode(audio)

which is what the teacher is trained on, without the training engine: no fixed (B, T), no saved activations, no
[B, T, 256] logits on their way to the host.

Per step of n <= max_chunk samples the launches are the streaming classifier's with another head: the stream entry
(``srwn_recog_stream_in``), one ``srwn_residual_group_fwd_stream_z`` per layer group, ``srwn_stream_score_head`` (skip sum,
both head 1x1s, log-softmax and the gather of the target's column in one launch; ``SRWN_SCORE_FUSED=0``: the parity twin,
three ``srwn_pw_linear`` calls into chunk-sized buffers and ``srwn_nll_rows``) and the roll -- one hipGraph per (B, n).

The teacher's RightShift (model.py:172) costs no kernel: the stack's input stream is the audio delayed by one sample, so a
step stages x'[0] = the sample before the chunk (0 at the stream's start) and x'[1:n] = chunk[:n-1], and the entry conv's
two taps then read a[t-2] and a[t-1] for row t -- the generator's input conv.  A row depends on absolute time only: a
stream has the same bits however its audio was cut, at any batch size and in any row of the batch.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import kernels as K
from . import packing as P
from ._lib import call
from .engine import WaveNetEngine
from .recognizer import StackWeights

# What SRWN_SCORE_FUSED means when it is not set: "1" the one-launch head, "0" the parity twin.
SCORE_FUSED_DEFAULT = "1"


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
                                      "head is not")
        if cfg.head_mode != "per_timestep":
            raise ValueError("a streaming scorer needs the per-sample softmax head of WaveNetTeacher (head_mode "
                             "'per_timestep'), this engine has %r" % (cfg.head_mode,))
        if cfg.gate_mode != "reference":
            raise NotImplementedError("gate_mode %r is not built for the streaming scorer" % (cfg.gate_mode,))
        if cfg.cond_channels:
            raise NotImplementedError("the streaming scorer is not built for the conditioned softmax teacher")
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


class StreamScorer:
    """``start`` a batch of streams, then ``push`` audio of any length: nll [B, n] fp32 of exactly the samples pushed,
    ``score`` for whole recordings.  A step of n rows is one hipGraph per (batch, n, outputs wanted), captured when it is
    used a second time (SRWN_MODEL_GRAPHS=0: eager launches)."""

    def __init__(self, weights: ScorerWeights, max_batch: int = 1, max_chunk: int = 1600):
        if min(int(max_batch), int(max_chunk)) < 1:
            raise ValueError("max_batch and max_chunk must be >= 1")
        K._need_gpu()
        w = self.w = weights
        self.max_batch, self.max_chunk = int(max_batch), int(max_chunk)
        self.dev, self.dt = w.dev, w.dt
        self.groups = K.group_plan(w.dil, 31, int(os.environ.get("SRWN_GROUP_LAYERS", "8")))
        self.hist = [sum(w.dil[l0:l1]) for l0, l1 in self.groups]
        Bm, C, R, S, L = self.max_batch, self.max_chunk, w.R, w.S, w.L
        z = lambda *s, dt=self.dt: torch.zeros(s, dtype=dt, device=self.dev)
        self.bufs = [z(Bm, h + C, R) for h in self.hist]      # [hist rows | chunk rows] per group
        self.top = z(Bm, C, R)                                # the last layer's output: nothing reads it
        self.zs = z(L, Bm, C, R)
        self.xbuf = z(Bm, C, dt=torch.float32)                # the chunk delayed by one sample
        self.carry = z(Bm, dt=torch.float32)
        self.clock = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.codes = z(Bm, C, dt=torch.int32)
        self.nll = z(Bm, C, dt=torch.float32)
        self.best = z(Bm, C, dt=torch.int32)
        self.logits_out: Optional[torch.Tensor] = None        # [Bm, C, classes] fp32, on the first return_logits
        self.roll = torch.tensor([[b.data_ptr(), h + C, h] for b, h in zip(self.bufs, self.hist)], dtype=torch.int64,
                                 device=self.dev)
        self.fused = os.environ.get("SRWN_SCORE_FUSED", SCORE_FUSED_DEFAULT) != "0"
        if not self.fused:
            self.r0, self.r1 = z(Bm * C, S), z(Bm * C, S)
            self.logits32 = z(Bm * C, w.Cp, dt=torch.float32)
        self.use_graphs = os.environ.get("SRWN_MODEL_GRAPHS", "1") != "0"
        self._graphs: Dict[tuple, object] = {}
        self._seen: set = set()
        self._serial = 0
        self._state: Optional[ScoreState] = None
        self.launches_per_step = 2 + len(self.groups) + (1 if self.fused else 4)

    def buffer_bytes(self) -> Dict[str, int]:
        """Device bytes by buffer family (DESIGN's table)."""
        nb = lambda ts: int(sum(t.numel() * t.element_size() for t in ts if t is not None))
        out = {"boundary": nb(self.bufs) + nb([self.top]), "z": nb([self.zs]), "audio": nb([self.xbuf, self.carry, self.codes]),
               "scores": nb([self.nll, self.best, self.logits_out]), "images": nb([self.w.packed])}
        if not self.fused:
            out["twin r0/r1/logits"] = nb([self.r0, self.r1, self.logits32])
        return out

    # ------------------------------------------------------------------------------------------------
    def start(self, batch: int = 1) -> ScoreState:
        """`batch` streams at clock 0: zero history (the conv's zero padding), zero carry, and 0 for the sample before
        the first one (the RightShift's padding)."""
        B = int(batch)
        if not 1 <= B <= self.max_batch:
            raise ValueError("batch %d: this scorer holds max_batch=%d" % (B, self.max_batch))
        for b in self.bufs:
            b.zero_()
        self.carry.zero_(); self.clock.zero_()
        self._serial += 1
        self._state = ScoreState(B, self._serial, self.dev)
        return self._state

    def _check_state(self, state):
        if state is not self._state or state._serial != self._serial:
            raise ValueError("this state is not the scorer's current one (start() began another)")

    def _check_audio(self, audio, batch=None) -> torch.Tensor:
        if isinstance(audio, torch.Tensor):
            x = audio
        else:
            x = torch.as_tensor(np.asarray(audio, dtype=np.float32))
        if x.dim() != 2:
            raise ValueError("audio must be [batch, samples], got shape %s" % (tuple(x.shape),))
        if not 1 <= x.shape[0] <= self.max_batch:
            raise ValueError("batch %d: this scorer holds max_batch=%d" % (x.shape[0], self.max_batch))
        if batch is not None and x.shape[0] != batch:
            raise ValueError("audio of %d streams pushed into a state of %d" % (x.shape[0], batch))
        return x

    def _launch_step(self, B: int, n: int, want_logits: bool = False, want_best: bool = False):
        """The launches of a step of n rows on the delayed audio staged in ``xbuf`` and the targets in ``codes``."""
        import ctypes as C_
        w = self.w
        st, dt, R, S, C, L = K._stream(), K.abi_dtype(self.dt), w.R, w.S, self.max_chunk, w.L
        v, when = w.view, self.clock.data_ptr()
        call("srwn_recog_stream_in", self.xbuf.data_ptr(), C, self.carry.data_ptr(), v("init_w").data_ptr(),
             v("init_b").data_ptr(), self.bufs[0].data_ptr(), self.hist[0] + C, self.hist[0], B, n, C, R, dt, st)
        G = len(self.groups)
        zstride = self.max_batch * C * R
        for g, (l0, l1) in enumerate(self.groups):
            last = g + 1 == G
            out = self.top if last else self.bufs[g + 1]
            nl = l1 - l0
            call("srwn_residual_group_fwd_stream_z", self.bufs[g].data_ptr(), self.hist[g] + C, out.data_ptr(),
                 C if last else self.hist[g + 1] + C, 0 if last else self.hist[g + 1], self.zs[l0].data_ptr(), zstride,
                 K._ptr_array([w.wptr(w.o_conv[l]) for l in range(l0, l1)]),
                 K._ptr_array([w.wptr(w.o_res[l]) for l in range(l0, l1)]),
                 K._ptr_array([v("BF")[l].data_ptr() for l in range(l0, l1)]),
                 K._ptr_array([v("BR")[l].data_ptr() for l in range(l0, l1)]),
                 None, 1, 1, R, (C_.c_int32 * nl)(*w.dil[l0:l1]), nl, B, n, C, R, w.Kw, dt, when, st)
        outs = (self.nll.data_ptr(), self.best.data_ptr() if want_best else None,
                self.logits_out.data_ptr() if want_logits else None, C, B, n)
        if self.fused:
            call("srwn_stream_score_head", self.zs.data_ptr(), zstride, C, L, w.wptr(w.o_skip), w.bs_sum.data_ptr(),
                 w.wptr(w.o_w1), v("head_b1").data_ptr(), w.wptr(w.o_w2), v("head_b2").data_ptr(), self.codes.data_ptr(),
                 *outs, C, R, S, w.C, dt, st)
        else:      # the training forward's three products (engine.forward: skip_sum, head_1x1 and the last 1x1 in fp32) on
            # the buffers' rows up to the last stream's chunk: one launch each, so the stale rows between the streams' chunks
            # ride along, and srwn_nll_rows never reads them
            rows = (B - 1) * C + n
            K.pw_linear(self.zs.data_ptr(), R, zstride, R, L * R, w.wptr(w.o_skip), w.bs_sum, self.r0[:rows], S, S, rows,
                        pro=K.PRO_GATE, epi=K.EPI_RELU)
            K.pw_linear(self.r0.data_ptr(), S, 0, S, S, w.wptr(w.o_w1), v("head_b1"), self.r1[:rows], S, S, rows,
                        epi=K.EPI_RELU)
            K.pw_linear(self.r1.data_ptr(), S, 0, S, S, w.wptr(w.o_w2), v("head_b2"), self.logits32[:rows], w.Cp, w.Cp,
                        rows, epi=K.EPI_F32, compute_dtype=self.dt)
            call("srwn_nll_rows", self.logits32.data_ptr(), w.Cp, C, self.codes.data_ptr(), *outs, w.C, st)
        call("srwn_recog_roll", self.roll.data_ptr(), G, self.xbuf.data_ptr(), C, self.carry.data_ptr(), when, B, n, C, R,
             dt, st)

    def push(self, state: ScoreState, audio, return_logits: bool = False, return_best: bool = False):
        """The next samples of every stream, audio [B, n] with any n >= 0 -> nll [B, n] fp32 (nats) of exactly those
        samples; with return_logits also the logits [B, n, C] fp32, with return_best also the most likely code [B, n]
        int32 (the lowest one on ties), in that order.  A device tensor is taken as it is.  Refuses (ValueError, state
        untouched) a wrong rank or batch."""
        self._check_state(state)
        x = self._check_audio(audio, state.B).to(device=self.dev, dtype=torch.float32).contiguous()
        B, n_all, Cc = state.B, int(x.shape[1]), self.w.C
        want_logits, want_best = bool(return_logits), bool(return_best)
        if want_logits and self.logits_out is None:
            self.logits_out = torch.zeros((self.max_batch, self.max_chunk, Cc), dtype=torch.float32, device=self.dev)
        nll = torch.empty((B, n_all), dtype=torch.float32, device=self.dev)
        logits = torch.empty((B, n_all, Cc), dtype=torch.float32, device=self.dev) if want_logits else None
        best = torch.empty((B, n_all), dtype=torch.int32, device=self.dev) if want_best else None
        codes = K.mu_law_encode(x, Cc) if n_all else None                 # ops.py:82-93: the targets
        for a, n in cut_push(n_all, self.max_chunk):
            self.xbuf[:B, 0].copy_(state._last)
            self.xbuf[:B, 1:n].copy_(x[:, a:a + n - 1])
            self.codes[:B, :n].copy_(codes[:, a:a + n])
            state._last = x[:, a + n - 1].clone()
            K.run_cached_graph(self._graphs, self._seen, (B, n, want_logits, want_best), self.use_graphs,
                               lambda: self._launch_step(B, n, want_logits, want_best))
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


def bits_per_sample(nll_sum: float, samples: int) -> float:
    """Mean nll in bits: nll_sum (nats) / samples / ln 2 (NaN before any sample)."""
    return float(nll_sum) / samples / math.log(2.0) if samples > 0 else float("nan")
