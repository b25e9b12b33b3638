"""The streaming stack: what every chunked stream of a residual stack stands on, once.

``StreamStack`` is the device side of one stack run chunk by chunk with the stream forms of the group kernels
(csrc/srwn_stream.hip, csrc/srwn_recog.hip): the group plan, per group a boundary buffer [hist rows | chunk rows], ``top``
for the last group's output, the stored z of every layer (``store_z``), the roll table [[buffer, rows, hist]] that the
owner's last launch moves the histories with, and the ONE loop over the groups (``launch_groups``), the only place of the
package that names the four group stream entry points.  The clock stays with the owner.  ``StreamHost`` is the host face
that ``StreamClassifier`` and the two scorers share on top of one ``StreamStack(store_z=True)``.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import kernels as K
from ._lib import call

# (store_z, slots) -> the entry point of a group launch
GROUP_STREAM = {(False, False): "srwn_residual_group_fwd_stream", (False, True): "srwn_residual_group_fwd_stream_slots",
                (True, False): "srwn_residual_group_fwd_stream_z", (True, True): "srwn_residual_group_fwd_stream_z_slots"}


def stream_history_rows(dilations, groups=None) -> List[int]:
    """Rows of its own input a layer group must keep between two chunks: the sum of its layers' dilations
    (= stride x halo of the group kernel), for every group of ``srwn_group_plan``'s cut."""
    dil = [int(d) for d in dilations]
    groups = K.group_plan(dil, 31, 8) if groups is None else groups
    return [sum(dil[l0:l1]) for l0, l1 in groups]


def nbytes(ts) -> int:
    return int(sum(t.numel() * t.element_size() for t in ts if t is not None))


class StreamStack:
    """The group plan, boundary buffers, ``top``, stored z and roll table of one stack, and its group launches.  `weights`:
    a ``StackWeights`` or ``FlowWeights`` (read: dil, R, Kw, dt, dev, wptr, o_conv, o_res and the views BF / BR).  top: a
    [max_batch, max_chunk, R] tensor to share with other stacks instead of one of its own."""

    @staticmethod
    def plan(dilations) -> Tuple[List[Tuple[int, int]], List[int]]:
        """(groups [(l0, l1)], history rows per group) of a stack: touches no device."""
        groups = K.group_plan(dilations, 31, int(os.environ.get("SRWN_GROUP_LAYERS", "8")))
        return groups, stream_history_rows(dilations, groups)

    def __init__(self, weights, max_batch: int, max_chunk: int, store_z: bool, top: Optional[torch.Tensor] = None):
        w = self.w = weights
        self.max_batch, self.max_chunk, self.store_z = int(max_batch), int(max_chunk), bool(store_z)
        self.groups, self.hist = self.plan(w.dil)
        self.hist_max = max(self.hist)
        Bm, C, R = self.max_batch, self.max_chunk, w.R
        z = lambda *s: torch.zeros(s, dtype=w.dt, device=w.dev)
        self.bufs = [z(Bm, h + C, R) for h in self.hist]      # [hist rows | chunk rows] per group
        self.top = z(Bm, C, R) if top is None else top        # the last layer's output, chunk rows only
        self.zs = z(len(w.dil), Bm, C, R) if self.store_z else None
        self.roll = torch.tensor([[b.data_ptr(), h + C, h] for b, h in zip(self.bufs, self.hist)], dtype=torch.int64,
                                 device=w.dev)

    def reset(self):
        """Zero history: the conv's zero padding before a stream's first sample."""
        for b in self.bufs:
            b.zero_()

    def nbytes(self) -> Dict[str, int]:
        """Device bytes of the boundary buffers with ``top`` and of the stored z, as the ``buffer_bytes`` tables name them."""
        return {"boundary": nbytes(self.bufs + [self.top]), "z": nbytes([self.zs])}

    def launch_groups(self, B: int, n: int, when: int, slots: bool = False, cond=None):
        """One launch per layer group on the chunk's n rows in ``bufs[0]``.  when: the address of the clock, or with
        `slots` of the table [t, t_end] per slot.  cond: None, or (pointers, frames, pool_stride, row stride in elements):
        per layer l the address of the conditioning table whose rows layer l adds for the layer above it, None for the
        stack's top layer."""
        w = self.w
        st, dt, R, C = K._stream(), K.abi_dtype(w.dt), w.R, self.max_chunk
        v, G = w.view, len(self.groups)
        cptrs, frames, pool, cstride = (None, 1, 1, R) if cond is None else cond
        name = GROUP_STREAM[self.store_z, bool(slots)]
        for g, (l0, l1) in enumerate(self.groups):
            last = g + 1 == G
            out = self.top if last else self.bufs[g + 1]
            zargs = (self.zs[l0].data_ptr(), self.max_batch * C * R) if self.store_z else ()
            call(name, self.bufs[g].data_ptr(), self.hist[g] + C, out.data_ptr(),
                 C if last else self.hist[g + 1] + C, 0 if last else self.hist[g + 1], *zargs,
                 K._ptr_array([w.wptr(w.o_conv[l]) for l in range(l0, l1)]),
                 K._ptr_array([w.wptr(w.o_res[l]) for l in range(l0, l1)]),
                 K._ptr_array([v("BF")[l].data_ptr() for l in range(l0, l1)]),
                 K._ptr_array([v("BR")[l].data_ptr() for l in range(l0, l1)]),
                 None if cptrs is None else K._ptr_array(cptrs[l0:l1]), frames, pool, cstride,
                 (ctypes.c_int32 * (l1 - l0))(*w.dil[l0:l1]), l1 - l0, B, n, C, R, w.Kw, dt, when, st)


class StreamHost:
    """What ``StreamClassifier``, ``StreamScorer`` and ``MolStreamScorer`` share: one ``StreamStack`` with stored z (its
    plan, buffers and roll table also under ``groups`` / ``hist`` / ``bufs`` / ``roll``), the chunk as the entry reads it and
    its carry, the clock, the parity twin's ``r0`` / ``r1``, the graph cache, the state's serial and the checks of a push.
    ``_noun`` names the owner in the refusals."""

    _noun = "stream"

    def __init__(self, weights, max_batch: int, max_chunk: int, fused: bool):
        K._need_gpu()
        w = self.w = weights
        self.max_batch, self.max_chunk, self.fused = int(max_batch), int(max_chunk), bool(fused)
        self.dev, self.dt = w.dev, w.dt
        sk = self.stack = StreamStack(w, self.max_batch, self.max_chunk, store_z=True)
        self.groups, self.hist, self.bufs, self.roll = sk.groups, sk.hist, sk.bufs, sk.roll
        self.xbuf = self._zeros(self.max_batch, self.max_chunk, dt=torch.float32)      # the chunk as the entry reads it
        self.carry = self._zeros(self.max_batch, dt=torch.float32)
        self.clock = torch.zeros(1, dtype=torch.int64, device=self.dev)
        if not self.fused:
            self.r0, self.r1 = (self._zeros(self.max_batch * self.max_chunk, w.S) for _ in range(2))
        self.use_graphs = os.environ.get("SRWN_MODEL_GRAPHS", "1") != "0"
        self._graphs: Dict[tuple, object] = {}
        self._seen: set = set()
        self._serial = 0
        self._state = None

    def _zeros(self, *shape, dt=None):
        return torch.zeros(shape, dtype=self.dt if dt is None else dt, device=self.dev)

    def _begin(self, batch) -> int:
        """What every ``start`` does: `batch` checked, zero history, zero carry, clock 0, and a new serial."""
        B = int(batch)
        if not 1 <= B <= self.max_batch:
            raise ValueError("batch %d: this %s holds max_batch=%d" % (B, self._noun, self.max_batch))
        self.stack.reset()
        self.carry.zero_(); self.clock.zero_()
        self._serial += 1
        return B

    def _check_state(self, state):
        if state is not self._state or state._serial != self._serial:
            raise ValueError("this state is not the %s's current one (start() began another)" % self._noun)

    def _check_audio(self, audio, batch=None) -> torch.Tensor:
        x = audio if isinstance(audio, torch.Tensor) else torch.as_tensor(np.asarray(audio, dtype=np.float32))
        if x.dim() != 2:
            raise ValueError("audio must be [batch, samples], got shape %s" % (tuple(x.shape),))
        if not 1 <= x.shape[0] <= self.max_batch:
            raise ValueError("batch %d: this %s holds max_batch=%d" % (x.shape[0], self._noun, self.max_batch))
        if batch is not None and x.shape[0] != batch:
            raise ValueError("audio of %d streams pushed into a state of %d" % (x.shape[0], batch))
        return x

    def _launch_twin_products(self, B: int, n: int) -> int:
        """The training forward's first two products (engine.forward: skip_sum, head_1x1) into ``r0`` / ``r1``, on the
        buffers' rows up to the last stream's chunk (returned): one launch each, so the stale rows between the streams'
        chunks ride along (in a pool also the rows of idle slots and those beyond a slot's ran), and the twin's last step
        never reads them."""
        w, C = self.w, self.max_chunk
        R, S = w.R, w.S
        rows = (B - 1) * C + n
        K.pw_linear(self.stack.zs.data_ptr(), R, self.max_batch * C * R, R, w.L * R, w.wptr(w.o_skip), w.bs_sum,
                    self.r0[:rows], S, S, rows, pro=K.PRO_GATE, epi=K.EPI_RELU)
        K.pw_linear(self.r0.data_ptr(), S, 0, S, S, w.wptr(w.o_w1), w.view("head_b1"), self.r1[:rows], S, S, rows,
                    epi=K.EPI_RELU)
        return rows

    def _launch_roll(self, B: int, n: int, when: int, slots: bool = False):
        """Every group's history rows behind the chunk to the front of its buffer; the staged chunk's last sample becomes the
        carry and the clock advances.  `slots`: the roll alone, on a pool's table."""
        C, tail = self.max_chunk, (B, n, self.max_chunk, self.w.R, K.abi_dtype(self.dt), K._stream())
        if slots:
            call("srwn_recog_roll_slots", self.roll.data_ptr(), len(self.groups), when, *tail)
        else:
            call("srwn_recog_roll", self.roll.data_ptr(), len(self.groups), self.xbuf.data_ptr(), C, self.carry.data_ptr(),
                 when, *tail)
