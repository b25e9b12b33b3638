"""The audio-ring side of a serving pool that takes audio: ``encoder.EncoderPool`` and ``recognizer.ClassifierPool``.

A slot's audio lives in its row of one device ring, sample s in column s mod audio_ring; ``push`` writes any number of
slots with one host-to-device copy and one ``srwn_audio_ring_put``.  What differs between the pools -- how much room a
slot has, which streams take no more audio and what the room message counts -- they give as ``audio_room``,
``_push_barred`` and ``_room_tail``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import kernels as K
from ._lib import call
from .slots import SlotTable


class AudioRingSlots(SlotTable):
    """``SlotTable`` with an audio ring per slot.  Like its base it has no state of its own: it reads ``self.capacity``,
    ``self.audio_ring``, ``self._active``, ``self._received`` (int64 [capacity], samples pushed per slot), ``self.dev``
    (the owner's device, read only once the GPU is known to be there) and the device buffers ``self.ring`` and ``self.stage`` that ``_alloc_audio_ring`` makes (a pool built without its
    constructor may leave them None: nothing here reads them before a sample is to be uploaded)."""

    def _alloc_audio_ring(self):
        """``self.ring`` [capacity, audio_ring] fp32 and ``self.stage``, the one upload of a push, on ``self.dev``.  A pool
        whose ring offsets leave int32 is refused before the GPU is asked for."""
        cap = self.capacity
        if cap * self.audio_ring + 4 * cap > 0x7fffffff:
            raise ValueError("pool: %d slots of %d samples" % (cap, self.audio_ring))
        K._need_gpu()
        self.ring = torch.zeros((cap, self.audio_ring), dtype=torch.float32, device=self.dev)
        # one upload per push: [streams | src_offset | first_col | counts] (n each) and the concatenated audio behind them
        self.stage = torch.zeros(4 * cap + cap * self.audio_ring, dtype=torch.int32, device=self.dev)

    def _push_barred(self):
        """Streams that hold a slot but take no more audio: ``(bool [capacity], message % slot)``, or None.  Asked once
        per push, not per slot: a push of many slots stays as cheap as it was."""
        return None

    def _room_tail(self, u: int) -> str:
        """What the refusal for want of room says of slot u after ``received``."""
        raise NotImplementedError

    def push(self, slots, audio) -> None:
        """audio[i], 1-D of any length (0 too), behind what slots[i] has received.  Refuses (ValueError, nothing changed) a
        slot that holds no stream, one the pool's ``_push_barred`` names, more than ``audio_room(slot)`` samples and
        audio that is not floating point.  One host-to-device copy and one srwn_audio_ring_put, whatever the number of
        slots; without a sample to write, no device work."""
        one = not np.ndim(slots)
        slots = self._slot_list(slots, "push", distinct=True)
        if one or isinstance(audio, (np.ndarray, torch.Tensor)):
            audio = [audio]
        audio = list(audio)
        if len(audio) != len(slots):
            raise ValueError("push: %d slots but %d pieces of audio" % (len(slots), len(audio)))
        barred = self._push_barred()
        xs = []
        for u, x in zip(slots, audio):
            if isinstance(x, torch.Tensor):
                if not x.is_floating_point():
                    raise ValueError("push: audio must be floating point, got %s" % x.dtype)
                x = x.detach().to("cpu", torch.float32).numpy()
            else:
                x = np.asarray(x)
                if x.dtype.kind != "f":
                    raise ValueError("push: audio must be floating point, got %s" % x.dtype)
                x = x.astype(np.float32, copy=False)
            if x.ndim != 1:
                raise ValueError("push: the audio of a slot is 1-D [samples], got shape %s" % (x.shape,))
            if not self._active[u]:
                raise ValueError("push: slot %d holds no stream" % u)
            if barred is not None and barred[0][u]:
                raise ValueError(barred[1] % u)
            if x.shape[0] > self.audio_room(u):
                raise ValueError("push: %d samples for slot %d, but its ring of %d has room for %d (received %d, %s)"
                                 % (x.shape[0], u, self.audio_ring, self.audio_room(u), self._received[u], self._room_tail(u)))
            xs.append(x)
        pairs = [(u, x) for u, x in zip(slots, xs) if x.shape[0] > 0]
        if not pairs:
            return
        n = len(pairs)
        counts = np.asarray([x.shape[0] for _, x in pairs], np.int64)
        us = np.asarray([u for u, _ in pairs], np.int64)
        host = np.empty(4 * n + int(counts.sum()), np.int32)
        host[0:n] = us
        host[n:2 * n] = np.cumsum(counts) - counts
        host[2 * n:3 * n] = self._received[us] % self.audio_ring
        host[3 * n:4 * n] = counts
        host[4 * n:].view(np.float32)[:] = np.concatenate([x for _, x in pairs])
        self.stage[:host.shape[0]].copy_(torch.from_numpy(host))
        sp = self.stage.data_ptr()
        call("srwn_audio_ring_put", self.ring.data_ptr(), self.audio_ring, self.capacity, sp + 16 * n, sp, sp + 4 * n,
             sp + 8 * n, sp + 12 * n, n, int(counts.max()), K._stream())
        self._received[us] += counts
