"""The host bookkeeping every serving pool shares: which slots hold a stream, which are free, how a caller names slots,
and how one argument becomes one value per stream.  Pure Python and NumPy: no device work, nothing here launches.

* ``SlotTable``  -- the base of ``engine.GenerationPool``, ``student.SynthPool``, ``audio_ring.AudioRingSlots`` (and
                    through it ``encoder.EncoderPool`` and ``recognizer.ClassifierPool``: the pools that take audio
                    share their device ring and their ``push`` there, which keeps this module free of device work)
                    and ``model.ResynthesisPool`` (whose ``_active`` is a read-only property computed from its streams'
                    conditions: it cannot be assigned).
* ``slot_list``  -- a scalar or a sequence of slots as ints, range-checked (the pools' faces in ``model`` use it too).
* ``per_stream`` -- None, a scalar or a sequence of n as a list of n.
"""
from __future__ import annotations

from typing import List

import numpy as np


def _is_scalar(x) -> bool:
    # (not np.ndim: a list of arrays of different lengths, such as the prompts of a join, is no array)
    return np.isscalar(x) or getattr(x, "ndim", None) == 0


def per_stream(x, n, what, who="join", default=None, counted="streams"):
    """One value per stream: None -> n defaults, a scalar -> n copies, a sequence -> its exactly n entries (an entry None
    takes the default when one is given).  ValueError names the caller `who`, the argument `what` and both counts."""
    if x is None:
        return [default] * n
    if _is_scalar(x):
        return [x] * n
    x = list(x)
    if len(x) != n:
        raise ValueError("%s: %s has %d entries for %d %s" % (who, what, len(x), n, counted))
    return x if default is None else [default if v is None else v for v in x]


def slot_list(slots, capacity, who, distinct=False) -> List[int]:
    """`slots` (one slot or a sequence) as a list of ints inside 0..capacity-1, optionally all different."""
    slots = [int(u) for u in ([slots] if _is_scalar(slots) else slots)]
    if any(u < 0 or u >= capacity for u in slots):
        raise ValueError("%s: slots %s outside the pool's %d" % (who, slots, capacity))
    if distinct and len(set(slots)) != len(slots):
        raise ValueError("%s: slots %s are not distinct" % (who, slots))
    return slots


class SlotTable:
    """A pool's slots.  Reads only ``self.capacity`` and the bool array ``self._active`` [capacity], which the pool owns
    and writes; there is no state of its own (a pool built without its constructor needs just those two)."""

    @property
    def active(self) -> List[int]:
        return [int(u) for u in np.flatnonzero(self._active)]

    @property
    def free(self) -> List[int]:
        return [int(u) for u in np.flatnonzero(~self._active)]

    def _slot_list(self, slots, who, distinct=False) -> List[int]:
        return slot_list(slots, self.capacity, who, distinct)

    def _take_slots(self, n, slots, who="join") -> List[int]:
        """The slots n joining streams get: the lowest n free ones, or `slots` once they are n distinct free slots of
        this pool (n None: however many `slots` names, at least one).  Nothing is marked taken here."""
        if slots is None:
            free = self.free
            if n < 1 or n > len(free):
                raise ValueError("%s: %d streams but %d free slots" % (who, n, len(free)))
            return free[:n]
        slots = self._slot_list(slots, who, distinct=True)
        if not slots or (n is not None and len(slots) != n):
            raise ValueError("%s: slots %s do not name %s slots" % (who, slots, "any" if n is None else n))
        if any(self._active[u] for u in slots):
            raise ValueError("%s: slots %s are not all free slots of this pool" % (who, slots))
        return slots
