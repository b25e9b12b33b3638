"""Training controls: learning-rate schedules, gradient clipping and EMA weights, as the host prepares them.

Pure NumPy, importable without a GPU.  The optimizer launch (``srwn_adam_step_ctl``, include/srwn.h) reads the learning
rate and the EMA decay of every step from a device table ``float32 [horizon, 2] = {lr, ema_decay}``; this module builds
that table.  The launch that makes step ``t`` (1-based, the count after the tick) reads row ``min(t - 1, horizon - 1)``:
row ``i`` belongs to the 0-based step ``i``, and steps at or beyond ``horizon`` keep the last row.

A schedule is a callable ``f(step) -> float`` of the 0-based step.  Those below evaluate in float64; the table rounds
each value once to float32.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Union

import numpy as np

Schedule = Callable[[int], float]


def constant(lr: float) -> Schedule:
    lr = float(lr)
    return lambda step: lr


def linear_warmup(lr: float, warmup_steps: int, then: Optional[Schedule] = None) -> Schedule:
    """``lr * (step + 1) / warmup_steps`` for the first `warmup_steps` steps (the last of them runs at ``lr``), then
    ``then(step - warmup_steps)`` (default: ``lr``, constant)."""
    lr, w = float(lr), int(warmup_steps)
    if w < 0:
        raise ValueError("linear_warmup: warmup_steps %d" % w)
    after = constant(lr) if then is None else as_schedule(then)
    return lambda step: lr * (step + 1) / w if step < w else after(step - w)


def exponential_decay(lr: float, decay_steps: int, rate: float, staircase: bool = False) -> Schedule:
    """tf.train.exponential_decay: ``lr * rate ** (step / decay_steps)``, the quotient floored with `staircase`."""
    lr, n, rate = float(lr), int(decay_steps), float(rate)
    if n < 1:
        raise ValueError("exponential_decay: decay_steps %d" % n)

    def f(step):
        p = step / n
        return lr * rate ** (math.floor(p) if staircase else p)
    return f


def piecewise(boundaries: Sequence[int], values: Sequence[float]) -> Schedule:
    """tf.train.piecewise_constant: ``values[0]`` while ``step <= boundaries[0]``, ``values[i]`` while
    ``boundaries[i - 1] < step <= boundaries[i]``, ``values[-1]`` beyond the last boundary."""
    b, v = [int(x) for x in boundaries], [float(x) for x in values]
    if len(v) != len(b) + 1:
        raise ValueError("piecewise: %d boundaries need %d values, got %d" % (len(b), len(b) + 1, len(v)))
    if any(y <= x for x, y in zip(b, b[1:])):
        raise ValueError("piecewise: boundaries must increase")

    def f(step):
        for x, val in zip(b, v):
            if step <= x:
                return val
        return v[-1]
    return f


def cosine(lr: float, total_steps: int, floor: float = 0.0) -> Schedule:
    """``floor + (lr - floor) * (1 + cos(pi * min(step, total_steps) / total_steps)) / 2``: `lr` at step 0, their mean at
    the midpoint, `floor` from `total_steps` on."""
    lr, n, floor = float(lr), int(total_steps), float(floor)
    if n < 1:
        raise ValueError("cosine: total_steps %d" % n)
    return lambda step: floor + (lr - floor) * 0.5 * (1.0 + math.cos(math.pi * min(step, n) / n))


def as_schedule(schedule: Union[Schedule, float]) -> Schedule:
    """A number is its constant schedule; a callable is itself."""
    if callable(schedule):
        return schedule
    return constant(schedule)


def ema_decay_at(decay: float, step: int, warmup: bool = True) -> float:
    """The decay tf.train.ExponentialMovingAverage(decay, num_updates=step) applies: ``min(decay, (1 + step) / (10 + step))``;
    `decay` itself with ``warmup=False``."""
    decay = float(decay)
    return min(decay, (1.0 + step) / (10.0 + step)) if warmup else decay


def control_table(schedule, horizon: int, ema_decay: Optional[float] = None, ema_warmup: bool = True) -> np.ndarray:
    """float32 [horizon, 2]: row i = {schedule(i), ema_decay_at(ema_decay, i, ema_warmup)} of the 0-based step i, each
    evaluated in float64 and rounded once.  Column 1 is 0 where there is no EMA.  Steps at or beyond `horizon` keep the
    last row: the optimizer launch clamps its row to ``horizon - 1``."""
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("control_table: horizon %d: at least 1" % horizon)
    f = as_schedule(schedule)
    lr = np.array([float(f(i)) for i in range(horizon)], dtype=np.float64)
    bad = np.flatnonzero(~(np.isfinite(lr) & (lr >= 0)))
    if bad.size:
        raise ValueError("control_table: the schedule gives lr %r at step %d: finite and not below 0" % (lr[bad[0]], bad[0]))
    out = np.zeros((horizon, 2), dtype=np.float32)
    out[:, 0] = lr
    if ema_decay is not None:      # ema_decay_at for every row (the same float64 operations)
        i = np.arange(horizon, dtype=np.float64)
        out[:, 1] = np.minimum(float(ema_decay), (1.0 + i) / (10.0 + i)) if ema_warmup else float(ema_decay)
    return out


def parse_schedule(text: str, lr: float) -> Schedule:
    """``NAME[:args]`` of the drivers' ``--lr-schedule``: constant, warmup:STEPS, exp:DECAY_STEPS:RATE[:staircase],
    piecewise:B1,B2,...:V0,V1,..., cosine:TOTAL[:FLOOR]; `lr` is the base rate."""
    name, _, rest = text.partition(":")
    a = rest.split(":") if rest else []
    try:
        if name == "constant" and not a:
            return constant(lr)
        if name == "warmup" and len(a) == 1:
            return linear_warmup(lr, int(a[0]))
        if name == "exp" and len(a) in (2, 3) and (len(a) == 2 or a[2] == "staircase"):
            return exponential_decay(lr, int(a[0]), float(a[1]), staircase=len(a) == 3)
        if name == "piecewise" and len(a) == 2:
            return piecewise([int(x) for x in a[0].split(",")], [float(x) for x in a[1].split(",")])
        if name == "cosine" and len(a) in (1, 2):
            return cosine(lr, int(a[0]), float(a[1]) if len(a) == 2 else 0.0)
    except ValueError as e:
        raise ValueError("lr schedule %r: %s" % (text, e))
    raise ValueError("lr schedule %r: constant, warmup:STEPS, exp:DECAY_STEPS:RATE[:staircase], "
                     "piecewise:B1,...:V0,V1,..., cosine:TOTAL[:FLOOR]" % text)


@dataclass
class TrainControls:
    """What ``set_controls`` of an engine takes.  `schedule`: a schedule or a number; `horizon`: the rows of the table
    (later steps keep the last row); `clip_norm`: tf.clip_by_global_norm's bound or None; `ema_decay`: the shadow's decay
    in [0, 1) or None for no shadow; `ema_warmup`: tf's ``num_updates`` ramp; `validate_ema`: ``fit(validate=...)`` judges
    the averaged weights.  Range errors raise ValueError here, before any device work."""
    schedule: Union[Schedule, float]
    horizon: int = 1
    clip_norm: Optional[float] = None
    ema_decay: Optional[float] = None
    ema_warmup: bool = True
    validate_ema: bool = False

    def __post_init__(self):
        self.horizon = int(self.horizon)
        if self.horizon < 1:
            raise ValueError("horizon %d: at least 1" % self.horizon)
        if self.clip_norm is not None:
            self.clip_norm = float(self.clip_norm)
            if not (math.isfinite(self.clip_norm) and self.clip_norm > 0):
                raise ValueError("clip_norm %r: above 0" % self.clip_norm)
        if self.ema_decay is not None:
            self.ema_decay = float(self.ema_decay)
            if not 0.0 <= self.ema_decay < 1.0:
                raise ValueError("ema_decay %r: in [0, 1)" % self.ema_decay)
        if self.validate_ema and self.ema_decay is None:
            raise ValueError("validate_ema needs ema_decay")
        self._table = control_table(self.schedule, self.horizon, self.ema_decay, self.ema_warmup)      # (lr range errors)

    def table(self) -> np.ndarray:
        """The control table, float32 [horizon, 2] (a copy)."""
        return self._table.copy()

    @property
    def features(self):
        """What decides the launch list: (clipping on, EMA on)."""
        return (self.clip_norm is not None, self.ema_decay is not None)

    def scalars(self) -> dict:
        """The scalar settings, as a training-state file keeps them (the schedule itself is code: the table stands for it)."""
        return {"horizon": self.horizon, "clip_norm": self.clip_norm, "ema_decay": self.ema_decay,
                "ema_warmup": bool(self.ema_warmup), "validate_ema": bool(self.validate_ema)}


# --- the drivers' flags (examples/) ----------------------------------------------------------------------------------------
def add_control_flags(parser, validate: bool = False):
    """--lr-schedule, --clip, --ema, --resume (and --validate-ema) of the example drivers."""
    parser.add_argument("--lr-schedule", type=str, default=None, metavar="NAME[:args]",
                        help="constant, warmup:STEPS, exp:DECAY_STEPS:RATE[:staircase], piecewise:B1,..:V0,V1,.., "
                             "cosine:TOTAL[:FLOOR] on the model's learning rate")
    parser.add_argument("--clip", type=float, default=None, help="clip the gradient to this global norm")
    parser.add_argument("--ema", type=float, default=None, help="keep EMA weights with this decay")
    parser.add_argument("--resume", action="store_true",
                        help="restore Adam's moments, the EMA and the sampler from the training state next to the "
                             "checkpoint, and write one with every checkpoint")
    if validate:
        parser.add_argument("--validate-ema", action="store_true", help="validation sweeps judge the EMA weights")


def apply_control_flags(model, args, lr: float, steps: int):
    """The flags onto ``model.set_training_controls``; with none of them given nothing is set: the driver runs what it ran
    before there were controls.  The table holds `steps` rows."""
    validate = bool(getattr(args, "validate_ema", False))
    if args.lr_schedule is None and args.clip is None and args.ema is None:
        if validate:
            raise ValueError("--validate-ema needs --ema")
        return None
    schedule = None if args.lr_schedule is None else parse_schedule(args.lr_schedule, lr)
    return model.set_training_controls(schedule=schedule, horizon=max(1, int(steps)), clip_norm=args.clip,
                                       ema_decay=args.ema, validate_ema=validate)
