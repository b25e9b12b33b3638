"""NumPy restatement of the rules ``srwn_adam_step_ctl`` adds to the Adam update (include/srwn.h): which row of the control
table a step reads, and the EMA shadow's update as three separately rounded float32 operations."""
import numpy as np

TINY = np.finfo(np.float32).tiny


def ctl_row(t, H):
    """The table row of the launch that makes step `t` (1-based, the count after the tick)."""
    return max(0, min(int(t) - 1, int(H) - 1))


def _no_subnormal(x, what):
    ax = np.abs(x)
    assert ((ax == 0) | (ax >= TINY)).all(), "subnormal %s: the restatement's bits depend on flush-to-zero modes" % what


def ema_reference(e, theta, d):
    """tf's assign_moving_average on float32 arrays: s = 1 - d; diff = e - theta; p = s * diff; e' = e - p, each rounded
    to float32.  No intermediate may be subnormal."""
    e, theta = np.asarray(e), np.asarray(theta)
    assert e.dtype == np.float32 and theta.dtype == np.float32
    s = np.float32(1.0) - np.float32(d)
    diff = e - theta
    p = s * diff
    out = e - p
    assert diff.dtype == p.dtype == out.dtype == np.float32
    for x, what in ((s, "s"), (diff, "diff"), (p, "p"), (out, "e'")):
        _no_subnormal(np.asarray(x), what)
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)
