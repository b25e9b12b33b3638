"""The rules of ``srwn_eval_classes`` (csrc/srwn_eval.hip) restated in NumPy, row by row, for the tests that hold the kernel
and ``evaluate`` to them.  Nothing here imports the package."""
import numpy as np


def eval_reference(probs, labels):
    """``probs [M, C]`` float32 and the rows' ``labels [M]`` -> ``(pred [M] int32, rank [M] int32, nll [M] float32,
    confusion [C, C] int32)``.

    pred: the first maximum, found with ``>`` over rising class index (on equal values the lower index stays).
    rank: the classes that come before the label's class in that order -- a strictly greater probability, or an equal one
    at a lower index -- so rank == 0 exactly where pred == label.
    nll: ``float32(-log(float64(probs[label])))``; +inf for a probability of 0.
    confusion[label, pred] counts the rows."""
    probs = np.asarray(probs)
    assert probs.dtype == np.float32 and probs.ndim == 2
    labels = np.asarray(labels).astype(np.int64)
    M, C = probs.shape
    assert labels.shape == (M,) and (labels >= 0).all() and (labels < C).all()
    pred = np.zeros(M, np.int32)
    rank = np.zeros(M, np.int32)
    nll = np.zeros(M, np.float32)
    confusion = np.zeros((C, C), np.int32)
    cls = np.arange(C)
    for m in range(M):
        row, lab = probs[m], int(labels[m])
        best = 0
        for c in range(1, C):
            if row[c] > row[best]:
                best = c
        pred[m] = best
        pl = row[lab]
        rank[m] = np.count_nonzero((row > pl) | ((row == pl) & (cls < lab)))
        with np.errstate(divide="ignore"):
            nll[m] = np.float32(-np.log(np.float64(pl)))
        confusion[lab, best] += 1
    return pred, rank, nll, confusion


def ulp_distance(a, b):
    """|a - b| in units of the last place of float32, per entry; 0 where both are the same infinity or both zeros of
    either sign."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)

    def key(x):                           # the floats' order as integers: negative values mirrored below zero
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
