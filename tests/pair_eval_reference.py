"""The rules of ``srwn_pair_sweep`` (include/srwn.h, srwn_version() 125) restated in NumPy as functions of a stored fp32
distance matrix and the labels, and the distance itself in float64 with the bound an fp32 launch is held to.

Order: a comes before b iff d_a < d_b, or d_a == d_b and a < b.  Per record i over j != i: the first j, the first j of i's
label, and the number of j of another label in front of that one.  Over i < j: bin = min(bins - 1, int(fp32(d * scale)));
a product that is not below bins, NaN included, goes to the last bin."""
import numpy as np


def pair_reference(dist, labels, bins, scale):
    """``(nearest, nearest_dist, same_nearest, same_dist, rank_same, hist_same, hist_diff)`` of dist [N, N] fp32."""
    dist = np.asarray(dist)
    assert dist.dtype == np.float32 and dist.ndim == 2 and dist.shape[0] == dist.shape[1]
    lab = np.asarray(labels).reshape(-1)
    n = dist.shape[0]
    assert lab.shape == (n,)
    nearest, same_nearest, rank_same = (np.full(n, -1, np.int32) for _ in range(3))
    nearest_dist, same_dist = (np.full(n, np.inf, np.float32) for _ in range(2))
    j = np.arange(n)
    for i in range(n):
        d = dist[i]
        other = j != i
        order = np.lexsort((j, d))                                   # by distance, on equal distances by index
        order = order[other[order]]
        if order.size:
            nearest[i], nearest_dist[i] = order[0], d[order[0]]
        same = order[lab[order] == lab[i]]
        if same.size:
            s = same[0]
            same_nearest[i], same_dist[i] = s, d[s]
            before = (d < d[s]) | ((d == d[s]) & (j < s))
            rank_same[i] = np.count_nonzero(before & other & (lab != lab[i]))
    hist_same, hist_diff = np.zeros(bins, np.int64), np.zeros(bins, np.int64)
    iu, ju = np.triu_indices(n, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (dist[iu, ju] * np.float32(scale)).astype(np.float32)
        below = p < np.float32(bins)                                 # (False for NaN)
        b = np.where(below, np.where(below, p, 0).astype(np.int64), bins - 1)
    eq = lab[iu] == lab[ju]
    np.add.at(hist_same, b[eq], 1)
    np.add.at(hist_diff, b[~eq], 1)
    return nearest, nearest_dist, same_nearest, same_dist, rank_same, hist_same, hist_diff


def distance_matrix_fp64(emb):
    """``(d, bound)`` in float64: sqrt(fp32(1e-8) + sum_k (e_i[k] - e_j[k])^2) of the fp32 embeddings, and a per-entry
    bound on what the fp32 launch may differ by.  With u = 2^-24 (half an ulp, relative): every difference carries one
    rounding and its square doubles it (2u), each fmaf adds one (u), a lane's chain is ceil(D / 64) fmafs long, the
    butterfly adds 6 roundings and the 1e-8 one more, so the radicand is within (2 + ceil(D / 64) + 6 + 1) u relative --
    all terms are non-negative, so relative errors do not amplify --; the square root halves that and adds its own
    rounding (sqrtf is held to one ulp = 2u here).  One more u covers the second-order terms, and the smallest normal
    covers results that round in the subnormal range."""
    e = np.asarray(emb, np.float32).astype(np.float64)
    dim = e.shape[1]
    ss = ((e[:, None, :] - e[None, :, :]) ** 2).sum(-1)
    d = np.sqrt(np.float64(np.float32(1e-8)) + ss)
    u = 2.0 ** -24
    rel = ((2 + -(-dim // 64) + 6 + 1) / 2.0 + 2 + 1) * u
    return d, rel * d + np.finfo(np.float32).tiny
