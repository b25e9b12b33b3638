"""What the tests of room reverberation share: the whole rule of a row as one function, the float64 reference with its
derived bound, the planted operands, and the variant of the tap sum that keeps a product unrounded -- the arithmetic a
fused multiply-add would do -- with which the GPU tests show, on the CPU, that their operands tell the two apart.

The bound.  ``reverb_rows`` forms ``e[j]`` as an in-order sum of K rounded products.  With u = 2^-24 the standard result
for such a sum (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1) is ``|e - ref| <= gamma_{K+1} *
sum_k |h[k]| |r[j - k]|`` with ``gamma_n = n u / (1 - n u)``: K products and K additions, each of relative error at most
u, at most K + 1 of them on any term.  It is derived, not measured; on random rows at T = 4099, K = 4096 the worst ratio
measured on the CPU is 0.0016 of it (no product of those rows is subnormal).

The plants.
  order   rows of ones with ``h = [1, 2^-24, 2^-24]`` give 1.0 at j >= 2 (each 2^-24 is half an ulp of 1 and the tie goes
          to even), the reversed response gives 1 + 2^-23 (the two small taps add up first): a sum in any other order shows.
  fusion  with ``a = 1 + 2^-12`` and ``c = -(1 + 2^-11)``, a row ``.. a, c ..`` under ``h = [1, a]`` gives at the c:
          ``fp32(c) + fp32(a * a)`` = c + (1 + 2^-11) = 0, because a * a = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11; a fused
          multiply-add keeps the 2^-24."""
import numpy as np

F = np.float32
U = 2.0 ** -24
A_PLANT = F(1.0 + 2.0 ** -12)
C_PLANT = F(-(1.0 + 2.0 ** -11))
ORDER_TAPS = np.array([1.0, 2.0 ** -24, 2.0 ** -24], F)


def gamma(n):
    return n * U / (1.0 - n * U)


def reference(row, h):
    """``np.convolve`` in float64, cut at the row's length, and the bound on ``reverb_rows``'s distance from it."""
    r, h = np.asarray(row, np.float64), np.asarray(h, np.float64)
    T = r.shape[0]
    ref = np.convolve(r, h)[:T]
    bound = gamma(h.shape[0] + 1) * np.convolve(np.abs(r), np.abs(h))[:T]
    return ref, bound


def room_rows(D, rows, steps, table, rplan, rirs, plan, noise=None):
    """The whole rule: ``augment_rows(reverb_rows(resample_rows(rows)))``; `table` None: no resampling."""
    r = np.ascontiguousarray(rows, dtype=F) if table is None else D.resample_rows(rows, steps, table)
    return D.augment_rows(D.reverb_rows(r, rplan, rirs), plan, noise)


def reverb_rows_unrounded_products(D, rows, plan, rirs):
    """``D.reverb_rows`` with every product kept exact (float64 holds the product of two float32) and only the sum rounded
    to float32: what contracting ``acc + h * r`` into one operation computes (up to the double rounding of the sum, which
    does not matter for counting the outputs that differ)."""
    x = np.ascontiguousarray(rows, dtype=F)
    rirs = np.asarray(rirs, dtype=F)
    out = x.copy()
    B, T = x.shape
    K = rirs.shape[1]
    for b in np.nonzero(plan.apply)[0]:
        h = rirs[int(plan.index[b])].astype(np.float64)
        padded = np.concatenate([np.zeros(K - 1, np.float64), x[b].astype(np.float64)])
        acc = np.zeros(T, F)
        with np.errstate(all="ignore"):
            for k in range(K):
                acc = (acc.astype(np.float64) + h[k] * padded[K - 1 - k:K - 1 - k + T]).astype(F)
        out[b] = acc
    return out


def plant_rows(T, scale=1.0):
    """Two rows: all ones (the order plant), and a, c alternating (the fusion plant at every c behind an a); `scale`, a
    power of two, keeps every rounding where it is and the tap sums inside the clamp of ``augment_rows``."""
    ones = np.ones(T, F)
    alt = np.where(np.arange(T) % 2 == 0, A_PLANT, C_PLANT).astype(F)
    return (np.stack([ones, alt]) * F(scale)).astype(F)


def plant_rirs(K):
    """The planted responses, zero-padded to K taps (K >= 3): the order plant, its reverse, the fusion plant."""
    h = np.zeros((3, K), F)
    h[0, :3] = ORDER_TAPS
    h[1, :3] = ORDER_TAPS[::-1]
    h[2, :2] = [1.0, A_PLANT]
    return h
