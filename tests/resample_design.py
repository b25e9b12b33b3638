"""What the tests of speed perturbation share: the quality measurement of ``dataset.resample_rows`` with its recorded
result, the whole rule as one function, and the variant of the tap sum that keeps a product unrounded -- the arithmetic a
fused multiply-add would do -- with which the GPU tests show, on the CPU, that their operands tell the two apart.

The quality measurement.  float32 sines ``sin(pi f n + 0.3)`` of 2048 samples at f = 0.05, 0.2 and 0.4 of Nyquist are
resampled at speeds 0.9, 1.1, 0.5 and 2.0, each through the table of ``Augment(speed=(s, s), taps=16)`` (cutoff min(1, 1 /
s)); at 2.0 only the tones at or below half the cutoff (0.05 and 0.2) are used.  The result is compared with the analytic
sine at the positions ``j * step / 2^24`` in float64, over the outputs from ``taps`` behind the row's first sample to
``taps`` in front of the last position inside the row.  With RESAMPLE_PHASES = 4096 and a Kaiser window of beta = 7 the
worst absolute error of the eleven cases is MEASURED_WORST below (speed 1.1, tone 0.4); the bound the tests assert is
twice that.  The same sweep over the window and the phase count, which chose the two constants, is in DESIGN section 5f."""
import numpy as np

F = np.float32
QUALITY_T = 2048
QUALITY_TAPS = 16
TONES = (0.05, 0.2, 0.4)
SPEEDS = (0.9, 1.1, 0.5, 2.0)
MEASURED_WORST = 4.75e-4          # measured by quality_errors on the CPU (float32 taps, float64 reference): 4.747e-4
QUALITY_BOUND = 2 * MEASURED_WORST


def quality_errors(D):
    """[(speed, tone, worst absolute error)] of the cases above, by ``D.resample_rows``."""
    out = []
    n = np.arange(QUALITY_T, dtype=np.float64)
    for s in SPEEDS:
        a = D.Augment(speed=(s, s), taps=QUALITY_TAPS)
        assert a.step_lo == a.step_hi
        speed = a.step_lo / 2.0 ** D.SPEED_BITS
        for f in TONES:
            if s == 2.0 and f > a.cutoff / 2:
                continue
            x = np.sin(np.pi * f * n + 0.3).astype(F)
            y = D.resample_rows(x[None], [a.step_lo], a.table())[0]
            ref = np.sin(np.pi * f * n * speed + 0.3)
            end = int(min(QUALITY_T, np.floor((QUALITY_T - 1) / speed))) - QUALITY_TAPS
            out.append((s, f, float(np.abs(y[QUALITY_TAPS:end] - ref[QUALITY_TAPS:end]).max())))
    return out


def warp_rows(D, rows, steps, table, plan, noise=None):
    """The whole rule: ``augment_rows(resample_rows(rows, steps, table), plan, noise)``."""
    return D.augment_rows(D.resample_rows(rows, steps, table), plan, noise)


def resample_rows_unrounded_products(D, rows, steps, table):
    """``D.resample_rows`` with every product kept exact (float64 holds the product of two float32) and only the sum
    rounded to float32: what contracting ``acc + h * x`` into one operation computes (up to the double rounding of the
    sum, which does not matter for counting the outputs that differ)."""
    x = np.ascontiguousarray(rows, dtype=F)
    table = np.asarray(table, dtype=F)
    B, T = x.shape
    taps = table.shape[1]
    shift = D.SPEED_BITS - (D.RESAMPLE_PHASES.bit_length() - 1)
    out = np.empty_like(x)
    j = np.arange(T, dtype=np.uint64)
    for b in range(B):
        q = j * np.uint64(steps[b])
        i = (q >> np.uint64(D.SPEED_BITS)).astype(np.int64)
        f = ((q >> np.uint64(shift)) & np.uint64(D.RESAMPLE_PHASES - 1)).astype(np.int64)
        acc = np.zeros(T, F)
        with np.errstate(all="ignore"):
            for k in range(taps):
                at = i - (taps // 2 - 1) + k
                xk = np.where((at >= 0) & (at < T), x[b, np.clip(at, 0, T - 1)], F(0.0)).astype(np.float64)
                acc = (acc.astype(np.float64) + table[f, k].astype(np.float64) * xk).astype(F)
        out[b] = acc
    return out
