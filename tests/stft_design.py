"""Inputs and the fp32 reference for the bin-by-bin tests of srwn_stft_power / srwn_stft_power_bwd (host code, NumPy;
used by tests/test_mol_design.py on the CPU and tests/test_gpu_mol_entries.py on the GPU).

The per-bin bounds are 4 x the error of the reference evaluated in float32 -- a direct 512-point DFT of the same windowed
frames with float32 twiddles, accumulated term by term in float32 (``dft32``), and the backward formula in float32 on that
spectrum (``bwd32``) -- against the fp64 oracle.  The factor covers the device's own sincospif / fmaf order."""
import numpy as np

from oracle import wavenet_np as O

FL, FS, NB = 512, 256, 257
LENGTHS = [512, 768, 1000]          # one frame, two frames, two frames and 232 dropped samples
BINS = [0, 1, 128, 255, 256]        # DC, the lowest, the middle, the highest below Nyquist, Nyquist
B = 2
TONE_AMP = 0.5
_CACHE = {}


def frames_of(T):
    return 1 + (T - FL) // FS


def noise(T):
    """White Gaussian noise, sigma = 0.3, float32 [B, T]: every bin carries comparable power."""
    return (np.random.default_rng(900 + T).standard_normal((B, T)) * 0.3).astype(np.float32)


def tone(T, f):
    """A pure tone at bin f, float32 [B, T] (row b at amplitude TONE_AMP / (b + 1)): f = 0 is a constant, f = 256
    alternates +-a."""
    t = np.arange(T)
    amp = TONE_AMP / (np.arange(B)[:, None] + 1.0)
    return (amp * np.cos(2.0 * np.pi * ((f * t) % FL) / FL)).astype(np.float32)


def _tables32():
    i = np.arange(FL)
    return np.cos(2.0 * np.pi * i / FL).astype(np.float32), np.sin(2.0 * np.pi * i / FL).astype(np.float32)


def dft32(x):
    """x [B, T] float32 -> (spec [B, nf, 257, 2], power [B, 257]) by a direct DFT in float32: one term at a time."""
    f32 = np.float32
    cs, sn = _tables32()
    nf = frames_of(x.shape[1])
    win = f32(0.5) - f32(0.5) * cs
    fr = np.stack([x[:, n * FS:n * FS + FL] for n in range(nf)], 1) * win
    re = np.zeros(fr.shape[:2] + (NB,), f32); im = np.zeros_like(re)
    f = np.arange(NB)
    for j in range(FL):
        idx = (f * j) & (FL - 1)
        re = re + fr[:, :, j, None] * cs[idx]
        im = im - fr[:, :, j, None] * sn[idx]
    fp = re * re + im * im
    pw = fp[:, 0]
    for n in range(1, nf):
        pw = pw + fp[:, n]
    pw = pw / f32(nf)
    assert pw.dtype == f32 and re.dtype == f32
    return np.stack([re, im], -1), pw


def bwd32(spec, f, T):
    """d power[:, f] / dx [B, T] in float32 from a float32 spectrum (the formula of srwn_stft_power_bwd for a one-hot
    dpower): dx[b, n FS + j] += win[j] (2 / nf) (Re cos - Im sin)(2 pi f j / 512)."""
    f32 = np.float32
    cs, sn = _tables32()
    nf = spec.shape[1]
    win = f32(0.5) - f32(0.5) * cs
    idx = (f * np.arange(FL)) & (FL - 1)
    dx = np.zeros((spec.shape[0], T), f32)
    for n in range(nf):
        s = spec[:, n, f, 0, None] * cs[idx] - spec[:, n, f, 1, None] * sn[idx]
        dx[:, n * FS:n * FS + FL] += s * (win * (f32(2.0) / f32(nf)))
    return dx


def bwd64(x, f):
    """The same by oracle (ii)'s autograd of that single bin's power, fp64 [B, T]."""
    import torch
    from oracle import wavenet_torch as OT
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    OT.stft_power(xt)[:, f].sum().backward()
    return xt.grad.numpy()


def reference(T):
    """Per clip length, computed once: the noise input, the fp64 oracle's power and one-bin gradients, and the fp32
    reference's worst per-bin relative error (fwd32) and worst max-normalised one-bin gradient error (bwd32)."""
    if T not in _CACHE:
        x = noise(T)
        want = O.stft_power(x.astype(np.float64))
        spec, pw = dft32(x)
        fwd = float((np.abs(pw - want) / want).max())
        grads = {f: bwd64(x, f) for f in BINS}
        bwd = max(float(np.abs(bwd32(spec, f, T) - g).max() / np.abs(g).max()) for f, g in grads.items())
        for a in (x, want) + tuple(grads.values()):
            a.setflags(write=False)
        _CACHE[T] = dict(x=x, power=want, grads=grads, fwd32=fwd, bwd32=bwd)
    return _CACHE[T]


def tone_reference(T, f):
    """(x, the fp64 power's peak bin f [B], fp32 reference's relative error at that bin)."""
    x = tone(T, f)
    want = O.stft_power(x.astype(np.float64))
    assert (want[:, f] > 0.999 * want.max(-1)).all()      # (the Hann window puts as much into bin 0 / 256 for f = 1 / 255)
    _, pw = dft32(x)
    return x, want[:, f], float((np.abs(pw[:, f] - want[:, f]) / want[:, f]).max())
