"""CPU tests of the SiameseWaveNet feature (model.py:660-797): the contrastive head's C-ABI entry point, its argument
errors, the build guard that holds it to zero scratch, the drop-in exports, the wave-pair helper of siamese.py, and the
float64 restatement of the contrastive loss the GPU tests judge the kernel and the engine against."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests._pkg import ROOT, sub


def contrastive_loss(emb: torch.Tensor, labels: torch.Tensor, margin: float):
    """model.py:731-750 on a [2P, D] embedding (the left clips, then the right ones): returns (loss, distance [P])."""
    P = emb.shape[0] // 2
    left, right = emb[:P], emb[P:]
    d = torch.sqrt(1e-8 + ((left - right) ** 2).sum(-1))
    losses = labels * 0.5 * d ** 2 + (1 - labels) * 0.5 * torch.clamp(margin - d, min=0.0) ** 2
    return losses.mean(), d


def _load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_contrastive_head_is_exported():
    L = sub("_lib")
    lib = L.load()
    assert "srwn_contrastive_head" in L.SIGNATURES
    assert hasattr(lib, "srwn_contrastive_head")
    assert lib.srwn_version() >= 101        # the version C callers test for the symbol


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_contrastive_head_argument_errors(binding):
    L = sub("_lib")
    lib = L.bind(binding)
    f = lib.srwn_contrastive_head
    # (mean, w2, b2, labels, margin, emb, dist, loss, gw2, gb2, dmean, rows, S, D, ldw, stream)
    assert f(None, None, None, None, 5.0, None, None, None, None, None, None, 0, 64, 2, 32, None) == 0      # no rows
    assert f(None, 1, 1, None, 5.0, 1, None, None, None, None, None, 2, 64, 2, 32, None) == -3             # mean
    assert b"null" in lib.srwn_last_error()
    assert f(1, 1, 1, None, 5.0, None, None, None, None, None, None, 2, 64, 2, 32, None) == -3             # emb
    assert f(1, 1, 1, 1, 5.0, 1, 1, 1, None, 1, 1, 2, 64, 2, 32, None) == -3                               # gw2
    assert f(1, 1, 1, 1, 5.0, 1, 1, None, 1, 1, 1, 2, 64, 2, 32, None) == -3                               # loss
    assert f(1, 1, 1, None, 5.0, 1, None, None, None, None, None, -2, 64, 2, 32, None) == -2               # rows < 0
    assert f(1, 1, 1, None, 5.0, 1, None, None, None, None, None, 2, 0, 2, 32, None) == -2                 # S
    assert f(1, 1, 1, None, 5.0, 1, None, None, None, None, None, 2, 64, 0, 32, None) == -2                # D
    assert f(1, 1, 1, None, 5.0, 1, None, None, None, None, None, 2, 64, 40, 32, None) == -2               # ldw < D
    assert f(1, 1, 1, 1, 5.0, 1, 1, 1, 1, 1, 1, 3, 64, 2, 32, None) == -2                                  # odd pairs
    assert b"even" in lib.srwn_last_error()
    assert f(1, 1, 1, None, 5.0, 1, 1, None, None, None, None, 3, 64, 2, 32, None) == -2                   # dist, odd
    assert f(1, 1, 1, 1, 5.0, 1, 1, 1, 1, 1, 1, 128, 64, 256, 256, None) == -2                             # LDS
    assert b"LDS" in lib.srwn_last_error()
    with pytest.raises(RuntimeError, match="contrastive_head"):
        L.call("srwn_contrastive_head", None, 1, 1, None, 5.0, 1, None, None, None, None, None, 2, 64, 2, 32, None)


def test_build_refuses_scratch_for_the_contrastive_head():
    B = sub("build")
    assert "contrastive_head_kernel" in B.NO_SPILL["srwn_siamese.hip"]
    clean = ("x.hip:1:1: remark: Function Name: _Z23contrastive_head_kernelPKf\n"
             "x.hip:1:1: remark:     ScratchSize [bytes/lane]: 0\n"
             "x.hip:1:1: remark:     SGPRs Spill: 0\n"
             "x.hip:1:1: remark:     VGPRs Spill: 0\n")
    B._check_no_spill("x.hip", "/nonexistent.o", clean, ["contrastive_head_kernel"])
    for bad in ("ScratchSize [bytes/lane]: 0", "SGPRs Spill: 0", "VGPRs Spill: 0"):
        with pytest.raises(RuntimeError, match="scratch"):
            B._check_no_spill("x.hip", "/nonexistent.o", clean.replace(bad, bad[:-1] + "16"),
                              ["contrastive_head_kernel"])


def test_contrastive_head_compiles_without_scratch():
    """What tools/kres.py reads: the kernel-resource-usage remarks of a device-only compile (no GPU needed)."""
    B = sub("build")
    if not os.path.exists(B.HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_siamese.hip")
    r = subprocess.run([B.HIPCC] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src,
                                              "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    block = r.stderr.split("contrastive_head_kernel", 1)[1]
    for key in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill"):
        m = re.search(re.escape(key) + r": (\d+)", block)
        assert m and int(m.group(1)) == 0, (key, m and m.group(0))


def test_generate_random_wave():
    SA = sub("simple_audio")
    rng = np.random.RandomState(3)
    for _ in range(20):
        x, y = SA.generate_random_wave(1024, rng=rng)
        assert x.shape == (1024,) and y.shape == (4,)
        assert x.min() == pytest.approx(-1.0) and x.max() == pytest.approx(1.0)
        assert y.sum() == 1 and set(np.unique(y)) <= {0.0, 1.0}
    counts = set()
    for _ in range(60):
        x, y = SA.generate_random_wave(512, combos=True, rng=rng)
        assert x.shape == (512,) and -1.0 <= x.min() and x.max() <= 1.0
        assert 1 <= y.sum() <= 4 and set(np.unique(y)) <= {0.0, 1.0}
        counts.add(int(y.sum()))
    assert len(counts) > 1
    x, _ = SA.generate_random_wave(256)          # the global generator, as siamese.py calls it
    assert x.shape == (256,)
    # 20 periods over the clip: a clean sine (noise off) crosses zero upwards 20 times
    clean = SA.Sine(frequency=20, duration=1, sample_rate=5120)
    assert int(np.sum((clean[:-1] < 0) & (clean[1:] >= 0))) in (19, 20)


def test_dropin_exports():
    d = os.path.join(ROOT, "sr-wavenet_amd", "dropin")
    m = _load_file("_dropin_model_siamese", os.path.join(d, "model.py"))
    assert m.SiameseWaveNet is sub("model").SiameseWaveNet
    sa = _load_file("_dropin_simple_audio_siamese", os.path.join(d, "simple_audio.py"))
    assert sa.generate_random_wave is sub("simple_audio").generate_random_wave
    import inspect
    sig = inspect.signature(m.SiameseWaveNet)
    assert list(sig.parameters)[:10] == ["input_size", "output_dimensions", "dilations", "margin", "filter_width",
                                         "dilation_channels", "skip_channels", "name", "learning_rate", "dtype"]
    assert sig.parameters["margin"].default == 5.0 and sig.parameters["name"].default == "SiameseWaveNet"
    assert sub("engine").StackConfig(dilations=[1]).margin == 5.0


def test_contrastive_loss_restatement_matches_finite_differences():
    """The test oracle itself: autograd of the float64 restatement against central differences, with similar,
    dissimilar and fractional labels and pairs on both sides of the margin."""
    g = torch.Generator().manual_seed(0)
    P, D = 5, 3
    emb = torch.randn(2 * P, D, generator=g, dtype=torch.float64)
    labels = torch.tensor([1.0, 0.0, 0.0, 0.3, 0.7], dtype=torch.float64)
    _, d = contrastive_loss(emb, labels, 1.0)
    margin = float(d.median())                  # some pairs inside the margin, some beyond it
    assert (d < margin).any() and (d > margin).any()
    e = emb.clone().requires_grad_(True)
    loss, _ = contrastive_loss(e, labels, margin)
    loss.backward()
    num = torch.zeros_like(emb)
    h = 1e-6
    for i in range(2 * P):
        for k in range(D):
            ep, em = emb.clone(), emb.clone()
            ep[i, k] += h
            em[i, k] -= h
            num[i, k] = (contrastive_loss(ep, labels, margin)[0] - contrastive_loss(em, labels, margin)[0]) / (2 * h)
    assert torch.allclose(e.grad, num, rtol=1e-6, atol=1e-8)
    assert torch.allclose(e.grad[:P], -e.grad[P:], rtol=0, atol=1e-15)     # translation-invariant: rows cancel
    # the closed form the kernel uses: de[p] = g_p (e_p - e_{P+p}) / d_p
    gp = (labels * d - (1 - labels) * torch.clamp(margin - d, min=0.0)) / P
    closed = gp[:, None] * (emb[:P] - emb[P:]) / d[:, None]
    assert torch.allclose(e.grad[:P], closed, rtol=1e-12, atol=1e-15)


def test_contrastive_batch_over_the_head_limit_is_refused_when_built():
    """srwn_contrastive_head holds rows*D + 2P floats in one workgroup's 64 KiB of LDS: the engine refuses a batch past
    that when it is built, naming B, D and the limit, not on its first forward."""
    EG = sub("engine")
    cfg = EG.StackConfig(dilations=[1, 2], dilation_channels=32, skip_channels=128, output_channels=63,
                         head_mode="contrastive")
    with pytest.raises(ValueError, match=r"B=258 .*D=63.*16384"):      # 258*63 + 258 floats
        EG.WaveNetEngine(cfg, 258, 64, "cpu")
    with pytest.raises(ValueError, match=r"B=261 .*D=63.*16384"):      # 261*63 floats (odd: embedding only)
        EG.WaveNetEngine(cfg, 261, 64, "cpu")
