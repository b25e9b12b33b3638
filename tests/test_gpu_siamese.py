"""GPU tests of SiameseWaveNet (model.py:660-797): the contrastive head kernel against numpy float64, the engine's
"contrastive" head mode against the float64 TorchStack oracle run on both towers as one batch, training with graph
replay, the model class with its checkpoints, and the siamese.py driver."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from oracle.wavenet_torch import TorchStack
from tests._pkg import ROOT, sub
from tests.test_gpu_kernels import DEV, dev, rel_err
from tests.test_siamese import contrastive_loss

pytestmark = pytest.mark.gpu


def _np_head(mean, w2, b2, labels, margin, D):
    """The contrastive head in float64: emb, dist, loss, gw2 [S,D], gb2 [D], dmean."""
    mean = mean.astype(np.float64)
    emb = mean @ w2[:, :D].astype(np.float64) + b2[:D].astype(np.float64)
    P = mean.shape[0] // 2
    diff = emb[:P] - emb[P:]
    d = np.sqrt(1e-8 + (diff ** 2).sum(-1))
    h = np.maximum(0.0, margin - d)
    y = labels.astype(np.float64)
    loss = np.mean(0.5 * (y * d ** 2 + (1 - y) * h ** 2))
    g = (y * d - (1 - y) * h) / P
    de = np.concatenate([g[:, None] * diff / d[:, None], -g[:, None] * diff / d[:, None]])
    return emb, d, loss, mean.T @ de, de.sum(0), de @ w2[:, :D].astype(np.float64).T


@pytest.mark.parametrize("P", [1, 3, 33])
@pytest.mark.parametrize("D", [2, 16, 30])
def test_contrastive_head_kernel(P, D):
    _contrastive_head_case(P, D)


@pytest.mark.parametrize("P,D", [(65, 2), (65, 30), (65, 65), (200, 2), (200, 30), (1, 65), (33, 65), (1, 256),
                                 (3, 256), (31, 256)])
def test_contrastive_head_kernel_many_pairs_and_wide_embeddings(P, D):
    """More pairs than the 64 lanes of the loss sum (65, 200) and embeddings wider than a wave (65, 256: the lane loop
    over k wraps).  The last pair is two identical clips (d = 1e-4, the 1e-8 floor: finite gradients, equal to the
    oracle's), and one margin is set to a pair's own fp32 distance (the hinge exactly at zero)."""
    _contrastive_head_case(P, D, identical_last=True)


def _contrastive_head_case(P, D, identical_last=False):
    L = sub("_lib")
    S = 96
    ldw = (D + 31) // 32 * 32
    rng = np.random.default_rng(100 * P + D)
    mean = rng.normal(0, 1, (2 * P, S)).astype(np.float32)
    if identical_last:
        mean[2 * P - 1] = mean[P - 1]
    w2 = rng.normal(0, 0.3, (S, ldw)).astype(np.float32)
    w2[:, D:] = 7.0                        # padding columns: never read
    b2 = rng.normal(0, 0.1, ldw).astype(np.float32)
    labels = np.resize(np.array([1.0, 0.0, 0.25, 0.0, 1.0, 0.6], np.float32), P)
    _, d0, *_ = _np_head(mean, w2, b2, labels, 1.0, D)
    margins = [0.5 * d0.min(), 2.0 * d0.max()] + ([float(np.median(d0))] if P > 1 else [])
    st = torch.cuda.current_stream().cuda_stream
    g_mean, g_w2, g_b2, g_lab = dev(mean), dev(w2), dev(b2), dev(labels)
    if identical_last:
        assert abs(d0[-1] - 1e-4) < 1e-12
        dist = torch.full((P,), np.nan, device=DEV)
        emb = torch.full((2 * P, D), np.nan, device=DEV)
        L.call("srwn_contrastive_head", g_mean.data_ptr(), g_w2.data_ptr(), g_b2.data_ptr(), None, 1.0,
               emb.data_ptr(), dist.data_ptr(), None, None, None, None, 2 * P, S, D, ldw, st)
        torch.cuda.synchronize()
        margins.append(float(dist[0].item()))          # the kernel's own fp32 distance of pair 0: max(0, m - d) == 0
    for margin in margins:
        emb = torch.full((2 * P, D), np.nan, device=DEV)
        dist = torch.full((P,), np.nan, device=DEV)
        loss = torch.full((1,), np.nan, device=DEV)
        gw2 = torch.full((S, ldw), np.nan, device=DEV)
        gb2 = torch.full((ldw,), np.nan, device=DEV)
        dmean = torch.full((2 * P, S), np.nan, device=DEV)
        L.call("srwn_contrastive_head", g_mean.data_ptr(), g_w2.data_ptr(), g_b2.data_ptr(), g_lab.data_ptr(),
               float(margin), emb.data_ptr(), dist.data_ptr(), loss.data_ptr(), gw2.data_ptr(), gb2.data_ptr(),
               dmean.data_ptr(), 2 * P, S, D, ldw, st)
        torch.cuda.synchronize()
        r_emb, r_d, r_loss, r_gw2, r_gb2, r_dmean = _np_head(mean, w2, b2, labels, margin, D)
        assert rel_err(emb.cpu().numpy(), r_emb) < 1e-5, margin
        assert rel_err(dist.cpu().numpy(), r_d) < 1e-5, margin
        assert abs(float(loss.item()) - r_loss) <= 1e-5 * abs(r_loss) + 1e-12, (margin, float(loss.item()), r_loss)
        gw = gw2.cpu().numpy()
        if np.abs(r_gw2).max() > 0:
            assert rel_err(gw[:, :D], r_gw2) < 1e-4, margin
            assert rel_err(dmean.cpu().numpy(), r_dmean) < 1e-4, margin
        else:      # every dissimilar pair beyond the margin and no similar one: no gradient at all
            assert not gw[:, :D].any() and not dmean.cpu().numpy().any()
        assert not gw[:, D:].any(), "padding columns of gw2 must be written as 0"
        assert torch.equal(gb2, torch.zeros_like(gb2)), "gb2 must come out exactly 0"
        assert np.abs(r_gb2).max() < 1e-12
    # without labels: the embedding, and the distance when asked for; nothing else is written
    emb = torch.zeros((2 * P, D), device=DEV)
    dist = torch.zeros((P,), device=DEV)
    gw2 = torch.full((S, ldw), 3.0, device=DEV)
    L.call("srwn_contrastive_head", g_mean.data_ptr(), g_w2.data_ptr(), g_b2.data_ptr(), None, 1.0, emb.data_ptr(),
           dist.data_ptr(), None, gw2.data_ptr(), None, None, 2 * P, S, D, ldw, st)
    emb1 = torch.zeros((1, D), device=DEV)
    L.call("srwn_contrastive_head", g_mean.data_ptr(), g_w2.data_ptr(), g_b2.data_ptr(), None, 1.0, emb1.data_ptr(),
           None, None, None, None, None, 1, S, D, ldw, st)       # one clip: any row count embeds
    torch.cuda.synchronize()
    r_emb, r_d, *_ = _np_head(mean, w2, b2, labels, 1.0, D)
    assert rel_err(emb.cpu().numpy(), r_emb) < 1e-5 and rel_err(dist.cpu().numpy(), r_d) < 1e-5
    assert rel_err(emb1.cpu().numpy(), r_emb[:1]) < 1e-5
    assert bool((gw2 == 3.0).all())


# --- the engine -------------------------------------------------------------------------------------------------
DIL = [1, 2, 4, 8, 16, 32]
R, S, T = 32, 128, 200


def _oracle(sp, audio, labels, margin):
    ts = TorchStack(sp)
    logits = ts.forward(torch.tensor(audio, dtype=torch.float64))           # [2P, T, D]; no RightShift (model.py:692)
    emb = logits.mean(dim=1)                                                # tf.nn.pool AVG over the clip
    loss, d = contrastive_loss(emb, torch.tensor(labels, dtype=torch.float64), margin)
    loss.backward()
    # (the top layer's residual 1x1 feeds nothing, model.py:696-701: no gradient reaches it)
    grads = {n: np.zeros(t.shape) if t.grad is None else t.grad.numpy() for n, t in ts.named(include_cond=False)}
    return emb.detach().numpy(), d.detach().numpy(), float(loss.detach()), grads


def _engine(sp, P, D, dt, margin, lr=1e-3):
    EG = sub("engine")
    cfg = EG.StackConfig(dilations=DIL, dilation_channels=R, skip_channels=S, output_channels=D, dtype=dt,
                         head_mode="contrastive", margin=margin, learning_rate=lr)
    eng = EG.WaveNetEngine(cfg, 2 * P, T, DEV)
    eng.load_oracle_params(sp)
    return eng


def _setup(P=4, D=16, seed=11):
    sp = O.init_stack_params(seed, DIL, 2, R, S, D, bias_scale=0.05)
    audio = O.synthetic_audio(2 * P, T, seed=seed).astype(np.float64)      # left clips, then right ones
    labels = np.resize(np.array([1.0, 0.0, 0.0, 0.25], np.float32), P)
    _, d, _, _ = _oracle(sp, audio, labels, 1.0)
    margin = float(np.median(d))             # pairs on both sides of the margin
    return sp, audio, labels, margin


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_engine_matches_torch_oracle(dt):
    P, D = 4, 16
    sp, audio, labels, margin = _setup(P, D)
    r_emb, r_d, r_loss, r_grads = _oracle(sp, audio, labels, margin)
    eng = _engine(sp, P, D, dt, margin)
    eng.set_inputs(dev(audio), dev(labels))
    eng.forward()
    eng.backward()
    torch.cuda.synchronize()
    got = eng.named_tensors(eng.grads)
    errs = {"emb": rel_err(eng.emb.cpu().numpy(), r_emb), "dist": rel_err(eng.dist.cpu().numpy(), r_d),
            "loss": abs(float(eng.loss.item()) - r_loss) / abs(r_loss)}
    for n, ref in r_grads.items():
        g = got[n].float().cpu().numpy()
        scale = np.abs(ref).max()
        if scale < 1e-12:
            assert not g.any(), n          # head_b2: exactly zero
            continue
        # fp32: the worst element; bf16: the tensor in L2 (relu-mask flips make single entries noisy)
        errs[n] = (np.abs(g - ref).max() / scale if dt == torch.float32 else
                   np.linalg.norm(g - ref) / np.linalg.norm(ref))
    print("contrastive engine %s: worst %s" % (dt, sorted(errs.items(), key=lambda kv: -kv[1])[:6]))
    # bf16: about twice the worst error measured on one MI355X (0.048, head_b1, in L2; fp32 worst 1.3e-5)
    tol = 1e-3 if dt == torch.float32 else 0.1
    for n, e in errs.items():
        assert e < tol, (n, e)


def test_training_lowers_loss_and_graph_replay_equals_eager():
    P, D = 4, 16
    sp, audio, labels, margin = _setup(P, D)
    eng = _engine(sp, P, D, torch.bfloat16, margin, lr=1e-3)
    eng.set_inputs(dev(audio), dev(labels))
    b2 = eng.view("head_b2").clone()
    losses = []
    for _ in range(6):
        eng.train_step()
        losses.append(float(eng.loss.item()))
    assert losses[-1] < losses[0], losses
    assert torch.equal(eng.view("head_b2"), b2), "the loss is translation-invariant: head_b2 must not move"
    # one graph-replayed step == one eager step from the same state
    eng.capture_graphs()
    state = [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v, eng.adam_step)]
    eng.train_step_graphed()
    torch.cuda.synchronize()
    g_loss, g_params, g_dist = eng.loss.clone(), eng.params.clone(), eng.dist.clone()
    for dst, src in zip((eng.params, eng.adam_m, eng.adam_v, eng.adam_step), state):
        dst.copy_(src)
    eng.repack()
    eng.train_step()
    torch.cuda.synchronize()
    assert torch.equal(eng.loss, g_loss) and torch.equal(eng.dist, g_dist)
    assert torch.equal(eng.params, g_params)
    assert torch.equal(eng.view("head_b2"), b2)


# --- the model class ----------------------------------------------------------------------------------------------
def test_siamese_model_train_embed_distance_and_checkpoints(tmp_path):
    M = sub("model")
    SA = sub("simple_audio")
    T2, D = 512, 4
    m = M.SiameseWaveNet(T2, D, DIL, margin=2.0, dilation_channels=R, skip_channels=S, learning_rate=1e-3,
                         dtype=torch.float32)
    rng = np.random.RandomState(5)
    x1, _ = SA.generate_random_wave(T2, rng=rng)
    x2, _ = SA.generate_random_wave(T2, rng=rng)
    d0 = m.get_distance(None, [x1], [x2])
    assert d0.shape == (1,)
    pair_emb = m._engine(2, T2).emb.cpu().numpy().copy()
    e = m.get_embedding(None, [x1, x2])
    assert e.shape == (2, 1, D)
    assert np.array_equal(e[:, 0, :], pair_emb)
    assert rel_err(np.sqrt(1e-8 + ((e[0, 0] - e[1, 0]) ** 2).sum()), d0[0]) < 1e-5
    e2 = m.get_embedding(None, [x2])                 # another batch size, same weights
    assert e2.shape == (1, 1, D) and rel_err(e2[0], e[1]) < 1e-4
    loss, dist = m.train(None, [x1], [x2], [0.0])
    assert isinstance(float(loss), float) and np.ndim(loss) == 0
    assert dist.shape == (1,) and rel_err(dist, d0) < 1e-6           # the distance before the update
    assert abs(float(loss) - 0.5 * max(0.0, 2.0 - d0[0]) ** 2) < 1e-4 * max(1.0, float(loss))
    # batches of pairs, graph-replayed after the second step
    xs = np.array([SA.generate_random_wave(T2, rng=rng)[0] for _ in range(6)], np.float32)
    ys = np.array([1.0, 0.0, 1.0], np.float32)
    l0 = None
    for _ in range(8):
        loss, dist = m.train(None, xs[:3], xs[3:], ys)
        l0 = float(loss) if l0 is None else l0
        assert dist.shape == (3,)
    assert float(loss) < l0
    assert getattr(m._engine(6, T2), "_graph_ready", False)
    with pytest.raises(ValueError):
        m.get_embedding(None, [x1[:-1]])
    with pytest.raises(ValueError):
        m.train(None, xs[:2], xs[2:5], [1.0, 0.0])
    with pytest.raises(ValueError):
        m.get_distance(None, xs[:2], xs[3:4])
    with pytest.raises(ValueError):
        m.train(None, xs[:2], xs[2:4], [1.0])
    names = m.network_params
    assert all(k.startswith("SiameseWaveNet/siamese/") for k in names)
    assert names["SiameseWaveNet/siamese/causal_conv_Kernel"].shape == (2, 1, R)
    assert names["SiameseWaveNet/siamese/conv1d_%d/kernel" % (2 * len(DIL) + 1)].shape == (1, S, D)
    assert "SiameseWaveNet/siamese/dilated_conv_5_gate/dilated_conv_5_Kernel" in names
    for fmt, step in (("pt", 3), ("tf", 4)):
        d = str(tmp_path / fmt)
        assert m.save(None, d, step, force=True, fmt=fmt) is True
        ref = m.get_embedding(None, xs)
        for _ in range(2):
            m.train(None, xs[:3], xs[3:], ys)
        assert not np.array_equal(m.get_embedding(None, xs), ref)
        assert m.load(None, d) is True
        assert np.array_equal(m.get_embedding(None, xs), ref), fmt
    fresh = M.SiameseWaveNet(T2, D, DIL, margin=2.0, dilation_channels=R, skip_channels=S, dtype=torch.float32, seed=9)
    assert fresh.load(None, str(tmp_path / "tf")) is True
    assert np.array_equal(fresh.get_embedding(None, xs), m.get_embedding(None, xs))


def test_siamese_driver_runs(tmp_path):
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "siamese.py"), "--train", "--test", "--steps", "3",
                        "--num-samples", "1024", "--print-steps", "1", "--seed", "0", "--logdir", str(tmp_path / "run")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert sum(1 for l in lines if l.split()[:1] in (["0"], ["1"], ["2"])) == 3, r.stdout[-2000:]
    assert "(2, 1, 2)" in r.stdout
    assert os.path.exists(tmp_path / "run" / "checkpoint")
