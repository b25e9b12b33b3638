"""GPU tests of the canonical WaveNet gate (gate_mode "wavenet": c = tanh(Wf*x + bf) * sigmoid(Wg*x + bg)).

  kernels   srwn_wavenet_layer_fwd / _bwd against oracle/wavenet_np.py (one layer; R 32 / 64, dilations 1 / 64 / 512,
            conditioned and not, a clip length that is not a multiple of the 32-step tile)
  stack     30 layers 3 x [1..512] against oracle/wavenet_torch.py (fp64 autograd): logits, loss and every gradient, the
            gate's included; a conditioned mixture-of-logistics decoder at teacher.py's shapes
  training  graph replay, Adam, the model classes, both checkpoint formats, the refusals
"""
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from oracle import wavenet_torch as OT
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev, rel_err

pytestmark = pytest.mark.gpu

DIL30 = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512] * 3
SQRT_HALF = np.sqrt(0.5)


def _layer(seed, R, d):
    sp = O.init_stack_params(seed, [d], 2, R, 64, 16, bias_scale=0.1)
    return sp.layers[0]


def _images(dt, R, *mats, transposed=False):
    """Packs (for the forward) [Wf | Wg] + Wr, or (for the backward) [WfT | WgT] + WrT (+ WsT)."""
    K = sub("kernels"); P = sub("packing")
    flat = torch.cat([dev(m).flatten() for m in mats])
    pk = K.Packer(DEV)
    offs = []
    if not transposed:
        offs.append(P.pack_conv(pk, 0, 2, R))
        assert P.pack_conv(pk, 2 * R * R, 2, R) == offs[0] + 2 * R * R
        offs.append(P.pack_res(pk, 4 * R * R, R))
    else:
        offs.append(P.pack_conv_T(pk, 0, 2, R))
        assert P.pack_conv_T(pk, 2 * R * R, 2, R) == offs[0] + 2 * R * R
        offs.append(P.pack_linear_T(pk, 4 * R * R, R, R, R, perm=True))
        if len(mats) > 3:
            S = mats[3].shape[1]
            offs.append(P.pack_linear_T(pk, 5 * R * R, R, S, R))
    pk.finalize()
    buf = torch.empty(pk.total, dtype=dt, device=DEV)
    pk.gather(flat, buf)
    es = buf.element_size()
    return buf, [buf.data_ptr() + o * es for o in offs]


@pytest.mark.parametrize("cond", [False, True])
@pytest.mark.parametrize("d", [1, 64, 512])
@pytest.mark.parametrize("R", [32, 64])
def test_wavenet_layer_fwd_vs_oracle(R, d, cond):
    K = sub("kernels")
    B, T, pool = 2, 700, 35
    l = _layer(10 + d, R, d)
    rng = np.random.default_rng(d + R)
    x = dev(rng.standard_normal((B, T, R)))
    dense, _, cache = O.residual_dilation_layer(x.double().cpu().numpy(), l, d, gate_mode="wavenet")
    cb = dev(rng.standard_normal((B, T // pool, R))) if cond else None
    buf, (pc, pr) = _images(torch.float32, R, l.wf, l.wg, l.wr)
    out = [torch.full((B, T, R), float("nan"), device=DEV) for _ in range(4)]
    K.wavenet_layer_fwd(x, cb, pc, pr, dev(l.bf), dev(l.bg), dev(l.br), *out, 2, d, pool)
    torch.cuda.synchronize()
    h, z, s, c = [t.cpu().numpy() for t in out]
    if cond:
        dense = dense + np.repeat(cb.double().cpu().numpy(), pool, axis=1)
    for name, got, want in (("z", z, cache["z"]), ("s", s, cache["s"]), ("c", c, cache["c"]), ("h", h, dense)):
        assert rel_err(got, want) < 1e-4, name


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_wavenet_layer_fwd_bf16_matches_fp32_scale(dt):
    """The bf16 instantiation computes the same layer within bf16 rounding (3e-2 of the tensor scale)."""
    K = sub("kernels")
    R, B, T, d = 64, 2, 300, 4
    l = _layer(3, R, d)
    x = dev(np.random.default_rng(1).standard_normal((B, T, R)), dt)
    dense, _, cache = O.residual_dilation_layer(x.double().cpu().numpy(), l, d, gate_mode="wavenet")
    buf, (pc, pr) = _images(dt, R, l.wf, l.wg, l.wr)
    out = [torch.full((B, T, R), float("nan"), dtype=dt, device=DEV) for _ in range(4)]
    K.wavenet_layer_fwd(x, None, pc, pr, dev(l.bf), dev(l.bg), dev(l.br), *out, 2, d)
    tol = 1e-4 if dt == torch.float32 else 3e-2
    assert rel_err(out[0].float().cpu().numpy(), dense) < tol
    assert rel_err(out[3].float().cpu().numpy(), cache["c"]) < tol


def _conv_dgrad(w, d, dy):
    dx, _ = O._conv_backward(np.zeros(dy.shape[:2] + (w.shape[1],)), w, d, dy)
    return dx


@pytest.mark.parametrize("skip", ["dcs", "dtotal"])
@pytest.mark.parametrize("cond", [False, True])
@pytest.mark.parametrize("d", [1, 64, 512])
@pytest.mark.parametrize("R", [32, 64])
def test_wavenet_layer_bwd_vs_oracle(R, d, cond, skip):
    """One UP + DOWN call: G_{l+1} from D_{l+1} (layer l+1 at dilation d) and D_l of layer l, against the oracle's
    formulas (stack_backward, gate_mode "wavenet").  `cond` runs the stored layer outputs of a conditioned forward."""
    K = sub("kernels")
    B, T, S = 2, 700, 128
    lo, up = _layer(20 + d, R, 1), _layer(30 + d, R, d)
    sp = O.init_stack_params(40 + d, [1], 2, R, S, 16, bias_scale=0.1)
    ws = sp.layers[0].ws
    rng = np.random.default_rng(R + d + cond)
    x = rng.standard_normal((B, T, R))
    if cond:
        x = x + np.repeat(rng.standard_normal((B, T // 35, R)), 35, axis=1)
    _, _, cache = O.residual_dilation_layer(x, lo, 1, gate_mode="wavenet")
    g_in = rng.standard_normal((B, T, R))
    d_up = rng.standard_normal((B, T, 2 * R)) * 0.5
    dtotal = rng.standard_normal((B, T, S)) * 0.3
    G = g_in * SQRT_HALF + _conv_dgrad(up.wf, d, d_up[..., :R]) + _conv_dgrad(up.wg, d, d_up[..., R:])
    dc = (G * SQRT_HALF) @ lo.wr.T + dtotal @ ws.T
    z, s = cache["z"], cache["s"]
    D = np.concatenate([dc * s * (1 - z * z), dc * z * s * (1 - s)], axis=-1)
    buf, ptrs = _images(torch.float32, R, up.wf, up.wg, lo.wr, ws, transposed=True)
    g_out = torch.full((B, T, R), float("nan"), device=DEV)
    d_out = torch.full((B, T, 2 * R), float("nan"), device=DEV)
    dcs = dev(dtotal @ ws.T) if skip == "dcs" else None
    wsk, dtt = (None, None) if skip == "dcs" else (ptrs[2], dev(dtotal))
    K.wavenet_layer_bwd(dev(g_in), dev(d_up), ptrs[0], g_out, ptrs[1], wsk, dtt, dcs, dev(z), dev(s), d_out, B, T, R, S,
                        2, d, True, True, torch.float32)
    torch.cuda.synchronize()
    assert rel_err(g_out.cpu().numpy(), G) < 1e-4
    assert rel_err(d_out.cpu().numpy(), D) < 1e-4
    # the two one-sided calls of the chain: the top layer (DOWN only, G = 0) and below layer 0 (UP only, no g_in)
    d_top = torch.full((B, T, 2 * R), float("nan"), device=DEV)
    K.wavenet_layer_bwd(None, None, None, None, None, wsk, dtt, dcs, dev(z), dev(s), d_top, B, T, R, S, 2, 1, False, True,
                        torch.float32)
    dc0 = dtotal @ ws.T
    assert rel_err(d_top.cpu().numpy(), np.concatenate([dc0 * s * (1 - z * z), dc0 * z * s * (1 - s)], -1)) < 1e-4
    g0 = torch.full((B, T, R), float("nan"), device=DEV)
    K.wavenet_layer_bwd(None, dev(d_up), ptrs[0], g0, None, None, None, None, None, None, None, B, T, R, S, 2, d, True,
                        False, torch.float32)
    assert rel_err(g0.cpu().numpy(), G - g_in * SQRT_HALF) < 1e-4


# ------------------------------------------------------------------------------------------------
# stack parity
# ------------------------------------------------------------------------------------------------
def _torch_oracle(sp, audio, *, codes=None, cond=None, pool=1):
    st = OT.TorchStack(sp)
    c = None if cond is None else torch.tensor(cond)
    logits = st.forward(torch.tensor(audio), shift_input=True, cond=c, pool_stride=pool, gate_mode="wavenet")
    if codes is not None:
        loss = OT.loss_per_timestep(logits, torch.tensor(codes))
    else:
        loss = OT.mol_loss_sum(torch.tensor(audio), logits)
    loss.backward()
    grads = {n: (np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()) for n, t in st.named(cond is not None)}
    for i, l in enumerate(st.layers):
        grads[f"l{i}.wg"] = l["wg"].grad.numpy()
        grads[f"l{i}.bg"] = l["bg"].grad.numpy()
    return logits.detach().numpy(), float(loss.detach()), grads


def _wn_engine(sp, dil, B, T, R, S, C, dt, **kw):
    EG = sub("engine")
    cfg = EG.StackConfig(dilations=list(dil), dilation_channels=R, skip_channels=S, output_channels=C, shift_input=True,
                         dtype=dt, gate_mode="wavenet", **kw)
    eng = EG.WaveNetEngine(cfg, B, T, DEV)
    eng.load_oracle_params(sp)
    return eng


def _compare(eng, logits, loss, grads, dt, bounds):
    lg = eng.forward(want_logits=True).cpu().numpy()
    eng.backward()
    torch.cuda.synchronize()
    got = eng.named_tensors(eng.grads)
    for i in range(eng.L):      # the gate's gradients exist and are not zero
        assert float(got[f"l{i}.wg"].abs().max()) > 0 and float(got[f"l{i}.bg"].abs().max()) > 0, i
    if dt == torch.float32:
        assert rel_err(lg, logits) < 1e-3
        assert abs(float(eng.loss.item()) - loss) < 1e-3 * abs(loss)
        for n, ref in grads.items():
            g = got[n].cpu().numpy()
            assert np.abs(g - ref).max() < 1e-3 * max(np.abs(ref).max(), 1e-12), n
        return
    errs = {"logits": rel_err(lg, logits), "loss": abs(float(eng.loss.item()) - loss) / abs(loss)}
    for n, ref in grads.items():
        g = got[n].float().cpu().numpy().ravel().astype(np.float64)
        r = ref.ravel()
        if not r.any():
            assert not g.any(), n
            continue
        errs[n] = float(np.linalg.norm(g - r) / np.linalg.norm(r))
    worst = max((v, k) for k, v in errs.items() if k not in ("logits", "loss"))
    print("bf16 errors: logits %.3g loss %.3g worst gradient %.3g (%s)" % (errs["logits"], errs["loss"], *worst))
    assert errs["logits"] < bounds[0], errs["logits"]
    assert errs["loss"] < bounds[1], errs["loss"]
    assert worst[0] < bounds[2], worst


# bf16 bounds: 2x the errors measured on one MI355X (logits max-relative, loss relative, worst per-tensor relative L2
# gradient error).  Measured: config 2 depth 4.76e-3 / 1.27e-5 / 1.92e-2 (l13.bg); conditioned MoL decoder
# 7.15e-3 / 1.63e-4 / 4.62e-2 (l28.wr)
BF16_CONFIG2 = (9.5e-3, 2.6e-5, 3.9e-2)
BF16_MOL = (1.43e-2, 3.3e-4, 9.3e-2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_config2_depth_wavenet_gate_vs_oracle(dt):
    """30 layers, 3 x [1..512], 64 residual / 256 skip channels, 256-way softmax, B = 2 clips of 4300 samples."""
    B, T, R, S, C = 2, 4300, 64, 256, 256
    sp = O.init_stack_params(3, DIL30, 2, R, S, C, bias_scale=0.05)
    audio = O.synthetic_audio(B, T, seed=4).astype(np.float64)
    codes = O.mu_law_encode(audio.astype(np.float32), C).astype(np.int64)
    logits, loss, grads = _torch_oracle(sp, audio, codes=codes)
    eng = _wn_engine(sp, DIL30, B, T, R, S, C, dt)
    assert not eng.fused_bwd and not eng.fused_wt and not eng.use_wl
    eng.set_inputs(dev(audio), dev(codes, torch.int32))
    _compare(eng, logits, loss, grads, dt, BF16_CONFIG2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_conditioned_mol_decoder_wavenet_gate_vs_oracle(dt):
    """teacher.py's decoder shapes: 30 layers, 32 residual / 128 skip channels, 5 logistics, 16 latent channels
    upsampled by 512, 4096-sample clips (batch 2)."""
    B, T, R, S, M, E, pool = 2, 4096, 32, 128, 5, 16, 512
    sp = O.init_stack_params(7, DIL30, 2, R, S, 4 * M, cond_channels=E, bias_scale=0.05)
    audio = O.synthetic_audio(B, T, seed=8).astype(np.float64)
    cond = np.random.default_rng(9).standard_normal((B, T // pool, E))
    logits, loss, grads = _torch_oracle(sp, audio, cond=cond, pool=pool)
    eng = _wn_engine(sp, DIL30, B, T, R, S, 4 * M, dt, cond_channels=E, pool_stride=pool, head_mode="mol")
    eng.set_inputs(dev(audio), None, dev(cond))
    _compare(eng, logits, loss, grads, dt, BF16_MOL)


# ------------------------------------------------------------------------------------------------
# training
# ------------------------------------------------------------------------------------------------
def _small(dt=torch.float32, lr=1e-3):
    B, T, R, S, C = 2, 600, 64, 256, 256
    dil = [1, 2, 4, 8, 16, 32]
    sp = O.init_stack_params(5, dil, 2, R, S, C, bias_scale=0.05)
    audio = O.synthetic_audio(B, T, seed=2).astype(np.float64)
    codes = O.mu_law_encode(audio.astype(np.float32), C)
    eng = _wn_engine(sp, dil, B, T, R, S, C, dt, learning_rate=lr)
    eng.set_inputs(dev(audio), dev(codes, torch.int32))
    return eng, sp, audio, codes


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_graphed_step_is_bit_equal_to_eager(dt):
    a, sp, audio, codes = _small(dt)
    b, _, _, _ = _small(dt)
    for _ in range(2):
        a.train_step(); b.train_step()
    b.capture_graphs()
    for _ in range(3):
        la = float(a.train_step().item())
        lb = float(b.train_step_graphed().item())
        torch.cuda.synchronize()
        assert la == lb
        assert torch.equal(a.params, b.params) and torch.equal(a.grads, b.grads)


def test_adam_steps_lower_the_loss_and_train_the_gate():
    eng, sp, audio, codes = _small(lr=3e-3)
    wg0 = eng.view("WG").clone(); bg0 = eng.view("BG").clone()
    l0 = float(eng.train_step().item())
    for _ in range(8):
        l1 = float(eng.train_step().item())
    assert l1 < l0, (l0, l1)
    assert not torch.equal(eng.view("WG"), wg0) and not torch.equal(eng.view("BG"), bg0)


def _model_classes():
    return sub("model")


def test_wavenet_class_trains_and_checkpoints_restore(tmp_path):
    M = _model_classes()
    B, T, C = 4, 512, 8
    rng = np.random.default_rng(0)
    x = O.synthetic_audio(B, T, seed=3).astype(np.float32)
    y = np.eye(C, dtype=np.float32)[rng.integers(0, C, B)]
    m = M.WaveNet(T, C, [1, 2, 4, 8], dilation_channels=32, skip_channels=128, output_channels=C, dtype=torch.float32,
                  gate_mode="wavenet")
    losses = [float(m.train(x, y)) for _ in range(10)]
    assert losses[-1] < losses[0]
    p = m.predict(x)
    for fmt in ("pt", "tf"):
        d = str(tmp_path / fmt)
        assert m.save(d, 10, force=True, fmt=fmt)
        m2 = M.WaveNet(T, C, [1, 2, 4, 8], dilation_channels=32, skip_channels=128, output_channels=C,
                       dtype=torch.float32, gate_mode="wavenet", seed=7)
        assert m2.load(d)
        assert np.array_equal(m2.predict(x), p), fmt
        names = m2.network_params
        assert "WaveNet/dilated_conv_0_gate/dilated_conv_0_Kernel" in names


def test_teacher_trains_checkpoints_and_rebuilds_from_config(tmp_path):
    import json
    M = _model_classes()
    T = 400
    x = O.synthetic_audio(2, T, seed=5).astype(np.float32)
    kw = dict(dilation_channels=32, skip_channels=128, dtype=torch.float32)
    m = M.WaveNetTeacher(T, 0, [1, 2, 4, 8, 16], gate_mode="wavenet", **kw)
    l0 = float(m.train(x))
    for _ in range(6):
        l1 = float(m.train(x))
    assert l1 < l0
    lg = m.get_logits(x)
    gate = m.network_params["WaveNetTeacher/dilated_conv_0_gate/dilated_conv_0_Kernel"]
    assert torch.equal(gate, m._primary.view("WG")[0])
    for fmt in ("pt", "tf"):
        d = str(tmp_path / fmt)
        assert m.save(d, 7, force=True, fmt=fmt)
        assert json.load(open(os.path.join(d, "config.json")))["gate_mode"] == "wavenet"
        r = M.WaveNetTeacher.from_checkpoint(d, dtype=torch.float32)
        assert r.gate_mode == "wavenet" and r._cfg.gate_mode == "wavenet"
        assert np.array_equal(r.get_logits(x), lg), fmt
    # a config.json written before the option existed loads as the reference gate
    d = str(tmp_path / "pt")
    cfg = json.load(open(os.path.join(d, "config.json")))
    del cfg["gate_mode"]
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    assert M.WaveNetTeacher.from_checkpoint(d, dtype=torch.float32).gate_mode == "reference"


def test_generation_and_distillation_refuse_the_wavenet_gate():
    M = _model_classes()
    m = M.WaveNetTeacher(256, 0, [1, 2, 4], dilation_channels=32, skip_channels=128, dtype=torch.float32,
                         gate_mode="wavenet")
    with pytest.raises(NotImplementedError, match="wavenet"):
        m.generate(1, 16)
    eng = m._engine(1, 256)
    with pytest.raises(NotImplementedError, match="wavenet"):
        eng.generate(16)
    mol = M.WaveNetTeacher(256, 0, [1, 2, 4], dilation_channels=32, skip_channels=128, dtype=torch.float32,
                           head="mol", use_encoding=True, pool_stride=32, gate_mode="wavenet")
    with pytest.raises(ValueError, match="gate_mode"):
        M.ParallelWaveNet(256, 0, [1, 2, 4], mol, pool_stride=32)
