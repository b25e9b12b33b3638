"""GPU tests of resumable generation: chunked runs equal one-shot `generate` bit for bit (both bodies, both dtypes, ragged
batches, chunk boundaries around the deepest delay and inside conditioning frames, teacher forcing); the ring fill
against a NumPy restatement of its slot mapping; a primed run continued with teacher forcing against the full forward and
the fp64 oracle; the model classes' prompt and stream API."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev, rel_err

pytestmark = pytest.mark.gpu

DIL = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1, 3]      # d_max = 512
DMAX = max(DIL)
T = DMAX + 90
SCHEDULES = [[1, 1, 7, 128], [DMAX - 1], [DMAX + 1]]      # + the rest
# bf16 primed continuation: 2 x the worst measured on MI355X (SRWN_PRINT_ERR=1 pytest -s prints it).  Against the fp64
# oracle: softmax 6.1e-3, mol 8.6e-3; against the full bf16 forward: 6.5e-3 (fp32: <= 1.3e-6 everywhere)
PRIME_ORACLE_TOL_BF16 = {"softmax": 1.2e-2, "mol": 1.7e-2}
PRIME_FULL_TOL_BF16 = 1.3e-2


def _softmax_engine(dt, seed=4, dil=DIL):
    EG = sub("engine")
    sp = O.init_stack_params(seed, dil, 2, 64, 256, 256, bias_scale=0.05)
    cfg = EG.StackConfig(dilations=dil, dilation_channels=64, skip_channels=256, output_channels=256, shift_input=True,
                         dtype=dt)
    eng = EG.WaveNetEngine(cfg, 1, 64, DEV)
    eng.load_oracle_params(sp)
    return eng, sp


def _mol_engine(dt, E=6, pool=16, M=10, dil=DIL):
    EG = sub("engine")
    sp = O.init_stack_params(7, dil, 2, 64, 256, 4 * M, cond_channels=E, bias_scale=0.05)
    cfg = EG.StackConfig(dilations=dil, dilation_channels=64, skip_channels=256, output_channels=4 * M, cond_channels=E,
                         pool_stride=pool, shift_input=True, head_mode="mol", dtype=dt)
    eng = EG.WaveNetEngine(cfg, 1, pool, DEV)
    eng.load_oracle_params(sp)
    return eng, sp


def _bits(x):
    x = x.contiguous()
    return x.view(torch.int32).cpu().numpy()


def _chunked(eng, B, sched, total, mode, seed, cond=None, forced=None):
    st = eng.generation_state(B, cond, seed)
    out, t = [], 0
    for n in list(sched) + [total - sum(sched)]:
        f = None if forced is None else forced[:, t:t + n]
        out.append(eng.generate_chunk(st, n, mode=mode, forced=f, want_logits=True))
        t += n
    assert st.t == total
    return [torch.cat([o[i] for o in out], dim=1) for i in range(3)]


@pytest.mark.parametrize("B", [1, 33, 70])
@pytest.mark.parametrize("dt,body", [(torch.float32, "0"), (torch.bfloat16, "0"), (torch.bfloat16, "1")])
@pytest.mark.parametrize("case", ["softmax_sample", "softmax_argmax", "mol_cond", "softmax_forced"])
def test_chunked_equals_one_shot(monkeypatch, case, dt, body, B):
    monkeypatch.setenv("SRWN_GEN16", body)
    cond = forced = None
    if case == "mol_cond":
        eng, _ = _mol_engine(dt)
        cond = dev(np.random.default_rng(2).standard_normal((B, -(-T // 16), 6)))
        mode = "sample"
    else:
        eng, _ = _softmax_engine(dt)
        mode = "argmax" if case == "softmax_argmax" else "sample"
        if case == "softmax_forced":
            forced = dev(O.synthetic_audio(B, T, seed=5))
    if dt == torch.bfloat16:
        assert eng.o_g16 is not None
    one = eng.generate(T, mode=mode, seed=13, forced=forced, want_logits=True, batch=B, cond=cond)
    for sched in SCHEDULES:
        got = _chunked(eng, B, sched, T, mode, 13, cond=cond, forced=forced)
        for i in range(3):
            assert np.array_equal(_bits(got[i]), _bits(one[i])), (sched, i)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_forced_chunks_carry_the_forced_samples(dt):
    """The carry a chunk leaves: the forced samples after a forced chunk (the older one still the carried sample after a
    one-step chunk), the emitted ones after a free-running chunk."""
    eng, _ = _softmax_engine(dt, dil=[1, 2, 4, 8])
    B = 5
    f = dev(O.synthetic_audio(B, 40, seed=8))
    st = eng.generation_state(B, None, 3)
    eng.generate_chunk(st, 1, forced=f[:, :1])
    assert torch.equal(st.carry[:, 0], f[:, 0]) and torch.equal(st.carry[:, 1], torch.zeros_like(f[:, 0]))
    eng.generate_chunk(st, 39, forced=f[:, 1:])
    assert torch.equal(st.carry[:, 0], f[:, 39]) and torch.equal(st.carry[:, 1], f[:, 38])
    a, _, _ = eng.generate_chunk(st, 3)
    assert torch.equal(st.carry[:, 0], a[:, 2]) and torch.equal(st.carry[:, 1], a[:, 1])


def _ring_reference(xs, P, dil, B, R):
    """NumPy restatement of srwn_generate_ring_fill: [groups][layers][d+1 slots][32 rows][R]."""
    G = (B + 31) // 32
    out = []
    for g in range(G):
        for l, d in enumerate(dil):
            ring = np.zeros((d + 1, 32, R), xs.dtype)
            for s in range(d + 1):
                ts = [t for t in range(P - 1 - d, P) if t % (d + 1) == s]
                assert len(ts) == 1
                t = ts[0]
                if t < 0:
                    continue
                for row in range(32):
                    u = 32 * g + row
                    if u < B:
                        ring[s, row] = xs[l, u, t]
            out.append(ring.reshape(-1))
    return np.concatenate(out)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 300])
def test_ring_fill_matches_numpy(dt, B, P):
    L_ = sub("_lib")
    K = sub("kernels")
    dil, R, Tsrc = [1, 2, 64, 7, 256], 64, 320
    rng = np.random.default_rng(P + B)
    xs32 = rng.standard_normal((len(dil), B, Tsrc, R)).astype(np.float32)
    xs = torch.tensor(xs32).to(device=DEV, dtype=dt)
    dl = (C.c_int32 * len(dil))(*dil)
    relems = int(L_.load().srwn_generate_ring_elems(dl, len(dil), R))
    G = (B + 31) // 32
    ring = torch.full((relems * G,), float("nan"), dtype=dt, device=DEV)      # every slot must be written
    L_.call("srwn_generate_ring_fill", xs.data_ptr(), B * Tsrc * R, Tsrc, P, dl, len(dil), B, R, ring.data_ptr(),
            K.abi_dtype(dt), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = _ring_reference(xs.cpu().float().numpy() if dt == torch.float32 else xs.cpu().view(torch.int16).numpy(),
                           P, dil, B, R)
    got = ring.cpu().view(torch.int32 if dt == torch.float32 else torch.int16).numpy()
    if dt == torch.float32:
        want = want.view(np.int32)
    assert got.shape == want.shape and np.array_equal(got, want)


def _print_err(what, e):
    if os.environ.get("SRWN_PRINT_ERR"):
        print("MEASURED %s: %.3e" % (what, e))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("P", [0, 1, 5, 512, 513, 300])
def test_prime_then_forced_continuation_softmax(dt, P):
    eng, sp = _softmax_engine(dt)
    B = 3
    audio = O.synthetic_audio(B, T, seed=9)
    codes = O.mu_law_encode(audio, 256)
    full_eng = sub("engine").WaveNetEngine(eng.cfg, B, T, DEV, share_from=eng)
    full_eng.set_inputs(dev(audio), dev(codes, torch.int32))
    full = full_eng.forward(want_logits=True).cpu().numpy()
    st = eng.generation_state(B, None, 1)
    eng.prime(st, dev(audio[:, :P]))
    assert st.t == P
    _, _, lg = eng.generate_chunk(st, T - P, mode="argmax", forced=dev(audio[:, P:]), want_logits=True)
    lg = lg.cpu().numpy()
    assert np.isfinite(lg).all()
    ref, _ = O.stack_forward(sp, audio.astype(np.float64), shift_input=True)
    e_full, e_ref = rel_err(lg, full[:, P:]), rel_err(lg, ref[:, P:])
    _print_err("prime softmax %s P=%d vs full forward / oracle: %.3e /" % (dt, P, e_full), e_ref)
    if dt == torch.float32:
        assert e_full < 1e-3 and e_ref < 1e-3
    else:
        assert e_ref < PRIME_ORACLE_TOL_BF16["softmax"] and e_full < PRIME_FULL_TOL_BF16


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("P", [0, 37, 300, 513])
def test_prime_then_forced_continuation_mol(dt, P):
    """The conditioned decoder, primed over a prompt that ends inside a conditioning frame (pool_stride 16)."""
    eng, sp = _mol_engine(dt)
    B, pool = 3, 16
    Tm = -(-T // pool) * pool
    rng = np.random.default_rng(3)
    audio = O.synthetic_audio(B, Tm, seed=9)
    cond = rng.standard_normal((B, Tm // pool, 6))
    full_eng = sub("engine").WaveNetEngine(eng.cfg, B, Tm, DEV, share_from=eng)
    full_eng.set_inputs(dev(audio), None, dev(cond))
    full = full_eng.forward(want_logits=True).cpu().numpy()
    st = eng.generation_state(B, dev(cond), 1)
    eng.prime(st, dev(audio[:, :P]))
    _, _, lg = eng.generate_chunk(st, Tm - P, mode="sample", forced=dev(audio[:, P:]), want_logits=True)
    lg = lg.cpu().numpy()
    assert np.isfinite(lg).all()
    ref, _ = O.stack_forward(sp, audio.astype(np.float64), shift_input=True, cond=cond, pool_stride=pool)
    e_full, e_ref = rel_err(lg, full[:, P:]), rel_err(lg, ref[:, P:])
    _print_err("prime mol %s P=%d vs full forward / oracle: %.3e /" % (dt, P, e_full), e_ref)
    if dt == torch.float32:
        assert e_full < 1e-3 and e_ref < 1e-3
    else:
        assert e_ref < PRIME_ORACLE_TOL_BF16["mol"] and e_full < PRIME_FULL_TOL_BF16
    with pytest.raises(ValueError):
        eng.generate_chunk(st, 1)                    # past frames * pool_stride
    with pytest.raises(ValueError):
        eng.prime(st, dev(audio[:, :4]))             # a prompt starts a run


def test_teacher_stream_equals_generate_and_prompt_api():
    M = sub("model")
    m = M.WaveNetTeacher(256, 0, [1, 2, 4, 8, 16, 32, 64], dilation_channels=64, skip_channels=256,
                         quantization_channels=256, dtype=torch.bfloat16)
    one = m.generate(3, 500, mode="sample", seed=7)
    blocks = list(m.stream(3, 160, mode="sample", seed=7, max_samples=500))
    assert [b.shape for b in blocks] == [(3, 160)] * 3 + [(3, 20)]
    assert np.array_equal(np.concatenate(blocks, 1).view(np.uint32), one.view(np.uint32))
    prompt = O.synthetic_audio(3, 100, seed=4)
    g = m.generate(3, 200, seed=7, prompt=prompt)
    assert g.shape == (3, 200) and np.isfinite(g).all()
    s = np.concatenate(list(m.stream(3, 64, seed=7, prompt=prompt, max_samples=200)), 1)
    assert np.array_equal(s.view(np.uint32), g.view(np.uint32))
    w = M.WaveNetTeacher(256, 0, [1, 2], dilation_channels=64, skip_channels=256, gate_mode="wavenet")
    with pytest.raises(NotImplementedError, match="wavenet"):
        w.generate(1, 10, prompt=np.zeros((1, 5)))
    with pytest.raises(NotImplementedError, match="wavenet"):
        w.stream(1, 10)
    with pytest.raises(NotImplementedError, match="wavenet"):
        w._engine(1, 256).generation_state(1)


def test_autoencoder_stream_ends_with_the_encoding():
    M = sub("model")
    B, Tc, pool, lat = 2, 256, 32, 8
    ae = M.WaveNetAutoEncoder(input_size=Tc, condition_size=0, num_mixtures=5, dilations=[1, 2, 4, 8, 16],
                              dilation_channels=64, skip_channels=256, latent_channels=lat, pool_stride=pool,
                              dtype=torch.float32)
    x = O.synthetic_audio(B, Tc, seed=2)
    ae.train(x)
    enc = ae.encode(x)
    one = ae.generate(enc, seed=5)
    blocks = list(ae.stream(enc, chunk_size=100, seed=5))
    assert [b.shape[1] for b in blocks] == [100, 100, 56]
    assert np.array_equal(np.concatenate(blocks, 1).view(np.uint32), one.view(np.uint32))
    g = ae.generate(enc, seed=5, prompt=x[:, :70])
    assert g.shape == (B, Tc - 70) and np.abs(g).max() <= 1.0
    s = np.concatenate(list(ae.stream(enc, chunk_size=50, seed=5, prompt=x[:, :70])), 1)
    assert np.array_equal(s.view(np.uint32), g.view(np.uint32))
    with pytest.raises(ValueError):
        ae.generate(enc, seed=5, prompt=x[:, :70], num_samples=Tc)
