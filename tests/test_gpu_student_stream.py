"""GPU tests of chunked student synthesis (student.FlowSynthesizer, model.StudentSynthesizer): chunking is invisible
bit for bit, the bits are the training engine's, any shape on one object with no teacher, the device noise, the memory
footprint, refused calls."""
import math

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev, rel_err
from tests.test_gpu_student import _setup

pytestmark = pytest.mark.gpu

D512 = [2 ** i for i in range(10)]


def _synth(dt, R, dil, F, E, pool, max_batch, max_chunk, max_frames, seed=50):
    EG = sub("engine"); ST = sub("student")
    cfg = EG.StackConfig(dilations=list(dil), dilation_channels=R, skip_channels=4 * R, cond_channels=E, pool_stride=pool,
                         dtype=dt)
    syn = ST.FlowSynthesizer(cfg, F, max_batch=max_batch, max_chunk=max_chunk, max_frames=max_frames)
    flows = [O.init_flow_params(seed + i, list(dil), 2, R, 4 * R, E, bias_scale=0.05) for i in range(F)]
    for w, p in zip(syn.weights, flows):
        p.head_w2 = p.head_w2 * 0.3      # keep exp(.) moderate so that the clamp does not hide differences
        w.load_oracle_params(p)
    return syn, flows


def _run(syn, cond, chunks, noise=None, seeds=0, temperature=1.0):
    st = syn.start(cond, seeds, temperature)
    out, t = [], 0
    for n in chunks:
        out.append(syn.step(st, n, None if noise is None else noise[:, t:t + n]))
        t += n
    torch.cuda.synchronize()
    return torch.cat(out, 1)


def _schedules(T):
    heads = [[1, 1, 7, 128], [30, 31, 32], [991, 992, 993], [160] * ((T - 1) // 160)]
    return [h + [T - sum(h)] for h in heads if sum(h) < T]


# ---------------------------------------------------------------------------------------------------
# 3. chunking is invisible
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,R,dil,F,B,T,pool", [
    (torch.bfloat16, 64, D512 * 3, 2, 1, 4096, 512),             # the 3 x [1..512] stack: history rows 31 / 992
    (torch.float32, 32, D512[:8] * 2, 2, 3, 2048, 64),
    (torch.bfloat16, 32, D512 + [1024], 1, 3, 4096, 256),        # a plan that ends in a group of one layer
    (torch.float32, 64, [1, 2, 4, 8], 3, 1, 1024, 128)])
def test_chunking_is_invisible(dt, R, dil, F, B, T, pool):
    E = 5
    syn, _ = _synth(dt, R, dil, F, E, pool, B, T, T // pool)
    rng = np.random.default_rng(T + R)
    cond = torch.tensor(rng.standard_normal((B, T // pool, E)), dtype=torch.float32)
    noise = dev(rng.logistic(0, 1, (B, T)) * 0.3)
    seeds = [11 + 5 * b for b in range(B)]
    syn.use_graphs = False
    one_given = _run(syn, cond, [T], noise)
    one_dev = _run(syn, cond, [T], None, seeds)
    assert torch.isfinite(one_given).all() and float(one_given.abs().max()) <= 1.0
    assert (one_given.abs() < 1).float().mean() > 0.5 and not torch.equal(one_given, one_dev)
    for graphs in (False, True):
        syn.use_graphs = graphs
        for chunks in _schedules(T):
            assert torch.equal(_run(syn, cond, chunks, noise), one_given), (graphs, chunks[:4])
            assert torch.equal(_run(syn, cond, chunks, None, seeds), one_dev), (graphs, chunks[:4])
    assert syn._graphs, "the repeated chunk sizes were captured and replayed"


def test_single_samples_and_the_overlapping_history_roll():
    """n = 1 for many chunks in a row (every roll overlaps itself), then odd sizes below the history lengths."""
    dil, B, T, pool, E = D512[:7], 2, 512, 64, 4
    syn, _ = _synth(torch.bfloat16, 64, dil, 2, E, pool, B, T, T // pool)
    rng = np.random.default_rng(3)
    cond = torch.tensor(rng.standard_normal((B, T // pool, E)), dtype=torch.float32)
    noise = dev(rng.logistic(0, 1, (B, T)) * 0.3)
    ref = _run(syn, cond, [T], noise)
    chunks = [1] * 70 + [2, 3, 5, 29, 95, 97]
    chunks.append(T - sum(chunks))
    assert torch.equal(_run(syn, cond, chunks, noise), ref)


# ---------------------------------------------------------------------------------------------------
# 4. the training engine's bits; the fp64 oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-3), (torch.bfloat16, 6e-2)])
@pytest.mark.parametrize("R,S,F,B,T,pool", [(64, 256, 2, 2, 1024, 64), (32, 128, 3, 2, 1024, 64), (32, 128, 2, 3, 640, 128)])
def test_same_bits_as_the_training_engine(dt, tol, R, S, F, B, T, pool):
    ST = sub("student")
    stu, flows, noise, cond, *_ = _setup(dt, R, S, F, B=B, T=T, pool=pool)
    stu.forward_flows()
    torch.cuda.synchronize()
    want = stu.out.view(B, T).clone()
    syn = ST.FlowSynthesizer(stu.flows[0].cfg, F, max_batch=B, max_chunk=T, max_frames=T // pool)
    for w, f in zip(syn.weights, stu.flows):
        w.params.copy_(f.params)
    syn.repack()
    nz = dev(noise)
    for chunks in ([T], [100, 1, 300, T - 401]):
        assert torch.equal(_run(syn, torch.tensor(cond, dtype=torch.float32), chunks, nz), want), chunks
    fw = O.student_forward(flows, noise, cond, pool)
    assert rel_err(want.cpu().numpy(), fw["out"]) < tol


def test_model_surface_any_shape_and_no_teacher(tmp_path, monkeypatch):
    """ParallelWaveNet.synthesizer() == ParallelWaveNet.generate bit for bit; two (B, T) in turn on one synthesizer, one
    several times the model's input_size; from_checkpoint with every training class made unconstructible."""
    M = sub("model"); ST = sub("student"); EG = sub("engine")
    dil = [1, 2, 4, 8, 16, 32]
    B, T, pool, lat, cs = 2, 1024, 64, 8, 4
    teacher = M.WaveNetTeacher(T, cs, dil, dilation_channels=64, skip_channels=256, latent_channels=lat, pool_stride=pool,
                               use_encoding=True, head="mol", num_mixtures=5, dtype=torch.bfloat16)
    student = M.ParallelWaveNet(input_size=T, condition_size=cs, dilations=dil, teacher=teacher, dilation_channels=64,
                                skip_channels=128, num_flows=2, latent_channels=lat, pool_stride=pool, gamma=1e-3,
                                dtype=torch.bfloat16)
    rng = np.random.default_rng(0)
    x = O.synthetic_audio(B, T, seed=3)
    enc = rng.standard_normal((B, T // pool, lat)).astype(np.float32)
    y = np.eye(cs, dtype=np.float32)[[0, 2]]
    noise = (rng.logistic(0, 1, (B, T)) * 0.5).astype(np.float32)
    for _ in range(2):
        student.train_fast(None, noise, x, enc, y)
    want = student.generate(None, noise, enc, y)
    syn = student.synthesizer(max_batch=3, max_chunk=700, max_frames=5 * T // pool)
    got = syn.synthesize(enc, y, noise=noise)
    assert got.shape == (B, T, 1) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    blocks = list(syn.stream(enc, y, chunk_size=160, noise=noise))
    assert [b.shape for b in blocks] == [(B, 160, 1)] * 6 + [(B, 64, 1)]
    assert np.array_equal(np.concatenate(blocks, 1).view(np.uint32), want.view(np.uint32))
    # a snapshot: more training changes the model, not the synthesizer
    student.train_fast(None, noise, x, enc, y)
    assert np.array_equal(syn.synthesize(enc, y, noise=noise), got)
    assert not np.array_equal(student.generate(None, noise, enc, y), want)
    # another (B, T) on the same object: three streams, five times the model's input_size
    T5 = 5 * T
    enc5 = rng.standard_normal((3, T5 // pool, lat)).astype(np.float32)
    y5 = np.eye(cs, dtype=np.float32)[[1, 3, 0]]
    long = syn.synthesize(enc5, y5, seed=[4, 5, 6], temperature=0.7)
    assert long.shape == (3, T5, 1) and np.isfinite(long).all() and np.abs(long).max() <= 1.0
    assert np.array_equal(np.concatenate(list(syn.stream(enc5, y5, chunk_size=333, seed=[4, 5, 6], temperature=0.7)), 1), long)
    assert np.array_equal(syn.synthesize(enc, y, noise=noise), got)            # and back
    # from a checkpoint, with no training class constructible
    sdir = str(tmp_path / "student")
    assert student.save(None, sdir, 3, force=True)
    saved = student.generate(None, noise, enc, y)

    def refuse(self, *a, **k):
        raise AssertionError("a training class was constructed")
    for cls in (M.WaveNetTeacher, M.WaveNetAutoEncoder, ST.StudentEngine, ST.FlowStack, EG.WaveNetEngine):
        monkeypatch.setattr(cls, "__init__", refuse)
    dep = M.StudentSynthesizer.from_checkpoint(sdir, dil, 2, dilation_channels=64, latent_channels=lat, condition_size=cs,
                                               pool_stride=pool, dtype=torch.bfloat16, max_batch=2, max_chunk=512,
                                               max_frames=T // pool)
    assert np.array_equal(dep.synthesize(enc, y, noise=noise).view(np.uint32), saved.view(np.uint32))
    with pytest.raises(FileNotFoundError):
        M.StudentSynthesizer.from_checkpoint(str(tmp_path / "nothing"), dil, 2, dilation_channels=64, latent_channels=lat,
                                             condition_size=cs, pool_stride=pool, dtype=torch.bfloat16)


# ---------------------------------------------------------------------------------------------------
# 6. noise
# ---------------------------------------------------------------------------------------------------
def _mix(seed, idx):
    """splitmix64 of (seed, index) as csrc/srwn_ops.hip mixes it; the top 23 bits."""
    m = (1 << 64) - 1
    z = (np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx.astype(np.uint64) + np.uint64(1)))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(41)).astype(np.int64) & 0x7fffff


def _noise(seeds, temps, clock, n, stride=None):
    L = sub("_lib")
    B = len(seeds)
    stride = stride or n
    out = torch.zeros(B, stride, device=DEV)
    sd = torch.tensor(seeds, dtype=torch.int64, device=DEV); tp = torch.tensor(temps, dtype=torch.float32, device=DEV)
    ck = torch.tensor([clock], dtype=torch.int64, device=DEV)
    L.call("srwn_logistic_noise", out.data_ptr(), stride, tp.data_ptr(), sd.data_ptr(), ck.data_ptr(), B, n,
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out[:, :n].cpu().numpy()


# Worst relative error of a draw against the fp64 restatement on the same uniforms, measured on an MI355X over the 10^6
# draws of test_logistic_noise (HIP's log1pf and the division are not exact): 1.1376e-07, i.e. just under two fp32
# ulp; the smallest |draw| among them is 2.1e-06.  The bound is 4 x that.
NOISE_REL_ERR_MEASURED = 1.14e-7


def test_logistic_noise():
    n = 1000000
    k = _mix(12345, np.arange(n))
    u = (k + 0.5) / 2 ** 23
    ref = np.log(u) - np.log1p(-u)
    got = _noise([12345], [1.0], 0, n)[0].astype(np.float64)
    assert np.isfinite(got).all()
    relerr = np.abs(got - ref) / np.abs(ref)
    print("logistic noise: worst relative error over %d draws %.4e (smallest |draw| %.3e)" % (n, relerr.max(), np.abs(ref).min()))
    assert 4 * NOISE_REL_ERR_MEASURED < 1e-4      # (a bound above that would mean something else is wrong)
    assert relerr.max() <= 4 * NOISE_REL_ERR_MEASURED
    # moments: logistic(0, 1) has variance pi^2 / 3 and excess kurtosis 1.2
    var = math.pi ** 2 / 3
    assert abs(got.mean()) < 5 * math.sqrt(var) / 1e3
    assert abs(got.var() - var) < 5 * var * math.sqrt(3.2 / n)
    # chunks == one call; a stream's row does not depend on the batch it is in or on its row
    a = _noise([12345], [1.0], 0, 1000)[0]
    b = np.concatenate([_noise([12345], [1.0], c, m)[0] for c, m in ((0, 1), (1, 499), (500, 500))])
    assert np.array_equal(a, got[:1000].astype(np.float32)) and np.array_equal(a, b)
    batch = _noise([7, 12345, 9], [1.0, 1.0, 1.0], 0, 1000, stride=1024)
    assert np.array_equal(batch[1], a) and not np.array_equal(batch[0], a)
    # temperatures scale their own rows only; zero gives +0
    tb = _noise([7, 12345, 9], [0.5, 1.0, 0.0], 0, 1000)
    assert np.array_equal(tb[0], np.float32(0.5) * batch[0]) and np.array_equal(tb[1], a)
    assert not tb[2].any() and not np.signbit(tb[2]).any()
    # the ends of the bit-to-uniform map
    L = sub("_lib")
    bits = torch.tensor([0, 2 ** 23 - 1, 2 ** 22], dtype=torch.int32, device=DEV)
    out = torch.zeros(3, device=DEV)
    L.call("srwn_logistic_from_bits", bits.data_ptr(), out.data_ptr(), 3, torch.cuda.current_stream().cuda_stream)
    lo, hi, mid = out.cpu().numpy().astype(np.float64)
    assert np.isfinite([lo, hi, mid]).all()
    assert abs(lo + 24 * math.log(2)) < 1e-4 and abs(hi - 24 * math.log(2)) < 1e-4 and abs(mid) < 1e-6


def test_synthesizer_noise_controls():
    dil, B, T, pool, E = D512[:6], 3, 512, 64, 4
    syn, _ = _synth(torch.bfloat16, 32, dil, 2, E, pool, B, T, T // pool)
    rng = np.random.default_rng(5)
    cond = torch.tensor(rng.standard_normal((B, T // pool, E)), dtype=torch.float32)
    seeds = [3, 1000, 77]
    full = _run(syn, cond, [T], None, seeds)
    for b in range(B):      # stream b of a batch == a batch of one with the same seed
        assert torch.equal(_run(syn, cond[b:b + 1], [200, T - 200], None, [seeds[b]])[0], full[b])
    zero = _run(syn, cond, [T], torch.zeros(B, T, device=DEV))
    assert torch.equal(_run(syn, cond, [T], None, seeds, 0.0), zero)
    mixed = _run(syn, cond, [T], None, seeds, [1.0, 0.0, 1.0])
    assert torch.equal(mixed[0], full[0]) and torch.equal(mixed[2], full[2]) and torch.equal(mixed[1], zero[1])
    assert torch.equal(_run(syn, cond, [T], None, 3)[0], full[0])      # a scalar seed s: stream b draws with s + b


# ---------------------------------------------------------------------------------------------------
# 7. footprint, 8. refused calls
# ---------------------------------------------------------------------------------------------------
def test_footprint():
    ST = sub("student"); EG = sub("engine")
    dil, R, E, F, B, C, frames, pool = D512 * 3, 64, 16, 4, 2, 1600, 32, 512
    L, elt, Ep = len(dil), 2, 16
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    cfg = EG.StackConfig(dilations=dil, dilation_channels=R, cond_channels=E, pool_stride=pool, dtype=torch.bfloat16)
    syn = ST.FlowSynthesizer(cfg, F, max_batch=B, max_chunk=C, max_frames=frames)
    st = syn.start(torch.zeros(B, frames, E))
    syn.step(st, C)
    torch.cuda.synchronize()
    used = torch.cuda.memory_allocated() - before
    hist = ST.stream_history_rows(dil)
    assert hist == [31, 992] * 3
    weights = F * (ST.FlowWeights.param_count(cfg) * 4 + (L * 2 * R * R + L * R * R + L * R * Ep) * elt)
    boundary = F * sum(B * (h + C) * R * elt for h in hist)
    tables = F * B * frames * L * R * elt
    print("synthesizer footprint %.2f MB; weights %.2f, boundary buffers %.2f, conditioning tables %.2f"
          % (used / 2 ** 20, weights / 2 ** 20, boundary / 2 ** 20, tables / 2 ** 20))
    assert used <= 1.5 * (weights + boundary + tables) + 4 * 2 ** 20


def test_refused_calls_leave_the_state_alone():
    dil, B, T, pool, E = [1, 2, 4, 8], 2, 256, 64, 4
    syn, _ = _synth(torch.float32, 32, dil, 2, E, pool, B, 100, T // pool)
    rng = np.random.default_rng(9)
    cond = torch.tensor(rng.standard_normal((B, T // pool, E)), dtype=torch.float32)
    noise = dev(rng.logistic(0, 1, (B, T)) * 0.3)
    ref = _run(syn, cond, [100, 100, 56], noise)
    st = syn.start(cond)
    a = syn.step(st, 100, noise[:, :100])
    for bad in (0, 101, -3):
        with pytest.raises(ValueError, match="max_chunk"):
            syn.step(st, bad)
    with pytest.raises(ValueError, match="noise"):
        syn.step(st, 50, noise[:, :49])
    b = syn.step(st, 100, noise[:, 100:200])
    with pytest.raises(ValueError, match="ends"):
        syn.step(st, 57, noise[:, 200:257])      # one sample past frames * pool_stride
    c = syn.step(st, 56, noise[:, 200:])
    with pytest.raises(ValueError, match="ends"):
        syn.step(st, 1)
    assert torch.equal(torch.cat([a, b, c], 1), ref)
    with pytest.raises(ValueError):
        syn.start(cond[:, :, :3])
    with pytest.raises(ValueError):
        syn.start(torch.zeros(3, 4, E))                  # more streams than max_batch
    with pytest.raises(ValueError):
        syn.start(torch.zeros(2, 5, E))                  # more frames than max_frames
    M = sub("model")
    ms = M.StudentSynthesizer(dil, 2, dilation_channels=32, latent_channels=3, condition_size=2, pool_stride=64,
                              dtype=torch.float32, max_batch=2, max_chunk=128, max_frames=4)
    enc = np.zeros((2, 4, 3), np.float32)
    with pytest.raises(ValueError, match="conditions"):
        ms.synthesize(enc)
    with pytest.raises(ValueError, match="encoding"):
        ms.synthesize(np.zeros((2, 4, 5), np.float32), np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match="max_frames"):
        ms.stream(np.zeros((2, 5, 3), np.float32), np.zeros((2, 2), np.float32), chunk_size=64)
    with pytest.raises(ValueError, match="chunk_size"):
        ms.stream(enc, np.zeros((2, 2), np.float32), chunk_size=129)
    with pytest.raises(ValueError, match="noise"):
        ms.synthesize(enc, np.zeros((2, 2), np.float32), noise=np.zeros((2, 255), np.float32))
    assert ms.synthesize(enc, np.zeros((2, 2), np.float32)).shape == (2, 256, 1)
