"""GPU tests of generation pools: streams that join a running pool at different steps, from prompts of any lengths, in
reused slots, equal their solo batch-of-one runs bit for bit (both bodies, both column blockings, both dtypes, the
conditioned mixture-of-logistics decoder); a forced pool equals batched forced generation; idle rows stay zero and a
stream ends at its own max_samples; the slot ring fill against a NumPy restatement of its mapping; the model classes'
pool API."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_generate_stream import _bits, _mol_engine, _softmax_engine
from tests.test_gpu_kernels import DEV, dev

pytestmark = pytest.mark.gpu

BODIES = [(torch.bfloat16, "1", "1"), (torch.bfloat16, "1", "2"), (torch.bfloat16, "0", None), (torch.float32, "1", None)]
BODY_IDS = ["bf16-latency-ncb1", "bf16-latency-ncb2", "bf16-throughput", "fp32"]


def _body(monkeypatch, gen16, ncb):
    monkeypatch.setenv("SRWN_GEN16", gen16)
    if ncb is None:
        monkeypatch.delenv("SRWN_GEN16_NCB", raising=False)
    else:
        monkeypatch.setenv("SRWN_GEN16_NCB", ncb)


def _solo(eng, seed, prompt, n, cond=None):
    """A batch-of-one run: generation_state + prime + generate_chunk (audio, codes, logits as [n] / [n, C])."""
    st = eng.generation_state(1, None if cond is None else dev(cond[None]), seed)
    if len(prompt):
        eng.prime(st, dev(prompt[None]))
    a, c, lg = eng.generate_chunk(st, n, mode="sample", want_logits=True)
    return a[0], c[0], lg[0]


class _Run:
    """Drives a pool and collects what each stream (by name) produced."""

    def __init__(self, pool):
        self.pool, self.out, self.slot, self.done = pool, {}, {}, set()

    def join(self, names, seeds, prompts, **kw):
        slots = self.pool.join(seeds, prompts, **kw)
        for nm, u in zip(names, slots):
            self.slot[nm], self.out[nm] = u, []
        return slots

    def step(self, n):
        a, c, lg, ran = self.pool.step(n, want_logits=True)
        for nm, u in self.slot.items():
            if nm in self.done:
                continue
            if ran[u]:
                self.out[nm].append((a[u, :ran[u]], c[u, :ran[u]], lg[u, :ran[u]]))
            if u not in self.pool.active:
                self.done.add(nm)
        return a, c, lg, ran

    def leave(self, nm):
        self.pool.leave([self.slot[nm]])
        self.done.add(nm)

    def got(self, nm):
        return [torch.cat([o[i] for o in self.out[nm]]) for i in range(3)]


def test_prime_forward_rows_do_not_depend_on_the_pass_shape():
    """What the pool's batched prompt pass relies on: a stream's stored layer inputs x_l[t] are the same bits whether
    its prompt is primed alone at (1, P) or as one row of a larger pass, padded in time."""
    for dt in (torch.bfloat16, torch.float32):
        eng, _ = _softmax_engine(dt)
        P = 513
        audio = O.synthetic_audio(1, P, seed=3)
        a = eng._prime_view(1, P)
        a.set_inputs(dev(audio))
        a.forward(want_logits=False, with_loss=False, train=False, stack_only=True)
        solo = _bits(a.xs[:, 0].float() if dt == torch.bfloat16 else a.xs[:, 0])
        b = sub("engine").WaveNetEngine(eng.cfg, 8, 1024, DEV, share_from=eng, frozen=True)
        x = np.zeros((8, 1024), np.float32)
        x[5, :P] = audio[0]
        x[2, :300] = audio[0, :300] * 0.5
        b.set_inputs(dev(x))
        b.forward(want_logits=False, with_loss=False, train=False, stack_only=True)
        big = _bits(b.xs[:, 5, :P].float() if dt == torch.bfloat16 else b.xs[:, 5, :P])
        assert np.array_equal(solo, big), dt


@pytest.mark.parametrize("dt,gen16,ncb", BODIES, ids=BODY_IDS)
def test_staggered_streams_equal_solo_runs(monkeypatch, dt, gen16, ncb):
    _body(monkeypatch, gen16, ncb)
    eng, _ = _softmax_engine(dt)
    pool = eng.generation_pool(40)                       # two ring groups, the second partial
    rng = np.random.default_rng(11)
    pr = lambda n: O.synthetic_audio(1, n, seed=int(rng.integers(1 << 30)))[0] if n else np.zeros(0, np.float32)
    run = _Run(pool)
    streams = {}                                         # name -> (seed, prompt)

    def join(names, lens):
        seeds = [1000 + 7 * len(streams) + i for i in range(len(names))]
        ps = [pr(n) for n in lens]
        for nm, s, p in zip(names, seeds, ps):
            streams[nm] = (s, p)
        return run.join(names, seeds, ps)

    join(["a", "b", "c"], [0, 1, 700])                   # clock 0
    run.step(1)
    join(["d", "e"], [2, 0])                             # clock 1
    run.step(6)
    join(["f", "g"], [511, 513])                         # clock 7
    for n in (16, 160, 160, 160, 8):
        run.step(n)
    run.leave("b")                                       # clock 511: b's and e's slots are reused
    run.leave("e")
    reuse = [run.slot["b"], run.slot["e"]]
    ph, pi = pr(513), pr(0)
    assert run.join(["h", "i"], [2001, 2002], [ph, pi], slots=reuse) == reuse
    streams["h"], streams["i"] = (2001, ph), (2002, pi)
    run.step(2)
    join(["j", "k"], [1, 700])                           # clock 513
    run.step(87)
    join(["l", "m", "n"], [2, 513, 0])                   # clock 600
    for n in (513, 160, 1):
        run.step(n)
    assert pool.clock == 1274
    assert len(run.out) >= 12
    for nm in sorted(run.out):
        seed, p = streams[nm]
        a, c, lg = run.got(nm)
        ra, rc, rl = _solo(eng, seed, p, a.shape[0])
        for got, want, what in ((a, ra, "audio"), (c, rc, "codes"), (lg, rl, "logits")):
            assert np.array_equal(_bits(got), _bits(want)), (nm, what, a.shape[0], len(p))


@pytest.mark.parametrize("dt,gen16,ncb", BODIES, ids=BODY_IDS)
def test_reused_slots_equal_solo_runs(monkeypatch, dt, gen16, ncb):
    """A slot freed by a leave and joined again from a prompt, at a clock that is no multiple of anything."""
    _body(monkeypatch, gen16, ncb)
    eng, _ = _softmax_engine(dt)
    pool = eng.generation_pool(40)
    run = _Run(pool)
    ps = {nm: O.synthetic_audio(1, n, seed=k)[0] for k, (nm, n) in enumerate([("x", 300), ("y", 513), ("z", 2)])}
    run.join(["x", "y"], [5, 6], [ps["x"], ps["y"]], slots=[17, 33])
    run.step(160)
    run.leave("x")
    run.join(["z"], [7], [ps["z"]], slots=[17])
    run.step(513)
    run.step(16)
    for nm, s in (("y", 6), ("z", 7)):
        a, c, lg = run.got(nm)
        ra, rc, rl = _solo(eng, s, ps[nm], a.shape[0])
        for got, want in ((a, ra), (c, rc), (lg, rl)):
            assert np.array_equal(_bits(got), _bits(want)), nm


@pytest.mark.parametrize("dt,gen16,ncb", BODIES, ids=BODY_IDS)
def test_forced_pool_equals_batched_forced_generation(monkeypatch, dt, gen16, ncb):
    _body(monkeypatch, gen16, ncb)
    eng, _ = _softmax_engine(dt)
    B, T = 40, 600
    f = dev(O.synthetic_audio(B, T, seed=21))
    _, _, want = eng.generate(T, mode="sample", seed=3, forced=f, want_logits=True, batch=B)
    pool = eng.generation_pool(B)
    pool.join(list(range(100, 100 + B)))
    got = []
    for a, b in ((0, 1), (1, 513), (513, T)):
        _, _, lg, ran = pool.step(b - a, forced=f[:, a:b], want_logits=True)
        assert (ran == b - a).all()
        got.append(lg)
    assert np.array_equal(_bits(torch.cat(got, 1)), _bits(want))


@pytest.mark.parametrize("dt,gen16,ncb", BODIES, ids=BODY_IDS)
def test_idle_and_finishing_slots(monkeypatch, dt, gen16, ncb):
    _body(monkeypatch, gen16, ncb)
    eng, _ = _softmax_engine(dt, dil=[1, 2, 4, 8, 16, 32])
    k = 37
    pool = eng.generation_pool(40)
    assert pool.join([1, 2, 3], [None, O.synthetic_audio(1, 9, seed=1)[0], None], max_samples=[None, k, None],
                     slots=[0, 21, 33]) == [0, 21, 33]
    outs = []
    for n in (100, 100):
        a, c, lg, ran = pool.step(n, want_logits=True)
        outs.append((a, c, lg))
        idle = [u for u in range(40) if u not in (0, 21, 33)]
        for x in (a, c, lg):
            assert not x[idle].any()                    # idle rows stay as the caller zeroed them
        assert ran[idle].sum() == 0 and ran[0] == n and ran[33] == n
        if len(outs) == 1:
            assert ran[21] == k and not a[21, k:].any() and not c[21, k:].any() and not lg[21, k:].any()
            assert 21 not in pool.active and 21 in pool.free and pool.t[21] == 9 + k
        else:
            assert ran[21] == 0 and not a[21].any()
    # the other streams are what they are without that stream
    ref = eng.generation_pool(40)
    ref.join([1, 3], slots=[0, 33])
    for i, n in enumerate((100, 100)):
        a, c, lg, _ = ref.step(n, want_logits=True)
        for got, want in zip(outs[i], (a, c, lg)):
            assert np.array_equal(_bits(got[[0, 33]]), _bits(want[[0, 33]]))
    assert ref.active == [0, 33]


@pytest.mark.parametrize("dt,gen16", [(torch.float32, "1"), (torch.bfloat16, "0"), (torch.bfloat16, "1")])
def test_conditioned_mol_streams_equal_solo_runs(monkeypatch, dt, gen16):
    _body(monkeypatch, gen16, None)
    eng, _ = _mol_engine(dt)                             # E = 6, pool_stride 16, M = 10
    rng = np.random.default_rng(5)
    pool = eng.generation_pool(8, frames=20)
    run = _Run(pool)
    enc = {}

    def join(names, frames, lens):
        seeds = [50 + len(enc) + i for i in range(len(names))]
        cs = [rng.standard_normal((f, 6)) for f in frames]
        ps = [O.synthetic_audio(1, n, seed=len(enc) + i)[0] if n else np.zeros(0, np.float32) for i, n in enumerate(lens)]
        for nm, s, c, p in zip(names, seeds, cs, ps):
            enc[nm] = (s, c, p)
        run.join(names, seeds, ps, cond=[dev(c) for c in cs])

    join(["a", "b", "c"], [3, 20, 7], [0, 37, 0])        # clock 0
    run.step(40)
    join(["d", "e"], [11, 4], [100, 0])                  # clock 40 (a ends at 48)
    run.step(90)
    join(["f"], [20], [0])                               # clock 130 (in a freed slot)
    for n in (160, 160, 160):
        run.step(n)
    assert not pool.active
    for nm, (s, c, p) in enc.items():
        a, cd, lg = run.got(nm)
        assert a.shape[0] == c.shape[0] * 16 - len(p), nm      # each ends at its own frames * pool_stride
        if len(p):
            ra, rc, rl = _solo(eng, s, p, a.shape[0], cond=c)
        else:
            ra, rc, rl = eng.generate(a.shape[0], mode="sample", seed=s, want_logits=True, batch=1, cond=dev(c[None]))
            ra, rc, rl = ra[0], rc[0], rl[0]
        for got, want, what in ((a, ra, "audio"), (cd, rc, "mixture"), (lg, rl, "logits")):
            assert np.array_equal(_bits(got), _bits(want)), (nm, what)


def _ring_slots_reference(ring, xs, dst, P, clock, dil, R):
    """NumPy restatement of srwn_generate_ring_fill_slots: local step tau of row i at ring position (clock - P + tau) mod
    (d+1) of slot dst[i], zero for tau < 0.  ring: [groups][layers][d+1][32][R] flattened, as srwn_generate_ring_elems."""
    out = ring.copy()
    per_group = sum((d + 1) * 32 * R for d in dil)
    for i, (u, p) in enumerate(zip(dst, P)):
        g, row = u // 32, u % 32
        off = g * per_group
        for l, d in enumerate(dil):
            r = out[off:off + (d + 1) * 32 * R].reshape(d + 1, 32, R)
            for tau in range(p - 1 - d, p):
                r[(clock - p + tau) % (d + 1), row] = xs[l, i, tau] if tau >= 0 else 0
            off += (d + 1) * 32 * R
    return out


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("clock", [0, 37, 1000])
def test_ring_fill_slots_matches_numpy(dt, clock):
    L_ = sub("_lib")
    K = sub("kernels")
    dil, R, Tsrc, B = [1, 2, 64, 7, 256], 64, 320, 70
    dst = [3, 20, 40, 69, 31, 16]                         # both halves of a ring group, and three groups
    P = [300, 5, 0, 100, 1, 256]                          # P < d, P = 0 clears, clock - P < 0 at clock 0 / 37
    rng = np.random.default_rng(clock)
    xs = torch.tensor(rng.standard_normal((len(dil), len(dst), Tsrc, R)).astype(np.float32)).to(device=DEV, dtype=dt)
    dl = (C.c_int32 * len(dil))(*dil)
    relems = int(L_.load().srwn_generate_ring_elems(dl, len(dil), R)) * ((B + 31) // 32)
    ring = torch.tensor(rng.standard_normal(relems).astype(np.float32)).to(device=DEV, dtype=dt)   # rows not named stay
    ring0 = ring.clone()
    dst_d, P_d = dev(dst, torch.int32), dev(P, torch.int32)      # (held: a freed temporary's block would be reused)
    L_.call("srwn_generate_ring_fill_slots", xs.data_ptr(), len(dst) * Tsrc * R, Tsrc, len(dst), dst_d.data_ptr(),
            P_d.data_ptr(), clock, dl, len(dil), B, R, ring.data_ptr(), K.abi_dtype(dt),
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    iv = torch.int32 if dt == torch.float32 else torch.int16
    want = _ring_slots_reference(ring0.cpu().view(iv).numpy(), xs.cpu().view(iv).numpy(), dst, P, clock, dil, R)
    assert np.array_equal(ring.cpu().view(iv).numpy(), want)


def test_model_pools_equal_generate():
    M = sub("model")
    m = M.WaveNetTeacher(256, 0, [1, 2, 4, 8, 16, 32, 64], dilation_channels=64, skip_channels=256,
                         quantization_channels=256, dtype=torch.bfloat16)
    pool = m.generation_pool(3)
    p = O.synthetic_audio(2, 100, seed=4)
    got = {0: [], 1: [], 2: []}
    slots = pool.join(seed=[7, 8], prompt=[p[0], None])
    assert slots == [0, 1] and pool.free == [2]
    for u, x in pool.step(50).items():
        got[u].append(x)
    assert pool.join(seed=[9], prompt=[p[1][:33]], max_samples=[70]) == [2]
    for n in (16, 64):
        for u, x in pool.step(n).items():
            got[u].append(x)
    assert pool.free == [2]                                # the max_samples stream ended inside the 64-step launch
    pool.leave([1])
    out = pool.step(10)
    assert sorted(out) == [0] and pool.active == [0]
    for u, x in out.items():
        got[u].append(x)
    cat = {u: np.concatenate(v) for u, v in got.items()}
    assert cat[0].shape == (140,) and cat[1].shape == (130,) and cat[2].shape == (70,)
    for u, (s, pr) in enumerate([(7, p[0]), (8, None), (9, p[1][:33])]):
        want = m.generate(1, cat[u].shape[0], seed=s, prompt=None if pr is None else pr[None])[0]
        assert np.array_equal(cat[u].view(np.uint32), want.view(np.uint32)), u


def test_autoencoder_pool_streams_in_a_reused_slot():
    M = sub("model")
    ae = M.WaveNetAutoEncoder(input_size=256, condition_size=0, num_mixtures=5, dilations=[1, 2, 4, 8, 16],
                              dilation_channels=64, skip_channels=256, latent_channels=8, pool_stride=32,
                              dtype=torch.float32)
    rng = np.random.default_rng(1)
    encs = [rng.standard_normal((f, 8)).astype(np.float32) for f in (4, 2, 3)]
    ap = ae.generation_pool(2, 4)
    assert ap.join(seed=[5, 6], encoding=encs[:2]) == [0, 1]
    got = {"a": [], "b": [], "c": []}
    out = ap.step(64)
    got["a"].append(out[0]); got["b"].append(out[1])
    assert ap.free == [1]                                  # the 2-frame stream ended at its 64 samples
    assert ap.join(seed=[7], encoding=[encs[2]]) == [1]
    for n in (50, 50):
        out = ap.step(n)
        got["a"].append(out[0]); got["c"].append(out[1])
    assert not ap.active
    for nm, s, e in (("a", 5, encs[0]), ("b", 6, encs[1]), ("c", 7, encs[2])):
        g = np.concatenate(got[nm])
        want = ae.generate(e[None], seed=s)[0]
        assert g.shape == want.shape == (e.shape[0] * 32,)
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), nm
    w = M.WaveNetTeacher(256, 0, [1, 2], dilation_channels=64, skip_channels=256, gate_mode="wavenet")
    with pytest.raises(NotImplementedError, match="wavenet"):
        w.generation_pool(4)
