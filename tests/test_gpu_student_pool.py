"""GPU tests of student synthesis pools (student.SynthPool, model.SynthesisPool): a stream in a pool has the bits of a
batch-of-one FlowSynthesizer run, in any slot, whenever it joined, whatever the chunk sizes and the other slots did."""
import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev, rel_err
from tests.test_gpu_student_stream import D512, _noise, _synth

pytestmark = pytest.mark.gpu


def _alone(ref, cond, seed, temperature, end, noise=None):
    """The stream by itself: a batch-of-one FlowSynthesizer run in chunks of max_chunk, truncated at `end`."""
    st = ref.start(torch.as_tensor(cond, dtype=torch.float32)[None], [seed], [temperature])
    out, t = [], 0
    while t < st.limit:
        n = min(ref.max_chunk, st.limit - t)
        out.append(ref.step(st, n, None if noise is None else noise[None, t:t + n])[0])
        t += n
    torch.cuda.synchronize()
    return torch.cat(out)[:end]


def _pair(dt, R, dil, F, E, pool, capacity, max_chunk, max_frames):
    """A synthesizer of `capacity` rows and a batch-of-one twin with the same weights."""
    syn, flows = _synth(dt, R, dil, F, E, pool, capacity, max_chunk, max_frames)
    ref, _ = _synth(dt, R, dil, F, E, pool, 1, max_chunk, max_frames)
    return syn, ref, flows


# ---------------------------------------------------------------------------------------------------
# 1. churn
# ---------------------------------------------------------------------------------------------------
SIZES = [160, 1, 31, 200, 77, 13, 160, 200, 31, 1, 160, 77]      # the cycle of chunk sizes (max_chunk = 200)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("R,dil", [(64, D512), (32, D512[:7])], ids=["R64-d512", "R32-d64"])
def test_churn_every_stream_has_its_own_bits(dt, R, dil):
    F, E, pool, cap, C, frames = 2, 5, 128, 4, 200, 16
    syn, ref, _ = _pair(dt, R, dil, F, E, pool, cap, C, frames)
    rng = np.random.default_rng(R + len(dil))
    # (frames, max_samples): ended by their frames or by max_samples, no length a multiple of a chunk size above 1
    specs = [(3, None), (9, 777), (7, None), (16, 1301), (16, None), (5, 555), (11, None), (9, 999), (3, 2000), (13, 1500)]
    streams = []
    for i, (fr, mx) in enumerate(specs):
        end = fr * pool if mx is None else min(fr * pool, mx)
        assert all(end % n for n in set(SIZES) if n > 1)
        cond = rng.standard_normal((fr, E)).astype(np.float32)
        streams.append(dict(cond=cond, seed=1000 + 17 * i, temp=[1.0, 0.7, 0.0, 1.3][i % 4], mx=mx, end=end))
    LEAVER, LEAVE_AFTER = 4, 300          # stream 4 is ended by leave() at the first chunk boundary past 300 samples
    want = [_alone(ref, s["cond"], s["seed"], s["temp"], s["end"]) for s in streams]
    assert not torch.equal(want[0][:300], want[2][:300])

    for graphs in (False, True):
        syn.use_graphs = graphs
        P = syn.pool()
        assert P.capacity == cap and P.free == [0, 1, 2, 3] and P.active == []
        got = [[] for _ in streams]
        where, pending, step, left_at = {}, list(range(len(streams))), 0, None

        def join(ids, slots=None):
            ss = [streams[i] for i in ids]
            us = P.join([s["cond"] for s in ss], [s["seed"] for s in ss], [s["temp"] for s in ss], [s["mx"] for s in ss],
                        slots=slots)
            assert len(us) == len(ids) and (slots is None or us == list(slots))
            for i, u in zip(ids, us):
                where[u] = i
                pending.remove(i)

        join([0, 1, 2])                       # three at once into the lowest slots
        assert P.active == [0, 1, 2]
        while P.active or pending:
            if step == 2:
                join([3], slots=[3])          # by name, two chunks later
            elif step > 2 and pending and P.free:
                free = P.free                 # into slots just freed: the lowest one, or the highest one by name
                if pending[0] % 2:
                    join([pending[0]], slots=[free[-1]])
                else:
                    join([pending[0]])
            n = SIZES[step % len(SIZES)]
            t0 = P.t
            audio, ran = P.step(n)
            assert audio.shape == (cap, n) and ran.shape == (cap,)
            for u in range(cap):
                if ran[u]:
                    got[where[u]].append(audio[u, :ran[u]])
                assert not audio[u, ran[u]:].any()
            assert np.array_equal(P.t, t0 + ran)
            if left_at is None and LEAVER in where.values():
                u = [k for k, v in where.items() if v == LEAVER][-1]
                if u in P.active and P.t[u] > LEAVE_AFTER:
                    left_at = int(P.t[u])
                    P.leave([u])
                    assert u in P.free
            step += 1
            assert step < 400
        torch.cuda.synchronize()
        assert left_at is not None and LEAVE_AFTER < left_at < streams[LEAVER]["end"]
        for i, s in enumerate(streams):
            end = left_at if i == LEAVER else s["end"]
            g = torch.cat(got[i])
            assert g.shape == (end,), (graphs, i, g.shape, end)
            assert torch.equal(g, want[i][:end]), (graphs, i)
        if graphs:
            assert P._graphs, "the repeated chunk sizes were captured and replayed"
        else:
            assert not P._graphs


# ---------------------------------------------------------------------------------------------------
# 2. a reused slot, idle slots
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_reused_slot_keeps_nothing_of_the_previous_stream(dt):
    F, E, pool, C, frames = 2, 4, 64, 160, 24
    syn, ref, _ = _pair(dt, 64, D512, F, E, pool, 2, C, frames)
    rng = np.random.default_rng(8)
    loud = (rng.standard_normal((frames, E)) * 1e4).astype(np.float32)      # conditioning biases of ~1e4 in every layer
    quiet = rng.standard_normal((frames, E)).astype(np.float32)
    P = syn.pool()
    assert P.join([loud], [5], [4.0]) == [0]
    for _ in range(8):                                      # 1280 samples: every history row of the slot is written
        P.step(C)
    top = max(float(b[0].float().abs().max()) for b in syn.bufs[0])
    assert top > 1e3, top
    P.leave([0])
    assert P.join([quiet], [6], [1.0]) == [0]               # the slot just left
    got = []
    while P.active:
        a, ran = P.step(C)
        got.append(a[0, :ran[0]])
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(got), _alone(ref, quiet, 6, 1.0, frames * pool))


def test_idle_slots_cost_no_bits():
    F, E, pool, C, frames = 2, 4, 64, 100, 9
    syn, ref, _ = _pair(torch.bfloat16, 32, D512[:8], F, E, pool, 8, C, frames)
    rng = np.random.default_rng(12)
    cond = rng.standard_normal((frames, E)).astype(np.float32)
    want = _alone(ref, cond, 77, 1.0, frames * pool)
    P = syn.pool()
    assert P.join([cond], [77], slots=[5]) == [5]
    got = []
    while P.active:
        a, ran = P.step(C)
        assert [int(r) for r in ran] == [0] * 5 + [int(ran[5])] + [0] * 2 and ran[5] > 0
        got.append(a[5, :ran[5]])
        assert not a[:5].any() and not a[6:].any() and not a[5, ran[5]:].any()
    assert int(ran[5]) == frames * pool % C              # the last chunk was cut by the stream's end
    assert torch.equal(torch.cat(got), want)
    a, ran = P.step(C)                                   # no live slot: zeros, nothing runs
    assert not ran.any() and not a.any() and a.shape == (8, C)


# ---------------------------------------------------------------------------------------------------
# 3. the fp64 oracle, the noise
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-3), (torch.bfloat16, 6e-2)], ids=["fp32", "bf16"])
def test_pool_streams_match_the_oracle(dt, tol):
    F, E, pool, C, frames, dil = 2, 5, 64, 100, 10, D512[:8]
    syn, flows = _synth(dt, 64, dil, F, E, pool, 3, C, frames)
    rng = np.random.default_rng(4)
    T = frames * pool
    cond = rng.standard_normal((2, frames, E)).astype(np.float32)
    noise = (rng.logistic(0, 1, (2, T)) * 0.3).astype(np.float32)
    P = syn.pool()
    got, t = [[], []], [0, 0]
    slot = {}
    slot[0] = P.join([cond[0]], [0])[0]
    step = 0
    while P.active:
        if step == 3:
            slot[1] = P.join([cond[1]], [0], slots=[2])[0]      # three chunks later, not the neighbouring slot
        nz = torch.zeros(3, C)
        for i, u in slot.items():
            m = min(C, T - t[i])
            nz[u, :m] = torch.from_numpy(noise[i, t[i]:t[i] + m])
        a, ran = P.step(C, noise=nz)
        for i, u in slot.items():
            got[i].append(a[u, :ran[u]])
            t[i] += int(ran[u])
        step += 1
    for i in range(2):
        fw = O.student_forward(flows, noise[i:i + 1].astype(np.float64), cond[i:i + 1].astype(np.float64), pool)
        g = torch.cat(got[i]).cpu().numpy()
        assert g.shape == (T,)
        err = rel_err(g[None], fw["out"])
        print("pool stream %d against the fp64 oracle: rel err %.3e (bound %.0e)" % (i, err, tol))
        assert err < tol


def test_a_late_slot_draws_its_own_noise():
    F, E, pool, C, frames = 1, 4, 64, 90, 8
    syn, _ = _synth(torch.float32, 32, [1, 2, 4, 8], F, E, pool, 3, C, frames)
    rng = np.random.default_rng(2)
    P = syn.pool()
    P.join([rng.standard_normal((frames, E))], [31], [1.0])
    for _ in range(2):
        P.step(C)
    assert P.join([rng.standard_normal((frames, E))], [4242], [0.6], slots=[2]) == [2]
    for n in (C, 37, 1):
        t0 = P.t
        P.step(n)
        torch.cuda.synchronize()
        assert t0[2] != t0[0]
        for u, seed, temp in ((0, 31, 1.0), (2, 4242, 0.6)):
            assert np.array_equal(syn.xbuf[0][u, :n].cpu().numpy(), _noise([seed], [temp], int(t0[u]), n)[0]), (n, u)


# ---------------------------------------------------------------------------------------------------
# 4. the synthesizer's own path, refused calls
# ---------------------------------------------------------------------------------------------------
def test_start_and_step_are_untouched_by_a_pool():
    F, E, pool, C, frames, B = 2, 4, 64, 160, 8, 3
    syn, _ = _synth(torch.bfloat16, 64, D512[:7], F, E, pool, B, C, frames)
    rng = np.random.default_rng(6)
    cond = torch.tensor(rng.standard_normal((B, frames, E)), dtype=torch.float32)

    def run():
        st = syn.start(cond, [3, 9, 27], [1.0, 0.5, 1.0])
        out = [syn.step(st, n) for n in (160, 31, 160, 160, 1)]
        torch.cuda.synchronize()
        return torch.cat(out, 1), st
    before, st = run()
    P = syn.pool()
    with pytest.raises(ValueError, match="current"):
        syn.step(st, 1)                                   # the state ended where the pool began
    P.join([cond[2].numpy() * 30, cond[0].numpy()], [1, 2], slots=[2, 0])
    for n in (160, 77, 160, 160):
        P.step(n)
    after, _ = run()
    assert torch.equal(before, after)
    with pytest.raises(ValueError, match="closed"):       # ... and start() closed the pool
        P.step(1)
    with pytest.raises(ValueError, match="closed"):
        P.join([cond[0]], [1])


def test_refused_calls_leave_the_pool_alone():
    F, E, pool, C, frames = 2, 4, 64, 100, 6
    rng = np.random.default_rng(10)
    conds = [rng.standard_normal((f, E)).astype(np.float32) for f in (6, 4, 5)]

    def run(refusals):
        syn, _ = _synth(torch.float32, 32, [1, 2, 4, 8, 16, 32], F, E, pool, 2, C, frames)
        st = syn.start(torch.zeros(1, 2, E))
        P = syn.pool()
        P.join(conds[:2], [7, 8], [1.0, 0.8])
        out = [P.step(60)[0]]
        if refusals:
            t, act = P.t, P.active
            for bad in (lambda: P.join([conds[2]], [9]),                                     # no free slot
                        lambda: P.join([conds[2]], [9], slots=[1]),                          # ... by name either
                        lambda: P.step(0), lambda: P.step(C + 1), lambda: P.step(-4),
                        lambda: P.step(50, noise=torch.zeros(2, 49)),
                        lambda: syn.step(st, 10)):                                           # the state from before pool()
                with pytest.raises(ValueError):
                    bad()
                assert np.array_equal(P.t, t) and P.active == act
        out.append(P.step(C)[0])
        P.leave([1])
        if refusals:
            t, act = P.t, P.active
            assert act == [0] and P.free == [1]
            for bad in (lambda: P.join([conds[2][:, :3]], [9]),                              # wrong width
                        lambda: P.join([conds[2][None]], [9]),                               # not [frames, E]
                        lambda: P.join([np.zeros((frames + 1, E), np.float32)], [9]),        # frames > max_frames
                        lambda: P.join([conds[2]], [9], max_samples=-1),
                        lambda: P.join([conds[2]], [9], temperature=-0.5),
                        lambda: P.join([conds[2], conds[1]], [9, 10]),                       # two streams, one free slot
                        lambda: P.join([conds[2]], [9], slots=[0]),                          # a live slot
                        lambda: P.join([conds[2]], [9], slots=[2]),                          # outside the pool
                        lambda: P.leave([2])):
                with pytest.raises(ValueError):
                    bad()
                assert np.array_equal(P.t, t) and P.active == act and P.free == [1]
        assert P.join([conds[2]], [9], max_samples=150) == [1]
        while P.active:
            out.append(P.step(C)[0])
        torch.cuda.synchronize()
        return torch.cat(out, 1)
    assert torch.equal(run(True), run(False))


# ---------------------------------------------------------------------------------------------------
# 5. the model surface
# ---------------------------------------------------------------------------------------------------
def test_model_surface_pools(tmp_path):
    M = sub("model")
    dil = [1, 2, 4, 8, 16, 32]
    T, pool, lat, cs = 1024, 64, 8, 4
    teacher = M.WaveNetTeacher(T, cs, dil, dilation_channels=64, skip_channels=256, latent_channels=lat, pool_stride=pool,
                               use_encoding=True, head="mol", num_mixtures=5, dtype=torch.bfloat16)
    student = M.ParallelWaveNet(input_size=T, condition_size=cs, dilations=dil, teacher=teacher, dilation_channels=64,
                                skip_channels=128, num_flows=2, latent_channels=lat, pool_stride=pool, gamma=1e-3,
                                dtype=torch.bfloat16)
    rng = np.random.default_rng(0)
    x = O.synthetic_audio(2, T, seed=3)
    enc = rng.standard_normal((2, T // pool, lat)).astype(np.float32)
    y = np.eye(cs, dtype=np.float32)[[0, 2]]
    noise = (rng.logistic(0, 1, (2, T)) * 0.5).astype(np.float32)
    for _ in range(2):
        student.train_fast(None, noise, x, enc, y)
    sdir = str(tmp_path / "student")
    assert student.save(None, sdir, 3, force=True)
    dep = M.StudentSynthesizer.from_checkpoint(sdir, dil, 2, dilation_channels=64, latent_channels=lat, condition_size=cs,
                                               pool_stride=pool, dtype=torch.bfloat16, max_batch=3, max_chunk=300,
                                               max_frames=T // pool)
    reqs = [(enc[0], y[0], 40, 1.0), (enc[1, :9], y[1], 41, 0.8)]          # two requests: 1024 and 576 samples
    for syn in (student.synthesizer(max_batch=3, max_chunk=300, max_frames=T // pool), dep):
        want = [syn.synthesize(e[None], c[None], seed=s, temperature=tp)[0, :, 0] for e, c, s, tp in reqs]
        P = syn.pool()
        assert P.capacity == 3 and P.free == [0, 1, 2]
        got = {0: [], 1: []}
        u0 = P.join([reqs[0][0]], [reqs[0][1]], seed=[40], temperature=[1.0])[0]
        who = {u0: 0}
        for i, n in enumerate([160, 300, 7, 160, 160, 300, 300]):
            if i == 2:
                who[P.join(reqs[1][0], reqs[1][1], seed=41, temperature=0.8)[0]] = 1
            for u, a in P.step(n).items():
                got[who[u]].append(a)
        assert P.active == []
        for i in range(2):
            g = np.concatenate(got[i])
            assert g.shape == want[i].shape and np.array_equal(g.view(np.uint32), want[i].view(np.uint32)), i
        with pytest.raises(ValueError, match="conditions"):
            P.join([enc[0]])
        assert np.array_equal(syn.synthesize(enc[:1], y[:1], seed=40)[0, :, 0], want[0])      # and the pool is closed
        with pytest.raises(ValueError, match="closed"):
            P.step(1)
