"""GPU tests of mixture-of-logistics scorer pools (srwn_version() 119; scorer.MolScorerPool, model.MolScorerStreamPool,
model.AutoEncoderScorerPool).  Every comparison in this file is bit for bit; the one bound, on the running means, is fp64
round-off.

  entry       srwn_mol_score_stream_in_slots against srwn_flow_stream_in_slots on the same chunk, carry and table: t = 0 and
              1 (the zero taps), special samples, frames across the conditioning ring's wrap, ran = 0, a ragged ran
  groups      srwn_residual_group_fwd_stream_z_slots WITH cond_next against the clock form at batch one
  head        srwn_stream_mol_score_head_slots / srwn_mol_score_rows_slots against one clock-form call per slot
  session     five conditioned streams in four slots -- joining, pushed, fed, starved of frames, leaving -- against
              MolStreamScorer(max_batch=1).score of each alone: both dtypes, the fused head and its twin, E = 0 too
  invariance  graph replay, max_chunk and a second session on the same object change no bit
  model       AutoEncoderScorerPool, StreamingMolScorer.pool, from_checkpoint(...).pool; buffer_bytes
"""
import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DEV = "cuda"
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 1, 2, 5]      # several layer groups of both kinds, the longest history > a chunk
POOL, MAX_CHUNK, CAP, RING = 20, 128, 4, 150      # an audio ring of 150: a chunk of 128 wraps it
SHAPES = [(64, 256, 10), (32, 128, 4)]            # R, S, M (Cp = 64 and 32)
LENGTHS = {6: [300, 20, 140, 520, 60], 0: [300, 1, 131, 517, 64]}      # per cond_channels E
LEAVES_AT = 70                                     # stream 2 leaves once it has scored this much
SPECIAL = [-1.0, 1.0, 0.0, -0.0, 1e-30]
_PARAMS, _ALONE = {}, {}


def _bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(t))
    return t.contiguous().view(torch.uint8)


def _hist_max():
    from types import SimpleNamespace
    return max(sum(DIL[a:b]) for a, b in sub("scorer").MolStreamScorer._plan(SimpleNamespace(dil=DIL)))


def _max_frames():
    """One frame more than the smallest ring a live stream can run on: the ring wraps."""
    return sub("student").live_min_frames(_hist_max(), POOL) + 1


def _params(R, S, M, E):
    if (R, S, M, E) not in _PARAMS:
        _PARAMS[R, S, M, E] = O.init_stack_params(11, DIL, 2, R, S, 4 * M, cond_channels=E, bias_scale=0.05)
    return _PARAMS[R, S, M, E]


def _scorer(R, S, M, E, dt, monkeypatch, fused=True, max_batch=CAP, max_chunk=MAX_CHUNK, graphs=True, max_frames=None):
    Sc = sub("scorer")
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1" if fused else "0")
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "1" if graphs else "0")
    w = Sc.MolScorerWeights(DIL, R, S, M, E, POOL, 2, dt)
    w.load_oracle_params(_params(R, S, M, E))
    s = Sc.MolStreamScorer(w, max_batch=max_batch, max_chunk=max_chunk, max_frames=max_frames or _max_frames())
    assert s.fused == fused and s.use_graphs == graphs
    return s


def _streams(E):
    """The five streams of a session: (audio [T] fp32, frames [T / POOL, E] fp32 or None) each, made once per call from
    fixed seeds; the special sample values lie at the start of stream 0 and across the first ring wrap of stream 3."""
    rng = np.random.default_rng(11)
    out = []
    for i, n in enumerate(LENGTHS[E]):
        a = O.synthetic_audio(1, n, seed=30 + i)[0].astype(np.float32).copy()
        if i == 0:
            a[:len(SPECIAL)] = SPECIAL
        if i == 3:
            a[148:148 + len(SPECIAL)] = SPECIAL
        out.append((a, rng.normal(size=(n // POOL, E)).astype(np.float32) if E else None))
    return out


def _alone(R, S, M, E, dt, monkeypatch):
    """Per stream (nll [T], logits [T, 4M]) of MolStreamScorer(max_batch=1).score of it alone: once per case, shared."""
    key = (R, S, M, E, dt)
    if key not in _ALONE:
        one = _scorer(R, S, M, E, dt, monkeypatch, max_batch=1)
        _ALONE[key] = [tuple(o[0].clone() for o in one.score(torch.tensor(a[None]), None if f is None else torch.tensor(f[None]),
                                                             return_logits=True)) for a, f in _streams(E)]
    return _ALONE[key]


# ---- the entry ---------------------------------------------------------------------------------------------------------
T0 = [0, 1, 77, 3 * RING + 5]      # t = 0 and 1: the zero taps; the last slot's chunk wraps the audio ring
RAN = [128, 128, 0, 45]
N = MAX_CHUNK


def _table(t0=T0, ran=RAN):
    return torch.tensor([[a, a + r] for a, r in zip(t0, ran)], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("R,conditioned", [(64, True), (32, True), (32, False)])
def test_entry_against_flow_stream_in_slots(R, conditioned, dt):
    K = sub("kernels"); L_ = sub("_lib")
    rng = np.random.default_rng(R + conditioned)
    hist, mc, sentinel = 11, MAX_CHUNK, 7.0
    frames, LR = (5, 3 * R) if conditioned else (1, R)      # 5 frames of 20 samples: every chunk crosses the ring's wrap
    init_w = torch.tensor(rng.normal(0, 0.5, (2, R)), dtype=F32, device=DEV)
    init_b = torch.tensor(rng.normal(0, 0.1, R), dtype=F32, device=DEV)
    cond = torch.tensor(rng.normal(0, 1, (CAP * frames, LR)) * conditioned, dtype=F32, device=DEV).to(dt)
    audio = []                  # per slot, its stream from time 0 to the end of the chunk
    for u in range(CAP):
        a = rng.uniform(-1.2, 1.2, T0[u] + max(RAN[u], 1)).astype(np.float32)
        at = T0[u] + (3 if RAN[u] > 20 else 0)
        a[at:at + len(SPECIAL)] = SPECIAL[:max(0, len(a) - at)]
        audio.append(a)
    ring = np.full((CAP, RING), np.nan, np.float32)      # what the kernel must not read is NaN
    for u in range(CAP):
        for s in range(max(T0[u] - 2, 0), T0[u] + RAN[u]):
            ring[u, s % RING] = audio[u][s]
    ring = torch.tensor(ring, device=DEV)
    x = torch.zeros((CAP, mc), dtype=F32, device=DEV)      # the clock-free reference: the chunk staged, its carry beside it
    carry = torch.zeros((CAP, 2), dtype=F32, device=DEV)
    for u in range(CAP):
        a = np.concatenate([np.zeros(2, np.float32), audio[u]])      # a[s + 2] = sample s, zeros before time 0
        x[u, :RAN[u]] = torch.tensor(a[T0[u] + 2:T0[u] + 2 + RAN[u]])
        carry[u] = torch.tensor([a[T0[u] + 1], a[T0[u]]])            # the samples t - 1 and t - 2
    out = torch.full((CAP, hist + mc, R), sentinel, dtype=dt, device=DEV)
    want = out.clone()
    x_out = torch.full((CAP, mc), -77.0, dtype=F32, device=DEV)
    cargs = (cond.data_ptr(), frames, POOL, LR)
    tail = (CAP, N, mc, R, K.abi_dtype(dt), _table().data_ptr(), K._stream())
    L_.call("srwn_mol_score_stream_in_slots", ring.data_ptr(), RING, init_w.data_ptr(), init_b.data_ptr(), *cargs,
            out.data_ptr(), hist + mc, hist, x_out.data_ptr(), mc, *tail)
    L_.call("srwn_flow_stream_in_slots", x.data_ptr(), mc, carry.data_ptr(), init_w.data_ptr(), init_b.data_ptr(), *cargs,
            want.data_ptr(), hist + mc, hist, *tail)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    for u in range(CAP):
        ran = RAN[u]
        assert torch.all(out[u, :hist] == sentinel) and torch.all(out[u, hist + ran:] == sentinel), u
        assert torch.all(x_out[u, ran:] == -77.0), u
        if ran:
            rows = out[u, hist:hist + ran].float()
            assert not torch.isnan(rows).any() and not torch.all(rows == sentinel), u
            assert torch.equal(_bits(x_out[u, :ran]), _bits(torch.tensor(audio[u][T0[u]:T0[u] + ran], device=DEV))), u
    assert torch.equal(_bits(x_out[0, 3:3 + len(SPECIAL)]), _bits(torch.tensor(SPECIAL, dtype=F32, device=DEV)))      # -0.0, 1e-30 kept


# ---- the group launches with conditioning ------------------------------------------------------------------------------
GT0 = [3, 600, 50, 1290]           # before the first history is full; frames across the ring's wrap (32 frames of 20)
GRAN = [128, 45, 0, 77]


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("R,S,M", SHAPES)
def test_group_launches_with_conditioning_in_slot_form(R, S, M, dt, monkeypatch):
    E, F = 6, 32
    s4 = _scorer(R, S, M, E, dt, monkeypatch, max_frames=F)
    s1 = _scorer(R, S, M, E, dt, monkeypatch, max_batch=1, max_frames=F)
    assert len(s4.groups) >= 2 and F * POOL > _hist_max() + MAX_CHUNK
    g = torch.Generator(device="cpu").manual_seed(R + M)
    s4.ring.copy_(torch.randn(s4.ring.shape, generator=g).to(dt))
    fill = [torch.randn(b.shape, generator=g).to(dt) for b in s4.bufs]
    for b, f in zip(s4.bufs, fill):
        b.copy_(f)
    s4.stack.top.fill_(9.0)
    s4.stack.zs.fill_(9.0)
    above = lambda s: [s.ring.data_ptr() + (l + 1) * R * s.ring.element_size() if l + 1 < s.w.L else None for l in range(s.w.L)]
    table = _table(GT0, GRAN)
    s4.stack.launch_groups(CAP, N, table.data_ptr(), True, cond=(above(s4), F, POOL, s4.LR))
    torch.cuda.synchronize()
    for u in range(CAP):
        ran = GRAN[u]
        if ran == 0:
            assert torch.all(s4.stack.top[u] == 9.0) and torch.all(s4.stack.zs[:, u] == 9.0)
            for b, f in zip(s4.bufs, fill):
                assert torch.equal(_bits(b[u]), _bits(f[u].to(DEV)))
            continue
        s1.ring.copy_(s4.ring[u * F:(u + 1) * F])
        for b, f in zip(s1.bufs, fill):
            b.copy_(f[u:u + 1])
        s1.clock.fill_(GT0[u])
        s1.stack.launch_groups(1, ran, s1.clock.data_ptr(), False, cond=(above(s1), F, POOL, s1.LR))
        torch.cuda.synchronize()
        assert torch.equal(_bits(s4.stack.top[u, :ran]), _bits(s1.stack.top[0, :ran])), u
        assert torch.equal(_bits(s4.stack.zs[:, u, :ran]), _bits(s1.stack.zs[:, 0, :ran])), u
        assert torch.all(s4.stack.zs[:, u, ran:] == 9.0), u
        for gi, (b4, b1) in enumerate(zip(s4.bufs[1:], s1.bufs[1:])):
            h = s4.hist[gi + 1]
            assert torch.equal(_bits(b4[u, h:h + ran]), _bits(b1[0, h:h + ran])), (u, gi)


# ---- the head and its twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("R,S,M", SHAPES)
def test_head_and_twin_slot_forms_against_the_clock_forms(R, S, M, dt, monkeypatch):
    K = sub("kernels"); L_ = sub("_lib")
    s = _scorer(R, S, M, 0, dt, monkeypatch, fused=False)      # (the twin's buffers; the fused head is called by hand)
    g = torch.Generator(device="cpu").manual_seed(S + M)
    s.stack.zs.copy_(torch.randn(s.stack.zs.shape, generator=g).to(dt))
    s.xbuf.copy_(torch.rand(s.xbuf.shape, generator=g) * 2.4 - 1.2)
    s.xbuf[:, 5:5 + len(SPECIAL)] = torch.tensor(SPECIAL, device=DEV)
    s.logits32.copy_(torch.randn(s.logits32.shape, generator=g))
    ran, C, C4 = [128, 45, 0, 33], MAX_CHUNK, 4 * M             # 45, 33: masked last tiles
    table = _table([0] * CAP, ran)
    abi, st = K.abi_dtype(dt), K._stream()

    def outs():
        return torch.full((CAP, C), -5.0, dtype=F32, device=DEV), torch.full((CAP, C, C4), -5.0, dtype=F32, device=DEV)

    def head(sfx, n, nll, lo, *tab):
        L_.call("srwn_stream_mol_score_head" + sfx, *s._head_args(), s.xbuf.data_ptr(), C, nll.data_ptr(), lo.data_ptr(), C, CAP,
                n, C, R, S, M, abi, *tab, st)

    def twin(sfx, n, nll, lo, *tab):
        L_.call("srwn_mol_score_rows" + sfx, s.logits32.data_ptr(), s.w.Cp, C, s.xbuf.data_ptr(), C, nll.data_ptr(),
                lo.data_ptr(), C, CAP, n, M, *tab, st)

    for form in (head, twin):
        nll, lo = outs()
        form("_slots", N, nll, lo, table.data_ptr())
        torch.cuda.synchronize()
        for u in range(CAP):
            assert torch.all(nll[u, ran[u]:] == -5.0) and torch.all(lo[u, ran[u]:] == -5.0), (form.__name__, u)
            if ran[u] == 0:
                continue
            wn, wl = outs()
            form("", ran[u], wn, wl)
            torch.cuda.synchronize()
            assert torch.isfinite(wn[u, :ran[u]]).all()
            assert torch.equal(_bits(nll[u, :ran[u]]), _bits(wn[u, :ran[u]])), (form.__name__, u)
            assert torch.equal(_bits(lo[u, :ran[u]]), _bits(wl[u, :ran[u]])), (form.__name__, u)


# ---- a session: five streams, four slots -------------------------------------------------------------------------------
def _session(s, E, audio_ring=RING, rounds=400):
    """The fixed ragged script on ``s.pool()``: streams join when a slot is free (every other round), push up to 90
    samples and are fed up to 3 frames per round, every third round feeds nobody (the streams are starved of frames for
    whole steps), stream 2 leaves once it has scored LEAVES_AT samples, the others when they are through; slots are
    reused.  Returns per stream (nll, logits) put together, and the slots they held."""
    streams = _streams(E)
    pool = s.pool(audio_ring)
    rng = np.random.default_rng(3)
    waiting, slot_of, sent, fed = list(range(len(streams))), {}, {}, {}
    got = {i: ([], []) for i in range(len(streams))}
    held = {}
    for rnd in range(rounds):
        if not waiting and not slot_of:
            break
        if waiting and pool.free and rnd % 2 == 0:
            i = waiting.pop(0)
            slot_of[i], = pool.join(1)
            sent[i] = fed[i] = 0
            held[i] = slot_of[i]
            assert pool.fed[slot_of[i]] == 0 and pool.scored[slot_of[i]] == 0
        us, xs, fu, fs = [], [], [], []
        for i, u in slot_of.items():
            a, f = streams[i]
            k = int(min(rng.integers(0, 91), pool.audio_room(u), len(a) - sent[i]))
            us.append(u); xs.append(a[sent[i]:sent[i] + k]); sent[i] += k
            if E and rnd % 3 != 2:
                k = int(min(rng.integers(0, 4), pool.room(u), len(f) - fed[i]))
                fu.append(u); fs.append(torch.tensor(f[fed[i]:fed[i] + k])); fed[i] += k
        pool.push(us, xs)
        if fu:
            pool.feed(fu, fs)
        want = {u: pool.available(u) for u in slot_of.values()}
        nll, logits = pool.step(return_logits=True)
        assert set(nll) == set(logits) == {u for u, m in want.items() if m > 0}
        for i, u in list(slot_of.items()):
            if u in nll:
                assert nll[u].shape == (want[u],) and logits[u].shape[0] == want[u]
                got[i][0].append(nll[u]); got[i][1].append(logits[u])
            done = pool.scored[u] == len(streams[i][0]) or (i == 2 and pool.scored[u] >= LEAVES_AT)
            if done:
                pool.leave(u)
                del slot_of[i]
    assert not waiting and not slot_of, "the session did not drain"
    cat = lambda p, tail: torch.cat(p, 0) if p else torch.zeros((0,) + tail, device=DEV)
    return [(cat(got[i][0], ()), cat(got[i][1], (4 * s.w.M,))) for i in range(len(streams))], held, pool


def _check_session(res, alone, E):
    for i, ((nll, logits), (wn, wl)) in enumerate(zip(res, alone)):
        m = nll.shape[0]
        assert m == (LENGTHS[E][i] if i != 2 else m) and (i != 2 or LEAVES_AT <= m <= LENGTHS[E][2]), (i, m)
        assert torch.isfinite(nll).all()
        assert torch.equal(_bits(nll), _bits(wn[:m])), i
        assert torch.equal(_bits(logits), _bits(wl[:m])), i


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twin"])
@pytest.mark.parametrize("E", [6, 0])
@pytest.mark.parametrize("R,S,M", SHAPES)
def test_pool_equals_score_alone(R, S, M, E, fused, dt, monkeypatch):
    alone = _alone(R, S, M, E, dt, monkeypatch)
    s = _scorer(R, S, M, E, dt, monkeypatch, fused=fused)
    res, held, pool = _session(s, E)
    _check_session(res, alone, E)
    assert len(set(held.values())) < len(held)                      # a slot was reused
    assert pool.launches_per_step == s.launches_per_step
    with pytest.raises(ValueError, match="closed"):                  # start() ends the pool
        s.start(1)
        pool.step()


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
def test_graphs_max_chunk_and_a_second_session_change_no_bit(dt, monkeypatch):
    R, S, M, E = 64, 256, 10, 6
    alone = _alone(R, S, M, E, dt, monkeypatch)
    eager = _scorer(R, S, M, E, dt, monkeypatch, graphs=False)
    _check_session(_session(eager, E)[0], alone, E)
    assert not eager._pool._graphs
    g = _scorer(R, S, M, E, dt, monkeypatch, graphs=True)
    for rep in range(2):                                             # the second session on the same object
        res, _, pool = _session(g, E)
        _check_session(res, alone, E)
        assert pool._graphs
    small = _scorer(R, S, M, E, dt, monkeypatch, max_chunk=32)
    _check_session(_session(small, E, audio_ring=RING)[0], alone, E)


def test_buffer_bytes(monkeypatch):
    s = _scorer(32, 128, 4, 6, BF16, monkeypatch)
    base = s.buffer_bytes()
    pool = s.pool(RING)
    bb = pool.buffer_bytes()
    assert bb["pool audio ring"] == CAP * RING * 4
    assert bb["pool stage + table"] == (4 * CAP + CAP * RING) * 4 + CAP * 2 * 8
    assert bb["pool feed rows"] == CAP * s.max_frames * 4
    assert {k: v for k, v in bb.items() if not k.startswith("pool ")} == base
    with pytest.raises(ValueError, match="audio_ring"):
        s.pool(MAX_CHUNK + 1)
    assert s._pool is pool                                           # a refused pool ends nothing


# ---- the model faces ---------------------------------------------------------------------------------------------------
def test_autoencoder_scorer_pool(tmp_path):
    Md = sub("model")
    dil, P, R, S, M, lat = [1, 2, 4, 8, 1, 2], 16, 32, 128, 4, 8
    Tm = 12 * P
    m = Md.WaveNetAutoEncoder(Tm, 0, M, dil, dilation_channels=R, skip_channels=S, latent_channels=lat, pool_stride=P,
                              dtype=F32, learning_rate=1e-3)
    m.train(O.synthetic_audio(2, Tm, seed=6))
    lengths = [Tm, 5 * P + 7, P - 3, 7 * P]                          # one stream shorter than a frame
    audio = [O.synthetic_audio(1, n, seed=40 + i)[0].astype(np.float32) for i, n in enumerate(lengths)]
    one = m.scorer(max_batch=1, max_chunk=64, max_frames=4)
    want = [one.score(a[None])[0] for a in audio]
    assert [w.shape[0] for w in want] == [n // P * P for n in lengths]
    for maker in (lambda: m.scorer(max_batch=3, max_chunk=64, max_frames=4),
                  lambda: Md.AutoEncoderScorer.from_checkpoint(str(tmp_path), dtype=F32, max_batch=3, max_chunk=64, max_frames=4)):
        assert m.save(str(tmp_path), 5, force=True)
        sc = maker()
        pool = sc.pool()
        assert pool.capacity == 3 and isinstance(pool, Md.AutoEncoderScorerPool)
        rng = np.random.default_rng(9)
        slots = pool.join(n=3)
        assert slots == [0, 1, 2] and pool.free == []
        stream_of, sent, got = dict(zip(slots, range(3))), [0] * 4, {i: [] for i in range(4)}
        left_at = None
        for rnd in range(200):
            if not stream_of:
                break
            for u, i in stream_of.items():
                if sent[i] < lengths[i]:
                    k = int(min(rng.integers(0, 2 * P + 1), pool.audio_room(u), lengths[i] - sent[i]))
                    pool.push(u, audio[i][sent[i]:sent[i] + k])
                    sent[i] += k
                    if sent[i] == lengths[i]:
                        pool.finish(u)
            out = pool.step()
            for u, v in out.items():
                assert isinstance(v, np.ndarray) and v.dtype == np.float32
                got[stream_of[u]].append(v)
            if 1 in stream_of.values() and pool.scored[1] >= 2 * P and left_at is None:      # stream 1 leaves early
                left_at = int(pool.scored[1])
                bps = pool.bits_per_sample(1)
                assert abs(bps - float(np.concatenate(got[1]).astype(np.float64).mean()) / np.log(2.0)) < 1e-9 * abs(bps)
                pool.leave(1)
            for u in [u for u in stream_of if u not in pool.active]:
                del stream_of[u]
            if 2 not in stream_of and 3 not in stream_of.values() and sent[3] == 0:          # the freed slot is reused
                u, = pool.join()
                stream_of[u] = 3
        assert not stream_of and pool.active == []
        cat = lambda p: np.concatenate(p) if p else np.zeros(0, np.float32)
        assert cat(got[2]).shape == (0,)                               # shorter than a frame: nothing, and its slot freed
        for i in (0, 3):
            assert np.array_equal(cat(got[i]), want[i]), i
        assert left_at is not None and np.array_equal(cat(got[1]), want[1][:left_at])
    with pytest.raises(ValueError, match="at least %d" % sub("scorer").ae_pool_min_audio_ring(64, P, sc.encoder._eng.L)):
        sc.pool(audio_ring=65)


def test_teacher_scorer_pool():
    Md = sub("model")
    dil, Tm, R, S, M, lat, P = [1, 2, 4, 8, 1, 2], 192, 32, 128, 10, 4, 16
    rng = np.random.default_rng(2)
    audio = O.synthetic_audio(2, Tm, seed=6).astype(np.float32)
    # unconditioned: audio alone
    m = Md.WaveNetTeacher(Tm, 0, dil, dilation_channels=R, skip_channels=S, dtype=F32, learning_rate=1e-3, head="mol",
                          num_mixtures=M)
    m.train(audio)
    sc = m.mol_scorer(max_batch=2, max_chunk=64)
    want = sc.score(audio)
    pool = sc.pool()
    assert pool.join(n=2) == [0, 1] and pool.room(0) == 0
    pool.push([0, 1], [audio[0, :70], audio[1, :5]])
    a = pool.step()
    pool.push(0, audio[0, 70:])
    b = pool.step()
    assert np.array_equal(np.concatenate([a[0], b[0]]), want[0]) and np.array_equal(a[1], want[1, :5])
    with pytest.raises(ValueError, match="not conditioned"):
        pool.feed(0, np.zeros((1, 4), np.float32))
    assert abs(pool.bits_per_sample(0) - float(want[0].astype(np.float64).mean()) / np.log(2.0)) < 1e-9
    # conditioned: frames fed while the stream runs
    m = Md.WaveNetTeacher(Tm, 0, dil, dilation_channels=R, skip_channels=S, latent_channels=lat, pool_stride=P,
                          use_encoding=True, dtype=F32, learning_rate=1e-3, head="mol", num_mixtures=M)
    enc = rng.normal(size=(2, Tm // P, lat)).astype(np.float32)
    m.train(audio, encoding=enc)
    sc = m.mol_scorer(max_batch=2, max_chunk=64, max_frames=8)
    want = sc.score(audio, enc)
    pool = sc.pool(audio_ring=Tm + 2)
    u, = pool.join()
    pool.push(u, audio[1])
    parts, f0 = [], 0
    while f0 < Tm // P:
        k = min(pool.room(u), 3, Tm // P - f0)
        assert k > 0
        pool.feed(u, enc[1, f0:f0 + k])
        f0 += k
        assert pool.available(u) == f0 * P - pool.scored[u]
        parts.append(pool.step()[u])
    assert pool.fed[u] == Tm // P and np.array_equal(np.concatenate(parts), want[1])
