"""GPU tests of live slots in generation pools (srwn_version() 114): a pool slot that is FED its encoding while the pool
runs -- GenerationPool.join(live=True) / feed / room / close, the rotation of resuming slots' layer-ring columns, the model
faces and the TeacherResynthesisPool -- has the bits of a batch-of-one `generate` over its whole encoding.  Every
comparison is np.array_equal on the uint32 view: there are no tolerances.

The shapes are those of tests/test_gpu_decode_live.py (9 layers with ring depths 2, 3, 5, 9, 17, 33 and 6, both widths, 5
mixtures, latent 8, pool_stride 16, a ring of 4 frames against 11 frames = 176 samples) in a pool of 34 slots: slots 0, 31,
32 and 33 span two ring groups and both workgroup sizes of the latency body."""
import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_decode_live import (BODIES, BODY_IDS, DIL, FRAMES, LAT, POOL, RING, SIZES, T, WIDTHS, _ae, _body,
                                        _engine, _u32)
from tests.test_gpu_kernels import DEV, dev

pytestmark = pytest.mark.gpu

CAP = 34
DEPTHS_OF = [d + 1 for d in DIL]
DEPTHS = sorted(set(DEPTHS_OF))
assert DEPTHS == [2, 3, 5, 6, 9, 17, 33]
_SOLO = {}


def _enc_of(u):
    """Stream u's whole encoding [FRAMES, LAT] (float32 NumPy)."""
    return np.random.default_rng(500 + u).standard_normal((FRAMES, LAT)).astype(np.float32)


def _solo(eng, body, R, u, seed, nsteps=T, **kw):
    """eng.generate of stream u alone over its whole encoding: computed once per case and left unchanged."""
    key = (body, R, u, seed, nsteps, tuple(sorted(kw.items())))
    if key not in _SOLO:
        out = eng.generate(nsteps, mode="sample", seed=seed, batch=1, cond=dev(_enc_of(u))[None], want_logits=True, **kw)
        _SOLO[key] = tuple(_u32(o)[0] for o in out)
    return _SOLO[key]


class _Rec:
    """What a test keeps of one pool run: each slot's outputs, and per launch (clock, n, ran, the open live slots)."""

    def __init__(self):
        self.out, self.launches = {}, []

    def step(self, pool, n, **kw):
        open_live = [u for u in pool.active if pool._live[u] and not pool._closed[u]]
        clock = pool.clock
        a, c, lg, ran = pool.step(n, want_logits=True, **kw)
        self.launches.append((clock, n, ran.copy(), open_live))
        for u in np.flatnonzero(ran):
            k = int(ran[u])
            self.out.setdefault(int(u), []).append((a[u, :k].clone(), c[u, :k].clone(), lg[u, :k].clone()))
        return ran

    def result(self, u):
        return tuple(_u32(torch.cat([o[j] for o in self.out[u]], dim=0)) for j in range(3))


def _same(got, want, n=None):
    for j, name in enumerate(("audio", "codes", "logits")):
        w = want[j] if n is None else want[j][:n]
        assert got[j].shape == w.shape, (name, got[j].shape, w.shape)
        assert np.array_equal(got[j], w), name


# ---------------------------------------------------------------------------------------------------
# 1. the rotation against NumPy
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("R", [64, 32])
def test_rotation_against_numpy(dt, R):
    K, L = sub("kernels"), sub("_lib")
    import ctypes
    dil = (ctypes.c_int32 * len(DIL))(*DIL)
    group = int(L.load().srwn_generate_ring_elems(dil, len(DIL), R))
    assert group == sum(DEPTHS_OF) * 32 * R
    idx = torch.arange(2 * group, dtype=torch.int64)                # a ring of two groups, its values told apart by position
    if dt == torch.bfloat16:
        ring = ((idx * 40503) % 65536 - 32768).to(torch.int16).view(torch.bfloat16)
    else:
        ring = idx.to(torch.int32).view(torch.float32)
    ring = ring.to(DEV)
    bits = torch.int16 if dt == torch.bfloat16 else torch.int32
    before = ring.view(bits).cpu().numpy().copy()
    slots, shifts = [0, 31, 32, 33], [1, 7, 6 * 33 * 5, 1000003]
    ids = torch.tensor(slots, dtype=torch.int32, device=DEV)

    def layers(flat):
        """{(slot, layer): [depth, R]} views of a flat ring image."""
        out, off = {}, 0
        for l, d in enumerate(DIL):
            blk = [flat[g * group + off: g * group + off + (d + 1) * 32 * R].reshape(d + 1, 32, R) for g in range(2)]
            for u in range(64):
                out[u, l] = blk[u >> 5][:, u & 31]
            off += (d + 1) * 32 * R
        return out

    K.ring_rotate_slots(ring, dil, len(DIL), CAP, R, ids, torch.zeros(4, dtype=torch.int32, device=DEV))
    assert np.array_equal(ring.view(bits).cpu().numpy(), before)    # shift 0: every bit stays
    K.ring_rotate_slots(ring, dil, len(DIL), CAP, R, ids, torch.tensor(shifts, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    old, new = layers(before), layers(ring.view(bits).cpu().numpy())
    moved = 0
    for (u, l), col in old.items():
        if u in slots:
            want = np.roll(col, shifts[slots.index(u)], axis=0)     # new[(p + s) mod D] = old[p]
            moved += not np.array_equal(want, col)
        else:
            want = col
        assert np.array_equal(new[u, l], want), (u, l)
    assert moved >= 3 * len(DIL)                                     # (6 * 33 * 5 is 0 mod most depths: those columns stay)


# ---------------------------------------------------------------------------------------------------
# 2. starved slots equal solo runs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", WIDTHS)
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_starved_slots_equal_solo_runs(monkeypatch, body, R, S):
    dt = _body(monkeypatch, body)
    eng = _engine(dt, R, S)
    pool = eng.generation_pool(CAP, RING, live=True)
    assert pool.live and pool.frames == RING
    A, D, B, C, E = 0, 1, 31, 32, 33                                 # (a) bursts, (d) bounded, (b) one frame, (c) mid-launch, (e) late
    seeds = {A: 11, D: 12, B: 13, C: 14, E: 15}
    enc = {u: dev(_enc_of(u)) for u in seeds}
    pool.join([seeds[A], seeds[B], seeds[C]], cond=[enc[A][:0], enc[B][:1], None], slots=[A, B, C], live=True)
    pool.join([seeds[D]], cond=[enc[D][:RING]], slots=[D])          # bounded: its 4 frames in rows 0..3, 64 samples
    assert pool.room(A) == RING and pool.room(B) == RING - 1 and pool.room(D) == 0 and pool.room(5) == 0
    rec, i = _Rec(), 0
    live = [A, B, C]
    stopped = {A: 0, B: 0, C: 0, D: 0}
    shifts = []
    while pool.active:
        if i == 2:
            assert pool.clock > 0
            pool.join([seeds[E]], cond=[enc[E][:1]], slots=[E], live=True)
            live.append(E)
            stopped[E] = pool.clock
        for u in live:
            if u not in pool.active or pool._closed[u]:
                continue
            fed, room = int(pool._fed[u]), pool.room(u)
            if u == A:
                k = min(room, FRAMES - fed)
            elif u == B:
                k = min(1, room, FRAMES - fed) if i % 3 == 0 else 0
            elif u == C:
                k = min(2, room, FRAMES - fed) if pool.t[u] == fed * POOL else 0
            else:
                k = min(1, room, FRAMES - fed)
            if k > 0:
                pool.feed([u], [enc[u][fed:fed + k]])
            if int(pool._fed[u]) == FRAMES:
                pool.close([u])
        n = SIZES[i % 3]
        clock = pool.clock
        ran = rec.step(pool, n)
        for u in np.flatnonzero(ran):
            shifts.append(clock - stopped[int(u)])
            stopped[int(u)] = clock + int(ran[u])
        i += 1
        assert i < 400
    # what the run exercised, from the clocks and `ran` alone
    assert any(0 < r < n for _, n, ran, _ in rec.launches for r in ran)                    # ran out mid-launch
    assert any(ran[u] == 0 for _, _, ran, op in rec.launches for u in op)                  # idled through a whole launch
    for depth in DEPTHS:
        assert any(s % depth for s in shifts), depth
    for u in live:
        assert pool._fed[u] == FRAMES > 2 * RING and pool.t[u] == T
    for u in live:
        _same(rec.result(u), _solo(eng, body, R, u, seeds[u]))
    _same(rec.result(D), _solo(eng, body, R, D, seeds[D]), RING * POOL)
    assert sorted(rec.out) == [A, D, B, C, E] and pool.free == list(range(CAP))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 3. teacher forcing and prompts
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_forcing_and_prompts_on_live_slots(monkeypatch, body):
    dt = _body(monkeypatch, body)
    R, S = 64, 256
    eng = _engine(dt, R, S)
    u, v, P = 32, 31, 20
    eu, ev = dev(_enc_of(u)), dev(_enc_of(v))
    f = O.synthetic_audio(1, T, seed=5).astype(np.float32)[0]
    out = eng.generate(T, mode="sample", seed=31, batch=1, cond=eu[None], want_logits=True, forced=dev(f)[None])
    want_forced = tuple(_u32(o)[0] for o in out)
    assert not np.array_equal(want_forced[2], _solo(eng, body, R, u, 31)[2])
    prompt = O.synthetic_audio(1, P, seed=9).astype(np.float32)
    st = eng.generation_state(1, ev[None], 32)
    eng.prime(st, dev(prompt))
    want_p = tuple(_u32(o)[0] for o in eng.generate_chunk(st, T - P, want_logits=True))

    def drive(pool, w, e, forced):
        """Slot w fed one frame at a time, and only once it has starved; every launch teacher-forced where `forced`."""
        rec, i, short = _Rec(), 0, 0
        while pool.active:
            fed = int(pool._fed[w])
            if not pool._closed[w]:
                if pool.t[w] == fed * POOL and fed < FRAMES:
                    pool.feed([w], [e[fed:fed + 1]])
                if int(pool._fed[w]) == FRAMES:
                    pool.close([w])
            n = SIZES[i % 3]
            fr = None
            if forced is not None:                                   # row w: the slot's own next n samples of the forced clip
                fr = torch.zeros((CAP, n), dtype=torch.float32)
                seg = forced[int(pool.t[w]):int(pool.t[w]) + n]
                fr[w, :len(seg)] = torch.from_numpy(seg)
                fr = fr.to(DEV)
            ran = rec.step(pool, n, forced=fr)
            short += int(ran[w] < n)
            i += 1
            assert i < 400
        assert short > 3
        return rec.result(w)

    pool = eng.generation_pool(CAP, RING, live=True)
    pool.join([31], cond=[eu[:1]], slots=[u], live=True)
    _same(drive(pool, u, eu, f), want_forced)
    # the prompted stream joins the same pool at clock > 0: its prompt's layer inputs enter the rings at that phase
    assert pool.clock > T
    with pytest.raises(ValueError, match="exceeds"):
        pool.join([32], prompts=[prompt[0]], cond=[ev[:1]], slots=[v], live=True)          # 20 samples, one frame
    assert pool.active == []
    pool.join([32], prompts=[prompt[0]], cond=[ev[:2]], slots=[v], live=True)
    assert pool.t[v] == P and pool.room(v) == RING - 2 + P // POOL
    _same(drive(pool, v, ev, None), want_p)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 4. per-slot temperature
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_temperatures_on_live_slots(monkeypatch, body):
    dt = _body(monkeypatch, body)
    R, S = 32, 128
    eng = _engine(dt, R, S)
    slots, temps, seeds = [0, 32, 33], [0.7, 1.0, 1.3], [41, 42, 43]
    enc = {u: dev(_enc_of(u)) for u in slots}
    want = {u: _solo(eng, body, R, u, s, temperature=t) for u, s, t in zip(slots, seeds, temps)}
    assert not np.array_equal(want[0][0], _solo(eng, body, R, 0, 41)[0])
    pool = eng.generation_pool(CAP, RING, live=True)
    pool.join(seeds, cond=[enc[u][:1] for u in slots], slots=slots, temperature=temps, live=True)
    assert pool.sampling is not None
    rec, i = _Rec(), 0
    while pool.active:
        for u in slots:
            if u in pool.active and not pool._closed[u]:
                fed = int(pool._fed[u])
                k = min(pool.room(u), FRAMES - fed, 1 + (u & 1))
                if k > 0 and (i + u) % 2 == 0:
                    pool.feed([u], [enc[u][fed:fed + k]])
                if int(pool._fed[u]) == FRAMES:
                    pool.close([u])
        rec.step(pool, SIZES[i % 3])
        i += 1
        assert i < 400
    for u in slots:
        _same(rec.result(u), want[u])


# ---------------------------------------------------------------------------------------------------
# 5. close / leave / reuse; a plain pool afterwards
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_close_leave_and_reuse(monkeypatch, body):
    dt = _body(monkeypatch, body)
    R, S = 64, 256
    eng = _engine(dt, R, S)
    pool = eng.generation_pool(CAP, RING, live=True)
    e0, e1 = dev(_enc_of(0)), dev(_enc_of(1))
    pool.join([51, 52], cond=[e0[:2], e1[:1]], slots=[0, 1], live=True)
    pool.close([0])
    rec = _Rec()
    ran = rec.step(pool, 50)
    assert ran[0] == 2 * POOL and ran[1] == POOL                    # the closed slot frees exactly at fed * pool_stride,
    assert pool.active == [1] and pool.t[0] == 2 * POOL             # the starved one stays taken
    _same(rec.result(0), _solo(eng, body, R, 0, 51), 2 * POOL)
    ran = rec.step(pool, 7)
    assert ran[1] == 0 and pool.active == [1]
    with pytest.raises(ValueError, match="no live, open stream"):
        pool.feed([0], [e0[2:3]])                                    # slot 0 is free
    pool.leave([1])                                                  # a starved slot can leave
    assert pool.active == [] and pool.room(1) == 0
    # the freed slots again: a live stream in slot 0 (closed at once at its end: zero frames), then a real one, and a
    # bounded stream in slot 1 -- joined at clock 57, so their rings are filled at that phase
    pool.join([53], cond=[None], slots=[0], live=True)
    pool.close([0])
    assert pool.active == [] and pool.clock == 57
    e3, e4 = dev(_enc_of(3)), dev(_enc_of(4))
    pool.join([53], cond=[e3[:1]], slots=[0], live=True)
    pool.join([54], cond=[e4[:3]], slots=[1])
    rec, i = _Rec(), 0
    while pool.active:
        if 0 in pool.active and not pool._closed[0]:
            fed = int(pool._fed[0])
            if pool.t[0] == fed * POOL and fed < FRAMES:
                pool.feed([0], [e3[fed:fed + 1]])
            if int(pool._fed[0]) == FRAMES:
                pool.close([0])
        rec.step(pool, SIZES[i % 3])
        i += 1
        assert i < 400
    _same(rec.result(0), _solo(eng, body, R, 3, 53))
    _same(rec.result(1), _solo(eng, body, R, 4, 54), 3 * POOL)
    # a pool made without `live` on the same engine afterwards: the launches it always ran, the bits of its solo runs
    plain = eng.generation_pool(3, FRAMES)
    assert not plain.live
    with pytest.raises(ValueError, match="live=True"):
        plain.join([55], cond=[e3[:1]], live=True)
    plain.join([55, 56], cond=[e3, e4])
    outs = [plain.step(n, want_logits=True) for n in (50, 7, T - 57)]
    for row, (u, s) in enumerate(((3, 55), (4, 56))):
        got = tuple(_u32(torch.cat([o[j][row] for o in outs], dim=0)) for j in range(3))
        _same(got, _solo(eng, body, R, u, s))
    assert plain.free == [0, 1, 2]


# ---------------------------------------------------------------------------------------------------
# 6. the feed's rows are the one-shot table's
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_feed_rows_are_the_one_shot_tables(dt):
    eng = _engine(dt, 32, 128)
    pool = eng.generation_pool(CAP, RING, live=True)
    slots = [0, 31, 33]
    enc = {u: dev(_enc_of(u)) for u in slots}
    table = {u: eng._project_cond(enc[u]) for u in slots}            # [FRAMES, L*R] each, one call per stream
    pool.join([1, 2, 3], cond=[None, enc[31][:1], enc[33][:2]], slots=slots, live=True)
    pool.feed(slots, [enc[0][:2], enc[31][1:4], enc[33][2:3].cpu().numpy()])      # ragged: 2, 3 and 1 frames
    assert [int(pool._fed[u]) for u in slots] == [2, 4, 3] and [pool.room(u) for u in slots] == [2, 0, 1]
    before = pool.cond_all.clone()
    with pytest.raises(ValueError, match="room for 0"):
        pool.feed([0, 31], [enc[0][2:3], enc[31][4:5]])              # slot 31's ring is full: nothing changes, slot 0 included
    with pytest.raises(ValueError, match="distinct slots"):
        pool.feed([0, 33], [enc[0][2:3]])
    assert torch.equal(pool.cond_all, before) and [int(pool._fed[u]) for u in slots] == [2, 4, 3]
    pool.step(40)                                                    # 32, 40 and 40 samples: frames 0 / 0, 1 / 0, 1 are done
    assert [int(pool.t[u]) for u in slots] == [32, 40, 40] and [pool.room(u) for u in slots] == [4, 2, 3]
    pool.feed([33, 0], [enc[33][3:6], enc[0][2:6]])
    pool.feed(31, enc[31][4:6])                                      # one slot, one 2-D array
    fed = {0: 6, 31: 6, 33: 6}
    ring = pool.cond_all.view(CAP, RING, -1)
    for u in slots:
        assert int(pool._fed[u]) == fed[u] and int(pool._end[u]) == fed[u] * POOL
        for q in range(fed[u] - RING, fed[u]):
            assert torch.equal(ring[u, q % RING], table[u][q]), (u, q)
    assert int(ring[[1, 2, 30, 32]].abs().sum()) == 0                # the other slots' rows were not touched
    tab = pool.slots.cpu().numpy()
    assert tab[slots, 1].tolist() == [6 * POOL] * 3                  # the device table's t_end with the host mirror's
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 7. the model level
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_model_pool_live_streams(monkeypatch, body):
    dt = _body(monkeypatch, body)
    ae = _ae(dt, 64, 256, cs=3)
    rng = np.random.default_rng(77)
    encs = rng.standard_normal((2, FRAMES, LAT)).astype(np.float32)
    conds = rng.standard_normal((2, 3)).astype(np.float32)
    want = [ae.generate(encs[i:i + 1], conditions=conds[i:i + 1], seed=60 + i)[0] for i in range(2)]
    gp = ae.generation_pool(3, RING, live=True)
    a, = gp.join(seed=60, encoding=encs[0][:2], conditions=conds[0], live=True)           # a single 2-D array: one stream
    assert (a, gp.room(a), gp.active) == (0, RING - 2, [0])
    got, i, b = {0: [], 1: []}, 0, None
    fed = {0: 2, 1: 0}
    while gp.active or b is None:
        if i == 1:
            b, = gp.join(seed=[61], encoding=[encs[1][:0]], conditions=[conds[1]], live=True)
            assert b == 1 and gp.room(b) == RING
        for s, u in ((0, a), (1, b)):
            if u is None or u not in gp.active or fed[s] == FRAMES:
                continue
            k = min(gp.room(u), FRAMES - fed[s], 1 + s)
            if k > 0:
                gp.feed(u if s == 0 else [u], encs[s][fed[s]:fed[s] + k] if s == 0 else [encs[s][fed[s]:fed[s] + k]])
                fed[s] += k
            if fed[s] == FRAMES:
                gp.close(u)
        for u, y in gp.step(SIZES[i % 3]).items():
            got[u].append(y)
        i += 1
        assert i < 400
    for s in range(2):
        assert np.array_equal(_u32(np.concatenate(got[s])), _u32(want[s])), s


@pytest.mark.parametrize("R,S", WIDTHS)
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_teacher_resynthesis_pool(monkeypatch, body, R, S):
    """Three streams on three slots joining at different times, audio in pieces of 0..2 * pool_stride samples, one finishing
    early and its slot taken again: each receives ae.generate(encoder.encode(audio)) of it alone."""
    dt = _body(monkeypatch, body)
    ae = _ae(dt, R, S)
    Mo = sub("model")
    rs = ae.resynthesizer(max_batch=3, max_frames=RING)
    lengths, seeds, temps = [T + 5, 3 * POOL + 2, T, 5 * POOL], [71, 72, 73, 74], [1.0, 0.8, 1.2, 1.0]
    whole = [O.synthetic_audio(1, n, seed=80 + i).astype(np.float32) for i, n in enumerate(lengths)]
    clips = [w[0] for w in whole]
    want = [ae.generate(rs.encoder.encode(w), seed=s, temperature=t)[0] for w, s, t in zip(whole, seeds, temps)]
    assert [len(w) for w in want] == [T, 3 * POOL, T, 5 * POOL]
    rp = rs.pool(chunk_size=50)
    assert isinstance(rp, Mo.TeacherResynthesisPool) and rp.capacity == 3 and rp.step() == {}
    slot_of, pushed, finished, got = {}, [0] * 4, set(), [[] for _ in range(4)]
    join_at = {0: 0, 1: 0, 2: 1}      # (stream 1 needs two pushes at least: its slot cannot be free before stream 2 has one)
    rng = np.random.default_rng(9)
    step = 0
    while rp.active or len(slot_of) < 4:
        for i, at in join_at.items():
            if i not in slot_of and step >= at:
                slot_of[i], = rp.join(seed=seeds[i], temperature=temps[i])
        if 3 not in slot_of and 1 in finished and slot_of[1] not in rp.active:
            slot_of[3], = rp.join(seed=[seeds[3]], temperature=[temps[3]])                  # the early finisher's slot again
            assert slot_of[3] == slot_of[1] and rp.t[slot_of[3]] == 0 and rp.received[slot_of[3]] == 0
        holder = {u: i for i, u in slot_of.items() if u in rp.active and not (i == 1 and 3 in slot_of) and i not in finished}
        us, xs = [], []
        for u, i in sorted(holder.items()):
            k = min(int(rng.integers(0, 2 * POOL + 1)), len(clips[i]) - pushed[i], rp.audio_room(u))
            us.append(u); xs.append(clips[i][pushed[i]:pushed[i] + k])
            pushed[i] += k
        if us:
            rp.push(us, xs)
        fin = [u for u, i in holder.items() if pushed[i] == len(clips[i])]
        if fin:
            rp.finish(fin)
            finished |= {holder[u] for u in fin}
        live_now = {u: i for i, u in slot_of.items() if u in rp.active and not (i == 1 and 3 in slot_of)}
        for u, y in rp.step().items():
            assert y.dtype == np.float32 and 1 <= len(y) <= 50
            got[live_now[u]].append(y)
        step += 1
        assert step < 2000
    assert rp.step() == {} and rp.free == [0, 1, 2] and rp._enc.free == [0, 1, 2] and rp._dec.free == [0, 1, 2]
    for i in range(4):
        g = np.concatenate(got[i])
        assert g.shape == want[i].shape, i
        assert np.array_equal(_u32(g), _u32(want[i])), i
    torch.cuda.synchronize()
