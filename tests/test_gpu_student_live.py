"""GPU tests of live synthesis (srwn_version() 110): a stream that is FED its encoding while it runs -- through
FlowSynthesizer.feed, a live slot of a SynthPool, or the Resynthesizer pipeline -- has the bits of a stream that got its
whole encoding at the start.  Everything is compared with torch.equal: there are no tolerances.

The shapes are the smallest that wrap the conditioning ring and hold both kinds of layer group: dilations [1..128] x 2
(history rows 31 / 224), 2 flows, pool_stride 64 and a ring of max_frames = 6 against 24 frames of stream (four wraps)."""
import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_student_stream import _synth

pytestmark = pytest.mark.gpu

DIL = [1, 2, 4, 8, 16, 32, 64, 128] * 2
F, POOL, RING, FRAMES, CHUNK = 2, 64, 6, 24, 300
T = FRAMES * POOL
# wanted chunk sizes, cut to what the fed frames allow: 1, hist -1/0/+1 of both group kinds, frame boundaries +-1, sizes
# repeated three times in a row (eager, capture, replay under graphs) and max_chunk
SIZES = [64, 64, 64, 1, 1, 1, 30, 31, 32, 37, 37, 37, 63, 65, 128, 160, 223, 224, 225, 300, 37, 64, 1]
CASES = [(torch.float32, 32, 5), (torch.float32, 64, 8), (torch.bfloat16, 32, 8), (torch.bfloat16, 64, 5)]
IDS = ["fp32-R32-E5", "fp32-R64-E8", "bf16-R32-E8", "bf16-R64-E5"]


def _pair(dt, R, E, max_batch, ring=RING):
    """A synthesizer on a ring of `ring` frames and a twin with the same weights that holds the whole encoding."""
    live, _ = _synth(dt, R, DIL, F, E, POOL, max_batch, CHUNK, ring)
    whole, _ = _synth(dt, R, DIL, F, E, POOL, max_batch, CHUNK, FRAMES + 1)
    return live, whole


def _whole(whole, cond, seeds, temps):
    st = whole.start(cond, seeds, temps)
    out = []
    while st.t < st.limit:
        out.append(whole.step(st, min(CHUNK, st.limit - st.t)))
    torch.cuda.synchronize()
    return torch.cat(out, 1)


def _drive(syn, st, cond, want, ks, sizes=SIZES):
    """Feeds cond [B, frames, E] in pieces of ks (cut to the room) and steps through `sizes` (cut to what is available),
    comparing every chunk with want[:, t:t+n].  Returns the chunk sizes that ran."""
    frames, ran, i = cond.shape[1], [], 0
    while st.t < frames * POOL:
        n = sizes[i % len(sizes)]
        while st.fed < frames and st.limit - st.t < n and syn.room(st) > 0:
            k = min(ks[(st.fed + i) % len(ks)], syn.room(st), frames - st.fed)
            syn.feed(st, cond[:, st.fed:st.fed + k])
        n = min(n, st.limit - st.t)
        assert n >= 1, (st.t, st.fed)
        t0 = st.t
        got = syn.step(st, n)
        assert torch.equal(got, want[:, t0:t0 + n]), (t0, n, st.fed)
        ran.append(n)
        i += 1
        assert i < 2000
    return ran


# ---------------------------------------------------------------------------------------------------
# 1. live equals whole
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,R,E", CASES, ids=IDS)
def test_live_stream_has_the_bits_of_the_whole_encoding(dt, R, E):
    B = 3
    live, whole = _pair(dt, R, E, 4)
    assert live.hist == [31, 224, 31, 224]
    rng = np.random.default_rng(R + E)
    cond = torch.tensor(rng.standard_normal((B, FRAMES, E)), dtype=torch.float32)
    seeds, temps = [7, 70, 700], [0.3, 0.2, 0.4]      # (low temperatures: most samples stay inside the clamp)
    want = _whole(whole, cond, seeds, temps)
    assert want.shape == (B, T) and torch.isfinite(want).all() and (want.abs() < 1).float().mean() > 0.5
    assert not torch.equal(want[0], want[1])
    for graphs in (False, True):
        live.use_graphs = graphs
        for ks, on_device, first in (([1], False, 0), ([2, 1, 3], True, 2), ([3], True, RING)):
            c = cond.to("cuda") if on_device else cond
            st = live.start(c[:, :first] if first else None, seeds, temps, live=True, batch=B)
            assert st.live and st.fed == first and st.limit == first * POOL and live.room(st) == RING - first
            ran = _drive(live, st, c, want, ks)
            assert st.fed == FRAMES > 4 * RING - 1 and st.t == T
            assert {1, 30, 31, 32, 63, 64, 65} <= set(ran) and max(ran) > 97      # (a ring of 6 allows 97..160 at a time)
            with pytest.raises(ValueError, match="encoding ends"):
                live.step(st, 1)
        if graphs:
            assert any(k[1] == 64 for k in live._graphs) and any(k[1] == 1 for k in live._graphs)
        else:
            assert not live._graphs
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 2. feed equals start
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,R,E", CASES, ids=IDS)
def test_fed_rows_are_the_rows_start_writes(dt, R, E):
    """srwn_cond_ring_feed writes the rows srwn_pw_linear_ychunks writes for the same frames: fed in pieces, and with a
    feed that straddles the wrap (frames 5 and 6 -> rows 5 and 0)."""
    B = 3
    live, _ = _pair(dt, R, E, 4)
    ref, _ = _synth(dt, R, DIL, F, E, POOL, 4, CHUNK, RING)
    rng = np.random.default_rng(5)
    cond = torch.tensor(rng.standard_normal((B, RING + 1, E)), dtype=torch.float32)

    def rows(syn):
        torch.cuda.synchronize()
        return [c.view(syn.L, syn.max_batch, RING, R)[:, :B].clone() for c in syn.cond_all]

    st = live.start(None, 1, 1.0, live=True, batch=B)
    for a, b in ((0, 2), (2, 5)):
        live.feed(st, cond[:, a:b].to("cuda"))
    ref.start(cond[:, :5])
    for x, y in zip(rows(live), rows(ref)):
        assert torch.equal(x[:, :, :5], y[:, :, :5])
    assert live.room(st) == 1
    while st.t < 320:
        live.step(st, 160)
    assert live.room(st) == RING - 5 + (320 - 224) // POOL == 2
    live.feed(st, cond[:, 5:7])                                  # rows 5 and 0
    assert st.fed == 7 and st.limit == 7 * POOL
    ref.start(torch.cat([cond[:, 6:7], cond[:, 1:6]], 1))       # ring order: frame 6 sits where frame 0 sat
    for x, y in zip(rows(live), rows(ref)):
        assert torch.equal(x, y)
        assert x.float().abs().max() > 0


# ---------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched():
    dt, R, E, B = torch.bfloat16, 64, 5, 2
    live, whole = _pair(dt, R, E, 2)
    rng = np.random.default_rng(9)
    cond = torch.tensor(rng.standard_normal((B, FRAMES, E)), dtype=torch.float32)
    want = _whole(whole, cond, 3, 0.3)
    small, _ = _synth(dt, R, DIL, F, E, POOL, 2, CHUNK, 4)
    with pytest.raises(ValueError, match=r"= 5 frames"):           # ceil(224 / 64) + 1
        small.start(None, 0, 1.0, live=True)
    assert small.start(cond[:, :4]).limit == 4 * POOL                # ... a bounded stream runs there as before
    with pytest.raises(ValueError, match="max_frames"):
        live.start(cond[:, :RING + 1], 3, 1.0, live=True)           # more first frames than the ring holds

    bounded = live.start(cond[:, :RING], 3, 0.3)
    assert not bounded.live and live.room(bounded) == 0
    tables = [c.clone() for c in live.cond_all]
    with pytest.raises(ValueError, match="live"):
        live.feed(bounded, cond[:, :1])
    assert bounded.limit == RING * POOL and all(torch.equal(a, b) for a, b in zip(tables, live.cond_all))
    assert torch.equal(live.step(bounded, 100), want[:, :100])

    st = live.start(cond[:, :4], 3, 0.3, live=True)
    assert live.room(st) == 2
    with pytest.raises(ValueError, match="room for 2"):
        live.feed(st, cond[:, 4:7])
    with pytest.raises(ValueError, match="frames must be"):
        live.feed(st, cond[:1, 4:5])
    with pytest.raises(ValueError, match="encoding ends"):
        live.step(st, 4 * POOL + 1)                                  # past fed * pool_stride
    assert (st.fed, st.t, st.limit) == (4, 0, 4 * POOL)
    assert torch.equal(live.step(st, 4 * POOL), want[:, :4 * POOL])
    live.feed(st, cond[:, 4:6])
    assert live.room(st) == RING - 6 + (256 - 224) // POOL == 0
    tables = [c.clone() for c in live.cond_all]
    with pytest.raises(ValueError, match="room for 0"):
        live.feed(st, cond[:, 6:7])
    torch.cuda.synchronize()
    assert st.fed == 6 and all(torch.equal(a, b) for a, b in zip(tables, live.cond_all))
    assert torch.equal(live.step(st, 37), want[:, 256:293])          # after the refused feed: the expected bits
    _drive(live, st, cond, want, [2])
    other = live.start(None, 0, 1.0, live=True)
    with pytest.raises(ValueError, match="current"):
        live.feed(st, cond[:, :1])
    assert other.fed == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 4. pool: bounded and live slots side by side
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,R", [(torch.float32, 32), (torch.bfloat16, 64)], ids=["fp32-R32", "bf16-R64"])
def test_pool_live_and_bounded_slots(dt, R):
    E = 5
    syn, _ = _synth(dt, R, DIL, F, E, POOL, 4, CHUNK, RING)
    ref, _ = _synth(dt, R, DIL, F, E, POOL, 1, CHUNK, FRAMES + 1)
    rng = np.random.default_rng(21)
    spec = {"A": dict(frames=5, mx=None, live=False), "B": dict(frames=6, mx=300, live=False),
            "L1": dict(frames=FRAMES, mx=None, live=True), "L2": dict(frames=FRAMES, mx=None, live=True)}
    for i, (name, s) in enumerate(spec.items()):
        s["cond"] = rng.standard_normal((s["frames"], E)).astype(np.float32)
        s["seed"], s["temp"] = 100 + 13 * i, [0.3, 0.2, 0.4, 0.25][i]
        s["end"] = s["frames"] * POOL if s["mx"] is None else s["mx"]
        st = ref.start(torch.as_tensor(s["cond"])[None], [s["seed"]], [s["temp"]])
        out = []
        while st.t < st.limit:
            out.append(ref.step(st, min(CHUNK, st.limit - st.t))[0])
        s["want"] = torch.cat(out)[:s["end"]]
    sizes = [64, 37, 1, 100, 64, 64, 31, 160, 225]

    for graphs in (False, True):
        syn.use_graphs = graphs
        P = syn.pool()
        got = {k: [] for k in spec}
        where, fed = {}, {"L1": 2, "L2": 0}
        starved = {"L1": 0, "L2": 0}
        resumed = {"L1": 0, "L2": 0}
        with pytest.raises(ValueError, match="max_samples"):
            P.join([None], [1], live=True, max_samples=10)
        # a bounded and a live stream (its first two frames) at once
        assert P.join([spec["A"]["cond"]], [spec["A"]["seed"]], [spec["A"]["temp"]]) == [0]
        assert P.join([spec["L1"]["cond"][:2]], [spec["L1"]["seed"]], [spec["L1"]["temp"]], live=True) == [1]
        where[0], where[1] = "A", "L1"
        assert P.room(1) == RING - 2 and P.room(0) == 0
        with pytest.raises(ValueError, match="no live"):
            P.feed([0], [spec["A"]["cond"][:1]])
        with pytest.raises(ValueError, match="room for"):
            P.feed([1], [spec["L1"]["cond"][2:2 + RING - 1]])
        step, closed_late = 0, False
        while P.active:
            if step == 2:                                             # a live stream with no frame yet: starved from the start
                assert P.join([None], [spec["L2"]["seed"]], [spec["L2"]["temp"]], live=True) == [2]
                where[2] = "L2"
                assert 2 in P.active and P.room(2) == RING
            if step == 3:
                s = spec["B"]
                assert P.join([s["cond"]], [s["seed"]], [s["temp"]], [s["mx"]]) == [3]
                where[3] = "B"
            # L1: two frames a tick; L2: one frame every third tick (it starves in between); both in ONE feed when due
            us, fr = [], []
            for name, u, k, due in (("L1", 1, 2, True), ("L2", 2, 1, step >= 2 and step % 3 == 0)):
                if u in where and where[u] == name and u in P.active and due and fed[name] < FRAMES:
                    k = min(k, P.room(u), FRAMES - fed[name])
                    if k:
                        us.append(u); fr.append(torch.as_tensor(spec[name]["cond"][fed[name]:fed[name] + k]).to("cuda"))
                        fed[name] += k
            if us:
                P.feed(us, fr)
            if fed["L1"] == FRAMES and 1 in P.active and where[1] == "L1":
                P.close([1])                                          # closed with samples left: frees itself at its end
            t0 = P.t
            if fed["L2"] == FRAMES and 2 in P.active and t0[2] == T:
                P.close([2])                                          # closed at its end: free at once
                closed_late = True
                assert 2 in P.free
                if not P.active:
                    break
            n = sizes[step % len(sizes)]
            active = P.active
            audio, ran = P.step(n)
            assert np.array_equal(P.t, t0 + ran)
            for u in range(4):
                if ran[u]:
                    got[where[u]].append(audio[u, :ran[u]])
                assert not audio[u, ran[u]:].any()
            for name, u in (("L1", 1), ("L2", 2)):
                if u in active and where.get(u) == name and u in P.active:
                    if ran[u] == 0:
                        starved[name] += 1                            # active, no rows: starved, not ended
                    elif starved[name]:
                        resumed[name] += 1
            step += 1
            assert step < 1500
        torch.cuda.synchronize()
        assert closed_late and starved["L2"] > 3 and resumed["L2"] > 3, (starved, resumed)
        assert P.free == [0, 1, 2, 3]
        for name, s in spec.items():
            g = torch.cat(got[name])
            assert g.shape == (s["end"],), (graphs, name, g.shape)
            assert torch.equal(g, s["want"]), (graphs, name)
        assert bool(P._graphs) == graphs


# ---------------------------------------------------------------------------------------------------
# 5. the pipeline: audio in, resynthesized audio out
# ---------------------------------------------------------------------------------------------------
def _models(dt, R, cs, lat=5, ring=RING, max_frames_whole=FRAMES + 1):
    M = sub("model")
    enc = M.AudioEncoder(4, skip_channels=64, latent_channels=lat, pool_stride=POOL, dtype=dt, max_batch=2, max_frames=8)
    enc._w.load_oracle_params(O.init_encoder_params(4, 4, 2, 128, 64, lat, bias_scale=0.05))
    flows = [O.init_flow_params(60 + i, DIL, 2, R, 4 * R, lat + cs, bias_scale=0.05) for i in range(F)]
    for p in flows:
        p.head_w2 = p.head_w2 * 0.3      # keep exp(.) moderate so that the clamp does not hide differences
    syns = []
    for mf in (ring, max_frames_whole):
        s = M.StudentSynthesizer(DIL, F, dilation_channels=R, latent_channels=lat, condition_size=cs, pool_stride=POOL,
                                 dtype=dt, max_batch=2, max_chunk=CHUNK, max_frames=mf)
        for w, p in zip(s._eng.weights, flows):
            w.load_oracle_params(p)
        syns.append(s)
    return M, enc, syns[0], syns[1]


@pytest.mark.parametrize("dt,R,cs", [(torch.bfloat16, 64, 3), (torch.float32, 32, 0), (torch.bfloat16, 32, 0)],
                         ids=["bf16-R64-cond3", "fp32-R32", "bf16-R32"])
def test_resynthesizer_equals_encode_then_synthesize(dt, R, cs):
    M, enc, syn, whole = _models(dt, R, cs)
    B, TA = 2, 1600
    audio = O.synthetic_audio(B, TA, seed=3).astype(np.float32)
    y = None if cs == 0 else np.random.default_rng(1).standard_normal((B, cs)).astype(np.float32)
    encoding = enc.encode(audio)
    assert encoding.shape == (B, TA // POOL, 5)
    want = whole.synthesize(encoding, y, seed=11, temperature=0.3)
    assert want.shape == (B, (TA // POOL) * POOL, 1) and np.abs(want).max() <= 1 and (np.abs(want) < 1).mean() > 0.5

    rs = M.Resynthesizer(enc, syn)
    assert rs.lookahead == POOL + 4 + 1
    for chunk in (160, 37):
        s = rs.stream(batch=B, conditions=y, seed=11, temperature=0.3, chunk_size=chunk)
        parts, t = [], 0
        for m in (1, 63, 64, 65, 300):
            out = s.push(audio[:, t:t + m])
            t += m
            assert out.dtype == np.float32 and out.shape[0] == B and out.shape[2] == 1
            due = max(0, (t - 4 - 1) // POOL) * POOL
            assert s.t == due and sum(p.shape[1] for p in parts) + out.shape[1] == due
            if t <= 64:
                assert out.shape == (B, 0, 1)                         # before the first frame's look-ahead is complete
            parts.append(out)
        out = s.push(audio[:, t:])                                   # 1107 samples: 17 frames through a ring of 6
        assert out.shape[1] > RING * POOL
        parts.append(out)
        parts.append(s.finish())
        got = np.concatenate(parts, axis=1)
        assert got.shape == (B, (TA // POOL) * POOL, 1)
        assert np.array_equal(got, want), chunk
        with pytest.raises(ValueError, match="closed"):
            s.push(audio[:, :1])

    # the NumPy face of a live batch and of a live pool slot: the same samples
    lv = syn.live(B, conditions=y, seed=11, temperature=0.3)
    assert (lv.t, lv.fed, lv.room, lv.available) == (0, 0, RING, 0)
    lv.feed(encoding[:, :3])
    assert lv.available == 3 * POOL
    assert np.array_equal(lv.step(100), want[:, :100])
    with pytest.raises(ValueError):
        lv.feed(encoding[:, 3:3 + RING])
    pool = syn.pool()
    slots = pool.join([encoding[0, :0]], None if y is None else [y[0]], seed=11, temperature=0.3, live=True)
    assert slots == [0] and pool.active == [0] and pool.step(10) == {}
    got, fed = [], 0
    while pool.active:
        k = min(2, pool.room(0), encoding.shape[1] - fed)
        if k:
            pool.feed(slots, [encoding[0, fed:fed + k]])
            fed += k
        elif fed == encoding.shape[1]:
            pool.close(slots)
        r = pool.step(100)
        if 0 in r:
            got.append(r[0])
    assert np.array_equal(np.concatenate(got), want[0, :, 0])


def test_resynthesizer_checks_its_halves():
    M, enc, syn, _ = _models(torch.bfloat16, 32, 0)
    with pytest.raises(TypeError):
        M.Resynthesizer(enc, enc)
    other = M.StudentSynthesizer(DIL, 1, dilation_channels=32, latent_channels=5, pool_stride=128, max_frames=RING)
    with pytest.raises(ValueError, match="pool_stride"):
        M.Resynthesizer(enc, other)
    other = M.StudentSynthesizer(DIL, 1, dilation_channels=32, latent_channels=4, pool_stride=POOL, max_frames=RING)
    with pytest.raises(ValueError, match="latent_channels"):
        M.Resynthesizer(enc, other)
    rs = M.Resynthesizer(enc, syn)
    with pytest.raises(ValueError, match="batch"):
        rs.stream(batch=3)
    with pytest.raises(ValueError, match="chunk_size"):
        rs.stream(chunk_size=CHUNK + 1)
    small = M.StudentSynthesizer(DIL, 1, dilation_channels=32, latent_channels=5, pool_stride=POOL, max_frames=4)
    with pytest.raises(ValueError, match=r"= 5 frames"):
        M.Resynthesizer(enc, small).stream()
