"""GPU tests of live autoregressive decoding (srwn_version() 112): a decoder run that is FED its encoding while it runs
-- WaveNetEngine.live_generation_state / feed, WaveNetAutoEncoder.live, the TeacherResynthesizer pipeline -- has the bits
of `generate` over the whole encoding.  Every comparison is np.array_equal on the uint32 view: there are no tolerances.

The shapes are the smallest that cross every boundary: 9 layers (an odd stack, a dilation of 5), both widths, 5 mixtures,
latent 8, pool_stride 16 and a ring of 4 frames against 11 frames = 176 samples (the ring wraps twice), batches 1 / 3 /
33 (33 crosses a ring group of 32 and both workgroup sizes of the latency body)."""
import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev

pytestmark = pytest.mark.gpu

DIL = [1, 2, 4, 8, 16, 32, 1, 2, 5]
M, LAT, POOL, RING, FRAMES = 5, 8, 16, 4, 11
T = FRAMES * POOL
WIDTHS = [(64, 256), (32, 128)]
# (dtype, SRWN_GEN16, SRWN_GEN16_NCB): bf16 on the throughput body and on both workgroup sizes of the latency body, fp32
BODIES = [(torch.bfloat16, "0", None), (torch.bfloat16, "1", "1"), (torch.bfloat16, "1", "2"), (torch.float32, "0", None)]
BODY_IDS = ["bf16-gen", "bf16-gen16-ncb1", "bf16-gen16-ncb2", "fp32-gen"]
SIZES = [7, 16, 50]


def _body(monkeypatch, body):
    monkeypatch.setenv("SRWN_GEN16", body[1])
    if body[2] is None:
        monkeypatch.delenv("SRWN_GEN16_NCB", raising=False)
    else:
        monkeypatch.setenv("SRWN_GEN16_NCB", body[2])
    return body[0]


def _u32(x):
    if isinstance(x, torch.Tensor):
        x = x.contiguous().cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint32)


_ENGINES, _REFS, _AES = {}, {}, {}


def _engine(dt, R, S, E=LAT):
    key = (dt, R, S, E)
    if key not in _ENGINES:
        EG = sub("engine")
        sp = O.init_stack_params(7, DIL, 2, R, S, 4 * M, cond_channels=E, bias_scale=0.05)
        cfg = EG.StackConfig(dilations=DIL, dilation_channels=R, skip_channels=S, output_channels=4 * M, cond_channels=E,
                             pool_stride=POOL, shift_input=True, head_mode="mol", dtype=dt)
        eng = EG.WaveNetEngine(cfg, 1, POOL, DEV)
        eng.load_oracle_params(sp)
        _ENGINES[key] = eng
    return _ENGINES[key]


def _cond(B, E=LAT):
    return dev(np.random.default_rng(B).standard_normal((B, FRAMES, E)))


def _forced(B):
    return dev(O.synthetic_audio(B, T, seed=5))


def _reference(eng, body, R, B, forced):
    """eng.generate over the whole 11-frame encoding, computed once per (body, width, batch, forced) and left unchanged."""
    key = (body, R, B, forced)
    if key not in _REFS:
        out = eng.generate(T, mode="sample", seed=13, forced=_forced(B) if forced else None, want_logits=True, batch=B,
                           cond=_cond(B))
        _REFS[key] = tuple(_u32(o) for o in out)
    return _REFS[key]


def _run_live(eng, B, cond, seed, burst, sizes, forced=None, temperature=1.0, st=None):
    """Feeds cond one frame at a time (or in bursts of `room`) as the chunks need it and steps through `sizes` (cut to what
    is available).  Returns ((audio, codes, logits), chunk sizes that ran, the state)."""
    room = sub("engine").live_decode_room
    st = st or eng.live_generation_state(B, RING, seed, temperature=temperature)
    frames, outs, ran, i = cond.shape[1], [], [], 0
    while st.t < frames * POOL:
        n = sizes[i % len(sizes)]
        while st.fed < frames and st.limit - st.t < n:
            r = room(RING, st.fed, st.t, POOL)
            if r == 0:
                break
            k = min(r, frames - st.fed) if burst else 1
            eng.feed(st, cond[:, st.fed:st.fed + k])
        n = min(n, st.limit - st.t)
        assert n >= 1, (st.t, st.fed)
        f = None if forced is None else forced[:, st.t:st.t + n]
        outs.append(eng.generate_chunk(st, n, mode="sample", forced=f, want_logits=True))
        ran.append(n)
        i += 1
        assert i < 1000
    return [torch.cat([o[j] for o in outs], dim=1) for j in range(3)], ran, st


# ---------------------------------------------------------------------------------------------------
# 1. ring = table
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("R,S", WIDTHS)
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_live_run_has_the_bits_of_the_whole_table(monkeypatch, body, R, S, B):
    dt = _body(monkeypatch, body)
    eng = _engine(dt, R, S)
    if dt == torch.bfloat16:
        assert eng.o_g16 is not None
    cond = _cond(B)
    for forced in (False, True):
        want = _reference(eng, body, R, B, forced)
        assert np.isfinite(want[0].view(np.float32)).all()
        f = _forced(B) if forced else None
        for burst in (False, True):
            got, ran, st = _run_live(eng, B, cond, 13, burst, SIZES, forced=f)
            assert st.fed == FRAMES > 2 * RING and st.t == T and set(SIZES) <= set(ran)
            for j, name in enumerate(("audio", "codes", "logits")):
                assert np.array_equal(_u32(got[j]), want[j]), (name, forced, burst)
    if B > 1:
        assert not np.array_equal(want[0][0], want[0][1])
    # the feed's rows are the one-shot table's: after the last feed the ring holds frames 8, 9, 10 and 7 (row q mod 4)
    table = eng._project_cond(cond.reshape(B * FRAMES, LAT)).view(B, FRAMES, -1)
    ring = st.cond_all.view(B, RING, -1)
    for q in range(FRAMES - RING, FRAMES):
        assert torch.equal(ring[:, q % RING], table[:, q]), q
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 2. temperature on every second stream
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 33])
@pytest.mark.parametrize("R,S", WIDTHS)
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_live_run_with_temperatures(monkeypatch, body, R, S, B):
    dt = _body(monkeypatch, body)
    eng = _engine(dt, R, S)
    cond = _cond(B)
    temps = [0.7 if u % 2 else 1.0 for u in range(B)]
    want = eng.generate(T, mode="sample", seed=21, want_logits=True, batch=B, cond=cond, temperature=temps)
    plain = eng.generate(T, mode="sample", seed=21, batch=B, cond=cond)
    assert np.array_equal(_u32(want[0])[0], _u32(plain[0])[0])         # stream 0 is at the defaults,
    assert not np.array_equal(_u32(want[0])[1], _u32(plain[0])[1])     # stream 1 is not
    got, _, st = _run_live(eng, B, cond, 21, False, [50, 7, 16], temperature=temps)
    assert st.sampling is not None
    for j in range(3):
        assert np.array_equal(_u32(got[j]), _u32(want[j])), j


# ---------------------------------------------------------------------------------------------------
# 3. the old path is untouched by a live run on the same engine
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_whole_table_paths_keep_their_bits_around_a_live_run(monkeypatch, body):
    dt = _body(monkeypatch, body)
    eng, B = _engine(dt, 64, 256), 3
    cond = _cond(B)

    def whole():
        one = eng.generate(T, mode="sample", seed=13, want_logits=True, batch=B, cond=cond)
        st = eng.generation_state(B, cond, 13)
        ch = [eng.generate_chunk(st, n, want_logits=True) for n in (50, 7, T - 57)]
        return [_u32(o) for o in one] + [_u32(torch.cat([c[j] for c in ch], dim=1)) for j in range(3)]

    before = whole()
    for j in range(3):
        assert np.array_equal(before[j], before[3 + j])
    _run_live(eng, B, cond, 99, True, SIZES)
    st = eng.live_generation_state(B, RING, 5)                         # a live run left in the middle
    eng.feed(st, cond[:, :2])
    eng.generate_chunk(st, 20)
    after = whole()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    # a whole-table state is not a live one
    ws = eng.generation_state(B, cond, 13)
    with pytest.raises(ValueError, match="live_generation_state"):
        eng.feed(ws, cond[:, :1])


# ---------------------------------------------------------------------------------------------------
# 4. the model face: starvation, prompt, conditions, pipeline
# ---------------------------------------------------------------------------------------------------
def _ae(dt, R, S, cs=0):
    key = (dt, R, S, cs)
    if key not in _AES:
        Mo = sub("model")
        ae = Mo.WaveNetAutoEncoder(input_size=T, condition_size=cs, num_mixtures=M, dilations=DIL, dilation_channels=R,
                                   skip_channels=S, latent_channels=LAT, pool_stride=POOL, learning_rate=1e-3, dtype=dt)
        x = O.synthetic_audio(2, T, seed=4)
        ae.train(x, np.ones((2, cs), np.float32) if cs else None)      # (moves the biases off their initial zeros)
        _AES[key] = ae
    return _AES[key]


def _enc(B):
    return np.random.default_rng(100 + B).standard_normal((B, FRAMES, LAT)).astype(np.float32)


@pytest.mark.parametrize("R,S", WIDTHS)
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_starved_stream_waits_and_continues(monkeypatch, body, R, S):
    dt = _body(monkeypatch, body)
    ae, B = _ae(dt, R, S), 3
    enc = _enc(B)
    want = ae.generate(enc, seed=5)
    assert want.shape == (B, T) and np.isfinite(want).all()
    lv = ae.live(B, max_frames=RING, seed=5)
    assert (lv.t, lv.fed, lv.room, lv.available) == (0, 0, RING, 0)
    with pytest.raises(ValueError, match="run past the encoding's frames"):
        lv.step(1)                                                     # nothing fed yet
    outs = []
    lv.feed(enc[:, :2])
    outs.append(lv.step(2 * POOL))                                     # exactly what is available
    assert lv.available == 0 and lv.t == 2 * POOL and lv.room == RING
    with pytest.raises(ValueError, match="run past the encoding's frames"):
        lv.step(1)
    assert lv.t == 2 * POOL
    with pytest.raises(ValueError, match="room for 4"):
        lv.feed(enc[:, 2:7])
    lv.feed(torch.as_tensor(enc[:, 2:6]).to("cuda"))                   # a device tensor, a full ring
    assert lv.room == 0 and lv.available == RING * POOL
    outs.append(lv.step(37))
    a, lg = lv.step(lv.available, return_logits=True)
    assert lg.shape == (B, RING * POOL - 37, 4 * M)
    outs.append(a)
    assert lv.available == 0
    while lv.fed < FRAMES:
        k = min(lv.room, FRAMES - lv.fed)
        lv.feed(enc[:, lv.fed:lv.fed + k])
        outs.append(lv.step(lv.available))
    got = np.concatenate(outs, axis=1)
    assert lv.t == T and np.array_equal(_u32(got), _u32(want))


@pytest.mark.parametrize("R,S", WIDTHS)
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_prompted_live_run(monkeypatch, body, R, S):
    dt = _body(monkeypatch, body)
    ae, B, P = _ae(dt, R, S), 3, 20
    enc = _enc(B)
    prompt = O.synthetic_audio(B, P, seed=9).astype(np.float32)
    want = ae.generate(enc, seed=6, prompt=prompt)
    assert want.shape == (B, T - P)
    lv = ae.live(B, max_frames=RING, seed=6, prompt_frames=enc[:, :2], prompt=prompt)
    assert (lv.t, lv.fed, lv.available, lv.room) == (P, 2, 2 * POOL - P, RING - 2 + P // POOL)
    with pytest.raises(ValueError, match="the state is at step"):
        ae._eng.dec.prime(lv._st, torch.zeros(B, 4))
    outs, i = [], 0
    while lv.t < T:
        if lv.fed < FRAMES and lv.room > 0:
            lv.feed(enc[:, lv.fed:lv.fed + 1])
        outs.append(lv.step(min(SIZES[i % 3], lv.available)))
        i += 1
    assert np.array_equal(_u32(np.concatenate(outs, axis=1)), _u32(want))


@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_conditions_are_tiled_onto_every_fed_frame(monkeypatch, body):
    dt = _body(monkeypatch, body)
    ae, B = _ae(dt, 64, 256, cs=3), 3
    enc = _enc(B)
    c = np.random.default_rng(3).standard_normal((B, 3)).astype(np.float32)
    want = ae.generate(enc, conditions=c, seed=8)
    assert not np.array_equal(_u32(want), _u32(ae.generate(enc, conditions=0 * c, seed=8)))
    lv = ae.live(B, conditions=c, max_frames=RING, seed=8)
    outs = []
    while lv.t < T:
        k = min(lv.room, FRAMES - lv.fed, 3)
        if k > 0:
            lv.feed(enc[:, lv.fed:lv.fed + k])
        outs.append(lv.step(min(50, lv.available)))
    assert np.array_equal(_u32(np.concatenate(outs, axis=1)), _u32(want))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R,S", WIDTHS)
@pytest.mark.parametrize("body", BODIES, ids=BODY_IDS)
def test_pipeline_audio_in_audio_out(monkeypatch, body, R, S, B):
    """TeacherResynthesizer.stream against ae.generate(encoder.encode(audio)): a clip of 11 frames and 5 samples more,
    longer than the ring's 4 x 16 samples, cut into pieces of 1, 16, 37 and 200 samples; finish() included."""
    dt = _body(monkeypatch, body)
    ae = _ae(dt, R, S)
    rs = ae.resynthesizer(max_batch=3, max_frames=RING)
    assert rs.lookahead == POOL + len(DIL) + 1 and rs.max_frames == RING
    audio = O.synthetic_audio(B, T + 5, seed=30 + B).astype(np.float32)
    want = ae.generate(rs.encoder.encode(audio), seed=17)
    assert want.shape == (B, T) and T > RING * POOL
    for cuts, chunk in (([1, 16, 37, 200], 160), ([200, 37, 16, 1], 7)):
        s = rs.stream(batch=B, seed=17, chunk_size=chunk)
        outs, pos, i = [], 0, 0
        while pos < audio.shape[1]:
            n = min(cuts[i % 4], audio.shape[1] - pos)
            o = s.push(audio[:, pos:pos + n])
            assert o.shape[0] == B and o.dtype == np.float32
            outs.append(o)
            pos += n
            i += 1
        assert s.received == T + 5 and s.t <= T
        outs.append(s.finish())
        got = np.concatenate(outs, axis=1)
        assert s.t == T and np.array_equal(_u32(got), _u32(want)), cuts
        with pytest.raises(ValueError, match="closed"):
            s.push(audio[:, :1])
