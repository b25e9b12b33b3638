"""GPU tests of encoder pools (srwn_version() 111; encoder.EncoderPool, model.AudioEncoder.pool): a stream in a slot of a
pool -- joined late, fed ragged audio, beside streams at other clocks, in a slot another stream left -- has the bits of
``FrameEncoder.encode`` of its audio alone, on the three paths of test_gpu_encoder_stream.  Everything is compared with
torch.equal; the one oracle comparison holds the pool to the bounds ``encode`` is held to."""
import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_encoder_stream import (ENC_STREAM_ORACLE_TOL, F32_TOL, LAT, PATHS, _clip, _encoder, _note, _params,
                                           rel_err)

pytestmark = pytest.mark.gpu

CAP, MAX_FRAMES = 5, 13                                  # 65 rows: max_rows = 64 fits
_ORACLE = {}


def _drive(pool, clips, P, L, limit_one, leaver):
    """Streams 0, 1 and the leaver join at step 0, stream 2 at step 2, stream 3 at step 5 (into the slot the leaver left at
    step 3, named), stream 4 into slot 0 once the longest clip has left it.  Push sizes cycle with a phase per stream, cut to what
    is left and to the slot's room.  Returns ({stream: frames}, the leaver's frames, steps)."""
    sizes = [0, 1, 7, P, P + 1, 3 * P - 5]
    join_at = {0: 0, 1: 0, "leaver": 0, 2: 2, 3: 5}
    slot_of, pushed, got, step = {}, {}, {}, 0
    audio = dict(enumerate(clips), leaver=leaver)
    left_slot = None
    while len(slot_of) < 6 or pool.active:
        for name, at in join_at.items():
            if name not in slot_of and step >= at:
                slot_of[name], = pool.join() if name != 3 else pool.join(slots=[left_slot])      # the slot that was left
                pushed[name], got[name] = 0, []
                assert pool.received[slot_of[name]] == 0 and pool.emitted[slot_of[name]] == 0
        if 4 not in slot_of and 0 in slot_of and slot_of[0] not in pool.active:
            slot_of[4], = pool.join(slots=[slot_of[0]])              # the slot that held the longest clip, by name
            pushed[4], got[4] = 0, []
        if step == 3:
            assert pool.emitted[slot_of["leaver"]] >= 1
            left_slot = slot_of["leaver"]
            pool.leave(left_slot)
            assert left_slot in pool.free
        holder = {u: n for n, u in slot_of.items() if u in pool.active and not (n == "leaver" and step >= 3)
                  and not (n == 0 and 4 in slot_of)}
        us, xs = [], []
        for u, n in sorted(holder.items(), key=lambda kv: kv[0]):
            x = audio[n]
            if pushed[n] == len(x):
                continue
            phase = (list(audio).index(n) + step) % len(sizes)
            k = min(sizes[phase], len(x) - pushed[n], pool.audio_room(u))
            us.append(u); xs.append(x[pushed[n]:pushed[n] + k])
            pushed[n] += k
        if us:
            pool.push(us, xs)
        fin = [u for u, n in holder.items() if pushed[n] == len(audio[n]) and not pool._final[u]]
        if fin:
            pool.finish(fin)
        before = pool.emitted
        out = pool.step({u: 1 for u in range(CAP)} if limit_one else None)
        for u, fr in out.items():
            assert fr.dtype == torch.float32 and fr.shape[1] == LAT and fr.shape[0] == pool.emitted[u] - before[u] >= 1
            assert not limit_one or fr.shape[0] == 1
            got[holder[u]].append(fr)
        for u in pool.active:
            assert pool.received[u] - pool.emitted[u] * P <= pool.audio_ring
        step += 1
        assert step < 3000
    return got, step


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("L,P", [(5, 25), (30, 128)])
@pytest.mark.parametrize("max_rows,min_ring", [(2, True), (64, False)], ids=["rows2-minring", "rows64-defaultring"])
def test_a_slot_has_the_bits_of_the_clip_alone(monkeypatch, path, L, P, max_rows, min_ring):
    fe = _encoder(monkeypatch, path, L, P, max_batch=CAP, max_frames=MAX_FRAMES)
    lengths = [6 * P + 50, P - 1, 3 * P, 3 * P + 7, 2 * P + L + 1]      # slot 0 holds the longest; stream 4 reuses it
    clips = [_clip(1, T, 40 + i)[0] for i, T in enumerate(lengths)]
    leaver = _clip(1, 5 * P, 77)[0]
    want = [fe.encode(torch.as_tensor(c.reshape(1, -1)))[0] for c in clips]
    want_leaver = fe.encode(torch.as_tensor(leaver.reshape(1, -1)))[0]
    for limit_one in (False, True):
        pool = fe.pool(audio_ring=P + L + 1 if min_ring else None, max_rows=max_rows)
        assert pool.capacity == CAP and pool.free == list(range(CAP))
        assert pool.audio_ring == (P + L + 1 if min_ring else MAX_FRAMES * P + L + 1 + P)
        assert pool.step() == {}
        got, steps = _drive(pool, clips, P, L, limit_one, leaver)
        for i, w in enumerate(want):
            g = torch.cat(got[i], 0) if got[i] else torch.zeros((0, LAT), device="cuda")
            assert g.shape == w.shape == (lengths[i] // P, LAT), (i, limit_one)
            assert torch.equal(g, w), (i, limit_one, (g - w).abs().max().item())
        g = torch.cat(got["leaver"], 0)
        assert 1 <= g.shape[0] < 5 and torch.equal(g, want_leaver[:g.shape[0]])
        assert pool.active == [] and pool.step() == {}
    if (L, P) == (30, 128) and max_rows == 64:                          # the pool equals encode; encode is held to these
        if "ref" not in _ORACLE:
            _ORACLE["ref"] = O.encoder_forward(_params(L), clips[3][None].astype(np.float64), P)[0]
        e = rel_err(torch.cat(got[3], 0).cpu().numpy(), _ORACLE["ref"])
        _note("%s pool vs oracle L=30 P=128" % path[0], e)
        assert e < (F32_TOL if path[1] == torch.float32 else ENC_STREAM_ORACLE_TOL), e
    torch.cuda.synchronize()


def test_list_kernel_skips_a_bad_item(monkeypatch):
    """One item names stream = capacity: its row of means is zero and its neighbours have the bits of a one-frame
    srwn_nc_encode_frames call on the same window -- one that wraps the ring, and one at the end of a clip."""
    L, P, cap, ring_len = 30, 128, 3, 200
    W = P + L + 1
    fe = _encoder(monkeypatch, PATHS[0], L, P, max_batch=cap, max_frames=2)
    lib, K = sub("_lib"), sub("kernels")
    w, v = fe.w, fe.w.view
    ring = torch.as_tensor(_clip(cap, ring_len, 3)).cuda()
    items = [(0, 17, W), (cap, 0, W), (1, ring_len - 40, P + 3), (2, ring_len - 1, W), (-1, 0, W), (0, ring_len, W),
             (0, 0, P - 1), (0, 0, W + 1)]
    n = len(items)
    table = torch.tensor([[u, c, k, 0] for u, c, k in items], dtype=torch.int32, device="cuda")
    parts = torch.zeros(int(lib.load().srwn_nc_encode_list_partials(n, P, L)), dtype=torch.float32, device="cuda")
    means = torch.ones((L, n, 128), dtype=torch.bfloat16, device="cuda")
    chain = (v("nc_w").data_ptr(), v("nc_b").data_ptr(), w.wptr(w.o_nc_wr_p), v("nc_br").data_ptr(), w.wptr(w.o_conv[0]),
             w.layer_stride, w.wptr(w.o_wr_p[0]), w.layer_stride, v("EB").data_ptr(), v("EBR").data_ptr())
    lib.call("srwn_nc_encode_frame_list", ring.data_ptr(), ring_len, cap, table.data_ptr(), n, *chain, parts.data_ptr(),
             means.data_ptr(), P, L, 128, 2, K.abi_dtype(w.dt), K._stream())
    torch.cuda.synchronize()
    for i, (u, c, k) in enumerate(items):
        if i in (0, 2, 3):
            x = torch.zeros((1, W), dtype=torch.float32, device="cuda")
            x[0, :k] = ring[u, (c + torch.arange(k, device="cuda")) % ring_len]
            p1 = torch.zeros(int(lib.load().srwn_nc_encode_partials(1, 1, P, L)), dtype=torch.float32, device="cuda")
            m1 = torch.ones((L, 1, 128), dtype=torch.bfloat16, device="cuda")
            lib.call("srwn_nc_encode_frames", x.data_ptr(), W, *chain, p1.data_ptr(), m1.data_ptr(), 1, 1, P, k, L, 128, 2,
                     K.abi_dtype(w.dt), K._stream())
            assert torch.equal(means[:, i], m1[:, 0]), i
            assert means[:, i].float().abs().max() > 0
        else:
            assert torch.equal(means[:, i], torch.zeros_like(means[:, i])), i      # skipped: zeros, not what was there


@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
def test_model_face(monkeypatch, path):
    M = sub("model")
    dt = path[1]
    monkeypatch.setenv("SRWN_ENC_FUSED", path[2])
    dil = [1, 2, 4, 8]
    B, T, pool_stride, lat = 2, 1024, 64, 8
    ae = M.WaveNetAutoEncoder(input_size=T, condition_size=0, num_mixtures=5, dilations=dil, latent_channels=lat,
                              skip_channels=128, pool_stride=pool_stride, learning_rate=1e-3, dtype=dt)
    x = O.synthetic_audio(B, T, seed=4)
    ae.train(x)
    enc = ae.encoder(max_batch=3, max_frames=8)
    assert enc._eng.fused == (path[0] == "fused")
    want = enc.encode(x)
    pool = enc.pool()
    assert pool.capacity == 3 and pool.join(2) == [0, 1] and pool.active == [0, 1] and pool.free == [2]
    got, t = {0: [], 1: []}, [0, 0]
    cuts = ([300, 1, 200, 523], [0, 65, 500, 459])
    for j in range(4):
        pool.push([0, 1], [x[i, t[i]:t[i] + cuts[i][j]] for i in range(2)])
        t = [t[i] + cuts[i][j] for i in range(2)]
        assert pool.received.tolist()[:2] == t
        if j == 3:
            pool.finish([0, 1])
        for u, fr in pool.step().items():
            assert isinstance(fr, np.ndarray) and fr.dtype == np.float32 and fr.shape[1] == lat
            got[u].append(fr)
    assert pool.active == [] and pool.emitted.tolist()[:2] == [T // pool_stride] * 2
    for i in range(2):
        assert np.array_equal(np.concatenate(got[i], 0), want[i]), i
    with pytest.raises(ValueError, match="holds no stream"):
        pool.push(0, x[0, :5])
