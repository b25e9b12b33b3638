"""GPU tests of resynthesis pools (srwn_version() 111; model.Resynthesizer.pool): independent callers on one encoder and one
synthesizer -- ragged audio, streams that join and leave while the batch runs, a conditioning ring smaller than the
frames that are due -- each receive ``synthesizer.synthesize(encoder.encode(audio), ...)`` of their audio alone, compared
with np.array_equal.  Shapes and models are those of test_gpu_student_live's pipeline test."""
import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests.test_gpu_student_live import POOL, _models

pytestmark = pytest.mark.gpu

LENGTHS = [1600, 420, 900]
SEEDS, TEMPS = [11, 5, 23], [0.3, 0.25, 0.35]
SIZES = [1, 63, 64, 65, 300]
L_ENC = 4


def _drive(rp, clips, conds, one_piece):
    """Streams 0 and 1 join at once, stream 2 when stream 1 has freed its slot.  Returns ({stream: samples}, steps in which
    a slot emitted fewer frames than were due)."""
    cs = lambda i: None if conds is None else conds[i]
    slot_of = dict(zip((0, 1), rp.join(cs(slice(0, 2)), seed=SEEDS[:2], temperature=TEMPS[:2], n=2)))
    assert slot_of == {0: 0, 1: 1} and rp.active == [0, 1] and rp.free == []
    with pytest.raises(ValueError, match="free slots"):
        rp.join(cs(slice(2, 3)))
    pushed, got, finished, held, step = [0, 0, 0], {0: [], 1: [], 2: []}, set(), 0, 0
    enc = rp._enc
    while rp.active or 2 not in slot_of:
        if 2 not in slot_of and slot_of[1] not in rp.active:
            slot_of[2], = rp.join(cs(slice(2, 3)), seed=[SEEDS[2]], temperature=[TEMPS[2]])
            assert slot_of[2] == slot_of[1] and rp.received[slot_of[2]] == 0 and rp.t[slot_of[2]] == 0
        holder = {u: i for i, u in slot_of.items() if u in rp.active and not (i == 1 and 2 in slot_of)}
        us, xs = [], []
        for u, i in sorted(holder.items()):
            left = len(clips[i]) - pushed[i]
            if i in finished:
                continue
            k = left if (one_piece and i == 0) else SIZES[(step + 2 * i) % len(SIZES)]
            k = min(k, left, rp.audio_room(u))
            us.append(u); xs.append(clips[i][pushed[i]:pushed[i] + k])
            pushed[i] += k
        if us:
            rp.push(us, xs)
        fin = [u for u, i in holder.items() if pushed[i] == len(clips[i]) and i not in finished]
        if fin:
            rp.finish(fin)
            finished |= {holder[u] for u in fin}
        due = {u: (enc.received[u] // POOL if enc._final[u] else max(0, (enc.received[u] - L_ENC - 1) // POOL)) - enc.emitted[u]
               for u in holder}
        before = enc.emitted
        out = rp.step()
        held += sum(enc.emitted[u] - before[u] < due[u] for u in holder)
        for u, y in out.items():
            assert y.dtype == np.float32 and y.ndim == 1 and 1 <= len(y) <= rp._chunk
            got[holder[u]].append(y)
        step += 1
        assert step < 4000
    assert rp.step() == {} and rp.active == [] and rp.free == [0, 1]
    return got, held


@pytest.mark.parametrize("dt,R,cs", [(torch.bfloat16, 64, 3), (torch.float32, 32, 0), (torch.bfloat16, 32, 0)],
                         ids=["bf16-R64-cond3", "fp32-R32", "bf16-R32"])
def test_a_caller_receives_what_it_would_receive_alone(dt, R, cs):
    M, enc, syn, whole = _models(dt, R, cs)
    audio = O.synthetic_audio(3, LENGTHS[0], seed=3).astype(np.float32)
    clips = [audio[i, :T].copy() for i, T in enumerate(LENGTHS)]
    conds = None if cs == 0 else np.random.default_rng(1).standard_normal((3, cs)).astype(np.float32)
    want = []
    for i, c in enumerate(clips):
        e = enc.encode(c.reshape(1, -1))
        assert e.shape == (1, LENGTHS[i] // POOL, 5)
        w = whole.synthesize(e, None if conds is None else conds[i:i + 1], seed=SEEDS[i], temperature=TEMPS[i])
        assert w.shape == (1, (LENGTHS[i] // POOL) * POOL, 1) and (np.abs(w) < 1).mean() > 0.5
        want.append(w[0, :, 0])
    assert not np.array_equal(want[0][:300], want[1][:300])
    rs = M.Resynthesizer(enc, syn)
    for chunk, one_piece in ((160, True), (37, False), (160, False)):
        rp = rs.pool(chunk_size=chunk, audio_ring=LENGTHS[0] if one_piece else None)
        assert rp.capacity == 2 and rp.step() == {}
        got, held = _drive(rp, clips, conds, one_piece)
        for i in range(3):
            g = np.concatenate(got[i])
            assert g.shape == want[i].shape, (chunk, one_piece, i)
            assert np.array_equal(g, want[i]), (chunk, one_piece, i, np.abs(g - want[i]).max())
        if one_piece:       # 25 frames due at once, a conditioning ring of 6: the frames held back stayed audio
            assert held > 0
    torch.cuda.synchronize()


def test_room_refusal_and_leaving_midway():
    M, enc, syn, whole = _models(torch.bfloat16, 32, 0)
    clip = O.synthetic_audio(1, 900, seed=5).astype(np.float32)[0]
    want = whole.synthesize(enc.encode(clip.reshape(1, -1)), seed=4, temperature=0.3)[0, :, 0]
    rp = M.Resynthesizer(enc, syn).pool(chunk_size=100)
    with pytest.raises(ValueError, match="chunk_size"):
        M.Resynthesizer(enc, syn).pool(chunk_size=301)
    a, b = rp.join(seed=[4, 9], temperature=0.3, n=2)
    room = rp.audio_room(a)
    assert room == 8 * POOL + L_ENC + 1 + POOL and rp.received.tolist() == [0, 0]
    with pytest.raises(ValueError, match="room for %d" % room):
        rp.push([a, b], [clip[:room + 1], clip[:10]])
    assert rp.received.tolist() == [0, 0] and rp.audio_room(a) == room and rp.step() == {}      # nothing changed
    rp.push([a, b], [clip[:400], clip[:400]])
    got = [rp.step()[a]]
    assert rp.t[a] == 100 == rp.t[b] and rp.received.tolist() == [400, 400]
    rp.leave(b)                                                   # midway: both halves are free again
    assert rp.active == [a] and rp.free == [b] and rp._enc.free == [b] and rp._syn.free == [b]
    with pytest.raises(ValueError, match="do not all hold a stream"):
        rp.push(b, clip[:1])
    c, = rp.join(seed=4, temperature=0.3)                         # the slot that was left, from sample 0: the same stream again
    assert c == b and rp.received[c] == 0 and rp.t[c] == 0
    rp.push([a, c], [clip[400:], clip[:500]])
    rp.finish(a)
    again = []
    for _ in range(3):
        out = rp.step()
        got.append(out[a]); again.append(out[c])
    rp.push(c, clip[500:])
    rp.finish(c)
    while rp.active:
        out = rp.step()
        if a in out:
            got.append(out[a])
        if c in out:
            again.append(out[c])
    assert np.array_equal(np.concatenate(got), want) and np.array_equal(np.concatenate(again), want)
    assert rp.step() == {} and rp.free == [0, 1] and rp._enc.free == [0, 1] and rp._syn.free == [0, 1]
    torch.cuda.synchronize()
