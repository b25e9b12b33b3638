"""CPU tests of live autoregressive decoding (srwn_version() 112): the room rule of the decoder's conditioning ring on
hand-computed cases, the refusals of the engine and model faces before any device work, and the new entry points under
both bindings with their argument errors as negative codes without a GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._pkg import ROOT, sub
from tests.test_generate_stream import A, E_NULL, E_SHAPE, _bare, _dl, _lib

LIVE = ["srwn_generate_mol_live_sampled", "srwn_generate16_mol_live_sampled"]
POOL, LAT, RING = 16, 8, 4


# ---------------------------------------------------------------------------------------------------
# the room rule
# ---------------------------------------------------------------------------------------------------
def test_live_decode_room_is_the_rule():
    room = sub("engine").live_decode_room
    # (max_frames, fed, t, pool_stride) -> frames that may be fed: max_frames - fed + t // pool_stride
    table = [((4, 0, 0, 16), 4),        # nothing fed: the whole ring
             ((4, 4, 0, 16), 0),        # a full ring at t = 0: frame 0 is still to be read
             ((4, 4, 15, 16), 0),       # ... and is read until its last sample
             ((4, 4, 16, 16), 1),       # frame 0 is behind: one row free
             ((4, 4, 40, 16), 2),       # t in mid-frame 2: frames 0 and 1 are behind, frame 2 is being read
             ((4, 4, 64, 16), 4),       # everything fed is made: the whole ring again
             ((4, 11, 8 * 16 + 3, 16), 1),   # a wrapped ring: frames 8, 9, 10 are kept, frame 7's row is free
             ((4, 11, 11 * 16, 16), 4),
             ((1, 1, 0, 16), 0), ((1, 1, 16, 16), 1),     # the smallest ring: one frame at a time
             ((32, 40, 37, 1), 29),     # pool_stride 1: every step is a frame (frames 37, 38, 39 are kept)
             ((6, 2, 1023, 512), 5)]
    for args, want in table:
        assert room(*args) == want, args
    # never negative and never more than the ring while t <= fed * pool_stride; fed frames minus made frames are kept
    for F in (1, 3, 4):
        for fed in range(0, 3 * F):
            for t in range(max(0, (fed - F) * 5), fed * 5 + 1):
                r = room(F, fed, t, 5)
                assert 0 <= r <= F and r == F - (fed - t // 5), (F, fed, t)
    for bad in ((0, 0, 0, 16), (4, -1, 0, 16), (4, 0, -1, 16), (4, 0, 0, 0), (4, 1, 17, 16)):
        with pytest.raises(ValueError, match="live_decode_room"):
            room(*bad)


# ---------------------------------------------------------------------------------------------------
# refusals before any device work
# ---------------------------------------------------------------------------------------------------
def _engine(E=LAT, mol=True, **attrs):
    """A decoder engine without its buffers (constructing one needs a GPU): what the live calls read before they refuse."""
    cfg = SimpleNamespace(pool_stride=POOL, head_mode="mol" if mol else "softmax")
    return _bare(sub("engine").WaveNetEngine, cfg=cfg, E=E, mol=mol, wavenet=False, o_gen=0, C=20, dev="cpu", **attrs)


def _state(fed=0, t=0, batch=2):
    st = sub("engine").LiveGenerationState(batch, None, None, 0, None, RING)
    st.fed, st.t, st.limit = fed, t, fed * POOL
    return st


def test_engine_feed_refuses_before_device_work():
    eng = _engine()
    st = _state(fed=3, t=20)                                     # room = 4 - 3 + 20 // 16 = 2
    with pytest.raises(ValueError, match="room for 2"):
        eng.feed(st, torch.zeros(2, 3, LAT))
    with pytest.raises(ValueError, match=r"frames must be \[2, k, 8\]"):
        eng.feed(st, torch.zeros(2, 1, LAT + 1))                 # wrong channel count
    with pytest.raises(ValueError, match="frames must be"):
        eng.feed(st, torch.zeros(3, 1, LAT))                     # wrong batch
    with pytest.raises(ValueError, match="frames must be"):
        eng.feed(st, torch.zeros(2, LAT))
    assert (st.fed, st.t, st.limit) == (3, 20, 48)               # untouched
    eng.feed(st, torch.zeros(2, 0, LAT))                         # no frame: nothing to do
    whole = sub("engine").GenerationState(2, None, None, 0)
    with pytest.raises(ValueError, match="live_generation_state"):
        eng.feed(whole, torch.zeros(2, 1, LAT))


def test_engine_step_past_the_fed_frames_and_late_prime_are_refused():
    eng = _engine()
    st = _state(fed=2, t=20)
    with pytest.raises(ValueError, match=r"run past the encoding's frames \* pool_stride = 32"):
        eng.generate_chunk(st, 13)
    with pytest.raises(ValueError, match="nsteps"):
        eng.generate_chunk(st, -1)
    with pytest.raises(ValueError, match="the state is at step 20"):
        eng.prime(st, torch.zeros(2, 5))                         # a prompt starts a run
    with pytest.raises(ValueError, match=r"exceeds frames \* pool_stride = 32"):
        eng.prime(_state(fed=2), torch.zeros(2, 33))             # longer than the frames fed
    with pytest.raises(ValueError, match="prompt must be"):
        eng.prime(_state(fed=2), torch.zeros(3, 5))
    assert st.t == 20


def test_live_state_is_for_the_conditioned_mixture_decoder():
    with pytest.raises(ValueError, match="this decoder is not conditioned"):
        _engine(E=0).live_generation_state(2, RING)
    with pytest.raises(NotImplementedError, match="conditioned softmax teacher is not built"):
        _engine(mol=False).live_generation_state(2, RING)
    with pytest.raises(ValueError, match="this decoder is not conditioned"):
        _engine(E=0, mol=False).live_generation_state(2, RING)
    with pytest.raises(NotImplementedError, match="gate_mode 'wavenet'"):
        _bare(sub("engine").WaveNetEngine, wavenet=True).live_generation_state(2, RING)
    for bad in ((0, RING), (2, 0)):
        with pytest.raises(ValueError, match="live_generation_state"):
            _engine().live_generation_state(*bad)
    with pytest.raises(ValueError, match="temperature"):
        _engine().live_generation_state(2, RING, temperature=0.0)


def _live(fed=0, t=0, batch=2, condition_size=0):
    M = sub("model")
    ae = _bare(M.WaveNetAutoEncoder, latent_channels=LAT, pool_stride=POOL, condition_size=condition_size, _eng=None)
    cond = torch.zeros(batch, condition_size) if condition_size else None
    return M.LiveDecoding(ae, _engine(E=LAT + condition_size), _state(fed, t, batch), cond, "sample")


def test_live_decoding_properties_and_refusals():
    lv = _live(fed=3, t=20)
    assert (lv.t, lv.fed, lv.room, lv.available, lv.batch_size) == (20, 3, 2, 28, 2)
    with pytest.raises(ValueError, match="room for 2"):
        lv.feed(np.zeros((2, 3, LAT), np.float32))
    with pytest.raises(ValueError, match="latent_channels=8"):
        lv.feed(np.zeros((2, 1, LAT + 3), np.float32))
    with pytest.raises(ValueError, match="latent_channels=8"):
        lv.feed(torch.zeros(3, 1, LAT))
    with pytest.raises(ValueError, match="run past the encoding's frames"):
        lv.step(29)                                              # one past `available`
    with pytest.raises(ValueError, match="run past the encoding's frames"):
        _live().step(1)                                          # nothing fed yet
    assert (lv.t, lv.fed) == (20, 3)


def test_autoencoder_live_refuses_bad_arguments_first():
    M = sub("model")
    ae = _bare(M.WaveNetAutoEncoder, latent_channels=LAT, pool_stride=POOL, condition_size=0, _eng=None)
    with pytest.raises(ValueError, match="batch 0"):
        ae.live(0)
    with pytest.raises(ValueError, match="max_frames 0"):
        ae.live(2, max_frames=0)
    with pytest.raises(ValueError, match="temperature"):
        ae.live(2, temperature=-1.0)
    with pytest.raises(ValueError, match="prompt must be"):
        ae.live(2, prompt=np.zeros((3, 5)), prompt_frames=np.zeros((2, 1, LAT)))
    with pytest.raises(ValueError, match="come together"):
        ae.live(2, prompt=np.zeros((2, 5)))
    with pytest.raises(ValueError, match="prompt_frames must be"):
        ae.live(2, max_frames=RING, prompt=np.zeros((2, 5)), prompt_frames=np.zeros((2, RING + 1, LAT)))
    with pytest.raises(ValueError, match="prompt_frames must be"):
        ae.live(2, prompt=np.zeros((2, 5)), prompt_frames=np.zeros((2, 1, LAT + 1)))
    with pytest.raises(ValueError, match=r"exceeds frames \* pool_stride = 16"):
        ae.live(2, prompt=np.zeros((2, 17)), prompt_frames=np.zeros((2, 1, LAT)))
    c = _bare(M.WaveNetAutoEncoder, latent_channels=LAT, pool_stride=POOL, condition_size=3, _eng=None)
    with pytest.raises(ValueError, match="pass conditions"):
        c.live(2)
    with pytest.raises(ValueError, match=r"conditions must be \[2, 3\]"):
        c.live(2, conditions=np.zeros((2, 4)))


def test_teacher_resynthesizer_checks_its_halves():
    M = sub("model")
    enc = _bare(M.AudioEncoder, pool_stride=POOL, latent_channels=LAT, num_layers=5, max_batch=2, max_frames=RING)
    ae = _bare(M.WaveNetAutoEncoder, pool_stride=POOL, latent_channels=LAT, condition_size=0)
    for a, b in ((None, None), (enc, None), (None, ae), (ae, enc), (enc, _bare(M.StudentSynthesizer))):
        with pytest.raises(TypeError, match="TeacherResynthesizer"):
            M.TeacherResynthesizer(a, b)
    with pytest.raises(ValueError, match="pool_stride"):
        M.TeacherResynthesizer(enc, _bare(M.WaveNetAutoEncoder, pool_stride=2 * POOL, latent_channels=LAT))
    with pytest.raises(ValueError, match="latent_channels"):
        M.TeacherResynthesizer(enc, _bare(M.WaveNetAutoEncoder, pool_stride=POOL, latent_channels=LAT + 8))
    assert sub("dropin.model").TeacherResynthesizer is M.TeacherResynthesizer
    if torch.cuda.is_available():
        rs = M.TeacherResynthesizer(enc, ae)
        assert rs.lookahead == POOL + 5 + 1 and rs.max_frames == RING and rs.pool_stride == POOL
        with pytest.raises(ValueError, match="batch 3"):
            rs.stream(batch=3)
        with pytest.raises(ValueError, match="chunk_size"):
            rs.stream(batch=1, chunk_size=0)
    else:
        with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
            M.TeacherResynthesizer(enc, ae)


# ---------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------
def test_live_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for n in LIVE + ["srwn_cond_ring_scatter"]:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n
    for base in ("srwn_generate", "srwn_generate16"):      # the arguments of the *_mol_resume_sampled twins
        assert L.SIGNATURES[base + "_mol_live_sampled"] == L.SIGNATURES[base + "_mol_resume_sampled"]


def _live_args(which, cond=A, cond_frames=RING, pool=POOL, cond_ld=2 * 64, M=5, B=2, nsteps=4, t0=0, carry=A):
    d = _dl([1, 2])
    shared = [A] * 7 + [A, A, A, None, None, d, 2, B, nsteps, nsteps, 64, 256]
    if which == "srwn_generate_mol_live_sampled":
        return [A] * 4 + shared + [2, M, cond, cond_frames, pool, cond_ld, 1, 0, 1, None, t0, carry, None]
    return [A] * 3 + shared + [M, cond, cond_frames, pool, cond_ld, 1, 0, None, t0, carry, None]


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
@pytest.mark.parametrize("which", LIVE)
def test_live_argument_errors_do_not_need_a_gpu(binding, which):
    lib = _lib(binding)
    assert lib.srwn_version() >= 112
    f = getattr(lib, which)
    assert f(*_live_args(which, cond=None)) == E_NULL == -3          # the ring is required
    msg = lib.srwn_last_error()
    assert msg and b"live" in msg
    assert f(*_live_args(which, cond_frames=0)) == E_SHAPE
    assert f(*_live_args(which, cond_frames=-2)) == E_SHAPE
    assert f(*_live_args(which, pool=0)) == E_SHAPE
    assert f(*_live_args(which, cond_ld=2 * 64 - 4)) == E_SHAPE       # narrower than nlayers * R
    assert f(*_live_args(which, M=0)) == E_SHAPE and f(*_live_args(which, M=17)) == E_SHAPE
    assert f(*_live_args(which, cond=None, B=0)) == E_NULL            # argument errors come before "nothing to do"
    assert f(*_live_args(which, t0=5, carry=None)) == E_NULL          # then the twins' checks
    assert f(*_live_args(which, t0=-1)) == E_SHAPE
    assert f(*_live_args(which, B=0)) == 0 and f(*_live_args(which, nsteps=0)) == 0
    if which.startswith("srwn_generate16"):
        assert f(*_live_args(which, cond_ld=2 * 64 + 2)) == E_SHAPE   # the latency body reads the rows in 8-byte vectors


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_cond_scatter_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    BF16, F32 = 1, 0

    def sc(rows=A, rows_ld=128, table=A, cond_ld=128, B=2, k=2, first=0, frames=RING, width=128, dtype=BF16):
        return lib.srwn_cond_ring_scatter(rows, rows_ld, table, cond_ld, B, k, first, frames, width, dtype, None)

    assert sc(B=0) == 0 and sc(k=0) == 0                              # nothing to do: no launch
    assert sc(rows=None) == E_NULL and sc(table=None) == E_NULL
    assert sc(dtype=7) == -1
    assert sc(k=RING + 1) == E_SHAPE                                  # more frames at once than the ring holds
    assert sc(frames=0) == E_SHAPE and sc(first=-1) == E_SHAPE and sc(B=-1) == E_SHAPE
    assert sc(width=132) == E_SHAPE                                   # not a whole number of 16-byte vectors (bf16: 8)
    assert sc(dtype=F32, width=126) == E_SHAPE
    assert sc(rows_ld=120) == E_SHAPE and sc(cond_ld=120) == E_SHAPE  # narrower than the row
    assert sc(rows_ld=132) == E_SHAPE and sc(rows=A + 2) == E_SHAPE and sc(table=A + 8) == E_SHAPE
    msg = lib.srwn_last_error()
    assert msg and b"cond_ring_scatter" in msg
