"""CPU tests of the streaming likelihood scorer of the conditioned mixture-of-logistics decoder (srwn_version() 117): the two
entry points declared, bound, generated and exported; their argument errors without a GPU; every refusal of the Python
classes before any device work; the room rule of the conditioning ring against brute force on a NumPy ring model; the
staging of the entry (RightShift, the two-sample carry, the first layer's conditioning bias from the ring) restated in
NumPy against the oracle; the feed / push pieces of ``score`` against brute force."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import wavenet_np as O
from tests._pkg import ROOT, sub

NEW = ["srwn_stream_mol_score_head", "srwn_mol_score_rows"]
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _lib(binding):
    L = sub("_lib")
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "sr-wavenet_amd", "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.build()
    return L.bind(binding)


def _bare(cls, **attrs):
    """An object without its device state (constructing one needs a GPU): what the checks read first."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    raw = open(os.path.join(ROOT, "include", "srwn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n
    assert "srwn_version() 117" in raw
    assert "cond_next: NULL, or all entries NULL" not in raw          # the _z form's contract takes conditioning now
    # the build holds the new head to zero spills and zero scratch: the guard matches kernel names by substring, and the
    # entry that guards the softmax head covers the kernel named mol_stream_score_head_kernel as well
    B = sub("build")
    hip = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_score.hip")).read()
    assert re.search(r"\bvoid mol_stream_score_head_kernel\(", hip)
    assert any(k in "mol_stream_score_head_kernel" for k in B.NO_SPILL["srwn_score.hip"])
    assert hip.count("void score_head_logits(") == 1                  # one device body through the logits, not a copy


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_version_and_exports(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 117
    for n in NEW:
        assert callable(getattr(lib, n))


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)

    def head(z=A, zst=2 * 64 * 32, zrows=64, L=3, w2=A, x=A, xs=64, nll=A, lo=None, ostride=64, B=2, n=40, mc=64, R=32,
             S=128, M=10, dt=7):
        # (dt = 7 by default: a call whose other arguments are all good ends at the dtype check, before any launch)
        return lib.srwn_stream_mol_score_head(z, zst, zrows, L, A, A, A, A, w2, A, x, xs, nll, lo, ostride, B, n, mc, R, S,
                                              M, dt, None)

    assert head() == E_DTYPE                       # every other check passed; logits_out may be NULL
    assert b"stream_mol_score_head" in lib.srwn_last_error()
    assert head(lo=A) == E_DTYPE
    for name in ("z", "w2", "x", "nll"):
        assert head(**{name: None}) == E_NULL, name
    assert head(R=48) == E_UNSUPPORTED
    assert head(S=192) == E_UNSUPPORTED
    assert head(n=0) == E_SHAPE
    assert head(n=65) == E_SHAPE                   # a chunk beyond max_chunk
    assert head(B=0) == E_SHAPE
    assert head(M=0) == E_SHAPE
    assert head(M=17) == E_SHAPE
    assert head(M=1) == E_DTYPE and head(M=16) == E_DTYPE
    assert head(xs=39) == E_SHAPE                  # audio rows shorter than the chunk
    assert head(zrows=32) == E_SHAPE
    assert head(ostride=39) == E_SHAPE
    assert head(zst=100) == E_SHAPE
    assert head(L=0) == E_SHAPE

    def rows(logits=A, ld=64, crows=64, x=A, xs=64, nll=A, ostride=64, B=2, n=40, M=10):
        return lib.srwn_mol_score_rows(logits, ld, crows, x, xs, nll, None, ostride, B, n, M, None)

    for name in ("logits", "x", "nll"):
        assert rows(**{name: None}) == E_NULL, name
    assert b"mol_score_rows" in lib.srwn_last_error()
    assert rows(n=0) == E_SHAPE
    assert rows(B=0) == E_SHAPE
    assert rows(M=0) == E_SHAPE
    assert rows(M=17, ld=128) == E_SHAPE
    assert rows(ld=39) == E_SHAPE                  # rows shorter than the 4M logits
    assert rows(crows=39) == E_SHAPE
    assert rows(xs=39) == E_SHAPE
    assert rows(ostride=39) == E_SHAPE


# ---- refusals, before any device work ----------------------------------------------------------------------------------
def test_weights_refuse_first():
    S = sub("scorer")
    cfg = dict(head_mode="mol", gate_mode="reference", shift_input=True, cond_channels=6, output_channels=40)
    eng = lambda **kw: SimpleNamespace(cfg=SimpleNamespace(**dict(cfg, **kw)))
    for head in ("per_timestep", "pooled", "contrastive"):
        with pytest.raises(ValueError, match="mixture-of-logistics"):
            S.MolScorerWeights.from_engine(eng(head_mode=head))
    with pytest.raises(NotImplementedError, match="wavenet"):
        S.MolScorerWeights.from_engine(eng(gate_mode="wavenet"))
    with pytest.raises(ValueError, match="RightShift"):
        S.MolScorerWeights.from_engine(eng(shift_input=False))
    with pytest.raises(NotImplementedError, match="mixtures"):
        S.MolScorerWeights.from_engine(eng(output_channels=68))
    for m in (0, 17, 64):
        with pytest.raises(NotImplementedError, match="num_mixtures"):
            S.MolScorerWeights([1, 2], 32, 128, m)
    with pytest.raises(ValueError, match="cond_channels"):
        S.MolScorerWeights([1, 2], 32, 128, 10, cond_channels=-1)
    with pytest.raises(NotImplementedError, match="streaming scorer.*built for"):
        S.MolScorerWeights([1, 2], 48, 128, 10)
    R = sub("recognizer")
    assert issubclass(S.MolScorerWeights, R.StackWeights)
    assert issubclass(S.MolStreamScorer, S._ScorerBase) and issubclass(S.StreamScorer, S._ScorerBase)
    # the softmax scorer keeps its refusals, and now says where the capability lives
    with pytest.raises(NotImplementedError, match="mixture-of-logistics.*MolStreamScorer"):
        S.ScorerWeights.check_config(SimpleNamespace(head_mode="mol"))


def test_scorer_refuses_first():
    S, St = sub("scorer"), sub("student")
    dil = [1, 2, 4, 8, 16, 32, 64, 128, 1, 2, 5]
    w = SimpleNamespace(E=6, pool=20, dil=dil)
    with pytest.raises(ValueError, match="max_chunk"):
        S.MolStreamScorer(w, max_batch=1, max_chunk=0)
    hist_max = max(sum(dil[a:b]) for a, b in S.MolStreamScorer._plan(w))
    need = St.live_min_frames(hist_max, 20)
    assert need == -(-hist_max // 20) + 1 and need > 2
    with pytest.raises(ValueError, match="max_frames %d.*at least %d" % (need - 1, need)):
        S.MolStreamScorer(w, max_batch=1, max_chunk=64, max_frames=need - 1)
    st = _bare(S.MolScoreState, B=2, _serial=1, t=40, fed=3)
    c = _bare(S.MolStreamScorer, max_batch=2, E=6, pool=20, hist_max=hist_max, max_frames=need, _state=st, _serial=1)
    assert c.available(st) == 20 and c.room(st) == need - 3
    with pytest.raises(ValueError, match="push: 21 samples"):             # beyond what the frames fed cover
        c.push(st, np.zeros((2, 21), np.float32))
    with pytest.raises(ValueError, match="streams"):
        c.push(st, np.zeros((1, 10), np.float32))
    with pytest.raises(ValueError, match="feed: %d frames" % (need - 2)):  # beyond the ring's room
        c.feed(st, np.zeros((2, need - 2, 6), np.float32))
    with pytest.raises(ValueError, match="frames must be"):
        c.feed(st, np.zeros((2, 1, 5), np.float32))
    with pytest.raises(ValueError, match="current"):                        # a stale state
        c.push(_bare(S.MolScoreState, B=2, _serial=0, t=0, fed=0), np.zeros((2, 1), np.float32))
    assert (st.t, st.fed) == (40, 3)                                        # refusals leave the state untouched
    u = _bare(S.MolStreamScorer, max_batch=2, E=0, pool=1, hist_max=0, max_frames=1, _state=st, _serial=1)
    assert u.available(st) == float("inf") and u.room(st) == 0
    with pytest.raises(ValueError, match="not conditioned"):
        u.feed(st, np.zeros((2, 1, 6), np.float32))


def test_models_refuse_first():
    M = sub("model")
    cfg = dict(head_mode="mol", gate_mode="reference", shift_input=True, cond_channels=0, filter_width=2,
               dilation_channels=32, skip_channels=128, output_channels=40)
    teacher = lambda **kw: _bare(M.WaveNetTeacher, _cfg=SimpleNamespace(**dict(cfg, **kw)), _primary=None)
    with pytest.raises(ValueError, match="mixture-of-logistics"):
        teacher(head_mode="per_timestep").mol_scorer()                       # the softmax teacher: scorer()
    with pytest.raises(NotImplementedError, match="mixtures"):
        teacher(output_channels=4 * 17).mol_scorer()
    with pytest.raises(NotImplementedError, match="wavenet"):
        teacher(gate_mode="wavenet").mol_scorer()
    with pytest.raises(NotImplementedError, match="built for"):
        teacher(skip_channels=64).mol_scorer()
    with pytest.raises(FileNotFoundError, match="config.json"):
        M.AutoEncoderScorer.from_checkpoint("/nonexistent")
    for name in ("StreamingMolScorer", "MolScorerStream", "AutoEncoderScorer", "AutoEncoderScoreStream"):
        assert isinstance(getattr(M, name), type)
    assert callable(M.WaveNetAutoEncoder.scorer)


# ---- the room rule, on a ring model ------------------------------------------------------------------------------------
def _frames_read(t, n, hists, pool):
    """Every conditioning frame a step of n rows at time t reads: the entry on the chunk's rows, each group launch on its
    halo rows back to t - hist_g as well (rows before the stream's start are the conv's padding: no frame)."""
    rows = set(range(t, t + n))
    for h in hists:
        rows |= set(range(max(t - h, 0), t + n))
    return {r // pool for r in rows}


@pytest.mark.parametrize("pool,hists,F_extra,max_chunk", [(20, [255, 8], 1, 128), (20, [255, 8], 0, 128), (7, [30, 100, 3], 2, 16),
                                                          (1, [5], 0, 4), (64, [10, 20], 0, 50), (3, [], 0, 5)])
def test_room_rule_against_brute_force(pool, hists, F_extra, max_chunk):
    S, St = sub("scorer"), sub("student")
    hist_max = max(hists, default=0)
    F = St.live_min_frames(hist_max, pool) + F_extra
    rng = np.random.default_rng(pool * 1000 + F)
    ring = np.full(F, -1, np.int64)
    fed = t = 0
    tight = 0
    for _ in range(300):
        room = St.live_room(fed, t, hist_max, pool, F)
        assert room == max(0, F - fed + max(t - hist_max, 0) // pool)
        over = fed + room - F            # the frame that one frame more than the room would overwrite
        k = int(rng.integers(0, room + 1)) if rng.random() < 0.6 else room
        for q in range(fed, fed + k):
            ring[q % F] = q
        fed += k
        avail = fed * pool - t
        if room and k == room and avail > 0 and t >= hist_max:      # ... is the oldest one the next step still reads
            assert over == (t - hist_max) // pool and over in _frames_read(t, 1, hists + [0], pool)
            tight += 1
        n_all = int(rng.integers(0, avail + 1)) if rng.random() < 0.7 else avail
        for a, n in S.cut_push(n_all, max_chunk):
            for q in _frames_read(t + a, n, hists, pool):
                assert ring[q % F] == q, (q, t + a, n, fed)                   # still resident
        t += n_all
    assert t > 3 * F * pool and tight > 0                                     # the ring wrapped, the bound was met
    assert St.live_room(fed, fed * pool, hist_max, pool, F) >= 1              # never stalls once every sample is scored


def test_score_pieces_against_brute_force():
    S, St = sub("scorer"), sub("student")
    for pool, hist_max in ((20, 255), (7, 100), (1, 5), (64, 20), (3, 0)):
        fmin = St.live_min_frames(hist_max, pool)
        with pytest.raises(ValueError):
            S.plan_score_pieces(10, pool, fmin - 1, hist_max)
        for F in (fmin, fmin + 1, fmin + 5, 3 * fmin):
            for frames in (0, 1, 2, F - 1, F, F + 1, 3 * F + 2):
                pieces = S.plan_score_pieces(frames, pool, F, hist_max)
                ring = np.full(F, -1, np.int64)
                fed = t = 0
                for k, n in pieces:
                    assert 1 <= k <= St.live_room(fed, t, hist_max, pool, F)
                    assert k == min(St.live_room(fed, t, hist_max, pool, F), frames - fed)      # greedy: as many as fit
                    for q in range(fed, fed + k):
                        ring[q % F] = q
                    fed += k
                    assert n == fed * pool - t and n >= 1
                    for q in _frames_read(t, n, [hist_max], pool):
                        assert ring[q % F] == q
                    t += n
                assert (fed, t) == (frames, frames * pool), (pool, hist_max, F, frames)


# ---- the staging is the decoder's entry ----------------------------------------------------------------------------------
def test_staging_is_the_conditioned_entry():
    """What a push stages, restated in NumPy: the chunk as it is, carry = (the sample before the chunk, the one before
    that; zeros at the start: the RightShift's and the conv's padding), the entry's row t = b + w0 a[t-2] + w1 a[t-1] plus
    the first layer's conditioning bias of frame (t0 + t) // pool, looked up in ring row frame mod max_frames of a ring
    fed by ``plan_score_pieces``.  That is the oracle's input of layer 0: conv(RightShift(audio)) + upsample(cond @ wc0 +
    bc0)."""
    S = sub("scorer")
    pool, E, F, hist_max, frames = 5, 3, 4, 12, 13
    T = frames * pool
    sp = O.init_stack_params(2, [1], 2, 8, 16, 8, cond_channels=E, bias_scale=0.1)
    audio = O.synthetic_audio(1, T, seed=5).astype(np.float64)[0]
    cond = np.random.default_rng(3).normal(size=(1, frames, E))
    h = O.dilated_causal_conv1d_bias(O.right_shift(audio[None, :, None]), sp.init_w, sp.init_b, 1)
    cb = cond @ sp.layers[0].wc + sp.layers[0].bc
    want = (h + O.resize_embedding_nearest_neighbor(cb, T))[0]
    ring = np.zeros((F, 8))
    got, carry, fed, t0 = [], np.zeros(2), 0, 0
    for k, n_all in S.plan_score_pieces(frames, pool, F, hist_max):
        for q in range(fed, fed + k):
            ring[q % F] = cb[0, q]
        fed += k
        for a, n in S.cut_push(n_all, 7):
            x = audio[t0 + a:t0 + a + n]
            for t in range(n):
                x1 = x[t - 1] if t >= 1 else carry[0]
                x0 = x[t - 2] if t >= 2 else carry[1 - t]
                got.append(sp.init_b + x0 * sp.init_w[0, 0] + x1 * sp.init_w[1, 0] + ring[((t0 + a + t) // pool) % F])
            carry = np.array([x[-1], x[-2] if n >= 2 else carry[0]])
        t0 += n_all
    assert t0 == T and F < frames                                             # the ring wrapped
    assert np.abs(np.array(got) - want).max() < 1e-14
