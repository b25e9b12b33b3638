"""CPU tests of live synthesis (srwn_version() 110): the room rule of the conditioning ring against a brute-force
statement of it; the ring scheme restated in NumPy on the fp64 oracle, with every overwritten frame poisoned; the new
entry point's declaration and argument errors through both bindings; no CPU fallback for the live faces."""
import os
import re

import numpy as np
import pytest

from oracle import wavenet_np as O
from tests._pkg import ROOT, sub
from tests.test_student_stream import _lib, plan_np

E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take
DIL = [1, 2, 4, 8, 16, 32, 64, 128] * 2
POOL, HIST = 64, 224


# ----------------------------------------------------------------------------------------------------------------
# 1. the room rule
# ----------------------------------------------------------------------------------------------------------------
def _room_brute(fed, t, hist_max, pool, capacity):
    """Frame f lives in row f mod capacity.  A chunk at t reads frames from max(t - hist_max, 0) // pool on.  Feeding
    frame q overwrites frame q - capacity: allowed while that frame is older than the oldest one still read."""
    oldest = max(t - hist_max, 0) // pool
    k = 0
    while k < capacity and (fed + k - capacity < 0 or fed + k - capacity < oldest):
        k += 1
    return k


def test_live_room_is_the_rule():
    S = sub("student")
    seen = set()
    for capacity in (1, 4, 5, 6, 8):
        for hist, pool in ((HIST, POOL), (31, 64), (992, 512), (0, 7)):
            for fed in range(0, 3 * capacity + 3):
                for t in sorted({0, 1, hist - 1, hist, hist + 1, fed * pool - 1, fed * pool, (fed * pool) // 2,
                                 hist + pool - 1, hist + pool}):
                    if not 0 <= t <= fed * pool:
                        continue
                    got = S.live_room(fed, t, hist, pool, capacity)
                    assert got == _room_brute(fed, t, hist, pool, capacity), (fed, t, hist, pool, capacity)
                    assert 0 <= got <= capacity
                    seen.add((t < hist, fed == 0, got == 0, got == capacity))
    assert {(True, True, False, True), (True, False, True, False), (False, False, True, False)} <= seen
    assert S.live_room(0, 0, HIST, POOL, 6) == 6                     # nothing fed: the whole ring
    assert S.live_room(6, 100, HIST, POOL, 6) == 0                   # a full ring, t < hist_max: frame 0 is still read
    assert S.live_room(6, 224 + 63, HIST, POOL, 6) == 0 and S.live_room(6, 224 + 64, HIST, POOL, 6) == 1
    assert S.live_min_frames(HIST, POOL) == 5 and S.live_min_frames(256, 64) == 5 and S.live_min_frames(31, 64) == 2


def _stalls(capacity, k, hist=HIST, pool=POOL, frames=200):
    """Feeds k frames whenever there is room for k and makes every sample that can be made; True when it gets stuck."""
    S = sub("student")
    fed = t = 0
    while fed < frames:
        if S.live_room(fed, t, hist, pool, capacity) >= k:
            fed += k
        elif fed * pool == t:
            return True
        t = fed * pool
    return False


@pytest.mark.parametrize("k", [1, 2, 3])
def test_no_stall_bound(k):
    need = -(-HIST // POOL) + k                                      # ceil(hist_max / pool) + k: 5, 6, 7
    assert need == 4 + k
    assert not _stalls(need, k) and not _stalls(need + 3, k)
    assert _stalls(need - 1, k)                                      # 4 for k = 1, 5 for k = 2
    for cap in range(1, need - 1):
        assert _stalls(cap, k)


# ----------------------------------------------------------------------------------------------------------------
# 2. the ring scheme on the fp64 oracle: the chunk scheme of tests/test_student_stream.py with the frames in a ring
# ----------------------------------------------------------------------------------------------------------------
class _Ring:
    """[B, capacity, E] of frames; `fed` frames written so far.  A lookup of a frame that is not (or no longer) in its
    row returns NaN: an overwritten frame is poisoned for whoever still reads it."""

    def __init__(self, B, capacity, E):
        self.cap, self.fed = capacity, 0
        self.rows = np.full((B, capacity, E), np.nan)
        self.held = np.full(capacity, -1)      # which frame a row holds

    def feed(self, frames):
        for j in range(frames.shape[1]):
            self.rows[:, (self.fed + j) % self.cap] = frames[:, j]
            self.held[(self.fed + j) % self.cap] = self.fed + j
        self.fed += frames.shape[1]

    def lookup(self, frames):
        # no lookup touches a frame outside [fed - capacity, fed)
        assert frames.min() >= max(self.fed - self.cap, 0) and frames.max() < self.fed, (frames.min(), frames.max(), self.fed)
        out = self.rows[:, frames % self.cap].copy()
        out[:, self.held[frames % self.cap] != frames] = np.nan
        return out


def _group_fwd_ring(p, l0, l1, h, ring, pool, t_origin):
    tabs = np.arange(h.shape[1]) + t_origin
    live = tabs >= 0
    for l in range(l0, l1):
        lp = p.layers[l]
        cb = np.zeros(h.shape[:2] + (lp.wc.shape[1],))
        cb[:, live] = ring.lookup(tabs[live] // pool) @ lp.wc + lp.bc
        h = h + cb
        h[:, ~live] = 0.0
        h, _s, _ = O.residual_dilation_layer(h, lp, p.dilations[l], "reference")
    return h


class _Flow:
    def __init__(self, p, groups, B):
        R = p.init_w.shape[-1]
        self.p, self.groups = p, groups
        self.hrows = [sum(p.dilations[l0:l1]) for l0, l1 in groups]
        self.hist = [np.zeros((B, H, R)) for H in self.hrows]
        self.carry = np.zeros((B, 2))

    def chunk(self, x, ring, pool, t0):
        p, n = self.p, x.shape[1]
        xx = np.concatenate([self.carry, x], 1)
        h = xx[:, 0:n, None] * p.init_w[0, 0][None, None, :] + xx[:, 1:n + 1, None] * p.init_w[1, 0][None, None, :] + p.init_b
        self.carry = xx[:, -2:]
        for gi, (l0, l1) in enumerate(self.groups):
            buf = np.concatenate([self.hist[gi], h], 1)
            self.hist[gi] = buf[:, buf.shape[1] - self.hrows[gi]:]
            h = _group_fwd_ring(p, l0, l1, buf, ring, pool, t0 - self.hrows[gi])[:, self.hrows[gi]:]
        prm = np.maximum(h, 0) @ p.head_w2 + p.head_b2
        return x * np.exp(prm[..., 0]) + prm[..., 1]


T_SCHEME = 1536
# wanted chunk sizes (cut to what the fed frames allow): 1, hist -1/0/+1 of both group kinds, frame boundaries, long ones
WANTED = [[1, 1, 7, 30, 31, 32, 64, 128, 223, 224, 225, 63, 65, 257], [160], [37, 1, 64], [257, 31, 1]]
_CASE = {}


def _case():
    if not _CASE:
        rng = np.random.default_rng(0)
        B, R, E = 2, 8, 5
        flows = [O.init_flow_params(11 + i, DIL, 2, R, 16, E, bias_scale=0.1) for i in range(2)]
        noise = rng.logistic(0, 1, (B, T_SCHEME)); cond = rng.standard_normal((B, T_SCHEME // POOL, E))
        _CASE.update(flows=flows, noise=noise, cond=cond, ref=O.student_forward(flows, noise, cond, POOL), B=B, E=E)
    return _CASE


@pytest.mark.parametrize("wanted", range(len(WANTED)))
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("capacity", [5, 6, 8])
def test_ring_scheme_equals_one_pass(capacity, k, wanted):
    S = sub("student")
    c = _case()
    groups = plan_np(DIL)
    assert [sum(DIL[a:b]) for a, b in groups] == [31, HIST, 31, HIST]
    frames = T_SCHEME // POOL
    ring = _Ring(c["B"], capacity, c["E"])
    flows = [_Flow(p, groups, c["B"]) for p in c["flows"]]
    sizes, outs, t, i = WANTED[wanted], [], 0, 0
    while t < T_SCHEME:
        n = sizes[i % len(sizes)]
        while ring.fed < frames and ring.fed * POOL - t < n:
            room = S.live_room(ring.fed, t, HIST, POOL, capacity)
            if room == 0:
                break
            m = min(k, room, frames - ring.fed)
            ring.feed(c["cond"][:, ring.fed:ring.fed + m])
        n = min(n, ring.fed * POOL - t)
        assert n >= 1, "the rule lets every run with capacity >= ceil(hist / pool) + 1 finish"
        x = c["noise"][:, t:t + n]
        for f in flows:
            x = f.chunk(x, ring, POOL, t)
        outs.append(x)
        t += n
        i += 1
    assert ring.fed == frames > 2 * capacity
    x = np.concatenate(outs, 1)
    assert np.isfinite(x).all()
    assert np.abs(x - c["ref"]["x_last"]).max() <= 1e-12
    assert np.abs(np.clip(x, -1, 1) - c["ref"]["out"]).max() <= 1e-12


def test_a_feed_past_the_room_is_what_the_poison_catches():
    """The scheme's own check: one frame more than the rule allows overwrites a frame a later chunk reads."""
    c = _case()
    groups = plan_np(DIL)
    ring = _Ring(c["B"], 5, c["E"])
    ring.feed(c["cond"][:, :5])
    flows = [_Flow(p, groups, c["B"]) for p in c["flows"][:1]]
    x = flows[0].chunk(c["noise"][:, :280], ring, POOL, 0)
    assert np.isfinite(x).all()
    assert sub("student").live_room(5, 280, HIST, POOL, 5) == 0      # (280 - 224) // 64 = 0: frame 0 is still read
    ring.feed(c["cond"][:, 5:6])                                     # ... and gone now
    with pytest.raises(AssertionError):
        flows[0].chunk(c["noise"][:, 280:300], ring, POOL, 280)


# ----------------------------------------------------------------------------------------------------------------
# 3. declaration, argument errors, no CPU fallback
# ----------------------------------------------------------------------------------------------------------------
def test_ring_feed_is_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    n = "srwn_cond_ring_feed"
    assert re.search(r"\b%s\s*\(" % n, hdr)
    assert n in L.SIGNATURES and len(L.SIGNATURES[n][1]) == 18
    assert '"%s"' % n in src
    assert _lib("ctypes").srwn_version() >= 110


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_ring_feed_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 110
    BF16 = 1

    def feed(x=A, xrs=16, xsr=6, cin=16, wpack=A, bias=A, table=A, L=16, R=64, frames=6, capacity=4, streams=A, first=A,
             counts=A, n=2, max_k=3, dtype=BF16):
        return lib.srwn_cond_ring_feed(x, xrs, xsr, cin, wpack, bias, table, L, R, frames, capacity, streams, first, counts, n,
                                       max_k, dtype, None)

    for name in ("x", "wpack", "bias", "table", "streams", "first", "counts"):
        assert feed(**{name: None}) == E_NULL, name
    assert b"null" in lib.srwn_last_error()
    assert feed(frames=0) == E_SHAPE                                 # cond_frames < 1
    assert feed(max_k=7) == E_SHAPE                                  # k > cond_frames
    assert b"ring of 6" in lib.srwn_last_error()
    assert feed(n=5) == E_SHAPE and feed(capacity=0) == E_SHAPE     # streams outside the table
    assert b"table holds" in lib.srwn_last_error()
    assert feed(n=-1) == E_SHAPE and feed(max_k=-1) == E_SHAPE
    assert feed(cin=8) == E_SHAPE and feed(xrs=8) == E_SHAPE and feed(xsr=2) == E_SHAPE and feed(L=0) == E_SHAPE
    assert feed(R=48) == E_UNSUPPORTED
    assert feed(dtype=9) == E_DTYPE
    assert feed(n=0) == 0 and feed(max_k=0) == 0                     # nothing to do: no launch


def test_no_cpu_fallback_for_the_live_faces():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    M = sub("model")
    with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
        M.Resynthesizer(None, None)
    with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
        M.StudentSynthesizer.live(None, 1)
    with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
        M.SynthesisPool.join(None, None, live=True)
