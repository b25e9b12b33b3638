"""CPU tests of student synthesis pools (srwn_version() 108): the slot scheme restated in NumPy on the fp64 oracle (every
slot at a time origin of its own); the new entry points' declarations, the slot table's layout and the argument errors
through both bindings; no CPU fallback for ``SynthPool`` / ``StudentSynthesizer.pool``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import wavenet_np as O
from tests._pkg import ROOT, sub
from tests.test_student_stream import _group_fwd, plan_np

NEW = ["srwn_logistic_noise_slots", "srwn_flow_stream_in_slots", "srwn_residual_group_fwd_stream_slots",
       "srwn_flow_stream_out_slots", "srwn_flow_stream_reset_slots"]
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _lib(binding):
    L = sub("_lib")
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "sr-wavenet_amd", "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.build()
    return L.bind(binding)


# ----------------------------------------------------------------------------------------------------------------
# 1. the scheme: one set of buffers [capacity][Hrows_g | n], slot u's row 0 at absolute time t_u - Hrows_g
# ----------------------------------------------------------------------------------------------------------------
class PoolNP:
    """The pool restated: per flow and group a history [capacity, Hrows_g, R] and a carry [capacity, 2]; per slot t and
    t_end.  A step gives slot u ran = clamp(t_end - t, 0, n) rows, computed at the slot's own time; a slot without rows
    is not touched; a join zeroes the slot's histories and carries and nothing else."""

    def __init__(self, flows, groups, capacity, pool):
        self.flows, self.groups, self.cap, self.pool = flows, groups, capacity, pool
        R = flows[0].init_w.shape[-1]
        self.hrows = [sum(flows[0].dilations[l0:l1]) for l0, l1 in groups]
        self.hist = [[np.zeros((capacity, H, R)) for H in self.hrows] for _ in flows]
        self.carry = [np.zeros((capacity, 2)) for _ in flows]
        self.t = np.zeros(capacity, np.int64); self.end = np.zeros(capacity, np.int64)
        self.noise = [None] * capacity; self.cond = [None] * capacity

    def join(self, u, noise, cond, end):
        assert self.t[u] >= self.end[u]
        for f in range(len(self.flows)):
            for h in self.hist[f]:
                h[u] = 0.0
            self.carry[f][u] = 0.0
        self.t[u], self.end[u], self.noise[u], self.cond[u] = 0, end, noise, cond

    def step(self, n):
        out = {}
        for u in range(self.cap):
            ran = int(np.clip(self.end[u] - self.t[u], 0, n))
            if ran == 0:
                continue
            t0 = int(self.t[u])
            x = self.noise[u][None, t0:t0 + ran]
            for f, p in enumerate(self.flows):
                xx = np.concatenate([self.carry[f][u:u + 1], x], 1)
                h = xx[:, 0:ran, None] * p.init_w[0, 0][None, None, :] + xx[:, 1:ran + 1, None] * p.init_w[1, 0][None, None, :] + p.init_b
                self.carry[f][u] = xx[0, -2:]
                for gi, (l0, l1) in enumerate(self.groups):
                    H = self.hrows[gi]
                    buf = np.concatenate([self.hist[f][gi][u:u + 1], h], 1)
                    self.hist[f][gi][u] = buf[0, buf.shape[1] - H:]
                    h = _group_fwd(p, l0, l1, buf, self.cond[u][None], self.pool, t0 - H)[:, H:]
                prm = np.maximum(h, 0) @ p.head_w2 + p.head_b2
                x = x * np.exp(prm[..., 0]) + prm[..., 1]
            out[u] = x[0]
            self.t[u] += n      # (as the kernel: a live slot's clock moves by the chunk)
        return out


def test_slot_scheme_equals_each_stream_alone():
    rng = np.random.default_rng(1)
    dil = [1, 2, 4, 8, 16, 32, 64, 128] * 2
    pool, R, E = 64, 8, 5
    flows = [O.init_flow_params(21 + i, dil, 2, R, 16, E, bias_scale=0.1) for i in range(2)]
    groups = plan_np(dil)
    assert [sum(dil[a:b]) for a, b in groups] == [31, 224, 31, 224]
    # (frames, max_samples): one ended by max_samples inside a frame, two by their frames
    specs = {"a": (12, 700), "b": (5, None), "c": (12, None)}
    streams = {}
    for k, (frames, mx) in specs.items():
        T = frames * pool
        noise = rng.logistic(0, 1, T); cond = rng.standard_normal((frames, E))
        ref = O.student_forward(flows, noise[None], cond[None], pool)
        end = T if mx is None else min(T, mx)
        streams[k] = dict(noise=noise, cond=cond, end=end, x_last=ref["x_last"][0, :end], out=ref["out"][0, :end], got=[])
    # chunk sizes Hrows_g - 1, Hrows_g, Hrows_g + 1 of both group kinds; joins at pool steps 0, 3 and 6: "b" starts on a
    # chunk boundary that lies inside one of "a"'s conditioning frames (a at t = 93) and then crosses its own frame
    # boundaries exactly (64, 128); "c" takes the slot "b" left
    chunks = [30, 31, 32, 64, 64, 223, 224, 225, 33, 1, 100, 200]
    joins = {0: ("a", 0), 3: ("b", 1), 6: ("c", 1)}
    P = PoolNP(flows, groups, 2, pool)
    where = {}
    for i, n in enumerate(chunks):
        if i in joins:
            k, u = joins[i]
            assert P.t[u] >= P.end[u], "the slot is free"
            P.join(u, streams[k]["noise"], streams[k]["cond"], streams[k]["end"])
            where[u] = k
        for u, x in P.step(n).items():
            streams[where[u]]["got"].append(x)
    for k, s in streams.items():
        got = np.concatenate(s["got"])
        assert got.shape == (s["end"],), (k, got.shape)
        assert np.abs(got - s["x_last"]).max() <= 1e-12, k
        assert np.abs(np.clip(got, -1, 1) - s["out"]).max() <= 1e-12, k


# ----------------------------------------------------------------------------------------------------------------
# 2. declarations, the table's layout, argument errors
# ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n
    assert re.search(r"typedef struct SrwnSynthSlot \{\s*int64_t t;\s*int64_t t_end;\s*\} SrwnSynthSlot;", hdr)
    assert C.sizeof(L.SrwnSynthSlot) == 16
    assert (L.SrwnSynthSlot.t.offset, L.SrwnSynthSlot.t_end.offset) == (0, 8)
    assert np.dtype(L.SrwnSynthSlot).itemsize == 16
    assert _lib("ctypes").srwn_version() >= 108


def _ptrs(n, v=A):
    return (C.c_void_p * n)(*[v] * n)


def _dl(d):
    return (C.c_int32 * len(d))(*d)


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_slot_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 108
    BF16 = 1

    def group(x_in=A, in_rows=31 + 160, x_out=A, out_rows=992 + 160, out_hist=992, w=_ptrs(5), cond=_ptrs(5), frames=4,
              pool=64, cstride=64, dil=(1, 2, 4, 8, 16), cap=2, n=160, max_chunk=160, R=64, K=2, dtype=BF16, slots=A):
        return lib.srwn_residual_group_fwd_stream_slots(x_in, in_rows, x_out, out_rows, out_hist, w, w, w, w, cond, frames,
                                                        pool, cstride, _dl(dil), len(dil), cap, n, max_chunk, R, K, dtype,
                                                        slots, None)

    assert group(slots=None) == E_NULL
    assert b"slots" in lib.srwn_last_error()
    assert group(x_in=None) == E_NULL and group(x_out=None) == E_NULL
    assert group(w=_ptrs(5, None)) == E_NULL
    assert group(n=0) == E_SHAPE and group(n=161) == E_SHAPE
    assert group(in_rows=31 + 159) == E_SHAPE and group(out_rows=992 + 159) == E_SHAPE
    assert group(cap=0) == E_SHAPE
    assert group(dil=(1, 0, 4)) == E_SHAPE
    assert group(R=48) == E_UNSUPPORTED and group(K=3) == E_UNSUPPORTED
    assert group(dil=(1, 2, 4, 8, 16, 32), w=_ptrs(6), cond=_ptrs(6), in_rows=63 + 160) == E_UNSUPPORTED   # halo 63 > 31
    assert group(dtype=7) == E_DTYPE

    def fin(x=A, xs=160, carry=A, cond=A, out=A, out_rows=31 + 160, hist=31, cap=2, n=160, mc=160, R=64, dtype=BF16, slots=A):
        return lib.srwn_flow_stream_in_slots(x, xs, carry, A, A, cond, 4, 64, 64, out, out_rows, hist, cap, n, mc, R, dtype,
                                             slots, None)

    assert fin(carry=None) == E_NULL and fin(slots=None) == E_NULL and fin(cond=None) == E_NULL
    assert fin(n=0) == E_SHAPE and fin(n=161) == E_SHAPE and fin(cap=0) == E_SHAPE
    assert fin(xs=159) == E_SHAPE and fin(out_rows=31 + 159) == E_SHAPE
    assert fin(R=48) == E_UNSUPPORTED
    assert fin(dtype=9) == E_DTYPE

    def fout(h=A, top=160, x_in=A, x_out=A, xs=160, carry=A, table=A, nroll=2, cap=2, n=160, mc=160, R=64, dtype=BF16,
             slots=A, arrive=A, adv=1):
        return lib.srwn_flow_stream_out_slots(h, top, A, A, x_in, x_out, xs, carry, 1, table, nroll, cap, n, mc, R, dtype,
                                              slots, arrive, adv, None)

    assert fout(h=None) == E_NULL and fout(carry=None) == E_NULL and fout(table=None) == E_NULL
    assert fout(slots=None) == E_NULL and fout(slots=None, adv=0) == E_NULL      # every flow's exit reads the table
    assert fout(arrive=None) == E_NULL                                            # advancing needs the counter
    assert fout(n=0) == E_SHAPE and fout(n=161) == E_SHAPE and fout(top=159) == E_SHAPE and fout(nroll=-1) == E_SHAPE
    assert fout(cap=0) == E_SHAPE
    assert fout(R=48) == E_UNSUPPORTED
    assert fout(dtype=9) == E_DTYPE

    assert lib.srwn_logistic_noise_slots(None, 160, A, A, A, 2, 160, None) == E_NULL
    assert lib.srwn_logistic_noise_slots(A, 160, A, A, None, 2, 160, None) == E_NULL
    assert lib.srwn_logistic_noise_slots(A, 159, A, A, A, 2, 160, None) == E_SHAPE
    assert lib.srwn_logistic_noise_slots(A, 160, A, A, A, 2, 0, None) == E_SHAPE
    assert lib.srwn_logistic_noise_slots(A, 160, A, A, A, 0, 160, None) == E_SHAPE

    def reset(table=A, nroll=8, carry=A, ncarry=4, cstride=4, ids=A, nslots=1, cap=2, R=64, dtype=BF16):
        return lib.srwn_flow_stream_reset_slots(table, nroll, carry, ncarry, cstride, ids, nslots, cap, R, dtype, None)

    assert reset(ids=None) == E_NULL and reset(table=None) == E_NULL and reset(carry=None) == E_NULL
    assert reset(cap=0) == E_SHAPE and reset(nslots=0) == E_SHAPE and reset(nslots=3) == E_SHAPE
    assert reset(nroll=-1) == E_SHAPE and reset(cstride=3) == E_SHAPE
    assert reset(R=48) == E_UNSUPPORTED
    assert reset(dtype=9) == E_DTYPE


def test_no_cpu_fallback_for_the_pool():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    M = sub("model"); S = sub("student")
    with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
        S.SynthPool(None)
    with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
        S.FlowSynthesizer.pool(None)
    with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
        M.StudentSynthesizer.pool(None)
