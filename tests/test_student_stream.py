"""CPU tests of chunked student synthesis (srwn_version() 107): the chunk scheme itself, restated in NumPy on the fp64
oracle; the history geometry; the new entry points' declarations and argument errors through both bindings; no CPU
fallback for ``StudentSynthesizer``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import wavenet_np as O
from tests._pkg import ROOT, sub

NEW = ["srwn_flow_stream_in", "srwn_residual_group_fwd_stream", "srwn_flow_stream_out", "srwn_logistic_noise",
       "srwn_logistic_from_bits"]
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
# 1. the scheme: fixed buffer geometry [Hrows | n] per group, taps and conditioning frames by ABSOLUTE time
# ----------------------------------------------------------------------------------------------------------------
def plan_np(dil, max_halo=31, max_layers=8):
    """srwn_group_plan restated: greedy runs whose halo (sum of dilations / their gcd) stays <= max_halo."""
    groups, l0 = [], 0
    while l0 < len(dil):
        l1 = l0 + 1
        while l1 < len(dil) and l1 - l0 < max_layers:
            ds = dil[l0:l1 + 1]
            if sum(ds) // int(np.gcd.reduce(ds)) > max_halo:
                break
            l1 += 1
        groups.append((l0, l1)); l0 = l1
    return groups


def _group_fwd(p, l0, l1, h, cond, pool, t_origin):
    """Layers [l0, l1) on a buffer whose row 0 lies at absolute time t_origin."""
    tabs = np.arange(h.shape[1]) + t_origin
    for l in range(l0, l1):
        lp = p.layers[l]
        cb = cond @ lp.wc + lp.bc
        h = h + cb[:, np.maximum(tabs, 0) // pool, :]
        h[:, tabs < 0] = 0.0      # a tap at absolute time < 0 reads the conv's zero padding, at EVERY layer
        h, _s, _ = O.residual_dilation_layer(h, lp, p.dilations[l], "reference")
    return h


def _chunked_flow(p, groups, x_in, cond, pool, chunks):
    B, _ = x_in.shape
    R = p.init_w.shape[-1]
    hrows = [sum(p.dilations[l0:l1]) for l0, l1 in groups]
    hist = [np.zeros((B, H, R)) for H in hrows]      # the last Hrows_g rows of every group's INPUT
    carry = np.zeros((B, 2))
    outs, t0 = [], 0
    for n in chunks:
        x = x_in[:, t0:t0 + n]
        xx = np.concatenate([carry, x], 1)             # x[t-2], x[t-1] for the input conv behind RightShift
        h = xx[:, 0:n, None] * p.init_w[0, 0][None, None, :] + xx[:, 1:n + 1, None] * p.init_w[1, 0][None, None, :] + p.init_b
        carry = xx[:, -2:]
        for gi, (l0, l1) in enumerate(groups):
            buf = np.concatenate([hist[gi], h], 1)     # [Hrows_g | n], row 0 at absolute time t0 - Hrows_g
            hist[gi] = buf[:, buf.shape[1] - hrows[gi]:]
            h = _group_fwd(p, l0, l1, buf, cond, pool, t0 - hrows[gi])[:, hrows[gi]:]
        prm = np.maximum(h, 0) @ p.head_w2 + p.head_b2
        outs.append(x * np.exp(prm[..., 0]) + prm[..., 1])
        t0 += n
    return np.concatenate(outs, 1)


T_SCHEME = 1536
SCHEDULES = [[T_SCHEME], [1, 1, 7, 128, 255, 257, 887], [160] * 9 + [96], [31, 32, 33, 480, 481, 479],
             # chunk sizes Hrows_g - 1, Hrows_g, Hrows_g + 1 of both group kinds (31 and 224 rows), boundaries on
             # conditioning-frame boundaries (64, 128) and inside frames
             [64, 64, 30, 31, 32, 223, 224, 225, 63, 1, 579]]


@pytest.mark.parametrize("chunks", SCHEDULES, ids=lambda c: "-".join(str(v) for v in c[:4]))
def test_chunk_scheme_equals_one_pass(chunks):
    rng = np.random.default_rng(0)
    dil = [1, 2, 4, 8, 16, 32, 64, 128] * 2
    B, T, pool, R, E = 2, T_SCHEME, 64, 8, 5
    assert sum(chunks) == T
    flows = [O.init_flow_params(11 + i, dil, 2, R, 16, E, bias_scale=0.1) for i in range(2)]
    noise = rng.logistic(0, 1, (B, T)); cond = rng.standard_normal((B, T // pool, E))
    ref = O.student_forward(flows, noise, cond, pool)
    groups = plan_np(dil)
    assert [sum(dil[a:b]) for a, b in groups] == [31, 224, 31, 224]
    x = noise
    for p in flows:
        x = _chunked_flow(p, groups, x, cond, pool, chunks)
    assert np.abs(x - ref["x_last"]).max() <= 1e-12
    assert np.abs(np.clip(x, -1, 1) - ref["out"]).max() <= 1e-12


# ----------------------------------------------------------------------------------------------------------------
# 2. geometry, declarations, argument errors
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dil,want", [([2 ** i for i in range(10)] * 3, [31, 992] * 3),
                                      ([1, 2, 4, 8, 16, 32, 64, 128] * 2, [31, 224] * 2),
                                      ([1, 2, 4, 8], [15])])
def test_history_rows_follow_the_group_plan(dil, want):
    _lib("ctypes")
    S = sub("student"); K = sub("kernels")
    groups = K.group_plan(dil, 31, 8)
    assert groups == plan_np(dil)
    got = S.stream_history_rows(dil)
    assert got == [sum(dil[a:b]) for a, b in plan_np(dil)] == want
    assert sum(got) == sum(dil)
    for (l0, l1), h in zip(groups, got):      # = stride x halo of the group kernel
        st = int(np.gcd.reduce(dil[l0:l1]))
        assert h == st * sum(d // st for d in dil[l0:l1]) and h // st <= 31


def test_new_symbols_are_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in L.SIGNATURES, n
        assert '"%s"' % n in src, n


def _ptrs(n, v=A):
    return (C.c_void_p * n)(*[v] * n)


def _dl(d):
    return (C.c_int32 * len(d))(*d)


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_stream_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    assert lib.srwn_version() >= 107
    BF16 = 1

    def group(x_in=A, in_rows=31 + 160, x_out=A, out_rows=992 + 160, out_hist=992, w=_ptrs(5), cond=_ptrs(5), frames=4,
              pool=64, cstride=64, dil=(1, 2, 4, 8, 16), B=2, n=160, max_chunk=160, R=64, K=2, dtype=BF16, clock=A):
        return lib.srwn_residual_group_fwd_stream(x_in, in_rows, x_out, out_rows, out_hist, w, w, w, w, cond, frames, pool,
                                                  cstride, _dl(dil), len(dil), B, n, max_chunk, R, K, dtype, clock, None)

    assert group(clock=None) == E_NULL                      # the state's device clock
    assert b"clock" in lib.srwn_last_error()
    assert group(x_in=None) == E_NULL and group(x_out=None) == E_NULL
    assert group(w=_ptrs(5, None)) == E_NULL
    assert group(n=0) == E_SHAPE and group(n=161) == E_SHAPE            # n < 1, n > max_chunk
    assert group(in_rows=31 + 159) == E_SHAPE                          # history + max_chunk rows per stream
    assert group(out_rows=992 + 159) == E_SHAPE
    assert group(B=0) == E_SHAPE
    assert group(dil=(1, 0, 4)) == E_SHAPE
    assert group(R=48) == E_UNSUPPORTED
    assert group(K=3) == E_UNSUPPORTED
    assert group(dil=(1, 2, 4, 8, 16, 32), w=_ptrs(6), cond=_ptrs(6), in_rows=63 + 160) == E_UNSUPPORTED   # halo 63 > 31
    assert b"halo" in lib.srwn_last_error()
    assert group(dtype=7) == E_DTYPE
    assert group(dil=(1024,), w=_ptrs(1), cond=_ptrs(1), in_rows=1024 + 159) == E_SHAPE     # a group of one layer: same checks
    assert group(dil=(1024,), w=_ptrs(1), cond=_ptrs(1), in_rows=1024 + 160, R=16) == E_UNSUPPORTED

    def fin(x=A, xs=160, carry=A, cond=A, out=A, out_rows=31 + 160, hist=31, B=2, n=160, mc=160, R=64, dtype=BF16, clock=A):
        return lib.srwn_flow_stream_in(x, xs, carry, A, A, cond, 4, 64, 64, out, out_rows, hist, B, n, mc, R, dtype, clock, None)

    assert fin(carry=None) == E_NULL and fin(clock=None) == E_NULL and fin(cond=None) == E_NULL
    assert fin(n=0) == E_SHAPE and fin(n=161) == E_SHAPE
    assert fin(xs=159) == E_SHAPE and fin(out_rows=31 + 159) == E_SHAPE
    assert fin(R=48) == E_UNSUPPORTED
    assert fin(dtype=9) == E_DTYPE

    def fout(h=A, top=160, x_in=A, x_out=A, xs=160, carry=A, table=A, nroll=2, B=2, n=160, mc=160, R=64, dtype=BF16, clock=A,
             adv=1):
        return lib.srwn_flow_stream_out(h, top, A, A, x_in, x_out, xs, carry, 1, table, nroll, B, n, mc, R, dtype, clock, adv,
                                        None)

    assert fout(h=None) == E_NULL and fout(carry=None) == E_NULL and fout(table=None) == E_NULL
    assert fout(clock=None) == E_NULL                       # advancing needs the clock
    assert fout(n=0) == E_SHAPE and fout(n=161) == E_SHAPE and fout(top=159) == E_SHAPE and fout(nroll=-1) == E_SHAPE
    assert fout(R=48) == E_UNSUPPORTED
    assert fout(dtype=9) == E_DTYPE

    assert lib.srwn_logistic_noise(None, 160, A, A, A, 2, 160, None) == E_NULL
    assert lib.srwn_logistic_noise(A, 160, A, A, None, 2, 160, None) == E_NULL
    assert lib.srwn_logistic_noise(A, 159, A, A, A, 2, 160, None) == E_SHAPE
    assert lib.srwn_logistic_noise(A, 160, A, A, A, 2, 0, None) == E_SHAPE
    assert lib.srwn_logistic_from_bits(None, None, 0, None) == 0
    assert lib.srwn_logistic_from_bits(None, A, 4, None) == E_NULL
    assert lib.srwn_logistic_from_bits(A, A, -1, None) == E_SHAPE


def test_bits_to_uniform_map_is_open_on_both_sides():
    """The map srwn.h states, in fp32 arithmetic: u = (k + 1/2) / 2^23 for the 23 bits k; at both ends u and 1 - u are
    exact and positive, so log u - log(1 - u) is finite.  (uniform01's 24 bits + 1/2 round to 1.0f at the top.)"""
    f = np.float32
    for k in (0, 2 ** 23 - 1):
        u = (f(k) + f(0.5)) * f(1.0 / 8388608.0)
        assert 0 < u < 1 and f(1) - u > 0
        assert float(u) == (k + 0.5) / 2 ** 23 and float(f(1) - u) == 1 - (k + 0.5) / 2 ** 23
        assert np.isfinite(np.log(u) - np.log(f(1) - u))
    assert (f(2 ** 24 - 1) + f(0.5)) * f(1.0 / 16777216.0) == f(1.0)


def test_no_cpu_fallback_for_the_synthesizer():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    M = sub("model"); S = sub("student"); EG = sub("engine")
    with pytest.raises(RuntimeError, match="needs an MI355X.*no CPU fallback"):
        M.StudentSynthesizer([1, 2, 4], 2, dilation_channels=32)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        S.FlowSynthesizer(EG.StackConfig(dilations=[1, 2], cond_channels=4, pool_stride=8), 1)
