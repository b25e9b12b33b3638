"""GPU tests that hold the Parallel-WaveNet student's own kernels (csrc/srwn_flow.hip: srwn_flow_affine_fwd / _bwd,
srwn_causal_conv1d_dgrad, srwn_power_loss, srwn_sumsq, srwn_clip_scale, srwn_clamp / _bwd, srwn_axpy_dev) and the Cin = 1
input-conv kernels every model starts with (csrc/srwn_util.hip: srwn_causal_conv1d_fwd, srwn_init_conv_wgrad,
srwn_reduce_loss) to exact references ENTRY BY ENTRY, where tests/test_gpu_student.py, test_gpu_kernels.py and
test_gpu_bwd.py hold them to max|a - b| / max|b| at one or two shapes.

The designs, their float64 references and the bound constants are tests/flow_design.py's (D); tests/test_flow_design.py
proves the designs' conditions on the CPU.  Every output is allocated with PAD spare elements behind its last and poisoned
with NaN, every input is NaN-padded past its stated length: the spare elements must keep their poison, and a NaN inside
a compared range equals no reference.

  flow head   R 32 / 64, fp32 / bf16, rows 1, 33, 65, 255, 256, 257, 513 (the row-group edges of both lane layouts, one
              block, one row more, three blocks).  Exact design (prm0 = 0): prm, x_out, every ent_partials[block], every
              row of w_partials (all 2R + 2 columns), g (bf16: rounded once, ties to even) and dx_in bit for bit.  General
              design (exact p0 over [-80, 80]): prm, ent_partials and the dprm1 columns of w_partials still bit for bit,
              x_out, dx_in, g and the dprm0 columns per entry; p0 = 89: x_out = +-inf with the sign of x_in.  h holds
              +0.0, -0.0 and negatives: g is +0 there.  ent_grad 0 and -1/4.  The backward's prm is a designed one.
  dgrad       B 3, T 1 / 2 / 255 / 256 / 257, (K, Cin, Cout) = (1,1,8), (2,1,64), (3,3,32), (2,96,64) (48 KiB of weights),
              dilation 1 / T - 1 / T / T + 5, shift 0 / 1 / T, plain and accumulating with scale 1/2: bit for bit
  conv fwd    the Cin = 1 kernels for K = 2 and for K != 2, the generic kernel (Cin 3, Cout 24, Cout 10); Cout 8 at 2049
              rows, Cout 2048 at 9 rows, Cout 64 at 255 / 256 / 257 rows, T = 1, dilation >= T, shift -1 / 0 / 1, bias and
              null, fp32 and bf16 out: bit for bit
  wgrad       srwn_init_conv_wgrad: R 32 / 64 / 128, K 1 / 2 / 3 / 7, shift -1 / 0 / 1, (B, T) = (1,255), (1,256), (1,257),
              (6,100), (3,1), (65,256), (1,16640): every partial of every block, gw and gb bit for bit; partials-only mode.
              The first stage's reduction buffer takes 8192 (K + 1) bytes of dynamic LDS whatever R, so K = 7 asks for
              exactly 64 KiB at EVERY R and K = 8 for 72 KiB: the MI355X launches K = 7 (correct at all three R) and the
              entry refuses K = 8 with its own SRWN_E_UNSUPPORTED at every R, R = 32 and 64 included -- K = 8 cannot be
              held bit for bit at any R; K = 7 stands in its place as the widest filter that launches.
  clipping    sumsq n 1 / 4095 / 4096 / 4097 / 12288 / 12289, each partial bit for bit, NaN directly behind g[n - 1];
              clip_scale over 1 / 255 / 256 / 257 / 1000 partials: norm below, above and exactly at clip_norm, all-zero
              partials, pre_scale 1 and 1/2, both outputs bit for bit
  the rest    power_loss (loss, dpow, dpow = null, n = 0), reduce_loss, clamp / clamp_bwd (on, just inside and just
              outside both bounds, +-0, +-inf, lo == hi, the backward in place as student.py calls it), axpy_dev
  refusals    the header's error codes with every output's poison in place; rows = 0 / n = 0 return 0 and write nothing

What is not exact is held per entry to the bounds of tests/flow_design.py, c = C_GPU = 4 x C_CPU (measured on the CPU,
never on a GPU).  SRWN_PRINT_ERR=1 pytest -s prints what the device reaches.

Worst error / bound scale:
                         x_out    dx_in    g fp32   g bf16   w_partials
  float32 NumPy (CPU)    1.623    2.939    1.197    1.981    1.900
  C_CPU (rounded up)     2        3        1.5      2        2
  bound = 4 x C_CPU      8        12       6        8        8
  MI355X, measured       0.937    1.759    0.837    1.981    2.604

Mutations of csrc/srwn_flow.hip and csrc/srwn_util.hip on scratch builds (values only, every access inside the tests'
padded buffers; never committed): tests of this file that fail, of 113, and which
   1 flow_affine_fwd: ent accumulated without the `ok` guard                4  flow_affine_fwd (general design: a tail row's p0)
   2 flow_affine_fwd: b0 and b1 swapped                                     8  flow_affine_fwd (both designs)
   3 flow_affine_bwd: v[j] > 0 made >= 0                                   16  flow_affine_bwd (all: g at h = +-0)
   4 flow_affine_bwd: bsum read at (r * LPR + 1) * 2                       16  flow_affine_bwd (all: the column sums of dprm)
   5 flow_affine_bwd, bf16: g truncated instead of rounded                  4  flow_affine_bwd (bf16, exact design; the general
                                                                               design's bound of 8 x 2^-9 cannot see it)
   6 conv_dgrad: tap index (K - 1 - k) made k                               6  causal_conv1d_dgrad (the three shapes with K > 1)
   7 conv_dgrad: shift dropped                                              8  causal_conv1d_dgrad (all)
   8 causal_conv_cin1_kernel<*, 0>: weight row k made K - 1 - k            10  causal_conv1d_fwd (the five Cin = 1, K = 3 cases)
   9 init_conv_wgrad_stage1: t without % Tlen                               6  init_conv_wgrad (all)
  10 init_conv_wgrad_stage2: lanes stop after their first partial           6  init_conv_wgrad (all: the two 65-partial clips)
  11 sumsq_kernel: k < n made k <= n                                        4  sumsq_partials (n = 1, 4095, 4097, 12289)
  12 clip_scale_kernel: fmax(norm, clip) made norm                          1  clip_scale_cases
  13 clamp_bwd_kernel: >= lo made > lo                                      8  clamp (all)
No run faulted.  No test of this file fails on the unmutated library: the suite found no kernel bug.
"""
import os

import numpy as np
import pytest
import torch

from tests import flow_design as D
from tests import gemm_design as G
from tests._pkg import sub

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAME = {F32: "fp32", BF16: "bf16"}
NAN = float("nan")
PAD = 8
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4          # include/srwn.h
BAD_DTYPE = 7


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _host(t):
    return t.double().cpu().numpy()


def _in(a, dt=F32):
    """A device copy of `a` with PAD NaN behind its last element: the kernel is told of a.shape only."""
    a = np.asarray(a, np.float64)
    buf = torch.full((a.size + PAD,), NAN, dtype=dt, device=DEV)
    buf[:a.size] = torch.tensor(a.reshape(-1), dtype=dt)
    return buf[:a.size].view(a.shape)


class _Out:
    """An output of `shape` with PAD spare elements behind it, all poisoned."""

    def __init__(self, shape, dt=F32, fill=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + PAD,), NAN, dtype=dt, device=DEV)
        self.t = self.buf[:self.n].view(shape)
        if fill is not None:
            self.t.copy_(torch.tensor(np.asarray(fill, np.float64), dtype=dt).view(shape))

    def got(self, what):
        """The written range on the host, after asserting that the spare elements kept their poison."""
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[self.n:]).all()), what + ": written behind the last element"
        return _host(self.t)

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.buf).all())


def _exact(what, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = G.same_bits(got, want)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d entries differ from the exact reference, first at %s: got %r, want %r"
                             % (what, len(bad), ok.size, list(i), got[i], want[i]))


def _bounded(what, key, got, ref, scale):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what + ": an entry not finite (unwritten or NaN)"
    r = D.ratio(got, ref, scale)
    c = D.C_GPU[key]
    _say("%-60s %-10s error / bound scale %.3f (<= %g)" % (what, key, r.max(initial=0), c))
    bad = np.argwhere(~(r <= c))
    assert len(bad) == 0, "%s: error / bound scale %.3g > %g at %s (%d entries)" % (what, r.max(), c, bad[0].tolist(), len(bad))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _refused(code, outs, name, *args):
    call = sub("_lib").call
    with pytest.raises(RuntimeError, match=r"\(code %d\)" % code):
        call(name, *args)
    for o in outs:
        assert o.untouched(), name + ": a refused call wrote an output"


def _nothing(outs, name, *args):
    """A call of zero rows returns 0 and writes nothing."""
    assert sub("_lib").call(name, *args) == 0
    for o in outs:
        assert o.untouched(), name + ": a call of no rows wrote an output"


# ---- the flow head ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", D.FLOW_RS)
def test_flow_affine_fwd_entries(R, dt, general):
    """prm and every ent_partials[block] bit for bit in both designs (p0 is dyadic in both); x_out bit for bit where
    prm0 = 0 (expf(0) = 1), per entry where it is not, +-inf with the sign of x_in where p0 = 89.  srwn_flow_partials(rows)
    entries are written and the next keeps its poison."""
    K = sub("kernels")
    for rows in D.FLOW_ROWS:
        d = D.flow_fwd(rows, R, general)
        nb = K.flow_partials(rows)
        assert nb == len(d["ent"]) == -(-rows // 256)
        prm, x_out, ent = _Out((rows, 2)), _Out((rows,)), _Out((nb,))
        K.flow_affine_fwd(_in(d["h"], dt), _in(d["w2"]), _in(d["b2"]), _in(d["x_in"]), prm.t, x_out.t, ent.t)
        what = "flow_affine_fwd %s R %d rows %d %s" % (NAME[dt], R, rows, "general" if general else "exact")
        _exact(what + " prm", prm.got(what), d["prm"])
        _exact(what + " ent_partials", ent.got(what), d["ent"])
        xo = x_out.got(what)
        if not general:
            _exact(what + " x_out", xo, d["x_out"])
            continue
        top = d["inf_rows"]
        assert np.array_equal(xo[top], d["x_out"][top]), what + ": x_out where expf overflows must be inf with the sign of x_in"
        _bounded(what + " x_out", "x_out", xo[~top], d["x_out"][~top], d["x_scale"][~top])


@pytest.mark.parametrize("ent_grad", D.ENT_GRADS)
@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", D.FLOW_RS)
def test_flow_affine_bwd_entries(R, dt, general, ent_grad):
    """On a DESIGNED prm (not the forward's output).  Exact design: g (rounded once to the dtype, ties to even), dx_in and
    every row of w_partials, all 2R + 2 columns, bit for bit.  General design: the dprm1 columns bit for bit, the rest per
    entry.  g is exactly +0 wherever h is +0.0, -0.0 or negative."""
    K = sub("kernels")
    mode = NAME[dt]
    for rows in D.FLOW_ROWS:
        d = D.flow_bwd(rows, R, general, ent_grad)
        nb = K.flow_partials(rows)
        g, dx_in, wp = _Out((rows, R), dt), _Out((rows,)), _Out((nb, 2 * R + 2))
        K.flow_affine_bwd(_in(d["h"], dt), _in(d["w2"]), _in(d["prm"]), _in(d["x_in"]), _in(d["dx_out"]), ent_grad, g.t,
                          dx_in.t, wp.t)
        what = "flow_affine_bwd %s R %d rows %d %s ent_grad %g" % (mode, R, rows, "general" if general else "exact", ent_grad)
        gg, gx, gw = g.got(what), dx_in.got(what), wp.got(what)
        off = ~d["pos"]
        assert (gg[off] == 0).all() and not np.signbit(gg[off]).any(), what + ": g must be +0 where h <= 0"
        ex = d["exact_cols"]
        _exact(what + " w_partials (exact columns)", gw[:, ex], d["wp"][:, ex])
        if not general:
            _exact(what + " g", gg, G.round_out(d["g"], mode))
            _exact(what + " dx_in", gx, d["dx_in"])
            continue
        _bounded(what + " g", "g_" + mode, gg, d["g"], D.g_scale(d, mode))
        _bounded(what + " dx_in", "dx_in", gx, d["dx_in"], D.EPS * np.abs(d["dx_in"]))
        _bounded(what + " w_partials", "w_partials", gw[:, ~ex], d["wp"][:, ~ex], d["wp_scale"][:, ~ex])


@pytest.mark.parametrize("dt", [F32, BF16])
def test_flow_affine_refusals(dt):
    R, rows = 32, 33
    d = D.flow_bwd(rows, R, False, 0.0)
    h, w2, b2, prm_in, x_in, dxo = _in(d["h"], dt), _in(d["w2"]), _in([0.0, 1.0]), _in(d["prm"]), _in(d["x_in"]), _in(d["dx_out"])
    prm, x_out, ent = _Out((rows, 2)), _Out((rows,)), _Out((1,))
    outs = [prm, x_out, ent]
    a = [h.data_ptr(), w2.data_ptr(), b2.data_ptr(), x_in.data_ptr(), prm.t.data_ptr(), x_out.t.data_ptr(), ent.t.data_ptr()]
    abi, st = sub("kernels").abi_dtype(dt), _stream()
    for i in range(7):
        _refused(E_NULL, outs, "srwn_flow_affine_fwd", *(a[:i] + [None] + a[i + 1:]), rows, R, abi, st)
    _refused(E_SHAPE, outs, "srwn_flow_affine_fwd", *a, -1, R, abi, st)
    _refused(E_UNSUPPORTED, outs, "srwn_flow_affine_fwd", *a, rows, 16, abi, st)
    _refused(E_DTYPE, outs, "srwn_flow_affine_fwd", *a, rows, R, BAD_DTYPE, st)
    _nothing(outs, "srwn_flow_affine_fwd", *a, 0, R, abi, st)
    g, dx_in, wp = _Out((rows, R), dt), _Out((rows,)), _Out((1, 2 * R + 2))
    outs = [g, dx_in, wp]
    a = [h.data_ptr(), w2.data_ptr(), prm_in.data_ptr(), x_in.data_ptr(), dxo.data_ptr(), 0.0, g.t.data_ptr(), dx_in.t.data_ptr(),
         wp.t.data_ptr()]
    for i in (0, 1, 2, 3, 4, 6, 7, 8):
        _refused(E_NULL, outs, "srwn_flow_affine_bwd", *(a[:i] + [None] + a[i + 1:]), rows, R, abi, st)
    _refused(E_SHAPE, outs, "srwn_flow_affine_bwd", *a, -1, R, abi, st)
    _refused(E_UNSUPPORTED, outs, "srwn_flow_affine_bwd", *a, rows, 16, abi, st)
    _refused(E_DTYPE, outs, "srwn_flow_affine_bwd", *a, rows, R, BAD_DTYPE, st)
    _nothing(outs, "srwn_flow_affine_bwd", *a, 0, R, abi, st)
    assert sub("kernels").flow_partials(0) == 0 and sub("kernels").flow_partials(-5) == 0


# ---- srwn_causal_conv1d_dgrad -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("shape", D.DGRAD_SHAPES)
def test_causal_conv1d_dgrad_entries(shape, dt):
    """Bit for bit at every T, dilation (1, T - 1, T: no tap but the last reaches a row; T + 5) and shift (0, 1, T: nothing
    reaches), plain and accumulating with scale 1/2 into a non-zero dx.  15 on every clip's first rows where the rest is
    <= 3: a read across the clip boundary shows."""
    Kn = sub("kernels")
    K, Cin, Cout = shape
    B = D.DGRAD_B
    for T in D.DGRAD_TS:
        d = D.dgrad(T, K, Cin, Cout)
        dy, w = _in(d["dy"], dt), _in(d["w"])
        for dil in D.dilations(T):
            for shift in D.dgrad_shifts(T):
                for acc in (False, True):
                    dx = _Out((B, T, Cin), fill=d["dx0"] if acc else None)
                    Kn.causal_conv1d_dgrad(dy, w, dx.t, dil, shift, acc, D.DGRAD_SCALE if acc else 1.0)
                    what = "causal_conv1d_dgrad %s K %d Cin %d Cout %d T %d d %d shift %d acc %d" % (NAME[dt], K, Cin, Cout, T, dil, shift, acc)
                    _exact(what, dx.got(what), D.dgrad_ref(d, dil, shift, acc))


def test_causal_conv1d_dgrad_refusals():
    B, T, (K, Cin, Cout) = 3, 2, D.DGRAD_SHAPES[1]
    d = D.dgrad(T, K, Cin, Cout)
    dy, w, dx = _in(d["dy"]), _in(d["w"]), _Out((B, T, Cin))
    p, st, n = (dy.data_ptr(), w.data_ptr(), dx.t.data_ptr()), _stream(), "srwn_causal_conv1d_dgrad"
    for i in range(3):
        _refused(E_NULL, [dx], n, *(p[:i] + (None,) + p[i + 1:]), B, T, Cin, Cout, K, 1, 0, 0, 1.0, 0, st)
    _refused(E_SHAPE, [dx], n, *p, -1, T, Cin, Cout, K, 1, 0, 0, 1.0, 0, st)
    _refused(E_SHAPE, [dx], n, *p, B, -1, Cin, Cout, K, 1, 0, 0, 1.0, 0, st)
    _refused(E_SHAPE, [dx], n, *p, B, T, Cin, 12, K, 1, 0, 0, 1.0, 0, st)          # Cout % 8
    _refused(E_SHAPE, [dx], n, *p, B, T, Cin, Cout, K, 0, 0, 0, 1.0, 0, st)        # dilation 0
    _refused(E_SHAPE, [dx], n, *p, B, T, Cin, Cout, K, 1, -1, 0, 1.0, 0, st)       # shift < 0
    _refused(E_DTYPE, [dx], n, *p, B, T, Cin, Cout, K, 1, 0, 0, 1.0, BAD_DTYPE, st)
    K2, C2, O2 = D.DGRAD_REFUSED                                                   # one input channel past 48 KiB of weights
    _refused(E_UNSUPPORTED, [dx], n, *p, B, T, C2, O2, K2, 1, 0, 0, 1.0, 0, st)
    _nothing([dx], n, *p, 0, T, Cin, Cout, K, 1, 0, 0, 1.0, 0, st)
    _nothing([dx], n, *p, B, 0, Cin, Cout, K, 1, 0, 0, 1.0, 0, st)


# ---- srwn_causal_conv1d_fwd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("case", D.CONV_FWD, ids=lambda c: "B%d-T%d-Cin%d-Cout%d-K%d" % c)
def test_causal_conv1d_fwd_entries(case, dt):
    """Bit for bit (bf16: rounded once, ties to even) on all four code paths: every dilation (>= T among them), shift
    -1 / 0 / 1, with a bias and without."""
    Kn = sub("kernels")
    B, T, Cin, Cout, K = case
    d = D.conv_fwd(B, T, Cin, Cout, K)
    x, w, b = _in(d["x"]), _in(d["w"]), _in(d["b"])
    for dil in D.conv_dilations(T):
        for shift in D.CONV_SHIFTS:
            for bias in (True, False):
                y = _Out((B, T, Cout), dt)
                Kn.causal_conv1d_fwd(x, w, b if bias else None, dil, shift, out=y.t)
                what = "causal_conv1d_fwd %s (%s) %s d %d shift %d bias %d" % (NAME[dt], D.conv_path(Cin, Cout, K), case, dil, shift, bias)
                _exact(what, y.got(what), G.round_out(D.conv_fwd_ref(d, dil, shift, bias), NAME[dt]))


def test_causal_conv1d_fwd_refusals():
    B, T, Cin, Cout, K = 3, 45, 1, 64, 2
    d = D.conv_fwd(B, T, Cin, Cout, K)
    x, w, b, y = _in(d["x"]), _in(d["w"]), _in(d["b"]), _Out((B, T, Cout))
    p, st, n = (x.data_ptr(), w.data_ptr(), b.data_ptr(), y.t.data_ptr()), _stream(), "srwn_causal_conv1d_fwd"
    for i in (0, 1, 3):                                                             # (a null bias is no bias)
        _refused(E_NULL, [y], n, *(p[:i] + (None,) + p[i + 1:]), B, T, Cin, Cout, K, 1, 0, 0, st)
    _refused(E_SHAPE, [y], n, *p, -1, T, Cin, Cout, K, 1, 0, 0, st)
    _refused(E_SHAPE, [y], n, *p, B, T, 0, Cout, K, 1, 0, 0, st)
    _refused(E_SHAPE, [y], n, *p, B, T, Cin, Cout, 0, 1, 0, 0, st)
    _refused(E_SHAPE, [y], n, *p, B, T, Cin, Cout, K, 0, 0, 0, st)
    _refused(E_DTYPE, [y], n, *p, B, T, Cin, Cout, K, 1, 0, BAD_DTYPE, st)         # (the Cin = 1 shape)
    _refused(E_DTYPE, [y], n, *p, B, T // 3, 3, Cout, K, 1, 0, BAD_DTYPE, st)      # (the generic one)
    _nothing([y], n, *p, 0, T, Cin, Cout, K, 1, 0, 0, st)
    _nothing([y], n, *p, B, 0, Cin, Cout, K, 1, 0, 0, st)


# ---- srwn_init_conv_wgrad -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", D.IC_RS)
def test_init_conv_wgrad_entries(R, dt):
    """Every partial of every block, gw and gb bit for bit: blocks that start inside a clip and span several ((6, 100)),
    65 partials over many clips and inside one (a second pass of the second stage's lane stride), one row per clip; K = 7
    asks for exactly 64 KiB of dynamic LDS.  srwn_init_conv_wgrad_partials(...) floats are written, no more.  The
    partials-only mode (gw = gb = null) leaves the same partials and the same poison behind them."""
    Kn = sub("kernels"); lib = sub("_lib").load()
    for (B, T) in D.IC_CLIPS:
        ic = D.init_conv(B, T, R)
        audio, g = _in(ic.audio), _in(ic.g, dt)
        nparts = -(-B * T // D.IC_BLOCK)
        for K in D.IC_KS:
            need = int(lib.srwn_init_conv_wgrad_partials(B, T, R, K))
            assert need == nparts * (K + 1) * R
            for shift in (-1, 0, 1):
                ref = ic.partials(K, shift)
                what = "init_conv_wgrad %s R %d B %d T %d K %d shift %d" % (NAME[dt], R, B, T, K, shift)
                for only in ((False, True) if shift == 0 or B * T <= 600 else (False,)):
                    ws = _Out((nparts, K + 1, R))
                    gw, gb = (None, None) if only else (_Out((K, R)), _Out((R,)))
                    n = Kn.init_conv_wgrad(audio, g, None if only else gw.t, None if only else gb.t, K, shift, ws.buf)
                    assert n == nparts
                    _exact(what + " partials" + (" (partials only)" if only else ""), ws.got(what), ref)
                    if not only:
                        _exact(what + " gw", gw.got(what), ref.sum(0)[:K])
                        _exact(what + " gb", gb.got(what), ref.sum(0)[K])


def test_init_conv_wgrad_refusals():
    """K = 8 asks for 72 KiB of LDS at every R: the entry's own SRWN_E_UNSUPPORTED, not a launch error."""
    B, T, R, K = 3, 1, 32, 2
    ic = D.init_conv(B, T, R)
    audio, g = _in(ic.audio), _in(ic.g)
    ws, gw, gb = _Out((1, 9, 128)), _Out((8, 128)), _Out((128,))
    outs = [ws, gw, gb]
    p, st, n = (audio.data_ptr(), g.data_ptr(), ws.t.data_ptr(), gw.t.data_ptr(), gb.t.data_ptr()), _stream(), "srwn_init_conv_wgrad"
    for i in range(5):                                                              # gw without gb, gb without gw among them
        _refused(E_NULL, outs, n, *(p[:i] + (None,) + p[i + 1:]), B, T, R, K, 0, 0, st)
    _refused(E_SHAPE, outs, n, *p, B, T, R, 9, 0, 0, st)
    _refused(E_SHAPE, outs, n, *p, B, T, R, 0, 0, 0, st)
    _refused(E_SHAPE, outs, n, *p, B, T, 48, K, 0, 0, st)
    _refused(E_SHAPE, outs, n, *p, 0, T, R, K, 0, 0, st)
    _refused(E_SHAPE, outs, n, *p, B, 0, R, K, 0, 0, st)
    for R_ in D.IC_RS:
        assert D.ic_lds(R_, D.IC_K_REFUSED) > 65536
        _refused(E_UNSUPPORTED, outs, n, *p, 1, 1, R_, D.IC_K_REFUSED, 0, 0, st)
    _refused(E_DTYPE, outs, n, *p, B, T, R, K, 0, BAD_DTYPE, st)


# ---- srwn_sumsq / srwn_clip_scale ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", D.SUMSQ_NS)
def test_sumsq_partials(n):
    """Each chunk's partial bit for bit; the NaN directly behind g[n - 1] reaches none; srwn_sumsq_partials(n) are written."""
    Kn = sub("kernels")
    d = D.sumsq(n)
    np_ = Kn.sumsq_partials(n)
    assert np_ == len(d["parts"]) == -(-n // D.SQ_CHUNK)
    g, parts = _in(d["g"]), _Out((np_,))
    Kn.sumsq(g, parts.t)
    _exact("sumsq n %d" % n, parts.got("sumsq"), d["parts"])


def test_clip_scale_cases():
    """norm below, above and exactly at clip_norm, all-zero partials (scale = pre_scale, finite), pre_scale 1 and 1/2, over
    1 ... 1000 partials: (scale, norm) bit for bit against the header's formula in float64, rounded once."""
    Kn = sub("kernels")
    for m in D.CLIP_COUNTS:
        for name, parts, clip, pre in D.clip_cases(m):
            out = _Out((2,))
            Kn.clip_scale(_in(parts), clip, pre, out.t)
            what = "clip_scale %s over %d partials, clip_norm %g, pre_scale %g" % (name, m, clip, pre)
            _exact(what, out.got(what), D.clip_ref(parts, clip, pre))


def test_sumsq_clip_scale_refusals():
    d = D.sumsq(1)
    g, parts, out = _in(d["g"]), _Out((1,)), _Out((2,))
    st = _stream()
    _refused(E_NULL, [parts], "srwn_sumsq", None, 1, parts.t.data_ptr(), st)
    _refused(E_NULL, [parts], "srwn_sumsq", g.data_ptr(), 1, None, st)
    _refused(E_SHAPE, [parts], "srwn_sumsq", g.data_ptr(), -1, parts.t.data_ptr(), st)
    _nothing([parts], "srwn_sumsq", g.data_ptr(), 0, parts.t.data_ptr(), st)
    assert sub("kernels").sumsq_partials(0) == 0
    p = _in(np.ones(4))
    _refused(E_NULL, [out], "srwn_clip_scale", None, 4, 1.0, 1.0, out.t.data_ptr(), st)
    _refused(E_NULL, [out], "srwn_clip_scale", p.data_ptr(), 4, 1.0, 1.0, None, st)
    _refused(E_SHAPE, [out], "srwn_clip_scale", p.data_ptr(), -1, 1.0, 1.0, out.t.data_ptr(), st)
    _refused(E_SHAPE, [out], "srwn_clip_scale", p.data_ptr(), 4, 0.0, 1.0, out.t.data_ptr(), st)
    _refused(E_SHAPE, [out], "srwn_clip_scale", p.data_ptr(), 4, -1.0, 1.0, out.t.data_ptr(), st)


# ---- srwn_power_loss / srwn_reduce_loss ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", D.POWER_NS)
def test_power_loss_entries(n):
    """loss bit for bit; dpow bit for bit against the float32 restatement in the kernel's written order (dyadic gamma and
    grad_scale: the order does not matter, and the restatement equals the float64 reference); dpow = null: the same loss."""
    Kn = sub("kernels")
    d = D.power(n)
    pt, po = _in(d["pt"]), _in(d["po"])
    for with_d in (True, False):
        dpow, loss = _Out((n,)), _Out((1,))
        Kn.power_loss(pt, po, D.POWER_GAMMA, D.POWER_GSCALE, dpow.t if with_d else None, loss.t)
        _exact("power_loss n %d loss" % n, loss.got("power_loss"), [d["loss"]])
        if with_d:
            got = dpow.got("power_loss dpow")
            _exact("power_loss n %d dpow" % n, got, D.power_dpow32(d))
            _exact("power_loss n %d dpow (float64)" % n, got, d["dpow"])
        else:
            assert dpow.untouched()


def test_power_loss_of_nothing_and_refusals():
    d = D.power(1)
    pt, po, dpow, loss = _in(d["pt"]), _in(d["po"]), _Out((1,)), _Out((1,))
    st = _stream()
    assert sub("_lib").call("srwn_power_loss", pt.data_ptr(), po.data_ptr(), 0, 0.5, 0.25, dpow.t.data_ptr(), loss.t.data_ptr(), st) == 0
    got = loss.got("power_loss n 0")
    assert got[0] == 0 and dpow.untouched()
    loss = _Out((1,))
    a = [pt.data_ptr(), po.data_ptr(), 1, 0.5, 0.25, dpow.t.data_ptr(), loss.t.data_ptr(), st]
    for i in (0, 1, 6):                                                             # (a null dpow is no dpow)
        _refused(E_NULL, [dpow, loss], "srwn_power_loss", *(a[:i] + [None] + a[i + 1:]))
    _refused(E_SHAPE, [dpow, loss], "srwn_power_loss", *(a[:2] + [-1] + a[3:]))


@pytest.mark.parametrize("n", D.REDUCE_NS)
def test_reduce_loss_entries(n):
    d = D.reduce_loss(n)
    out = _Out((1,))
    p = _in(d["p"]) if n else torch.full((PAD,), NAN, device=DEV)                   # (an empty tensor's pointer is null)
    sub("kernels").reduce_loss(p, n, D.REDUCE_SCALE, out.t)
    _exact("reduce_loss n %d" % n, out.got("reduce_loss"), [d["out"]])


def test_reduce_loss_refusals():
    p, out, st = _in(np.ones(4)), _Out((1,)), _stream()
    _refused(E_NULL, [out], "srwn_reduce_loss", None, 4, 1.0, out.t.data_ptr(), st)
    _refused(E_NULL, [out], "srwn_reduce_loss", p.data_ptr(), 4, 1.0, None, st)


# ---- srwn_clamp / srwn_clamp_bwd / srwn_axpy_dev ------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", D.CLAMP_BOUNDS)
@pytest.mark.parametrize("n", D.CLAMP_NS)
def test_clamp_entries(n, bounds):
    """Values on, just inside and just outside both bounds, +-0, +-inf (n = 1: each of them in turn); lo == hi; the backward
    in place (dx is dy), as student.py calls it, equals the out-of-place result."""
    call, st = sub("_lib").call, _stream()
    lo, hi = bounds
    for first in (range(len(D.clamp_specials(lo, hi))) if n == 1 else (0,)):
        d = D.clamp(n, lo, hi, first)
        x = _in(d["x"])
        y, dx, dy = _Out((n,)), _Out((n,)), _in(d["dy"])
        call("srwn_clamp", x.data_ptr(), y.t.data_ptr(), n, lo, hi, st)
        call("srwn_clamp_bwd", x.data_ptr(), dy.data_ptr(), dx.t.data_ptr(), n, lo, hi, st)
        what = "clamp n %d [%g, %g] first %d" % (n, lo, hi, first)
        _exact(what + " y", y.got(what), d["y"])
        _exact(what + " dx", dx.got(what), d["dx"])
        inplace = _Out((n,), fill=d["dy"])
        call("srwn_clamp_bwd", x.data_ptr(), inplace.t.data_ptr(), inplace.t.data_ptr(), n, lo, hi, st)
        _exact(what + " dx in place", inplace.got(what), d["dx"])


@pytest.mark.parametrize("n", D.AXPY_NS)
def test_axpy_dev_entries(n):
    """y += alpha scale_dev[0] x with alpha = 1/4 and the scale read from the device: 0, 1 and 2^-3."""
    call, st = sub("_lib").call, _stream()
    d = D.axpy(n)
    x = _in(d["x"])
    for s in D.AXPY_SCALES:
        y, sd = _Out((n,), fill=d["y"]), _in([s])
        call("srwn_axpy_dev", y.t.data_ptr(), x.data_ptr(), sd.data_ptr(), D.AXPY_ALPHA, n, st)
        _exact("axpy_dev n %d scale %g" % (n, s), y.got("axpy_dev"), d["y"] + D.AXPY_ALPHA * s * d["x"])


def test_clamp_axpy_refusals():
    st = _stream()
    x, y, dx = _in(np.ones(4)), _Out((4,)), _Out((4,))
    px, py, pd = x.data_ptr(), y.t.data_ptr(), dx.t.data_ptr()
    outs = [y, dx]
    _refused(E_NULL, outs, "srwn_clamp", None, py, 4, -1.0, 1.0, st)
    _refused(E_NULL, outs, "srwn_clamp", px, None, 4, -1.0, 1.0, st)
    _refused(E_SHAPE, outs, "srwn_clamp", px, py, -1, -1.0, 1.0, st)
    _refused(E_SHAPE, outs, "srwn_clamp", px, py, 4, 1.0, -1.0, st)                # lo > hi
    _nothing(outs, "srwn_clamp", px, py, 0, -1.0, 1.0, st)
    _refused(E_NULL, outs, "srwn_clamp_bwd", None, px, pd, 4, -1.0, 1.0, st)
    _refused(E_NULL, outs, "srwn_clamp_bwd", px, None, pd, 4, -1.0, 1.0, st)
    _refused(E_NULL, outs, "srwn_clamp_bwd", px, px, None, 4, -1.0, 1.0, st)
    _refused(E_SHAPE, outs, "srwn_clamp_bwd", px, px, pd, -1, -1.0, 1.0, st)
    _refused(E_SHAPE, outs, "srwn_clamp_bwd", px, px, pd, 4, 1.0, -1.0, st)
    _nothing(outs, "srwn_clamp_bwd", px, px, pd, 0, -1.0, 1.0, st)
    _refused(E_NULL, outs, "srwn_axpy_dev", None, px, px, 0.25, 4, st)
    _refused(E_NULL, outs, "srwn_axpy_dev", py, None, px, 0.25, 4, st)
    _refused(E_NULL, outs, "srwn_axpy_dev", py, px, None, 0.25, 4, st)
    _refused(E_SHAPE, outs, "srwn_axpy_dev", py, px, px, 0.25, -1, st)
    _nothing(outs, "srwn_axpy_dev", py, px, px, 0.25, 0, st)
