"""GPU tests that hold the canonical WaveNet-gate layer kernels (csrc/srwn_wngate.hip: srwn_wavenet_layer_fwd / _bwd) and
srwn_wgrad at the gate's shapes to exact references ENTRY BY ENTRY, in fp32 and in bf16, where
tests/test_gpu_gate_wavenet.py holds them to max|a - b| / max|b| at one clip shape.

The designs, their float64 references and the bound constants are tests/wngate_design.py's (W); tests/test_wngate_design.py
proves the designs' conditions on the CPU.  Every output is allocated with one spare row behind the last and poisoned
with NaN: the spare row must keep its poison and every valid entry must be finite.

  shapes      R 32 / 64; (B, T) = (1, 1), (2, 31), (2, 32), (2, 33), (3, 45), (1, 513); dilations 1, 31, 32, T - 1, T, 512;
              B = 2049, T = 33, R = 64 for the persistent loop (4098 tiles: a second and a third pass per wave)
  forward     z, s and c per entry against tanh(f), sigmoid(g) and their product on exact pre-activations: the grid
              design (|f| <= 2.25) and the saturation design (f, g beyond 44.4 and 88.7, where the exp2 of the bf16 forms
              and expf overflow); z = 0 exactly where f = 0; |z| <= 1 and 0 <= s <= 1.
              h per entry against the layer-local reference (x + c_dev Wr + br) sqrt(1/2) + cond, c_dev being the c the
              kernel stored, read back: in both dtypes the stored c has the bits of the residual MFMA operand (cf.set and
              the c_out store take the same z * s, rounded the same way), so the product's only error is its fp32
              accumulation, and c itself is pinned by the check before.  Conditioning: pool 8, frames * pool > T and no
              divisor of it, a cond row stride of 3R with 64 in the columns that must not be read.
  backward    UP only: g2 bit for bit at every shape and dilation (d = T - 1, d >= T, 15 at the clip edges where the
              rest is <= 3); with g_in per entry.  DOWN only: both halves of D bit for bit, each half on its own, for
              both skip forms.  UP + DOWN: g2 bit for bit, D per entry.  z = +-1 / s in {0, 1}: exact zeros.
  wgrad       srwn_wgrad + srwn_reduce_partials at (cin, cout) = (64, 128) and (32, 64) as engine._wgrad_wavenet_convs
              calls it (shifts (K - 1 - k) d, bias partials on the last tap only): bit for bit
  refusals    the header's error codes, poisoned outputs untouched; B = 0 and T = 0 return 0 and write nothing

What is not exact is held per entry to
    |got - ref| <= c (u_out |ref| + K 2^-24 S + f_abs),   c = 4 x the float32 NumPy restatement's worst ratio
(W.C_CPU, measured by tests/test_wngate_design.py; never a GPU figure).  SRWN_PRINT_ERR=1 pytest -s prints what the
device reaches.

Worst error / bound scale (bf16 | fp32):
                         wn_z            wn_s            wn_c            wn_h            wn_g2_gin        wn_D
  float32 NumPy (CPU)    1.265 | 0.568   1.349 | 0.581   1.814 | 0.609   1.989 | 0.111   1.949 | 0.005    1.982 | 0.118
  C_CPU (rounded up)     1.5   | 0.625   1.5   | 0.625   2     | 0.625   2     | 0.125   2     | 0.0625   2     | 0.125
  bound = 4 x C_CPU      6     | 2.5     6     | 2.5     8     | 2.5     8     | 0.5     8     | 0.25     8     | 0.5
  MI355X, measured       1.265 | 0.214   1.349 | 0.581   1.814 | 0.609   1.989 | 0.088   1.949 | 0.005    1.982 | 0.100
(the bf16 figures are the output rounding's: half an ulp is up to 2^-8 of a binade's lower end, against u_out = 2^-9.)

Mutations of csrc/srwn_wngate.hip on scratch builds (in-bounds arithmetic only; never committed): tests of this file
that fail / tests of tests/test_gpu_gate_wavenet.py that RUN the mutated code and still pass:
  1 forward tap mask tk >= 0 made tk >= -1                               18 of 44 fail /  5 of 23
  2 backward tap mask tk < Tlen made tk <= Tlen                          14 of 44 fail /  7 of 33 (both bf16 stacks among them)
  3 bias_g read as bias_f for the gate half                              18 of 44 fail /  5 of 23
  4 dg = dc s (1 - s), the z dropped                                     14 of 44 fail /  5 of 33
  5 rows_valid one too small in the last row store of each kernel        32 of 44 fail /  5 of 47
  6 filter / gate image swapped for one k-slice of the backward          14 of 44 fail /  5 of 33
  7 the tile loop ended after a wave's first tile                         4 of 44 fail / 47 of 47 (none runs > 2048 tiles)
  8 wn_sigmoid<bf16_t> replaced by the polynomial valid on [-1, 1]        9 of 44 fail /  2 of 4  (the 30-layer bf16 stack)
The five that pass 1 - 6 compare the kernels with themselves (graph replay against eager, the loss going down,
checkpoints restoring); the max-norm kernel tests catch 1 - 6 at T = 700 because a whole row or half moves, and miss 7
(a shape they never run) and, at stack level, 2 and 8 inside the bf16 bounds.
"""
import os

import numpy as np
import pytest
import torch

from tests import gemm_design as G
from tests import wngate_design as W
from tests._pkg import sub

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAME = {F32: "fp32", BF16: "bf16"}
NAN = float("nan")
E_SHAPE, E_NULL, E_UNSUPPORTED = -2, -3, -4          # include/srwn.h


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _dev(a, dt=F32):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


def _host(t):
    return t.double().cpu().numpy()


def _nan(shape, dt):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def _spare(rows, C, dt):
    """(buffer of rows + 1 poisoned rows, its first `rows` rows): the kernel is told of `rows` only."""
    buf = _nan((rows + 1, C), dt)
    return buf, buf[:rows]


def _intact(what, buf, rows):
    """The spare row keeps its poison; every entry of a valid row is finite.  Returns the valid rows on the host."""
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[rows]).all()), what + ": the row behind the last was written"
    got = _host(buf[:rows])
    bad = np.argwhere(~np.isfinite(got))
    assert len(bad) == 0, "%s: %d entries not finite (unwritten or NaN), first at %s" % (what, len(bad), bad[0].tolist())
    return got


def _exact(what, got, want):
    ok = G.same_bits(got, want)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d entries differ from the exact reference, first at %s: got %r, want %r"
                             % (what, len(bad), ok.size, list(i), got[i], want[i]))


def _bounded(what, key, mode, got, ref, S, K, f_abs=0.0):
    r = G.ratio(got, ref, S, K, mode, f_abs)
    assert np.isfinite(r).all(), what + ": a non-zero entry where the reference and its bound are exactly 0"
    c = W.C_GPU[key][mode]
    _say("%-64s %s %s error / bound scale %.3f (<= %g)" % (what, key, mode, r.max(), c))
    bad = np.argwhere(r > c)
    assert len(bad) == 0, "%s: error / bound scale %.3g > %g at %s (%d entries)" % (what, r.max(), c, bad[0].tolist(), len(bad))


def _images(dt, R, wf, wg, wr=None, ws=None, transposed=False):
    """The packed images: forward [Wf | Wg] and Wr; transposed [WfT | WgT], WrT (permuted k) and WsT.  Returns the buffer
    (kept alive by the caller) and the device pointers."""
    K = sub("kernels"); P = sub("packing")
    wr = np.zeros((R, R)) if wr is None else wr
    mats = [wf, wg, wr] + ([] if ws is None else [ws])
    flat = torch.cat([_dev(m).flatten() for m in mats])
    pk = K.Packer(DEV)
    if not transposed:
        offs = [P.pack_conv(pk, 0, 2, R)]
        assert P.pack_conv(pk, 2 * R * R, 2, R) == offs[0] + 2 * R * R
        offs.append(P.pack_res(pk, 4 * R * R, R))
    else:
        offs = [P.pack_conv_T(pk, 0, 2, R)]
        assert P.pack_conv_T(pk, 2 * R * R, 2, R) == offs[0] + 2 * R * R
        offs.append(P.pack_linear_T(pk, 4 * R * R, R, R, R, perm=True))
        if ws is not None:
            offs.append(P.pack_linear_T(pk, 5 * R * R, R, ws.shape[1], R))
    pk.finalize()
    buf = torch.empty(pk.total, dtype=dt, device=DEV)
    pk.gather(flat, buf)
    return buf, [buf.data_ptr() + o * buf.element_size() for o in offs]


# ---- forward ------------------------------------------------------------------------------------------------------------
def _fwd_case(dt, R, B, T, dil, sat, cond):
    K = sub("kernels")
    mode, rows = NAME[dt], B * T
    d = W.fwd(R, B, T, dil, sat, cond)
    f, g = W.fwd_pre(d, B, T, dil, sat)
    buf, (pc, pr) = _images(dt, R, d["wf"], d["wg"], d["wr"])
    cb = _dev(d["cond"], dt) if cond else None
    bufs, outs = zip(*[_spare(rows, R, dt) for _ in range(4)])
    K.wavenet_layer_fwd(_dev(d["x"], dt).view(B, T, R), cb, pc, pr, _dev(d["bf"]), _dev(d["bg"]), _dev(d["br"]),
                        *[o.view(B, T, R) for o in outs], 2, dil, W.POOL if cond else 1)
    what = "wavenet_layer_fwd %s R %d B %d T %d d %d%s%s" % (mode, R, B, T, dil, " sat" if sat else "", " cond" if cond else "")
    h, z, s, c = (_intact("%s %s" % (what, n), b, rows) for n, b in zip("hzsc", bufs))
    _bounded(what + " z", "wn_z", mode, z, np.tanh(f), 0.0, 0, W.f_abs_z(mode, sat))
    _bounded(what + " s", "wn_s", mode, s, W.sigmoid64(g), 0.0, 0, W.f_abs_s(mode, sat))
    _bounded(what + " c", "wn_c", mode, c, np.tanh(f) * W.sigmoid64(g), 0.0, 0, W.f_abs_c(mode, sat))
    assert (z[f == 0] == 0).all(), what + ": tanh(0) = 0 exactly"
    assert np.abs(z).max() <= 1 and s.min() >= 0 and s.max() <= 1, what
    ref, Sm = W.h_ref(d, c, B, T)
    _bounded(what + " h", "wn_h", mode, h, ref, Sm, R)


@pytest.mark.parametrize("sat", [False, True])
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", W.RS)
def test_wavenet_layer_fwd_entries(R, dt, sat):
    """z, s, c against tanh(f), sigmoid(g) and their product on exact pre-activations, h against the layer-local
    reference built from the stored c (see the module docstring): every clip of W.CLIPS at every dilation of
    W.dilations -- one row, 31 / 32 / 33 rows, a ragged last tile, d = T - 1 (one row reaches the delayed tap), d >= T
    (none does), the top of the range on both sides of every clip boundary."""
    for (R_, B, T, dil) in [c for c in W.FWD if c[0] == R]:
        _fwd_case(dt, R, B, T, dil, sat, False)


@pytest.mark.parametrize("sat", [False, True])
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", W.RS)
def test_wavenet_layer_fwd_conditioned_entries(R, dt, sat):
    """The next layer's frame bias: pool 8, frames * pool > T, T no multiple of the pool, rows 3R apart with 64 in the
    columns from R on."""
    for (R_, B, T, dil) in [c for c in W.FWD_COND if c[0] == R]:
        _fwd_case(dt, R, B, T, dil, sat, True)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_wavenet_layer_fwd_persistent_loop(dt):
    """4098 tiles on 512 workgroups of 4 waves: every wave takes a second tile, some a third, reusing its LDS stage."""
    R, B, T, dil = W.BIG
    assert B * ((T + 31) // 32) > 2 * 4 * 512
    _fwd_case(dt, R, B, T, dil, False, False)


# ---- backward -----------------------------------------------------------------------------------------------------------
def _bwd_up_case(dt, R, B, T, dil):
    K = sub("kernels")
    mode, rows = NAME[dt], B * T
    d = W.bwd_up(R, B, T, dil)
    buf, ptrs = _images(dt, R, d["wf"], d["wg"], transposed=True)
    Dd = _dev(d["D"], dt).view(B, T, 2 * R)
    a, w = W.bwd_up_ops(d, B, T, dil)
    what = "wavenet_layer_bwd UP %s R %d B %d T %d d %d" % (mode, R, B, T, dil)
    gb, g2 = _spare(rows, R, dt)
    K.wavenet_layer_bwd(None, Dd, ptrs[0], g2.view(B, T, R), None, None, None, None, None, None, None, B, T, R, 4 * R, 2, dil,
                        True, False, dt)
    _exact(what, _intact(what, gb, rows), G.round_out(a @ w, mode))
    gb, g2 = _spare(rows, R, dt)
    K.wavenet_layer_bwd(_dev(d["g_in"], dt).view(B, T, R), Dd, ptrs[0], g2.view(B, T, R), None, None, None, None, None, None,
                        None, B, T, R, 4 * R, 2, dil, True, False, dt)
    ref, Sm, Kk = W.g2_gin_ref(d, B, T, dil)
    _bounded(what + " g_in", "wn_g2_gin", mode, _intact(what + " g_in", gb, rows), ref, Sm, Kk)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", W.RS)
def test_wavenet_layer_bwd_up_exact(R, dt):
    """g2 = sum_k [WfT | WgT][k] D_up[t + (K - 1 - k) d] bit for bit without g_in, per entry with it; d = T - 1 (one row
    reaches the advanced tap), d >= T (none), 15 on both sides of every clip boundary where the rest is <= 3."""
    for (R_, B, T, dil) in [c for c in W.BWD_UP if c[0] == R]:
        _bwd_up_case(dt, R, B, T, dil)


def _zeros(what, D, z, s, R):
    assert (D[:, :R][np.abs(z) == 1] == 0).all(), what + ": df where z = +-1"
    assert (D[:, R:][(s == 0) | (s == 1) | (z == 0)] == 0).all(), what + ": dg where s is 0 or 1, or z = 0"


def _bwd_down_case(dt, R, S, B, T, form):
    K = sub("kernels")
    mode, rows = NAME[dt], B * T
    d = W.bwd_down(R, S, B, T)
    dc = W.down_dc(d, form)
    W.down_bits(dc, d["z"], d["s"])
    buf, ptrs = _images(dt, R, np.zeros((2, R, R)), np.zeros((2, R, R)), None, d["ws"], transposed=True)
    dcs = _dev(d["dcs"], dt).view(B, T, R) if form == "dcs" else None
    wsk, dtt = (None, None) if form == "dcs" else (ptrs[2], _dev(d["dtotal"], dt))
    Db, Dout = _spare(rows, 2 * R, dt)
    K.wavenet_layer_bwd(None, None, None, None, None, wsk, dtt, dcs, _dev(d["z"], dt).view(B, T, R),
                        _dev(d["s"], dt).view(B, T, R), Dout.view(B, T, 2 * R), B, T, R, S, 2, 1, False, True, dt)
    what = "wavenet_layer_bwd DOWN %s %s R %d S %d B %d T %d" % (mode, form, R, S, B, T)
    got = _intact(what, Db, rows)
    want = G.round_out(W.down_D(dc, d["z"], d["s"]), mode)
    _exact(what + " df half", got[:, :R], want[:, :R])
    _exact(what + " dg half", got[:, R:], want[:, R:])
    _zeros(what, got, d["z"], d["s"], R)


@pytest.mark.parametrize("form", W.SKIP_FORMS)
@pytest.mark.parametrize("dt", [F32, BF16])
def test_wavenet_layer_bwd_down_exact(dt, form):
    """D = [dc s (1 - z^2) | dc z s (1 - s)] on factors of few bits (W.down_bits): both halves bit for bit, each on its own
    (a stride or offset error of either store shows), dc a dyadic dcs or the exact dtotal Ws^T."""
    for (R, S, B, T) in W.DOWN:
        _bwd_down_case(dt, R, S, B, T, form)


def _bwd_updown_case(dt, R, S, B, T, dil, form):
    K = sub("kernels")
    mode, rows = NAME[dt], B * T
    up, dn = W.bwd_up(R, B, T, dil), W.bwd_down(R, S, B, T)
    buf, ptrs = _images(dt, R, up["wf"], up["wg"], dn["wr"], dn["ws"], transposed=True)
    dcs = _dev(dn["dcs"], dt).view(B, T, R) if form == "dcs" else None
    wsk, dtt = (None, None) if form == "dcs" else (ptrs[2], _dev(dn["dtotal"], dt))
    gb, g2 = _spare(rows, R, dt)
    Db, Dout = _spare(rows, 2 * R, dt)
    K.wavenet_layer_bwd(None, _dev(up["D"], dt).view(B, T, 2 * R), ptrs[0], g2.view(B, T, R), ptrs[1], wsk, dtt, dcs,
                        _dev(dn["z"], dt).view(B, T, R), _dev(dn["s"], dt).view(B, T, R), Dout.view(B, T, 2 * R), B, T, R, S, 2,
                        dil, True, True, dt)
    what = "wavenet_layer_bwd UP+DOWN %s %s R %d S %d B %d T %d d %d" % (mode, form, R, S, B, T, dil)
    Gx, ref, Sm, Kk = W.updown_ref(up, dn, B, T, dil, form, mode)
    _exact(what + " g2", _intact(what + " g2", gb, rows), G.round_out(Gx, mode))
    got = _intact(what + " D", Db, rows)
    _bounded(what + " df half", "wn_D", mode, got[:, :R], ref[:, :R], Sm[:, :R], Kk)
    _bounded(what + " dg half", "wn_D", mode, got[:, R:], ref[:, R:], Sm[:, R:], Kk)
    _zeros(what, got, dn["z"], dn["s"], R)


@pytest.mark.parametrize("form", W.SKIP_FORMS)
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", W.RS)
def test_wavenet_layer_bwd_up_down_entries(R, dt, form):
    """One UP + DOWN call with g_in = None: g2 bit for bit; the residual operand round_T(float32(G) float32(sqrt(1/2))) is
    computed exactly on the host (W.res_operand), so D carries the Wr product's fp32 accumulation only: per entry."""
    for (R_, B, T, dil) in [c for c in W.BWD_UP if c[0] == R]:
        _bwd_updown_case(dt, R, 2 * R, B, T, dil, form)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_wavenet_layer_bwd_persistent_loop(dt):
    """4098 tiles: UP (exact, and with g_in), DOWN only (exact) and UP + DOWN (per entry), over every tile."""
    R, B, T, dil = W.BIG
    assert B * ((T + 31) // 32) > 2 * 4 * 512
    _bwd_up_case(dt, R, B, T, dil)
    _bwd_down_case(dt, R, W.BIG_S, B, T, "dcs")
    _bwd_updown_case(dt, R, W.BIG_S, B, T, dil, "dtotal")


# ---- srwn_wgrad at the gate's shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("cin,cout", W.WGRAD_SHAPES)
def test_wgrad_gate_conv_shapes_exact(dt, cin, cout):
    """Both convolutions' weight gradients as engine._wgrad_wavenet_convs forms them: per tap one srwn_wgrad over a stack
    of four layers with cin = R, cout = 2R and shifts (K - 1 - k) d (d = 1, 31, T - 1, beyond T), bias partials on the last
    tap only; one row, 31 / 32 / 33 rows, two ragged clips, one slab plus a row.  Bit for bit after the reduction."""
    K = sub("kernels")
    assert K.wgrad_slabs(3072) == 1 and K.wgrad_slabs(3073) == 2, "W.wgrad_cases() assumes a 3072-row slab"
    nb = 4
    for (cin_, cout_, B, T) in [c for c in W.wgrad_cases() if c[:2] == (cin, cout)]:
        rows = B * T
        d = G.wgrad(cin, cout, B, T)
        dil = W.wgrad_dilations(T)
        ns = K.wgrad_slabs(rows)
        xd, dd = _dev(d["x"], dt), _dev(d["dy"], dt)
        for k in range(2):
            last = k == 1
            shifts = [(1 - k) * v for v in dil]
            parts = _nan((nb * ns * cin * cout,), F32); bparts = _nan((nb * ns * cout,), F32)
            K.wgrad(xd.data_ptr(), rows * cin, cin, dd.data_ptr(), rows * cout, cout, shifts, nb, parts, bparts if last else None,
                    rows, T, ns, dt)
            ob, out = _spare(nb * cin, cout, F32)
            K.reduce_partials(parts, ns, cin * cout, nb, True, 1.0, out.data_ptr(), cin * cout)
            what = "wgrad %s %dx%d B %d T %d tap %d" % (NAME[dt], cin, cout, B, T, k)
            got = _intact(what, ob, nb * cin).reshape(nb, cin, cout)
            for l in range(nb):
                a, w = G.wgrad_ops(d["x"][l], d["dy"][l], B, T, shifts[l])
                _exact(what + " layer %d (shift %d)" % (l, shifts[l]), got[l], G.round_out(a @ w, "fp32"))
            if last:
                bb, bout = _spare(nb, cout, F32)
                K.reduce_partials(bparts, ns, cout, nb, True, 1.0, bout.data_ptr(), cout)
                _exact(what + " bias", _intact(what + " bias", bb, nb), G.round_out(d["dy"].sum(1), "fp32"))
            else:
                torch.cuda.synchronize()
                assert bool(torch.isnan(bparts).all()), what + ": bias partials written without a buffer"


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _refused(code, outs, fn, *args):
    with pytest.raises(RuntimeError, match=r"\(code %d\)" % code):
        fn(*args)
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o).all()), "a refused call wrote an output"


@pytest.mark.parametrize("dt", [F32, BF16])
def test_wavenet_layer_fwd_refusals(dt):
    K = sub("kernels"); call = sub("_lib").call
    R, B, T = 32, 2, 33
    d = W.fwd(R, B, T, 1)
    buf, (pc, pr) = _images(dt, R, d["wf"], d["wg"], d["wr"])
    x = _dev(d["x"], dt).view(B, T, R)
    b3 = [_dev(d[k]) for k in ("bf", "bg", "br")]
    outs = [_nan((B, T, R), dt) for _ in range(4)]
    _refused(E_UNSUPPORTED, outs, K.wavenet_layer_fwd, x, None, pc, pr, *b3, *outs, 3, 1)               # K != 2
    _refused(E_SHAPE, outs, K.wavenet_layer_fwd, x, None, pc, pr, *b3, *outs, 2, 0)                     # dilation 0
    o48 = [_nan((B, T, 48), dt) for _ in range(4)]
    z48 = [torch.zeros(48, device=DEV) for _ in range(3)]
    _refused(E_UNSUPPORTED, o48, K.wavenet_layer_fwd, torch.zeros((B, T, 48), dtype=dt, device=DEV), None, pc, pr, *z48, *o48, 2, 1)
    cond = torch.zeros((B, 4, R), dtype=dt, device=DEV)
    _refused(E_SHAPE, outs, K.wavenet_layer_fwd, x, cond, pc, pr, *b3, *outs, 2, 1, 8)                  # 4 frames x 8 < 33
    cond = torch.zeros((B, 5, R + 4), dtype=dt, device=DEV)
    _refused(E_SHAPE, outs, K.wavenet_layer_fwd, x, cond, pc, pr, *b3, *outs, 2, 1, 8)                  # row stride 36
    for (B0, T0) in ((0, T), (B, 0)):
        assert call("srwn_wavenet_layer_fwd", x.data_ptr(), None, pc, pr, *[b.data_ptr() for b in b3],
                    *[o.data_ptr() for o in outs], B0, T0, R, 2, 1, 1, 1, R, K.abi_dtype(dt),
                    torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_wavenet_layer_bwd_refusals(dt):
    K = sub("kernels"); call = sub("_lib").call
    R, S, B, T = 32, 64, 2, 33
    up, dn = W.bwd_up(R, B, T, 1), W.bwd_down(R, S, B, T)
    buf, ptrs = _images(dt, R, up["wf"], up["wg"], dn["wr"], dn["ws"], transposed=True)
    Dd = _dev(up["D"], dt).view(B, T, 2 * R)
    z, s, dcs = (_dev(dn[k], dt).view(B, T, R) for k in ("z", "s", "dcs"))
    dtt = _dev(dn["dtotal"], dt)
    g2, Do = _nan((B, T, R), dt), _nan((B, T, 2 * R), dt)
    outs = [g2, Do]
    bwd = K.wavenet_layer_bwd
    _refused(E_UNSUPPORTED, outs, bwd, None, Dd, ptrs[0], g2, ptrs[1], None, None, dcs, z, s, Do, B, T, R, S, 3, 1, True, True, dt)
    _refused(E_SHAPE, outs, bwd, None, Dd, ptrs[0], g2, ptrs[1], None, None, dcs, z, s, Do, B, T, R, S, 2, 0, True, True, dt)
    _refused(E_NULL, outs, bwd, None, None, None, None, None, None, None, None, z, s, Do, B, T, R, S, 2, 1, False, True, dt)
    _refused(E_NULL, outs, bwd, None, None, None, None, None, ptrs[2], None, None, z, s, Do, B, T, R, S, 2, 1, False, True, dt)
    _refused(E_NULL, outs, bwd, None, None, None, None, None, None, dtt, None, z, s, Do, B, T, R, S, 2, 1, False, True, dt)
    _refused(E_NULL, outs, bwd, None, Dd, ptrs[0], g2, None, None, None, dcs, z, s, Do, B, T, R, S, 2, 1, True, True, dt)
    g48, D48 = _nan((B, T, 48), dt), torch.zeros((B, T, 96), dtype=dt, device=DEV)
    _refused(E_UNSUPPORTED, [g48], bwd, None, D48, ptrs[0], g48, None, None, None, None, None, None, None, B, T, 48, S, 2, 1,
             True, False, dt)
    for (B0, T0) in ((0, T), (B, 0)):
        assert call("srwn_wavenet_layer_bwd", None, Dd.data_ptr(), ptrs[0], g2.data_ptr(), ptrs[1], None, None, dcs.data_ptr(),
                    z.data_ptr(), s.data_ptr(), Do.data_ptr(), B0, T0, R, S, 2, 1, 1, 1, K.abi_dtype(dt),
                    torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs)
