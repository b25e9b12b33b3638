"""GPU tests that hold the MFMA contraction kernels to an integer reference BIT FOR BIT, in fp32 and in bf16, where
max|a - b| / max|b| < 3e-2 lets a single wrong entry, or one row dropped among thousands, pass.

On a dyadic design (tests/gemm_design.py: small integers times a power of two, every sum |a||w| below 2^22 units) every
product and every partial sum is an exact fp32 number, so the result depends on no summation order, MFMA shape, slab cut
or wave count: the kernel's output must equal the float64 reference rounded once (nearest-even) to the output dtype.
tests/test_gemm_design.py proves the designs' conditions on the CPU.  Outputs are poisoned with NaN first; what the
header calls unwritten must keep its poison.

  rowgemm     srwn_pw_linear: every (Cin, Cout) of tests/test_gpu_kernels.py x rows 1, 31, 32, 33, 257 x EPI_NONE / RELU /
              MASK (aux with zeros of both signs) / F32, a spare row behind `rows` keeping its poison; cout_valid < cout_pad; the skip sum over a [L, rows, R] stack with
              PRO_GATE (bf16: z in {-1, 0, 1} gates to 0, 187/256, -69/256 exactly; fp32: bounded); _ychunks; _ksplit
  colgemm     srwn_skip_dgrad_all: (R, S) = (64, 256), (32, 128), L in {1, 3}, rows 1, 33, 257
  head        srwn_head_softmax_ce: logits_out exact for C in {30, 32, 100, 256}; dlogits per entry, padding exactly 0
  wgrad       srwn_wgrad + srwn_reduce_partials: one row, 31 / 32 / 33 rows, one slab plus a row, ragged T with B = 2;
              shifts 0, 1, T - 1, >= T with large values before every clip start; the conditioning add (pool 8 and 16,
              frames that do not divide T); PRO_GATE; bias partials = the exact column sums
  layers      srwn_wgrad_layers: dilations 1, 31, 512, > T; conditioned and not; R = 32 and 64; one row, 31 / 32 / 33 rows,
              two and three slabs with a ragged last one
  wide        srwn_wgrad_wide (srwn_wgrad256) and srwn_wgrad_wide_pair: stacks of z with the gate, flat 256 / 128-wide
              products, 1 / 31 / 32 / 33 rows and one slab plus a row (the pair at the same row counts)
  skip_wt     srwn_wgrad_skip_wt from tiles written here: strides 1, 4, 32, ragged segments, fp32 and bf16 partial blocks
  chain       srwn_head_chain: r1 bit-exact; dlogits, da1, dtotal per entry; both relu masks exact (zeros and exact ties)
  bwd         srwn_residual_layer_bwd, UP only: g2 = conv^T(df_up) bit-exact
  fwd         srwn_residual_layer_fwd: z against tanh of an exact pre-activation, h per entry; dilations 1, 32, 512
  bwd down    srwn_residual_layer_bwd, DOWN only: df per entry on an exact dc; bit-exact at z = 0, absolute at z = +-1
  encoder     srwn_tap_linear (forward taps, backward taps, 1x1 + frame add) and srwn_wgrad_nc_layers, one exact case each

What is not exact (the gate in fp32 mode, tanh, the gate's derivative, the softmax, sqrt(1/2)) is held per entry to
    |got - ref| <= c (u_out |ref| + K 2^-24 S + f_abs),   c = 4 x the float32 NumPy restatement's worst ratio
(tests/gemm_design.py: C_CPU, measured by tests/test_gemm_design.py; never a GPU figure).  SRWN_PRINT_ERR=1 pytest -s
prints what the device reaches.

Worst error / bound scale (bf16 | fp32 where both run):
                         skip_sum_gate  wgrad_gate  softmax_dlogits  chain_product  fwd_z         fwd_h         bwd_df
  float32 NumPy (CPU)    0.105          0.173       1.99             1.97           1.27          1.98          1.99
  C_CPU (rounded up)     0.125          0.1875      2                2              1.5           2             2
  bound = 4 x C_CPU      0.5            0.75        8                8              6             8             8
  MI355X, measured       0.097          0.190       1.99 | 0.30      1.97           1.27 | 0.21   1.98 | 0.09   1.99 | 0.99
(the bf16 outputs: half an ulp is 2^-9 of a binade's upper end and 2^-8 of its lower end, so a
correctly rounded output reaches 2 against u_out = 2^-9; the accumulation adds < 0.01.  wgrad_gate_fp32: the one-row
products, where f_abs is all there is; 0.035 at 90 rows.)

Mutations on scratch builds (in-bounds arithmetic only; never committed): tests of this file that fail / existing
max-norm tests (tests/test_gpu_kernels.py, test_gpu_bwd.py, test_gpu_group.py) that RUN the mutated code and still pass:
  last 16-wide k-slice of the rowgemm loop skipped for one column tile   14 fail / 0 of 13
  rows_valid off by one in a rowgemm tail tile (a row left unwritten)    14 fail / 0 of 12
  final partial 32-row chunk of a srwn_wgrad slab skipped                14 fail / 0 of 10 (4 more never reach such a chunk)
  shifted tap of srwn_wgrad reading across the clip start                14 fail / 0 of 6  (8 more have one clip or no shift)
  (r0 > 0) of the head chain made >=                                      8 fail / 0 of 4
  two k indices swapped in the first row tile of every packed image      72 fail / 0 of 98
  ONE output entry of the rowgemm epilogue off by 3 %                    14 fail / 10 of 12 (every bf16 case)
  ONE row of a srwn_wgrad slab dropped                                   14 fail / 1 of 14  (5000 rows, bf16)
The six mutations of whole tiles, chunks or masks move a dense Gaussian result by more than 3e-2 of its maximum, so the
max-norm tests catch them where they execute the code; what they let through is the single entry, the single row among
thousands, and the shapes they never run (one row, 31 / 33 rows, a slab plus a row, dilation 31, T - 1 shifts).
"""
import os

import numpy as np
import pytest
import torch

from tests import gemm_design as G
from tests._pkg import sub

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAME = {F32: "fp32", BF16: "bf16"}
NAN = float("nan")


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _dev(a, dt=F32):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


def _host(t):
    return t.double().cpu().numpy()


def _nan(shape, dt):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def _exact(what, got, want):
    """got (device tensor or array) equals want (float64, already rounded to the output dtype) bit for bit."""
    got = _host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ok = G.same_bits(got, want)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d entries differ from the integer reference, first at %s: got %r, want %r"
                             % (what, len(bad), ok.size, list(i), got[i], want[i]))


def _bounded(what, key, got, ref, S, K, dtype, f_abs=0.0):
    r = G.ratio(_host(got) if torch.is_tensor(got) else got, ref, S, K, dtype, f_abs)
    assert np.isfinite(r).all(), what
    _say("%-52s %s error / bound scale %.3f (<= %g)" % (what, key, r.max(), G.C_GPU[key]))
    bad = np.argwhere(r > G.C_GPU[key])
    assert len(bad) == 0, "%s: error / bound scale %.3g > %g at %s (%d entries)" % (
        what, r.max(), G.C_GPU[key], bad[0].tolist(), len(bad))


def _image(w, Cin, Cout, cout_pad, dt, transposed=False):
    """The packed MFMA image of w [Cin, Cout] (the integers are exact in dt): (buffer, device pointer)."""
    K = sub("kernels"); P = sub("packing")
    pk = K.Packer(DEV)
    off = P.pack_linear_T(pk, 0, Cin, Cout, cout_pad) if transposed else P.pack_linear(pk, 0, Cin, Cout, cout_pad)
    pk.finalize()
    buf = torch.empty(pk.total, dtype=dt, device=DEV)
    pk.gather(_dev(w).flatten(), buf)
    return buf, buf.data_ptr() + off * buf.element_size()


# ---- the arithmetic assumption ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
def test_smallest_design_one_tile(dt):
    """One 32 x 32 tile, K = 16, integers in +-3: in-range sums are exact in MFMA accumulation.  If a bit-exact case
    below fails while this passes, the kernel is wrong at that case's shape."""
    K = sub("kernels")
    x = G.exact((32, 16), 3, 1.0, 1)
    w = G.exact((16, 32), 3, 1.0, 2)
    G.check_exact(x, w, None, 1.0, 1.0)
    buf, wp = _image(w, 16, 32, 32, dt)
    xd = _dev(x, dt)
    y = _nan((32, 32), dt)
    K.pw_linear(xd.data_ptr(), 16, 0, 16, 16, wp, None, y, 32, 32, 32)
    _exact("32 x 32 x 16", y, G.round_out(x @ w, NAME[dt]))


# ---- srwn_pw_linear -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("Cin,Cout", G.ROWGEMM_SHAPES)
def test_pw_linear_exact(dt, Cin, Cout):
    K = sub("kernels")
    for rows in G.ROWGEMM_ROWS:
        d = G.rowgemm(Cin, Cout, rows)
        buf, wp = _image(d["w"], Cin, Cout, Cout, dt)
        x = _dev(d["x"], dt); b = _dev(d["b"]); aux = _dev(d["aux"], dt)
        zeros = aux[aux == 0]
        assert bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all())      # zeros of both signs arrive
        y0, _ = G.contract(d["x"], d["w"], d["b"])
        want = {K.EPI_NONE: y0, K.EPI_RELU: np.maximum(y0, 0.0), K.EPI_MASK: y0 * (d["aux"] > 0), K.EPI_F32: y0}
        for epi in (K.EPI_NONE, K.EPI_RELU, K.EPI_MASK, K.EPI_F32):
            odt = F32 if epi == K.EPI_F32 else dt
            spare = _nan((rows + 1, Cout), odt)          # one row more than the kernel is told of: it keeps its poison
            y = spare[:rows]
            K.pw_linear(x.data_ptr(), Cin, 0, Cin, Cin, wp, b, y, Cout, Cout, rows, aux=aux if epi == K.EPI_MASK else None,
                        epi=epi, compute_dtype=dt)
            what = "pw_linear %s %dx%d rows %d epi %d" % (NAME[dt], Cin, Cout, rows, epi)
            _exact(what, y, G.round_out(want[epi], NAME[odt]))
            assert bool(torch.isnan(spare[rows]).all()), what + ": the row behind `rows` was written"


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("Cin,Cp,Cv", G.ROWGEMM_VALID)
def test_pw_linear_cout_valid_leaves_the_padding_alone(dt, Cin, Cp, Cv):
    """cout_valid < cout_pad: columns from cout_valid on are not stored (include/srwn.h) and keep their poison.  The entry
    point takes cout_valid in multiples of 4 (its stores are 4 wide) and must refuse 30 of 32 rather than store 32."""
    K = sub("kernels")
    rows = 33
    d = G.rowgemm(Cin, Cp, rows)
    w = d["w"][:, :Cv]
    buf, wp = _image(w, Cin, Cv, Cp, dt)
    x = _dev(d["x"], dt); b = _dev(d["b"][:Cv])
    y0, _ = G.contract(d["x"], w, d["b"][:Cv])
    for epi in (K.EPI_NONE, K.EPI_RELU, K.EPI_F32):
        odt = F32 if epi == K.EPI_F32 else dt
        y = _nan((rows, Cp), odt)
        K.pw_linear(x.data_ptr(), Cin, 0, Cin, Cin, wp, b, y, Cp, Cv, rows, epi=epi, compute_dtype=dt)
        want = np.maximum(y0, 0.0) if epi == K.EPI_RELU else y0
        _exact("pw_linear %d of %d epi %d" % (Cv, Cp, epi), y[:, :Cv], G.round_out(want, NAME[odt]))
        assert bool(torch.isnan(y[:, Cv:]).all()), "columns behind cout_valid were written"
    y = _nan((rows, Cp), dt)
    with pytest.raises(RuntimeError):
        K.pw_linear(x.data_ptr(), Cin, 0, Cin, Cin, wp, _dev(d["b"]), y, Cp, Cv + 2, rows)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("L,R", [(1, 32), (5, 32), (1, 64), (5, 64)])
def test_skip_sum_gate_chunks(dt, L, R):
    """The skip sum: one contraction over a [L, rows, R] stack of z read through chunk strides, c = z sigmoid(z) rebuilt
    in the prologue.  bf16: bit-exact (the gate of -1, 0, 1 is on the grid 1/256); fp32: per entry."""
    K = sub("kernels"); P = sub("packing")
    S = 4 * R
    for (L_, R_, S_, rows) in [c for c in G.SKIPSUM if c[:2] == (L, R)]:
        d = G.skipsum(L, R, S, rows)
        pk = K.Packer(DEV)
        off = pk.reserve(S // 32, L * R // 16)
        for l in range(L):
            P.fill_linear(pk, off, l * R * S, R, S, S // 32, L * R // 16, ks_offset=l * R // 16, ks_count=R // 16)
        pk.finalize()
        buf = torch.empty(pk.total, dtype=dt, device=DEV); pk.gather(_dev(d["w"]).flatten(), buf)
        z = _dev(d["z"], dt)
        za = G.skipsum_a(d["z"])
        for epi in (K.EPI_NONE, K.EPI_RELU):
            y = _nan((rows, S), dt)
            K.pw_linear(z.data_ptr(), R, rows * R, R, L * R, buf.data_ptr() + off * buf.element_size(), _dev(d["b"]), y, S, S,
                        rows, pro=K.PRO_GATE, epi=epi)
            what = "skip sum %s L %d R %d rows %d epi %d" % (NAME[dt], L, R, rows, epi)
            if dt == BF16:
                y0, _ = G.contract(G.gated(za), d["w"], d["b"])
                _exact(what, y, G.round_out(np.maximum(y0, 0.0) if epi else y0, "bf16"))
            else:
                ref, Sm = G.contract(G.gate64(za), d["w"], d["b"])
                _bounded(what, "skip_sum_gate_fp32", y, np.maximum(ref, 0.0) if epi else ref, Sm, L * R, "fp32",
                         G.f_abs_gate32() * np.abs(d["w"]).sum(0))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_pw_linear_ychunks_exact(dt):
    """Outputs stored layer by layer ([L][rows][R]); 200 rows take the one-row-tile launch, 3 layers x 64 channels."""
    K = sub("kernels"); call = sub("_lib").call
    L, R, Cin, rows = G.YCHUNKS
    d = G.rowgemm(Cin, L * R, rows)
    buf, wp = _image(d["w"], Cin, L * R, L * R, dt)
    x = _dev(d["x"], dt); b = _dev(d["b"])
    y = _nan((L, rows, R), dt)
    call("srwn_pw_linear_ychunks", x.data_ptr(), Cin, Cin, wp, b.data_ptr(), y.data_ptr(), R, R, rows * R, L * R, L * R, rows,
         K.abi_dtype(dt), torch.cuda.current_stream().cuda_stream)
    y0, _ = G.contract(d["x"], d["w"], d["b"])
    want = G.round_out(y0, NAME[dt]).reshape(rows, L, R).transpose(1, 0, 2)
    _exact("ychunks %s" % NAME[dt], y, want)


@pytest.mark.parametrize("dt", [F32, BF16])
def test_pw_linear_ksplit_partials_exact(dt):
    """The contraction split over k: every fp32 partial is the exact sum of its own k-slice (bias in slice 0), and
    srwn_reduce_partials finishes the exact product."""
    K = sub("kernels"); call = sub("_lib").call
    L, EC, S, rows = G.KSPLIT
    d = G.ksplit(L, EC, S, rows)
    x, w, b = d["x"], d["w"], d["b"]
    a = G.skipsum_a(x)
    buf, wp = _image(w, L * EC, S, S, dt)
    xd = _dev(x, dt)
    parts = _nan((L, rows, S), F32)
    call("srwn_pw_linear_ksplit", xd.data_ptr(), EC, rows * EC, EC, L * EC, wp, _dev(b).data_ptr(), parts.data_ptr(), S, S, S,
         rows, L, K.abi_dtype(dt), torch.cuda.current_stream().cuda_stream)
    for l in range(L):
        want = x[l] @ w[l * EC:(l + 1) * EC] + (b if l == 0 else 0.0)
        _exact("ksplit %s slice %d" % (NAME[dt], l), parts[l], G.round_out(want, "fp32"))
    out = _nan((rows, S), F32)
    K.reduce_partials(parts.view(-1), L, rows * S, 1, True, 1.0, out.data_ptr(), 0)
    _exact("ksplit %s reduced" % NAME[dt], out, G.round_out(a @ w + b, "fp32"))


# ---- srwn_skip_dgrad_all ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R,S", [(64, 256), (32, 128)])
def test_skip_dgrad_all_exact(dt, R, S):
    K = sub("kernels"); P = sub("packing")
    for (R_, S_, L, rows) in [c for c in G.COLGEMM if c[:2] == (R, S)]:
        d = G.colgemm(R, S, L, rows)
        pk = K.Packer(DEV)
        per = (R // 32) * (S // 16) * 512
        o_all = pk.reserve(L * (R // 32), S // 16)
        for l in range(L):
            P.fill_linear_T(pk, o_all + l * per, l * R * S, R, S, R // 32, S // 16)
        pk.finalize()
        buf = torch.empty(pk.total, dtype=dt, device=DEV); pk.gather(_dev(d["ws"]).flatten(), buf)
        dcs = _nan((L, rows, R), dt)
        K.skip_dgrad_all(_dev(d["d"], dt), buf.data_ptr() + o_all * buf.element_size(), dcs, R, S)
        for l in range(L):
            _exact("skip_dgrad_all %s R %d L %d rows %d layer %d" % (NAME[dt], R, L, rows, l), dcs[l],
                   G.round_out(d["d"] @ d["ws"][l].T, NAME[dt]))


# ---- srwn_head_softmax_ce -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("C", G.HEAD_CLASSES)
def test_head_softmax_ce_entries(dt, C):
    """logits_out: the fp32 output of an exact contraction, bit for bit.  dlogits per entry against the softmax of the
    exact logits (its condition is the softmax's own: S = (p + onehot) |scale|, K = C terms of the normaliser); padding
    columns exactly 0."""
    K = sub("kernels")
    rows, S = G.HEAD_ROWS, 64
    Cp = (C + 31) // 32 * 32
    d = G.head(C)
    buf, wp = _image(d["w"], S, C, Cp, dt)
    parts = torch.zeros((rows + 31) // 32, dtype=F32, device=DEV)
    dl = _nan((rows, Cp), dt); lo = _nan((rows, C), F32)
    scale = 1.0 / rows
    K.head_softmax_ce(_dev(d["x"], dt), wp, _dev(d["b"]), _dev(d["tg"], torch.int32), parts, dl, lo, Cp, C, scale)
    logits, _ = G.contract(d["x"], d["w"], d["b"])
    _exact("head logits %s C %d" % (NAME[dt], C), lo, G.round_out(logits, "fp32"))
    ref, Sm, p = G.dlogits_ref(logits, d["tg"], scale)
    _bounded("head dlogits %s C %d" % (NAME[dt], C), "softmax_dlogits", dl[:, :C], ref, Sm, C, NAME[dt])
    assert bool((dl[:, C:] == 0).all()), "padding columns of dlogits"


# ---- srwn_wgrad ---------------------------------------------------------------------------------------------------------
def _slab_rows(slabs_fn):
    """The longest row count one slab takes, from the entry point itself."""
    lo, hi = 1, 1 << 20
    assert slabs_fn(lo) == 1 and slabs_fn(hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if slabs_fn(mid) == 1 else (lo, mid)
    return lo


def _wgrad_run(K, dt, x, dy, B, T, shifts, pro, **cond):
    nb, rows, cin = x.shape
    cout = dy.shape[-1]
    ns = K.wgrad_slabs(rows)
    parts = _nan((nb * ns * cin * cout,), F32); bparts = _nan((nb * ns * cout,), F32)
    xd, dd = _dev(x, dt), _dev(dy, dt)
    K.wgrad(xd.data_ptr(), rows * cin, cin, dd.data_ptr(), rows * cout, cout, shifts, nb, parts, bparts, rows, T, ns, dt,
            pro=pro, **cond)
    out = _nan((nb, cin, cout), F32); bout = _nan((nb, cout), F32)
    K.reduce_partials(parts, ns, cin * cout, nb, True, 0.5, out.data_ptr(), cin * cout)
    K.reduce_partials(bparts, ns, cout, nb, True, 1.0, bout.data_ptr(), cout)
    return out, bout, ns


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("cin,cout", G.WGRAD_SHAPES)
def test_wgrad_exact(dt, cin, cout):
    """Rows across every cut (one row; 31 / 32 / 33; ragged T with two clips; one slab plus a row), shifts 0, 1, T - 1 and
    beyond T, values of 15 before every clip start where the rest is <= 3.  fp32 partials, the reduce scale a power of
    two: everything exact, the bias partials' sums included."""
    K = sub("kernels")
    slab = _slab_rows(K.wgrad_slabs)
    assert slab == 3072, "tests/gemm_design.py:cases() checks the design of a 3072-row slab"
    for (B, T) in G.wgrad_clips(slab + 1):
        d = G.wgrad(cin, cout, B, T)
        shifts = G.wgrad_shifts(T)
        out, bout, ns = _wgrad_run(K, dt, d["x"], d["dy"], B, T, shifts, K.PRO_NONE)
        assert ns == (2 if B * T > slab else 1)
        for l, sh in enumerate(shifts):
            a, w = G.wgrad_ops(d["x"][l], d["dy"][l], B, T, sh)
            what = "wgrad %s %dx%d B %d T %d shift %d" % (NAME[dt], cin, cout, B, T, sh)
            _exact(what, out[l], G.round_out(0.5 * (a @ w), "fp32"))
            _exact(what + " bias", bout[l], G.round_out(d["dy"][l].sum(0), "fp32"))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_wgrad_gate(dt):
    """PRO_GATE: bf16 exact on z in {-1, 0, 1}; fp32 per entry."""
    K = sub("kernels")
    B, T, cin, cout = 2, 45, 64, 64
    d = G.wgrad(cin, cout, B, T, gate=True)
    shifts = G.wgrad_shifts(T)
    out, bout, _ = _wgrad_run(K, dt, d["x"], d["dy"], B, T, shifts, K.PRO_GATE)
    for l, sh in enumerate(shifts):
        what = "wgrad gate %s shift %d" % (NAME[dt], sh)
        if dt == BF16:
            a, w = G.wgrad_ops(G.gated(d["x"][l]), d["dy"][l], B, T, sh)
            _exact(what, out[l], G.round_out(0.5 * (a @ w), "fp32"))
        else:
            a, w = G.wgrad_ops(G.gate64(d["x"][l]), d["dy"][l], B, T, sh)
            ref, Sm = G.contract(a, w)
            _bounded(what, "wgrad_gate_fp32", out[l], 0.5 * ref, 0.5 * Sm, B * T, "fp32",
                     0.5 * G.f_abs_gate32() * np.abs(w).sum(0))
        _exact(what + " bias", bout[l], G.round_out(d["dy"][l].sum(0), "fp32"))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("pool,frames", G.WGRAD_POOLS)
def test_wgrad_cond_exact(dt, pool, frames):
    """The conditioning add: x + cond[frame] is exact in bf16 by design; frames * pool > T, T no multiple of pool."""
    K = sub("kernels")
    B, T, cin, cout, shift = G.WGRAD_COND
    d = G.wgrad_cond(cin, cout, B, T, pool, frames)
    xin = d["x"][0] + G.pool_rows(d["cond"], B, T, pool)
    assert G.is_bf16(xin)
    cb = _dev(d["cond"], dt)
    out, bout, _ = _wgrad_run(K, dt, d["x"], d["dy"], B, T, [shift], K.PRO_NONE, cond_ptr=cb.data_ptr(),
                              cond_frames=frames, pool_stride=pool)
    a, w = G.wgrad_ops(xin, d["dy"][0], B, T, shift)
    _exact("wgrad cond %s pool %d" % (NAME[dt], pool), out[0], G.round_out(0.5 * (a @ w), "fp32"))
    _exact("wgrad cond %s pool %d bias" % (NAME[dt], pool), bout[0], G.round_out(d["dy"][0].sum(0), "fp32"))


# ---- srwn_wgrad_layers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R,B,T,pool,nslabs", G.LAYERS)
def test_wgrad_layers_exact(dt, R, B, T, pool, nslabs):
    """Conv taps + residual 1x1 gradients of four layers in one pass: dilations 1, 31, 512 and beyond T; ragged T with two
    clips and large values before the clip start; the conditioning add with pool 8 / 16 and frames that do not divide T;
    one row and 31 / 32 / 33 rows (a second row group of bf16 mode with nothing to do, for both staging widths); two and
    three slabs whose last one is ragged (the entry point takes any slab count).
    Conv-tap gradients and bias sums are exact in both dtypes; the residual gradient (gate prologue) is exact in bf16 and
    held per entry in fp32."""
    K = sub("kernels")
    L, rows = 4, B * T
    dil = G.layer_dilations(T)
    d = G.layers(R, B, T, pool)
    x, z, df, g = (_dev(d[k], dt) for k in ("x", "z", "df", "g"))
    ns = nslabs or K.wgrad_slabs(rows)
    assert ns == (nslabs or 1)
    if nslabs:      # the last slab is ragged: neither empty nor whole
        kr = 32 if R == 64 else 64
        rps = -(-(-(-rows // ns)) // kr) * kr
        assert 0 < rows - (ns - 1) * rps < rps and (rows - (ns - 1) * rps) % kr
    pf = _nan((L * ns * 2 * R * R,), F32); pr = _nan((L * ns * R * R,), F32)
    pbf = _nan((L * ns * R,), F32); pbr = _nan((L * ns * R,), F32)
    ckw = {}
    if pool:
        cond = _dev(d["cond"], dt)
        ckw = dict(cond_ptr=cond.data_ptr(), cond_layer_stride=R, cond_frames=d["frames"], pool_stride=pool, cond_row_stride=L * R)
    K.wgrad_layers(x, z, df, g.data_ptr(), dil, pf, pr, pbf, pbr, T, ns, **ckw)
    of = _nan((L, 2, R, R), F32); orr = _nan((L, R, R), F32); obf = _nan((L, R), F32); obr = _nan((L, R), F32)
    K.reduce_partials(pf, ns, 2 * R * R, L, True, 1.0, of.data_ptr(), 2 * R * R)
    K.reduce_partials(pr, ns, R * R, L, True, 0.5, orr.data_ptr(), R * R)
    K.reduce_partials(pbf, ns, R, L, True, 1.0, obf.data_ptr(), R)
    K.reduce_partials(pbr, ns, R, L, True, 1.0, obr.data_ptr(), R)
    for l in range(L):
        what = "wgrad_layers %s R %d T %d pool %s layer %d (dilation %d)" % (NAME[dt], R, T, pool, l, dil[l])
        ops = G.layers_ops(d, l, B, T, R, pool, dil[l])
        for k in range(2):
            _exact(what + " tap %d" % k, of[l, k], G.round_out(ops[k][0] @ ops[k][1], "fp32"))
        if dt == BF16:
            _exact(what + " residual", orr[l], G.round_out(0.5 * (ops[2][0] @ ops[2][1]), "fp32"))
        else:
            ref, Sm = G.contract(G.gate64(d["z"][l]).T, d["g"][l])
            _bounded(what + " residual", "wgrad_gate_fp32", orr[l], 0.5 * ref, 0.5 * Sm, rows, "fp32",
                     0.5 * G.f_abs_gate32() * np.abs(d["g"][l]).sum(0))
        _exact(what + " bias f", obf[l], G.round_out(d["df"][l].sum(0), "fp32"))
        _exact(what + " bias r", obr[l], G.round_out(d["g"][l].sum(0), "fp32"))


# ---- srwn_wgrad_wide / srwn_wgrad256 / srwn_wgrad_wide_pair -------------------------------------------------------------
def _wide_run(K, dt, mode, cw, dw, L, rows, d):
    ns = K.wgrad256_slabs(rows, L, cw)
    parts = _nan((ns * L * cw * dw,), F32); bparts = _nan((ns * dw,), F32)
    a = _dev(d["a"], dt); dd = _dev(d["d"], dt)
    if mode == "stack":
        K.wgrad256(a.data_ptr(), rows * cw, cw, L, dd, parts, bparts, rows, ns, pro=K.PRO_GATE, chunk_width=cw)
    else:
        K.wgrad256(a.data_ptr(), cw, L * cw, L, dd, parts, bparts, rows, ns, chunk_width=cw)
    out = _nan((L * cw, dw), F32); bout = _nan((dw,), F32)
    K.reduce_partials(parts, ns, L * cw * dw, 1, True, 2.0, out.data_ptr(), 0)
    K.reduce_partials(bparts, ns, dw, 1, True, 1.0, bout.data_ptr(), 0)
    return out, bout, ns


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("mode,cw,dw,L", G.WIDE)
def test_wgrad_wide_exact(dt, mode, cw, dw, L):
    """The wide weight-gradient GEMM (all skip 1x1s at once over a stack of z with the gate prologue, and the head's
    256 / 128-wide products): one row, 31 / 32 / 33 rows, one slab plus a row.  bf16: exact; fp32 with the gate: per entry."""
    K = sub("kernels")
    slab = _slab_rows(lambda n: K.wgrad256_slabs(n, L, cw))
    assert slab == 256, "tests/gemm_design.py:cases() checks the design of a 256-row slab"
    for rows in G.WIDE_ROWS + [slab + 1]:
        d = G.wide(mode, cw, dw, L, rows)
        out, bout, ns = _wide_run(K, dt, mode, cw, dw, L, rows, d)
        assert ns == (2 if rows > slab else 1)
        what = "wgrad_wide %s %s %d x %d, %d chunks, rows %d" % (NAME[dt], mode, cw, dw, L, rows)
        if mode == "flat":
            _exact(what, out, G.round_out(2.0 * (d["a"].T @ d["d"]), "fp32"))
        elif dt == BF16:
            _exact(what, out, G.round_out(2.0 * (G.gated(G.skipsum_a(d["a"])).T @ d["d"]), "fp32"))
        else:
            ref, Sm = G.contract(G.gate64(G.skipsum_a(d["a"])).T, d["d"])
            _bounded(what, "wgrad_gate_fp32", out, 2.0 * ref, 2.0 * Sm, rows, "fp32", 2.0 * G.f_abs_gate32() * np.abs(d["d"]).sum(0))
        _exact(what + " bias", bout, G.round_out(d["d"].sum(0), "fp32"))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("rows", G.WIDE_PAIR_ROWS)
def test_wgrad_wide_pair_exact(dt, rows):
    """Two 256 x 256 products as one launch: each equals its own integer reference."""
    K = sub("kernels")
    d0 = G.wide("flat", 64, 256, 4, rows)
    d1 = G.wide("flat", 64, 256, 4, rows, variant=1)
    ns = K.wgrad256_slabs(rows, 4)
    p = [_nan((ns * 256 * 256,), F32) for _ in range(2)]; bp = [_nan((ns * 256,), F32) for _ in range(2)]
    a0, a1, e0, e1 = _dev(d0["a"], dt), _dev(d1["a"], dt), _dev(d0["d"], dt), _dev(d1["d"], dt)
    K.wgrad256_pair(a0.data_ptr(), e0, p[0], bp[0], a1.data_ptr(), e1, p[1], bp[1], 64, 256, 4, rows, ns)
    for i, d in enumerate((d0, d1)):
        out = _nan((256, 256), F32); bout = _nan((256,), F32)
        K.reduce_partials(p[i], ns, 256 * 256, 1, True, 1.0, out.data_ptr(), 0)
        K.reduce_partials(bp[i], ns, 256, 1, True, 1.0, bout.data_ptr(), 0)
        _exact("wgrad_wide_pair %s rows %d product %d" % (NAME[dt], rows, i), out, G.round_out(d["a"].T @ d["d"], "fp32"))
        _exact("wgrad_wide_pair %s rows %d bias %d" % (NAME[dt], rows, i), bout, G.round_out(d["d"].sum(0), "fp32"))


# ---- srwn_head_chain ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", G.CHAIN_ROWS)
@pytest.mark.parametrize("C", [256, 250])
def test_head_chain_entries(rows, C):
    """r1 = relu(r0 W1 + b1) bit for bit (the design puts exact zeros into r0 and pre-activations of exactly 0 into r1);
    dlogits per entry against the softmax of the exact logits; da1 and dtotal per entry, each against the exact product of
    the operand THE KERNEL STORED (its bf16 dlogits, its bf16 da1: the rounding points of csrc/srwn_head.hip), so that the
    only error left is the fp32 accumulation and the output rounding; masked entries exactly 0."""
    K = sub("kernels"); P = sub("packing")
    S = 256
    d = G.chain(rows, C)
    pre, r1_ref, logits = G.chain_forward(d)
    assert (pre == 0).sum() >= S // 2 and (d["r0"] == 0).any()      # every second column by design; r0 is drawn with zeros
    pk = K.Packer(DEV)
    o1 = P.pack_linear(pk, 0, S, S, S)
    o2p = P.pack_linear(pk, S * S, S, 256, 256, perm=True)
    o2Tp = P.pack_linear_T(pk, S * S, S, 256, S, perm=True)
    o1Tp = P.pack_linear_T(pk, 0, S, S, S, perm=True)
    pk.finalize()
    buf = torch.empty(pk.total, dtype=BF16, device=DEV)
    pk.gather(torch.cat([_dev(d["w1"]).flatten(), _dev(d["w2"]).flatten()]), buf)
    wp = lambda o: buf.data_ptr() + 2 * o
    parts = torch.zeros((rows + 31) // 32, dtype=F32, device=DEV)
    r1, dl, da1, dtot = (_nan((rows, S), BF16) for _ in range(4))
    scale = 1.0 / rows
    K.head_chain(_dev(d["r0"], BF16), wp(o1), wp(o2p), wp(o2Tp), wp(o1Tp), _dev(d["b1"]), _dev(d["b2"]),
                 _dev(d["tg"], torch.int32), parts, r1, dl, da1, dtot, C, scale)
    what = "head_chain rows %d C %d" % (rows, C)
    _exact(what + " r1", r1, r1_ref)
    ref, Sm, p = G.dlogits_ref(logits[:, :C], d["tg"], scale)
    _bounded(what + " dlogits", "softmax_dlogits", dl[:, :C], ref, Sm, C, "bf16")
    assert bool((dl[:, C:] == 0).all()), "padding columns of dlogits"
    dlq = _host(dl)
    ref, Sm = G.contract(dlq, d["w2"].T)
    m1 = r1_ref > 0
    _bounded(what + " da1", "chain_product", da1, ref * m1, Sm, 256, "bf16")
    assert bool((da1[torch.tensor(~m1, device=DEV)] == 0).all()), "da1 behind the mask (r1 > 0)"
    ref, Sm = G.contract(_host(da1), d["w1"].T)
    m0 = d["r0"] > 0
    _bounded(what + " dtotal", "chain_product", dtot, ref * m0, Sm, 256, "bf16")
    assert bool((dtot[torch.tensor(~m0, device=DEV)] == 0).all()), "dtotal behind the mask (r0 > 0)"


# ---- srwn_residual_layer_bwd, UP only -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", [32, 64])
def test_residual_layer_bwd_up_exact(dt, R):
    """g2 = conv^T(df_up): both taps of the upper layer's conv as one 2R-deep contraction; dilations 1, 32 and beyond T."""
    K = sub("kernels"); P = sub("packing")
    for (R_, B, T, dil) in [c for c in G.BWD_UP if c[0] == R]:
        d = G.bwd_up(R, B, T, dil)
        pk = K.Packer(DEV); oc = P.pack_conv_T(pk, 0, 2, R); pk.finalize()
        buf = torch.empty(pk.total, dtype=dt, device=DEV); pk.gather(_dev(d["wf"]).flatten(), buf)
        g2 = _nan((B, T, R), dt)
        K.residual_layer_bwd(None, _dev(d["df"], dt).view(B, T, R), buf.data_ptr() + oc * buf.element_size(), g2, None, None,
                             None, None, None, B, T, R, 4 * R, 2, dil, True, False, dt)
        a, w = G.bwd_up_ops(d, B, T, dil)
        _exact("residual_layer_bwd UP %s R %d B %d T %d dilation %d" % (NAME[dt], R, B, T, dil), g2.view(B * T, R),
               G.round_out(a @ w, NAME[dt]))


# ---- srwn_wgrad_skip_wt -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part16", [False, True])
@pytest.mark.parametrize("B,T,st,seg", G.SKIP_WT)
def test_wgrad_skip_wt_exact(part16, B, T, st, seg):
    """The skip weight gradients contracted from transposed gate tiles written here from a designed c (the layout of
    csrc/srwn_group.h, encoded by tests/gemm_design.py): strides 1, 4, 32, segment lengths that are no multiple of 32, two
    clips of a ragged T.  fp32 partials and bf16 16 x 16 partial blocks (sparse design: every possible partial sum is
    exact in bf16) are both bit-exact after the reduction; tile elements beyond a segment's length hold 256 and must not
    count; the bias partials are the exact column sums."""
    K = sub("kernels")
    L, R, S = len(st), 64, 256
    d = G.skip_wt(B, T, L, part16)
    tiles = [G.ct_encode(d["c"][l], B, T, R, st[l], seg[l], G.CT_POISON) for l in range(L)]
    elems = max(t.size for t in tiles)
    cT = torch.full((L, elems), G.CT_POISON, dtype=BF16, device=DEV)
    for l in range(L):
        cT[l, :tiles[l].size] = _dev(tiles[l], BF16)
    ns = K.wgrad_skip_wt_slabs(st, seg, T)
    assert ns >= 1
    parts = _nan((ns * L * R * S,), BF16 if part16 else F32)
    bparts = _nan((ns * S,), F32)
    K.wgrad_skip_wt(cT, st, seg, _dev(d["d"], BF16), parts, bparts, ns, B, T, R)
    out = _nan((L * R, S), F32); bout = _nan((S,), F32)
    job = (parts, ns, L * R * S, 1, True, 1.0, out.data_ptr(), 0)
    K.reduce_partials_multi([job + (S,) if part16 else job, (bparts, ns, S, 1, True, 1.0, bout.data_ptr(), 0)])
    for l in range(L):
        _exact("wgrad_skip_wt B %d T %d part16 %d layer %d (st %d, segments of %d)" % (B, T, part16, l, st[l], seg[l]),
               out[l * R:(l + 1) * R], G.round_out(d["c"][l].T @ d["d"], "fp32"))
    _exact("wgrad_skip_wt bias", bout, G.round_out(d["d"].sum(0), "fp32"))


# ---- the encoder's kernels: srwn_tap_linear, srwn_wgrad_nc_layers -------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("cout", [128, 256])
def test_tap_linear_exact(dt, cout):
    """The time-tap GEMM at the shapes of tests/test_gpu_autoencoder.py: the K = 2 conv forward (relu), its taps backwards
    in time (masked), and a 1x1 with the per-frame fp32 broadcast (times 1/2) added before the mask."""
    K = sub("kernels"); P = sub("packing"); call = sub("_lib").call
    B, T, Cin, pool = G.TAP
    frames, rows = T // pool, B * T
    d = G.tap(cout)
    pk = K.Packer(DEV)
    off = pk.reserve(cout // 32, 2 * Cin // 16)
    P.fill_linear(pk, off, 0, 2 * Cin, cout, cout // 32, 2 * Cin // 16)
    offT = pk.reserve(cout // 32, Cin // 16)
    P.fill_linear(pk, offT, 0, Cin, cout, cout // 32, Cin // 16)
    pk.finalize()
    packed = torch.zeros(pk.total, dtype=dt, device=DEV); pk.gather(_dev(d["w"].reshape(-1)), packed)
    es = packed.element_size()
    x = _dev(d["x"], dt); b = _dev(d["b"]); aux = _dev(d["aux"], dt); fadd = _dev(d["fadd"])
    mask = d["aux"] > 0

    def run(ntaps, step, wp, bias, aux_, fadd_, fscale, epi):
        y = _nan((rows, cout), dt)
        call("srwn_tap_linear", x.data_ptr(), Cin, ntaps, step, T, Cin, wp, None if bias is None else bias.data_ptr(),
             y.data_ptr(), cout, cout, rows, None if aux_ is None else aux_.data_ptr(), cout,
             None if fadd_ is None else fadd_.data_ptr(), 0 if fadd_ is None else fadd_.shape[-1], frames if fadd_ is not None
             else 1, pool if fadd_ is not None else 1, fscale, epi, K.abi_dtype(dt), torch.cuda.current_stream().cuda_stream)
        return y

    a, w = G.tap_ops(d, 1)
    _exact("tap_linear %s %d forward" % (NAME[dt], cout), run(2, 1, packed.data_ptr() + off * es, b, None, None, 0.0, K.EPI_RELU),
           G.round_out(np.maximum(a @ w + d["b"], 0.0), NAME[dt]))
    a, w = G.tap_ops(d, -1)
    _exact("tap_linear %s %d backward" % (NAME[dt], cout), run(2, -1, packed.data_ptr() + off * es, None, aux, None, 0.0, K.EPI_MASK),
           G.round_out((a @ w) * mask, NAME[dt]))
    fa = G.pool_rows(d["fadd"].reshape(B, frames, -1)[:, :, :cout], B, T, pool)
    _exact("tap_linear %s %d 1x1 + frame add" % (NAME[dt], cout),
           run(1, 0, packed.data_ptr() + offT * es, b, aux, fadd, 0.5, K.EPI_MASK),
           G.round_out((d["x"] @ d["w"][0] + d["b"] + 0.5 * fa) * mask, NAME[dt]))


@pytest.mark.parametrize("dt", [F32, BF16])
def test_wgrad_nc_layers_exact(dt):
    """Both conv taps (t and t + 1 inside the clip), the 1x1 and the two bias gradients of every encoder layer."""
    K = sub("kernels"); call = sub("_lib").call
    L, B, T, C, ns = G.NC
    rows = B * T
    d = G.nc()
    r, a, dp, dh = (_dev(d[k], dt) for k in ("r", "a", "dp", "dh"))
    pw, pr, pb, pbr = _nan((L * ns * 2 * C * C,), F32), _nan((L * ns * C * C,), F32), _nan((L * ns * C,), F32), _nan((L * ns * C,), F32)
    call("srwn_wgrad_nc_layers", r.data_ptr(), a.data_ptr(), dp.data_ptr(), dh.data_ptr(), rows * C, L, pw.data_ptr(),
         pr.data_ptr(), pb.data_ptr(), pbr.data_ptr(), rows, T, ns, C, 2, K.abi_dtype(dt), torch.cuda.current_stream().cuda_stream)
    ow, orr, ob, obr = _nan((L, 2, C, C), F32), _nan((L, C, C), F32), _nan((L, C), F32), _nan((L, C), F32)
    K.reduce_partials(pw, ns, 2 * C * C, L, True, 1.0, ow.data_ptr(), 2 * C * C)
    K.reduce_partials(pr, ns, C * C, L, True, 1.0, orr.data_ptr(), C * C)
    K.reduce_partials(pb, ns, C, L, True, 1.0, ob.data_ptr(), C)
    K.reduce_partials(pbr, ns, C, L, True, 1.0, obr.data_ptr(), C)
    for l in range(L):
        ops = G.nc_ops(d, l)
        what = "wgrad_nc_layers %s layer %d" % (NAME[dt], l)
        _exact(what + " tap 0", ow[l, 0], G.round_out(ops[0][0] @ ops[0][1], "fp32"))
        _exact(what + " tap 1", ow[l, 1], G.round_out(ops[1][0] @ ops[1][1], "fp32"))
        _exact(what + " 1x1", orr[l], G.round_out(ops[2][0] @ ops[2][1], "fp32"))
        _exact(what + " bias", ob[l], G.round_out(d["dp"][l].sum(0), "fp32"))
        _exact(what + " bias r", obr[l], G.round_out(d["dh"][l].sum(0), "fp32"))


# ---- srwn_residual_layer_fwd --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", [32, 64])
def test_residual_layer_fwd_entries(dt, R):
    """An exact pre-activation f on the grid 1/4 in [-2.25, 2.25] (one weight of +-1/4 per tap and column): z against
    tanh(f) per entry -- the contraction contributes no error -- and h per entry; in bf16 mode the c that enters the
    residual 1x1 is rounded where the kernel rounds it, the same bits for any tanh (tests/gemm_design.py:fwd_c_bf16), so
    the residual product is exact too and only sqrt(1/2) and the output rounding remain.  Dilations 1, 32, 512; T 33, 513."""
    K = sub("kernels"); P = sub("packing")
    mode = NAME[dt]
    for (R_, B, T, dil) in [c for c in G.FWD if c[0] == R]:
        d = G.fwd_layer(R, B, T, dil)
        f = G.fwd_pre(d, B, T, dil)
        pk = K.Packer(DEV)
        oc = P.pack_conv(pk, 0, 2, R)
        orr = P.pack_res(pk, 2 * R * R, R)
        pk.finalize()
        buf = torch.empty(pk.total, dtype=dt, device=DEV)
        pk.gather(torch.cat([_dev(d["wf"]).flatten(), _dev(d["wr"]).flatten()]), buf)
        es = buf.element_size()
        h = _nan((B, T, R), dt); z = _nan((B, T, R), dt)
        K.residual_layer_fwd(_dev(d["x"], dt).view(B, T, R), None, buf.data_ptr() + oc * es, buf.data_ptr() + orr * es,
                             _dev(d["bf"]), _dev(d["br"]), h, z, 2, dil)
        what = "residual_layer_fwd %s R %d B %d T %d dilation %d" % (mode, R, B, T, dil)
        _bounded(what + " z", "fwd_z", z.view(B * T, R), np.tanh(f), 0.0, 0, mode, G.f_abs_tanh(mode))
        ref, Sm, fa = G.fwd_h_ref(d, f, mode)
        _bounded(what + " h", "fwd_h", h.view(B * T, R), ref, Sm, R, mode, fa)
        assert bool((z.view(B * T, R)[torch.tensor(f == 0, device=DEV)] == 0).all())      # tanh(0) = 0 exactly


# ---- srwn_residual_layer_bwd, DOWN only ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R,S,B,T", G.BWD_DOWN)
def test_residual_layer_bwd_df_entries(dt, R, S, B, T):
    """df = (dtotal Ws^T) d(z sigmoid z)/df with an exact dc and z in {-1, -1/2, 0, 1/2, 1}: per entry; where z = 0 the
    derivative is exactly 1/2 and df is bit-exact; where z = +-1 (1 - z^2 = 0) df is bounded absolutely by the
    derivative's own error times |dc|."""
    K = sub("kernels"); P = sub("packing")
    mode = NAME[dt]
    d = G.bwd_down(R, S, B, T)
    pk = K.Packer(DEV); osk = P.pack_linear_T(pk, 0, R, S, R); pk.finalize()
    buf = torch.empty(pk.total, dtype=dt, device=DEV); pk.gather(_dev(d["ws"]).flatten(), buf)
    df = _nan((B, T, R), dt)
    K.residual_layer_bwd(None, None, None, None, None, buf.data_ptr() + osk * buf.element_size(), _dev(d["d"], dt),
                         _dev(d["z"], dt).view(B, T, R), df, B, T, R, S, 2, 1, False, True, dt)
    dc, _ = G.contract(d["d"], d["ws"].T)
    got = _host(df).reshape(B * T, R)
    what = "residual_layer_bwd DOWN %s R %d S %d B %d T %d" % (mode, R, S, B, T)
    _bounded(what, "bwd_df", got, dc * G.dgate64(d["z"]), 0.0, 0, mode, G.f_abs_dgate(mode) * np.abs(dc))
    z0 = d["z"] == 0
    _exact(what + " at z = 0", got[z0], G.round_out(0.5 * dc, mode)[z0])
    if dt == F32:
        assert (got[np.abs(d["z"]) == 1] == 0).all()          # (s + z s (1 - s)) * (1 - 1) is an exact zero
