"""GPU tests that hold the fused encoder layer kernels (csrc/srwn_nc.hip: srwn_nc_layer_fwd, srwn_nc_layer_bwd,
srwn_nc_mask_bits) to a layer-local float64 reference ENTRY BY ENTRY, where tests/test_gpu_autoencoder.py judges them by
max|a - b| / max|b| against a twin that shares their packers, wiring and roundings, at <= 16 tiles.

On the chained exact designs of tests/nc_design.py (proved on the CPU by tests/test_nc_design.py) the first product of a
kernel lands on bf16 numbers and the second stays below 2^22 units, so a_out, r_out, dh_out and dpre_out must equal the
float64 reference rounded once to bf16, bit for bit, in every variant the entry points have:

  forward    with the residual product and without (the last layer); a_bits / r_bits given and None
  backward   dpre_out None; given without frame_add; given with frame_add at pool 32, 25 (frames change inside a tile), 1
             and > T, frames * pool > T, tables wider than 128 read at a column offset, a scale that is not 1 / pool
  shapes     (1, 1); (1, 31), (1, 32), (2, 33), (3, 50), (2, 64), (3, 96): ragged and full last tiles, a clip boundary on,
             before and after a tile edge; (33, 1024): 1056 tiles, the first second trip of the grid-stride loops;
             (3, 22405): 2103 tiles, some waves three tiles and the rest two (forward: two trips of the prefetch loop before
             the peeled tile; backward: register sets ra, rb, ra)

The mask words the forward kernel writes, and those srwn_nc_mask_bits makes of the same tensors, equal
nc_design.mask_words (written from the documented layout) in every lane whose time row is inside the clip; the backward
kernel reads host-made words, with the lanes beyond T all ones in one run and all zeros in another: same output bits.
Outputs are pre-filled with NaN (none may remain) and followed directly, after row B T - 1, by 32 canary rows that must
not change.  The random designs hold every entry within c (u_out |ref| + K 2^-24 S), c = 4 C_CPU, against a reference fed
the kernel's own stored first stage, so that what was stored is what the chain consumed.

Worst error / bound scale (SRWN_PRINT_ERR=1 pytest -s prints them):
                         nc_fwd_a   nc_fwd_r   nc_bwd_dh   nc_bwd_dpre
  float32 NumPy (CPU)    1.92       1.97       1.95        1.98
  C_CPU (rounded up)     2          2          2           2
  bound = 4 x C_CPU      8          8          8           8
  MI355X, measured       1.92       1.97       1.95        1.98
(set by the bf16 outputs: a correctly rounded result reaches 2 against u_out = 2^-9 at a binade's lower end.)

Mutations on scratch builds of csrc/srwn_nc.hip (in-bounds arithmetic only; never committed): cases of this file (24) that
fail / of the 11 tests of tests/test_gpu_autoencoder.py that run both kernels in bf16 (forward_backward x 5, the fused /
two-launch comparison x 5, the mask words), how many still pass:
  forward tap validity < made <=                                        11 fail / 6 of 11 pass
  backward t - 1 at t = 0 reads the previous clip's last row             8 fail / 8 of 11
  the forward's a_bits call an exactly zero pre-activation positive      9 fail / 11 of 11
  mask_bit with mt & 1 and mt >> 1 swapped                              11 fail / 1 of 11
  frame_add row t0 / pool for tc / pool                                 10 fail / 10 of 11
  forward prefetch loads `tile` for `tile + stride`                      3 fail / 11 of 11 (no test reached the loop)
  rb used where ra is due on the third trip                              1 fail / 11 of 11 (no test reached a third trip)
  the chained operand truncated to bf16 where it should round            2 fail / 7 of 11
(of the 23 bf16 twin tests of test_gpu_encoder_stream.py / test_gpu_encoder_pool.py, which run the forward kernel: 17, 23
and 23 pass under the first, sixth and last mutation.)
"""
import os

import numpy as np
import pytest
import torch

from tests import gemm_design as G
from tests import nc_design as N
from tests._pkg import sub

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
C = N.C
CANARY_ROWS = 32
WORD_FILL = 0x5A5A5A5A5A5A5A5A


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _dev(a, dt=F32):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


def _host(t):
    return t.double().cpu().numpy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """[rows, C] bf16 pre-filled with NaN, directly followed by CANARY_ROWS rows of a fixed pattern."""

    def __init__(self, rows):
        self.rows = rows
        self.buf = torch.full((rows + CANARY_ROWS, C), float("nan"), dtype=BF16, device=DEV)
        self.buf[rows:] = (torch.arange(CANARY_ROWS * C, device=DEV) % 251 - 125).to(BF16).view(CANARY_ROWS, C)
        self.canary = self.buf[rows:].clone()
        self.ptr = self.buf.data_ptr()

    def check(self, what):
        got = self.buf[:self.rows]
        assert not bool(torch.isnan(got).any()), what + ": an entry was left unwritten"
        assert torch.equal(self.buf[self.rows:].view(torch.int16), self.canary.view(torch.int16)), what + ": rows behind B T written"
        return got


class Words:
    """Mask words pre-filled with a pattern, followed by 64 canary words."""

    def __init__(self, B, T):
        self.n = N.nwords(B, T)
        self.buf = torch.full((self.n + 64,), WORD_FILL, dtype=torch.int64, device=DEV)
        self.ptr = self.buf.data_ptr()

    def check(self, what, want, inside):
        got = self.buf.cpu().numpy().view(np.uint64)
        assert (got[self.n:] == np.uint64(WORD_FILL)).all(), what + ": words behind the last tile written"
        bad = np.nonzero((got[:self.n] != want) & inside)[0]
        assert len(bad) == 0, "%s: %d of %d mask words differ, first at tile %d lane %d: got %016x, want %016x" % (
            what, len(bad), int(inside.sum()), bad[0] // 64, bad[0] % 64, int(got[bad[0]]), int(want[bad[0]]))


def _exact(what, got, want):
    got = _host(got)
    ok = G.same_bits(got, want)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d entries differ from the reference, first at row %d channel %d: got %r, want %r"
                             % (what, len(bad), ok.size, i[0], i[1], got[i], want[i]))


def _images(w, wr):
    """The four packed images of a layer as the engine builds them, from the flat fp32 parameters [W | Wr]:
    (buffer, conv, 1x1 permuted, conv transposed, 1x1 transposed permuted) as device pointers."""
    K = sub("kernels"); P = sub("packing")
    pk = K.Packer(DEV)
    offs = [P.pack_conv(pk, 0, 2, C), P.pack_linear(pk, 2 * C * C, C, C, C, perm=True), P.pack_conv_T(pk, 0, 2, C),
            P.pack_linear_T(pk, 2 * C * C, C, C, C, perm=True)]
    pk.finalize()
    buf = torch.zeros(pk.total, dtype=BF16, device=DEV)
    pk.gather(_dev(np.concatenate([w.reshape(-1), wr.reshape(-1)])), buf)
    return (buf,) + tuple(buf.data_ptr() + o * buf.element_size() for o in offs)


def _fwd(r, img, bc, br, B, T, res, bits):
    """One launch of srwn_nc_layer_fwd: (a_out, r_out or None, a_bits or None, r_bits or None), unchecked."""
    call = sub("_lib").call
    a_out, r_out = Out(B * T), Out(B * T) if res else None
    ab, rb = (Words(B, T), Words(B, T) if res else None) if bits else (None, None)
    call("srwn_nc_layer_fwd", r.data_ptr(), img[1], img[2] if res else None, bc.data_ptr(), br.data_ptr() if res else None,
         a_out.ptr, r_out.ptr if res else None, ab.ptr if ab else None, rb.ptr if rb else None, B, T, C, 2, 1, _stream())
    torch.cuda.synchronize()
    return a_out, r_out, ab, rb


def _bwd(dp, img, rbits, abits, B, T, down, fadd=None, ld=0, frames=0, pool=1, scale=0.0, off=0):
    call = sub("_lib").call
    dh, dpre = Out(B * T), Out(B * T) if down else None
    call("srwn_nc_layer_bwd", dp.data_ptr(), img[3], rbits.data_ptr(), dh.ptr, img[4] if down else None,
         None if fadd is None else fadd.data_ptr() + 4 * off, ld, frames, pool, scale, abits.data_ptr() if down else None,
         dpre.ptr if down else None, B, T, C, 2, 1, _stream())
    torch.cuda.synchronize()
    return dh, dpre


def _words_dev(m, B, T, beyond):
    return torch.from_numpy(N.mask_words(m, B, T, beyond).view(np.int64)).to(DEV)


# ---- forward, exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", N.SHAPES)
def test_nc_layer_fwd_exact(B, T):
    d = N.fwd_exact(B, T)
    pre_a, _, a, pre_r, _ = N.fwd_ref(d, B, T)
    want_a, want_r = G.round_out(a, "bf16"), G.round_out(np.maximum(pre_r, 0.0), "bf16")
    inside = N.lanes_inside(B, T)
    words_a, words_r = N.mask_words(pre_a, B, T), N.mask_words(pre_r, B, T)
    img = _images(d["w"], d["wr"])
    r = _dev(d["r"], BF16); bc = _dev(d["bc"]); br = _dev(d["br"])
    large = (B, T) in N.LARGE
    for res, bits in ((True, True), (False, False)) if large else ((True, True), (True, False), (False, True), (False, False)):
        what = "nc_layer_fwd (%d, %d) res %d bits %d" % (B, T, res, bits)
        a_out, r_out, ab, rb = _fwd(r, img, bc, br, B, T, res, bits)
        _exact(what + " a_out", a_out.check(what + " a_out"), want_a)
        if res:
            _exact(what + " r_out", r_out.check(what + " r_out"), want_r)
        if bits:
            ab.check(what + " a_bits", words_a, inside)
            if res:
                rb.check(what + " r_bits", words_r, inside)
    # srwn_nc_mask_bits on the tensors the last (res, bits) = (True, True) launch would have stored: the same words
    call = sub("_lib").call
    for name, x, want in (("a", want_a, words_a), ("r", want_r, words_r)):
        xd = _dev(x, BF16)
        wd = Words(B, T)
        call("srwn_nc_mask_bits", xd.data_ptr(), wd.ptr, B, T, C, 1, _stream())
        torch.cuda.synchronize()
        wd.check("nc_mask_bits (%d, %d) %s" % (B, T, name), want, inside)


def test_nc_mask_bits_signs_and_tiny_values():
    """Zeros of both signs and negative values clear the bit; the smallest positive normal number sets it."""
    call = sub("_lib").call
    B, T = 2, 33
    rng = np.random.default_rng(5)
    x = rng.choice([-1.0, -0.0, 0.0, 2.0 ** -126, -2.0 ** -126, 0.5], (B * T, C))
    xd = _dev(x, BF16)
    assert bool(torch.signbit(xd[xd == 0]).any()) and not bool(torch.signbit(xd[xd == 0]).all())
    wd = Words(B, T)
    call("srwn_nc_mask_bits", xd.data_ptr(), wd.ptr, B, T, C, 1, _stream())
    torch.cuda.synchronize()
    wd.check("nc_mask_bits signs", N.mask_words(x, B, T), N.lanes_inside(B, T))


# ---- backward, exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", N.SHAPES)
def test_nc_layer_bwd_exact(B, T):
    d = N.bwd_exact(B, T)
    dh_ref, _ = N.bwd_dh_ref(d, B, T)
    want_dh = G.round_out(dh_ref, "bf16")
    img = _images(d["w"], d["wr"])
    dp = _dev(d["dp"], BF16)
    ragged = T % 32 != 0
    words = {b: (_words_dev(d["mr"], B, T, b), _words_dev(d["ma"], B, T, b)) for b in ((1, 0) if ragged else (0,))}
    cases = [("dh only", None)] + [("no frame_add", (None, 0, 0, 0))] + [("frame_add", c) for c in N.fadd_cases(B, T)]
    for name, case in cases:
        first = None
        want_dp = None
        if case is not None:
            pool, frames, ld, off = case
            fa, fd = None, None
            if pool is not None:
                tab = G.exact((B * frames, ld), 64, 1.0, 7 + pool, N.GB2 / N.FADD_SCALE)      # what lies beside the columns read
                tab.reshape(B, frames, ld)[:, :, off:off + C] = d["fadd"][:, :frames]
                fa, fd = N.FADD_SCALE * N.frame_rows(d["fadd"][:, :frames], B, T, pool), _dev(tab)
            want_dp = G.round_out(N.bwd_dpre_ref(dh_ref, d, fa)[0], "bf16")
        for beyond, (rbits, abits) in words.items():
            what = "nc_layer_bwd (%d, %d) %s %s, lanes beyond T %d" % (B, T, name, case, beyond)
            if case is None:
                dh, dpre = _bwd(dp, img, rbits, abits, B, T, False)
            elif case[0] is None:
                dh, dpre = _bwd(dp, img, rbits, abits, B, T, True)
            else:
                dh, dpre = _bwd(dp, img, rbits, abits, B, T, True, fd, ld, frames, pool, N.FADD_SCALE, off)
            got = [dh.check(what + " dh_out")] + ([dpre.check(what + " dpre_out")] if dpre else [])
            _exact(what + " dh_out", got[0], want_dh)
            if dpre:
                _exact(what + " dpre_out", got[1], want_dp)
            if first is None:
                first = got
            else:        # what the words hold beyond T decides nothing
                assert all(torch.equal(g.view(torch.int16), f.view(torch.int16)) for g, f in zip(got, first)), what


# ---- random designs: every entry within the bound -----------------------------------------------------------------------
def _ratio_ok(what, key, r):
    assert np.isfinite(r).all(), what
    _say("%-44s %s error / bound scale %.3f (<= %g)" % (what, key, r.max(), N.C_GPU[key]))
    bad = np.argwhere(r > N.C_GPU[key])
    assert len(bad) == 0, "%s: error / bound scale %.3g > %g at %s (%d entries)" % (what, r.max(), N.C_GPU[key], bad[0].tolist(), len(bad))


@pytest.mark.parametrize("B,T", N.RANDOM_SHAPES)
def test_nc_layer_fwd_random_entries(B, T):
    d = N.fwd_random(B, T)
    img = _images(d["w"], d["wr"])
    a_out, r_out, ab, rb = _fwd(_dev(d["r"], BF16), img, _dev(d["bc"]), _dev(d["br"]), B, T, True, True)
    what = "nc_layer_fwd random (%d, %d)" % (B, T)
    a_got, r_got = _host(a_out.check(what + " a_out")), _host(r_out.check(what + " r_out"))
    pre_a, S1, _, _, _ = N.fwd_ref(d, B, T)
    pre_r, S2 = G.contract(a_got, d["wr"], d["br"])          # fed the a the kernel stored: it is the a the chain consumed
    inside = N.lanes_inside(B, T)
    for key, got, pre, S, K, wd in (("nc_fwd_a", a_got, pre_a, S1, 2 * C, ab), ("nc_fwd_r", r_got, pre_r, S2, C, rb)):
        r, undecided, wrong = N.relu_entries(got, pre, S, K, key)
        assert undecided.mean() <= N.UNDECIDED_CAP
        assert not wrong.any(), "%s %s: %d entries on the wrong side of the relu, first at %s" % (
            what, key, wrong.sum(), np.argwhere(wrong)[0].tolist())
        _ratio_ok(what, key, r)
        wd.check(what + " " + key + " words", N.mask_words(got, B, T), inside)     # the words say what was stored


@pytest.mark.parametrize("B,T", N.RANDOM_SHAPES)
def test_nc_layer_bwd_random_entries(B, T):
    d = N.bwd_random(B, T)
    img = _images(d["w"], d["wr"])
    rbits, abits = _words_dev(d["mr"], B, T, 1), _words_dev(d["ma"], B, T, 1)
    fd = _dev(d["fadd"].reshape(B * d["frames"], C))
    dh, dpre = _bwd(_dev(d["dp"], BF16), img, rbits, abits, B, T, True, fd, C, d["frames"], d["pool"], d["scale"])
    what = "nc_layer_bwd random (%d, %d)" % (B, T)
    dh_got, dp_got = _host(dh.check(what + " dh_out")), _host(dpre.check(what + " dpre_out"))
    ref, S1 = N.bwd_dh_ref(d, B, T)
    assert ((dh_got != 0) <= (d["mr"] > 0)).all() and ((dp_got != 0) <= (d["ma"] > 0)).all(), what + ": a masked entry is not 0"
    _ratio_ok(what, "nc_bwd_dh", G.ratio(dh_got, ref, S1, 2 * C, "bf16"))
    fa = np.float64(np.float32(d["scale"])) * N.frame_rows(d["fadd"], B, T, d["pool"])
    ref, S2 = N.bwd_dpre_ref(dh_got, d, fa)                  # fed the dh the kernel stored
    _ratio_ok(what, "nc_bwd_dpre", G.ratio(dp_got, ref, S2, C + 1, "bf16"))


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_nc_layer_kernels_refuse_what_they_cannot_run():
    call = sub("_lib").call
    B, T = 1, 64
    z = torch.zeros(T * C, device=DEV, dtype=BF16)
    w = torch.zeros(3 * C * C, device=DEV, dtype=BF16)
    b = torch.zeros(2 * C, device=DEV)
    bits = torch.zeros(N.nwords(B, T), device=DEV, dtype=torch.int64)
    zp, wp, bp, mp = z.data_ptr(), w.data_ptr(), b.data_ptr(), bits.data_ptr()
    out = Out(B * T)
    fwd = lambda *tail: call("srwn_nc_layer_fwd", zp, wp, wp, bp, bp, out.ptr, None, None, None, *tail, None)
    with pytest.raises(RuntimeError, match="128 channels"):
        fwd(B, T, 64, 2, 1)
    with pytest.raises(RuntimeError, match="K=2"):
        fwd(B, T, C, 3, 1)
    with pytest.raises(RuntimeError, match="bf16"):
        fwd(B, T, C, 2, 0)
    with pytest.raises(RuntimeError, match="B=-1"):
        fwd(-1, T, C, 2, 1)
    with pytest.raises(RuntimeError, match="wres"):
        call("srwn_nc_layer_fwd", zp, wp, None, bp, bp, out.ptr, out.ptr, None, None, B, T, C, 2, 1, None)
    with pytest.raises(RuntimeError, match="null"):
        call("srwn_nc_layer_fwd", zp, wp, wp, None, bp, out.ptr, None, None, None, B, T, C, 2, 1, None)
    bwd = lambda fadd, ld, frames, pool, abits=mp, dpre=out.ptr, C_=C: call(
        "srwn_nc_layer_bwd", zp, wp, mp, out.ptr, wp, fadd, ld, frames, pool, 1.0, abits, dpre, B, T, C_, 2, 1, None)
    with pytest.raises(RuntimeError, match="frames 1 x pool 32 < T 64"):
        bwd(bp, C, 1, 32)                                     # frames * pool < T
    with pytest.raises(RuntimeError):
        bwd(bp, C - 4, 2, 32)                                 # frame_add_ld < 128
    with pytest.raises(RuntimeError):
        bwd(bp, C, 64, 0)                                     # pool_stride < 1
    with pytest.raises(RuntimeError):
        bwd(bp, C, 64, -1)
    with pytest.raises(RuntimeError, match="a_bits"):
        bwd(None, 0, 0, 1, abits=None)
    with pytest.raises(RuntimeError, match="128 channels"):
        bwd(None, 0, 0, 1, C_=64)
    with pytest.raises(RuntimeError, match="128 channels"):
        call("srwn_nc_mask_bits", zp, mp, B, T, 64, 1, None)
    with pytest.raises(RuntimeError, match="null"):
        call("srwn_nc_mask_bits", zp, None, B, T, C, 1, None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf[:B * T]).all())           # nothing ran
    assert call("srwn_nc_layer_bwd", zp, wp, mp, out.ptr, None, None, 0, 0, 1, 1.0, None, None, 0, T, C, 2, 1, None) == 0
    assert int(sub("_lib").load().srwn_nc_mask_words(3, 22405)) == N.nwords(3, 22405) == 3 * 701 * 64
