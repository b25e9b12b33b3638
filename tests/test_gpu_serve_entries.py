"""GPU tests that hold the kernels around the streamed stack -- csrc/srwn_recog.hip (stream entry, pooled head, hop sum,
window mean, roll), csrc/srwn_embed.hip (window embed match, gallery match) and the softmax half of csrc/srwn_score.hip
(pool entry with its codes, score head, nll rows), each with its slot form -- to exact references ENTRY BY ENTRY, in fp32
and in bf16, where tests/test_gpu_recognizer.py, test_gpu_scorer.py and test_gpu_embedder.py hold them to max-norm bounds
at one geometry and the pool files compare the slot forms with the clock forms, kernel against kernel.

The designs, their float64 references and the bound constants are tests/serve_design.py's (D); tests/test_serve_design.py
proves the designs' conditions on the CPU.  Every output is allocated with one spare row behind what the kernel is told of
and poisoned with NaN (integer outputs: a sentinel): the spare row and everything the kernel's header calls unwritten must
keep the poison, every valid entry must be finite.

  stream entry   b + x0 w0 + x1 w1 on dyadic audio and weights: bit for bit.  R 32 / 64; (B, n) = (1, 1), (2, 31), (3, 33)
                 and n = max_chunk; out_hist 0 and 5; carry 0 and +-1.  Slot forms: ring_len = max_chunk + 1 (+ 2 for the
                 scorer), a slot at t = 0 whose columns before sample 0 hold the design's largest value, a chunk that wraps
                 the ring at t = 2^33 + a non-multiple of ring_len, an idle slot, ran = 0 and 0 < ran < n; the scorer's codes
                 against oracle.wavenet_np.mu_law_encode for C = 256 and 100
  hop sum        dyadic r1 against the float64 sum and Gaussian r1 against the float32 restatement of the header's order
                 (xor butterfly 1, 2, 4, 8, 16 over a tile's 32 rows, masked rows +0, tiles in time order), both bit for bit;
                 S in {2, 6, 128, 256}, hop in {1, 31, 32, 33, 40, 96}, k in {1, 3}, B in {1, 3}, a ring that wraps, one clock
                 at 2^33 hop, 2^10 x the design behind the chunk
  pooled head    the chained design: ring rows bit for bit in bf16, per entry in fp32; the four (R, S), L in {1, 3}, the six
                 hops, NaN in z behind the chunk; the twin (srwn_pw_linear PRO_GATE + RELU, srwn_pw_linear RELU, srwn_hop_sum)
                 gives the same bits; slot form with an idle slot and one with ran = one hop of two
  window mean    rows with j < nW - 1 (slot form: beyond ran) exact zeros; power-of-two windows bit for bit, mean and logits;
                 windows 96 and 320: the mean bit for bit against the exact sum divided once in float32, the logits per entry
  roll           a distinct value per (buffer, stream, row, column); hist on both sides of the 64- and 256-row steps; n <, =,
                 > hist; nroll 0, 1, 3; carry and clock (from 0 and from 2^33); slot form: each slot by its own ran
  score head     logits_out bit for bit (bf16) / per entry (fp32); best = the lowest index of the maximum with built ties at
                 distance 1 and 8; nll per entry against the float64 log-sum-exp; srwn_nll_rows on the head's logits gives the
                 head's bits, also with ld > C and 1e30 behind column C; slot forms
  match          distances bit for bit against sqrt_f32(f32(1e-8) + ss) on dyadic rows, D in {1, 2, 63, 64, 65, 256}, *n_gallery
                 from -3 to max_gallery + 7, ties at distance 1, 4 and across the four waves; srwn_window_embed_match has the
                 bits of srwn_window_mean's logits and of srwn_gallery_match on them
  refusals       the header's error codes, poisoned outputs untouched

What is not exact is held per entry to |got - ref| <= c (2^-24 |ref| + scale), c = 4 x the float32 NumPy restatement's worst
ratio (D.C_CPU, measured by tests/test_serve_design.py; never a GPU figure).  SRWN_PRINT_ERR=1 pytest -s prints what the device
reaches.

Worst error / bound scale:
                         pooled_ring_fp32   score_logits_fp32   score_nll (bf16 | fp32)   window_logits
  float32 NumPy (CPU)    0.0049             0.0022              0.434 | 0.447             0.363
  C_CPU (rounded up)     0.0625             0.0625              0.4375 | 0.5              0.375
  bound = 4 x C_CPU      0.25               0.25                1.75 | 2                  1.5
  MI355X, measured       0.0054             0.0025              0.539 | 0.734             0.403
(K 2^-24 S is the worst case of K roundings of one sign, so the two chained products stay two orders below it; the nll and
the window logits at S = 1 are a handful of roundings each.)  The two one-ulp allowances the designs provide for -- the
float32 division of the window mean and sqrtf of the gallery distance -- were not needed: the device is bit for bit.

Run time on the MI355X: 106 tests in 4.6 s (the slowest 0.26 s).

Mutations of the three kernel files on scratch builds (in-bounds arithmetic only; never committed), each run once: tests of
this file that fail / tests of the existing files that run the mutated code and still pass (R = tests/test_gpu_recognizer.py
+ test_gpu_recognizer_pool.py, 77 tests; S = test_gpu_scorer.py + test_gpu_scorer_pool.py, 86; E = test_gpu_embedder.py +
test_gpu_embedder_pool.py, 48).  The file had 100 tests at the time; the six mixture-head tests added since run none of the
mutated lines.
  1 pooled head: the hop sum's mask one row too large in the last tile (col <= valid)   16 of 100 fail / R 64 of 77 pass
  2 pooled head only: ring row (j + 1) % ring_rows                                      16 of 100 fail / R 31 of 77
  3 pooled head: one 16-wide k-step of W1 skipped for wave 3                            16 of 100 fail / R 42 of 77
  4 >= for > in a relu: not a mutation here -- every relu of the three files is fmaxf(acc, 0), and relu(0) is a zero
    either way (G.same_bits takes a zero of either sign); the design still places an exact 0 in every relu column
  5 row_nll: ob < bi made ob > bi (a tie across lanes goes to the higher index)         36 of 100 fail / S 86 of 86
  6 slot entry: s >= 1 made s >= 0 (the sample before time 0 is read)                    4 of 100 fail / pool file 9 of 22
  7 window mean: the loop starts at j - nW + 2                                           6 of 100 fail / R 49 of 77
  8 match_body: the strict < made <= (a wave keeps its last minimum)                     6 of 100 fail / E 48 of 48
  9 roll: the first barrier removed for n < hist                                         0 of 100 fail / R 77 of 77
(1 is the in-bounds form of "valid one too large": the mask of the sum alone, so that no row behind the buffer is read.
9 is a race, not arithmetic: it cannot hang -- the condition is uniform over the workgroup -- but the four waves issue
their loads within a few cycles of each other and long before any store retires, so the overlap never shows; no test of the
suite can force that interleaving, and the roll test holds what a wrong order WOULD produce: every element of every buffer.)
"""
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests import gemm_design as G
from tests import serve_design as D
from tests._pkg import sub

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NAME = {F32: "fp32", BF16: "bf16"}
NAN = float("nan")
SENT = -7                                            # the poison of integer outputs
E_DTYPE, E_SHAPE, E_NULL, E_UNSUPPORTED = -1, -2, -3, -4          # include/srwn.h
T33 = 1 << 33


def _say(*a):
    if os.environ.get("SRWN_PRINT_ERR"):
        print(*a)


def _dev(a, dt=F32):
    return torch.tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()


def _host(t):
    return t.double().cpu().numpy()


def _nan(shape, dt=F32):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def _spare(rows, C, dt=F32):
    """(buffer of rows + 1 poisoned rows, its first `rows` rows): the kernel is told of `rows` only."""
    buf = _nan((rows + 1, C), dt)
    return buf, buf[:rows]


def _spare_int(rows, C):
    buf = torch.full((rows + 1, C), SENT, dtype=torch.int32, device=DEV)
    return buf, buf[:rows]


def _intact(what, buf, rows, written=None):
    """The spare row keeps its poison, and so does every row the kernel must not write (`written`: a boolean per row; None:
    all are written); every entry of a written row is finite.  Returns the rows on the host."""
    torch.cuda.synchronize()
    if buf.dtype == torch.int32:
        got = buf.cpu().numpy().astype(np.float64)
        poison = got == SENT
    else:
        got = _host(buf)
        poison = np.isnan(got)
    assert poison[rows].all(), what + ": the row behind the last was written"
    got, poison = got[:rows], poison[:rows]
    written = np.ones(rows, bool) if written is None else np.asarray(written, bool).reshape(-1)
    bad = np.argwhere(~poison[~written])
    assert len(bad) == 0, "%s: %d entries written that the header calls unwritten, first at %s" % (what, len(bad), bad[0].tolist())
    bad = np.argwhere(poison[written] | ~np.isfinite(got[written]))
    assert len(bad) == 0, "%s: %d entries not finite (unwritten or NaN), first at %s" % (what, len(bad), bad[0].tolist())
    return got


def _exact(what, got, want):
    ok = G.same_bits(got, want)
    if not ok.all():
        bad = np.argwhere(ok.reshape(got.shape) == 0)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d entries differ from the exact reference, first at %s: got %r, want %r"
                             % (what, len(bad), ok.size, list(i), got[i], want[i]))


def _bounded(what, key, mode, got, ref, scale):
    r = D.ratio(got, ref, scale)
    assert np.isfinite(r).all(), what + ": a non-zero entry where the reference and its bound are exactly 0"
    c = D.C_GPU[key][mode]
    _say("%-64s %s %s error / bound scale %.4f (<= %g)" % (what, key, mode, r.max(), c))
    bad = np.argwhere(r > c)
    assert len(bad) == 0, "%s: error / bound scale %.3g > %g at %s (%d entries)" % (what, r.max(), c, bad[0].tolist(), len(bad))


def _table(slots):
    """[(t, ran)] -> the device table of SrwnSynthSlot (t < 0: idle)."""
    return torch.tensor([[t, t + r] if t >= 0 else [-1, -1] for (t, r) in slots], dtype=torch.int64, device=DEV)


def _abi(dt):
    return sub("kernels").abi_dtype(dt)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    return sub("_lib").call(name, *args)


# ---- stream entry ---------------------------------------------------------------------------------------------------------
ENTRY_CLIPS = [(1, 1, 1), (2, 31, 40), (3, 33, 40), (2, 40, 40)]      # (B, n, max_chunk)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", [32, 64])
def test_recog_stream_in_exact(R, dt):
    """out[b, hist + t] = bias + x[t - 1] w0 + x[t] w1 bit for bit (x[-1] the carry: 0 for stream 0, +-1 for the others);
    the history rows and the rows from hist + n on keep their poison, as does the x behind the chunk (NaN)."""
    mode, e = NAME[dt], D.entry(R)
    w, b = _dev(e["w"]), _dev(e["b"])
    for (B, n, mc) in ENTRY_CLIPS:
        for hist in (0, 5):
            a = D.audio((B, n), n + hist)
            carry = np.array([0.0, 1.0, -1.0])[:B]
            x = _nan((B, mc)); x[:, :n] = _dev(a)
            clip = hist + mc
            buf, out = _spare(B * clip, R, dt)
            cd = _dev(carry)                                          # (every device operand is held until the check is done)
            _call("srwn_recog_stream_in", x.data_ptr(), mc, cd.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(),
                  clip, hist, B, n, mc, R, _abi(dt), _st())
            what = "recog_stream_in %s R %d B %d n %d hist %d" % (mode, R, B, n, hist)
            written = np.zeros((B, clip), bool); written[:, hist:hist + n] = True
            got = _intact(what, buf, B * clip, written).reshape(B, clip, R)
            x0 = np.concatenate([carry[:, None], a[:, :-1]], 1)
            _exact(what, got[:, hist:hist + n].reshape(B * n, R), D.entry_ref(e, x0.reshape(-1), a.reshape(-1), mode))


def _slot_audio(cap_slots, ring_len, back, seed):
    """The pool's audio ring [capacity, ring_len], the design's largest value everywhere but in the columns of the samples
    [t - back, t + ran) of every live slot (those at or after time 0); returns (ring, sample(u, s) with 0 before time 0)."""
    ring = np.full((len(cap_slots), ring_len), D.A_TOP)
    samples = {}
    for u, (t, ran) in enumerate(cap_slots):
        if t < 0:
            continue
        a = D.audio((ran + back,), seed + u)
        for i, s in enumerate(range(t - back, t + ran)):
            if s >= 0:
                ring[u, s % ring_len] = a[i]
                samples[(u, s)] = a[i]
    return ring, lambda u, s: samples.get((u, s), 0.0) if s >= 0 else 0.0


def _entry_slots(n, mc, ring_len):
    """A slot at t = 0, one at 2^33 + a non-multiple of ring_len whose chunk wraps the ring, an idle one, ran = 0 and
    0 < ran < n."""
    off = (ring_len - 3 - T33 % ring_len) % ring_len
    t1 = T33 + off
    assert t1 % ring_len == ring_len - 3 > 0 and (n <= 3 or t1 % ring_len + n > ring_len)
    return [(0, n), (t1, n), (-1, 0), (7, 0), (5 * ring_len + 2, n // 2)]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", [32, 64])
def test_recog_stream_in_slots_exact(R, dt):
    """The slot form on the smallest audio ring (max_chunk + 1): every live row bit for bit from the ring's samples, the
    column before sample 0 (the design's largest value) read as 0, rows from ran on and idle slots' rows untouched."""
    mode, e = NAME[dt], D.entry(R)
    w, b = _dev(e["w"]), _dev(e["b"])
    for (n, mc) in ((31, 33), (33, 33), (2, 3)):
        for hist in (0, 5):
            ring_len = mc + 1
            slots = _entry_slots(n, mc, ring_len)
            cap, clip = len(slots), hist + mc
            ring, smp = _slot_audio(slots, ring_len, 1, n + hist)
            buf, out = _spare(cap * clip, R, dt)
            rd, tb = _dev(ring), _table(slots)
            _call("srwn_recog_stream_in_slots", rd.data_ptr(), ring_len, w.data_ptr(), b.data_ptr(), out.data_ptr(), clip,
                  hist, cap, n, mc, R, _abi(dt), tb.data_ptr(), _st())
            what = "recog_stream_in_slots %s R %d n %d hist %d" % (mode, R, n, hist)
            written = np.zeros((cap, clip), bool)
            for u, (t, ran) in enumerate(slots):
                written[u, hist:hist + max(ran, 0)] = t >= 0
            got = _intact(what, buf, cap * clip, written).reshape(cap, clip, R)
            for u, (t, ran) in enumerate(slots):
                if t >= 0 and ran:
                    x0 = np.array([smp(u, s - 1) for s in range(t, t + ran)])
                    x1 = np.array([smp(u, s) for s in range(t, t + ran)])
                    _exact("%s slot %d" % (what, u), got[u, hist:hist + ran], D.entry_ref(e, x0, x1, mode))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("C", [256, 100])
@pytest.mark.parametrize("R", [32, 64])
def test_score_stream_in_slots_exact(R, C, dt):
    """The scorer's pool entry: rows from a[s - 2] and a[s - 1] (0 before time 0, at s = 0 and s = 1 the columns hold the
    design's largest value) bit for bit, codes = mu_law_encode(a[s]); code rows from ran on keep the sentinel."""
    mode, e = NAME[dt], D.entry(R, 1)
    w, b = _dev(e["w"]), _dev(e["b"])
    for (n, mc, hist) in ((31, 33, 0), (33, 33, 5), (2, 3, 0)):
        ring_len = mc + 2
        slots = _entry_slots(n, mc, ring_len)
        cap, clip = len(slots), hist + mc
        ring, smp = _slot_audio(slots, ring_len, 2, n + hist + C)
        buf, out = _spare(cap * clip, R, dt)
        cbuf, codes = _spare_int(cap, mc)
        rd, tb = _dev(ring), _table(slots)
        _call("srwn_score_stream_in_slots", rd.data_ptr(), ring_len, w.data_ptr(), b.data_ptr(), out.data_ptr(), clip, hist,
              codes.data_ptr(), mc, cap, n, mc, R, C, _abi(dt), tb.data_ptr(), _st())
        what = "score_stream_in_slots %s R %d C %d n %d hist %d" % (mode, R, C, n, hist)
        written = np.zeros((cap, clip), bool)
        for u, (t, ran) in enumerate(slots):
            written[u, hist:hist + max(ran, 0)] = t >= 0
        got = _intact(what, buf, cap * clip, written).reshape(cap, clip, R)
        torch.cuda.synchronize()
        cg = cbuf.cpu().numpy()
        assert (cg[cap] == SENT).all(), what + ": the code row behind the last was written"
        for u, (t, ran) in enumerate(slots):
            ran = ran if t >= 0 else 0
            assert (cg[u, ran:] == SENT).all(), "%s slot %d: codes written from ran on" % (what, u)
            if ran:
                x0 = np.array([smp(u, s - 2) for s in range(t, t + ran)])
                x1 = np.array([smp(u, s - 1) for s in range(t, t + ran)])
                _exact("%s slot %d" % (what, u), got[u, hist:hist + ran], D.entry_ref(e, x0, x1, mode))
                want = O.mu_law_encode(np.array([smp(u, s) for s in range(t, t + ran)]), C)
                assert np.array_equal(cg[u, :ran], want), "%s slot %d: codes" % (what, u)


# ---- hop sum -----------------------------------------------------------------------------------------------------------------
def _owned(B, ring_rows, js):
    """The ring rows the chunk's hops own: js [B][...] hop indices per stream."""
    own = np.zeros((B, ring_rows), bool)
    for b, jl in enumerate(js):
        for j in jl:
            own[b, j % ring_rows] = True
    return own


def _hop_want(x, k, hop, kind, dt):
    """x [B, mc, S] -> [B, k, S]: the float64 sum (dyadic) or the float32 restatement of the documented order."""
    B, mc, S = x.shape
    rows = x[:, :k * hop].reshape(B, k, hop, S)
    if kind == "dyadic":
        return G.round_out(rows.sum(2), "fp32")
    return D.hop_sum32(rows).astype(np.float64)


@pytest.mark.parametrize("kind", ["dyadic", "gauss"])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_hop_sum_exact(dt, kind):
    """Every ring row of the chunk's hops bit for bit; the rows no hop owns keep their poison; the r1 rows behind k * hop
    (2^10 x the design) do not count.  ring_rows = k + 1 and j0 = k: the chunk's hops wrap the ring."""
    mode = NAME[dt]
    for S in (2, 6, 128, 256):
        for hop in D.HOPS:
            for k in (1, 3):
                for B in (1, 3):
                    j0s = [k] + ([T33] if (S, B) == (6, 3) else [])
                    x = D.hopsum(S, hop, k, B, kind, mode)
                    mc, rr = k * hop + 2, k + 1
                    xd = _dev(x, dt)
                    want = _hop_want(x, k, hop, kind, dt)
                    for j0 in j0s:
                        buf, ring = _spare(B * rr, S)
                        clock = torch.tensor([j0 * hop], dtype=torch.int64, device=DEV)
                        _call("srwn_hop_sum", xd.data_ptr(), mc, ring.data_ptr(), rr, clock.data_ptr(), B, k, hop, mc, S, _abi(dt), _st())
                        what = "hop_sum %s %s S %d hop %d k %d B %d j0 %d" % (mode, kind, S, hop, k, B, j0)
                        own = _owned(B, rr, [[j0 + i for i in range(k)]] * B)
                        got = _intact(what, buf, B * rr, own).reshape(B, rr, S)
                        for i in range(k):
                            _exact("%s hop %d" % (what, i), got[:, (j0 + i) % rr], want[:, i])


@pytest.mark.parametrize("kind", ["dyadic", "gauss"])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_hop_sum_slots_exact(dt, kind):
    """The slot form: slot 0 with all three hops, slot 1 idle, slot 2 at another clock with ran = one hop of three; the ring
    rows of the hops beyond ran keep their poison."""
    mode, k, B = NAME[dt], 3, 3
    for S in (6, 128):
        for hop in D.HOPS:
            x = D.hopsum(S, hop, k, B, kind, mode)
            mc, rr = k * hop + 2, k + 1
            slots = [(k * hop, k * hop), (-1, 0), ((T33 + 2) * hop, hop)]
            buf, ring = _spare(B * rr, S)
            xd, tb = _dev(x, dt), _table(slots)
            _call("srwn_hop_sum_slots", xd.data_ptr(), mc, ring.data_ptr(), rr, tb.data_ptr(), B, k, hop, mc, S,
                  _abi(dt), _st())
            what = "hop_sum_slots %s %s S %d hop %d" % (mode, kind, S, hop)
            js = [[k + i for i in range(k)], [], [T33 + 2]]
            got = _intact(what, buf, B * rr, _owned(B, rr, js)).reshape(B, rr, S)
            want = _hop_want(x, k, hop, kind, dt)
            for b in (0, 2):
                for i, j in enumerate(js[b]):
                    _exact("%s slot %d hop %d" % (what, b, i), got[b, j % rr], want[b, i])


# ---- pooled head ---------------------------------------------------------------------------------------------------------
def _head_images(dt, d, L, R, S):
    """The packed skip image (rows = skip channel, k = l R + n), W1 and, for the scorer, W2: (buffer, pointers)."""
    K = sub("kernels"); P = sub("packing")
    mats = [d["ws"], d["w1"]] + ([d["w2"]] if d["C"] else [])
    flat = torch.cat([_dev(m).flatten() for m in mats])
    pk = K.Packer(DEV)
    o_skip = pk.reserve(S // 32, L * R // 16)
    for l in range(L):
        P.fill_linear(pk, o_skip, l * R * S, R, S, S // 32, L * R // 16, ks_offset=l * R // 16, ks_count=R // 16)
    offs = [o_skip, P.pack_linear(pk, L * R * S, S, S, S)]
    if d["C"]:
        Cp = d["w2"].shape[1]
        offs.append(P.pack_linear(pk, L * R * S + S * S, S, Cp, Cp))
    pk.finalize()
    buf = torch.empty(pk.total, dtype=dt, device=DEV)
    pk.gather(flat, buf)
    return buf, [buf.data_ptr() + o * buf.element_size() for o in offs]


def _pooled_want(d, mode, B, k, hop, mc):
    """(hop sums [B, k, S], their error scale or None)."""
    r1, e1, _, _ = D.head_ref(d, mode)
    want = D.hop_rows(r1, B, k, hop, mc).sum(2)
    return want, None if e1 is None else D.hop_rows(e1, B, k, hop, mc).sum(2)


def _pooled_check(what, mode, got, want, scale):
    if mode == "bf16":
        _exact(what, got, G.round_out(want, "fp32"))
    else:
        _bounded(what, "pooled_ring_fp32", mode, got, want, scale)


def _pooled_case(dt, R, S, L, hop, j0=2):
    K = sub("kernels")
    mode, B, k, rr = NAME[dt], 2, 2, 3
    mc = k * hop + 3
    d = D.head(L, R, S, B * mc)
    ibuf, (pskip, pw1) = _head_images(dt, d, L, R, S)
    z = _dev(d["z"], dt).view(L, B, mc, R)
    z[:, :, k * hop:] = NAN                                           # a read behind the chunk shows
    bs, b1 = _dev(d["bs"]), _dev(d["b1"])
    want, scale = _pooled_want(d, mode, B, k, hop, mc)
    what = "pooled_stream_head %s R %d S %d L %d hop %d j0 %d" % (mode, R, S, L, hop, j0)
    own = _owned(B, rr, [[j0 + i for i in range(k)]] * B)
    clock = torch.tensor([j0 * hop], dtype=torch.int64, device=DEV)
    buf, ring = _spare(B * rr, S)
    _call("srwn_pooled_stream_head", z.data_ptr(), B * mc * R, mc, L, pskip, bs.data_ptr(), pw1, b1.data_ptr(), ring.data_ptr(), rr,
          clock.data_ptr(), B, k, hop, mc, R, S, _abi(dt), _st())
    got = _intact(what, buf, B * rr, own).reshape(B, rr, S)
    for i in range(k):
        _pooled_check("%s hop %d" % (what, i), mode, got[:, (j0 + i) % rr], want[:, i], None if scale is None else scale[:, i])
    # the twin: the two products through srwn_pw_linear, the sum through srwn_hop_sum -- the fused head's bits
    rows = (B - 1) * mc + k * hop
    r0, r1 = _nan((B * mc, S), dt), _nan((B * mc, S), dt)
    K.pw_linear(z.data_ptr(), R, B * mc * R, R, L * R, pskip, bs, r0[:rows], S, S, rows, pro=K.PRO_GATE, epi=K.EPI_RELU)
    K.pw_linear(r0.data_ptr(), S, 0, S, S, pw1, b1, r1[:rows], S, S, rows, epi=K.EPI_RELU)
    tbuf, tring = _spare(B * rr, S)
    _call("srwn_hop_sum", r1.data_ptr(), mc, tring.data_ptr(), rr, clock.data_ptr(), B, k, hop, mc, S, _abi(dt), _st())
    twin = _intact(what + " twin", tbuf, B * rr, own).reshape(B, rr, S)
    _exact(what + " twin against the fused head", twin[own], got[own])
    return d, ibuf, (pskip, pw1), z, bs, b1, want, scale


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R,S", D.WIDTHS)
def test_pooled_stream_head_entries(R, S, dt):
    """The ring rows of a chunk of two hops, B = 2, in a ring of three rows at j0 = 2 (rows 2 and 0: the ring wraps, row 1
    keeps its poison): bit for bit the chained design's hop sums in bf16, per entry in fp32; z behind the chunk is NaN; the
    twin gives the fused head's bits.  One case per width at a clock of (2^33 + 2) hops."""
    for L in (1, 3):
        for hop in D.HOPS:
            _pooled_case(dt, R, S, L, hop)
    _pooled_case(dt, R, S, 3, 33, T33 + 2)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R,S", D.WIDTHS)
def test_pooled_stream_head_slots_entries(R, S, dt):
    """The slot form on the same design: slot 0 at (2^33 + 3) hop with both hops (ring rows 2 and 0), slot 1 at j = 2 with ran = one hop of
    two (its second hop's z rows are NaN and its ring row keeps the poison), slot 2 idle (all of its z is NaN)."""
    mode, L, k, rr, cap = NAME[dt], 3, 2, 3, 3
    for hop in D.HOPS:
        mc = k * hop + 3
        d = D.head(L, R, S, 2 * mc)
        ibuf, (pskip, pw1) = _head_images(dt, d, L, R, S)
        z = _nan((L, cap, mc, R), dt)
        z[:, :2] = _dev(d["z"], dt).view(L, 2, mc, R)
        z[:, 0, k * hop:] = NAN
        z[:, 1, hop:] = NAN
        slots = [((T33 + 3) * hop, k * hop), (2 * hop, hop), (-1, 0)]
        js = [[T33 + 3, T33 + 4], [2], []]
        buf, ring = _spare(cap * rr, S)
        bs, b1, tb = _dev(d["bs"]), _dev(d["b1"]), _table(slots)
        _call("srwn_pooled_stream_head_slots", z.data_ptr(), cap * mc * R, mc, L, pskip, bs.data_ptr(), pw1,
              b1.data_ptr(), ring.data_ptr(), rr, tb.data_ptr(), cap, k, hop, mc, R, S, _abi(dt), _st())
        what = "pooled_stream_head_slots %s R %d S %d hop %d" % (mode, R, S, hop)
        got = _intact(what, buf, cap * rr, _owned(cap, rr, js)).reshape(cap, rr, S)
        want, scale = _pooled_want(d, mode, 2, k, hop, mc)
        for b in (0, 1):
            for i, j in enumerate(js[b]):
                _pooled_check("%s slot %d hop %d" % (what, b, i), mode, got[b, j % rr], want[b, i], None if scale is None else scale[b, i])


# ---- window mean ---------------------------------------------------------------------------------------------------------
def _window_want(ring, js, nW, win):
    """ring [B, rr, S], js [B][k] hop indices (None: a row that is not due) -> (mean [B k, S] as float32 values, exact?)."""
    rows = []
    for b, jl in enumerate(js):
        for j in jl:
            rows.append(np.zeros(ring.shape[2]) if j is None else D.window_sum(ring[b], j, nW))
    tot = np.stack(rows)
    return tot / win if D.pow2(win) else D.mean32(tot, win)


def _window_check(what, win, S, C, h, mbuf, lbuf, rows, want):
    got = _intact(what + " mean", mbuf, rows)
    _exact(what + " mean", got, G.round_out(want, "fp32"))
    lg = _intact(what + " logits", lbuf, rows)
    w2, b2 = h["w2"][:, :C], h["b2"]
    if D.pow2(win):
        _exact(what + " logits", lg, G.round_out(want @ w2 + b2, "fp32"))
    else:
        ref, Sm = G.contract(want, w2, b2)
        _bounded(what + " logits", "window_logits", "fp32", lg, ref, S * D.EPS * Sm)
    return got, lg


def test_window_mean_entries():
    """Rows with j < nW - 1 are exact zeros (their logits: b2); power-of-two windows: mean and logits bit for bit; windows
    96 and 320: the mean bit for bit against the exact sum divided once in float32, the logits per entry with K = S.  The
    smallest ring (nW + k - 1 rows), a clock of 0 and one that wraps the ring; ldw > C with 2^10 x the design behind C."""
    n = 0
    for (hop, nW) in D.WINDOWS:
        win = hop * nW
        for S in D.WM_S:
            for k in (1, 3):
                B, rr = 2, nW + k - 1
                C = D.WM_C[n % 3]; n += 1
                h = D.wm_head(S, C, C + 3)
                ring = D.ringrows(B, rr, S, nW)
                rd, w2, b2 = _dev(ring), _dev(h["w2"]), _dev(h["b2"])
                for j0 in (0, 2 * rr - 1, T33 + 1):
                    clock = torch.tensor([j0 * hop], dtype=torch.int64, device=DEV)
                    mbuf, mean = _spare(B * k, S)
                    lbuf, lg = _spare(B * k, C)
                    _call("srwn_window_mean", rd.data_ptr(), rr, mean.data_ptr(), clock.data_ptr(), B, k, hop, win, S, w2.data_ptr(),
                          b2.data_ptr(), lg.data_ptr(), C, C + 3, _st())
                    what = "window_mean hop %d nW %d S %d k %d C %d j0 %d" % (hop, nW, S, k, C, j0)
                    want = _window_want(ring, [[j0 + i for i in range(k)]] * B, nW, win)
                    got, _ = _window_check(what, win, S, C, h, mbuf, lbuf, B * k, want)
                    if j0 == 0:
                        assert not got.reshape(B, k, S)[:, :min(k, nW - 1)].any(), what + ": rows before the first whole window"
                mbuf, mean = _spare(B * k, S)                          # without logits: the mean alone, nothing else touched
                _call("srwn_window_mean", rd.data_ptr(), rr, mean.data_ptr(), clock.data_ptr(), B, k, hop, win, S, None, None, None, 0, 0,
                      _st())
                _exact(what + " mean alone", _intact(what + " mean alone", mbuf, B * k), got)


def test_window_mean_slots_entries():
    """The slot form: slot 0 with all its hops, slot 1 idle, slot 2 at 2^33 + 1 with ran = one hop: rows beyond ran and the
    idle slot's rows are exact zeros with logits b2."""
    k, cap = 3, 3
    for n, (hop, nW) in enumerate(D.WINDOWS):
        win, rr = hop * nW, nW + k - 1
        for S in (100, 256):
            C = D.WM_C[n % 3]
            h = D.wm_head(S, C, C + 3)
            ring = D.ringrows(cap, rr, S, nW)
            slots = [((2 * rr - 1) * hop, k * hop), (-1, 0), ((T33 + 1) * hop, hop)]
            js = [[2 * rr - 1 + i for i in range(k)], [None] * k, [T33 + 1, None, None]]
            mbuf, mean = _spare(cap * k, S)
            lbuf, lg = _spare(cap * k, C)
            rd, tb, w2, b2 = _dev(ring), _table(slots), _dev(h["w2"]), _dev(h["b2"])
            _call("srwn_window_mean_slots", rd.data_ptr(), rr, mean.data_ptr(), tb.data_ptr(), cap, k, hop, win, S,
                  w2.data_ptr(), b2.data_ptr(), lg.data_ptr(), C, C + 3, _st())
            what = "window_mean_slots hop %d nW %d S %d C %d" % (hop, nW, S, C)
            got, glg = _window_check(what, win, S, C, h, mbuf, lbuf, cap * k, _window_want(ring, js, nW, win))
            idle = np.array([j is None for jl in js for j in jl])
            assert not got[idle].any(), what + ": rows beyond ran"
            _exact(what + " logits of the rows beyond ran", glg[idle], np.broadcast_to(G.round_out(h["b2"], "fp32"), glg[idle].shape))


# ---- roll --------------------------------------------------------------------------------------------------------------------
def _roll_buffers(dt, hists, B, mc, R):
    """One boundary buffer per hist, [B (hist + mc) + 1, R] with a distinct value per element: (device buffers, their host
    bit images, the roll table)."""
    if not hists:
        return [], [], torch.zeros((1, 3), dtype=torch.int64, device=DEV)
    rows = [B * (h + mc) + 1 for h in hists]
    vals = D.roll_values(len(hists), 1, max(rows), R)[:, 0]
    bufs, bits = [], []
    for i, h in enumerate(hists):
        v = vals[i, :rows[i]]
        if dt == F32:
            t = torch.tensor(v.astype(np.float32), device=DEV)
            bits.append(v.astype(np.float32).view(np.int32).copy())
        else:
            b16 = D.roll_bits16(v)
            t = torch.tensor(b16, device=DEV).view(torch.bfloat16)
            bits.append(b16.copy())
        bufs.append(t.contiguous())
    table = torch.tensor([[b.data_ptr(), h + mc, h] for b, h in zip(bufs, hists)], dtype=torch.int64, device=DEV)
    return bufs, bits, table


def _roll_check(what, dt, bufs, bits, hists, B, mc, ns):
    """Stream b of every buffer rolled by ns[b] rows (0: untouched): rows [0, hist) are the old rows [n, n + hist), every
    other element -- the rows behind, the other streams, the spare row -- is intact."""
    torch.cuda.synchronize()
    for i, h in enumerate(hists):
        got = bufs[i].view(torch.int32 if dt == F32 else torch.int16).cpu().numpy()
        want = bits[i].copy()
        clip = h + mc
        for b in range(B):
            if ns[b] > 0:
                want[b * clip:b * clip + h] = bits[i][b * clip + ns[b]:b * clip + ns[b] + h]
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s buffer %d (hist %d): %d elements wrong, first at %s" % (what, i, h, len(bad), bad[0].tolist())


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", [32, 64])
def test_recog_roll_moves_every_row_once(R, dt):
    """hist on both sides of the 64-row step of fp32 R = 64 and of the 256-row step of bf16 R = 32; n < hist (overlapping
    ranges), n = hist, n > hist; nroll 0, 1, 3 with a different hist per buffer; carry[b] = x[b][n - 1]; the clock is
    old + n from 0 and from 2^33."""
    B = 2
    assert sorted({h for hs, _ in D.ROLL_CASES for h in hs}) == D.ROLL_HISTS
    for (hists, ns) in D.ROLL_CASES:
        mc = max(ns)
        for n in ns:
            for old in (0, T33):
                bufs, bits, table = _roll_buffers(dt, hists, B, mc, R)
                x = _dev(D.audio((B, mc), n))
                carry = _nan((B + 1,))
                clock = torch.tensor([old, SENT], dtype=torch.int64, device=DEV)
                _call("srwn_recog_roll", table.data_ptr() if hists else None, len(hists), x.data_ptr(), mc, carry.data_ptr(),
                      clock.data_ptr(), B, n, mc, R, _abi(dt), _st())
                what = "recog_roll %s R %d hists %s n %d" % (NAME[dt], R, hists, n)
                _roll_check(what, dt, bufs, bits, hists, B, mc, [n] * B)
                assert torch.equal(carry[:B], x[:, n - 1]) and bool(torch.isnan(carry[B])), what + ": carry"
                assert clock.tolist() == [old + n, SENT], what + ": clock"


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R", [32, 64])
def test_recog_roll_slots_moves_every_slot_by_its_own_ran(R, dt):
    """Slot 0 rolls by n, slot 1 is idle, slot 2 has ran = 0 (both untouched), slot 3 rolls by n // 2; nroll = 0 returns 0
    without a launch."""
    cap = 4
    for (hists, ns) in D.ROLL_CASES:
        mc = max(ns)
        for n in ns:
            slots = [(T33 + 3, n), (-1, 0), (9, 0), (64, n // 2)]
            bufs, bits, table = _roll_buffers(dt, hists, cap, mc, R)
            tb = _table(slots)
            keep = tb.clone()
            _call("srwn_recog_roll_slots", table.data_ptr() if hists else None, len(hists), tb.data_ptr(), cap, n, mc, R, _abi(dt), _st())
            what = "recog_roll_slots %s R %d hists %s n %d" % (NAME[dt], R, hists, n)
            _roll_check(what, dt, bufs, bits, hists, cap, mc, [n, 0, 0, n // 2])
            assert torch.equal(tb, keep), what + ": the table is the host's"


# ---- score head and nll rows -----------------------------------------------------------------------------------------------
def _score_outputs(B, mc, C):
    nb, nll = _spare(B * mc, 1)
    bb, best = _spare_int(B * mc, 1)
    lb, lo = _spare(B * mc, C)
    return (nb, bb, lb), (nll, best, lo)


def _score_check(what, mode, d, rans, mc, bufs, pairs):
    """rans [B]: the rows each stream has (design row b * max(rans) + t).  Returns the device's (nll, best, logits)."""
    B, n, C = len(rans), max(rans), d["C"]
    written = np.zeros((B, mc), bool)
    for b, r in enumerate(rans):
        written[b, :r] = True
    nll = _intact(what + " nll", bufs[0], B * mc, written).reshape(B, mc)
    best = _intact(what + " best", bufs[1], B * mc, written).reshape(B, mc)
    lo = _intact(what + " logits_out", bufs[2], B * mc, written).reshape(B, mc, C)
    _, _, lg, e2 = D.head_ref(d, mode)
    code = D.codes(d)
    sel = np.array([b * n + t for b, r in enumerate(rans) for t in range(r)], int)
    got_lg = np.concatenate([lo[b, :r] for b, r in enumerate(rans)])
    got_nll = np.concatenate([nll[b, :r] for b, r in enumerate(rans)])
    got_best = np.concatenate([best[b, :r] for b, r in enumerate(rans)]).astype(int)
    lg, code = lg[sel], code[sel]
    want_best, gap = D.top_gap(lg, pairs)
    if mode == "bf16":
        _exact(what + " logits_out", got_lg, G.round_out(lg, "fp32"))
        assert np.array_equal(got_best, want_best), "%s: best differs from the lowest index of the exact maximum at rows %s" % (
            what, np.nonzero(got_best != want_best)[0][:5].tolist())
        base = lg
    else:
        e2 = e2[sel]
        _bounded(what + " logits_out", "score_logits_fp32", mode, got_lg, lg, e2)
        assert np.array_equal(got_best, got_lg.argmax(1)), what + ": best is not the lowest index of the returned maximum"
        clear = gap > 2 * D.C_GPU["score_logits_fp32"]["fp32"] * (D.EPS * np.abs(lg) + e2).max(1)
        assert np.array_equal(got_best[clear], want_best[clear]), what + ": best differs from the exact argmax across a clear gap"
        base = got_lg
    ref, m, lc, ls = D.nll64(base, code)
    _bounded(what + " nll", "score_nll", mode, got_nll, ref, D.nll_scale(ref, m, lc, ls, C) - D.EPS * np.abs(ref))
    return nll, best, lo


def _score_case(dt, R, S, C, B, n, slots=False):
    mode, L = NAME[dt], 3
    mc = n + 3
    d = D.head(L, R, S, B * n, C)
    ibuf, (pskip, pw1, pw2) = _head_images(dt, d, L, R, S)
    rans = [n] * B
    tb = ()
    if slots:
        rans = [n, 0, n // 2][:B]
        table = _table([(T33 + 1, n), (-1, 0), (5, n // 2)][:B])
        tb = (table.data_ptr(),)
    z = _nan((L, B, mc, R), dt)
    zd = _dev(d["z"], dt).view(L, B, n, R)
    for b, r in enumerate(rans):
        z[:, b, :r] = zd[:, b, :r]
    codes = torch.full((B, mc), 1 << 20, dtype=torch.int32, device=DEV)
    cd = _dev(D.codes(d).reshape(B, n), torch.int32)
    for b, r in enumerate(rans):
        codes[b, :r] = cd[b, :r]
    bs, b1, b2 = _dev(d["bs"]), _dev(d["b1"]), _dev(d["b2"])
    bufs, (nll, best, lo) = _score_outputs(B, mc, C)
    sfx = "_slots" if slots else ""
    _call("srwn_stream_score_head" + sfx, z.data_ptr(), B * mc * R, mc, L, pskip, bs.data_ptr(), pw1, b1.data_ptr(), pw2, b2.data_ptr(),
          codes.data_ptr(), nll.data_ptr(), best.data_ptr(), lo.data_ptr(), mc, B, n, mc, R, S, C, _abi(dt), *tb, _st())
    what = "stream_score_head%s %s R %d S %d C %d B %d n %d" % (sfx, mode, R, S, C, B, n)
    g_nll, g_best, g_lo = _score_check(what, mode, d, rans, mc, bufs, d["pairs"])
    # srwn_nll_rows on the head's own logits_out: the head's nll and best, bit for bit -- also at ld > C with 1e30 behind C
    written = np.zeros((B, mc), bool)
    for b, r in enumerate(rans):
        written[b, :r] = True
    for ld in (C, C + 5):
        src = torch.full((B * mc, ld), 1e30, dtype=F32, device=DEV)
        src[:, :C] = torch.nan_to_num(lo, nan=0.0)                     # (the rows beyond ran are never read as live rows)
        tbufs, (tn, tbst, tl) = _score_outputs(B, mc, C)
        _call("srwn_nll_rows" + sfx, src.data_ptr(), ld, mc, codes.data_ptr(), tn.data_ptr(), tbst.data_ptr(), tl.data_ptr(), mc, B, n, C,
              *tb, _st())
        w2 = "%s, nll_rows%s ld %d" % (what, sfx, ld)
        _exact(w2 + " nll", _intact(w2 + " nll", tbufs[0], B * mc, written).reshape(B, mc)[written], g_nll[written])
        assert np.array_equal(_intact(w2 + " best", tbufs[1], B * mc, written).reshape(B, mc)[written], g_best[written]), w2
        _exact(w2 + " logits_out", _intact(w2 + " logits_out", tbufs[2], B * mc, written).reshape(B, mc, C)[written], g_lo[written])


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("C", D.SCORE_C)
def test_stream_score_head_entries(C, dt):
    """(R, S) = (32, 128) at every class count: C below, at and above the 8 lanes of a row and the 32 columns of a tile."""
    for (B, n) in D.SCORE_CLIPS:
        _score_case(dt, 32, 128, C, B, n)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("C", [256, 100])
@pytest.mark.parametrize("R,S", D.WIDTHS[1:])
def test_stream_score_head_entries_other_widths(R, S, C, dt):
    for (B, n) in D.SCORE_CLIPS:
        _score_case(dt, R, S, C, B, n)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("R,S,C", [(32, 128, 9), (32, 128, 100), (64, 256, 256), (64, 128, 33)])
def test_stream_score_head_slots_entries(R, S, C, dt):
    """The slot forms: slot 0 with all n rows, slot 1 idle (its z is NaN), slot 2 with ran = n // 2: the same references per
    row, and the tiles at or behind ran write nothing."""
    for n in (31, 33, 45, 66):
        _score_case(dt, R, S, C, 3, n, slots=True)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("M", D.MOL_M)
def test_stream_mol_score_head_logits_and_twin(M, dt):
    """srwn_stream_mol_score_head on the chained design with 4 M logits: logits_out bit for bit in bf16 (every row finite in
    fp32), and its nll has the bits of srwn_mol_score_rows on those logits (tests/test_gpu_mol_entries.py holds the rows
    kernel to fp64); the rows from n on keep their poison."""
    mode, L, R, S, C = NAME[dt], 3, 32, 128, 4 * M
    for (B, n) in D.MOL_CLIPS:
        mc = n + 3
        d = D.head(L, R, S, B * n, C)
        ibuf, (pskip, pw1, pw2) = _head_images(dt, d, L, R, S)
        z = _nan((L, B, mc, R), dt)
        z[:, :, :n] = _dev(d["z"], dt).view(L, B, n, R)
        x = _nan((B, mc)); x[:, :n] = _dev(D.audio((B, n), M))
        bs, b1, b2 = _dev(d["bs"]), _dev(d["b1"]), _dev(d["b2"])
        nb, nll = _spare(B * mc, 1)
        lb, lo = _spare(B * mc, C)
        _call("srwn_stream_mol_score_head", z.data_ptr(), B * mc * R, mc, L, pskip, bs.data_ptr(), pw1, b1.data_ptr(), pw2, b2.data_ptr(),
              x.data_ptr(), mc, nll.data_ptr(), lo.data_ptr(), mc, B, n, mc, R, S, M, _abi(dt), _st())
        what = "stream_mol_score_head %s M %d B %d n %d" % (mode, M, B, n)
        written = np.zeros((B, mc), bool); written[:, :n] = True
        g_nll = _intact(what + " nll", nb, B * mc, written)
        g_lo = _intact(what + " logits_out", lb, B * mc, written)
        if mode == "bf16":
            _exact(what + " logits_out", g_lo.reshape(B, mc, C)[:, :n].reshape(B * n, C), G.round_out(D.head_ref(d, mode)[2], "fp32"))
        src = torch.nan_to_num(lo, nan=0.0).contiguous()
        tb, tn = _spare(B * mc, 1)
        tlb, tl = _spare(B * mc, C)
        _call("srwn_mol_score_rows", src.data_ptr(), C, mc, x.data_ptr(), mc, tn.data_ptr(), tl.data_ptr(), mc, B, n, M, _st())
        _exact(what + " nll against mol_score_rows", _intact(what + " twin nll", tb, B * mc, written)[written.reshape(-1)],
               g_nll[written.reshape(-1)])
        _exact(what + " twin logits_out", _intact(what + " twin logits_out", tlb, B * mc, written)[written.reshape(-1)],
               g_lo[written.reshape(-1)])


# ---- embed and match -------------------------------------------------------------------------------------------------------
def _match_outputs(rows, mg):
    db, dist = _spare(rows, mg)
    nb, near = _spare_int(rows, 1)
    mb, dmin = _spare(rows, 1)
    return (db, nb, mb), (dist, near, dmin)


def _match_check(what, bufs, rows, mg, N):
    """dist columns from N on keep their poison; returns (dist [rows, N], nearest, dmin)."""
    N = int(np.clip(N, 0, mg))
    torch.cuda.synchronize()
    dist = _host(bufs[0])
    assert np.isnan(dist[rows]).all() and np.isnan(dist[:rows, N:]).all(), what + ": dist written from column N on"
    assert np.isfinite(dist[:rows, :N]).all(), what + ": dist"
    near = bufs[1].cpu().numpy()
    dmin = _host(bufs[2])
    assert near[rows, 0] == SENT and np.isnan(dmin[rows]).all(), what + ": the row behind the last was written"
    return dist[:rows, :N], near[:rows, 0], dmin[:rows, 0]


@pytest.mark.parametrize("Dm", D.MATCH_D)
def test_gallery_match_exact(Dm):
    """dist = sqrt_f32(f32(1e-8) + ss) bit for bit on dyadic rows (ss exact); a gallery row equal to the embedding gives
    sqrtf(1e-8f); nearest = the lowest index of the minimum with duplicates in another wave, in the same wave and across
    all four; *n_gallery clamped into [0, max_gallery]; N = 0 gives -1 and +inf.  The rows behind max_gallery are NaN."""
    d = D.match(Dm)
    rows, mg = len(d["emb"]), D.MAX_GALLERY
    emb = _dev(d["emb"])
    gal = _nan((mg + 8, Dm)); gal[:mg] = _dev(d["gal"])
    for N in D.MATCH_N:
        count = torch.tensor([N, SENT], dtype=torch.int32, device=DEV)
        bufs, (dist, near, dmin) = _match_outputs(rows, mg)
        _call("srwn_gallery_match", emb.data_ptr(), rows, Dm, gal.data_ptr(), count.data_ptr(), mg, dist.data_ptr(), near.data_ptr(),
              dmin.data_ptr(), _st())
        what = "gallery_match D %d N %d" % (Dm, N)
        gd, gn, gm = _match_check(what, bufs, rows, mg, N)
        wd, wn, wm = D.match_ref(d["emb"], d["gal"], N)
        _exact(what + " dist", gd, wd)
        assert np.array_equal(gn, wn), "%s: nearest %s, want %s" % (what, gn.tolist(), wn.tolist())
        if np.clip(N, 0, mg) == 0:
            assert np.isposinf(gm).all(), what
        else:
            _exact(what + " dmin", gm, wm)
        assert count.tolist() == [N, SENT]


@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("kind", ["dyadic", "gauss"])
def test_window_embed_match_has_the_bits_of_its_parts(kind, slots):
    """emb has the bits of srwn_window_mean's logits on the same ring, clock, w2 and b2; dist, nearest and dmin have the bits
    of srwn_gallery_match (held to the exact reference above) on that emb."""
    k, B, S, Dm, mg = 3, 3, 100, 65, D.MAX_GALLERY
    for (hop, nW) in ((64, 2), (32, 3)):
        win, rr = hop * nW, nW + k - 1
        h = D.wm_head(S, Dm, Dm + 3)
        ring = D.ringrows(B, rr, S, nW)
        if kind == "gauss":
            ring = np.random.default_rng(hop).normal(0, 1, ring.shape)
        m = D.match(Dm)
        rd, w2, b2, gal = _dev(ring), _dev(h["w2"]), _dev(h["b2"]), _dev(m["gal"])
        count = torch.tensor([70], dtype=torch.int32, device=DEV)
        sfx = "_slots" if slots else ""
        clock = (_table([((2 * rr - 1) * hop, k * hop), (-1, 0), ((T33 + 1) * hop, hop)]) if slots
                 else torch.tensor([(2 * rr - 1) * hop], dtype=torch.int64, device=DEV))
        rows = B * k
        ebuf, emb = _spare(rows, Dm)
        bufs, (dist, near, dmin) = _match_outputs(rows, mg)
        _call("srwn_window_embed_match" + sfx, rd.data_ptr(), rr, clock.data_ptr(), B, k, hop, win, S, w2.data_ptr(), b2.data_ptr(), Dm,
              Dm + 3, gal.data_ptr(), count.data_ptr(), mg, emb.data_ptr(), dist.data_ptr(), near.data_ptr(), dmin.data_ptr(), _st())
        what = "window_embed_match%s %s hop %d nW %d" % (sfx, kind, hop, nW)
        ge = _intact(what + " emb", ebuf, rows)
        gd, gn, gm = _match_check(what, bufs, rows, mg, 70)
        mbuf, mean = _spare(rows, S)
        lbuf, lg = _spare(rows, Dm)
        _call("srwn_window_mean" + sfx, rd.data_ptr(), rr, mean.data_ptr(), clock.data_ptr(), B, k, hop, win, S, w2.data_ptr(),
              b2.data_ptr(), lg.data_ptr(), Dm, Dm + 3, _st())
        _exact(what + " emb against window_mean's logits", ge, _intact(what + " logits", lbuf, rows))
        tbufs, (td, tn, tm) = _match_outputs(rows, mg)
        _call("srwn_gallery_match", emb.data_ptr(), rows, Dm, gal.data_ptr(), count.data_ptr(), mg, td.data_ptr(), tn.data_ptr(),
              tm.data_ptr(), _st())
        wd, wn, wm = _match_check(what + " twin", tbufs, rows, mg, 70)
        _exact(what + " dist", gd, wd)
        _exact(what + " dmin", gm, wm)
        assert np.array_equal(gn, wn), what


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refused(code, outs, name, *args):
    with pytest.raises(RuntimeError, match=r"\(code %d\)" % code):
        _call(name, *args)
    torch.cuda.synchronize()
    for o in outs:
        keep = (o == SENT) if o.dtype in (torch.int32, torch.int64) else torch.isnan(o)
        assert bool(keep.all()), name + ": a refused call wrote an output"


def _vary(base, **kw):
    a = dict(base); a.update(kw)
    return list(a.values())


def test_recog_entry_points_refuse_what_their_headers_refuse():
    R, S, B, k, hop, mc, rr = 32, 128, 2, 2, 8, 16, 3
    dt = _abi(F32)
    z = torch.zeros((1, B, mc, R), device=DEV)
    w = torch.zeros(4096 * 16, device=DEV)
    f = torch.zeros(4096, device=DEV)
    clock = torch.zeros(2, dtype=torch.int64, device=DEV)
    tb = _table([(0, k * hop), (-1, 0)])
    ring, out, mean, lg = _nan((B * rr, S)), _nan((B * mc, R)), _nan((B * k, S)), _nan((B * k, 12))
    p = lambda t: t.data_ptr()
    # stream entry
    base = dict(x=p(f), xs=mc, carry=p(f), w=p(f), b=p(f), out=p(out), clip=mc, hist=0, B=B, n=8, mc=mc, R=R, dt=dt, st=_st())
    for code, kw in ((E_NULL, dict(carry=None)), (E_UNSUPPORTED, dict(R=48)), (E_DTYPE, dict(dt=7)), (E_SHAPE, dict(n=0)),
                     (E_SHAPE, dict(n=mc + 1)), (E_SHAPE, dict(xs=mc - 1)), (E_SHAPE, dict(clip=mc - 1))):
        _refused(code, [out], "srwn_recog_stream_in", *_vary(base, **kw))
    base = dict(x=p(f), rl=mc + 1, w=p(f), b=p(f), out=p(out), clip=mc, hist=0, B=B, n=8, mc=mc, R=R, dt=dt, tb=p(tb), st=_st())
    for code, kw in ((E_NULL, dict(tb=None)), (E_UNSUPPORTED, dict(R=48)), (E_DTYPE, dict(dt=7)), (E_SHAPE, dict(n=0)),
                     (E_SHAPE, dict(n=mc + 1)), (E_SHAPE, dict(rl=mc))):
        _refused(code, [out], "srwn_recog_stream_in_slots", *_vary(base, **kw))
    # pooled head, both forms
    for name, ck in (("srwn_pooled_stream_head", p(clock)), ("srwn_pooled_stream_head_slots", p(tb))):
        base = dict(z=p(z), zs=B * mc * R, zc=mc, L=1, ws=p(w), bs=p(f), w1=p(w), b1=p(f), ring=p(ring), rr=rr, ck=ck, B=B, k=k, hop=hop,
                    mc=mc, R=R, S=S, dt=dt, st=_st())
        for code, kw in ((E_NULL, dict(ck=None)), (E_NULL, dict(z=None)), (E_UNSUPPORTED, dict(R=48)), (E_UNSUPPORTED, dict(S=64)),
                         (E_DTYPE, dict(dt=7)), (E_SHAPE, dict(k=3)), (E_SHAPE, dict(hop=0)), (E_SHAPE, dict(zs=B * mc * R - 1)),
                         (E_SHAPE, dict(L=0))):
            _refused(code, [ring], name, *_vary(base, **kw))
    # hop sum, both forms
    r1 = torch.zeros((B, mc, S), device=DEV)
    for name, ck in (("srwn_hop_sum", p(clock)), ("srwn_hop_sum_slots", p(tb))):
        base = dict(r1=p(r1), rc=mc, ring=p(ring), rr=rr, ck=ck, B=B, k=k, hop=hop, mc=mc, S=S, dt=dt, st=_st())
        for code, kw in ((E_NULL, dict(r1=None)), (E_DTYPE, dict(dt=7)), (E_SHAPE, dict(k=3)), (E_SHAPE, dict(S=5)), (E_SHAPE, dict(S=0)),
                         (E_SHAPE, dict(rc=mc - 1)), (E_SHAPE, dict(rr=0))):
            _refused(code, [ring], name, *_vary(base, **kw))
    # window mean, both forms
    rg = torch.zeros((B, rr, S), device=DEV)
    for name, ck in (("srwn_window_mean", p(clock)), ("srwn_window_mean_slots", p(tb))):
        base = dict(ring=p(rg), rr=rr, mean=p(mean), ck=ck, B=B, k=k, hop=hop, win=2 * hop, S=S, w2=p(f), b2=p(f), lg=p(lg), C=12, ldw=12,
                    st=_st())
        for code, kw in ((E_NULL, dict(mean=None)), (E_NULL, dict(w2=None)), (E_SHAPE, dict(rr=2)), (E_SHAPE, dict(win=2 * hop + 1)),
                         (E_SHAPE, dict(win=hop - 1)), (E_SHAPE, dict(S=257)), (E_SHAPE, dict(ldw=11)), (E_SHAPE, dict(C=0))):
            _refused(code, [mean, lg], name, *_vary(base, **kw))
    # roll, both forms
    buf = _nan((B * (4 + mc), R))
    table = torch.tensor([[buf.data_ptr(), 4 + mc, 4]], dtype=torch.int64, device=DEV)
    carry = _nan((B,))
    base = dict(t=p(table), nr=1, x=p(f), xs=mc, carry=p(carry), ck=p(clock), B=B, n=8, mc=mc, R=R, dt=dt, st=_st())
    for code, kw in ((E_NULL, dict(t=None)), (E_NULL, dict(carry=None)), (E_UNSUPPORTED, dict(R=48)), (E_DTYPE, dict(dt=7)),
                     (E_SHAPE, dict(n=0)), (E_SHAPE, dict(n=mc + 1)), (E_SHAPE, dict(xs=mc - 1)), (E_SHAPE, dict(nr=-1))):
        _refused(code, [buf, carry], "srwn_recog_roll", *_vary(base, **kw))
    assert clock.tolist() == [0, 0]
    base = dict(t=p(table), nr=1, tb=p(tb), B=B, n=8, mc=mc, R=R, dt=dt, st=_st())
    for code, kw in ((E_NULL, dict(tb=None)), (E_UNSUPPORTED, dict(R=48)), (E_DTYPE, dict(dt=7)), (E_SHAPE, dict(n=0)),
                     (E_SHAPE, dict(n=mc + 1))):
        _refused(code, [buf], "srwn_recog_roll_slots", *_vary(base, **kw))


def test_score_and_match_entry_points_refuse_what_their_headers_refuse():
    R, S, B, n, mc, C = 32, 128, 2, 8, 16, 12
    dt = _abi(F32)
    z = torch.zeros((1, B, mc, R), device=DEV)
    w = torch.zeros(4096 * 16, device=DEV)
    f = torch.zeros(4096, device=DEV)
    codes = torch.zeros((B, mc), dtype=torch.int32, device=DEV)
    tb = _table([(0, n), (-1, 0)])
    nll, lo = _nan((B * mc,)), _nan((B * mc, C))
    best = torch.full((B * mc,), SENT, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    outs = [nll, best, lo]
    for name, tail in (("srwn_stream_score_head", {}), ("srwn_stream_score_head_slots", dict(tb=p(tb)))):
        base = dict(z=p(z), zs=B * mc * R, zc=mc, L=1, ws=p(w), bs=p(f), w1=p(w), b1=p(f), w2=p(w), b2=p(f), codes=p(codes), nll=p(nll),
                    best=p(best), lo=p(lo), os=mc, B=B, n=n, mc=mc, R=R, S=S, C=C, dt=dt, **tail, st=_st())
        base["st"] = base.pop("st")
        cases = [(E_NULL, dict(codes=None)), (E_NULL, dict(nll=None)), (E_UNSUPPORTED, dict(R=48)), (E_UNSUPPORTED, dict(S=64)),
                 (E_DTYPE, dict(dt=7)), (E_SHAPE, dict(n=mc + 1)), (E_SHAPE, dict(os=n - 1)), (E_SHAPE, dict(zs=1)),
                 (E_UNSUPPORTED if tail else E_SHAPE, dict(C=257))]
        cases += [(E_NULL, dict(tb=None))] if tail else [(E_SHAPE, dict(n=0))]
        for code, kw in cases:
            _refused(code, outs, name, *_vary(base, **kw))
    lg = torch.zeros((B * mc, C), device=DEV)
    for name, tail in (("srwn_nll_rows", {}), ("srwn_nll_rows_slots", dict(tb=p(tb)))):
        base = dict(lg=p(lg), ld=C, cr=mc, codes=p(codes), nll=p(nll), best=p(best), lo=p(lo), os=mc, B=B, n=n, C=C, **tail, st=_st())
        base["st"] = base.pop("st")
        cases = [(E_NULL, dict(lg=None)), (E_SHAPE, dict(ld=C - 1)), (E_SHAPE, dict(cr=n - 1)), (E_UNSUPPORTED if tail else E_SHAPE, dict(C=0))]
        cases += [] if tail else [(E_SHAPE, dict(n=0))]
        for code, kw in cases:
            _refused(code, outs, name, *_vary(base, **kw))
    out = _nan((B * mc, R))
    cbuf = torch.full((B, mc), SENT, dtype=torch.int32, device=DEV)
    base = dict(ring=p(f), rl=mc + 2, w=p(f), b=p(f), out=p(out), clip=mc, hist=0, codes=p(cbuf), cs=mc, B=B, n=n, mc=mc, R=R, C=256, dt=dt,
                tb=p(tb), st=_st())
    for code, kw in ((E_NULL, dict(codes=None)), (E_UNSUPPORTED, dict(R=48)), (E_UNSUPPORTED, dict(C=1)), (E_DTYPE, dict(dt=7)),
                     (E_SHAPE, dict(n=mc + 1)), (E_SHAPE, dict(rl=mc + 1)), (E_SHAPE, dict(cs=mc - 1))):
        _refused(code, [out, cbuf], "srwn_score_stream_in_slots", *_vary(base, **kw))
    # embed and match
    k, hop, rr, Dm, mg = 2, 8, 3, 12, 16
    clock = torch.zeros(1, dtype=torch.int64, device=DEV)
    count = torch.tensor([3], dtype=torch.int32, device=DEV)
    emb, dist, dmin = _nan((B * k, Dm)), _nan((B * k, mg)), _nan((B * k,))
    near = torch.full((B * k,), SENT, dtype=torch.int32, device=DEV)
    outs = [emb, dist, near, dmin]
    for name, ck in (("srwn_window_embed_match", p(clock)), ("srwn_window_embed_match_slots", p(tb))):
        base = dict(ring=p(f), rr=rr, ck=ck, B=B, k=k, hop=hop, win=2 * hop, S=S, w2=p(f), b2=p(f), D=Dm, ldw=Dm, gal=p(f), cnt=p(count), mg=mg,
                    emb=p(emb), dist=p(dist), near=p(near), dmin=p(dmin), st=_st())
        for code, kw in ((E_NULL, dict(cnt=None)), (E_SHAPE, dict(D=257)), (E_SHAPE, dict(mg=1025)), (E_SHAPE, dict(rr=2)),
                         (E_SHAPE, dict(win=2 * hop + 1)), (E_SHAPE, dict(S=257)), (E_SHAPE, dict(ldw=Dm - 1))):
            _refused(code, outs, name, *_vary(base, **kw))
    base = dict(emb=p(f), rows=B * k, D=Dm, gal=p(f), cnt=p(count), mg=mg, dist=p(dist), near=p(near), dmin=p(dmin), st=_st())
    for code, kw in ((E_NULL, dict(gal=None)), (E_SHAPE, dict(D=257)), (E_SHAPE, dict(D=0)), (E_SHAPE, dict(mg=1025)), (E_SHAPE, dict(rows=-1))):
        _refused(code, outs[1:], "srwn_gallery_match", *_vary(base, **kw))
    assert _call("srwn_gallery_match", *_vary(base, rows=0)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dist).all())
