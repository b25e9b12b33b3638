"""GPU tests that hold the multi-layer (group) kernels of csrc/srwn_group.hip ENTRY BY ENTRY to a layer-local float64
reference, where tests/test_gpu_group.py holds them to their per-layer twins in a norm over whole tensors (bf16:
2e-2 .. 3e-2), which one wrong entry, one tap read from a clamped row or one mask off by one passes.

The kernels store df_g and G_g of every layer and hand the STORED gradient from layer to layer, so every layer is
compared with a float64 restatement of that one layer fed with the kernel's own stored operands of the layer above
(tests/group_design.py; no error travels further than one layer).  On the dyadic designs every entry is either
DECIDED -- its float64 value lies farther from a rounding midpoint of the output type than REACH x the entry's own error
scale e, or e = 0 -- and must match the reference BIT FOR BIT, or it is held to ulp(ref) + c (u_out |ref| + e).  REACH and c
are 4 x what the float32 NumPy restatement measures on the same designs (C_CPU of tests/group_design.py, proved by
tests/test_group_design.py on the CPU); never a GPU figure.  Outputs are poisoned with NaN first.

  srwn_residual_group_bwd     df_g and G_g of every layer, fp32 and bf16, R = 32 and 64, with and without g_top and dcs, at
                              the shapes of D.CASES (one position; less than a tile at stride 2; halo 31 in several ragged
                              segments; 17 tiles; residue classes whose lengths differ by one; stride 32 without halo;
                              gcd 3; eight layers), two of them again with two workgroups walking several segments each
  its exact corner            g_top = None, z = 0: the top layer's df = dcs / 2 and G = the taps of df bit for bit with no
                              entry excluded, and every layer's df bit for bit wherever that layer's Wr row is zero
  srwn_residual_group_bwd_wt  write_all_g, tiles written here (G.ct_encode): G_g of every layer through the RECONSTRUCTED df
                              (a sparser conv and z off +-1 keep 90 % of G decided, D.wt_design); dWf, dbf, dWr, dbr after
                              the reduction per entry to c (rows 2^-24 S + the undecided-df term), fp32 slabs and bf16
                              blocks (+ one rounding per segment a workgroup walks); the first group's input conv gradient
                              from dyadic audio, shifts 0 and 1; two workgroups
  its exact corner            g_top = None, z = 0, Wr_top = 0: dWf_top, dbf_top, dWr and dbr of the layer below equal the
                              float64 sums rounded once; bf16 blocks on a sparser design wherever S <= 256 units
  srwn_residual_group_fwd     weight-gradient-tile mode: every element of every xT tile bit-equal to the stored row it
  (and _fwd_ic)               stands for and exactly zero beyond the segment, unowned tiles untouched; cT per entry against
                              the gate of the stored z (layer 0 bit-exact in bf16 mode); store_inner_x = False;
                              conditioning; the input conv fused in on dyadic audio, shifts 0 and 1

fp32 mode: half an ulp of the output lies below the accumulation's own error, so an fp32 entry is decided only where its
value is exact (e = 0); every other one is held by the bound, whose u_out is 2^-24.  The cap on undecided entries (10 % of
every stored tensor) is bf16 mode's, where the twin tests hold the chain to 2e-2 in a norm (tests/group_design.py).

Worst error / scale (|got - float64| / (u_out |ref| + e); weight gradients: / (rows 2^-24 S + ...)), bf16 | fp32:
                         df            G             cT (gate)      dWf    dbf    dWr    dbr    input conv
  float32 NumPy (CPU)    1.992 | 0.481 1.990 | 0.382 1.435 | 0.846  0.594 (one constant for the weight gradients)
  C_CPU (rounded up)     2     | 0.5   2     | 0.4375 1.5  | 0.875  0.625
  bound = 4 x C_CPU      8     | 2     8     | 1.75  6     | 3.5    2.5
  MI355X, measured       1.992 | 0.502 1.992 | 0.360 1.435 | 0.813  0.249 | 0.154   0.249 | 0.072   0.019 | 0.330
                                                                    0.003 | 0.313 (dbr)   0.001 | 0.256 (input conv)
  MI355X, bf16 blocks                                               0.981 (dWf)   0.750 (dWr)
REACH (which entries are decided): 4 x the restatement's worst |value before rounding - float64| / e = 4 x 1.5 | 0.875 (df;
the bf16 figure is set at z = +-1, where the float64 value is 0 and e is the polynomial's residue) and 4 x 0.3125 | 0.4375 (G).
Decided entries on the MI355X, bf16: >= 96.4 % of every df and G (df stored), >= 98.8 % of every G (df reconstructed); every
one of them has the reference's bits.  The whole file takes about 7 s, no case more than half a second.

Mutations on scratch builds (in-bounds arithmetic only; never committed): tests of this file that fail, of 175 / the
123 existing group-kernel tests of tests/test_gpu_group.py (forward / backward / _wt twins, input conv, oracle, skip
gradient from tiles) and tests/test_gpu_multiseg.py (capped grid, bf16 partials) that pass with the mutated library:
  a tap reading row src + 1 in the last tile of a segment      110 fail / 94 of 123 still pass
  the ownership mask col < hi made <= when parking G            26 fail / 116 still pass
  sqrt(1/2) dropped for the second tile's accG                  64 fail / 110 still pass
  the sit > 0 read-back of one dWr block skipped                 8 fail / 106 still pass (tests/test_gpu_multiseg.py fails 15)
  ONE df entry per segment off by 3 %                          118 fail / 108 still pass -- EVERY bf16 test among them; only
                                                                          the fp32 twins' bit-equality notices
  two positions of kordW swapped in wt_store_tile               36 fail / 86 still pass
The twin tests run the mutated code on both sides of most comparisons (plain group kernel against the _wt one, capped
against uncapped grid, bf16 blocks against fp32 slabs), so they pass whatever it computes; the tests here compare with
a reference that is not the kernel.

SRWN_PRINT_ERR=1 pytest -s prints, per case, the worst ratio per key and the decided share.
"""
import os

import numpy as np
import pytest
import torch

from tests import gemm_design as G
from tests import group_design as D
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


def _pack_T(d, dt):
    """The transposed MFMA images the backward kernels take: (buffer, conv pointers, 1x1 pointers), as the engine packs."""
    K = sub("kernels"); P = sub("packing")
    n, R = len(d["dil"]), d["R"]
    pk = K.Packer(DEV)
    oc = [P.pack_conv_T(pk, l * 2 * R * R, 2, R) for l in range(n)]
    orr = [P.pack_linear_T(pk, n * 2 * R * R + l * R * R, R, R, R, perm=True) for l in range(n)]
    pk.finalize()
    buf = torch.empty(pk.total, dtype=dt, device=DEV)
    pk.gather(torch.cat([_dev(d["wf"]).flatten(), _dev(d["wr"]).flatten()]), buf)
    es = buf.element_size()
    return buf, [buf.data_ptr() + o * es for o in oc], [buf.data_ptr() + o * es for o in orr]


def _run_bwd(d, dt, seg):
    """srwn_residual_group_bwd on a design: (df, G) as float64 [n, B T, R].  The stacks carry one layer slot more than the
    group has: it must keep its poison."""
    K = sub("kernels")
    n, B, T, R = len(d["dil"]), d["B"], d["T"], d["R"]
    buf, pc, pr = _pack_T(d, dt)
    z = _dev(d["z"], dt).view(n, B, T, R)
    dcs = None if d["dcs"] is None else _dev(d["dcs"], dt).view(n, B, T, R)
    gt = None if d["g_top"] is None else _dev(d["g_top"], dt).view(B, T, R)
    g_out, df_out = _nan((n + 1, B, T, R), dt), _nan((n + 1, B, T, R), dt)
    K.residual_group_bwd(gt, g_out, df_out, z, dcs, pc, pr, d["dil"], 2, seg_rows=seg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(g_out[n]).all()) and bool(torch.isnan(df_out[n]).all()), "a store behind the group's layers"
    return _host(df_out[:n]).reshape(n, B * T, R), _host(g_out[:n]).reshape(n, B * T, R)


def _hold(what, key, got, r, mode, stats):
    """Decided entries bit for bit, every entry within its bound."""
    assert np.isfinite(got).all(), what + ": an entry left unwritten (or not finite)"
    dec = D.decided(r, mode, D.REACH[key][mode])
    same = G.same_bits(got, r["ref"])
    bad = np.argwhere(dec & ~same)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d decided entries differ from the layer-local reference, first at %s: got %r, want %r "
                             "(float64 %r, reach %.3g, midpoint distance %.3g)" % (
                                 what, len(bad), int(dec.sum()), list(i), got[i], r["ref"][i], r["x"][i],
                                 D.REACH[key][mode] * r["e"][i], D.midpoint_distance(r["x"], mode)[i]))
    err = np.abs(got - r["x"])
    over = np.argwhere(err > D.bound(r, mode, D.C_GPU[key][mode]))
    assert len(over) == 0, "%s: %d entries beyond their bound, first at %s: got %r, float64 %r" % (
        what, len(over), over[0].tolist(), got[tuple(over[0])], r["x"][tuple(over[0])])
    ratio = float(D.out_ratio(got, r, mode).max())
    k = (key, mode)
    stats[k] = (max(stats.get(k, (0.0, 1.0, 0))[0], ratio), min(stats.get(k, (0.0, 1.0, 0))[1], float(dec.mean())),
                stats.get(k, (0.0, 1.0, 0))[2] + int((~dec & ~same).sum()))


def _hold_chain(what, d, df, Gs, mode):
    """Every layer, top first, against the reference fed with the kernel's own stored gradient of the layer above."""
    stats = {}
    Gup = d["g_top"]
    for l in range(len(d["dil"]) - 1, -1, -1):
        _hold("%s layer %d df" % (what, l), "df", df[l], D.layer_df_ref(d, l, Gup, mode), mode, stats)
        _hold("%s layer %d G" % (what, l), "G", Gs[l], D.layer_G_ref(d, l, Gup, df[l], mode), mode, stats)
        Gup = Gs[l]
    for (key, m), (ratio, share, flips) in sorted(stats.items()):
        _say("%-64s %-2s error / scale %.3f (<= %g)  decided >= %.1f %%  undecided entries that round the other way: %d" % (
            what, key, ratio, D.C_GPU[key][m], 100 * share, flips))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("i,R,variant", D.RUNS)
def test_group_bwd_entries(monkeypatch, dt, i, R, variant):
    """srwn_residual_group_bwd.  Contract (read from the kernel): every row of every clip is owned by exactly one segment,
    so all B T rows of df_g and G_g of all n layers are written and nothing else is (the layer slot behind the group keeps
    its poison); beyond a clip's end there is no gradient -- the adjoint of the delayed tap reads ZERO for t + d >= T, not
    the clamped last row and not the next clip's first rows (the designs put their largest values there) -- and a missing
    g_top is a zero gradient.  A launch with neither g_top nor dcs is refused."""
    monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    dil, B, T, seg = D.CASES[i]
    d = D.design(dil, B, T, R, variant)
    mode = NAME[dt]
    df, Gs = _run_bwd(d, dt, seg)
    _hold_chain("group_bwd %s %s B %d T %d seg %d R %d %s" % (mode, dil, B, T, seg, R, variant), d, df, Gs, mode)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("i", D.GRID2)
def test_group_bwd_entries_two_workgroups(monkeypatch, dt, i):
    """The same with SRWN_GROUP_GRID = 2: each workgroup walks several segments, the LDS image and the registers of one
    segment are what the next one finds."""
    dil, B, T, seg = D.CASES[i]
    d = D.design(dil, B, T, 64, "both")
    monkeypatch.setenv("SRWN_GROUP_GRID", "2")
    try:
        df, Gs = _run_bwd(d, dt, seg)
    finally:
        monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    _hold_chain("group_bwd %s %s B %d T %d seg %d two workgroups" % (NAME[dt], dil, B, T, seg), d, df, Gs, NAME[dt])


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("i", range(len(D.CASES)))
def test_group_bwd_exact_corner(monkeypatch, dt, i):
    """g_top = None and z = 0 (c' is exactly 1/2): the top layer's df = dcs / 2 and G = the taps of df are sums of dyadic
    products in range -- bit for bit, no entry excluded, which also proves the premise (in-range sums are exact in this
    kernel's MFMA accumulation) -- and in every layer df is bit-exact wherever that layer's Wr row is zero."""
    monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    dil, B, T, seg = D.CASES[i]
    mode = NAME[dt]
    for R in (32, 64):
        d = D.design(dil, B, T, R, exact_corner=True)
        n = len(dil)
        df, Gs = _run_bwd(d, dt, seg)
        what = "group_bwd exact corner %s %s B %d T %d seg %d R %d" % (mode, dil, B, T, seg, R)
        dfx, tx, _ = D.exact_top(d)
        for name, got, want in (("df", df[n - 1], D.round_to(dfx, mode)), ("G", Gs[n - 1], D.round_to(tx, mode))):
            ok = G.same_bits(got, want)
            assert ok.all(), "%s: top layer %s: %d entries differ, first at %s" % (what, name, (~ok).sum(), np.argwhere(~ok)[0].tolist())
        for l in range(n):
            zero_rows = ~np.abs(d["wr"][l]).any(1)
            assert G.same_bits(df[l][:, zero_rows], 0.5 * d["dcs"][l][:, zero_rows]).all(), "%s: layer %d df where Wr = 0" % (what, l)
        _hold_chain(what, d, df, Gs, mode)


def test_group_bwd_refusals():
    """What the entry point refuses: no gradient source at all, more than kMaxGroup layers, a halo beyond 31."""
    K = sub("kernels")
    d = D.design([1, 2, 4], 1, 8, 32, "both")
    buf, pc, pr = _pack_T(d, F32)
    z = _dev(d["z"]).view(3, 1, 8, 32)
    out = lambda: _nan((3, 1, 8, 32), F32)
    with pytest.raises(RuntimeError, match="no top gradient"):
        K.residual_group_bwd(None, out(), out(), z, None, pc, pr, [1, 2, 4], 2)
    with pytest.raises(RuntimeError, match="halo"):
        K.residual_group_bwd(None, out(), out(), z, z, pc, pr, [1, 2, 29], 2)
    z9 = _nan((9, 1, 8, 32), F32)
    with pytest.raises(RuntimeError, match="nlayers"):
        K.residual_group_bwd(None, z9.clone(), z9.clone(), z9, z9, pc * 3, pr * 3, [1] * 9, 2)


# ---- srwn_residual_group_fwd / _fwd_ic in the weight-gradient-tile mode ---------------------------------------------------
def _pack_fwd(d, dt):
    K = sub("kernels"); P = sub("packing")
    n, R = len(d["dil"]), d["R"]
    pk = K.Packer(DEV)
    oc = [P.pack_conv(pk, l * 2 * R * R, 2, R) for l in range(n)]
    orr = [P.pack_res(pk, n * 2 * R * R + l * R * R, R) for l in range(n)]
    pk.finalize()
    buf = torch.empty(pk.total, dtype=dt, device=DEV)
    pk.gather(torch.cat([_dev(d["wf"]).flatten(), _dev(d["wr"]).flatten()]), buf)
    es = buf.element_size()
    return buf, [buf.data_ptr() + o * es for o in oc], [buf.data_ptr() + o * es for o in orr]


def _run_fwd(d, dt, seg, store_inner_x=True, ic=None):
    """The forward group kernel with tiles: dict of x_out, z_out [n, B T, R], xT, cT [n, nseg, KT, 4, 8, R] (float64) and
    the geometry.  ic = (design, shift): the input conv fused in instead of input rows."""
    K = sub("kernels")
    n, B, T, R = len(d["dil"]), d["B"], d["T"], d["R"]
    buf, pc, pr = _pack_fwd(d, dt)
    W, KT, elems, ns = K.group_wt_geometry(d["dil"], B, T, R, dt, seg)
    st = int(np.gcd.reduce(d["dil"]))
    row, ok = G.ct_rows(B, T, st, W)
    nseg = row.shape[0]
    assert row.shape[1] == KT and nseg * KT * R * 32 == elems and ns >= 1
    x_out, z_out = _nan((n + 1, B, T, R), dt), _nan((n + 1, B, T, R), dt)
    xT, cT = _nan((n + 1, elems + 64), dt), _nan((n + 1, elems + 64), dt)
    bfs, brs = [_dev(d["bf"][l]) for l in range(n)], [_dev(d["br"][l]) for l in range(n)]
    if ic is None:
        kw = {}
        if d["cond"] is not None:
            kw = dict(cond=_dev(d["cond"], dt), cond_channel_offsets=[g * R for g in range(n)], pool_stride=d["pool"])
        K.residual_group_fwd(_dev(d["x"], dt).view(B, T, R), x_out, z_out, pc, pr, bfs, brs, d["dil"], 2, seg_rows=W, xT=xT,
                             cT=cT, store_inner_x=store_inner_x, **kw)
    else:
        K.residual_group_fwd_ic(_dev(ic[0]["audio"]), _dev(ic[0]["w"]), _dev(ic[0]["b"]), ic[1], x_out, z_out, pc, pr, bfs, brs,
                                d["dil"], 2, seg_rows=W, xT=xT, cT=cT, store_inner_x=store_inner_x)
    torch.cuda.synchronize()
    for name, t in (("x_out", x_out), ("z_out", z_out)):
        assert bool(torch.isnan(t[n]).all()), name + ": a store behind the group's layers"
    for name, t in (("xT", xT), ("cT", cT)):
        assert bool(torch.isnan(t[n]).all()) and bool(torch.isnan(t[:, elems:]).all()), name + ": a store outside the tiles"
    dec = lambda t: np.stack([D.ct_decode(_host(t[l]), nseg, KT, R) for l in range(n)])
    return dict(x=_host(x_out[:n]).reshape(n, B * T, R), z=_host(z_out[:n]).reshape(n, B * T, R), xT=dec(xT), cT=dec(cT),
                row=row, ok=ok, written=D.tile_written(B, T, st, W), W=W, st=st)


def _hold_tiles(what, d, o, mode, x0):
    """xT: every element of every written tile is the stored row it stands for, bit for bit, and exactly zero beyond the
    segment; a tile the segment owns no position of keeps its poison (both tile stacks).  cT: per entry against the gate of
    the stored z."""
    n = len(d["dil"])
    row, ok, written = o["row"], o["ok"], o["written"]
    wr4 = np.broadcast_to(written[:, :, None, None], ok.shape)
    for l in range(n):
        src = x0 if l == 0 else o["x"][l - 1]
        xt, ct = o["xT"][l], o["cT"][l]
        assert np.isfinite(o["z"][l]).all(), "%s: z of layer %d" % (what, l)
        same = G.same_bits(xt[ok], src[row[ok]])
        assert same.all(), "%s: xT of layer %d: %d owned elements differ from their rows" % (what, l, (~same).sum())
        assert (xt[wr4 & ~ok] == 0).all(), "%s: xT of layer %d is not zero beyond a segment" % (what, l)
        assert np.isnan(xt[~wr4]).all() and np.isnan(ct[~wr4]).all(), "%s: layer %d: a tile nobody owns was written" % (what, l)
        z = o["z"][l][row[ok]]
        r = np.abs(ct[ok] - G.gate64(z)) / D.gate_scale(z, mode)
        assert np.isfinite(r).all(), "%s: cT of layer %d" % (what, l)
        _say("%-72s layer %d cT error / scale %.3f (<= %g)" % (what, l, r.max(), D.C_GPU_GATE[mode]))
        assert r.max() <= D.C_GPU_GATE[mode], "%s: cT of layer %d: error / scale %.3g" % (what, l, r.max())


FWD_CASES = list(range(len(D.CASES)))


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("i", FWD_CASES)
def test_group_fwd_tiles(monkeypatch, dt, i):
    """srwn_residual_group_fwd with xT / cT, store_inner_x = True and False.  Contract (read from the kernel): a segment
    writes the tiles it owns a position of, whole -- xT with zeros beyond its last owned position, cT with whatever the
    image holds there (finite; the backward kernels mask it) -- and no other tile; every row of z is written; with
    store_inner_x = False the inner layers' output rows keep their poison and everything else has the same bits.  Layer 0's
    cT is bit-exact in bf16 mode (an exact pre-activation, G.fwd_c_bf16)."""
    monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    dil, B, T, seg = D.CASES[i]
    mode = NAME[dt]
    for R in (64, 32):
        d = D.fwd_design(dil, B, T, R)
        n = len(dil)
        what = "group_fwd_wt %s %s B %d T %d seg %d R %d" % (mode, dil, B, T, seg, R)
        o = _run_fwd(d, dt, seg)
        assert np.isfinite(o["x"]).all(), what
        _hold_tiles(what, d, o, mode, d["x"])
        if dt == BF16:
            c0 = G.fwd_c_bf16(G.fwd_pre(dict(x=d["x"], wf=d["wf"][0], bf=d["bf"][0]), B, T, dil[0]))
            same = G.same_bits(o["cT"][0][o["ok"]], c0[o["row"][o["ok"]]])
            assert same.all(), "%s: cT of layer 0: %d elements differ from the exact gate" % (what, (~same).sum())
        p = _run_fwd(d, dt, seg, store_inner_x=False)
        assert np.isnan(p["x"][:n - 1]).all(), what + ": store_inner_x = False wrote an inner layer's rows"
        assert G.same_bits(p["x"][n - 1], o["x"][n - 1]).all() and G.same_bits(p["z"], o["z"]).all(), what
        wr4 = np.broadcast_to(o["written"][None, :, :, None, None, None], o["xT"].shape)
        assert G.same_bits(p["xT"][wr4], o["xT"][wr4]).all(), what
        ok6 = np.broadcast_to(o["ok"][None, :, :, :, :, None], o["cT"].shape)
        assert G.same_bits(p["cT"][ok6], o["cT"][ok6]).all(), what


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("i", D.GRID2)
def test_group_fwd_tiles_two_workgroups(monkeypatch, dt, i):
    dil, B, T, seg = D.CASES[i]
    d = D.fwd_design(dil, B, T, 64)
    monkeypatch.setenv("SRWN_GROUP_GRID", "2")
    try:
        o = _run_fwd(d, dt, seg)
    finally:
        monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    _hold_tiles("group_fwd_wt %s %s B %d T %d seg %d two workgroups" % (NAME[dt], dil, B, T, seg), d, o, NAME[dt], d["x"])


@pytest.mark.parametrize("dt", [F32, BF16])
def test_group_fwd_tiles_conditioned(monkeypatch, dt):
    """Conditioning rows (pool_stride 8, frames that do not divide T): the stored rows and the tiles of the layer above
    both include the conditioning bias."""
    monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    dil, B, T, seg = D.CASES[2]
    d = D.fwd_design(dil, B, T, 64, cond_pool=8)
    d["pool"] = 8
    o = _run_fwd(d, dt, seg)
    _hold_tiles("group_fwd_wt conditioned %s" % NAME[dt], d, o, NAME[dt], d["x"])
    plain = dict(d, cond=None)
    q = _run_fwd(plain, dt, seg)
    assert G.same_bits(q["z"][0], o["z"][0]).all() and not G.same_bits(q["x"][0], o["x"][0]).all()


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("i", [1, 2, 4])
def test_group_fwd_ic_tiles(monkeypatch, dt, shift, i):
    """srwn_residual_group_fwd_ic on dyadic audio and a dyadic input conv: x_0 is exact, so layer 0's xT tiles must hold
    it bit for bit, and every stored row and tile must have the bits of the run that is given x_0 as rows."""
    monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    dil, B, T, seg = D.CASES[i]
    R = 64 if i != 1 else 32
    d = D.fwd_design(dil, B, T, R)
    icd = D.ic_design(B, T, R)
    x0 = D.ic_x0(icd, B, T, shift)
    what = "group_fwd_ic %s %s B %d T %d shift %d" % (NAME[dt], dil, B, T, shift)
    o = _run_fwd(d, dt, seg, ic=(icd, shift))
    _hold_tiles(what, d, o, NAME[dt], x0)
    q = _run_fwd(dict(d, x=x0), dt, seg)
    for k in ("x", "z"):
        assert G.same_bits(o[k], q[k]).all(), "%s: %s differs from the run on stored input rows" % (what, k)
    wr4 = np.broadcast_to(o["written"][None, :, :, None, None, None], o["xT"].shape)
    assert G.same_bits(o["xT"][wr4], q["xT"][wr4]).all(), what


# ---- srwn_residual_group_bwd_wt, write_all_g ------------------------------------------------------------------------------
def _reduce(p, ns, per, nbatch, cols16=None):
    K = sub("kernels")
    out = _nan((nbatch, per), F32)
    job = (p, ns, per, nbatch, True, 1.0, out.data_ptr(), per)
    K.reduce_partials_multi([job + (cols16,) if cols16 else job])
    return _host(out)


def _run_bwd_wt(d, dt, seg, part16=False, ic_shift=None):
    """srwn_residual_group_bwd_wt on tiles WRITTEN HERE (G.ct_encode): xT zero beyond a segment inside the tiles it owns (the
    forward kernel's contract), 256 in the tiles it does not; cT 256 everywhere beyond a segment.  Returns the stored G of
    every layer and the reduced weight gradients."""
    K = sub("kernels")
    n, B, T, R = len(d["dil"]), d["B"], d["T"], d["R"]
    buf, pc, pr = _pack_T(d, dt)
    W, KT, elems, ns = K.group_wt_geometry(d["dil"], B, T, R, dt, seg)
    st = int(np.gcd.reduce(d["dil"]))
    row, ok = G.ct_rows(B, T, st, W)
    nseg = row.shape[0]
    assert nseg * KT * R * 32 == elems
    unowned = np.repeat(~D.tile_written(B, T, st, W).reshape(-1), R * 32)
    xT = torch.full((n, elems), G.CT_POISON, dtype=dt, device=DEV)
    cT = torch.full((n, elems), G.CT_POISON, dtype=dt, device=DEV)
    for l in range(n):
        xt = G.ct_encode(d["x"][l], B, T, R, st, W, 0.0)
        xt[unowned] = G.CT_POISON
        xT[l] = _dev(xt, dt)
        cT[l] = _dev(G.ct_encode(d["c"][l], B, T, R, st, W, G.CT_POISON), dt)
    z = _dev(d["z"], dt).view(n, B, T, R)
    dcs = None if d["dcs"] is None else _dev(d["dcs"], dt).view(n, B, T, R)
    gt = None if d["g_top"] is None else _dev(d["g_top"], dt).view(B, T, R)
    g_out = _nan((n + 1, B, T, R), dt)
    pdt = BF16 if part16 else F32
    pad = 64
    pf, prr = _nan((n * ns * 2 * R * R + pad,), pdt), _nan((n * ns * R * R + pad,), pdt)
    pbf, pbr = _nan((n * ns * R + pad,), F32), _nan((n * ns * R + pad,), F32)
    NH = 8 // (R // 16)
    ic = None
    if ic_shift is not None:
        icp = _nan((ns * NH * 3 * R + pad,), F32)
        ic = (_dev(d["audio"]), icp, ic_shift)
    K.residual_group_bwd_wt(gt, g_out, z, dcs, xT, cT, pc, pr, d["dil"], pf, prr, pbf, pbr, ns, W, 2, write_all_g=True, ic=ic)
    torch.cuda.synchronize()
    assert bool(torch.isnan(g_out[n]).all()), "a store behind the group's layers"
    for name, p in (("part_f", pf), ("part_r", prr), ("part_bf", pbf), ("part_br", pbr)):
        assert bool(torch.isnan(p[-pad:].float()).all()), name + ": a store behind the partial slabs"
        assert bool(torch.isfinite(p[:-pad].float()).all()), name + ": a partial left unwritten"
    out = dict(G=_host(g_out[:n]).reshape(n, B * T, R), ns=ns, nseg=nseg,
               dWf=_reduce(pf, ns, 2 * R * R, n, R if part16 else None).reshape(n, 2, R, R),
               dWr=_reduce(prr, ns, R * R, n, R if part16 else None).reshape(n, R, R),
               dbf=_reduce(pbf, ns, R, n), dbr=_reduce(pbr, ns, R, n))
    if ic is not None:
        assert bool(torch.isnan(icp[-pad:]).all())
        out["ic"] = _reduce(icp, ns * NH, 3 * R, 1).reshape(3, R)
    return out


def _hold_wt(what, d, o, mode, part16=False, ic_shift=None):
    """Layer-local, top first: G_g from the stored G_{g+1} through the RECONSTRUCTED df (an undecided df entry makes the G
    entries that read it undecided), and the four weight gradients contracted in float64 from the tiles' operands, the stored
    G_{g+1} and the reconstructed df."""
    n, rows = len(d["dil"]), d["B"] * d["T"]
    k16 = -(-o["nseg"] // o["ns"]) if part16 else 0          # segments a workgroup walks = roundings of its bf16 blocks
    stats = {}
    Gup = d["g_top"]
    for l in range(n - 1, -1, -1):
        rdf, udf, rG, extra, dec = D.wt_layer_refs(d, l, Gup, mode)
        got = o["G"][l]
        assert np.isfinite(got).all(), "%s: G of layer %d left unwritten" % (what, l)
        same = G.same_bits(got, rG["ref"])
        assert same[dec].all(), "%s: G of layer %d: %d of %d decided entries differ, first at %s" % (
            what, l, (dec & ~same).sum(), dec.sum(), np.argwhere(dec & ~same)[0].tolist())
        over = np.abs(got - rG["x"]) > D.bound(rG, mode, D.C_GPU["G"][mode]) + extra
        assert not over.any(), "%s: G of layer %d: %d entries beyond their bound" % (what, l, over.sum())
        stats["G decided"] = min(stats.get("G decided", 1.0), float(dec.mean()))
        for name, (val, S, ex) in D.wgrad_refs(d, l, Gup, rdf["ref"], udf).items():
            scale = D.wgrad_scale(S, rows, ex, k16 if name in ("dWf", "dWr") else 0)
            err = np.abs(o[name][l] - val)
            assert (err[scale == 0] == 0).all(), "%s: %s of layer %d where no term exists" % (what, name, l)
            r = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0)
            stats[name] = max(stats.get(name, 0.0), float(r.max()))
            assert r.max() <= D.C_GPU_WGRAD, "%s: %s of layer %d: error / scale %.3g > %g at %s" % (
                what, name, l, r.max(), D.C_GPU_WGRAD, np.unravel_index(r.argmax(), r.shape))
        Gup = got
    if ic_shift is not None:
        val, S = D.ic_refs(d, o["G"][0], ic_shift)
        r = np.abs(o["ic"] - val) / np.maximum(D.wgrad_scale(S, rows, 0.0), 1e-300)
        stats["ic"] = float(r.max())
        assert r.max() <= D.C_GPU_WGRAD, "%s: input conv gradient: error / scale %.3g" % (what, r.max())
    _say("%-76s %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(stats.items()))))


WT_RUNS = [(i, R, v) for (i, R, v) in D.RUNS if R == 64 or i in (1, 2)]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("i,R,variant", WT_RUNS)
def test_group_bwd_wt_entries(monkeypatch, dt, i, R, variant):
    """srwn_residual_group_bwd_wt with write_all_g and fp32 partial slabs (bf16 mode: bf16 partial blocks as well); where
    the launch has a skip path, the first group's input conv gradient rides along (shift 1, and shift 0 in the block run).
    Contract: G of every layer is written for every row of every clip; every partial slab of every layer is written (zeros
    where a layer has no gradient from above), nothing behind them."""
    monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    dil, B, T, seg = D.CASES[i]
    d = D.wt_design(dil, B, T, R, variant)
    mode = NAME[dt]
    what = "group_bwd_wt %s %s B %d T %d seg %d R %d %s" % (mode, dil, B, T, seg, R, variant)
    ics = 1 if d["dcs"] is not None else None
    _hold_wt(what, d, _run_bwd_wt(d, dt, seg, ic_shift=ics), mode, ic_shift=ics)
    if dt == BF16:
        ics = 0 if d["dcs"] is not None else None
        _hold_wt(what + " blocks", d, _run_bwd_wt(d, dt, seg, part16=True, ic_shift=ics), mode, part16=True, ic_shift=ics)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("i", D.GRID2)
def test_group_bwd_wt_entries_two_workgroups(monkeypatch, dt, i):
    """SRWN_GROUP_GRID = 2: every workgroup walks several segments and adds each one's sums to its partial slab (bf16
    blocks: read back, added in fp32, rounded again -- one rounding per segment, counted in the bound)."""
    dil, B, T, seg = D.CASES[i]
    d = D.wt_design(dil, B, T, 64, "both")
    mode = NAME[dt]
    what = "group_bwd_wt %s %s B %d T %d seg %d two workgroups" % (mode, dil, B, T, seg)
    monkeypatch.setenv("SRWN_GROUP_GRID", "2")
    try:
        o = _run_bwd_wt(d, dt, seg, ic_shift=1)
        assert o["ns"] == 2 and o["nseg"] > 4
        p = _run_bwd_wt(d, dt, seg, part16=True, ic_shift=1) if dt == BF16 else None
    finally:
        monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
    _hold_wt(what, d, o, mode, ic_shift=1)
    if p is not None:
        _hold_wt(what + " blocks", d, p, mode, part16=True, ic_shift=1)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("i,grid", [(i, None) for i in range(len(D.CASES))] + [(i, "2") for i in D.GRID2])
def test_group_bwd_wt_exact_corner(monkeypatch, dt, i, grid):
    """g_top = None, z = 0, Wr_top = 0: dWf_top, dbf_top, dWr and dbr of the layer below are sums of dyadic products in
    range and must equal the float64 reference rounded once -- tile indexing, ownership masks, tap shifts, ragged last
    tiles and the sums over a workgroup's segments with no tolerance at all; with bf16 partial blocks on a sparser design,
    wherever the entry's S stays within 256 units (every partial a block can hold is then exact in bf16; more than half
    of the entries)."""
    dil, B, T, seg = D.CASES[i]
    mode = NAME[dt]
    n = len(dil)
    for part16 in ([False, True] if dt == BF16 else [False]):
        d = D.wt_design(dil, B, T, 64, exact_corner=True, blocks=part16)
        dfx, tx, _ = D.exact_top(d)
        Gtop = D.round_to(tx, mode)
        top = D.wgrad_refs(d, n - 1, None, dfx, np.zeros_like(dfx))
        below = D.wgrad_refs(d, n - 2, Gtop, dfx, np.zeros_like(dfx))
        want = [("dWf", n - 1, top["dWf"], D.GX * 0.5 * D.GD), ("dbf", n - 1, top["dbf"], 0.5 * D.GD),
                ("dWr", n - 2, below["dWr"], D.GC * 0.5 * D.GD * G.GW), ("dbr", n - 2, below["dbr"], 0.5 * D.GD * G.GW)]
        if grid:
            monkeypatch.setenv("SRWN_GROUP_GRID", grid)
        else:
            monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
        try:
            o = _run_bwd_wt(d, dt, seg, part16=part16)
        finally:
            monkeypatch.delenv("SRWN_GROUP_GRID", raising=False)
        what = "group_bwd_wt exact corner %s %s B %d T %d seg %d blocks %d grid %s" % (mode, dil, B, T, seg, part16, grid)
        assert G.same_bits(o["G"][n - 1], Gtop).all(), what + ": G of the top layer"
        for name, l, (val, S, _), unit in want:
            ok = G.same_bits(o[name][l], G.round_out(val, "fp32"))
            held = (S / unit <= G.S_MAX16) if (part16 and name in ("dWf", "dWr")) else np.ones_like(ok)
            _say("%-80s %s: %d of %d entries held bit for bit" % (what, name, held.sum(), held.size))
            assert held.mean() >= 0.5, "%s: %s: the design leaves too few sums within 256 units" % (what, name)
            assert ok[held].all(), "%s: %s of layer %d: %d entries differ from the integer reference, first at %s" % (
                what, name, l, (held & ~ok).sum(), np.argwhere(held & ~ok)[0].tolist())
        _hold_wt(what, d, o, mode, part16=part16)
