"""GPU tests of ``srwn_embed_collect`` and ``srwn_pair_sweep`` (csrc/srwn_pair_eval.hip) alone, on planted embeddings.

For every shape and design: the stored matrix equals ``srwn_gallery_match`` of the same rows bit for bit (N <= 1024), is
symmetric bit for bit and lies within a per-entry bound of float64 that is derived from the operation count
(tests/pair_eval_reference.py: no GPU figure enters it, no entry is left out); every counted output equals
``pair_reference`` applied to the stored matrix, bit for bit; the histograms sum to N (N - 1) / 2; a NULL ``dist`` and a
second launch into the same slot give the same outputs; poisoned neighbouring slots and the elements behind the last slot
keep their bits.  The collect launch writes nothing for tail rows and ticks by ``sweep_plan``.

Designs: normal embeddings; an integer lattice in [-2, 2] (many exactly equal distances and exact duplicates: every tie
rule decides in every launch); normal embeddings with a d_max at their median distance (half the pairs beyond the last
bin)."""
import numpy as np
import pytest
import torch

from tests._pkg import sub
from tests.pair_eval_reference import distance_matrix_fp64, pair_reference

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 1), (2, 1, 2), (3, 2, 3), (5, 3, 2), (65, 2, 4), (257, 5, 7), (130, 65, 5), (300, 64, 3), (70, 256, 2),
          (1030, 2, 30), (67, 12, 3)]          # (the last one: the tree of 16 leaves)
CAP, SLOT, PAD, BINS = 3, 1, 7, 37
POISON_I, POISON_F = -77, -123.5
NAMES_I, NAMES_F, NAMES_H = ("nearest", "same_nearest", "rank_same"), ("nearest_dist", "same_dist"), ("hist_same", "hist_diff")


def _design(kind, n, dim, classes):
    rng = np.random.default_rng(1000 * n + dim)
    labels = rng.integers(0, classes, n).astype(np.int32)
    if classes == n:
        labels = np.arange(n, dtype=np.int32)                   # every class single
    if kind == "lattice":
        emb = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    else:
        emb = rng.standard_normal((n, dim)).astype(np.float32)
    d64, _ = distance_matrix_fp64(emb)
    off = d64[np.triu_indices(n, 1)]
    if kind == "overflow" and off.size:
        d_max = float(np.median(off))
    else:
        d_max = float(1.25 * off.max()) if off.size else 1.0
    return emb, labels, max(d_max, 1e-3)


class _Buffers(object):
    """Result slots as flat poisoned buffers with PAD elements behind the last slot, and the planted embeddings."""

    def __init__(self, emb, labels):
        n, dim = emb.shape
        dev = "cuda"
        self.n, self.dim = n, dim
        slots = np.full(CAP * n * dim + PAD, POISON_F, np.float32)
        slots[SLOT * n * dim:(SLOT + 1) * n * dim] = emb.reshape(-1)
        self.slots = torch.as_tensor(slots, device=dev)
        self.labels = torch.as_tensor(labels, device=dev)
        self.state = torch.tensor([5, 0, SLOT + 1 + 2 * CAP], dtype=torch.int64, device=dev)      # sweeps completed: slot SLOT
        self.out = {}
        for k in NAMES_I:
            self.out[k] = torch.full((CAP * n + PAD,), POISON_I, dtype=torch.int32, device=dev)
        for k in NAMES_F:
            self.out[k] = torch.full((CAP * n + PAD,), POISON_F, dtype=torch.float32, device=dev)
        for k in NAMES_H:
            self.out[k] = torch.full((CAP * BINS + PAD,), POISON_I, dtype=torch.int64, device=dev)
        self.dist = torch.full((n * n + PAD,), POISON_F, dtype=torch.float32, device=dev)

    def launch(self, scale, with_dist=True):
        K = sub("kernels")
        o = self.out
        K.call("srwn_pair_sweep", self.slots.data_ptr(), self.labels.data_ptr(), self.state.data_ptr(), self.n, self.dim, CAP,
               BINS, float(scale), o["nearest"].data_ptr(), o["same_nearest"].data_ptr(), o["rank_same"].data_ptr(),
               o["nearest_dist"].data_ptr(), o["same_dist"].data_ptr(), o["hist_same"].data_ptr(), o["hist_diff"].data_ptr(),
               self.dist.data_ptr() if with_dist else None, K._stream())
        torch.cuda.synchronize()

    def host(self):
        """The slot's outputs, after checking that nothing else was written."""
        got = {}
        for k, t in self.out.items():
            a = t.cpu().numpy()
            per = BINS if k in NAMES_H else self.n
            poison = POISON_F if k in NAMES_F else POISON_I
            keep = np.ones(a.shape, bool)
            keep[SLOT * per:(SLOT + 1) * per] = False
            assert (a[keep] == poison).all(), "%s: written outside slot %d" % (k, SLOT)
            got[k] = a[SLOT * per:(SLOT + 1) * per].copy()
        return got

    def matrix(self):
        a = self.dist.cpu().numpy()
        assert (a[self.n * self.n:] == POISON_F).all()
        return a[:self.n * self.n].reshape(self.n, self.n).copy()


def _gallery(emb):
    """``srwn_gallery_match`` of every row against all rows: dist [N, N]."""
    K = sub("kernels")
    n, dim = emb.shape
    e = torch.as_tensor(emb, device="cuda")
    ng = torch.tensor([n], dtype=torch.int32, device="cuda")
    dist = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    near = torch.zeros(n, dtype=torch.int32, device="cuda")
    dmin = torch.zeros(n, dtype=torch.float32, device="cuda")
    K.call("srwn_gallery_match", e.data_ptr(), n, dim, e.data_ptr(), ng.data_ptr(), n, dist.data_ptr(), near.data_ptr(),
           dmin.data_ptr(), K._stream())
    return dist.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    return a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("kind", ["normal", "lattice", "overflow"])
@pytest.mark.parametrize("n,dim,classes", SHAPES)
def test_pair_sweep(n, dim, classes, kind):
    emb, labels, d_max = _design(kind, n, dim, classes)
    scale = np.float32(BINS / d_max)
    buf = _Buffers(emb, labels)
    buf.launch(scale)
    got, dist = buf.host(), buf.matrix()
    # the matrix: the gallery's bits, symmetric, within the derived bound of float64 -- every entry
    if n <= 1024 and dim <= 256:
        assert _same_bits(dist, _gallery(emb)), "dist differs from srwn_gallery_match"
    assert _same_bits(dist, dist.T.copy()), "dist is not symmetric"
    d64, bound = distance_matrix_fp64(emb)
    err = np.abs(dist.astype(np.float64) - d64)
    print("N=%d D=%d %s: max |dist - fp64| / bound = %.3f" % (n, dim, kind, float((err / bound).max())))
    assert (err <= bound).all()
    # everything counted: the rules applied to the stored matrix
    want = dict(zip(("nearest", "nearest_dist", "same_nearest", "same_dist", "rank_same", "hist_same", "hist_diff"),
                    pair_reference(dist, labels, BINS, scale)))
    for k in want:
        assert _same_bits(got[k], want[k]), k
    pairs = n * (n - 1) // 2
    assert int(got["hist_same"].sum() + got["hist_diff"].sum()) == pairs
    if kind == "lattice" and n >= 65:                                # the design does what it is there for
        off = dist[np.triu_indices(n, 1)]
        assert np.unique(off).size < off.size // 4, "the lattice gives equal distances"
        if dim <= 3:
            assert (off == dist[0, 0]).any(), "the lattice gives exact duplicates"
    if kind == "overflow" and pairs >= 10:
        last = int(got["hist_same"][-1] + got["hist_diff"][-1])
        assert pairs // 4 <= last <= pairs - pairs // 4, "the d_max of this design leaves a share of the pairs beyond it"
    # a second launch into the same slot counts afresh; a NULL dist gives the same counted outputs
    buf.launch(scale)
    again = buf.host()
    for k in want:
        assert _same_bits(again[k], got[k]), "second launch: " + k
    assert _same_bits(buf.matrix(), dist)
    buf.dist.fill_(POISON_F)
    buf.launch(scale, with_dist=False)
    nodist = buf.host()
    for k in want:
        assert _same_bits(nodist[k], got[k]), "NULL dist: " + k
    assert (buf.dist.cpu().numpy() == POISON_F).all()


def test_pair_sweep_before_the_first_sweep_writes_nothing():
    emb, labels, d_max = _design("normal", 5, 3, 2)
    buf = _Buffers(emb, labels)
    buf.state[2] = 0
    buf.launch(np.float32(BINS / d_max))
    for k, t in buf.out.items():
        assert (t.cpu().numpy() == (POISON_F if k in NAMES_F else POISON_I)).all(), k
    assert (buf.dist.cpu().numpy() == POISON_F).all()


def test_pair_sweep_takes_the_slot_from_the_device_state():
    """The same arguments, another sweep count: the launch moves to that sweep's slot."""
    emb, labels, d_max = _design("normal", 9, 2, 3)
    scale = np.float32(BINS / d_max)
    buf = _Buffers(emb, labels)
    buf.launch(scale)
    got = buf.host()
    n = 9
    buf.slots[2 * n * 2:3 * n * 2] = buf.slots[SLOT * n * 2:(SLOT + 1) * n * 2]
    buf.state[2] = 3                                              # sweep 2 is the last one completed: slot 2
    buf.launch(scale)
    for k, t in buf.out.items():
        per = BINS if k in NAMES_H else n
        a = t.cpu().numpy()
        assert _same_bits(a[2 * per:3 * per], got[k]), k
        assert _same_bits(a[SLOT * per:(SLOT + 1) * per], got[k]), k          # (slot 1 keeps what it held)
        assert (a[:per] == (POISON_F if k in NAMES_F else POISON_I)).all(), k


@pytest.mark.parametrize("n,B,dim", [(11, 4, 3), (11, 16, 2), (12, 4, 5), (1, 3, 1), (300, 7, 64)])
def test_embed_collect(n, B, dim):
    D, K = sub("dataset"), sub("kernels")
    rng = np.random.default_rng(n * 100 + B)
    steps = D.sweep_steps(n, B)
    slots = torch.full((CAP * n * dim + PAD,), POISON_F, dtype=torch.float32, device="cuda")
    seen = torch.full((CAP + 1,), POISON_I, dtype=torch.int32, device="cuda")
    state = torch.tensor([9, 0, 4], dtype=torch.int64, device="cuda")          # sweep 4 lands in slot 1
    want = np.full((CAP, n, dim), POISON_F, np.float32)
    total = 0
    for sweep in (4, 5):
        slot = sweep % CAP
        for s in range(steps):
            idx, valid = D.sweep_plan(s, B, n)
            rows = rng.standard_normal((B, dim)).astype(np.float32)
            emb, indices = torch.as_tensor(rows, device="cuda"), torch.as_tensor(idx, device="cuda")
            assert state.cpu().tolist() == [9, s, sweep]
            K.call("srwn_embed_collect", emb.data_ptr(), indices.data_ptr(), state.data_ptr(), n, B, dim, 0, 1, CAP,
                   slots.data_ptr(), seen.data_ptr(), K._stream())
            torch.cuda.synchronize()
            want[slot][idx[valid]] = rows[valid]
            total = int(valid.sum()) if s == 0 else total + int(valid.sum())
            got = slots.cpu().numpy()
            assert _same_bits(got[:CAP * n * dim].reshape(CAP, n, dim), want), "sweep %d step %d" % (sweep, s)
            assert (got[CAP * n * dim:] == POISON_F).all()
            assert int(seen[slot].item()) == total
        assert total == n and state.cpu().tolist() == [9, 0, sweep + 1]
    sn = seen.cpu().numpy()
    assert sn[0] == POISON_I and sn[CAP] == POISON_I and sn[1] == n and sn[2] == n
    assert (want[0] == POISON_F).all()                               # slot 0 was never the device's sweep
