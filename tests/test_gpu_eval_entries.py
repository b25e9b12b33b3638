"""GPU tests of ``srwn_eval_classes`` alone (csrc/srwn_eval.hip) on hand-made posteriors, against ``eval_reference``:
``pred``, ``rank``, ``confusion`` and ``seen`` bit for bit in every entry, ``nll`` within 1 fp32 ulp; poisoned outputs show
that invalid rows, records not owned and other slots are never written; three sweeps through two slots show the wrap, the
zeroing of a reused slot and the state; eager launches and a replayed graph agree in every bit.

The nll margin is derived, not measured: the device's double ``log`` is accurate to 1 ulp of a double, so after the single
rounding to fp32 the kernel and the float64 reference can differ only where the exact value lies that close to a rounding
midpoint -- at most one fp32 ulp; where p is 0 or 1 the logarithm is exact and the two are equal."""
import numpy as np
import pytest
import torch

from tests._pkg import sub
from tests.eval_reference import eval_reference, ulp_distance

pytestmark = pytest.mark.gpu

POISON_I = np.int32(-0x21524111)          # 0xDEADBEEF
POISON_F = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]      # a NaN with a payload
SEED = 5


def _probs(rows, C, rng):
    """Posteriors on a coarse grid -- ties everywhere -- with exact zeros, exact ones and rows of all-equal values."""
    q = rng.integers(0, 4, (rows, C)).astype(np.float32) / np.float32(8.0)
    for m in range(rows):
        kind = m % 5
        if kind == 1:
            q[m] = 0.0
            q[m, rng.integers(0, C)] = 1.0                    # a one-hot row: p = 1 at one class, 0 elsewhere
        elif kind == 2:
            q[m] = np.float32(1.0 / C)                        # every class tied
        elif kind == 3:
            q[m] = rng.random(C).astype(np.float32)           # no ties: general fp32 values for the logarithm
    return np.ascontiguousarray(q)


class _Slots(object):
    """The device arrays of an evaluation with `cap` slots over `N` records of `C` classes, poisoned."""

    def __init__(self, N, C, cap, labels):
        dev = "cuda"
        self.N, self.C, self.cap = N, C, cap
        self.labels = torch.as_tensor(np.asarray(labels, np.int32)).to(dev)
        self.state = torch.tensor([SEED, 0, 0], dtype=torch.int64, device=dev)
        self.pred = torch.full((cap, N), int(POISON_I), dtype=torch.int32, device=dev)
        self.rank = torch.full((cap, N), int(POISON_I), dtype=torch.int32, device=dev)
        self.nll = torch.as_tensor(np.full((cap, N), POISON_F, np.float32)).to(dev)
        self.conf = torch.full((cap, C, C), int(POISON_I), dtype=torch.int32, device=dev)
        self.seen = torch.full((cap,), int(POISON_I), dtype=torch.int32, device=dev)

    def launch(self, probs, indices, B, rank=0, world=1):
        K = sub("kernels")
        K.call("srwn_eval_classes", probs.data_ptr(), indices.data_ptr(), self.labels.data_ptr(), self.state.data_ptr(),
               self.N, B, self.C, rank, world, self.cap, self.pred.data_ptr(), self.rank.data_ptr(), self.nll.data_ptr(),
               self.conf.data_ptr(), self.seen.data_ptr(), K._stream())

    def host(self):
        return dict(pred=self.pred.cpu().numpy(), rank=self.rank.cpu().numpy(),
                    nll=self.nll.cpu().numpy(), conf=self.conf.cpu().numpy(), seen=self.seen.cpu().numpy(),
                    state=self.state.cpu().tolist())


def _expect_sweep(want, slot, probs_of_step, labels, N, B, C, rank, world):
    """One sweep of the reference into slot `slot` of the host arrays `want`: the confusion and seen of the slot start
    over, the valid rows of every step land at their records, nothing else is touched."""
    D = sub("dataset")
    want["conf"][slot] = 0
    want["seen"][slot] = 0
    for s, probs in enumerate(probs_of_step):
        idx, valid = D.sweep_plan(s, B, N, rank, world)
        if not valid.any():
            continue
        rec = idx[valid]
        pred, rk, nll, conf = eval_reference(probs[valid], labels[rec])
        want["pred"][slot, rec], want["rank"][slot, rec], want["nll"][slot, rec] = pred, rk, nll
        want["conf"][slot] += conf
        want["seen"][slot] += int(valid.sum())


def _check(got, want, where):
    for k in ("pred", "rank", "conf", "seen"):
        assert np.array_equal(got[k], want[k]), (where, k)            # every entry, poison included
    g, w = got["nll"], want["nll"]
    poison = w.view(np.uint32) == POISON_F.view(np.uint32)
    assert np.array_equal(g.view(np.uint32)[poison], w.view(np.uint32)[poison]), (where, "nll poison")
    d = ulp_distance(g[~poison], w[~poison])
    print(where, "nll: max ulp distance", int(d.max()) if d.size else 0, "over", d.size)
    assert (d <= 1).all(), (where, "nll")
    exact = ~poison & (np.isinf(w) | (w == 0))                        # p = 0 and p = 1
    assert np.array_equal(g[exact], w[exact]), (where, "nll at p = 0 or 1")


def _sweeps(N, B, C, rank, world, cap, nsweeps, graph):
    """Drives `nsweeps` sweeps through `cap` slots and checks every bit of every array after each."""
    D = sub("dataset")
    rng = np.random.default_rng(1000 * C + 10 * B + N)
    labels = rng.integers(0, C, N).astype(np.int64)
    slots = _Slots(N, C, cap, labels)
    steps = D.sweep_steps(N, B, world)
    probs_d = torch.zeros((B, C), dtype=torch.float32, device="cuda")
    idx_d = torch.zeros(B, dtype=torch.int32, device="cuda")
    want = slots.host()
    g = None
    if graph:                                     # (capturing launches nothing: the state does not tick)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            slots.launch(probs_d, idx_d, B, rank, world)
    for sweep in range(nsweeps):
        probs_of_step = [_probs(B, C, rng) for _ in range(steps)]
        for s in range(steps):
            idx, _ = D.sweep_plan(s, B, N, rank, world)
            probs_d.copy_(torch.as_tensor(probs_of_step[s]))
            idx_d.copy_(torch.as_tensor(idx))
            if g is not None:
                g.replay()
            else:
                slots.launch(probs_d, idx_d, B, rank, world)
        _expect_sweep(want, sweep % cap, probs_of_step, labels, N, B, C, rank, world)
        want["state"] = [SEED, 0, sweep + 1]
        got = slots.host()
        assert got["state"] == want["state"]
        _check(got, want, "N=%d B=%d C=%d sweep %d" % (N, B, C, sweep))
    return slots.host()


@pytest.mark.parametrize("C", [1, 5, 100, 256])
@pytest.mark.parametrize("N,B", [(1, 1), (1, 4), (1, 70), (11, 1), (11, 4), (11, 70), (150, 1), (150, 4),
                                 (150, 70)])
def test_eval_classes_against_the_reference(N, B, C):
    """A ragged last step (11 = 2 * 4 + 3, 150 = 2 * 70 + 10), B > N (70 rows on 11 records, 4 on 1), one class, a class
    count that is no multiple of four and the full 256.  Two slots, one sweep: slot 1 keeps every poisoned bit."""
    got = _sweeps(N, B, C, 0, 1, 2, 1, graph=False)
    assert (got["pred"][1] == POISON_I).all() and (got["conf"][1] == POISON_I).all() and got["seen"][1] == POISON_I
    assert got["seen"][0] == N and got["conf"][0].sum() == N


def test_one_rank_of_two_writes_its_share_only():
    """Rank 1 of world 2, N = 11, B = 4: positions 4..7 in step 0, 12..15 (none valid) in step 1.  Records 0..3 and 8..10
    belong to rank 0 and keep their poison."""
    got = _sweeps(11, 4, 5, 1, 2, 2, 1, graph=False)
    own = np.zeros(11, bool)
    own[4:8] = True
    assert (got["pred"][0][~own] == POISON_I).all() and (got["rank"][0][~own] == POISON_I).all()
    assert (got["pred"][0][own] != POISON_I).all()
    assert got["seen"][0] == 4


@pytest.mark.parametrize("graph", [False, True])
def test_three_sweeps_through_two_slots(graph):
    """The slot index wraps (sweeps 0, 1, 2 -> slots 0, 1, 0); the reused slot's confusion is cleared at its step 0 and
    holds the third sweep only; the state reads {seed, 0, 3}.  Eager launches and a replayed graph: the same bits."""
    got = _sweeps(11, 4, 5, 0, 1, 2, 3, graph=graph)
    assert got["state"] == [SEED, 0, 3]
    assert got["conf"][0].sum() == 11 and got["conf"][1].sum() == 11 and got["seen"].tolist() == [11, 11]
    if graph:
        eager = _sweeps(11, 4, 5, 0, 1, 2, 3, graph=False)            # (the same seeds: the same posteriors)
        for k in ("pred", "rank", "conf", "seen"):
            assert np.array_equal(got[k], eager[k]), k
        assert np.array_equal(got["nll"].view(np.uint32), eager["nll"].view(np.uint32))
