"""GPU tests of ``srwn_adam_step_ctl`` (srwn_version() 126) on its own: the Adam half against its twin ``srwn_adam_step`` /
``srwn_adam_step_scaled`` handed ``lr = table[row]`` from the host, bit for bit at every step; which row a step reads; the
EMA half against the NumPy float32 restatement (tests/opt_reference.py) applied to the kernel's own parameters, every entry
bit for bit; nothing written past ``n``; the step word.

Shapes: n in {1, 3, 1023, 1024, 1025, 2 * 262144 + 7} -- below one vector, around one block of 256 threads x 4, more than
two grid-stride rounds of 256 blocks -- with 16-byte aligned buffers (the vector path and its tail) and with every buffer
offset by one float (the scalar path).  Inputs: theta and e in +-[0.1, 2], g in +-[1e-3, 1], decays in {0, 0.5, 0.9999},
lr >= 1e-4 or exactly 0: no intermediate of the EMA rule is subnormal (asserted in the restatement)."""
import itertools

import numpy as np
import pytest
import torch

from tests._pkg import sub
from tests.opt_reference import bits, ctl_row, ema_reference

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 1023, 1024, 1025, 2 * 262144 + 7]
PAD, POISON = 64, 3.0e33
B1, B2, EPS = 0.9, 0.999, 1e-8
TABLE5 = np.array([[1e-2, 0.0], [3e-3, 0.5], [1e-3, 0.9999], [2e-4, 0.5], [1e-4, 0.0]], np.float32)


def _signed(rng, lo, hi, n):
    return (rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


class Bufs:
    """theta, g, m, v, e as views [off : off + n] of buffers n + PAD + off floats long, filled with a poison value."""

    def __init__(self, n, off, seed):
        self.n, self.off = n, off
        rng = np.random.default_rng(seed)
        self.rng = np.random.default_rng(seed + 1)
        self.raw = {k: torch.full((n + PAD + off,), POISON, dtype=torch.float32, device="cuda") for k in "tgmve"}
        self.t, self.g, self.m, self.v, self.e = (self.raw[k][off:off + n] for k in "tgmve")
        assert all(x.data_ptr() % 16 == (4 * off) % 16 for x in (self.t, self.g, self.m, self.v, self.e))
        self.t.copy_(torch.from_numpy(_signed(rng, 0.1, 2.0, n)))
        self.e.copy_(torch.from_numpy(_signed(rng, 0.1, 2.0, n)))
        self.m.zero_(); self.v.zero_()
        self.step = torch.zeros(1, dtype=torch.int64, device="cuda")

    def next_grad(self):
        self.g.copy_(torch.from_numpy(_signed(self.rng, 1e-3, 1.0, self.n)))

    def get(self, k):
        return getattr(self, k).cpu().numpy()

    def check_isolation(self, t_expected):
        for k, raw in self.raw.items():
            h = raw.cpu().numpy()
            assert (h[:self.off] == np.float32(POISON)).all() and (h[self.off + self.n:] == np.float32(POISON)).all(), k
        w = self.step.view(torch.int32).cpu().numpy()
        assert w[1] == 0, "the arrival counter is not back to zero"
        assert w[0] == t_expected and int(self.step.item()) == t_expected


def _dev_table(table, capacity=None):
    table = np.asarray(table, np.float32).reshape(-1, 2)
    cap = capacity or len(table)
    ctl = torch.zeros((cap, 2), dtype=torch.float32, device="cuda")
    ctl[:len(table)].copy_(torch.from_numpy(table))
    return ctl, torch.full((1,), len(table), dtype=torch.int32, device="cuda")


def _twin_step(K, b, lr, scale_dev, grad_scale, tick):
    """The same update from entry points older than srwn_adam_step_ctl, lr from the host."""
    if scale_dev is None and tick:
        K.adam_step(b.t, b.g, b.m, b.v, b.step, lr, B1, B2, EPS, grad_scale=grad_scale)
    else:           # (1.0f * x is x: a scale tensor holding grad_scale stands for the host scalar)
        sd = scale_dev if scale_dev is not None else torch.full((1,), grad_scale, dtype=torch.float32, device="cuda")
        K.adam_step_scaled(b.t, b.g, b.m, b.v, b.step, lr, sd, tick, B1, B2, EPS)


def _run_pair(n, off, table, steps, with_ema, with_scale, tick, seed=0, H=None, capacity=None, on_step=None):
    """`steps` steps of srwn_adam_step_ctl on one set of buffers and of its twin on another, compared at every step."""
    K = sub("kernels")
    table = np.asarray(table, np.float32).reshape(-1, 2)
    a, b = Bufs(n, off, seed), Bufs(n, off, seed)
    ctl, ctl_len = _dev_table(table, capacity)
    if H is not None:
        ctl_len.fill_(H)
    scale_dev = torch.tensor([0.37, 123.0], dtype=torch.float32, device="cuda") if with_scale else None
    grad_scale = 1.0 if with_scale else 0.5
    for k in range(1, steps + 1):
        if on_step is not None:
            table = on_step(k, ctl, ctl_len, table)
        a.next_grad(); b.next_grad()
        if not tick:      # another buffer of the same optimizer has ticked the shared counter
            a.step.fill_(k); b.step.fill_(k)
        e_before = a.get("e")
        K.adam_step_ctl(a.t, a.g, a.m, a.v, a.step, ctl, ctl_len, ema=a.e if with_ema else None, scale_dev=scale_dev,
                        tick=tick, grad_scale=grad_scale, beta1=B1, beta2=B2, eps=EPS)
        rows = min(int(ctl_len.item()), ctl.shape[0])
        row = ctl_row(k, rows)
        lr, d = float(table[row, 0]), table[row, 1]
        _twin_step(K, b, lr, scale_dev, grad_scale, tick)
        torch.cuda.synchronize()
        for name in "tmv":
            assert np.array_equal(bits(a.get(name)), bits(b.get(name))), (name, "step", k, "row", row)
        assert torch.equal(a.step, b.step)
        if with_ema:
            assert np.array_equal(bits(a.get("e")), bits(ema_reference(e_before, a.get("t"), d))), ("ema", "step", k)
        else:
            assert np.array_equal(bits(a.get("e")), bits(e_before))
        a.check_isolation(k); b.check_isolation(k)
    return a, b


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_five_steps_equal_the_twin_and_the_restatement(n, off):
    """Every combination of the shadow given or not, the clip factor given or not, tick 1 and 0: theta, m, v and the step
    word equal the twin's at every step -- so they do not depend on the shadow --, e' equals the restatement on the
    kernel's own theta', and nothing past n is written."""
    for with_ema, with_scale, tick in itertools.product([False, True], [False, True], [True, False]):
        _run_pair(n, off, TABLE5, 5, with_ema, with_scale, tick, seed=n)


def test_theta_m_v_do_not_depend_on_the_shadow():
    K = sub("kernels")
    n = 1025
    a, b = Bufs(n, 0, 4), Bufs(n, 0, 4)
    ctl, ctl_len = _dev_table(TABLE5)
    for k in range(5):
        a.next_grad(); b.next_grad()
        K.adam_step_ctl(a.t, a.g, a.m, a.v, a.step, ctl, ctl_len, ema=a.e)
        K.adam_step_ctl(b.t, b.g, b.m, b.v, b.step, ctl, ctl_len, ema=None)
        for name in "tmv":
            assert np.array_equal(bits(a.get(name)), bits(b.get(name))), (name, k)
    assert not np.array_equal(bits(a.get("e")), bits(b.get("e")))


def test_a_row_of_zero_lr_leaves_theta_alone():
    """Table lr = [1e-2, 0, 1e-3, 0]: steps 2 and 4 leave theta bit-unchanged while m and v move; steps 1 and 3 move it.  A
    launch reading the row before or behind its own fails this."""
    K = sub("kernels")
    n = 1025
    a = Bufs(n, 0, 9)
    ctl, ctl_len = _dev_table([[1e-2, 0.5], [0.0, 0.5], [1e-3, 0.5], [0.0, 0.5]])
    for k in range(1, 5):
        a.next_grad()
        t0, m0, v0 = a.get("t"), a.get("m"), a.get("v")
        K.adam_step_ctl(a.t, a.g, a.m, a.v, a.step, ctl, ctl_len, ema=a.e)
        same = np.array_equal(bits(a.get("t")), bits(t0))
        assert same == (k in (2, 4)), k
        # (an entry whose moment keeps its bits needs g within an ulp of it: none, or a stray one, among 1025)
        assert (a.get("m") != m0).mean() > 0.99 and (a.get("v") != v0).mean() > 0.99, k
        a.check_isolation(k)


@pytest.mark.parametrize("off", [0, 1])
def test_steps_beyond_the_table_keep_its_last_row(off):
    """H = 3: steps 4..6 run at table[2], the EMA decay included (``_run_pair`` picks the twin's row by the same rule)."""
    _run_pair(1025, off, TABLE5[:3], 6, True, False, True)


def test_one_row_is_a_constant():
    _run_pair(1023, 0, [[2e-3, 0.9999]], 4, True, True, True)


def test_the_length_is_held_inside_the_allocated_rows():
    """A length word above the capacity (or below 1) never reads past the table: the row stays inside [0, capacity)."""
    _run_pair(1024, 0, TABLE5[:2], 4, True, False, True, H=100)
    _run_pair(1024, 0, TABLE5[:2], 2, True, False, True, H=0)


def test_a_table_rewritten_in_place_steers_the_next_launch():
    """Two steps on {A0, A1} (H = 2) in a table allocated for four rows; then the rows and the length are rewritten in
    place (H = 3, other values): step 3 reads the new row 2, steps 4 and 5 keep it."""
    new = np.array([[7e-3, 0.5], [6e-3, 0.0], [5e-4, 0.9999]], np.float32)

    def on_step(k, ctl, ctl_len, table):
        if k == 3:
            ctl[:3].copy_(torch.from_numpy(new))
            ctl_len.fill_(3)
            return new
        return table
    _run_pair(1025, 0, TABLE5[:2], 5, True, True, True, capacity=4, on_step=on_step)


def test_decay_zero_follows_theta_up_to_rounding():
    """d = 0: s = 1, p = diff, e' = e - round(e - theta').  Two roundings, each at most half an ulp of its result
    (2^-24 relative): |e' - theta'| <= 2^-24 (|diff| + |e'|) (1 + 2^-23).  The restatement gives e' itself."""
    K = sub("kernels")
    n = 1025
    a = Bufs(n, 0, 21)
    ctl, ctl_len = _dev_table([[1e-3, 0.0]])
    a.next_grad()
    e0 = a.get("e")
    K.adam_step_ctl(a.t, a.g, a.m, a.v, a.step, ctl, ctl_len, ema=a.e)
    t1, e1 = a.get("t"), a.get("e")
    assert np.array_equal(bits(e1), bits(ema_reference(e0, t1, 0.0)))
    diff = (e0 - t1).astype(np.float64)
    bound = 2.0 ** -24 * (np.abs(diff) + np.abs(e1.astype(np.float64))) * (1 + 2.0 ** -23)
    assert (np.abs(e1.astype(np.float64) - t1.astype(np.float64)) <= bound).all()


def test_wrapper_refuses_bad_tables():
    K = sub("kernels")
    a = Bufs(8, 0, 1)
    ctl, ctl_len = _dev_table(TABLE5)
    with pytest.raises(ValueError):
        K.adam_step_ctl(a.t, a.g, a.m, a.v, a.step, ctl.reshape(-1), ctl_len)
    with pytest.raises(TypeError):
        K.adam_step_ctl(a.t, a.g, a.m, a.v, a.step, ctl, ctl_len.to(torch.int64))
    with pytest.raises(ValueError):
        K.adam_step_ctl(a.t, a.g, a.m, a.v, a.step, ctl, ctl_len, ema=a.e[:4])
    a.check_isolation(0)
