"""CPU proofs of the designs of tests/gen_design.py (no GPU): the conditions that make design A exact -- the grid of f,
the tanh margins, the gate constants, the exact sums, coverage -- and that the float32 NumPy restatement of a step has the
reference's bits on A and stays below C_CPU on B.  SRWN_PRINT_ERR=1 pytest -s prints the measured figures."""
import os

import numpy as np
import pytest

from tests import gemm_design as G
from tests import gen_design as N
from tests import group_design as D

PRINT = bool(os.environ.get("SRWN_PRINT_ERR"))


def test_tanh_is_decided_on_the_grid():
    z64, z32, err, margin, at = N.tanh_grid()
    if PRINT:
        print("MEASURED tanh grid: restatement error %.3e, smallest midpoint distance %.3e at f = %+.2f" % (err, margin, at))
    assert np.array_equal(z64, z32)
    assert err <= 1.0e-7 and margin >= 100 * err and margin >= 2.0e-4
    assert len(N.GRID_F) == 25 and G.is_bf16(z64)


def test_gate_is_25_constants():
    z = N.tanh_grid()[0]
    c = G.gate_poly32(z)
    assert G.is_bf16(c) and len(c) == 25
    # the constants are the gate of z up to the polynomial's error and their own rounding, and multiples of 2^-11
    assert (np.abs(c - G.gate64(z)) <= G.POLY_ERR + 0.5 * D.ulp_of(c, "bf16") + 1e-12).all()
    assert np.array_equal(c * 2 ** 11, np.rint(c * 2 ** 11))
    assert c[12] == 0.0 and (c[N.GRID_F != 0] != 0).all()


def test_fma32_is_one_rounding():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(20000).astype(np.float32)
    c = (rng.integers(-3, 4, 20000) * 0.25).astype(np.float32)
    got = N.fma32(a, N.K32, c)
    from fractions import Fraction
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(N.K32)) + Fraction(float(c[i]))
        lo = np.float32(float(exact))
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))
        assert got[i] == float(best)


def _grids(d):
    for k, g in (("wr", 1 / 8), ("ws", 1 / 8), ("w1", 1 / 8), ("w2", 1 / 8), ("wf", 1 / 8), ("bf", 1 / 16), ("br", 1 / 32),
                 ("bs", 1 / 8), ("b1", 1 / 8), ("b2", 1 / 8), ("init_w", 0.5), ("init_b", 1 / 8)):
        v = d[k]
        assert G.is_bf16(v) and np.array_equal(v / g, np.rint(v / g)), k
    for l in range(d["L"]):
        for w in (d["wr"][l], d["ws"][l], d["wf"][l, 0]) + ((d["wf"][l, 1],) if d["wf"][l, 1].any() else ()):
            assert np.abs(w).sum(0).min() > 0 and np.abs(w).sum(1).min() > 0      # every row (k) and column covered
    for w in (d["w1"], d["w2"]):
        assert np.abs(w).sum(0).min() > 0 and np.abs(w).sum(1).min() > 0


@pytest.mark.parametrize("case", N.CASES_A, ids=lambda c: "-".join(str(v) for v in c))
def test_design_a_is_exact(case):
    d = N.design_a(*case)
    _grids(d)
    assert np.isin(np.abs(d["wf"][d["wf"] != 0]), [0.25]).all() and not d["wf"][1:, 1].any()
    dil, B = d["dil"], d["B"]
    frames = N.frames_of(1001)
    cb_all = N.cond_table(d, N.encoding(d, frames)) if d["cond"] else None
    if cb_all is not None:
        assert G.is_bf16(cb_all) and np.array_equal(cb_all[0], np.rint(cb_all[0])) and np.abs(cb_all[0]).max() <= 1
        assert np.array_equal(cb_all * 4, np.rint(cb_all * 4))
    ndiff = nent = same = cross = 0
    winners = set()
    seen, live = np.zeros(d["C"], bool), 0.0
    for t in N.steps_a(dil):
        carry, forced = N.samples_a(d, t, 1)
        cb = None if cb_all is None else cb_all[:, :, min(t // N.POOL, frames - 1)]
        for pad in (False, True):
            ring = N.plant(d, t, pad)
            assert all(np.abs(v).max() <= 4 and np.array_equal(v, np.rint(v)) for v in ring)
            ref = N.step_a(d, ring, t, carry[:, 0], carry[:, 1], cb, tap_from_ring=pad)
            r32 = N.step_a(d, ring, t, carry[:, 0], carry[:, 1], cb, tap_from_ring=pad, arith="f32")
            assert G.same_bits(r32["logits"], ref["logits"]).all()
            for l in range(d["L"]):
                assert len(ref["x"][l]) == len(r32["x"][l])
                for a, b in zip(ref["x"][l], r32["x"][l]):
                    assert G.same_bits(a, b).all() and G.is_bf16(a)
            ndiff += ref["diff"]
            nent += B * d["R"] * (d["L"] - 1)
            lg = ref["logits"]
            if d["head"] == "softmax":
                ks = N.tie_kinds(lg)
                same, cross = same + ks[0], cross + ks[1]
                winners |= set(ks[2].tolist())
                assert ((lg == lg.max(-1, keepdims=True)).sum(-1) >= 2).all()      # every row's maximum is a tie
            seen |= (lg != N.b2_step(d, t)).any(0)
            live += float((lg != N.b2_step(d, t)).mean())
        # the padded and the unpadded ring give the throughput body one answer: it reads no slot of a step before 0
        a = N.step_a(d, N.plant(d, t, False), t, carry[:, 0], carry[:, 1], cb)
        b = N.step_a(d, N.plant(d, t, True), t, carry[:, 0], carry[:, 1], cb)
        assert np.array_equal(a["logits"], b["logits"])
    # every class carries a term beyond its bias somewhere: a dropped class tile cannot hide in the bias
    assert seen.all() and live / (2 * len(N.steps_a(dil))) > 0.5
    if d["head"] == "softmax":
        # the argmax's tie rule is exercised: maxima tied inside one lane's four classes and across lanes, in every case,
        # and the winner changes with the step (not one class for every launch)
        assert same > 0 and cross > 0 and len(winners) >= 2, (same, cross, winners)
    if PRINT:
        cd = "the two conditioned forms differ on %d of %d entries" % (ndiff, nent) if d["cond"] else "unconditioned"
        tie = "; maxima tied inside a lane in %d rows, across lanes in %d, %d distinct winners" % (same, cross, len(winners))
        print("MEASURED design A %s: %s%s; %.0f %% of the logits off their bias"
              % (case, cd, tie if d["head"] == "softmax" else "", 100 * live / (2 * len(N.steps_a(dil)))))


def test_design_a_multi_step_launches_read_planted_taps_only():
    d = N.design_a("d4", 64, 256, 33, "softmax", 256, False)
    for t, n in ((1000, 2), (1000, 4), (3, 4)):
        carry, forced = N.samples_a(d, t, n)
        ring = N.plant(d, t, True)
        after, steps = N.run_a(d, ring, t, carry, forced, n)
        after32, steps32 = N.run_a(d, ring, t, carry, forced, n, arith="f32")
        for a, b in zip(after, after32):
            assert G.same_bits(a, b).all()
        for l, dl in enumerate(d["dil"]):
            written = {(t + j) % (dl + 1) for j in range(n)}
            for s in range(dl + 1):
                assert (s in written) or np.array_equal(after[l][s], ring[l][s])
        assert all(G.same_bits(a["logits"], b["logits"]).all() for a, b in zip(steps, steps32))


def test_restatement_errors_are_upper_figures():
    te, ge = N.measured_errs()
    if PRINT:
        print("MEASURED restatement errors: tanh %s gate %s" % (te, ge))
    for m in ("bf16", "fp32"):
        assert te[m] <= N.TANH_ERR[m] and ge[m] <= N.GATE_ERR[m]
    z = np.linspace(-1, 1, 4001)
    s = 1 / (1 + np.exp(-z))
    assert np.abs(s + z * s * (1 - s)).max() <= N.GATE_SLOPE


def free_run_restated(d, mode):
    """The float32 restatement's free run: (rings before each step, rings after, logits per step, cb per step)."""
    n = N.length_b(d["dil"])
    audio = N.audio_b(d, n)
    frames = N.frames_of(n)
    cb_all = None
    if d["cond"]:
        cb_all = D.round_to(N.cond_table(d, N.encoding(d, frames)), mode)
    rows = 32 * ((d["B"] + 31) // 32)
    ring = [np.zeros((dl + 1, rows, d["R"])) for dl in d["dil"]]
    out = []
    for t in range(n):
        a1 = audio[:, t - 1] if t >= 1 else np.zeros(d["B"])
        a2 = audio[:, t - 2] if t >= 2 else np.zeros(d["B"])
        cb = None if cb_all is None else cb_all[:, :, min(t // N.POOL, frames - 1)]
        before = [v.copy() for v in ring]
        r = N.restate_b(d, ring, t, a1, a2, cb, mode)
        for l, dl in enumerate(d["dil"]):
            ring[l][t % (dl + 1), :d["B"]] = r["x"][l]
        out.append((before, [v.copy() for v in ring], r, cb))
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", N.CASES_B, ids=lambda c: "-".join(str(v) for v in c))
def test_design_b_restatement_stays_below_c_cpu(case, mode):
    d = N.design_b(*case)
    _grids(d)
    worst_pre, worst = 0.0, {"x": 0.0, "logits": 0.0}
    ndec = nall = 0
    for t, (before, after, r, cb) in enumerate(free_run_restated(d, mode)):
        res = N.check_b(d, before, after, t, r["logits"], cb, mode, N.REACH[mode], N.C_GPU[mode])
        assert not res["bad"], res["bad"][:3]
        for k in worst:
            worst[k] = max(worst[k], res["worst"][k])
        ndec += res["decided"][0]; nall += res["decided"][1]
        # the value before rnd_T against the reach alone (sets REACH)
        for l, dl in enumerate(d["dil"][:-1]):
            x_t = after[l][t % (dl + 1)][:d["B"]]
            x_tap = before[l][(t + 1) % (dl + 1)][:d["B"]] if t - dl >= 0 else np.zeros_like(x_t)
            ref = N.layer_b(d, l, x_t, x_tap, cb[l + 1] if cb is not None else None, mode, N.REACH[mode])
            err = np.abs(r["pre"][l] - ref["x"])
            worst_pre = max(worst_pre, float(np.where(err == 0, 0.0, err / np.maximum(ref["e"], 1e-300)).max()))
    if PRINT:
        print("MEASURED design B %s %s: pre %.3f  x %.3f  logits %.3f  decided %.1f %%"
              % (case, mode, worst_pre, worst["x"], worst["logits"], 100.0 * ndec / max(nall, 1)))
    assert worst_pre <= N.C_CPU_PRE[mode]
    assert all(worst[k] <= N.C_CPU[mode][k] for k in worst)
