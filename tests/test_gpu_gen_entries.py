"""The queue-cached generators (csrc/srwn_gen.hip, csrc/srwn_gen16.hip and their slot / live forms) held to the
references of tests/gen_design.py ENTRY BY ENTRY: every ring row a launch writes, every ring row it must leave alone,
every logit, the codes, the audio and the carry.

Design A (planted rings, bf16 mode): bit for bit, no entry of a stream < B left out.  Rows of streams >= B in the last
group are outside the contract (the kernels compute on them and the throughput body stores them) and are excluded in the
slot a launch writes; in every other slot they too must keep their planted bits.  The latency body reads the causal
padding from the ring (its callers hand the rings over zero-filled), so it runs on the padded planting and the bodies are
compared with each other there; the throughput body runs on both plantings against ONE reference.
Design B (free run on the kernel's own rings, both modes): per entry within
    |got - x| <= ulp_T(ref) + c (u_out |x| + e),    c = 4 C_CPU,
and bit for bit where the midpoint distance exceeds REACH x e; then one launch and chunks of 1 and N - 1 against the
chain of one-step launches, bit for bit.

Float32 NumPy restatement on the CPU (tests/test_gen_design.py), C_CPU, the bound's c, and the MI355X
(SRWN_PRINT_ERR=1 pytest -s -m gpu tests/test_gpu_gen_entries.py), per quantity:

                          float32 NumPy   C_CPU    c      MI355X (worst over the cases; thr = lat1 = lat2 to the digit)
    design A              bit for bit      -       -      bit for bit: 10.8 M ring entries and logits over the nine cases
    design B  bf16  x     1.992            2.0     8.0    1.992   (99.1 / 99.1 / 99.9 % of the ring entries decided: bit-equal)
              bf16  logit 0.479            0.5     2.0    0.479
              fp32  x     0.113            0.125   0.5    0.117
              fp32  logit 0.001            0.0625  0.25   0.001
    (pre-rounding ratio that sets REACH: bf16 0.946 -> 1.0, fp32 0.121 -> 0.125; the bf16 figures are those of a correctly
    rounded output against u_out = 2^-9, reached on the CPU and the GPU alike.)
Design A's argmax: every softmax row's maximum is an exact tie of two twin classes (N.b2_step).  Rows of the kernels' own
logits tied inside one lane's four classes / across lanes, per case: 12 / 4, 396 / 264, 512 / 256, 528 / 264, 528 / 272.
Wall time of the whole file on the MI355X: 6.7 s for its 28 tests, the slowest 0.6 s.

Mutations (scratch builds of the library, never committed; in-bounds arithmetic only).  "new": tests of this file that
fail, of 28; "old": of the 340 tests of the seven existing generation files (test_gpu_generate*.py,
test_gpu_decode_live.py, test_gpu_depth.py), run against the same mutated library, those that still pass:

    mutation                                                                    new fail   old pass
    one k-slice of wave 1's delayed-tap conv image skipped (srwn_gen16.hip)     21 / 28    301 / 340
    ring store at slot t+1 and the delayed-tap read moved by one (srwn_gen.hip) 27 / 28    303 / 340
    tap0 true one step early (srwn_gen.hip)                                     14 / 28    274 / 340
    z left unrounded before the gate (srwn_gen.hip)                             21 / 28    340 / 340
    stream 5's column of the skip accumulator x 1.03 (srwn_gen.hip)             17 / 28    325 / 340
    last class tile of a C = 100 head skipped (srwn_gen.hip)                     4 / 28    338 / 340
    argmax: `>` made `>=` inside a lane's four classes (srwn_gen.hip)            9 / 28    340 / 340
    argmax: on equal values the HIGHER index wins between lanes (srwn_gen16.hip) 6 / 28    340 / 340
    `>` made `>=` in a head relu                                                 not built: an equivalent mutant -- the
        relus are fmaxf(x, 0), and either comparison returns a zero at an exact zero (the designs reach exact zeros in r0
        and r1; G.same_bits takes a zero of either sign for a zero, as the MFMA operand does)
"""
import os

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests import gemm_design as G
from tests import gen_design as N
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev

pytestmark = pytest.mark.gpu

PRINT = bool(os.environ.get("SRWN_PRINT_ERR"))
BODIES = (("thr", {"SRWN_GEN16": "0"}), ("lat1", {"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "1"}),
          ("lat2", {"SRWN_GEN16": "1", "SRWN_GEN16_NCB": "2"}))
POISON_F, POISON_I = 7.5, -77
_ENGINES = {}


def _ids(c):
    return "-".join(str(v) for v in c)


def _engine(d, dt):
    key = (d["seed"], dt)
    if key not in _ENGINES:
        EG = sub("engine")
        L, R = d["L"], d["R"]
        zero = np.zeros((2, R, R))
        layers = [O.LayerParams(d["wf"][l], d["bf"][l], zero, np.zeros(R), d["wr"][l], d["br"][l], d["ws"][l], d["bs"][l],
                                d["wc"][l] if d["cond"] else None, d["bc"][l] if d["cond"] else None) for l in range(L)]
        sp = O.StackParams(d["init_w"].reshape(2, 1, R), d["init_b"], layers, d["w1"], d["b1"], d["w2"], d["b2"],
                           tuple(d["dil"]))
        cfg = EG.StackConfig(dilations=d["dil"], dilation_channels=R, skip_channels=d["S"], output_channels=d["C"],
                             cond_channels=N.ENC if d["cond"] else 0, pool_stride=N.POOL if d["cond"] else 1,
                             shift_input=True, head_mode="mol" if d["head"] == "mol" else "per_timestep", dtype=dt)
        eng = EG.WaveNetEngine(cfg, d["B"], 8, DEV)
        eng.load_oracle_params(sp)
        _ENGINES.clear()          # (one engine alive at a time: the cases are visited in order)
        _ENGINES[key] = eng
    return _ENGINES[key]


def _set_body(monkeypatch, env):
    monkeypatch.delenv("SRWN_GEN16_NCB", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _ring_to_dev(layers, d, dt):
    return dev(N.ring_pack(layers, d["dil"], d["R"], d["B"]), dt)


def _ring_from_dev(t, d):
    return N.ring_unpack(t.float().cpu().numpy(), d["dil"], d["R"], d["B"])


def _check_outputs(d, logits, codes, audio):
    """codes / audio of a mode-0 launch against the kernel's OWN logits [B, C] (bit for bit)."""
    if d["head"] == "softmax":
        assert np.array_equal(codes, N.first_max(logits)), "codes are not the first maximum of the logits"
        assert np.array_equal(audio.view(np.uint32), O.mu_law_decode(codes, d["C"]).astype(np.float32).view(np.uint32))
    else:
        M = d["M"]
        assert (codes >= 0).all() and (codes < M).all()
        mean = np.take_along_axis(logits, (M + codes)[:, None], 1)[:, 0]
        assert G.same_bits(audio, np.clip(mean, -1.0, 1.0)).all(), "audio is not the selected mixture's clamped mean"


def _check_ring(d, got, planted, written, ref_x, rows_owned, what):
    """got / planted: per layer [depth, rows, R]; written: per layer the set of slots the launch writes; ref_x: per layer
    {slot: [admissible rows [B, R]]}; rows_owned: the rows whose written slot is under the contract."""
    for l, dl in enumerate(d["dil"]):
        for s in range(dl + 1):
            if s in written[l]:
                ok = N.matches_any(got[l][s][:d["B"]], ref_x[l][s])[rows_owned]
                assert ok.all(), "%s: layer %d slot %d: %d of %d written entries differ" % (what, l, s, int((~ok).sum()), ok.size)
            else:
                ok = G.same_bits(got[l][s], planted[l][s])
                assert ok.all(), "%s: layer %d slot %d: %d untouched entries changed" % (what, l, s, int((~ok).sum()))


def _set_b2(eng, d, t):
    """The last bias of a launch at step t (N.b2_step: the step's boosted twins): the generators read it from the
    parameters at every launch, so it is written there."""
    if d["head"] == "softmax":
        eng.view("head_b2")[:d["C"]].copy_(dev(N.b2_step(d, t)))


def _project(eng, enc):
    """The engine's conditioning table [rows * frames, L R] of an encoding [rows, frames, ENC]."""
    return eng._project_cond(dev(enc).reshape(-1, N.ENC))


def _cond(d, frames, key=0):
    """(encoding, cb [L, B, frames, R]) of a conditioned design."""
    if not d["cond"]:
        return None, None
    enc = N.encoding(d, frames, key)
    return enc, N.cond_table(d, enc)


# ---- design A, the resume forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.CASES_A, ids=_ids)
def test_planted_step_bit_for_bit(monkeypatch, case):
    d = N.design_a(*case)
    eng = _engine(d, torch.bfloat16)
    assert eng.o_g16 is not None
    B, L = d["B"], d["L"]
    frames = N.frames_of(1001)
    enc, cb_all = _cond(d, frames)
    rows = np.arange(B)
    nent = same = cross = 0
    for t in N.steps_a(d["dil"]):
        _set_b2(eng, d, t)
        carry, _ = N.samples_a(d, t, 1)
        cb = None if cb_all is None else cb_all[:, :, min(t // N.POOL, frames - 1)]
        ref = N.step_a(d, N.plant(d, t, True), t, carry[:, 0], carry[:, 1], cb)
        outs = {}
        for name, env, pad in [("thr-unpadded", BODIES[0][1], False)] + [(n, e, True) for n, e in BODIES]:
            _set_body(monkeypatch, env)
            planted = N.plant(d, t, pad)
            st = eng.generation_state(B, cond=None if enc is None else dev(enc), seed=3)
            if cb_all is not None:      # the projected table itself: cb = enc Wc + bc, exact
                tab = st.cond_all.float().cpu().numpy().reshape(B, frames, L, d["R"]).transpose(2, 0, 1, 3)
                assert G.same_bits(tab, cb_all).all()
            st.ring.copy_(_ring_to_dev(planted, d, torch.bfloat16))
            st.carry.copy_(dev(carry))
            st.t = t
            audio, codes, logits = eng.generate_chunk(st, 1, mode="argmax", want_logits=True)
            what = "%s t=%d" % (name, t)
            lg = logits.cpu().numpy()[:, 0].astype(np.float64)
            ok = G.same_bits(lg, ref["logits"])
            assert ok.all(), "%s: %d of %d logits differ" % (what, int((~ok).sum()), ok.size)
            a, c = audio.cpu().numpy()[:, 0], codes.cpu().numpy()[:, 0]
            _check_outputs(d, lg, c, a)
            got = _ring_from_dev(st.ring, d)
            _check_ring(d, got, planted, [{s} for s in ref["wslot"]],
                        [{ref["wslot"][l]: ref["x"][l]} for l in range(L)], rows, what)
            cr = st.carry.cpu().numpy()
            assert G.same_bits(cr[:, 0], a).all() and G.same_bits(cr[:, 1], carry[:, 0]).all(), what + ": carry"
            assert st.t == t + 1
            outs[name] = (st.ring.clone(), logits, codes, audio, st.carry.clone())
            nent += lg.size + sum(v.size for v in got)
            if d["head"] == "softmax":
                ks = N.tie_kinds(lg)
                same, cross = same + ks[0], cross + ks[1]
        if ref["diff"] == 0:      # the bodies and both workgroup sizes: identical bits, not agreement within a norm
            for name in ("lat1", "lat2"):
                for x, y in zip(outs["thr"][1:], outs[name][1:]):
                    assert torch.equal(x, y), "%s differs from the throughput body at t=%d" % (name, t)
                gr, gt = _ring_from_dev(outs[name][0], d), _ring_from_dev(outs["thr"][0], d)
                for l in range(L):
                    assert G.same_bits(gr[l][:, :B], gt[l][:, :B]).all()
    # the kernel's own logits held ties among their maxima of both kinds, so `codes` met the tie rule inside a lane and
    # between lanes
    assert d["head"] != "softmax" or (same > 0 and cross > 0)
    if PRINT:
        ties = "; maxima tied inside a lane in %d rows, across lanes in %d" % (same, cross) if d["head"] == "softmax" else ""
        print("MEASURED design A %s: %d entries (ring rows, logits) bit for bit over 4 launches x %d steps%s"
              % (_ids(case), nent, len(N.steps_a(d["dil"])), ties))


@pytest.mark.parametrize("t,n", [(1000, 2), (1000, 4), (3, 4)])
def test_planted_multi_step_launch_bit_for_bit(monkeypatch, t, n):
    """nsteps <= min d reads only planted taps: the in-kernel step loop (ring slot advance, forced rows, the weight double
    buffer across steps, the latency body's look-ahead into the next step) bit for bit."""
    d = N.design_a("d4", 64, 256, 33, "softmax", 256, False)
    eng = _engine(d, torch.bfloat16)
    B, L = d["B"], d["L"]
    _set_b2(eng, d, t)
    carry, forced = N.samples_a(d, t, n)
    planted = N.plant(d, t, True)
    after, steps = N.run_a(d, planted, t, carry, forced, n)
    written = [{(t + j) % (dl + 1) for j in range(n)} for dl in d["dil"]]
    ref_x = [{s: [after[l][s][:B]] for s in written[l]} for l in range(L)]
    for name, env in BODIES:
        _set_body(monkeypatch, env)
        st = eng.generation_state(B, seed=3)
        st.ring.copy_(_ring_to_dev(planted, d, torch.bfloat16))
        st.carry.copy_(dev(carry))
        st.t = t
        audio, codes, logits = eng.generate_chunk(st, n, mode="argmax", forced=dev(forced), want_logits=True)
        lg = logits.cpu().numpy().astype(np.float64)
        for j in range(n):
            ok = G.same_bits(lg[:, j], steps[j]["logits"])
            assert ok.all(), "%s step %d: %d logits differ" % (name, t + j, int((~ok).sum()))
            _check_outputs(d, lg[:, j], codes.cpu().numpy()[:, j], audio.cpu().numpy()[:, j])
        _check_ring(d, _ring_from_dev(st.ring, d), planted, written, ref_x, np.arange(B), "%s t=%d n=%d" % (name, t, n))
        cr = st.carry.cpu().numpy()      # forced: the samples the next step reads are the forced ones
        assert G.same_bits(cr[:, 0], forced[:, n - 1]).all() and G.same_bits(cr[:, 1], forced[:, n - 2]).all()


@pytest.mark.parametrize("case", [N.CASES_A[0], N.CASES_A[1], N.CASES_A[6]], ids=_ids)
def test_planted_step_fp32_exact_part(monkeypatch, case):
    """fp32 mode, throughput body: what needs no transcendental is exact -- x_0 in layer 0's written slot, and every slot
    the step does not own."""
    d = N.design_a(*case)
    eng = _engine(d, torch.float32)
    _set_body(monkeypatch, BODIES[0][1])
    B, L = d["B"], d["L"]
    frames = N.frames_of(1001)
    enc, cb_all = _cond(d, frames)
    for t in N.steps_a(d["dil"]):
        carry, _ = N.samples_a(d, t, 1)
        x0 = d["init_w"][0] * carry[:, 1:2] + d["init_w"][1] * carry[:, 0:1] + d["init_b"]
        if cb_all is not None:
            x0 = x0 + cb_all[0][:, min(t // N.POOL, frames - 1)]
        planted = N.plant(d, t, False)
        st = eng.generation_state(B, cond=None if enc is None else dev(enc), seed=3)
        st.ring.copy_(_ring_to_dev(planted, d, torch.float32))
        st.carry.copy_(dev(carry))
        st.t = t
        _, _, logits = eng.generate_chunk(st, 1, mode="argmax", want_logits=True)
        assert torch.isfinite(logits).all()
        got = _ring_from_dev(st.ring, d)
        for l, dl in enumerate(d["dil"]):
            for s in range(dl + 1):
                if s != t % (dl + 1):
                    assert G.same_bits(got[l][s], planted[l][s]).all(), "t=%d layer %d slot %d changed" % (t, l, s)
        assert G.same_bits(got[0][t % (d["dil"][0] + 1)][:B], x0).all(), "t=%d: x_0" % t


def test_planted_step_live_form_bit_for_bit(monkeypatch):
    """The live form: the conditioning table is a ring of 7 frames and step 1000 reads row (1000 / 4) mod 7 = 5."""
    d = N.design_a(*N.CASES_A[6])
    eng = _engine(d, torch.bfloat16)
    B, L, t, F = d["B"], d["L"], 1000, 7
    enc, cb_all = _cond(d, F, key=4)
    cb = cb_all[:, :, (t // N.POOL) % F]
    carry, _ = N.samples_a(d, t, 1, key=4)
    planted = N.plant(d, t, True, key=4)
    ref = N.step_a(d, planted, t, carry[:, 0], carry[:, 1], cb)
    for name, env in BODIES:
        _set_body(monkeypatch, env)
        st = eng.live_generation_state(B, F, seed=3)
        st.cond_all.copy_(_project(eng, enc))
        st.fed = t // N.POOL + 1
        st.limit, st.t = st.fed * N.POOL, t
        st.ring.copy_(_ring_to_dev(planted, d, torch.bfloat16))
        st.carry.copy_(dev(carry))
        audio, codes, logits = eng.generate_chunk(st, 1, mode="argmax", want_logits=True)
        lg = logits.cpu().numpy()[:, 0].astype(np.float64)
        assert G.same_bits(lg, ref["logits"]).all(), name
        _check_outputs(d, lg, codes.cpu().numpy()[:, 0], audio.cpu().numpy()[:, 0])
        _check_ring(d, _ring_from_dev(st.ring, d), planted, [{s} for s in ref["wslot"]],
                    [{ref["wslot"][l]: ref["x"][l]} for l in range(L)], np.arange(B), name)


# ---- design A, the slot forms ----------------------------------------------------------------------------------------------
def _pool_at(eng, d, clock, t_own, end, live=False, frames=None, enc=None, key=0):
    """A pool of d["B"] slots put at `clock` with every slot at its own step (t_own, end) without running there: the one
    place that reaches into GenerationPool's host mirror.  Rings and carry are planted (nothing padded: the slot forms
    read what the ring holds).  Returns (pool, planted ring, carry)."""
    cap = d["B"]
    pool = eng.generation_pool(cap, frames if d["cond"] else None, live=live)
    pool.clock = clock
    pool._t[:], pool._end[:], pool._seed[:], pool._active[:] = t_own, end, list(range(11, 11 + cap)), True
    pool._upload()
    if enc is not None:
        pool.cond_all.copy_(_project(eng, enc))
    planted = N.plant(d, clock, False, key=key)
    carry, _ = N.samples_a(d, clock, 1, key=key)
    pool.ring.copy_(_ring_to_dev(planted, d, torch.bfloat16))
    pool.carry.copy_(dev(carry))
    _set_b2(eng, d, clock)
    return pool, planted, carry


def _slot_launch(eng, pool, n, live=False):
    """One launch of the pool's slot form into POISONED outputs (the caller owns them: rows of steps that do not run must
    keep what it put there)."""
    cap, C = pool.capacity, eng.C
    audio = torch.full((cap, n), POISON_F, dtype=torch.float32, device=DEV)
    codes = torch.full((cap, n), POISON_I, dtype=torch.int32, device=DEV)
    logits = torch.full((cap, n, C), POISON_F, dtype=torch.float32, device=DEV)
    eng._launch_generation(ring=pool.ring, audio=audio, codes=codes, logits=logits, forced=None, batch=cap, nsteps=n,
                           mode="argmax", seed=0, t0=pool.clock, carry=pool.carry, sampling=None, cond_all=pool.cond_all,
                           frames=pool.frames, slots=pool.slots, live=live)
    return audio.cpu().numpy(), codes.cpu().numpy(), logits.cpu().numpy().astype(np.float64)


def _slot_table(cap, clock):
    """Each slot at its own step, none equal to the clock; slot 3 idle (t_end = t), slot 5 past its end (t_end < t)."""
    t = np.array([7 + 3 * (u % 5) for u in range(cap)], np.int64)
    end = t + 100
    end[3], end[5] = t[3], t[5] - 4
    assert (t != clock).all()
    return t, end


@pytest.mark.parametrize("case,live", [(N.CASES_A[4], False), (N.CASES_A[6], False), (N.CASES_A[6], True)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else ("live" if v else "pool"))
def test_planted_slot_form_bit_for_bit(monkeypatch, case, live):
    """A pool of 33 slots at clock 1000, every slot at its own step: ring slots follow the clock, the conditioning frame
    the slot's own step; an idle slot, one past its end (and, live, a starved one) keep their outputs, carry and t --
    and the starved slot of a live pool its ring rows."""
    d = N.design_a(*case)
    eng = _engine(d, torch.bfloat16)
    cap, L, clock = d["B"], d["L"], 1000
    assert cap == 33
    frames = 9
    for name, env in BODIES:
        _set_body(monkeypatch, env)
        t_own, end = _slot_table(cap, clock)
        if live:      # slot 8 is starved: it has used up the frames it was fed
            end[8] = t_own[8]
        idle = end <= t_own
        enc, cb_all = _cond(d, frames, key=1)
        cb = None
        if d["cond"]:
            fr = t_own // N.POOL
            fr = fr % frames if live else np.clip(fr, 0, frames - 1)      # the live table is a ring of `frames` rows
            cb = cb_all[:, np.arange(cap), fr]
        pool, planted, carry = _pool_at(eng, d, clock, t_own, end, live, frames, enc, key=2)
        ref = N.step_a(d, planted, 0, carry[:, 0], carry[:, 1], cb, tap_from_ring=True, slot=clock)
        audio, codes, lg = _slot_launch(eng, pool, 1, live)
        run = ~idle
        ok = G.same_bits(lg[run, 0], ref["logits"][run])
        assert ok.all(), "%s: %d logits differ" % (name, int((~ok).sum()))
        _check_outputs(d, lg[run, 0], codes[run, 0], audio[run, 0])
        assert (audio[idle] == POISON_F).all() and (codes[idle] == POISON_I).all() and (lg[idle] == POISON_F).all()
        cr = pool.carry.cpu().numpy()
        assert G.same_bits(cr[run, 0], audio[run, 0]).all() and G.same_bits(cr[run, 1], carry[run, 0]).all()
        assert G.same_bits(cr[idle], carry[idle]).all(), "an idle slot's carry changed"
        tab = pool.slots.cpu().numpy()
        assert np.array_equal(tab[:, 0], t_own + run) and np.array_equal(tab[:, 1], end)
        # the ring: the written slot of every slot that runs; everything else keeps its planted bits -- in the live form
        # also the written slot of the rows that do not run
        owned = np.flatnonzero(run)
        got = _ring_from_dev(pool.ring, d)
        _check_ring(d, got, planted, [{s} for s in ref["wslot"]], [{ref["wslot"][l]: ref["x"][l]} for l in range(L)],
                    owned, name)
        if live:
            for l in range(L):
                s = ref["wslot"][l]
                assert G.same_bits(got[l][s][:cap][idle], planted[l][s][:cap][idle]).all(), \
                    "%s: a slot that did not run stored into layer %d" % (name, l)


def test_planted_slot_form_rows_beyond_the_steps_that_ran(monkeypatch):
    """A launch of 4 pool steps (<= min d: planted taps only) in which slot 2 has one step left and slot 4 two: their
    rows beyond keep the poison, their carry and t stop with them."""
    d = N.design_a(*N.CASES_A[4])
    eng = _engine(d, torch.bfloat16)
    cap, clock, n = d["B"], 1000, 4
    for name, env in BODIES:
        _set_body(monkeypatch, env)
        t_own, end = _slot_table(cap, clock)
        end[2], end[4] = t_own[2] + 1, t_own[4] + 2
        ran = np.clip(end - t_own, 0, n)
        pool, planted, carry = _pool_at(eng, d, clock, t_own, end, key=3)
        audio, codes, lg = _slot_launch(eng, pool, n)
        # free running: from the second step on the input is the slot's own emitted sample (off the grid of design A), so
        # the logits are held at step 0 and the codes / audio of every step to the kernel's own logits
        prev = [carry[:, 0].copy(), carry[:, 1].copy()]
        for j in range(n):
            live = ran > j
            if j == 0:
                ref = N.step_a(d, planted, 0, prev[0], prev[1], None, tap_from_ring=True, slot=clock)
                assert G.same_bits(lg[live, 0], ref["logits"][live]).all()
            _check_outputs(d, lg[live, j], codes[live, j], audio[live, j])
            assert (audio[~live, j] == POISON_F).all() and (codes[~live, j] == POISON_I).all() \
                and (lg[~live, j] == POISON_F).all(), "%s: a row beyond the steps that ran was written" % name
        cr = pool.carry.cpu().numpy()
        for u in range(cap):
            if ran[u] == 0:
                assert G.same_bits(cr[u], carry[u]).all()
            else:
                want1 = audio[u, ran[u] - 2] if ran[u] >= 2 else carry[u, 0]
                assert G.same_bits(cr[u, 0], audio[u, ran[u] - 1]).all() and G.same_bits(cr[u, 1], want1).all()
        assert np.array_equal(pool.slots.cpu().numpy()[:, 0], t_own + ran)


# ---- design B ------------------------------------------------------------------------------------------------------------
def _free_run(eng, d, dt, audio, enc, chunks):
    """The run as launches of the given lengths: (ring copies after each launch, logits, codes, carry, final ring)."""
    st = eng.generation_state(d["B"], cond=None if enc is None else dev(enc), seed=5)
    rings, lgs, cds, t = [], [], [], 0
    for n in chunks:
        _, codes, logits = eng.generate_chunk(st, n, mode="argmax", forced=dev(audio[:, t:t + n]), want_logits=True)
        rings.append(st.ring.clone())
        lgs.append(logits); cds.append(codes)
        t += n
    return rings, torch.cat(lgs, 1), torch.cat(cds, 1), st.carry.clone(), st


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("case", N.CASES_B, ids=_ids)
def test_free_run_per_entry(monkeypatch, case, mode):
    d = N.design_b(*case)
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    eng = _engine(d, dt)
    B, L = d["B"], d["L"]
    n = N.length_b(d["dil"])
    audio = N.audio_b(d, n)
    frames = N.frames_of(n)
    enc, cb_all = _cond(d, frames)
    worst = {}
    for name, env in (BODIES if mode == "bf16" else BODIES[:1]):
        _set_body(monkeypatch, env)
        rings, logits, codes, carry, st = _free_run(eng, d, dt, audio, enc, [1] * n)
        if cb_all is not None:
            tab = st.cond_all.float().cpu().numpy().reshape(B, frames, L, d["R"]).transpose(2, 0, 1, 3)
            assert G.same_bits(tab, N.D.round_to(cb_all, mode)).all()
            cb_t = tab
        lg = logits.cpu().numpy().astype(np.float64)
        before = [np.zeros((dl + 1, 32 * ((B + 31) // 32), d["R"])) for dl in d["dil"]]
        w = {"x": 0.0, "logits": 0.0}
        ndec = nall = 0
        for t in range(n):
            after = _ring_from_dev(rings[t], d)
            cb = None if cb_all is None else cb_t[:, :, min(t // N.POOL, frames - 1)]
            a1 = audio[:, t - 1] if t >= 1 else np.zeros(B)
            a2 = audio[:, t - 2] if t >= 2 else np.zeros(B)
            x0 = N.x0_b(d, a1, a2, None if cb is None else cb[0], mode)
            assert G.same_bits(after[0][t % (d["dil"][0] + 1)][:B], x0).all(), "%s step %d: x_0" % (name, t)
            for l, dl in enumerate(d["dil"]):      # one writer, the right slot: every other slot keeps its bits
                for s in range(dl + 1):
                    if s != t % (dl + 1):
                        assert np.array_equal(after[l][s], before[l][s]), "%s step %d layer %d slot %d" % (name, t, l, s)
            res = N.check_b(d, before, after, t, lg[:, t], cb, mode, N.REACH[mode], N.C_GPU[mode])
            assert not res["bad"], (name, res["bad"][:4])
            for k in w:
                w[k] = max(w[k], res["worst"][k])
            ndec += res["decided"][0]; nall += res["decided"][1]
            before = after
        worst[name] = (w, ndec, nall)
        # the same steps as one launch, and as chunks of 1 and n - 1: the bits of the one-step chain
        for chunks in ([n], [1, n - 1]) if n > 1 else ([n],):
            r2, lg2, cd2, cr2, _ = _free_run(eng, d, dt, audio, enc, chunks)
            assert torch.equal(lg2, logits) and torch.equal(cd2, codes) and torch.equal(cr2, carry), (name, chunks)
            ga, gb = _ring_from_dev(r2[-1], d), _ring_from_dev(rings[-1], d)
            for l in range(L):
                assert G.same_bits(ga[l][:, :B], gb[l][:, :B]).all(), (name, chunks, l)
    if PRINT:
        for name, (w, ndec, nall) in worst.items():
            print("MEASURED design B %s %s %s: x %.3f (c = %.2f)  logits %.3f (c = %.2f)  decided %.1f %% of %d ring entries"
                  % (_ids(case), mode, name, w["x"], N.C_GPU[mode]["x"], w["logits"], N.C_GPU[mode]["logits"],
                     100.0 * ndec / max(nall, 1), nall))
