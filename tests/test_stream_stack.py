"""CPU tests of the one streaming stack (stream_stack.StreamStack) and of its users' launch lists: every group launch names
the entry point of its form with an argument list of that entry point's length and kinds on the stack's own buffers; one
step of the classifier, of both scorers and of the synthesizer records exactly the launches its docstring and its
launches_per_step / launches_per_chunk promise; and no other code of the package names a group stream entry point or reads
the group plan's environment variable.  ``_lib.call`` is a recorder here and the weights are stand-ins on host memory."""
import ctypes as C
import glob
import itertools
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests._pkg import ROOT, sub

DIL = [1, 2, 4, 8, 16, 32, 64]
L, R, S, KW = len(DIL), 32, 128, 2
BM, CHUNK, N = 3, 48, 17
CALLERS = ("_lib", "kernels", "stream_stack", "recognizer", "scorer", "student")
NAMES = {(False, False): "srwn_residual_group_fwd_stream", (False, True): "srwn_residual_group_fwd_stream_slots",
         (True, False): "srwn_residual_group_fwd_stream_z", (True, True): "srwn_residual_group_fwd_stream_z_slots"}


class Weights:
    """What the streaming users read of a StackWeights / FlowWeights, on host memory: sections, zero parameters, an image
    buffer and made-up image offsets."""

    def __init__(self, cfg=None, device="cpu", classes=256, E=0, M=0, pool=1):
        EG = sub("engine")
        self.dil, self.L, self.R, self.S, self.Kw, self.dt, self.dev = list(DIL), L, R, S, KW, torch.bfloat16, torch.device("cpu")
        self.C, self.E, self.Ep, self.M, self.pool = classes, E, (E + 15) // 16 * 16, M, pool
        self.Cp = (classes + 31) // 32 * 32
        shapes = {"init_w": (KW, 1, R), "init_b": (R,), "BF": (L, R), "BR": (L, R), "BC": (L, R), "head_b1": (S,),
                  "head_w2": (S, self.Cp), "head_b2": (self.Cp,), "flow_w": (R, 2), "flow_b": (2,)}
        self.sections, off = {}, 0
        for name, shp in shapes.items():
            self.sections[name] = EG.Section(name, off, shp)
            off += self.sections[name].numel
        self.params, self.bs_sum = torch.zeros(off), torch.zeros(S)
        self.packed = torch.zeros(64 * (2 * L + 8), dtype=self.dt)
        self.o_conv, self.o_res = [64 * l for l in range(L)], [64 * (L + l) for l in range(L)]
        self.o_skip, self.o_w1, self.o_w2, self.o_wc = (64 * (2 * L + i) for i in range(4))

    def view(self, name):
        s = self.sections[name]
        return self.params[s.offset:s.offset + s.numel].view(s.shape)

    def wptr(self, off):
        return self.packed.data_ptr() + off * self.packed.element_size()

    def repack(self):
        pass


@pytest.fixture
def calls(monkeypatch):
    """The recorder in the place of ``_lib.call`` wherever a module of the package holds it, no device needed to build a
    user, and K.pw_linear's tensors taken from the host."""
    rec = []
    for m in CALLERS:
        if hasattr(sub(m), "call"):
            monkeypatch.setattr(sub(m), "call", lambda name, *args: rec.append((name, args)))
    monkeypatch.setattr(sub("kernels"), "_need_gpu", lambda: None)
    monkeypatch.setattr(sub("kernels"), "_chk", lambda t, name, dtype=None, shape=None: t.data_ptr())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: SimpleNamespace(cuda_stream=0))
    monkeypatch.delenv("SRWN_GROUP_LAYERS", raising=False)
    return rec


def _check_kinds(name, args):
    """What both bindings can pass: None, an address or a ctypes array for a pointer, a plain int for a number."""
    LIB = sub("_lib")
    kinds = LIB.SIGNATURES[name][1]
    assert len(args) == len(kinds), (name, len(args), len(kinds))
    for i, (a, k) in enumerate(zip(args, kinds)):
        if k is LIB._p:
            assert a is None or isinstance(a, (int, C.Array)), (name, i, a)
        else:
            assert isinstance(a, int) and not isinstance(a, bool), (name, i, a)


# ---- 1. the group launches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store_z,slots,with_cond", list(itertools.product([False, True], repeat=3)))
def test_launch_groups_names_its_form_on_its_own_buffers(calls, store_z, slots, with_cond):
    w = Weights()
    sk = sub("stream_stack").StreamStack(w, BM, CHUNK, store_z=store_z)
    G = len(sk.groups)
    assert G >= 2 and sk.groups[0][0] == 0 and sk.groups[-1][1] == L
    assert sk.hist == [sum(DIL[a:b]) for a, b in sk.groups] and sk.hist_max == max(sk.hist)
    assert [tuple(b.shape) for b in sk.bufs] == [(BM, h + CHUNK, R) for h in sk.hist] and tuple(sk.top.shape) == (BM, CHUNK, R)
    assert (sk.zs is None) == (not store_z)
    assert sk.roll.tolist() == [[b.data_ptr(), h + CHUNK, h] for b, h in zip(sk.bufs, sk.hist)]
    table = torch.zeros((L, 8, R), dtype=w.dt)
    ptrs = [table[l + 1].data_ptr() if l + 1 < L else None for l in range(L)]
    when = 0x7700
    sk.launch_groups(BM, N, when, slots, (ptrs, 8, 5, R) if with_cond else None)
    assert [n for n, _ in calls] == [NAMES[store_z, slots]] * G
    for g, ((l0, l1), (name, a)) in enumerate(zip(sk.groups, calls)):
        _check_kinds(name, a)
        last = g + 1 == G
        assert a[:2] == (sk.bufs[g].data_ptr(), sk.hist[g] + CHUNK)
        if last:
            assert a[2:5] == (sk.top.data_ptr(), CHUNK, 0)
        else:
            assert a[2:5] == (sk.bufs[g + 1].data_ptr(), sk.hist[g + 1] + CHUNK, sk.hist[g + 1])
        rest = a[5:]
        if store_z:
            assert rest[:2] == (sk.zs[l0].data_ptr(), BM * CHUNK * R)
            rest = rest[2:]
        wconv, wres, bf, br, cond, frames, pool, cstride, dil, nl = rest[:10]
        assert list(wconv) == [w.wptr(w.o_conv[l]) for l in range(l0, l1)]
        assert list(wres) == [w.wptr(w.o_res[l]) for l in range(l0, l1)]
        assert list(bf) == [w.view("BF")[l].data_ptr() for l in range(l0, l1)]
        assert list(br) == [w.view("BR")[l].data_ptr() for l in range(l0, l1)]
        if with_cond:
            assert list(cond) == ptrs[l0:l1] and (frames, pool, cstride) == (8, 5, R)
            assert (cond[l1 - l0 - 1] is None) == last      # above the stack's top layer there is no layer to condition
        else:
            assert cond is None and (frames, pool, cstride) == (1, 1, R)
        assert list(dil) == DIL[l0:l1] and nl == l1 - l0
        assert rest[10:] == (BM, N, CHUNK, R, KW, sub("kernels").abi_dtype(w.dt), when, 0)


def test_stacks_share_a_top_and_count_their_bytes(calls):
    SK = sub("stream_stack")
    a = SK.StreamStack(Weights(), BM, CHUNK, store_z=True)
    b = SK.StreamStack(Weights(), BM, CHUNK, store_z=False, top=a.top)
    assert b.top is a.top
    es = 2
    boundary = (sum(h + CHUNK for h in a.hist) + CHUNK) * BM * R * es
    assert a.nbytes() == {"boundary": boundary, "z": L * BM * CHUNK * R * es} and b.nbytes() == {"boundary": boundary, "z": 0}
    a.bufs[1].fill_(1)
    a.reset()
    assert not any(bool(x.any()) for x in a.bufs)
    assert SK.StreamStack.plan(DIL) == (a.groups, a.hist)


# ---- 2. one step of every user --------------------------------------------------------------------------------------------
def _names(calls):
    for name, args in calls:
        _check_kinds(name, args)
    return [n for n, _ in calls]


def _classifier(monkeypatch, fused):
    monkeypatch.setenv("SRWN_RECOG_FUSED", "1" if fused else "0")
    return sub("recognizer").StreamClassifier(Weights(classes=12), max_batch=BM, hop=8, window=32, max_hops=4)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twin"])
@pytest.mark.parametrize("pooled", [False, True], ids=["alone", "pool"])
def test_classifier_step(calls, monkeypatch, fused, pooled):
    c = _classifier(monkeypatch, fused)
    assert (c.groups, c.hist, c.bufs, c.roll) == (c.stack.groups, c.stack.hist, c.stack.bufs, c.stack.roll) and c.max_chunk == 32
    pool = SimpleNamespace(table=torch.zeros((BM, 2), dtype=torch.int64), ring=torch.zeros((BM, 65)), audio_ring=65) if pooled else None
    c._launch_step(BM, 2, pool)
    sfx, G = "_slots" if pooled else "", len(c.groups)
    head = ["srwn_pooled_stream_head" + sfx] if fused else ["srwn_pw_linear"] * 2 + ["srwn_hop_sum" + sfx]
    assert _names(calls) == ["srwn_recog_stream_in" + sfx] + [NAMES[True, pooled]] * G + head + [
        "srwn_window_mean" + sfx, "srwn_pooled_head", "srwn_recog_roll" + sfx]
    assert len(calls) == c.launches_per_step
    when = pool.table.data_ptr() if pooled else c.clock.data_ptr()
    assert all(a[-2] == when for n, a in calls if n == NAMES[True, pooled])
    assert set(c.buffer_bytes()) == {"boundary", "z", "ring", "audio", "emissions", "images"} | (set() if fused else {"twin r0/r1"})
    assert {k: c.buffer_bytes()[k] for k in ("boundary", "z")} == c.stack.nbytes()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twin"])
def test_scorer_step(calls, monkeypatch, fused):
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1" if fused else "0")
    s = sub("scorer").StreamScorer(Weights(), max_batch=BM, max_chunk=CHUNK)
    s._launch_step(BM, N)
    G = len(s.groups)
    head = ["srwn_stream_score_head"] if fused else ["srwn_pw_linear"] * 3 + ["srwn_nll_rows"]
    assert _names(calls) == ["srwn_recog_stream_in"] + [NAMES[True, False]] * G + head + ["srwn_recog_roll"]
    assert len(calls) == s.launches_per_step
    assert all(a[-2] == s.clock.data_ptr() and a[11] is None for n, a in calls if n == NAMES[True, False])
    assert set(s.buffer_bytes()) == {"boundary", "z", "audio", "scores", "images"} | (set() if fused else {"twin r0/r1/logits"})
    assert {k: s.buffer_bytes()[k] for k in ("boundary", "z")} == s.stack.nbytes()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "twin"])
@pytest.mark.parametrize("E", [6, 0])
def test_mol_scorer_step(calls, monkeypatch, fused, E):
    monkeypatch.setenv("SRWN_SCORE_FUSED", "1" if fused else "0")
    w = Weights(classes=40, E=E, M=10, pool=20 if E else 1)
    s = sub("scorer").MolStreamScorer(w, max_batch=BM, max_chunk=CHUNK, max_frames=32)
    assert s.hist_max == (s.stack.hist_max if E else 0) and s.max_frames == (32 if E else 1)
    s._launch_step(BM, N)
    G = len(s.groups)
    head = ["srwn_stream_mol_score_head"] if fused else ["srwn_pw_linear"] * 3 + ["srwn_mol_score_rows"]
    assert _names(calls) == ["srwn_flow_stream_in"] + [NAMES[True, False]] * G + head + ["srwn_recog_roll"]
    assert len(calls) == s.launches_per_step
    # the conditioning ring [B * frames][L * R]: layer l adds the columns of layer l + 1
    es, groups = s.ring.element_size(), [a for n, a in calls if n == NAMES[True, False]]
    for (l0, l1), a in zip(s.groups, groups):
        if E:
            assert list(a[11]) == [s.ring.data_ptr() + (l + 1) * R * es if l + 1 < L else None for l in range(l0, l1)]
            assert a[12:15] == (32, 20, L * R)
        else:
            assert a[11] is None and a[12:15] == (1, 1, R)
    assert set(s.buffer_bytes()) == {"boundary", "z", "audio", "scores", "conditioning", "images"} | (
        set() if fused else {"twin r0/r1/logits"})


@pytest.mark.parametrize("pooled", [False, True], ids=["alone", "pool"])
@pytest.mark.parametrize("device_noise", [True, False], ids=["noise", "given"])
def test_synthesizer_chunk(calls, monkeypatch, pooled, device_noise):
    St, EG = sub("student"), sub("engine")
    monkeypatch.setattr(St, "FlowWeights", Weights)
    cfg = EG.StackConfig(dilations=DIL, dilation_channels=R, cond_channels=6, pool_stride=20)
    syn = St.FlowSynthesizer(cfg, 2, max_batch=BM, max_chunk=CHUNK, max_frames=8, device="cpu")
    G = len(syn.groups)
    assert len(syn.stacks) == 2 and all(sk.top is syn.top for sk in syn.stacks)
    assert syn.bufs == [sk.bufs for sk in syn.stacks] and (syn.groups, syn.hist) == (syn.stacks[0].groups, syn.stacks[0].hist)
    assert syn.roll_all.tolist() == [[b.data_ptr(), h + CHUNK, h] for sk in syn.stacks for b, h in zip(sk.bufs, sk.hist)]
    pool = SimpleNamespace(slots=torch.zeros((BM, 2), dtype=torch.int64), arrive=torch.zeros(1, dtype=torch.int32)) if pooled else None
    syn._launch_chunk(BM, N, device_noise, pool)
    sfx = "_slots" if pooled else ""
    flow = ["srwn_flow_stream_in" + sfx] + [NAMES[False, pooled]] * G + ["srwn_flow_stream_out" + sfx]
    assert _names(calls) == (["srwn_logistic_noise" + sfx] if device_noise else []) + flow * 2
    assert len(calls) == syn.launches_per_chunk - (0 if device_noise else 1)
    when = pool.slots.data_ptr() if pooled else syn.clock.data_ptr()
    groups = [a for n, a in calls if n == NAMES[False, pooled]]
    for i in range(2):      # one conditioning table [rows, R] per layer: layer l adds layer l + 1's
        for (l0, l1), a in zip(syn.groups, groups[i * G:(i + 1) * G]):
            assert list(a[9]) == [syn.cond_all[i][l + 1].data_ptr() if l + 1 < L else None for l in range(l0, l1)]
            assert a[10:13] == (8, 20, R) and a[-2] == when


# ---- 3. the entry points and the plan are named in one place --------------------------------------------------------------
def test_group_stream_entry_points_and_the_plan_are_named_in_one_place():
    pkg = os.path.join(ROOT, "sr-wavenet_amd")
    quoted = re.compile(r"""["'](srwn_residual_group_fwd_stream\w*)["']""")
    named, planned = {}, set()
    for path in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True):
        base, src = os.path.basename(path), open(path).read()
        if base != "_lib.py":      # (the ABI's table of signatures)
            named[base] = set(quoted.findall(src))
        if re.search(r"\bgroup_plan\(", src) and "SRWN_GROUP_LAYERS" in src:
            planned.add(base)
    assert {b for b, n in named.items() if n} == {"stream_stack.py"}
    assert named["stream_stack.py"] == set(NAMES.values())
    assert planned == {"stream_stack.py", "engine.py"}      # engine.py: the training engine's own plan
    ss = open(os.path.join(pkg, "stream_stack.py")).read()
    for name in NAMES.values():
        assert len(re.findall(r"[\"']%s[\"']" % name, ss)) == 1, name
