"""CPU test of the one launch routine of teacher generation (WaveNetEngine._launch_generation): for every head, body, form
and with or without sampling controls it names the expected general entry point of the C ABI with an argument list of that
entry point's length and kinds, and no other code of the package names a generator entry point."""
import ctypes as C
import glob
import itertools
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests._pkg import ROOT, sub

L, R, S, KW, B, NSTEPS = 2, 64, 256, 2, 3, 5
EIGHT = ["srwn_generate%s%s_%s_sampled" % (b, h, f) for b in ("", "16") for h in ("", "_mol") for f in ("resume", "slots")]


def _bare_engine(mol):
    """An engine without its device state (constructing one needs a GPU): what the launch routine reads."""
    EG = sub("engine")
    Cc = 20 if mol else 256
    shapes = {"BF": (L, R), "BR": (L, R), "head_b1": (S,), "head_b2": (256,), "init_w": (KW, 1, R), "init_b": (R,)}
    sections, off = {}, 0
    for name, shp in shapes.items():
        sections[name] = EG.Section(name, off, shp)
        off += sections[name].numel
    e = object.__new__(EG.WaveNetEngine)
    attrs = dict(sections=sections, params=torch.zeros(off), packed=torch.zeros(4096, dtype=torch.bfloat16),
                 bs_sum=torch.zeros(S), o_gen=0, o_skip_gen=256, o_w1=512, o_w2=768, o_g16=1024, o_g16_h1=1280,
                 o_g16_h2=1536, dil=[1, 2], L=L, R=R, S=S, C=Cc, Kw=KW, E=0, mol=mol, dt=torch.bfloat16, dev="cpu",
                 cfg=SimpleNamespace(pool_stride=4, head_mode="mol" if mol else "per_timestep"))
    for k, v in attrs.items():
        setattr(e, k, v)
    return e


@pytest.mark.parametrize("mol,g16,slots,sampled", list(itertools.product([False, True], repeat=4)))
def test_launch_names_one_general_form_with_its_argument_list(monkeypatch, mol, g16, slots, sampled):
    LIB = sub("_lib")
    calls = []
    monkeypatch.setattr(LIB, "call", lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: SimpleNamespace(cuda_stream=0))
    monkeypatch.setenv("SRWN_GEN16", "1" if g16 else "0")
    e = _bare_engine(mol)
    ring, audio, codes = torch.zeros(8), torch.zeros((B, NSTEPS)), torch.zeros((B, NSTEPS), dtype=torch.int32)
    carry = torch.zeros((B, 2))
    table = torch.zeros((B, 4), dtype=torch.int32) if slots else None
    samp = torch.zeros((B, 4), dtype=torch.int32) if sampled else None
    e._launch_generation(ring, audio, codes, None, None, B, NSTEPS, "sample", 7, 11, carry, samp, None, 0, table)
    assert len(calls) == 1
    name, args = calls[0]
    assert name == "srwn_generate%s%s_%s_sampled" % ("16" if g16 else "", "_mol" if mol else "",
                                                     "slots" if slots else "resume")
    assert name in LIB.SIGNATURES
    kinds = LIB.SIGNATURES[name][1]
    assert len(args) == len(kinds)
    # what both bindings can pass: None, an address or a ctypes array for a pointer, a plain int for a number
    for i, (a, k) in enumerate(zip(args, kinds)):
        if k is LIB._p:
            assert a is None or isinstance(a, (int, C.Array)), (i, a)
        else:
            assert isinstance(a, int) and not isinstance(a, bool), (i, a)
    assert (args[-1] is None) == (not sampled)
    if sampled:
        assert args[-1] == samp.data_ptr()
    # the shape block after the pointers: nlayers, B, Tout, nsteps, R, S; then C (softmax) or [K,] num_mixtures (mol)
    first = [i for i, k in enumerate(kinds) if k is not LIB._p][0]
    assert first == (16 if g16 else 17) and list(args[first - 1]) == [1, 2]
    assert args[first:first + 6] == (L, B, NSTEPS, NSTEPS, R, S)
    assert args[first + 6:first + 8] == {(False, False): (256, KW), (False, True): (256, 1),
                                         (True, False): (KW, 5), (True, True): (5, None)}[(mol, g16)]
    # the tail: t0 (the pool's clock), carry, [slots,] sampling
    want = [11, carry.data_ptr()] + ([table.data_ptr()] if slots else [])
    assert list(args[-1 - len(want):-1]) == want


def test_generator_entry_points_are_named_in_one_place():
    pkg = os.path.join(ROOT, "sr-wavenet_amd")
    calls = (re.compile(r"\b(srwn_generate\w*)\s*\("), re.compile(r"""call\(\s*["'](srwn_generate\w*)"""))
    helpers = {"srwn_generate_ring_elems", "srwn_generate_ring_fill", "srwn_generate_ring_fill_slots",
               "srwn_generate16_image_elems"}
    for path in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True):
        if os.path.basename(path) in ("engine.py", "_lib.py"):
            continue
        src = open(path).read()
        hits = {n for rx in calls for n in rx.findall(src)} - helpers
        assert not hits, (path, hits)
    eng = open(os.path.join(pkg, "engine.py")).read()
    for name in EIGHT:
        assert len(re.findall(r"\b%s\b" % name, eng)) <= 1, name
    # ... and nothing but the launch routine's table of the eight, and the ring helpers, in engine.py
    named = set(re.findall(r"[\"'](srwn_generate\w*)[\"']", eng))
    assert named == set(EIGHT) | {"srwn_generate_ring_fill", "srwn_generate_ring_fill_slots"}
