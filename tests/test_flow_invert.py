"""CPU tests of student flow inversion (srwn_version() 121): the entry point declared, bound and exported; its argument
errors without a GPU; the rule itself -- a NumPy step-by-step inversion on the fp64 oracle, which is also the reference of
tests/test_gpu_flow_invert.py --; the likelihood formula; every refusal of the host layers before any device work."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import ROOT, sub

# the common inputs of both test files: 7 layers (not a multiple of the kernel's three rotating operand sets), dilation 8
# puts taps before the clip, 6 frames of 16 samples are well past the receptive field
DIL, POOL, T, E, F = [1, 2, 4, 8, 1, 2, 4], 16, 96, 6, 2
SHAPES = [(R, B) for R in (32, 64) for B in (3, 33)]      # 33 streams: two workgroups, one nearly empty


def make_flows(R):
    return [O.init_flow_params(100 + 17 * f, DIL, 2, R, 128, E, bias_scale=0.1) for f in range(F)]


def invert_oracle(flows, audio, cond, pool):
    """The rule, step by step in fp64: from the last flow to the first, x_in[t] = (x_out[t] - p1[t]) * exp(-p0[t]) with
    (p0, p1)[t] from the flow's stack on the samples recovered so far.  The stack's row t is flow_forward's, computed by
    the oracle's own layer routines on the window of rows it reads (a whole-clip pass per step would give the same row
    200 times slower): the entry conv on (x_in[t-2], x_in[t-1]), layer l on its inputs at t - d_l and t, zeros before the
    clip.  test_step_by_step_inversion_recovers_the_noise holds every row to flow_forward's.
    Returns (noise, per flow the recovered input, per flow prm [B, T, 2]), flows in their forward order."""
    y = np.asarray(audio, np.float64)
    B, T_ = y.shape
    xs, prms = [None] * len(flows), [None] * len(flows)
    for f in range(len(flows) - 1, -1, -1):
        p = flows[f]
        R = p.init_b.shape[-1]
        x = np.zeros((B, T_ + 2))                                        # x[:, t + 2] = x_in[t]: two zeros before the clip
        hist = [np.zeros((B, T_ + d, R)) for d in p.dilations]           # hist[l][:, t + d] = layer l's input at t
        prm = np.zeros((B, T_, 2))
        for t in range(T_):
            h = O.dilated_causal_conv1d_bias(O.right_shift(x[:, t:t + 3, None]), p.init_w, p.init_b, 1)[:, -1]
            for l, (lp, d) in enumerate(zip(p.layers, p.dilations)):
                hist[l][:, t + d] = h + (cond[:, t // pool] @ lp.wc + lp.bc)
                h = O.residual_dilation_layer(hist[l][:, t:t + d + 1], lp, d, "reference")[0][:, -1]
            prm[:, t] = np.maximum(h, 0) @ p.head_w2 + p.head_b2
            x[:, t + 2] = (y[:, t] - prm[:, t, 1]) * np.exp(-prm[:, t, 0])
        xs[f], prms[f] = x[:, 2:], prm
        y = x[:, 2:]
    return xs[0], xs, prms


@functools.lru_cache(maxsize=None)
def common(R, B):
    """The common inputs at (R, B) and their fp64 reference, computed once and shared (read-only) by every test."""
    flows = make_flows(R)
    rng = np.random.default_rng(0)
    cond = rng.normal(0, 1, (B, T // POOL, E))
    z = np.clip(rng.logistic(0, 1, (B, T)), -8, 8)
    fw = O.student_forward(flows, z, cond, POOL)
    audio = fw["x_last"]                                   # the unclipped output
    z_rec, xs, prms = invert_oracle(flows, audio, cond, POOL)
    log_scale = np.sum([np.log(s) for s in fw["scales"]], 0)
    nll = -(-z - 2.0 * np.log1p(np.exp(-z))) + log_scale   # -log f(z) of the logistic(0, 1) density f, + sum log scales
    out = dict(flows=flows, cond=cond, z=z, audio=audio, z_rec=z_rec, xs=xs, prms=prms, scales=fw["scales"],
               log_scale=log_scale, nll=nll)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _bare(cls, **attrs):
    """An object without its device state (constructing one needs a GPU): what the refusals check first."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_entry_point_is_exported_by_both_bindings():
    L = sub("_lib")
    assert "srwn_flow_invert" in L.SIGNATURES
    assert "srwn_flow_inv.hip" in sub("build").SOURCES
    assert "srwn_flow_invert" in open(os.path.join(ROOT, "include", "srwn.h")).read()
    for binding in ("pybind11", "ctypes"):
        lib = L.bind(binding)
        assert callable(lib.srwn_flow_invert)
        assert lib.srwn_version() >= 121


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = sub("_lib").bind(binding)
    dil = (C.c_int32 * 3)(1, 2, 4)
    ok = dict(wcr=1, bias_f=1, bias_r=1, init_w=1, init_b=1, flow_w=1, flow_b=1, ring=1, y=1, x_in=1, prm=1, dilations=dil,
              nlayers=3, B=2, Tout=16, nsteps=16, R=64, K=2, cond=1, cond_frames=1, pool=16, cond_ld=64, cond_ls=256,
              dtype=1, stream=None, t0=0, carry=None)

    def run(**kw):
        return lib.srwn_flow_invert(*dict(ok, **kw).values())

    assert run(B=0, wcr=None) == 0 and run(nsteps=0, wcr=None) == 0          # nothing to do, before anything is looked at
    for name in ("wcr", "bias_f", "bias_r", "init_w", "init_b", "flow_w", "flow_b", "ring", "y", "x_in", "dilations", "cond"):
        assert run(**{name: None}) == -3, name
    assert b"flow_invert" in lib.srwn_last_error() and b"null" in lib.srwn_last_error()
    assert run(t0=16, cond_frames=2, carry=None) == -3                        # a resumed launch reads the carry
    # (the encoding covers cond_frames * pool_stride = 16 steps: one more, or a start one later, is past its end)
    for bad in (dict(nsteps=-1), dict(t0=-1), dict(cond_frames=0), dict(t0=1, carry=1), dict(nsteps=17, Tout=17),
                dict(nsteps=17), dict(B=-1), dict(nlayers=0), dict(nlayers=65), dict(cond_ld=32), dict(pool=0),
                dict(cond_ls=-1), dict(dilations=(C.c_int32 * 3)(1, 0, 4))):
        assert run(**bad) == -2, bad
    for bad in (dict(R=48), dict(R=128), dict(K=3), dict(K=1)):
        assert run(**bad) == -4, bad
    assert b"R=64 or 32" in lib.srwn_last_error()
    for bad in (dict(dtype=7), dict(dtype=-1)):
        assert run(**bad) == -1, bad


# ---- the rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,B", SHAPES)
def test_step_by_step_inversion_recovers_the_noise(R, B):
    c = common(R, B)
    assert min(s.min() for s in c["scales"]) < 0.5 and max(s.max() for s in c["scales"]) > 1.5      # not a trivial inverse
    assert np.abs(c["z_rec"] - c["z"]).max() <= 1e-12
    # the recovered input of every flow is the forward pass's, and so are the parameters
    x = c["z"]
    for f, p in enumerate(c["flows"]):
        assert np.abs(c["xs"][f] - x).max() <= 1e-12
        _, _, x, prm = O.flow_forward(p, x, c["cond"], POOL)
        assert np.abs(c["prms"][f] - prm).max() <= 1e-12


@pytest.mark.parametrize("R,B", SHAPES)
def test_nll_formula_is_the_logistic_density_and_the_log_scales(R, B):
    ST = sub("student")
    c = common(R, B)
    z = c["z"]
    dens = np.exp(-z) / (1.0 + np.exp(-z)) ** 2                   # logistic(0, 1), the student's noise (student.py:104)
    want = -np.log(dens) + c["log_scale"]
    got = ST.logistic_nll(torch.tensor(z), torch.tensor(np.sum([p[..., 0] for p in c["prms"]], 0))).numpy()
    assert got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(c["nll"] - want).max() <= 1e-12


# ---- refusals, before any device work ---------------------------------------------------------------------------------
def test_inverter_refuses_first():
    EG = sub("engine"); ST = sub("student")
    cfg = dict(dilations=DIL, dilation_channels=64, skip_channels=128, cond_channels=E, pool_stride=POOL)
    with pytest.raises(NotImplementedError, match="wavenet"):
        ST.FlowInverter(EG.StackConfig(**dict(cfg, gate_mode="wavenet")), F)
    with pytest.raises(NotImplementedError, match="filter_width"):
        ST.FlowInverter(EG.StackConfig(**dict(cfg, filter_width=3)), F)
    with pytest.raises(NotImplementedError, match="32 / 64"):
        ST.FlowInverter(EG.StackConfig(**dict(cfg, dilation_channels=48)), F)
    with pytest.raises(ValueError, match="conditioned"):
        ST.FlowInverter(EG.StackConfig(**dict(cfg, cond_channels=0)), F)
    with pytest.raises(ValueError, match=">= 1"):
        ST.FlowInverter(EG.StackConfig(**cfg), 0)
    inv = _bare(ST.FlowInverter, E=E, max_batch=2, _state=None, _serial=0)
    for bad in (np.zeros((2, E)), np.zeros((2, 3, E + 1)), np.zeros((3, 3, E)), np.zeros((2, 0, E))):
        with pytest.raises(ValueError, match="cond"):
            inv.start(bad)
        with pytest.raises(ValueError, match="cond"):
            inv.invert(np.zeros((2, 48)), bad)
    with pytest.raises(ValueError, match="current"):
        inv.step(ST.InvertState(2, 3, 48, 1, None), np.zeros((2, 4)))


def test_model_faces_refuse_first():
    M = sub("model")
    with pytest.raises(NotImplementedError, match="wavenet"):
        M.StudentInverter(DIL, F, dilation_channels=64, latent_channels=E, pool_stride=POOL, gate_mode="wavenet")
    with pytest.raises(NotImplementedError, match="filter_width"):
        M.StudentInverter(DIL, F, filter_width=3, dilation_channels=64, latent_channels=E, pool_stride=POOL)
    with pytest.raises(NotImplementedError, match="32 / 64"):
        M.StudentInverter.from_checkpoint("/nonexistent", DIL, F, dilation_channels=48, latent_channels=E, pool_stride=POOL)
    hp = dict(dilations=DIL, num_flows=F, dilation_channels=64, skip_channels=128, latent_channels=E - 2, condition_size=2,
              pool_stride=POOL, _name="ParallelWaveNet", max_batch=2, input_size=T)
    for cls in (M.ParallelWaveNet, M.StudentSynthesizer):
        with pytest.raises(NotImplementedError, match="filter_width"):
            _bare(cls, **dict(hp, filter_width=3, _flow_cfg=SimpleNamespace(dtype=torch.float32),
                              _eng=SimpleNamespace(dt=torch.float32, dev="cpu", weights=[]))).inverter()
        with pytest.raises(NotImplementedError, match="32 / 64"):
            _bare(cls, **dict(hp, filter_width=2, dilation_channels=48, _flow_cfg=SimpleNamespace(dtype=torch.float32),
                              _eng=SimpleNamespace(dt=torch.float32, dev="cpu", weights=[]))).inverter()
    inv = _bare(M.StudentInverter, latent_channels=E - 2, condition_size=2, pool_stride=POOL, max_batch=2)
    y = np.zeros((2, 2), np.float32)
    for call in (inv.invert, inv.log_likelihood):
        with pytest.raises(ValueError, match="encoding"):
            call(np.zeros((2, 48)), np.zeros((2, E - 2)), y)                   # rank 2
        with pytest.raises(ValueError, match="encoding"):
            call(np.zeros((2, 48)), np.zeros((2, 3, E)), y)                    # the channels of encoding_w_condition
        with pytest.raises(ValueError, match="max_batch"):
            call(np.zeros((3, 48)), np.zeros((3, 3, E - 2)), np.zeros((3, 2)))
        with pytest.raises(ValueError, match="conditions"):
            call(np.zeros((2, 48)), np.zeros((2, 3, E - 2)))
        with pytest.raises(ValueError, match="audio"):
            call(np.zeros((2, 47)), np.zeros((2, 3, E - 2)), y)                # T = frames * pool_stride
    with pytest.raises(ValueError, match="encoding"):
        inv.stream(np.zeros((2, E - 2)), y)
