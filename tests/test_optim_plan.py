"""CPU tests of the training controls (srwn_version() 126): the schedules of ``optim`` against their closed forms, the control
table -- dtype, shape, the last-row rule, the EMA decay column --, every range error before any device work, the models'
refusals, and the C entry ``srwn_adam_step_ctl`` declared, bound, generated and exported, with its argument errors without
a GPU."""
import math
import os
import re

import numpy as np
import pytest

from tests._pkg import ROOT, sub
from tests.opt_reference import ctl_row, ema_reference

E_SHAPE, E_NULL = -2, -3
A = 4096          # a 16-byte aligned stand-in address: nothing is dereferenced on the paths these tests take


def _lib(binding):
    L = sub("_lib")
    if not os.path.exists(L.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("b", os.path.join(ROOT, "sr-wavenet_amd", "build.py"))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m); m.build()
    return L.bind(binding)


def _bare(cls, **attrs):
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


# ---- schedules against closed forms -------------------------------------------------------------------------------------
def test_constant_and_numbers():
    O = sub("optim")
    assert O.constant(3e-4)(0) == O.constant(3e-4)(10 ** 6) == 3e-4
    assert O.as_schedule(2e-3)(7) == 2e-3
    f = lambda step: 1.0 / (1 + step)
    assert O.as_schedule(f) is f


def test_linear_warmup_endpoints():
    O = sub("optim")
    f = O.linear_warmup(1e-3, 4)
    assert f(0) == 1e-3 * 1 / 4 and f(1) == 1e-3 * 2 / 4
    assert f(3) == 1e-3                      # the last warm-up step runs at the full rate
    assert f(4) == 1e-3 and f(1000) == 1e-3  # then: constant
    g = O.linear_warmup(1e-3, 4, then=O.exponential_decay(1e-3, 10, 0.5))
    assert g(3) == 1e-3 and g(4) == 1e-3 and g(14) == 1e-3 * 0.5      # `then` counts from the end of the warm-up
    assert O.linear_warmup(1e-3, 0)(0) == 1e-3
    with pytest.raises(ValueError):
        O.linear_warmup(1e-3, -1)


def test_exponential_decay_and_its_staircase_boundaries():
    O = sub("optim")
    smooth = O.exponential_decay(1e-2, 100, 0.1)
    assert smooth(0) == 1e-2 and smooth(100) == 1e-2 * 0.1 ** 1.0 and smooth(50) == 1e-2 * 0.1 ** 0.5
    stair = O.exponential_decay(1e-2, 100, 0.1, staircase=True)
    assert stair(99) == 1e-2                             # decay_steps - 1: still the first stair
    assert stair(100) == 1e-2 * 0.1                      # decay_steps
    assert stair(101) == 1e-2 * 0.1                      # decay_steps + 1
    assert stair(199) == 1e-2 * 0.1 and stair(200) == 1e-2 * 0.1 ** 2
    with pytest.raises(ValueError):
        O.exponential_decay(1e-2, 0, 0.1)


def test_piecewise_at_each_boundary():
    O = sub("optim")
    f = O.piecewise([2, 5], [1e-2, 1e-3, 1e-4])
    assert [f(i) for i in range(8)] == [1e-2, 1e-2, 1e-2, 1e-3, 1e-3, 1e-3, 1e-4, 1e-4]     # tf: step <= boundary
    with pytest.raises(ValueError):
        O.piecewise([2, 5], [1e-2, 1e-3])
    with pytest.raises(ValueError):
        O.piecewise([5, 2], [1e-2, 1e-3, 1e-4])


def test_cosine_at_start_midpoint_and_end():
    O = sub("optim")
    f = O.cosine(1e-3, 100, floor=1e-5)
    assert f(0) == 1e-3
    assert f(50) == pytest.approx((1e-3 + 1e-5) / 2, rel=1e-15)
    assert f(100) == pytest.approx(1e-5, rel=1e-15) and f(1000) == f(100)
    assert O.cosine(1e-3, 10)(10) == pytest.approx(0.0, abs=1e-19)
    assert f(25) == 1e-5 + (1e-3 - 1e-5) * 0.5 * (1.0 + math.cos(math.pi * 0.25))


def test_parse_schedule():
    O = sub("optim")
    assert O.parse_schedule("constant", 1e-3)(5) == 1e-3
    assert O.parse_schedule("warmup:4", 1e-3)(0) == 1e-3 / 4
    assert O.parse_schedule("exp:100:0.1:staircase", 1e-2)(100) == 1e-2 * 0.1
    assert O.parse_schedule("piecewise:2,5:1e-2,1e-3,1e-4", 0.0)(3) == 1e-3
    assert O.parse_schedule("cosine:100:1e-5", 1e-3)(0) == 1e-3
    for bad in ("linear", "warmup", "exp:100", "cosine:x", "piecewise:1,2:1e-3"):
        with pytest.raises(ValueError):
            O.parse_schedule(bad, 1e-3)


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_ema_decay_at():
    O = sub("optim")
    assert O.ema_decay_at(0.9, 0) == 0.1 and O.ema_decay_at(0.9, 1) == 2.0 / 11.0      # the ramp (1 + t) / (10 + t)
    assert O.ema_decay_at(0.9, 79) == 80.0 / 89.0 < 0.9                                # ... up to where it meets the decay
    for step in (0, 1, 79, 80, 89, 90, 10 ** 6):
        assert O.ema_decay_at(0.9, step) == min(0.9, (1.0 + step) / (10.0 + step)), step
        assert O.ema_decay_at(0.9, step, warmup=False) == 0.9
    for step in (89, 90, 10 ** 6):
        assert O.ema_decay_at(0.9, step) == 0.9


def test_control_table_dtype_shape_and_columns():
    O = sub("optim")
    sched = O.piecewise([1, 3], [1e-2, 1e-3, 1e-4])
    t = O.control_table(sched, 6, ema_decay=0.9)
    assert t.dtype == np.float32 and t.shape == (6, 2) and t.flags["C_CONTIGUOUS"]
    for i in range(6):                                    # float64, rounded once
        assert t[i, 0] == np.float32(sched(i)) and t[i, 1] == np.float32(O.ema_decay_at(0.9, i))
    none = O.control_table(sched, 6)
    assert (none[:, 1] == 0).all() and np.array_equal(none[:, 0], t[:, 0])
    flat = O.control_table(sched, 3, ema_decay=0.9, ema_warmup=False)
    assert (flat[:, 1] == np.float32(0.9)).all()
    long = O.control_table(1e-3, 10 ** 6 + 1, ema_decay=0.9)
    for step in (0, 1, 89, 90, 10 ** 6):
        assert long[step, 1] == np.float32(min(0.9, (1.0 + step) / (10.0 + step))), step
    assert (long[:, 0] == np.float32(1e-3)).all()


def test_steps_beyond_the_horizon_keep_the_last_row():
    O = sub("optim")
    t = O.control_table(O.exponential_decay(1e-2, 2, 0.5), 4)
    assert [ctl_row(step + 1, len(t)) for step in range(7)] == [0, 1, 2, 3, 3, 3, 3]
    assert ctl_row(0, 4) == 0 and ctl_row(1, 1) == 0 and ctl_row(9, 1) == 0
    assert "last row" in O.control_table.__doc__


def test_ema_restatement_on_hand_cases():
    e, th = np.float32([1.0, 0.5, -2.0]), np.float32([0.5, 0.5, 1.0])
    assert ema_reference(e, th, 0.5).tolist() == [0.75, 0.5, -0.5]
    assert ema_reference(e, th, 0.0).tolist() == th.tolist()
    with pytest.raises(AssertionError):
        ema_reference(np.float32([1e-38]), np.float32([0.0]), 0.5)        # p would be subnormal


# ---- range errors before any device work --------------------------------------------------------------------------------
def test_train_controls_range_errors():
    O = sub("optim")
    ok = O.TrainControls(1e-3, 4, clip_norm=1.0, ema_decay=0.999)
    assert ok.features == (True, True) and ok.table().shape == (4, 2)
    assert O.TrainControls(1e-3).features == (False, False) and O.TrainControls(1e-3).horizon == 1
    assert O.TrainControls(0.0, 2).table()[:, 0].tolist() == [0.0, 0.0]                   # lr exactly 0 is allowed
    for kw in (dict(horizon=0), dict(horizon=-3), dict(schedule=-1e-3), dict(schedule=float("nan")),
               dict(schedule=float("inf")), dict(schedule=lambda s: -1.0 if s == 2 else 1.0, horizon=3),
               dict(clip_norm=0.0), dict(clip_norm=-1.0), dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=1.5),
               dict(validate_ema=True)):
        args = dict(schedule=1e-3, horizon=2)
        args.update(kw)
        with pytest.raises(ValueError):
            O.TrainControls(**args)
    with pytest.raises(ValueError):
        O.control_table(1e-3, 0)


def _models():
    M = sub("model")
    return [M.WaveNet, M.WaveNetTeacher, M.WaveNetAutoEncoder, M.ParallelWaveNet, M.SiameseWaveNet]


def test_models_refuse_before_any_device_work():
    M, D = sub("model"), sub("dataset")
    for cls in _models():
        m = _bare(cls)
        with pytest.raises(ValueError, match="no EMA"):
            m.ema_weights()
        with pytest.raises(ValueError):                       # range errors come before the engine is touched
            m.set_training_controls(schedule=1e-3, clip_norm=-1.0)
        with pytest.raises(ValueError):
            m.set_training_controls(schedule=1e-3, ema_decay=1.0)
        with pytest.raises(ValueError):
            m.set_training_controls(validate_ema=True)
        inside = _bare(cls, _in_ema=True)
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            inside.fit(object(), 1)
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            inside.set_training_controls(schedule=1e-3)
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            inside.save_training_state("/nonexistent", 0)
    with pytest.raises(RuntimeError, match="inside ema_weights"):
        _bare(M.WaveNet, _in_ema=True).train(None, None)
    with pytest.raises(RuntimeError, match="inside ema_weights"):
        _bare(M.WaveNetTeacher, _in_ema=True).train(None)
    with pytest.raises(RuntimeError, match="inside ema_weights"):
        _bare(M.WaveNetAutoEncoder, _in_ema=True).train(None)
    with pytest.raises(RuntimeError, match="inside ema_weights"):
        _bare(M.ParallelWaveNet, _in_ema=True).train_fast(None, None, None, None)
    with pytest.raises(RuntimeError, match="inside ema_weights"):
        _bare(M.ParallelWaveNet, _in_ema=True).train(None, None, None, None)
    with pytest.raises(RuntimeError, match="inside ema_weights"):
        _bare(M.SiameseWaveNet, _in_ema=True).train(None, None, None, None)


def test_controls_set_before_the_first_engine_are_kept_for_it():
    M = sub("model")
    m = _bare(M.WaveNet, _primary=None, _cfg=sub("engine").StackConfig(dilations=[1, 2], learning_rate=2e-3))
    c = m.set_training_controls(horizon=3, ema_decay=0.5)
    assert m._controls is c and c.table()[:, 0].tolist() == [np.float32(2e-3)] * 3      # schedule=None: the constructor's rate
    assert m.set_training_controls() is None and m._controls is None


def test_load_training_state_without_a_file(tmp_path):
    M = sub("model")
    assert _bare(M.WaveNet).load_training_state(str(tmp_path)) is False


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_generated():
    L = sub("_lib")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srwn.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "sr-wavenet_amd", "csrc", "srwn_pybind.cpp")).read()
    lib = _lib("ctypes")
    n = "srwn_adam_step_ctl"
    assert re.search(r"\b%s\s*\(" % n, hdr)
    assert n in L.SIGNATURES and 'm.def("%s"' % n in src
    assert hasattr(lib, n)
    assert lib.srwn_version() >= 126
    assert "since srwn_version() 126" in open(os.path.join(ROOT, "include", "srwn.h")).read()


def _ctl(lib, params=A, grads=A, m=A, v=A, ema=A, n=8, step=A, ctl=A, ctl_len=A, cap=4, scale=A, tick=1):
    return lib.srwn_adam_step_ctl(params, grads, m, v, ema, n, step, ctl, ctl_len, cap, 0.9, 0.999, 1e-8, 1.0, scale, tick,
                                  None)


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_argument_errors_do_not_need_a_gpu(binding):
    lib = _lib(binding)
    for name in ("params", "grads", "m", "v", "step", "ctl", "ctl_len"):
        assert _ctl(lib, **{name: None}) == E_NULL, name
        assert b"adam_step_ctl: null" in lib.srwn_last_error()
    assert _ctl(lib, n=-1) == E_SHAPE and b"adam_step_ctl" in lib.srwn_last_error()
    assert _ctl(lib, cap=0) == E_SHAPE and _ctl(lib, cap=-2) == E_SHAPE
    assert _ctl(lib, n=0) == 0                                   # empty work: nothing launched
    assert _ctl(lib, n=0, params=None, ctl=None, ema=None, scale=None) == 0
