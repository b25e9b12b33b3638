"""CPU tests of the canonical WaveNet gate option (gate_mode "wavenet"): the library exports its two layer kernels through
both bindings, their argument errors come back as negative codes before any launch, and a bad configuration is refused
before anything touches a device."""
import pytest

from tests._pkg import sub

X = 1      # any non-null "device pointer": every call below fails its argument checks first


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_wavenet_layer_entry_points_are_exported(binding):
    L = sub("_lib")
    lib = L.bind(binding)
    for n in ("srwn_wavenet_layer_fwd", "srwn_wavenet_layer_bwd"):
        assert n in L.SIGNATURES
        assert callable(getattr(lib, n))
    assert lib.srwn_version() >= 102


def _fwd(lib, *, x=X, wg_bias=X, B=2, T=64, R=64, K=2, d=1, cond=None, frames=1, pool=1, cstride=64, dtype=1):
    return lib.srwn_wavenet_layer_fwd(x, cond, X, X, X, wg_bias, X, X, X, X, X, B, T, R, K, d, frames, pool, cstride,
                                      dtype, None)


def _bwd(lib, *, g_in=None, d_up=X, wT=X, g_out=X, wresT=X, wskipT=None, dtotal=None, dcs=X, z=X, s=X, d_out=X, B=2,
         T=64, R=64, S=256, K=2, d=1, up=1, down=1, dtype=1):
    return lib.srwn_wavenet_layer_bwd(g_in, d_up, wT, g_out, wresT, wskipT, dtotal, dcs, z, s, d_out, B, T, R, S, K, d,
                                      up, down, dtype, None)


@pytest.mark.parametrize("binding", ["pybind11", "ctypes"])
def test_wavenet_layer_argument_errors_do_not_need_a_gpu(binding):
    lib = sub("_lib").bind(binding)
    # forward
    assert _fwd(lib, x=None) == -3 and b"null" in lib.srwn_last_error()
    assert _fwd(lib, wg_bias=None) == -3                       # the gate bias is required
    assert _fwd(lib, x=None, B=0) == -3                        # (null pointers are refused even for empty work)
    assert _fwd(lib, B=-1) == -2
    assert _fwd(lib, d=0) == -2
    assert _fwd(lib, cond=X, frames=1, pool=16, T=64) == -2   # 1 frame x 16 < 64 steps
    assert _fwd(lib, cond=X, frames=4, pool=16, cstride=12) == -2
    assert _fwd(lib, K=3) == -4
    assert _fwd(lib, R=48) == -4
    assert _fwd(lib, dtype=7) == -1
    assert _fwd(lib, B=0) == 0 and _fwd(lib, T=0) == 0         # empty work: nothing launched
    # backward
    assert _bwd(lib, up=0, down=0) == -2
    assert _bwd(lib, up=2) == -2
    assert _bwd(lib, d_up=None) == -3
    assert _bwd(lib, s=None) == -3                             # DOWN needs the stored gate
    assert _bwd(lib, dcs=None) == -3                           # ... and dcs, or wskipT + dtotal
    assert _bwd(lib, wresT=None) == -3
    assert _bwd(lib, dcs=None, wskipT=X, dtotal=X, S=24) == -2
    assert _bwd(lib, d=0) == -2
    assert _bwd(lib, K=3) == -4
    assert _bwd(lib, R=96) == -4
    assert _bwd(lib, dtype=5) == -1
    assert _bwd(lib, B=0) == 0


def test_stack_config_default_is_the_reference_gate():
    EG = sub("engine")
    assert EG.StackConfig(dilations=[1, 2]).gate_mode == "reference"


def test_bad_gate_mode_is_refused_before_any_device_work():
    EG = sub("engine")
    cfg = EG.StackConfig(dilations=[1, 2], dilation_channels=64, gate_mode="canonical")
    with pytest.raises(ValueError, match="gate_mode"):
        EG.WaveNetEngine(cfg, 2, 64, device="cuda")
    flow = EG.StackConfig(dilations=[1, 2], dilation_channels=64, head_mode="flow", gate_mode="wavenet")
    with pytest.raises(NotImplementedError, match="wavenet"):
        EG.WaveNetEngine(flow, 2, 64, device="cuda")


def test_model_classes_validate_gate_mode_first():
    M = sub("model")
    with pytest.raises(ValueError, match="gate_mode"):
        M.WaveNetTeacher(256, 0, [1, 2], gate_mode="gated")
    with pytest.raises(TypeError):            # keyword-only: the positional signature of the reference is unchanged
        M.WaveNetTeacher(256, 0, [1, 2], 2, 32, 256, 256, 16, 512, "T", 1e-3, False, None, 0, "softmax", 5, "wavenet")
