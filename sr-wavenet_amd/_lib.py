"""Python binding of libsrwn.so (the C-ABI declared in include/srwn.h).

Two interchangeable bindings of the SAME library and symbol table: the pybind11 module ``_srwn_pyb`` that build.py
generates from SIGNATURES and compiles against the header's prototypes (default: the binding north_star names), and
plain ctypes (``SRWN_BINDING=ctypes``).  Callers pass the same arguments to either -- integers for device pointers,
None for null, ctypes arrays / byref() for the few host arrays.

The product path has NO fallback: if the HIP library is missing or a symbol is absent the import
fails loudly, and every call raises RuntimeError on a non-zero return code.
"""
from __future__ import annotations

import ctypes as C
import numbers
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsrwn.so")
# A/B measurements of kernel variants on one box: another build of the same library (ctypes binding, no manifest check)
_ALT_LIB = os.environ.get("SRWN_LIB_PATH")
if _ALT_LIB:
    LIB_PATH = _ALT_LIB

F32, BF16 = 0, 1
PRO_NONE, PRO_GATE = 0, 1
EPI_NONE, EPI_RELU, EPI_MASK, EPI_F32 = 0, 1, 2, 4

_p, _i32, _i64, _f32, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double


class SrwnGenSlot(C.Structure):
    """Mirror of srwn.h's SrwnGenSlot (16 bytes): one slot of a generation pool, passed to the *_slots entry points as a
    device array."""
    _fields_ = [("t", C.c_int32), ("t_end", C.c_int32), ("seed", C.c_uint64)]


class SrwnSynthSlot(C.Structure):
    """Mirror of srwn.h's SrwnSynthSlot (16 bytes): one slot of a student synthesis pool -- its own absolute time and its
    stream's end -- passed to the synthesis *_slots entry points as a device array."""
    _fields_ = [("t", C.c_int64), ("t_end", C.c_int64)]


class SrwnEncFrame(C.Structure):
    """Mirror of srwn.h's SrwnEncFrame (16 bytes): one frame of a launch of srwn_nc_encode_frame_list, passed as a device
    array -- the row of the audio ring, the ring column of the frame's first sample and the real samples from there on."""
    _fields_ = [("stream", C.c_int32), ("col", C.c_int32), ("valid", C.c_int32), ("reserved", C.c_int32)]


class SrwnGenSampling(C.Structure):
    """Mirror of srwn.h's SrwnGenSampling (16 bytes): one utterance's (or pool slot's) sampling controls, passed to the
    *_sampled entry points and to srwn_sample_filtered as a device array.  The defaults (1, 1, 0) mean "off"."""
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32), ("reserved", C.c_int32)]


# name -> (restype, argtypes); must list every symbol of include/srwn.h (checked by tests/test_abi.py)
SAMPLED = ["srwn_generate_resume", "srwn_generate_mol_resume", "srwn_generate16_resume", "srwn_generate16_mol_resume",
           "srwn_generate_slots", "srwn_generate_mol_slots", "srwn_generate16_slots", "srwn_generate16_mol_slots"]

SIGNATURES = {
    "srwn_version": (C.c_int, []),
    "srwn_last_error": (C.c_char_p, []),
    "srwn_mu_law_encode": (C.c_int, [_p, _p, _i64, _i32, _p]),
    "srwn_mu_law_decode": (C.c_int, [_p, _p, _i64, _i32, _p]),
    "srwn_pack_a_index": (C.c_int, [_p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_pack_gather": (C.c_int, [_p, _p, _p, _i64, _i32, _p]),
    "srwn_pack_gather_rowsum": (C.c_int, [_p, _p, _p, _i64, _i32, _p, _i32, _i32, _p, _p]),
    "srwn_causal_conv1d_fwd": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_init_conv_wgrad_partials": (_i64, [_i32, _i32, _i32, _i32]),
    "srwn_init_conv_wgrad": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_residual_layer_fwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                          _i32, _i32, _p]),
    "srwn_residual_group_fwd": (C.c_int, [_p, _p, _p, _i64, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p, _i32, _i32, _i32,
                                          _i32, _i32, _i32, _i32, _p]),
    "srwn_residual_group_bwd": (C.c_int, [_p, _p, _p, _p, _p, _i64, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_group_wt_geometry": (C.c_int, [_p, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p]),
    "srwn_residual_group_fwd_wt": (C.c_int, [_p, _p, _p, _i64, _p, _p, _i64, _i32, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p,
                                             _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_residual_group_fwd_ic": (C.c_int, [_p, _p, _p, _i32, _p, _p, _i64, _p, _p, _i64, _i32, _p, _p, _p, _p, _p, _i32,
                                             _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_residual_group_bwd_wt": (C.c_int, [_p, _p, _i32, _p, _p, _i64, _p, _p, _i64, _p, _p, _p, _i32, _p, _p, _p, _p,
                                             _i32, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_debug_stamp_buffer": (C.c_int, [_p]),
    "srwn_group_plan_auto": (_i32, [_p, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_log_softmax": (C.c_int, [_p, _p, _p, _i64, _i32, _p]),
    "srwn_categorical_sample": (C.c_int, [_p, _p, _i64, _i32, C.c_uint64, _p]),
    "srwn_probs_logistic": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _f32, _p]),
    "srwn_tanh_gate": (C.c_int, [_p, _p, _p, _i64, _p]),
    "srwn_gated_activation": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _p]),
    "srwn_residual_combine": (C.c_int, [_p, _i32, _p, _i32, _p, _i64, _p]),
    "srwn_relu": (C.c_int, [_p, _p, _i64, _p]),
    "srwn_mol_nll_rows": (C.c_int, [_p, _i64, _p, _i32, _p, _i64, _p]),
    "srwn_group_plan": (_i32, [_p, _i32, _i32, _i32, _p]),
    "srwn_pw_linear_ychunks": (C.c_int, [_p, _i64, _i32, _p, _p, _p, _i64, _i32, _i64, _i32, _i32, _i64, _i32, _p]),
    "srwn_pw_linear": (C.c_int, [_p, _i64, _i64, _i32, _i32, _p, _p, _p, _i64, _i32, _i32, _i64, _p, _i64, _i32,
                                 _i32, _i32, _p]),
    "srwn_pw_linear_ksplit": (C.c_int, [_p, _i64, _i64, _i32, _i32, _p, _p, _p, _i64, _i32, _i32, _i64, _i32, _i32, _p]),
    "srwn_softmax_ce_partials": (_i64, [_i64]),
    "srwn_head_softmax_ce": (C.c_int, [_p, _i64, _i32, _p, _p, _p, _p, _p, _p, _i32, _i32, _i64, _f32, _i32, _p]),
    "srwn_reduce_loss": (C.c_int, [_p, _i64, _f32, _p, _p]),
    "srwn_head_chain": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i64, _f32,
                                  _i32, _p]),
    "srwn_residual_layer_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32,
                                          _i32, _i32, _i32, _p]),
    "srwn_wgrad_slabs": (_i32, [_i64]),
    "srwn_wgrad": (C.c_int, [_p, _i64, _i32, _p, _i64, _i32, _p, _i64, _i32, _i32, _i32, _p, _i32, _p, _p, _i64,
                             _i32, _i32, _i32, _i32, _p]),
    "srwn_reduce_partials": (C.c_int, [_p, _i32, _i64, _i32, _i32, _f32, _p, _i64, _p]),
    "srwn_reduce_partials_multi": (C.c_int, [_p, _i32, _p]),
    "srwn_add_frame_bias": (C.c_int, [_p, _p, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_frame_sum": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_frame_sum_batched": (C.c_int, [_p, _i64, _p, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _p]),
    "srwn_adam_step": (C.c_int, [_p, _p, _p, _p, _i64, _p, _f32, _f32, _f32, _f32, _f32, _p]),
    "srwn_time_mean_slabs": (_i32, [_i32]),
    "srwn_time_mean": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _p]),
    "srwn_pooled_head": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _p]),
    "srwn_bcast_mask": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _f32, _i32, _p]),
    "srwn_contrastive_head": (C.c_int, [_p, _p, _p, _p, _f32, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _p]),
    "srwn_wavenet_layer_fwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32,
                                         _i32, _i32, _i32, _p]),
    "srwn_wavenet_layer_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32,
                                         _i32, _i32, _i32, _p]),
    "srwn_skip_dgrad_all": (C.c_int, [_p, _p, _p, _i64, _i32, _i64, _i32, _i32, _i32, _p]),
    "srwn_wgrad_layers": (C.c_int, [_p, _p, _p, _p, _i64, _p, _i64, _i32, _i32, _i32, _p, _i32, _p, _p, _p, _p, _i64,
                                    _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_wgrad_skip_wt_slabs": (_i32, [_p, _p, _i32, _i32]),
    "srwn_wgrad_skip_wt": (C.c_int, [_p, _i64, _p, _p, _i32, _p, _i64, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_generate_ring_elems": (_i64, [_p, _i32, _i32]),
    "srwn_generate": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32,
                                _i32, _i32, _i32, _i32, _i32, _i32, C.c_uint64, _i32, _p]),
    "srwn_generate16_image_elems": (_i64, [_i32, _i32, _i32, _i32]),
    "srwn_generate16": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32,
                                  _i32, _i32, _i32, _i32, C.c_uint64, _p]),
    "srwn_generate16_mol": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32,
                                      _i32, _i32, _i32, _i32, _p, _i32, _i32, _i64, _i32, C.c_uint64, _p]),
    "srwn_generate_mol": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32,
                                    _i32, _i32, _i32, _i32, _i32, _p, _i32, _i32, _i64, _i32, C.c_uint64, _i32, _p]),
    "srwn_generate_resume": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32,
                                       _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.c_uint64, _i32, _p, _i32, _p]),
    "srwn_generate_mol_resume": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32,
                                           _i32, _i32, _i32, _i32, _i32, _i32, _p, _i32, _i32, _i64, _i32, C.c_uint64,
                                           _i32, _p, _i32, _p]),
    "srwn_generate16_resume": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32,
                                         _i32, _i32, _i32, _i32, _i32, _i32, C.c_uint64, _p, _i32, _p]),
    "srwn_generate16_mol_resume": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32,
                                             _i32, _i32, _i32, _i32, _i32, _p, _i32, _i32, _i64, _i32, C.c_uint64, _p,
                                             _i32, _p]),
    "srwn_generate_ring_fill": (C.c_int, [_p, _i64, _i32, _i32, _p, _i32, _i32, _i32, _p, _i32, _p]),
    # generation pools: each *_slots is its *_resume twin without the seed, (clock, carry, slots) for (t0, carry)
    "srwn_generate_slots": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32,
                                      _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _i32, _p, _p]),
    "srwn_generate_mol_slots": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32,
                                          _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _i32, _i32, _i64, _i32, _i32, _p,
                                          _i32, _p, _p]),
    "srwn_generate16_slots": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32,
                                        _i32, _i32, _i32, _i32, _i32, _i32, _p, _i32, _p, _p]),
    "srwn_generate16_mol_slots": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32,
                                            _i32, _i32, _i32, _i32, _i32, _p, _i32, _i32, _i64, _i32, _p, _i32, _p, _p]),
    "srwn_generate_ring_fill_slots": (C.c_int, [_p, _i64, _i32, _i32, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _i32, _p]),
    "srwn_sample_filtered": (C.c_int, [_p, _i64, _p, _p, _p, _i64, _i32, _p]),
    "srwn_mol_loss": (C.c_int, [_p, _i64, _p, _i32, _p, _p, _i64, _i64, _f32, _i32, _p]),
    "srwn_wgrad256_slabs": (_i32, [_i64, _i32]),
    "srwn_wgrad256": (C.c_int, [_p, _i64, _i64, _i32, _p, _i64, _p, _p, _i64, _i32, _i32, _i32, _p]),
    "srwn_wgrad_wide_slabs": (_i32, [_i64, _i32, _i32]),
    "srwn_wgrad_wide_pair": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _i32, _i64, _i32, _i64, _i32, _i32,
                                       _i32, _p]),
    "srwn_wgrad_wide": (C.c_int, [_p, _i64, _i64, _i32, _i32, _p, _i64, _i32, _p, _p, _i64, _i32, _i32, _i32, _p]),
    "srwn_tap_linear": (C.c_int, [_p, _i64, _i32, _i32, _i32, _i32, _p, _p, _p, _i64, _i32, _i64, _p, _i64, _p, _i64,
                                  _i32, _i32, _f32, _i32, _i32, _p]),
    "srwn_wgrad_nc_layers": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_nc_input_fwd": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_nc_layer_fwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_nc_mask_words": (_i64, [_i32, _i32]),
    "srwn_nc_mask_bits": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _p]),
    "srwn_nc_layer_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _f32, _p, _p, _i32, _i32, _i32, _i32,
                                    _i32, _p]),
    # the encoder for inference (srwn_version() 109)
    "srwn_nc_encode_max_layers": (_i32, []),
    "srwn_nc_encode_partials": (_i64, [_i32, _i32, _i32, _i32]),
    "srwn_nc_encode_frames": (C.c_int, [_p, _i64, _p, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p, _p, _i32, _i32, _i32, _i32,
                                        _i32, _i32, _i32, _i32, _p]),
    # encoder pools (srwn_version() 111): the chain over a device list of SrwnEncFrame, audio from a ring per stream
    "srwn_nc_encode_list_partials": (_i64, [_i32, _i32, _i32]),
    "srwn_nc_encode_frame_list": (C.c_int, [_p, _i32, _i32, _p, _i32, _p, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p, _p,
                                            _i32, _i32, _i32, _i32, _i32, _p]),
    "srwn_audio_ring_put": (C.c_int, [_p, _i32, _i32, _p, _p, _p, _p, _p, _i32, _i32, _p]),
    "srwn_small_gemm": (C.c_int, [_p, _i64, _i32, _i64, _i32, _p, _i64, _i64, _i32, _i64, _p, _p, _i64, _i32, _i32,
                                  _i32, _i32, _i32, _p]),
    "srwn_small_wgrad": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _i32, _i32, _i32, _f32, _p]),
    "srwn_mol_sample": (C.c_int, [_p, _i64, _i32, _p, _p, _p, _i64, _p]),
    "srwn_mol_loss_dx": (C.c_int, [_p, _i64, _p, _i32, _p, _p, _i64, _f32, _p]),
    "srwn_clamp": (C.c_int, [_p, _p, _i64, _f32, _f32, _p]),
    "srwn_clamp_bwd": (C.c_int, [_p, _p, _p, _i64, _f32, _f32, _p]),
    "srwn_flow_partials": (_i64, [_i64]),
    "srwn_flow_affine_fwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p]),
    "srwn_flow_affine_bwd": (C.c_int, [_p, _p, _p, _p, _p, _f32, _p, _p, _p, _i64, _i32, _i32, _p]),
    # chunked synthesis with the student (srwn_version() 107)
    "srwn_flow_stream_in": (C.c_int, [_p, _i64, _p, _p, _p, _p, _i32, _i32, _i64, _p, _i64, _i32, _i32, _i32, _i32, _i32,
                                      _i32, _p, _p]),
    "srwn_residual_group_fwd_stream": (C.c_int, [_p, _i64, _p, _i64, _i32, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p, _i32,
                                                 _i32, _i32, _i32, _i32, _i32, _i32, _p, _p]),
    "srwn_flow_stream_out": (C.c_int, [_p, _i64, _p, _p, _p, _p, _i64, _p, _i32, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p,
                                       _i32, _p]),
    "srwn_logistic_noise": (C.c_int, [_p, _i64, _p, _p, _p, _i32, _i32, _p]),
    "srwn_logistic_from_bits": (C.c_int, [_p, _p, _i64, _p]),
    # student synthesis pools (srwn_version() 108): the slot forms take the device table of SrwnSynthSlot for the clock
    "srwn_logistic_noise_slots": (C.c_int, [_p, _i64, _p, _p, _p, _i32, _i32, _p]),
    "srwn_flow_stream_in_slots": (C.c_int, [_p, _i64, _p, _p, _p, _p, _i32, _i32, _i64, _p, _i64, _i32, _i32, _i32, _i32,
                                            _i32, _i32, _p, _p]),
    "srwn_residual_group_fwd_stream_slots": (C.c_int, [_p, _i64, _p, _i64, _i32, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p,
                                                       _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p]),
    "srwn_flow_stream_out_slots": (C.c_int, [_p, _i64, _p, _p, _p, _p, _i64, _p, _i32, _p, _i32, _i32, _i32, _i32, _i32,
                                             _i32, _p, _p, _i32, _p]),
    "srwn_flow_stream_reset_slots": (C.c_int, [_p, _i32, _p, _i32, _i64, _p, _i32, _i32, _i32, _i32, _p]),
    # live synthesis (srwn_version() 110): new frames of running streams into the ring conditioning table of one flow
    "srwn_cond_ring_feed": (C.c_int, [_p, _i64, _i64, _i32, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _i32, _i32,
                                      _i32, _p]),
    "srwn_causal_conv1d_dgrad": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _p]),
    "srwn_stft_frames": (_i32, [_i32]),
    "srwn_stft_power": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _p]),
    "srwn_power_loss": (C.c_int, [_p, _p, _i64, _f32, _f32, _p, _p, _p]),
    "srwn_stft_power_bwd": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _p]),
    "srwn_axpy_dev": (C.c_int, [_p, _p, _p, _f32, _i64, _p]),
    "srwn_sumsq_partials": (_i64, [_i64]),
    "srwn_sumsq": (C.c_int, [_p, _i64, _p, _p]),
    "srwn_clip_scale": (C.c_int, [_p, _i64, _f32, _f32, _p, _p]),
    "srwn_adam_step_scaled": (C.c_int, [_p, _p, _p, _p, _i64, _p, _f32, _f32, _f32, _f32, _p, _i32, _p]),
}

# sampling controls: each *_sampled entry point is the call it is named after plus the device array of SrwnGenSampling
for _n in SAMPLED:
    SIGNATURES[_n + "_sampled"] = (SIGNATURES[_n][0], SIGNATURES[_n][1] + [_p])
del _n
# live autoregressive decoding (srwn_version() 112): the *_mol_resume_sampled twins over a ring conditioning table, and the
# feed's scatter of projected frames into it
for _n in ("srwn_generate", "srwn_generate16"):
    SIGNATURES[_n + "_mol_live_sampled"] = SIGNATURES[_n + "_mol_resume_sampled"]
del _n
SIGNATURES["srwn_cond_ring_scatter"] = (C.c_int, [_p, _i64, _p, _i64, _i32, _i32, _i64, _i32, _i32, _i32, _p])
# streaming classifier (srwn_version() 113): the stream entry, the z-storing stream group, the pooled head of a chunk of
# hops and its parity twin, the window mean and the roll
SIGNATURES["srwn_recog_stream_in"] = (C.c_int, [_p, _i64, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p])
SIGNATURES["srwn_residual_group_fwd_stream_z"] = (C.c_int, [_p, _i64, _p, _i64, _i32, _p, _i64, _p, _p, _p, _p, _p, _i32, _i32,
                                                            _i32, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p])
SIGNATURES["srwn_pooled_stream_head"] = (C.c_int, [_p, _i64, _i64, _i32, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _i32,
                                                   _i32, _i32, _i32, _p])
SIGNATURES["srwn_hop_sum"] = (C.c_int, [_p, _i64, _p, _i32, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p])
SIGNATURES["srwn_window_mean"] = (C.c_int, [_p, _i32, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _i32, _i32, _p])
SIGNATURES["srwn_recog_roll"] = (C.c_int, [_p, _i32, _p, _i64, _p, _p, _i32, _i32, _i32, _i32, _i32, _p])

# live slots in generation pools (srwn_version() 114): the *_mol_slots_sampled twins over per-slot conditioning rings, the
# rotation of resuming slots' layer-ring columns and the feed's scatter by a device list of table rows
for _n in ("srwn_generate", "srwn_generate16"):
    SIGNATURES[_n + "_mol_live_slots_sampled"] = SIGNATURES[_n + "_mol_slots_sampled"]
del _n
SIGNATURES["srwn_generate_ring_rotate_slots"] = (C.c_int, [_p, _p, _i32, _i32, _i32, _p, _p, _i32, _i32, _p])
SIGNATURES["srwn_cond_ring_scatter_slots"] = (C.c_int, [_p, _i64, _p, _i64, _i32, _p, _i32, _i32, _i32, _p])
# classifier pools (srwn_version() 115): the slot forms of the streaming classifier's launches, on the device table of
# SrwnSynthSlot for the clock; the stream entry reads the pool's audio ring and there is no carry
SIGNATURES["srwn_recog_stream_in_slots"] = (C.c_int, [_p, _i32, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p])
SIGNATURES["srwn_residual_group_fwd_stream_z_slots"] = SIGNATURES["srwn_residual_group_fwd_stream_z"]
SIGNATURES["srwn_pooled_stream_head_slots"] = SIGNATURES["srwn_pooled_stream_head"]
SIGNATURES["srwn_hop_sum_slots"] = SIGNATURES["srwn_hop_sum"]
SIGNATURES["srwn_window_mean_slots"] = SIGNATURES["srwn_window_mean"]
SIGNATURES["srwn_recog_roll_slots"] = (C.c_int, [_p, _i32, _p, _i32, _i32, _i32, _i32, _i32, _p])
# streaming likelihood scorer (srwn_version() 116): the one-launch score head over the stored z and its parity twin's
# last step
SIGNATURES["srwn_stream_score_head"] = (C.c_int, [_p, _i64, _i64, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i32,
                                                  _i32, _i32, _i32, _i32, _i32, _i32, _p])
SIGNATURES["srwn_nll_rows"] = (C.c_int, [_p, _i64, _i64, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _p])
# its mixture-of-logistics form (srwn_version() 117): the target audio [B][x_stride] in the place of the codes, no `best`
SIGNATURES["srwn_stream_mol_score_head"] = (C.c_int, [_p, _i64, _i64, _i32, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _i64,
                                                      _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p])
SIGNATURES["srwn_mol_score_rows"] = (C.c_int, [_p, _i64, _i64, _p, _i64, _p, _p, _i64, _i32, _i32, _i32, _p])
# scorer pools (srwn_version() 118): the pool's entry (first stack row and target codes from the audio ring, one launch) and
# the slot forms of the softmax score head and of its twin's last step: the table of SrwnSynthSlot in front of the stream
SIGNATURES["srwn_score_stream_in_slots"] = (C.c_int, [_p, _i32, _p, _p, _p, _i64, _i32, _p, _i64, _i32, _i32, _i32, _i32, _i32,
                                                      _i32, _p, _p])
SIGNATURES["srwn_stream_score_head_slots"] = (C.c_int, SIGNATURES["srwn_stream_score_head"][1][:-1] + [_p, _p])
SIGNATURES["srwn_nll_rows_slots"] = (C.c_int, SIGNATURES["srwn_nll_rows"][1][:-1] + [_p, _p])
# mixture-of-logistics scorer pools (srwn_version() 119): the pool's entry (first stack row with its conditioning bias and
# the target samples from the audio ring, one launch) and the slot forms of the mixture head and of its twin's last step
SIGNATURES["srwn_mol_score_stream_in_slots"] = (C.c_int, [_p, _i32, _p, _p, _p, _i32, _i32, _i64, _p, _i64, _i32, _p, _i64,
                                                          _i32, _i32, _i32, _i32, _i32, _p, _p])
SIGNATURES["srwn_stream_mol_score_head_slots"] = (C.c_int, SIGNATURES["srwn_stream_mol_score_head"][1][:-1] + [_p, _p])
SIGNATURES["srwn_mol_score_rows_slots"] = (C.c_int, SIGNATURES["srwn_mol_score_rows"][1][:-1] + [_p, _p])

# streaming embedder (srwn_version() 120): window mean, embedding, gallery distances and the nearest row in one launch, its
# slot form on the pool's table, and the twin's last step (the distances and the nearest row of embeddings that are there)
SIGNATURES["srwn_window_embed_match"] = (C.c_int, [_p, _i32, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _i32, _i32, _p, _p, _i32,
                                                   _p, _p, _p, _p, _p])
SIGNATURES["srwn_window_embed_match_slots"] = SIGNATURES["srwn_window_embed_match"]
SIGNATURES["srwn_gallery_match"] = (C.c_int, [_p, _i32, _i32, _p, _p, _i32, _p, _p, _p, _p])
# student flow inversion (srwn_version() 121): one flow run backwards over [t0, t0 + nsteps), in the resume form
SIGNATURES["srwn_flow_invert"] = (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32,
                                            _p, _i32, _i32, _i64, _i64, _i32, _p, _i32, _p])

# device-resident datasets (srwn_version() 122): the draw and the log launch around a training step fed by a BatchSampler
SIGNATURES["srwn_batch_draw"] = (C.c_int, [_p, _p, _i32, _i64, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _i32, _p,
                                           _i64, _i32, _i32, _i32, _i32, _p, _p])
SIGNATURES["srwn_step_log"] = (C.c_int, [_p, _p, _i32, _p, _p])
# device-resident training for the student and the twins (srwn_version() 123): a DistillSampler's and a PairSampler's launches
SIGNATURES["srwn_distill_draw"] = (C.c_int, [_p, _p, _i32, _i64, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _f32,
                                             _p, _i32, _i64, _i32, _i32, _i32, _i32, _p, _p])
SIGNATURES["srwn_cond_scatter"] = (C.c_int, [_p, _i64, _i32, _p, _i32, _i64, _i32, _p])
SIGNATURES["srwn_distill_log"] = (C.c_int, [_p, _p, _p, _f64, _f64, _i64, _f64, _p, _p, _p, _i32, _p, _p])
SIGNATURES["srwn_pair_draw"] = (C.c_int, [_p, _p, _p, _p, _p, _i32, _i32, _i64, _p, _i32, _i32, _i64, _i32, _i32, _i32, _i32,
                                          _p, _p, _p, _p, _p, _p])
SIGNATURES["srwn_pair_log"] = (C.c_int, [_p, _p, _i32, _p, _p, _i32, _p, _p])
# device-resident evaluation (srwn_version() 124): an EvalSampler's launch behind the classifier's forward pass
SIGNATURES["srwn_eval_classes"] = (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p])
# device-resident evaluation of an embedding model (srwn_version() 125): an EmbedSampler's launch behind a tower's forward
# pass, and the all-pairs launch behind a sweep's last step
SIGNATURES["srwn_embed_collect"] = (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p])
SIGNATURES["srwn_pair_sweep"] = (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _f32, _p, _p, _p, _p, _p, _p, _p, _p, _p])
# training controls (srwn_version() 126): the Adam update with lr and EMA decay from a device table, the shadow in the same pass
SIGNATURES["srwn_adam_step_ctl"] = (C.c_int, [_p, _p, _p, _p, _p, _i64, _p, _p, _p, _i32, _f32, _f32, _f32, _f32, _p, _i32, _p])
# augmented draws (srwn_version() 127): the two draws with the augmentation block behind their own arguments -- shift bound,
# gain range, the noise set's pointer, count and clip length, the coin threshold, volume range
_AUG = [_i32, _f32, _f32, _p, _i32, _i64, _i64, _f32, _f32]
SIGNATURES["srwn_batch_draw_aug"] = (C.c_int, SIGNATURES["srwn_batch_draw"][1][:-1] + _AUG + [_p])
SIGNATURES["srwn_pair_draw_aug"] = (C.c_int, SIGNATURES["srwn_pair_draw"][1][:-1] + _AUG + [_p])
# speed perturbation (srwn_version() 128): the augmented draws with the resampling block behind the augmentation block --
# the polyphase table, its taps, the fixed-point step range
_WARP = [_p, _i32, _i32, _i32]
SIGNATURES["srwn_batch_draw_warp"] = (C.c_int, SIGNATURES["srwn_batch_draw_aug"][1][:-1] + _WARP + [_p])
SIGNATURES["srwn_pair_draw_warp"] = (C.c_int, SIGNATURES["srwn_pair_draw_aug"][1][:-1] + _WARP + [_p])
# room reverberation (srwn_version() 129): the resampling draws with the room block behind the resampling block -- the
# impulse responses, their count, their taps, the coin's threshold
_ROOM = [_p, _i32, _i32, _i64]
SIGNATURES["srwn_batch_draw_room"] = (C.c_int, SIGNATURES["srwn_batch_draw_warp"][1][:-1] + _ROOM + [_p])
SIGNATURES["srwn_pair_draw_room"] = (C.c_int, SIGNATURES["srwn_pair_draw_warp"][1][:-1] + _ROOM + [_p])

_lib = None
BINDING = None     # "pybind11" or "ctypes" once loaded


def signature_hash() -> str:
    """Identifies the symbol table a pybind11 module was generated from (compiled into it as SIGNATURE_HASH)."""
    import hashlib
    txt = ";".join("%s:%s:%s" % (n, r.__name__, ",".join(a.__name__ for a in args)) for n, (r, args) in SIGNATURES.items())
    return hashlib.sha256(txt.encode()).hexdigest()[:16]


def _address(a):
    """What the pybind11 functions take for an argument the ctypes binding would have converted itself."""
    if a is None:
        return 0
    if isinstance(a, (int, float)):
        return a
    if isinstance(a, numbers.Integral):          # numpy integers
        return int(a)
    if isinstance(a, numbers.Real):
        return float(a)
    if isinstance(a, C.Array):
        return C.addressof(a)
    if isinstance(a, C._SimpleCData):            # c_void_p(...) and friends
        return a.value or 0
    if hasattr(a, "_obj"):                       # ctypes.byref(x)
        return C.addressof(a._obj)
    raise TypeError("cannot pass %r through the C-ABI" % (a,))


class _PybindLib:
    """The pybind11 module behind the attribute interface of a ctypes library (lib.srwn_xxx(args))."""

    def __init__(self, mod, keepalive):
        self._keepalive = keepalive
        for name in SIGNATURES:
            fn = getattr(mod, name)              # AttributeError if the symbol is missing
            setattr(self, name, (lambda f: lambda *args: f(*[_address(a) for a in args]))(fn))


def pybind_path() -> str:
    import sysconfig
    return os.path.join(HERE, "_srwn_pyb" + sysconfig.get_config_var("EXT_SUFFIX"))


def bind(kind: str):
    """A fresh binding of libsrwn.so of the given kind ("pybind11" / "ctypes"); load() caches the default one."""
    if kind not in ("pybind11", "ctypes"):
        raise RuntimeError("SRWN_BINDING=%s: pybind11 or ctypes" % kind)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libsrwn.so not found at %s: build it with `python sr-wavenet_amd/build.py` "
            "(there is no CPU fallback for the product path)" % LIB_PATH)
    if _ALT_LIB:
        kind = "ctypes"
    else:
        _check_manifest()
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    if kind == "pybind11":
        path = pybind_path()
        if not os.path.exists(path):
            raise RuntimeError("pybind11 module %s not built: run `python sr-wavenet_amd/build.py` "
                               "(or SRWN_BINDING=ctypes for the ctypes binding of the same library)" % path)
        import importlib.util
        spec = importlib.util.spec_from_file_location("_srwn_pyb", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if mod.SIGNATURE_HASH != signature_hash():
            raise RuntimeError("the pybind11 module was generated from a different symbol table: rebuild with "
                               "`python sr-wavenet_amd/build.py`")
        return _PybindLib(mod, lib)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Loads libsrwn.so once and binds every symbol (SRWN_BINDING: pybind11, the default, or ctypes); raises if anything
    is missing."""
    global _lib, BINDING
    if _lib is None:
        kind = "ctypes" if _ALT_LIB else os.environ.get("SRWN_BINDING", "pybind11")
        _lib, BINDING = bind(kind), kind
    return _lib


def _check_manifest():
    """build.py records the sha256 of every source next to the library; a library older than the sources it ships with
    (an edit without a rebuild) is refused instead of silently running yesterday's kernels."""
    man = os.path.join(HERE, "libsrwn.manifest.json")
    if not os.path.exists(man) or not os.path.isdir(os.path.join(HERE, "csrc")):
        return
    import hashlib
    import json
    root = os.path.dirname(HERE)
    for rel, digest in json.load(open(man)).get("sources", {}).items():
        path = os.path.join(root, rel)
        if os.path.exists(path) and hashlib.sha256(open(path, "rb").read()).hexdigest() != digest:
            raise RuntimeError("libsrwn.so was built from a different %s: rebuild with `python sr-wavenet_amd/build.py`" % rel)


def call(name, *args):
    """Calls an int-returning entry point and raises RuntimeError on a non-zero code."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.srwn_last_error()
        raise RuntimeError("%s failed (code %d): %s" % (name, rc, msg.decode() if msg else ""))
    return rc
