"""The auto-encoder's encoder and the joint encoder+decoder training step on one MI355X.

Mirrors ``WaveNetAutoEncoder.createEncoder`` / ``createNetwork`` (model.py:136-156, 203-216) and
``ResidualDilationLayerNC`` (ops.py:48-58):

  a_0     = relu(conv_K(relu(inputs)))                      1 -> EC channels, SAME padding ('nc_conv')
  r_0     = relu(a_0 W_r + b_r)                             (every consumer of a layer output applies relu first,
  a_{l+1} = relu(conv_K(r_l) + b_l);  r_{l+1} = relu(a_{l+1} Wr_l + br_l)       so relu(h) is what is stored)
  encoding = avgpool_T( (sum_l a_{l+1} Ws_l + bs_l) W_lat + b_lat )

The skip path is linear up to the pool, so the pool is applied FIRST: per-frame means of a_l ([B*frames, EC] per layer,
one batched pass), then the skip 1x1s of all layers as ONE K = L*EC product and the latent 1x1 on B*frames rows --
the [B,T,S] skip tensors of the reference are never formed, and their gradient returns to the layers as a
per-frame broadcast inside the backward GEMM epilogue (srwn_tap_linear's frame_add).

The K = 2 non-causal convolutions, their data gradients and the 1x1s run as time-tap MFMA GEMMs (srwn_tap_linear);
weight gradients are time-contraction GEMMs (srwn_wgrad) batched over layers.
"""
from __future__ import annotations

import os

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import kernels as K
from . import packing as P
from . import _lib
from ._lib import call
from .engine import OptControls, Section, StackConfig, WaveNetEngine, adam_update, swap_with_ema
from .audio_ring import AudioRingSlots

# What SRWN_ENC_FUSED means when it is not set (FrameEncoder in bf16): "0" the layer-by-layer twin, "1" the one-launch
# chain.  Set by measurement: tools/encode_bench.py case (b) at B = 1, pool 512 has the chain at 0.160 ms per push
# against the twin's 0.367 (spreads <= 0.016).  The README's knob table, FrameEncoder's docstring and that
# tool's header state the same value (tests/test_encoder_stream.py holds the knob table to it).
ENC_FUSED_DEFAULT = "1"


def plan_frames(received: int, emitted: int, nlayers: int, pool_stride: int, final: bool = False,
                max_frames: Optional[int] = None):
    """Which frames of a stream can be encoded now, and from which samples.

    With 'nc_conv' plus ``nlayers`` K = 2 layers that each look one sample ahead and none back, frame f depends on the
    samples [f*P, (f+1)*P + nlayers + 1) and nothing else.  A running stream (``final=False``) that has received
    ``received`` samples may therefore emit frame f once (f+1)*P + nlayers + 1 <= received; at the end of the clip
    (``final=True``) every whole frame is due and the missing look-ahead is the clip-end zero padding.  Returns the
    launches for the frames [emitted, due) as tuples ``(first_frame, nframes, start, valid_rows)``: a window of the stream
    starting at sample ``start = first_frame * P`` with ``valid_rows`` real samples in it, at most ``max_frames`` frames
    each.  Pure Python: the CPU tests drive the fp64 oracle with it."""
    received, emitted, L, P = int(received), int(emitted), int(nlayers), int(pool_stride)
    if received < 0 or emitted < 0 or L < 0 or P < 1 or emitted * P > received:
        raise ValueError("plan_frames: received=%d emitted=%d nlayers=%d pool_stride=%d" % (received, emitted, L, P))
    if max_frames is not None and max_frames < 1:
        raise ValueError("plan_frames: max_frames %r" % (max_frames,))
    due = received // P if final else max(0, (received - L - 1) // P)
    out = []
    f = emitted
    while f < due:
        n = due - f if max_frames is None else min(due - f, int(max_frames))
        out.append((f, n, f * P, min(received - f * P, n * P + L + 1)))
        f += n
    return out


def plan_pool(received, emitted, final, active, nlayers, pool_stride, max_rows, limit=None):
    """One step of an encoder POOL: which frames of which slots are encoded now, as launches of frames of any streams.

    Slot u holds a stream of its own with ``received[u]`` samples in, ``emitted[u]`` frames out and ``final[u]`` once no
    more audio comes.  A frame is due by ``plan_frames``' rule -- running: (f+1)*P + L + 1 <= received, final: every whole
    frame -- and ``limit[u]`` (a sequence or a dict; None or a missing slot: no cap) caps the frames a slot emits this
    step: the back-pressure of a consumer with a bounded ring, under which the frames held back simply stay audio.
    Returns the launches, each a list of ``(slot, frame, first_sample, valid)`` ordered by slot, then frame (one slot's
    frames are neighbouring rows), at most ``max_rows`` items each; ``first_sample = frame * P`` and ``valid =
    min(received - frame * P, P + L + 1)`` real samples from there on.  Pure Python: the CPU tests drive the fp64 oracle
    with it."""
    L, P, max_rows = int(nlayers), int(pool_stride), int(max_rows)
    n = len(received)
    if L < 0 or P < 1 or max_rows < 1 or not (len(emitted) == len(final) == len(active) == n):
        raise ValueError("plan_pool: nlayers=%d pool_stride=%d max_rows=%d over %d slots" % (L, P, max_rows, n))
    items = []
    for u in range(n):
        if not active[u]:
            continue
        r, e = int(received[u]), int(emitted[u])
        if r < 0 or e < 0 or e * P > r:
            raise ValueError("plan_pool: slot %d received=%d emitted=%d" % (u, r, e))
        due = r // P if final[u] else max(0, (r - L - 1) // P)
        cap = None if limit is None else (limit.get(u) if isinstance(limit, dict) else limit[u])
        if cap is not None:
            if int(cap) < 0:
                raise ValueError("plan_pool: limit %d for slot %d" % (int(cap), u))
            due = min(due, e + int(cap))
        items.extend((u, f, f * P, min(r - f * P, P + L + 1)) for f in range(e, due))
    return [items[i:i + max_rows] for i in range(0, len(items), max_rows)]


class _EncoderParams:
    """The encoder's flat fp32 parameter buffer by section, its initialisation and the reference's variable names:
    what ``EncoderStack`` (training) and ``EncoderWeights`` (inference) share.  Needs self.L/EC/S/Kw/lat/dev."""

    def _build_sections(self):
        L, EC, S, Kw, lat = self.L, self.EC, self.S, self.Kw, self.lat
        secs: Dict[str, Section] = {}
        off = 0
        for name, shape in (("nc_w", (Kw, 1, EC)), ("nc_b", (EC,)), ("nc_wr", (EC, EC)), ("nc_br", (EC,)),
                            ("EW", (L, Kw, EC, EC)), ("EB", (L, EC)), ("EWR", (L, EC, EC)), ("EBR", (L, EC)),
                            ("EWS", (L, EC, S)), ("EBS", (L, S)), ("lat_w", (S, lat)), ("lat_b", (lat,))):
            secs[name] = Section(name, off, shape)
            off += secs[name].numel
        self.sections, self.nparams = secs, off
        self.params = torch.zeros(off, dtype=torch.float32, device=self.dev)
        # 'nc_conv' has a skip 1x1 whose output is discarded (model.py:141): a variable without gradient
        self.dead = {"nc_ws": torch.zeros((EC, S), device=self.dev), "nc_bs": torch.zeros(S, device=self.dev)}

    def view(self, name: str, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
        s = self.sections[name]
        buf = self.params if buf is None else buf
        return buf[s.offset:s.offset + s.numel].view(s.shape)

    def _init_host(self, seed: int):
        """Xavier-uniform kernels, zero biases -> self.params and the dead skip kernel."""
        rng = np.random.default_rng(seed)

        def xav(shape, fan_in, fan_out):
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            return torch.tensor(rng.uniform(-lim, lim, size=shape), dtype=torch.float32)

        L, EC, S, Kw, lat = self.L, self.EC, self.S, self.Kw, self.lat
        host = torch.zeros(self.nparams, dtype=torch.float32)

        def put(name, t):
            s = self.sections[name]
            host[s.offset:s.offset + s.numel] = t.reshape(-1)

        put("nc_w", xav((Kw, 1, EC), Kw, Kw * EC)); put("nc_wr", xav((EC, EC), EC, EC))
        put("EW", xav((L, Kw, EC, EC), Kw * EC, Kw * EC)); put("EWR", xav((L, EC, EC), EC, EC))
        put("EWS", xav((L, EC, S), EC, S)); put("lat_w", xav((S, lat), S, lat))
        self.params.copy_(host)
        self.dead["nc_ws"].copy_(xav((EC, S), EC, S))

    def _oracle_host(self, ep):
        host = torch.zeros(self.nparams, dtype=torch.float32)

        def put(name, arr):
            s = self.sections[name]
            host[s.offset:s.offset + s.numel] = torch.tensor(np.asarray(arr), dtype=torch.float32).reshape(-1)

        put("nc_w", ep.nc.w); put("nc_b", ep.nc.b); put("nc_wr", ep.nc.wr); put("nc_br", ep.nc.br)
        for nm, f in (("EW", "w"), ("EB", "b"), ("EWR", "wr"), ("EBR", "br"), ("EWS", "ws"), ("EBS", "bs")):
            put(nm, np.stack([getattr(p, f) for p in ep.layers]))
        put("lat_w", ep.lat_w); put("lat_b", ep.lat_b)
        self.params.copy_(host)

    def named_tensors(self, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        v = lambda n: self.view(n, buf)
        out = {"nc.w": v("nc_w"), "nc.b": v("nc_b"), "nc.wr": v("nc_wr"), "nc.br": v("nc_br")}
        for i in range(self.L):
            out[f"e{i}.w"] = v("EW")[i]; out[f"e{i}.b"] = v("EB")[i]
            out[f"e{i}.wr"] = v("EWR")[i]; out[f"e{i}.br"] = v("EBR")[i]
            out[f"e{i}.ws"] = v("EWS")[i]; out[f"e{i}.bs"] = v("EBS")[i]
        out["lat_w"] = v("lat_w"); out["lat_b"] = v("lat_b")
        return out

    def tf_variables(self, scope: str) -> Dict[str, torch.Tensor]:
        """Reference names under ``<scope>`` = 'WaveNetAutoEncoder/Encoder': the K-tap conv lives in '<name>_NC/conv1d'
        (ops.py:50-51); the unnamed 1x1s number per scope -- residual conv1d_{2j}, skip conv1d_{2j+1} for the j-th
        NC layer ('nc_conv' is j = 0), the latent 1x1 is conv1d_{2(L+1)} (model.py:141-152)."""
        cname = lambda j: "conv1d" if j == 0 else "conv1d_%d" % j
        n = self.named_tensors()
        out = {f"{scope}/nc_conv_NC/conv1d/kernel": n["nc.w"], f"{scope}/nc_conv_NC/conv1d/bias": n["nc.b"],
               f"{scope}/{cname(0)}/kernel": n["nc.wr"].unsqueeze(0), f"{scope}/{cname(0)}/bias": n["nc.br"],
               f"{scope}/{cname(1)}/kernel": self.dead["nc_ws"].unsqueeze(0), f"{scope}/{cname(1)}/bias": self.dead["nc_bs"]}
        for i in range(self.L):
            nm = f"dilated_conv_{i}_NC"
            out[f"{scope}/{nm}/conv1d/kernel"] = n[f"e{i}.w"]
            out[f"{scope}/{nm}/conv1d/bias"] = n[f"e{i}.b"]
            out[f"{scope}/{cname(2 * i + 2)}/kernel"] = n[f"e{i}.wr"].unsqueeze(0)
            out[f"{scope}/{cname(2 * i + 2)}/bias"] = n[f"e{i}.br"]
            out[f"{scope}/{cname(2 * i + 3)}/kernel"] = n[f"e{i}.ws"].unsqueeze(0)
            out[f"{scope}/{cname(2 * i + 3)}/bias"] = n[f"e{i}.bs"]
        out[f"{scope}/{cname(2 * self.L + 2)}/kernel"] = n["lat_w"].unsqueeze(0)
        out[f"{scope}/{cname(2 * self.L + 2)}/bias"] = n["lat_b"]
        return out


def _check_encoder_widths(encoder_channels, filter_width, skip_channels):
    if encoder_channels != 128:
        raise NotImplementedError("encoder_channels %d: the encoder kernels are built for 128 (the reference "
                                  "default, model.py:76)" % encoder_channels)
    if filter_width != 2:
        raise NotImplementedError("filter_width %d: only 2 is built" % filter_width)
    if skip_channels % 32 or skip_channels < 32:
        raise NotImplementedError("skip_channels must be a multiple of 32")


class EncoderStack(_EncoderParams):
    def __init__(self, nlayers: int, batch: int, length: int, pool_stride: int, encoder_channels: int = 128,
                 skip_channels: int = 256, latent_channels: int = 16, filter_width: int = 2,
                 dtype: torch.dtype = torch.bfloat16, learning_rate: float = 1e-3, device="cuda", seed: int = 0):
        _check_encoder_widths(encoder_channels, filter_width, skip_channels)
        if length % pool_stride:
            raise ValueError("length %d is not a multiple of pool_stride %d" % (length, pool_stride))
        self.L, self.B, self.T, self.pool = int(nlayers), int(batch), int(length), int(pool_stride)
        self.N = self.B * self.T
        self.frames = self.T // self.pool
        self.rows_c = self.B * self.frames
        self.EC, self.S, self.lat, self.Kw = encoder_channels, skip_channels, latent_channels, filter_width
        self.dt, self.dev, self.lr = dtype, torch.device(device), learning_rate
        self.ctl = OptControls()      # training controls (optim.TrainControls) of this parameter buffer
        self.ctl.engines.add(self)
        self._build_params(seed)
        self._build_packing()
        self._alloc()
        self.repack()

    # -- parameters ----------------------------------------------------------------------------------
    def _build_params(self, seed):
        self._build_sections()
        z = lambda: torch.zeros(self.nparams, dtype=torch.float32, device=self.dev)
        self.grads, self.adam_m, self.adam_v = z(), z(), z()
        self.adam_step = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.init_parameters(seed)

    def init_parameters(self, seed: int):
        self._init_host(seed)
        self.adam_m.zero_(); self.adam_v.zero_(); self.adam_step.zero_()
        self.ctl.reset_ema(self.params)

    def load_oracle_params(self, ep):
        self._oracle_host(ep)
        self.adam_m.zero_(); self.adam_v.zero_(); self.adam_step.zero_()
        self.ctl.reset_ema(self.params)
        self.repack()

    # -- MFMA weight images --------------------------------------------------------------------------
    def _build_packing(self):
        L, EC, S, Kw = self.L, self.EC, self.S, self.Kw
        sec = self.sections
        pk = K.Packer(self.dev)
        self.o_nc_wr = P.pack_linear(pk, sec["nc_wr"].offset, EC, EC, EC)
        self.o_nc_wrT = P.pack_linear_T(pk, sec["nc_wr"].offset, EC, EC, EC)
        self.o_conv, self.o_convT, self.o_wr, self.o_wrT = [], [], [], []
        # fused layer kernels (srwn_nc_layer_fwd/_bwd: bf16, 128 channels, K = 2; SRWN_NC_FUSED=0 keeps the two-launch
        # path): the 1x1's B operand is the conv's accumulator tile -> the 1x1 images in permuted k order
        self.fused = (self.dt == torch.bfloat16 and EC == 128 and Kw == 2 and
                      os.environ.get("SRWN_NC_FUSED", "1") != "0")
        self.o_wr_p, self.o_wrT_p = [], []
        for l in range(L):
            self.o_conv.append(P.pack_conv(pk, sec["EW"].offset + l * Kw * EC * EC, Kw, EC))
            self.o_convT.append(P.pack_conv_T(pk, sec["EW"].offset + l * Kw * EC * EC, Kw, EC))
            self.o_wr.append(P.pack_linear(pk, sec["EWR"].offset + l * EC * EC, EC, EC, EC))
            self.o_wrT.append(P.pack_linear_T(pk, sec["EWR"].offset + l * EC * EC, EC, EC, EC))
            if self.fused:
                self.o_wr_p.append(P.pack_linear(pk, sec["EWR"].offset + l * EC * EC, EC, EC, EC, perm=True))
                self.o_wrT_p.append(P.pack_linear_T(pk, sec["EWR"].offset + l * EC * EC, EC, EC, EC, perm=True))
        if self.fused:
            self.o_nc_wrT_p = P.pack_linear_T(pk, sec["nc_wr"].offset, EC, EC, EC, perm=True)
        # every skip 1x1 as one image: rows = skip channel, k = layer*EC + n (applied to the frame means)
        self.o_ws = pk.reserve(S // 32, L * EC // 16)
        for l in range(L):
            P.fill_linear(pk, self.o_ws, sec["EWS"].offset + l * EC * S, EC, S, S // 32, L * EC // 16,
                          ks_offset=l * EC // 16, ks_count=EC // 16)
        # and transposed: rows = layer*EC + n, k = skip channel (gradient back to the frame means)
        per = (EC // 32) * (S // 16) * 512
        self.o_wsT = pk.reserve(L * (EC // 32), S // 16)
        for l in range(L):
            P.fill_linear_T(pk, self.o_wsT + l * per, sec["EWS"].offset + l * EC * S, EC, S, EC // 32, S // 16)
        pk.finalize()
        self.packer = pk
        self.packed = torch.zeros(max(pk.total, 1), dtype=self.dt, device=self.dev)

    def wptr(self, off: int) -> int:
        return self.packed.data_ptr() + off * self.packed.element_size()

    def repack(self):
        self.packer.gather(self.params, self.packed)

    # -- buffers -------------------------------------------------------------------------------------
    def _alloc(self):
        B, T, N, L, EC, S = self.B, self.T, self.N, self.L, self.EC, self.S
        z = lambda *s, dt=self.dt: torch.zeros(s, dtype=dt, device=self.dev)
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.dev)
        self.x = f(B, T); self.xr = f(B, T)
        self.a = z(L + 1, N, EC)          # a[0] from 'nc_conv', a[l+1] from layer l (post-relu)
        self.r = z(L, N, EC)              # r[l] = relu(residual output feeding layer l)
        self.dpre = z(L + 1, N, EC)       # gradient at the conv pre-activations
        self.dh = z(L + 1, N, EC)         # gradient at the residual pre-activations; dh[L] stays 0 (unused output)
        if self.fused:                    # relu masks as bit words in the fused kernels' tile/lane layout
            nw = int(_lib.load().srwn_nc_mask_words(B, T))
            self.abits = torch.zeros(L + 1, nw, dtype=torch.int64, device=self.dev)
            self.rbits = torch.zeros(L, nw, dtype=torch.int64, device=self.dev)
        self.a_mean = z(L, self.rows_c, EC)
        self.bs_sum = f(S)
        self.s_mean = f(self.rows_c, S)
        self.s_parts = f(L * self.rows_c * S)
        self.enc = f(self.rows_c, self.lat)
        self.ds_mean = z(self.rows_c, S)
        self.da_all = f(self.rows_c, L * EC)
        self.nslabs = K.wgrad_slabs(N)
        # (few frame rows: 128-row slabs, or the skip 1x1 gradients are L workgroups walking them in 32-row steps: 139 us)
        self.nslabs_c = max(K.wgrad_slabs(self.rows_c), min(max(1, 256 // max(L, 1)), max(1, self.rows_c // 128)))
        self.wg_parts = f(max(self.nslabs * EC * EC, self.nslabs_c * L * EC * S))
        self.wg_bparts = f(max(self.nslabs * EC, self.nslabs_c * L * S))
        # fused per-layer weight-gradient pass: about two 8-wave workgroups per CU over (slab, layer)
        self.ns_enc = max(1, min(self.nslabs, max(4, 512 // max(L, 1))))
        ne = self.ns_enc
        self.pe_w = f(L * ne * self.Kw * EC * EC); self.pe_r = f(L * ne * EC * EC)
        self.pe_b = f(L * ne * EC); self.pe_br = f(L * ne * EC)
        self.ic_ws = f(int(_lib.load().srwn_init_conv_wgrad_partials(B, T, EC, self.Kw)))

    # -- forward -------------------------------------------------------------------------------------
    def _tap(self, x, ntaps, step, wp, bias, y, epi, aux=None, fadd_ptr=None):
        EC, L = self.EC, self.L
        call("srwn_tap_linear", x.data_ptr(), EC, ntaps, step, self.T, EC, wp, None if bias is None else bias.data_ptr(),
             y.data_ptr(), EC, EC, self.N, None if aux is None else aux.data_ptr(), EC, fadd_ptr, L * EC, self.frames,
             self.pool, 1.0 / self.pool, epi, K.abi_dtype(self.dt), K._stream())

    def forward(self, inputs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """inputs [B,T] fp32 -> self.enc [B*frames, latent] fp32 (model.py:136-156)."""
        B, T, N, L, EC, S = self.B, self.T, self.N, self.L, self.EC, self.S
        v = self.view
        if inputs is not None:
            self.x.copy_(inputs.reshape(B, T))
        st = K._stream()
        call("srwn_nc_input_fwd", self.x.data_ptr(), v("nc_w").data_ptr(), v("nc_b").data_ptr(), self.a[0].data_ptr(),
             B, T, EC, self.Kw, K.abi_dtype(self.dt), st)
        self._tap(self.a[0], 1, 0, self.wptr(self.o_nc_wr), v("nc_br"), self.r[0], K.EPI_RELU)
        for l in range(L):
            if self.fused:   # conv + relu + 1x1 + relu in one launch; the last layer's residual output is never used
                call("srwn_nc_layer_fwd", self.r[l].data_ptr(), self.wptr(self.o_conv[l]), self.wptr(self.o_wr_p[l]),
                     v("EB")[l].data_ptr(), v("EBR")[l].data_ptr(), self.a[l + 1].data_ptr(),
                     self.r[l + 1].data_ptr() if l < L - 1 else None, self.abits[l + 1].data_ptr(),
                     self.rbits[l + 1].data_ptr() if l < L - 1 else None, B, T, EC, self.Kw, K.abi_dtype(self.dt), st)
                continue
            self._tap(self.r[l], self.Kw, 1, self.wptr(self.o_conv[l]), v("EB")[l], self.a[l + 1], K.EPI_RELU)
            if l < L - 1:   # the last layer's residual output is never used (model.py:144-150)
                self._tap(self.a[l + 1], 1, 0, self.wptr(self.o_wr[l]), v("EBR")[l], self.r[l + 1], K.EPI_RELU)
        # pooled skip path: frame means, all skip 1x1s as one product, latent 1x1
        call("srwn_frame_sum_batched", self.a[1].data_ptr(), N * EC, self.a_mean.data_ptr(), self.rows_c * EC, L, B, T,
             EC, self.frames, self.pool, 1.0 / self.pool, K.abi_dtype(self.dt), st)
        K.reduce_partials(v("EBS").reshape(-1), L, S, 1, True, 1.0, self.bs_sum.data_ptr(), 0)
        # K = L*EC on few rows: one k-slice per layer, then a fixed-order sum of the slices
        call("srwn_pw_linear_ksplit", self.a_mean.data_ptr(), EC, self.rows_c * EC, EC, L * EC, self.wptr(self.o_ws),
             self.bs_sum.data_ptr(), self.s_parts.data_ptr(), S, S, S, self.rows_c, L, K.abi_dtype(self.dt), st)
        K.reduce_partials(self.s_parts, L, self.rows_c * S, 1, True, 1.0, self.s_mean.data_ptr(), 0)
        call("srwn_small_gemm", self.s_mean.data_ptr(), S, S, 0, K.F32, v("lat_w").data_ptr(), self.lat, 1, S, 0,
             v("lat_b").data_ptr(), self.enc.data_ptr(), self.lat, K.F32, self.rows_c, self.lat, S, 0, st)
        return self.enc

    # -- backward ------------------------------------------------------------------------------------
    def backward(self, denc: torch.Tensor):
        """denc [B*frames, latent] fp32 = d loss / d encoding; fills self.grads."""
        B, T, N, L, EC, S, Kw = self.B, self.T, self.N, self.L, self.EC, self.S, self.Kw
        v = self.view
        g = self.grads
        gp, sec, dt, st = g.data_ptr(), self.sections, self.dt, K._stream()
        rc = self.rows_c
        K._chk(denc, "denc", torch.float32, (rc, self.lat))
        # latent 1x1 and the skip 1x1s on the frame axis
        call("srwn_small_wgrad", self.s_mean.data_ptr(), S, denc.data_ptr(), self.lat, v("lat_w", g).data_ptr(),
             v("lat_b", g).data_ptr(), rc, S, self.lat, 1.0, st)
        call("srwn_small_gemm", denc.data_ptr(), self.lat, self.lat, 0, K.F32, v("lat_w").data_ptr(), 1, self.lat,
             self.lat, 0, None, self.ds_mean.data_ptr(), S, K.abi_dtype(dt), rc, S, self.lat, 0, st)
        K.wgrad(self.a_mean.data_ptr(), rc * EC, EC, self.ds_mean.data_ptr(), 0, S, None, L, self.wg_parts,
                self.wg_bparts, rc, self.frames, self.nslabs_c, dt)
        K.reduce_partials(self.wg_parts, self.nslabs_c, EC * S, L, True, 1.0, gp + 4 * sec["EWS"].offset, EC * S)
        K.reduce_partials(self.wg_bparts, self.nslabs_c, S, L, True, 1.0, gp + 4 * sec["EBS"].offset, S)
        K.pw_linear(self.ds_mean.data_ptr(), S, 0, S, S, self.wptr(self.o_wsT), None, self.da_all, L * EC, L * EC, rc,
                    epi=K.EPI_F32, compute_dtype=dt)
        # layer chain, top down: the pooled skip gradient enters as a per-frame broadcast (frame_add)
        if self.fused:
            # one launch per layer: the conv data gradient of layer l, then the 1x1 data gradient of the layer below it
            # (layer l-1's residual 1x1, or 'nc_conv''s under layer 0) on the tile still in registers
            self._tap(self.dh[L], 1, 0, self.wptr(self.o_wrT[L - 1]), None, self.dpre[L], K.EPI_MASK, aux=self.a[L],
                      fadd_ptr=self.da_all.data_ptr() + 4 * (L - 1) * EC)          # dh[L] = 0: the skip path only
            for t_, bits in ((self.a[0], self.abits[0]), (self.r[0], self.rbits[0])):   # written by the generic kernels
                call("srwn_nc_mask_bits", t_.data_ptr(), bits.data_ptr(), B, T, EC, K.abi_dtype(dt), st)
            for l in range(L - 1, -1, -1):
                call("srwn_nc_layer_bwd", self.dpre[l + 1].data_ptr(), self.wptr(self.o_convT[l]),
                     self.rbits[l].data_ptr(), self.dh[l].data_ptr(),
                     self.wptr(self.o_wrT_p[l - 1] if l else self.o_nc_wrT_p),
                     self.da_all.data_ptr() + 4 * (l - 1) * EC if l else None, L * EC, self.frames, self.pool,
                     1.0 / self.pool, self.abits[l].data_ptr(), self.dpre[l].data_ptr(), B, T, EC, Kw, K.abi_dtype(dt), st)
        else:
            for l in range(L - 1, -1, -1):
                self._tap(self.dh[l + 1], 1, 0, self.wptr(self.o_wrT[l]), None, self.dpre[l + 1], K.EPI_MASK,
                          aux=self.a[l + 1], fadd_ptr=self.da_all.data_ptr() + 4 * l * EC)
                self._tap(self.dpre[l + 1], Kw, -1, self.wptr(self.o_convT[l]), None, self.dh[l], K.EPI_MASK,
                          aux=self.r[l])
            self._tap(self.dh[0], 1, 0, self.wptr(self.o_nc_wrT), None, self.dpre[0], K.EPI_MASK, aux=self.a[0])
        # weight gradients of the L layers -- both conv taps, the 1x1 residual and the two biases -- in ONE pass over
        # r, a, dpre, dh (layer l: r[l], a[l+1], dpre[l+1], dh[l+1]; the last layer's residual 1x1 sees dh[L] = 0)
        NE = N * EC
        ne = self.ns_enc
        call("srwn_wgrad_nc_layers", self.r.data_ptr(), self.a[1].data_ptr(), self.dpre[1].data_ptr(),
             self.dh[1].data_ptr(), NE, L, self.pe_w.data_ptr(), self.pe_r.data_ptr(), self.pe_b.data_ptr(),
             self.pe_br.data_ptr(), N, T, ne, EC, Kw, K.abi_dtype(dt), st)
        K.reduce_partials(self.pe_w, ne, Kw * EC * EC, L, True, 1.0, gp + 4 * sec["EW"].offset, Kw * EC * EC)
        K.reduce_partials(self.pe_b, ne, EC, L, True, 1.0, gp + 4 * sec["EB"].offset, EC)
        K.reduce_partials(self.pe_r, ne, EC * EC, L, True, 1.0, gp + 4 * sec["EWR"].offset, EC * EC)
        K.reduce_partials(self.pe_br, ne, EC, L, True, 1.0, gp + 4 * sec["EBR"].offset, EC)
        # 'nc_conv': its residual 1x1 (a[0], dh[0]) ...
        ns = self.nslabs
        K.wgrad(self.a.data_ptr(), NE, EC, self.dh.data_ptr(), NE, EC, None, 1, self.wg_parts, self.wg_bparts, N, T, ns,
                dt)
        K.reduce_partials(self.wg_parts, ns, EC * EC, 1, True, 1.0, gp + 4 * sec["nc_wr"].offset, 0)
        K.reduce_partials(self.wg_bparts, ns, EC, 1, True, 1.0, gp + 4 * sec["nc_br"].offset, 0)
        # ... and its K-tap conv on the raw clip: taps relu(x)[t+k]
        call("srwn_clamp", self.x.data_ptr(), self.xr.data_ptr(), N, 0.0, 3.0e38, st)
        K.init_conv_wgrad(self.xr, self.dpre[0].view(B, T, EC), v("nc_w", g).reshape(-1), v("nc_b", g), Kw,
                          -(Kw - 1) + (Kw - 1) // 2, self.ic_ws)

    def optimizer_step(self, grad_scale: float = 1.0, joint_clip: bool = False):
        self._adam_update(grad_scale, joint_clip)
        self.repack()

    def _adam_update(self, grad_scale: float, joint_clip: bool = False):
        """As ``WaveNetEngine._adam_update``: srwn_adam_step without controls; with them [srwn_sumsq -> srwn_clip_scale ->]
        srwn_adam_step_ctl, the two clip launches left to the owner of a joint norm (`joint_clip`)."""
        c = self.ctl
        if c.controls is not None and c.clip is not None:
            if not joint_clip:
                K.sumsq(self.grads, c.sq_parts)
                K.clip_scale(c.sq_parts, c.controls.clip_norm, grad_scale, c.clip)
            grad_scale = 1.0
        adam_update(c, self.params, self.grads, self.adam_m, self.adam_v, self.adam_step, self.lr, grad_scale, c.clip)

    # -- training controls (optim.py), as WaveNetEngine's -------------------------------------------------
    @property
    def clip(self):
        return self.ctl.clip

    @property
    def ema(self):
        return self.ctl.ema

    def set_controls(self, controls):
        if self.ctl.set(controls, self.params):
            self.ctl.drop_graphs()

    def swap_ema(self):
        swap_with_ema(self.ctl, self.params)
        self.repack()


class AutoEncoderEngine:
    """Encoder + conditioned mixture-of-logistics decoder trained jointly (model.py:103-116, 203-216)."""

    def __init__(self, dec_cfg: StackConfig, batch: int, length: int, encoder_channels: int, latent_channels: int,
                 condition_size: int, device="cuda", seed: int = 0, process_group=None):
        if dec_cfg.head_mode != "mol" or not dec_cfg.shift_input:
            raise ValueError("the decoder is the RightShift-ed mixture-of-logistics stack (model.py:158-200)")
        if dec_cfg.cond_channels != latent_channels + condition_size:
            raise ValueError("decoder cond_channels must be latent_channels + condition_size (model.py:161-167)")
        self.dec = WaveNetEngine(dec_cfg, batch, length, device, seed=seed, process_group=process_group)
        self.enc = EncoderStack(len(dec_cfg.dilations), batch, length, dec_cfg.pool_stride, encoder_channels,
                                dec_cfg.skip_channels, latent_channels, dec_cfg.filter_width, dec_cfg.dtype,
                                dec_cfg.learning_rate, device, seed + 1)
        self.B, self.T, self.N = self.dec.B, self.dec.T, self.dec.N
        self.lat, self.cs = latent_channels, condition_size
        self.denc = torch.zeros((self.enc.rows_c, self.lat), dtype=torch.float32, device=self.dec.dev)
        self.loss = self.dec.loss
        self._sq_parts = None      # training controls with clipping: the partials of ONE norm over both gradient buffers
        self.dec.ctl.engines.add(self)      # (the graphs of train / fit hang on this object)

    def set_inputs(self, inputs: torch.Tensor, conditions: Optional[torch.Tensor] = None):
        d = self.dec
        self.enc.x.copy_(inputs.reshape(self.B, self.T))
        d.audio.copy_(self.enc.x)
        d.cond_in.zero_()
        if self.cs:
            if conditions is None:
                raise ValueError("this auto-encoder was built with condition_size > 0; pass conditions [B, condition_size]")
            c = conditions.reshape(self.B, 1, self.cs).expand(-1, d.frames, -1)              # model.py:162-165
            d.cond_in.view(self.B, d.frames, d.Ep)[:, :, self.lat:self.lat + self.cs].copy_(c)

    def encode(self):
        """Runs the encoder and writes the encoding into the decoder's conditioning rows."""
        e, d = self.enc, self.dec
        e.forward()
        call("srwn_small_gemm", e.s_mean.data_ptr(), e.S, e.S, 0, K.F32, e.view("lat_w").data_ptr(), e.lat, 1, e.S, 0,
             e.view("lat_b").data_ptr(), d.cond_in.data_ptr(), d.Ep, K.abi_dtype(d.dt), e.rows_c, e.lat, e.S, 0,
             K._stream())
        return e.enc

    def forward(self, want_logits: bool = False):
        self.encode()
        return self.dec.forward(want_logits=want_logits)

    def backward(self):
        d, e = self.dec, self.enc
        d.backward(join=False)   # its weight-gradient tail runs beside the encoder's backward
        # d loss / d encoding = sum_l dcb_l Wc_l^T restricted to the latent columns (model.py:180)
        call("srwn_small_gemm", d.dcb.data_ptr(), d.R, d.R, e.rows_c * d.R, K.abi_dtype(d.dt),
             d.view("WC").data_ptr(), 1, d.R, d.R, d.E * d.R, None, self.denc.data_ptr(), self.lat, K.F32, e.rows_c,
             self.lat, d.L * d.R, 0, K._stream())
        e.backward(self.denc)
        d.join_side()

    def allreduce_grads(self):
        self.dec.allreduce_grads()
        from . import dp
        dp.allreduce_sum_(self.enc.grads, self.dec.pg)

    def optimizer_step(self):
        d, e = self.dec, self.enc
        joint = d.ctl.controls is not None and d.ctl.clip is not None
        if joint:       # tf.clip_by_global_norm over the encoder's and the decoder's gradients: one norm, one factor
            pd = K.sumsq_partials(d.nparams)
            K.sumsq(d.grads, self._sq_parts[:pd])
            K.sumsq(e.grads, self._sq_parts[pd:])
            K.clip_scale(self._sq_parts, d.ctl.controls.clip_norm, 1.0, d.ctl.clip)
        d._adam_update(joint)      # the mixture loss is a SUM over batch and time: shard gradients add
        d.repack()
        e.optimizer_step(1.0, joint)

    # -- training controls (optim.py): both buffers follow one table; each keeps its step counter and its shadow ------
    @property
    def clip(self):
        return self.dec.ctl.clip

    @property
    def world(self):
        return self.dec.world

    def set_controls(self, controls):
        d, e = self.dec, self.enc
        drop = d.ctl.set(controls, d.params)
        drop = e.ctl.set(controls, e.params) or drop
        if controls is not None and controls.clip_norm is not None:
            if self._sq_parts is None:
                self._sq_parts = torch.zeros(K.sumsq_partials(d.nparams) + K.sumsq_partials(e.nparams),
                                             dtype=torch.float32, device=d.dev)
            e.ctl.clip = d.ctl.clip
        else:
            self._sq_parts = None
        if drop:
            d.ctl.drop_graphs()

    def swap_ema(self):
        self.dec.swap_ema()
        self.enc.swap_ema()

    def train_step(self):
        self.forward()
        self.backward()
        self.allreduce_grads()
        self.optimizer_step()
        return self.loss

    def capture_graphs(self):
        """{forward, backward} and {Adam, re-pack} as two hipGraphs with the all-reduce between them (see
        WaveNetEngine.capture_graphs).  Call after one eager train_step."""
        torch.cuda.synchronize()
        self._g_fb = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g_fb):
            self.forward()
            self.backward()
        self._g_opt = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g_opt, pool=self._g_fb.pool()):
            self.optimizer_step()
        torch.cuda.synchronize()

    def train_step_graphed(self):
        self._g_fb.replay()
        self.allreduce_grads()
        self._g_opt.replay()
        return self.loss


# ----------------------------------------------------------------------------------------------------------------------
# The encoder on its own: weights without a training shape, and the frame encoder that serves any batch and length
# ----------------------------------------------------------------------------------------------------------------------
class EncoderWeights(_EncoderParams):
    """The encoder's parameters and MFMA images for inference: the sections, names and loaders of ``EncoderStack`` with
    no batch, length, gradients or Adam state."""

    def __init__(self, nlayers: int, encoder_channels: int = 128, skip_channels: int = 256, latent_channels: int = 16,
                 filter_width: int = 2, dtype: torch.dtype = torch.bfloat16, device="cuda", seed: int = 0):
        _check_encoder_widths(encoder_channels, filter_width, skip_channels)
        if nlayers < 1:
            raise ValueError("nlayers %d" % nlayers)
        self.L = int(nlayers)
        self.EC, self.S, self.lat, self.Kw = encoder_channels, skip_channels, latent_channels, filter_width
        self.dt, self.dev = dtype, torch.device(device)
        self._build_sections()
        self._init_host(seed)
        self._build_packing()
        self.repack()

    def load_oracle_params(self, ep):
        self._oracle_host(ep)
        self.repack()

    def _build_packing(self):
        L, EC, S, Kw = self.L, self.EC, self.S, self.Kw
        sec = self.sections
        pk = K.Packer(self.dev)
        # per layer [conv | 1x1 in permuted k order] back to back: the one-launch kernel walks them by a stride
        self.o_conv, self.o_wr_p, self.o_wr = [], [], []
        for l in range(L):
            self.o_conv.append(P.pack_conv(pk, sec["EW"].offset + l * Kw * EC * EC, Kw, EC))
            self.o_wr_p.append(P.pack_linear(pk, sec["EWR"].offset + l * EC * EC, EC, EC, EC, perm=True))
        self.layer_stride = self.o_conv[1] - self.o_conv[0] if L > 1 else 0
        self.o_nc_wr_p = P.pack_linear(pk, sec["nc_wr"].offset, EC, EC, EC, perm=True)
        # natural k order: the layer-by-layer path's row-streaming GEMMs (srwn_tap_linear)
        self.o_nc_wr = P.pack_linear(pk, sec["nc_wr"].offset, EC, EC, EC)
        for l in range(L):
            self.o_wr.append(P.pack_linear(pk, sec["EWR"].offset + l * EC * EC, EC, EC, EC))
        # every skip 1x1 as one image: rows = skip channel, k = layer*EC + n (applied to the frame means)
        self.o_ws = pk.reserve(S // 32, L * EC // 16)
        for l in range(L):
            P.fill_linear(pk, self.o_ws, sec["EWS"].offset + l * EC * S, EC, S, S // 32, L * EC // 16,
                          ks_offset=l * EC // 16, ks_count=EC // 16)
        pk.finalize()
        self.packer = pk
        self.packed = torch.zeros(max(pk.total, 1), dtype=self.dt, device=self.dev)
        self.bs_sum = torch.zeros(S, dtype=torch.float32, device=self.dev)

    def wptr(self, off: int) -> int:
        return self.packed.data_ptr() + off * self.packed.element_size()

    def repack(self):
        """Images and the sum of the skip biases from the current parameters (call after changing ``params``)."""
        self.packer.gather(self.params, self.packed)
        K.reduce_partials(self.view("EBS").reshape(-1), self.L, self.S, 1, True, 1.0, self.bs_sum.data_ptr(), 0)


class EncoderStreamState:
    """One batch of streams moving in lockstep through a ``FrameEncoder``: the samples received, the frames emitted and
    the audio not consumed yet (fewer than pool_stride + nlayers + 1 samples per stream, on the device)."""
    __slots__ = ("owner", "B", "received", "emitted", "tail", "closed")

    def __init__(self, owner, B, tail):
        self.owner, self.B, self.received, self.emitted, self.tail, self.closed = owner, B, 0, 0, tail, False


class FrameEncoder:
    """Audio in, latent frames out (createEncoder, model.py:136-156) for any batch <= ``max_batch`` and any length, whole
    clips (``encode``) or chunk by chunk (``start`` / ``push`` / ``finish``).

    Every layer of the encoder looks one sample ahead and none back, so a frame depends on its own pool_stride + L + 1
    samples only (``plan_frames``): a stream carries no activations, only the audio it has not consumed, and a frame's
    value does not depend on how the audio was cut.  In bf16 the whole chain of a launch's frames is ONE kernel
    (srwn_nc_encode_frames) that leaves the per-frame means of a_1..a_L: the default (``ENC_FUSED_DEFAULT``), up to the
    kernel's 32 layers.  SRWN_ENC_FUSED=0, fp32 and deeper encoders run the same windows one launch per layer with the
    training kernels (each window as a clip of its own); ``fused`` says which path an object runs.  Both end in the
    pooled skip product, its reduction and the latent 1x1."""

    def __init__(self, weights: EncoderWeights, pool_stride: int, max_batch: int = 1, max_frames: int = 32):
        self._check_weights(weights)
        if pool_stride < 1 or max_batch < 1 or max_frames < 1:
            raise ValueError("FrameEncoder: pool_stride=%r max_batch=%r max_frames=%r" % (pool_stride, max_batch, max_frames))
        w = self.w = weights
        self.P, self.max_batch, self.max_frames = int(pool_stride), int(max_batch), int(max_frames)
        self.L, self.lat = w.L, w.lat
        lib = _lib.load()
        self.fused = (w.dt == torch.bfloat16 and os.environ.get("SRWN_ENC_FUSED", ENC_FUSED_DEFAULT) != "0" and
                      w.L <= int(lib.srwn_nc_encode_max_layers()))
        # the twin's layers: srwn_nc_layer_fwd in bf16 unless SRWN_NC_FUSED=0 (two time-tap GEMMs per layer, as in training)
        self.layer_fused = w.dt == torch.bfloat16 and os.environ.get("SRWN_NC_FUSED", "1") != "0"
        rows = self.max_batch * self.max_frames
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=w.dev)
        self.a_mean = torch.zeros(w.L * rows * w.EC, dtype=w.dt, device=w.dev)
        self.s_parts = f(w.L * rows * w.S)
        self.s_mean = f(rows * w.S)
        self.enc = f(rows * w.lat)
        self.wmax = self.max_frames * self.P + w.L + 1          # the longest window of one launch
        if self.fused:
            self.parts = f(int(lib.srwn_nc_encode_partials(self.max_batch, self.max_frames, self.P, w.L)))
        else:
            n = self.max_batch * self.wmax
            self.xs = f(n)
            self.r = torch.zeros(2 * n * w.EC, dtype=w.dt, device=w.dev)
            self.a = torch.zeros((w.L + 1) * n * w.EC, dtype=w.dt, device=w.dev)      # [a_0 | a_1 .. a_L]

    @staticmethod
    def _check_weights(w):
        if getattr(w, "EC", None) != 128:
            raise NotImplementedError("encoder_channels %r: the encoder kernels are built for 128" % getattr(w, "EC", None))
        if getattr(w, "Kw", None) != 2:
            raise NotImplementedError("filter_width %r: only 2 is built" % getattr(w, "Kw", None))

    def device_bytes(self) -> int:
        """Bytes of the buffers this object owns (the weights' parameters and images are counted with the weights)."""
        return sum(t.numel() * t.element_size() for t in vars(self).values() if isinstance(t, torch.Tensor))

    # -- one launch sequence: B streams x nframes frames from a window --------------------------------------------
    def _run(self, x: torch.Tensor, nframes: int, valid: int) -> torch.Tensor:
        """x [B, >= valid] fp32 (rows `x.stride(0)` apart), column 0 = the first frame's first sample."""
        w, P_, L = self.w, self.P, self.L
        B, EC, S, dt = x.shape[0], w.EC, w.S, K.abi_dtype(w.dt)
        rows, st, v = B * nframes, K._stream(), w.view
        if self.fused:
            call("srwn_nc_encode_frames", x.data_ptr(), x.stride(0), v("nc_w").data_ptr(), v("nc_b").data_ptr(),
                 w.wptr(w.o_nc_wr_p), v("nc_br").data_ptr(), w.wptr(w.o_conv[0]), w.layer_stride, w.wptr(w.o_wr_p[0]),
                 w.layer_stride, v("EB").data_ptr(), v("EBR").data_ptr(), self.parts.data_ptr(), self.a_mean.data_ptr(),
                 B, nframes, P_, valid, L, EC, w.Kw, dt, st)
        else:
            self._layers(x, nframes, valid)
        call("srwn_pw_linear_ksplit", self.a_mean.data_ptr(), EC, rows * EC, EC, L * EC, w.wptr(w.o_ws),
             w.bs_sum.data_ptr(), self.s_parts.data_ptr(), S, S, S, rows, L, dt, st)
        K.reduce_partials(self.s_parts, L, rows * S, 1, True, 1.0, self.s_mean.data_ptr(), 0)
        call("srwn_small_gemm", self.s_mean.data_ptr(), S, S, 0, K.F32, v("lat_w").data_ptr(), self.lat, 1, S, 0,
             v("lat_b").data_ptr(), self.enc.data_ptr(), self.lat, K.F32, rows, self.lat, S, 0, st)
        return self.enc[:rows * self.lat].view(B, nframes, self.lat).clone()

    def _layers(self, x, nframes, valid):
        """The window as a clip of its own, one launch per layer (EncoderStack.forward's kernels): the false zero padding
        at its end moves inward one row per layer and never reaches a frame row."""
        w, P_, L = self.w, self.P, self.L
        B, EC, T = x.shape[0], w.EC, int(valid)
        N, dt, st, v, es = B * T, K.abi_dtype(w.dt), K._stream(), w.view, self.a.element_size()
        xs = self.xs[:N].view(B, T)
        xs.copy_(x[:, :T])
        a = lambda l: self.a.data_ptr() + l * N * EC * es
        r = lambda l: self.r.data_ptr() + (l & 1) * N * EC * es
        frames = (T + P_ - 1) // P_

        def tap(xp, ntaps, step, wp, bias, yp):
            call("srwn_tap_linear", xp, EC, ntaps, step, T, EC, wp, bias.data_ptr(), yp, EC, EC, N, None, EC, None, L * EC,
                 frames, P_, 1.0 / P_, K.EPI_RELU, dt, st)

        call("srwn_nc_input_fwd", xs.data_ptr(), v("nc_w").data_ptr(), v("nc_b").data_ptr(), a(0), B, T, EC, w.Kw, dt, st)
        tap(a(0), 1, 0, w.wptr(w.o_nc_wr), v("nc_br"), r(0))
        for l in range(L):
            last = l == L - 1          # the last layer's residual output is never used (model.py:144-150)
            if self.layer_fused:
                call("srwn_nc_layer_fwd", r(l), w.wptr(w.o_conv[l]), w.wptr(w.o_wr_p[l]), v("EB")[l].data_ptr(),
                     v("EBR")[l].data_ptr(), a(l + 1), None if last else r(l + 1), None, None, B, T, EC, w.Kw, dt, st)
                continue
            tap(r(l), w.Kw, 1, w.wptr(w.o_conv[l]), v("EB")[l], a(l + 1))
            if not last:
                tap(a(l + 1), 1, 0, w.wptr(w.o_wr[l]), v("EBR")[l], r(l + 1))
        call("srwn_frame_sum_batched", a(1), N * EC, self.a_mean.data_ptr(), B * nframes * EC, L, B, T, EC, nframes, P_,
             1.0 / P_, dt, st)

    # -- public --------------------------------------------------------------------------------------------------
    def _audio(self, audio, B=None):
        if isinstance(audio, torch.Tensor):
            x = audio
        else:
            x = torch.as_tensor(np.asarray(audio, dtype=np.float32))
        if x.dim() != 2:
            raise ValueError("audio must be [batch, samples], got shape %s" % (tuple(x.shape),))
        if not 1 <= x.shape[0] <= self.max_batch:
            raise ValueError("batch %d: this encoder was built for max_batch=%d" % (x.shape[0], self.max_batch))
        if B is not None and x.shape[0] != B:
            raise ValueError("audio of %d streams pushed into a state of %d" % (x.shape[0], B))
        if x.dtype not in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
            raise ValueError("audio must be floating point, got %s" % x.dtype)
        return x

    def _emit(self, buf, base, received, emitted, final):
        """Runs the launches `plan_frames` asks for over buf (column 0 = sample `base`) -> ([B, k, latent], frames)."""
        outs = []
        for (f0, n, start, valid) in plan_frames(received, emitted, self.L, self.P, final, self.max_frames):
            outs.append(self._run(buf[:, start - base:], n, valid))
            emitted = f0 + n
        if not outs:
            return torch.zeros((buf.shape[0], 0, self.lat), dtype=torch.float32, device=self.w.dev), emitted
        return (outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)), emitted

    def encode(self, audio) -> torch.Tensor:
        """audio [B, T] -> [B, T // pool_stride, latent] fp32 on the device (T < pool_stride: no frame)."""
        x = self._audio(audio).to(device=self.w.dev, dtype=torch.float32).contiguous()
        return self._emit(x, 0, x.shape[1], 0, True)[0]

    def start(self, batch: int = 1) -> EncoderStreamState:
        if not 1 <= int(batch) <= self.max_batch:
            raise ValueError("batch %r: this encoder was built for max_batch=%d" % (batch, self.max_batch))
        return EncoderStreamState(self, int(batch), torch.zeros((int(batch), 0), dtype=torch.float32, device=self.w.dev))

    def _state(self, state):
        if not isinstance(state, EncoderStreamState) or state.owner is not self:
            raise ValueError("this state was not started by this encoder")
        if state.closed:
            raise ValueError("this stream is closed (finish was called)")
        return state

    def push(self, state: EncoderStreamState, audio) -> torch.Tensor:
        """audio [B, n], n >= 0 -> the frames whose look-ahead is now complete, [B, k, latent] (k may be 0)."""
        st = self._state(state)
        x = self._audio(audio, st.B)
        buf = torch.cat([st.tail, x.to(device=self.w.dev, dtype=torch.float32)], dim=1)
        base, received = st.emitted * self.P, st.received + int(x.shape[1])
        out, emitted = self._emit(buf, base, received, st.emitted, False)
        st.tail = buf[:, emitted * self.P - base:].clone()
        st.received, st.emitted = received, emitted
        return out

    def finish(self, state: EncoderStreamState) -> torch.Tensor:
        """The remaining whole frames, with the clip-end padding; the state is closed afterwards."""
        st = self._state(state)
        out, emitted = self._emit(st.tail, st.emitted * self.P, st.received, st.emitted, True)
        st.emitted, st.closed = emitted, True
        st.tail = st.tail[:, :0]
        return out

    def pool(self, audio_ring: Optional[int] = None, max_rows: Optional[int] = None) -> "EncoderPool":
        """An ``EncoderPool`` on this encoder's buffers: its ``max_batch`` rows as slots, each a stream at a clock of its
        own.  audio_ring: samples a slot can hold (>= pool_stride + L + 1; default max_frames * pool_stride + L + 1 +
        pool_stride); max_rows: frames per launch (default, and at most, max_batch * max_frames)."""
        return EncoderPool(self, audio_ring, max_rows)


class EncoderPool(AudioRingSlots):
    """``FrameEncoder.pool()``: the encoder's ``max_batch`` rows as SLOTS, each holding a stream with its own samples
    received, frames emitted and end.  Streams ``join`` free slots, ``push`` audio of any length whenever it arrives
    (``audio_ring.AudioRingSlots``, shared with the classifier pool: one upload and one srwn_audio_ring_put however many
    slots are written; a slot's audio lives in its row of a device ring, sample s in column s mod audio_ring, and
    nothing is re-allocated), ``step`` encodes every frame that is due -- of
    every slot, as launches over a LIST of frames (``plan_pool``; srwn_nc_encode_frame_list on the fused path, the same
    plan gathered into windows and run layer by layer otherwise) -- and a stream that was ``finish``ed frees its slot
    with its last frame.  A stream's frames put together equal ``FrameEncoder.encode`` of its audio alone, bit for bit:
    in any slot, whenever it joined, however its audio was cut and whatever the other slots hold.  A frame reads its own
    ``valid`` samples counted from its first one, so what an earlier stream left in a slot's ring is never read."""

    def __init__(self, owner: FrameEncoder, audio_ring: Optional[int] = None, max_rows: Optional[int] = None):
        fe = self.fe = owner
        self.P, self.L, self.lat, self.capacity = fe.P, fe.L, fe.lat, fe.max_batch
        self.window = self.P + self.L + 1                                  # the samples one frame reads
        rows = fe.max_batch * fe.max_frames
        self.audio_ring = fe.max_frames * self.P + self.L + 1 + self.P if audio_ring is None else int(audio_ring)
        self.max_rows = rows if max_rows is None else int(max_rows)
        if self.audio_ring < self.window:
            raise ValueError("pool: audio_ring %d holds less than one frame's pool_stride + L + 1 = %d samples"
                             % (self.audio_ring, self.window))
        if not 1 <= self.max_rows <= rows:
            raise ValueError("pool: max_rows %d: 1..max_batch * max_frames = %d" % (self.max_rows, rows))
        self._alloc_audio_ring()
        cap = self.capacity
        self._received = np.zeros(cap, np.int64)
        self._emitted = np.zeros(cap, np.int64)
        self._final = np.zeros(cap, bool)
        self._active = np.zeros(cap, bool)
        self.table = torch.zeros((self.max_rows, 4), dtype=torch.int32, device=self.dev)      # SrwnEncFrame per item

    # ---- inspection
    dev = property(lambda self: self.fe.w.dev, doc="The encoder's device.")

    @property
    def received(self) -> np.ndarray:
        """Samples pushed into each slot's stream so far."""
        return self._received.copy()

    @property
    def emitted(self) -> np.ndarray:
        """Frames each slot's stream has emitted so far."""
        return self._emitted.copy()

    def audio_room(self, slot: int) -> int:
        """Samples a slot can take now: audio_ring minus what it holds beyond its emitted frames."""
        u, = self._slot_list(slot, "audio_room")
        return int(self.audio_ring - (self._received[u] - self._emitted[u] * self.P))

    # ---- streams come and go
    def join(self, n: int = 1, slots=None):
        """n streams into free slots (the lowest ones, or `slots`); returns the slots.  A slot starts at sample 0."""
        slots = self._take_slots(int(n) if slots is None else None, slots)
        for u in slots:
            self._received[u] = self._emitted[u] = 0
            self._final[u], self._active[u] = False, True
        return list(slots)

    def leave(self, slots) -> None:
        """Ends the streams in `slots` where they are (a slot already free stays free) and frees their slots."""
        for u in self._slot_list(slots, "leave", distinct=True):
            self._active[u] = False

    def finish(self, slots) -> None:
        """No more audio comes for these streams: their remaining whole frames are due with the clip-end padding, and each
        frees its slot with its last frame (at the next ``step``)."""
        slots = self._slot_list(slots, "finish", distinct=True)
        if any(not self._active[u] for u in slots):
            raise ValueError("finish: slots %s do not all hold a stream" % (slots,))
        for u in slots:
            self._final[u] = True

    def _push_barred(self):
        """``AudioRingSlots.push``: a finished stream takes no more audio."""
        return self._final, "push: the stream in slot %d was finished"

    def _room_tail(self, u):
        return "emitted %d frames" % self._emitted[u]

    # ---- one step: every frame that is due
    def _launch(self, items) -> torch.Tensor:
        """The frames of one launch of ``plan_pool`` -> [len(items), latent] fp32 (a copy)."""
        fe, w, n = self.fe, self.fe.w, len(items)
        tab = np.zeros((n, 4), np.int32)
        tab[:, 0] = [it[0] for it in items]
        tab[:, 1] = [it[2] % self.audio_ring for it in items]
        tab[:, 2] = [it[3] for it in items]
        if not fe.fused:
            return self._launch_windows(tab)
        self.table[:n].copy_(torch.from_numpy(tab))
        EC, S, L, dt, st, v = w.EC, w.S, self.L, K.abi_dtype(w.dt), K._stream(), w.view
        call("srwn_nc_encode_frame_list", self.ring.data_ptr(), self.audio_ring, self.capacity, self.table.data_ptr(), n,
             v("nc_w").data_ptr(), v("nc_b").data_ptr(), w.wptr(w.o_nc_wr_p), v("nc_br").data_ptr(), w.wptr(w.o_conv[0]),
             w.layer_stride, w.wptr(w.o_wr_p[0]), w.layer_stride, v("EB").data_ptr(), v("EBR").data_ptr(),
             fe.parts.data_ptr(), fe.a_mean.data_ptr(), self.P, L, EC, w.Kw, dt, st)
        call("srwn_pw_linear_ksplit", fe.a_mean.data_ptr(), EC, n * EC, EC, L * EC, w.wptr(w.o_ws), w.bs_sum.data_ptr(),
             fe.s_parts.data_ptr(), S, S, S, n, L, dt, st)
        K.reduce_partials(fe.s_parts, L, n * S, 1, True, 1.0, fe.s_mean.data_ptr(), 0)
        call("srwn_small_gemm", fe.s_mean.data_ptr(), S, S, 0, K.F32, v("lat_w").data_ptr(), self.lat, 1, S, 0,
             v("lat_b").data_ptr(), fe.enc.data_ptr(), self.lat, K.F32, n, self.lat, S, 0, st)
        return fe.enc[:n * self.lat].view(n, self.lat).clone()

    def _launch_windows(self, tab) -> torch.Tensor:
        """The layer-by-layer encoders (fp32, SRWN_ENC_FUSED=0, more than 32 layers) on the same plan: the items' windows
        gathered from the ring, grouped by `valid`, each group a batch of one-frame windows through ``FrameEncoder._run``."""
        fe, dev = self.fe, self.fe.w.dev
        out = torch.zeros((tab.shape[0], self.lat), dtype=torch.float32, device=dev)
        gmax = max(1, min(fe.max_batch * fe.max_frames, (fe.max_batch * fe.wmax) // self.window))
        for valid in sorted(set(int(x) for x in tab[:, 2])):
            idx = np.flatnonzero(tab[:, 2] == valid)
            for g0 in range(0, len(idx), gmax):
                g = idx[g0:g0 + gmax]
                cols = (tab[g, 1].astype(np.int64)[:, None] + np.arange(valid)[None, :]) % self.audio_ring
                x = self.ring[torch.from_numpy(tab[g, 0].astype(np.int64)).to(dev)[:, None], torch.from_numpy(cols).to(dev)]
                out[torch.from_numpy(g).to(dev)] = fe._run(x.contiguous(), 1, valid)[:, 0]
        return out

    def step(self, limit=None):
        """Every frame that is due now (``plan_pool``; limit: frames per slot at most, a sequence or a dict) -> {slot:
        frames [k, latent] fp32 on the device} for the slots with k > 0.  A finished slot whose frames are all out becomes
        free.  With nothing due nothing is launched."""
        launches = plan_pool(self._received, self._emitted, self._final, self._active, self.L, self.P, self.max_rows, limit)
        pieces = {}
        for items in launches:
            out = self._launch(items)
            i = 0
            while i < len(items):
                j = i
                while j < len(items) and items[j][0] == items[i][0]:
                    j += 1
                pieces.setdefault(items[i][0], []).append(out[i:j])
                self._emitted[items[i][0]] += j - i
                i = j
        done = self._active & self._final & ((self._emitted + 1) * self.P > self._received)
        self._active[done] = False
        return {u: (p[0] if len(p) == 1 else torch.cat(p, dim=0)) for u, p in pieces.items()}
