"""Parallel-WaveNet student on one MI355X: inverse-autoregressive flows distilled against a frozen teacher.

Mirrors ``ParallelWaveNet`` (model.py:290-537):

  flow i     x_{i+1} = x_i * exp(p_i[...,0]) + p_i[...,1],  p_i = head(stack_i(RightShift(x_i), encoding))
             (createPartialFlow / createFlow, model.py:415-487: the conditioned residual stack WITHOUT its skip
             path -- model.py:440-449 is commented out -- and a relu -> 1x1 R->2 head)
  out        clip(z * s_tot + mu_tot, -1, 1) (model.py:517-535) -- algebraically x_F, which is what is computed
  loss       (beta * MoL_NLL(out | teacher logits on the TRUTH clip) - alpha * sum(log s_tot + 2)
              + gamma * ||mean_frames|STFT(truth)|^2 - mean_frames|STFT(out)|^2||_F^2) / B      (model.py:356-379)
             The teacher runs on ``inputs_truth`` (input_map, model.py:318-324) and is frozen (stop_gradient,
             model.py:334): the student's gradient enters the cross entropy through x only.
  update     tf.clip_by_global_norm(grads, 1.0) then Adam (model.py:382-401, the train_fast path student.py:107 uses)

All flows share one flat fp32 parameter / gradient / Adam buffer (one all-reduce, one norm, one update).
Inference (``FlowSynthesizer``, ``SynthPool``) runs the flows as chunked streams: one ``stream_stack.StreamStack`` per flow
(group plan, boundary buffers, roll table, group launches) on a shared top buffer and one clock.
"""
from __future__ import annotations

import math
import os
from dataclasses import replace
from typing import Dict, List, Optional

import numpy as np
import torch

from . import dp
from . import kernels as K
from ._lib import call
from .engine import SQRT_HALF, OptControls, Section, StackConfig, WaveNetEngine, _Span, adam_update, swap_with_ema
from .slots import SlotTable, per_stream
from .stream_stack import StreamStack, stream_history_rows      # (the latter for this module's users)


class FlowStorage:
    """Flat fp32 buffers shared by all flows of one student."""

    def __init__(self, n: int, device):
        z = lambda: torch.zeros(n, dtype=torch.float32, device=device)
        self.params, self.grads, self.adam_m, self.adam_v = z(), z(), z(), z()
        self.adam_step = torch.zeros(1, dtype=torch.int64, device=device)


class FlowStack(WaveNetEngine):
    """One flow: ``createPartialFlow`` + the affine transform of ``createFlow`` (model.py:415-487)."""

    def __init__(self, cfg: StackConfig, batch: int, length: int, device="cuda", seed: int = 0,
                 storage: Optional[FlowStorage] = None, slot: int = 0):
        if not cfg.cond_channels:
            raise ValueError("a flow is conditioned on the teacher's encoding (model.py:431): cond_channels > 0")
        cfg = replace(cfg, head_mode="flow", shift_input=True, output_channels=2)
        self._storage, self._slot = storage, slot
        super().__init__(cfg, batch, length, device=device, seed=seed)

    # -- parameters ----------------------------------------------------------------------------------
    @staticmethod
    def layout(cfg: StackConfig) -> Dict[str, Section]:
        L, R, Kw, E = len(cfg.dilations), cfg.dilation_channels, cfg.filter_width, cfg.cond_channels
        secs: Dict[str, Section] = {}
        off = 0
        for name, shape in (("init_w", (Kw, 1, R)), ("init_b", (R,)), ("WF", (L, Kw, R, R)), ("BF", (L, R)),
                            ("WR", (L, R, R)), ("BR", (L, R)), ("WC", (L, E, R)), ("BC", (L, R)),
                            ("flow_w", (R, 2)), ("flow_b", (2,))):   # flow_w | flow_b stay adjacent (one reduce)
            secs[name] = Section(name, off, shape)
            off += secs[name].numel
        return secs

    @staticmethod
    def param_count(cfg: StackConfig) -> int:
        secs = FlowStack.layout(cfg)
        last = secs["flow_b"]
        return last.offset + last.numel

    def _build_params(self, seed):
        self.sections = self.layout(self.cfg)
        self.nparams = self.param_count(self.cfg)
        st = self._storage or FlowStorage(self.nparams, self.dev)
        lo = self._slot * self.nparams
        self.params, self.grads = st.params[lo:lo + self.nparams], st.grads[lo:lo + self.nparams]
        self.adam_m, self.adam_v = st.adam_m[lo:lo + self.nparams], st.adam_v[lo:lo + self.nparams]
        self.adam_step = st.adam_step
        L, R, S, Kw = self.L, self.R, self.S, self.Kw
        # variables the reference creates but never trains in a flow: the dead gate conv (ops.py:31-33) and the
        # unused skip 1x1s (ops.py:44, model.py:440-449); kept for checkpoint interchange
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.dev)
        self.dead_gate = {"WG": f(L, Kw, R, R), "BG": f(L, R)}
        self.dead_skip = {"WS": f(L, R, S), "BS": f(L, S)}
        self.init_parameters(seed)

    def init_parameters(self, seed: int):
        rng = np.random.default_rng(seed)

        def xav(shape, fan_in, fan_out):
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            return torch.tensor(rng.uniform(-lim, lim, size=shape), dtype=torch.float32)

        L, R, S, Kw, E = self.L, self.R, self.S, self.Kw, self.E
        host = torch.zeros(self.nparams, dtype=torch.float32)

        def put(name, t):
            s = self.sections[name]
            host[s.offset:s.offset + s.numel] = t.reshape(-1)

        put("init_w", xav((Kw, 1, R), Kw, Kw * R))
        put("WF", xav((L, Kw, R, R), Kw * R, Kw * R))
        put("WR", xav((L, R, R), R, R))
        put("WC", xav((L, E, R), E, R))
        put("flow_w", xav((R, 2), R, 2))
        self.params.copy_(host)
        self.dead_gate["WG"].copy_(xav((L, Kw, R, R), Kw * R, Kw * R))
        self.dead_skip["WS"].copy_(xav((L, R, S), R, S))

    def load_oracle_params(self, sp):
        host = torch.zeros(self.nparams, dtype=torch.float32)

        def put(name, arr):
            s = self.sections[name]
            host[s.offset:s.offset + s.numel] = torch.tensor(np.asarray(arr), dtype=torch.float32).reshape(-1)

        put("init_w", sp.init_w); put("init_b", sp.init_b)
        for nm, f in (("WF", "wf"), ("BF", "bf"), ("WR", "wr"), ("BR", "br"), ("WC", "wc"), ("BC", "bc")):
            put(nm, np.stack([getattr(l, f) for l in sp.layers]))
        put("flow_w", sp.head_w2); put("flow_b", sp.head_b2)
        self.params.copy_(host)
        self.repack()

    def named_tensors(self, buf: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        out = {"init_w": self.view("init_w", buf), "init_b": self.view("init_b", buf)}
        for i in range(self.L):
            for nm, f in (("WF", "wf"), ("BF", "bf"), ("WR", "wr"), ("BR", "br"), ("WC", "wc"), ("BC", "bc")):
                out[f"l{i}.{f}"] = self.view(nm, buf)[i]
        out["head_w2"] = self.view("flow_w", buf); out["head_b2"] = self.view("flow_b", buf)
        return out

    def tf_variables(self, scope: str, decoder: bool = True) -> Dict[str, torch.Tensor]:
        """Reference names inside ``<scope>`` = 'ParallelWaveNet/Flow{i}/Flow{i}' (model.py:417,468): per layer
        cond = conv1d_{3i}, residual = conv1d_{3i+1}, skip = conv1d_{3i+2}; the head is conv1d_{3L}."""
        cname = lambda j: "conv1d" if j == 0 else "conv1d_%d" % j
        n = self.named_tensors()
        out = {f"{scope}/causal_conv_Kernel": n["init_w"], f"{scope}/causal_conv_Bias": n["init_b"].view(1, 1, -1)}
        for i in range(self.L):
            nm = f"dilated_conv_{i}"
            out[f"{scope}/{nm}_filter/{nm}_Kernel"] = n[f"l{i}.wf"]
            out[f"{scope}/{nm}_filter/{nm}_Bias"] = n[f"l{i}.bf"].view(1, 1, -1)
            out[f"{scope}/{nm}_gate/{nm}_Kernel"] = self.dead_gate["WG"][i]
            out[f"{scope}/{nm}_gate/{nm}_Bias"] = self.dead_gate["BG"][i].view(1, 1, -1)
            out[f"{scope}/{cname(3 * i)}/kernel"] = n[f"l{i}.wc"].unsqueeze(0)
            out[f"{scope}/{cname(3 * i)}/bias"] = n[f"l{i}.bc"]
            out[f"{scope}/{cname(3 * i + 1)}/kernel"] = n[f"l{i}.wr"].unsqueeze(0)
            out[f"{scope}/{cname(3 * i + 1)}/bias"] = n[f"l{i}.br"]
            out[f"{scope}/{cname(3 * i + 2)}/kernel"] = self.dead_skip["WS"][i].unsqueeze(0)
            out[f"{scope}/{cname(3 * i + 2)}/bias"] = self.dead_skip["BS"][i]
        out[f"{scope}/{cname(3 * self.L)}/kernel"] = n["head_w2"].unsqueeze(0)
        out[f"{scope}/{cname(3 * self.L)}/bias"] = n["head_b2"]
        return out

    # -- images / buffers ----------------------------------------------------------------------------
    def _pack_head(self, pk):
        pass   # the R->2 head is a streaming dot product on fp32 weights (srwn_flow_affine_*)

    def _alloc_head_buffers(self):
        N, L, R = self.N, self.L, self.R
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=self.dev)
        self.pooled = self.mol = False
        self.prm = z(N, 2)
        self.x_out = z(N)
        self.dx_in = z(N)
        self.ent_parts = z(K.flow_partials(N))
        self.flow_parts = z(K.flow_partials(N), 2 * R + 2)
        if not self.use_wl:   # legacy per-product weight gradients (dilation_channels = 32)
            self.wg_parts = z(self.nslabs * L * R * R)
            self.wg_bparts = z(self.nslabs * L * R)

    def set_cond(self, cond: torch.Tensor):
        self.cond_in.zero_()
        self.cond_in[:, :self.E].copy_(cond.reshape(self.B * self.frames, self.E))

    # -- forward / backward ------------------------------------------------------------------------------
    def forward(self, x_in: Optional[torch.Tensor] = None):
        """x_in [B,T] fp32 (default: the staged ``self.audio``) -> self.x_out [B*T], self.prm [B*T,2]."""
        B, T, N, L, R = self.B, self.T, self.N, self.L, self.R
        v = self.view
        if x_in is not None:
            self.audio = x_in
        x = self.audio
        K.causal_conv1d_fwd(x.view(B, T, 1), v("init_w"), v("init_b"), 1, 1, out=self.xs[0])   # model.py:423-424
        self._cond_bias_to_input()                                                               # model.py:431-435
        with _Span(self, "flow_fwd_layers"):
            self._stack_fwd(self.cond_all)
        K.flow_affine_fwd(self.xs[L].view(N, R), v("flow_w"), v("flow_b"), x.view(N), self.prm, self.x_out,
                          self.ent_parts)                                                       # model.py:451-483

    def backward(self, dx_out: torch.Tensor, ent_grad: float, join: bool = True):
        """dx_out [B*T] = d loss / d x_out; leaves d loss / d x_in in self.dx_in and parameter gradients.
        join=False leaves the weight-gradient work running on the side stream (the caller joins ``self.side`` later):
        the flow below only needs dx_in, so its dgrad chain starts while this flow's weight gradients finish."""
        B, T, N, L, R, Kw = self.B, self.T, self.N, self.L, self.R, self.Kw
        dt = self.dt
        gp, sec = self.grads.data_ptr(), self.sections
        x = self.audio
        K.flow_affine_bwd(self.xs[L].view(N, R), self.view("flow_w"), self.prm, x.view(N), dx_out, ent_grad,
                          self.gs[L].view(N, R), self.dx_in, self.flow_parts)
        K.reduce_partials(self.flow_parts, self.flow_parts.shape[0], 2 * R + 2, 1, True, 1.0,
                          gp + 4 * sec["flow_w"].offset, 0)
        main = torch.cuda.current_stream()
        overlap = self.overlap and not self.timing and self.use_wl
        side = self.side if overlap else main
        groups = self._wl_groups() if self.use_wl else []
        group_lo = {g[0]: g for g in groups}
        with _Span(self, "flow_bwd_layers"):
            for l0, l1 in (reversed(self.groups) if self.fused_bwd else ()):   # one launch per layer group
                if self.fused_wt:       # ... that also sums the group's weight gradients (srwn_residual_group_bwd_wt)
                    self._group_bwd_wt(l0, l1)
                    continue
                self._group_bwd(l0, l1)
                if overlap:
                    ev = torch.cuda.Event()
                    ev.record(main)
                    side.wait_event(ev)
                with torch.cuda.stream(side):
                    self._wgrad_layers_group(l0, l1)
            for l in (() if self.fused_bwd else range(L - 1, -1, -1)):
                top = l == L - 1
                K.residual_layer_bwd(None if top else self.gs[l + 2], None if top else self.dfs[l + 1],
                                     None if top else self.wptr(self.o_convT[l + 1]), self.gs[l + 1],
                                     self.wptr(self.o_resT[l]), None, None, self.zs[l], self.dfs[l], B, T, R, 0, Kw,
                                     1 if top else self.dil[l + 1], 2 if top else 1, True, dt)
                if l in group_lo:
                    if overlap:
                        ev = torch.cuda.Event()
                        ev.record(main)
                        side.wait_event(ev)
                    with torch.cuda.stream(side):
                        self._wgrad_layers_group(*group_lo[l])
            if not self.fused_bwd:
                K.residual_layer_bwd(self.gs[1], self.dfs[0], self.wptr(self.o_convT[0]), self.gs[0],
                                     None, None, None, None, None, B, T, R, 0, Kw, self.dil[0], 1, False, dt)
        if overlap:   # gs[0] (and every G_l for the conditioning gradients) is complete
            ev = torch.cuda.Event()
            ev.record(main)
            side.wait_event(ev)
        with torch.cuda.stream(side):
            self._wgrad_layers_finish()
            self._wgrad_input_and_cond()
        # through the input conv and RightShift to the flow input (model.py:423-424)
        K.causal_conv1d_dgrad(self.gs[0], self.view("init_w"), self.dx_in.view(B, T, 1), 1, shift=1, accumulate=True)
        if overlap and join:
            main.wait_stream(side)


class StudentEngine:
    """``ParallelWaveNet``'s graph and training step (model.py:290-401, 490-535) over pre-allocated buffers."""

    def __init__(self, teacher: WaveNetEngine, flow_cfg: StackConfig, num_flows: int, alpha: float = 1.0,
                 beta: float = 1.0, gamma: float = 1.0, learning_rate: float = 1e-3, seed: int = 0,
                 process_group=None):
        if not teacher.mol or not teacher.E or not teacher.cfg.shift_input:
            raise ValueError("the teacher must be the conditioned mixture-of-logistics decoder (model.py:158-200)")
        if flow_cfg.cond_channels != teacher.E or flow_cfg.pool_stride != teacher.cfg.pool_stride:
            raise ValueError("flows and teacher share encoding_w_condition (model.py:318-324): cond_channels/pool_stride differ")
        self.teacher = teacher
        self.B, self.T, self.N = teacher.B, teacher.T, teacher.N
        self.loss_div = float(self.B)      # the loss divides by the number of noise rows fed (model.py:379)
        self.dev = teacher.dev
        if K.stft_frames(self.T) < 1:
            raise ValueError("clips must hold at least one 512-sample STFT frame (model.py:360)")
        self.alpha, self.beta, self.gamma, self.lr = float(alpha), float(beta), float(gamma), float(learning_rate)
        self.pg = process_group
        self.world = dp.world_size(process_group)
        self.F = int(num_flows)
        per = FlowStack.param_count(replace(flow_cfg, head_mode="flow"))
        self.storage = FlowStorage(per * self.F, self.dev)
        self.ctl = OptControls()      # training controls (optim.TrainControls) of the flows' one parameter buffer
        self.ctl.engines.add(self)
        self.flows: List[FlowStack] = [FlowStack(flow_cfg, self.B, self.T, device=self.dev, seed=seed + 101 * i,
                                                 storage=self.storage, slot=i) for i in range(self.F)]
        B, T, N = self.B, self.T, self.N
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.dev)
        self.noise, self.truth = z(B, T), z(B, T)
        self.out = z(N)                    # clip(x_F, -1, 1)  (model.py:535)
        self.dx = z(N)                     # d loss / d out, then d loss / d x_F
        nf = K.stft_frames(T)
        self.spec = z(B, nf, 257, 2); self.fpow = z(B, nf, 257)
        self.pow_truth, self.pow_out, self.dpow = z(B, 257), z(B, 257), z(B, 257)
        self.ce_parts = z((N + 255) // 256)
        self.ce, self.power, self.logs = z(1), z(1), z(1)
        self.sq_parts = z(K.sumsq_partials(self.storage.grads.numel()))
        self.clip = z(2)                   # [combined gradient scale, global norm]
        import os as _os
        self.tstream = torch.cuda.Stream() if _os.environ.get("SRWN_OVERLAP", "1") != "0" else None
        self.ent_all = z(self.F, K.flow_partials(N))
        for i, f in enumerate(self.flows):  # flow i reads flow i-1's output in place
            f.audio = self.noise if i == 0 else self.flows[i - 1].x_out.view(B, T)
            f.ent_parts = self.ent_all[i]

    # ------------------------------------------------------------------------------------------------
    def set_inputs(self, noise: torch.Tensor, truth: Optional[torch.Tensor], cond: torch.Tensor):
        """noise [B,T] logistic samples (student.py:100), truth [B,T], cond = encoding_w_condition [B,frames,E]."""
        self.noise.copy_(noise.reshape(self.B, self.T))
        if truth is not None:
            self.truth.copy_(truth.reshape(self.B, self.T))
            self.teacher.set_inputs(self.truth, None, cond)
        for f in self.flows:
            f.set_cond(cond)

    def forward_flows(self):
        """model.py:490-535: the flows and the clipped output; also sum(log s_tot) for the entropy."""
        for f in self.flows:
            f.forward()
        call("srwn_clamp", self.flows[-1].x_out.data_ptr(), self.out.data_ptr(), self.N, -1.0, 1.0, K._stream())
        # sum over flows and rows of prm0 = sum(log s_tot)  (model.py:517-519, 356)
        K.reduce_loss(self.ent_all, self.ent_all.numel(), 1.0, self.logs)

    def forward(self):
        """Teacher logits on the truth clip, the flows, and the three loss terms (model.py:356-379)."""
        B, T, N = self.B, self.T, self.N
        tch = self.teacher
        main = torch.cuda.current_stream()
        if self.tstream is not None:   # the frozen teacher depends on (truth, encoding) only: run it beside the flows
            self.tstream.wait_stream(main)
            with torch.cuda.stream(self.tstream):
                tch.forward(with_loss=False, train=False)              # logits32 [N, 4M] on RightShift(truth); forward only
        else:                                                          # (stop_gradient, model.py:334): no weight-gradient tiles
            tch.forward(with_loss=False, train=False)
        self.forward_flows()
        K.stft_power(self.truth, None, self.fpow, self.pow_truth)      # model.py:360,367
        K.stft_power(self.out.view(B, T), self.spec, self.fpow, self.pow_out)
        K.power_loss(self.pow_truth, self.pow_out, self.gamma, 1.0 / self.loss_div, self.dpow, self.power)
        if self.tstream is not None:
            main.wait_stream(self.tstream)
        K.mol_loss_dx(tch.logits32, self.out, tch.C // 4, self.ce_parts, self.dx, self.beta / self.loss_div)   # model.py:374
        K.reduce_loss(self.ce_parts, self.ce_parts.numel(), 1.0, self.ce)

    def losses(self) -> Dict[str, float]:
        """Host-side combination of the device scalars (model.py:356,371,375-379)."""
        ce, power, logs = float(self.ce.item()), float(self.power.item()), float(self.logs.item())
        entropy = logs + 2.0 * self.N
        return dict(loss=(self.beta * ce - self.alpha * entropy + power) / self.loss_div, power_loss=power,
                    entropy=entropy, cross_entropy=self.beta * ce)

    def backward(self):
        B, T, N = self.B, self.T, self.N
        K.stft_power_bwd(self.spec, self.dpow, self.dx.view(B, T), accumulate=True)
        # tf.minimum/maximum (model.py:535) pass the gradient where the pre-clip value lies in [-1, 1]
        call("srwn_clamp_bwd", self.flows[-1].x_out.data_ptr(), self.dx.data_ptr(), self.dx.data_ptr(), N, -1.0, 1.0,
             K._stream())
        g = self.dx
        for f in reversed(self.flows):
            f.backward(g, -self.alpha / self.loss_div, join=False)
            g = f.dx_in
        main = torch.cuda.current_stream()
        for f in self.flows:   # every flow's weight gradients must be in before the norm / update
            if f.side is not None and f.overlap and not f.timing and f.use_wl:
                main.wait_stream(f.side)

    def allreduce_grads(self):
        dp.allreduce_sum_(self.storage.grads, self.pg)

    def optimizer_step(self):
        """tf.clip_by_global_norm(grads, 1.0) + Adam over every flow's variables (model.py:382-385, 401); under data
        parallelism the flat buffer holds the SUM of the ranks' (loss / local B) gradients -> mean, then clip."""
        st = self.storage
        K.sumsq(st.grads, self.sq_parts)
        K.clip_scale(self.sq_parts, self._clip_norm(), 1.0 / self.world, self.clip)
        self._adam_update(1.0, self.clip)
        for f in self.flows:
            f.repack()

    def _adam_update(self, grad_scale, scale_dev):
        """The update launch of both training paths: srwn_adam_step(_scaled) at the fixed rate without controls,
        srwn_adam_step_ctl with them (``engine.adam_update``)."""
        st = self.storage
        adam_update(self.ctl, st.params, st.grads, st.adam_m, st.adam_v, st.adam_step, self.lr, grad_scale, scale_dev)

    def _clip_norm(self) -> float:
        """The reference clips at 1.0 (model.py:385); controls with a clip_norm replace it."""
        c = self.ctl.controls
        return 1.0 if c is None or c.clip_norm is None else c.clip_norm

    # -- training controls (optim.py) ----------------------------------------------------------------------
    @property
    def ema(self):
        return self.ctl.ema

    def set_controls(self, controls):
        """As ``WaveNetEngine.set_controls``, for the flows' shared buffer.  The student always clips (``self.clip``
        holds the factor and the norm): `clip_norm` None keeps the reference's 1.0, so clipping is no feature here."""
        if self.ctl.set(controls, self.storage.params):
            self.ctl.drop_graphs()

    def swap_ema(self):
        swap_with_ema(self.ctl, self.storage.params)
        for f in self.flows:
            f.repack()

    def train_step(self):
        self.forward()
        self.backward()
        self.allreduce_grads()
        self.optimizer_step()

    def train_per_sample(self):
        """``ParallelWaveNet.train`` (model.py:599-632), the slow path: for every noise row i the graph is run with
        ``inputs = [noise_i]`` against the WHOLE batch of encodings and truths (the 1-row noise broadcasts over them,
        ``h + upsampled`` at model.py:435), its loss divided by 1 row, its gradient clipped to norm 1 on its own;
        the clipped gradients are averaged and applied without further clipping.  Returns (mean loss, mean power)."""
        st = self.storage
        if not hasattr(self, "_acc"):
            self._acc = torch.zeros_like(st.grads)
            self._noise_all = torch.zeros_like(self.noise)
        self._noise_all.copy_(self.noise)
        self._acc.zero_()
        losses, powers = [], []
        keep = self.loss_div
        self.loss_div = 1.0
        try:
            for i in range(self.B):
                self.noise.copy_(self._noise_all[i:i + 1].expand(self.B, -1))
                self.forward()
                self.backward()
                K.sumsq(st.grads, self.sq_parts)
                K.clip_scale(self.sq_parts, self._clip_norm(), 1.0, self.clip)
                call("srwn_axpy_dev", self._acc.data_ptr(), st.grads.data_ptr(), self.clip.data_ptr(), 1.0 / self.B,
                     st.grads.numel(), K._stream())
                l = self.losses()
                losses.append(l["loss"]); powers.append(l["power_loss"])
        finally:
            self.loss_div = keep
            self.noise.copy_(self._noise_all)
        st.grads.copy_(self._acc)
        self.allreduce_grads()
        self._adam_update(1.0 / self.world, None)
        for f in self.flows:
            f.repack()
        return float(np.mean(losses)), float(np.mean(powers))

    def capture_graphs(self):
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


# ----------------------------------------------------------------------------------------------------------------------
# Inference: the flows as a chunked stream (csrc/srwn_stream.hip).  No teacher, no training buffers: per flow the weights,
# a StreamStack (one boundary buffer per layer group) and a conditioning table.
# ----------------------------------------------------------------------------------------------------------------------
def live_room(fed: int, t: int, hist_max: int, pool_stride: int, capacity: int) -> int:
    """How many frames a LIVE stream may be fed now.  Its conditioning tables are rings of ``capacity`` frames: frame f
    lives in row f mod capacity.  A chunk starting at time t recomputes the halo rows of group g back to t - hist_g, so
    the oldest frame still read is max(t - hist_max, 0) // pool_stride; a feed must not overwrite that frame or a newer
    one.  With ``fed`` frames written so far: max(0, capacity - fed + max(t - hist_max, 0) // pool_stride).  Feeding k
    frames at a time never stalls iff capacity >= ceil(hist_max / pool_stride) + k.  Pure Python: the CPU tests drive
    the fp64 oracle with it."""
    fed, t, hist_max, pool_stride, capacity = int(fed), int(t), int(hist_max), int(pool_stride), int(capacity)
    if fed < 0 or t < 0 or hist_max < 0 or pool_stride < 1 or capacity < 1 or t > fed * pool_stride:
        raise ValueError("live_room: fed=%d t=%d hist_max=%d pool_stride=%d capacity=%d" % (fed, t, hist_max, pool_stride, capacity))
    return max(0, capacity - fed + max(t - hist_max, 0) // pool_stride)


def live_min_frames(hist_max: int, pool_stride: int) -> int:
    """The smallest ring a live stream can run on one frame at a time: ceil(hist_max / pool_stride) + 1."""
    return -(-int(hist_max) // int(pool_stride)) + 1


class FlowWeights:
    """The weight side of one flow without the training engine around it: ``FlowStack``'s parameter layout, reference
    variable names and image packing (the forward images only), on buffers of its own."""

    layout = staticmethod(FlowStack.layout)
    param_count = staticmethod(FlowStack.param_count)
    view = WaveNetEngine.view
    wptr = WaveNetEngine.wptr
    named_tensors = FlowStack.named_tensors
    load_oracle_params = FlowStack.load_oracle_params

    def __init__(self, cfg: StackConfig, device="cuda"):
        self.cfg = cfg
        self.dev = torch.device(device)
        self.dt = cfg.dtype
        self.dil = [int(d) for d in cfg.dilations]
        self.L, self.R, self.Kw, self.E = len(self.dil), cfg.dilation_channels, cfg.filter_width, cfg.cond_channels
        self.S = cfg.skip_channels
        self.Ep = (self.E + 15) // 16 * 16
        self.sections = self.layout(cfg)
        self.nparams = self.param_count(cfg)
        self.params = torch.zeros(self.nparams, dtype=torch.float32, device=self.dev)
        # the variables a flow never reads (ops.py:31-33, 44) exist in checkpoints only: stride-0 host placeholders, so that
        # FlowStack.tf_variables can be asked for the names; `tf_variables` below drops them again
        ph = torch.zeros(1)
        L, R, S, Kw = self.L, self.R, self.S, self.Kw
        self.dead_gate = {"WG": ph.expand(L, Kw, R, R), "BG": ph.expand(L, R)}
        self.dead_skip = {"WS": ph.expand(L, R, S), "BS": ph.expand(L, S)}
        self.packed = None
        self._plan()

    def tf_variables(self, scope: str) -> Dict[str, torch.Tensor]:
        """Reference name -> tensor for the variables a flow reads (the dead gate and skip variables are left out)."""
        return {k: v for k, v in FlowStack.tf_variables(self, scope).items() if v.is_cuda}

    def _plan(self):
        from . import packing as P
        L, R, Kw, E, Ep, sec = self.L, self.R, self.Kw, self.E, self.Ep, self.sections
        pk = K.Packer(self.dev)
        self.o_conv = [P.pack_conv(pk, sec["WF"].offset + l * Kw * R * R, Kw, R) for l in range(L)]
        self.o_res = [P.pack_res(pk, sec["WR"].offset + l * R * R, R) for l in range(L)]
        self.o_wc = pk.reserve(L * R // 32, Ep // 16)      # every layer's conditioning 1x1 as one product (model.py:180)
        for l in range(L):
            P.fill_linear(pk, self.o_wc + l * (R // 32) * (Ep // 16) * 512, sec["WC"].offset + l * E * R, E, R,
                          R // 32, Ep // 16)
        self._pk = pk
        self.packed_elems = pk.total

    def repack(self):
        """The images from the current parameters.  The gather index is as large as the images and only needed here: it
        is built for the call and dropped."""
        if self.packed is None:
            self.packed = torch.zeros(self.packed_elems, dtype=self.dt, device=self.dev)
        self._pk.finalize()
        self._pk.gather(self.params, self.packed)
        torch.cuda.current_stream().synchronize()
        self._pk.idx = None


def _check_flow_cfg(flow_cfg: StackConfig):
    """What the flows' inference classes refuse about a configuration, before any device work."""
    if not flow_cfg.cond_channels:
        raise ValueError("a flow is conditioned on the encoding (model.py:431): cond_channels > 0")
    if flow_cfg.gate_mode != "reference":
        raise NotImplementedError("gate_mode %r is not built for the flows of ParallelWaveNet" % (flow_cfg.gate_mode,))
    if flow_cfg.filter_width != 2 or flow_cfg.dilation_channels not in (32, 64):
        raise NotImplementedError("flows: filter_width 2 and dilation_channels 32 / 64 are built")


def logistic_nll(noise: torch.Tensor, log_scale: torch.Tensor) -> torch.Tensor:
    """-log p(audio[t] | audio[< t]) in nats, from the two outputs of a ``FlowInverter``: the logistic(0, 1) base density
    of the student's noise (student.py:104) at z, -log f(z) = |z| + 2 log(1 + exp(-|z|)), plus log |d audio / d z| =
    the sum of the flows' log scales."""
    a = noise.abs()
    return a + 2.0 * torch.log1p(torch.exp(-a)) + log_scale


class InvertState:
    """One batch of streams of a ``FlowInverter`` (which holds the device side: an inverter serves one state at a time).
    ``t``: samples inverted so far; ``limit`` = frames * pool_stride."""

    def __init__(self, batch: int, frames: int, limit: int, serial: int, cond_all):
        self.B, self.frames, self.limit, self.t, self._serial = batch, frames, limit, 0, serial
        self.cond_all = cond_all      # per flow [L, B * frames, R]: cb of every layer and frame


class FlowInverter:
    """``num_flows`` flows (model.py:456-487) run backwards: audio in, the noise that makes it and log |d audio / d noise|
    out.  A flow's inverse is sequential (x_in[t] needs the stack's output on the recovered x_in[< t]), so a chunk costs one
    launch of csrc/srwn_flow_inv.hip per flow, the last flow first, each a persistent kernel that steps through the chunk
    on the queue-cached layer rings of the generators.  ``start`` a batch of streams on their encodings, then ``step`` it
    chunk by chunk; any cut into chunks gives the bits of one call.  weights: the ``FlowWeights`` to serve (a
    ``FlowSynthesizer``'s own: ``FlowSynthesizer.inverter``); default: new ones."""

    def __init__(self, flow_cfg: StackConfig, num_flows: int, max_batch: int = 1, device="cuda", weights=None):
        _check_flow_cfg(flow_cfg)
        if min(int(num_flows), int(max_batch)) < 1:
            raise ValueError("num_flows and max_batch must be >= 1")
        K._need_gpu()
        from . import _lib, packing as P
        import ctypes
        cfg = replace(flow_cfg, head_mode="flow", shift_input=True, output_channels=2)
        self.cfg, self.F, self.max_batch = cfg, int(num_flows), int(max_batch)
        self.dev, self.dt = torch.device(device), cfg.dtype
        self.L, self.R, self.E, self.pool_stride = len(cfg.dilations), cfg.dilation_channels, cfg.cond_channels, int(cfg.pool_stride)
        self.weights = list(weights) if weights is not None else [FlowWeights(cfg, self.dev) for _ in range(self.F)]
        if len(self.weights) != self.F:
            raise ValueError("%d FlowWeights for %d flows" % (len(self.weights), self.F))
        L, R, Kw = self.L, self.R, cfg.filter_width
        self._dil = (ctypes.c_int32 * L)(*[int(d) for d in cfg.dilations])
        # generation-order images, per layer [conv (last tap permuted) | residual] back to back (packing.pack_conv_gen)
        sec = self.weights[0].sections
        self._pk = K.Packer(self.dev)
        for l in range(L):
            P.pack_conv_gen(self._pk, sec["WF"].offset + l * Kw * R * R, Kw, R)
            P.pack_res(self._pk, sec["WR"].offset + l * R * R, R)
        z = lambda *s, dt=self.dt: torch.zeros(s, dtype=dt, device=self.dev)
        self.images = [z(self._pk.total) for _ in range(self.F)]
        self.groups = (self.max_batch + 31) // 32
        relems = int(_lib.load().srwn_generate_ring_elems(self._dil, L, R))
        self.rings = [z(self.groups * relems) for _ in range(self.F)]
        self.carry_all = z(self.F, self.max_batch, 2, dt=torch.float32)
        self._serial = 0
        self._state: Optional[InvertState] = None
        if weights is None:
            for w in self.weights:
                w.repack()
        self.repack()

    def repack(self):
        """The generation-order images from the weights' current parameters (after a load, or when the synthesizer that
        shares the weights was given new ones)."""
        self._pk.finalize()
        for w, img in zip(self.weights, self.images):
            self._pk.gather(w.params, img)
        torch.cuda.current_stream().synchronize()
        self._pk.idx = None

    # ------------------------------------------------------------------------------------------------
    def _check_cond(self, cond) -> torch.Tensor:
        cond = torch.as_tensor(cond, dtype=torch.float32)
        if cond.dim() != 3 or cond.shape[2] != self.E:
            raise ValueError("cond must be [batch, frames, %d], got %s" % (self.E, tuple(cond.shape)))
        if not 1 <= cond.shape[0] <= self.max_batch or cond.shape[1] < 1:
            raise ValueError("cond: %d streams x %d frames; this inverter holds max_batch=%d"
                             % (cond.shape[0], cond.shape[1], self.max_batch))
        return cond

    def start(self, cond) -> InvertState:
        """cond [B <= max_batch, frames, E] (encoding_w_condition) -> a state at clock 0: zero rings, zero carries."""
        cond = self._check_cond(cond)
        B, frames = int(cond.shape[0]), int(cond.shape[1])
        rows, st = B * frames, K._stream()
        Ep = self.weights[0].Ep
        cin = torch.zeros((rows, Ep), dtype=self.dt, device=self.dev)
        cin[:, :self.E].copy_(cond.reshape(rows, self.E).to(self.dev))
        cond_all = []
        for w, ring in zip(self.weights, self.rings):      # cb of every layer and frame (model.py:180), as FlowSynthesizer.start
            ca = torch.empty((self.L, rows, self.R), dtype=self.dt, device=self.dev)
            call("srwn_pw_linear_ychunks", cin.data_ptr(), Ep, Ep, w.wptr(w.o_wc), w.view("BC").reshape(-1).data_ptr(),
                 ca.data_ptr(), self.R, self.R, rows * self.R, self.L * self.R, self.L * self.R, rows, K.abi_dtype(self.dt), st)
            cond_all.append(ca)
            ring.zero_()
        self.carry_all.zero_()
        self._serial += 1
        self._state = InvertState(B, frames, frames * self.pool_stride, self._serial, cond_all)
        return self._state

    def step(self, state: InvertState, audio, want_params: bool = False):
        """The next n samples of every stream: audio [B, n] (taken as the flows' unclipped output) -> (noise [B, n],
        log_scale [B, n] = the sum over the flows of p0) fp32; want_params: also (prm, x_in), per flow the [B, n, 2]
        parameters and the [B, n] recovered input.  Refuses (ValueError, state untouched) a state that is not the current
        one and steps past frames * pool_stride."""
        if state is not self._state or state._serial != self._serial:
            raise ValueError("this state is not the inverter's current one (start() began another)")
        y = torch.as_tensor(audio, dtype=torch.float32)
        if y.dim() != 2 or y.shape[0] != state.B:
            raise ValueError("audio must be [%d, n], got %s" % (state.B, tuple(y.shape)))
        B, n = state.B, int(y.shape[1])
        if state.t + n > state.limit:
            raise ValueError("chunk of %d samples at %d: the encoding ends at frames * pool_stride = %d"
                             % (n, state.t, state.limit))
        y = y.to(self.dev).contiguous()
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.dev)
        xs, prms = [None] * self.F, [None] * self.F
        st, dt = K._stream(), K.abi_dtype(self.dt)
        for i in range(self.F - 1, -1, -1):      # the last flow first; each reads what the launch before recovered
            w, ca = self.weights[i], state.cond_all[i]
            v = w.view
            xs[i], prms[i] = z(B, n), z(B, n, 2)
            call("srwn_flow_invert", self.images[i].data_ptr(), v("BF").data_ptr(), v("BR").data_ptr(),
                 v("init_w").data_ptr(), v("init_b").data_ptr(), v("flow_w").data_ptr(), v("flow_b").data_ptr(),
                 self.rings[i].data_ptr(), y.data_ptr(), xs[i].data_ptr(), prms[i].data_ptr(), self._dil, self.L, B, n, n,
                 self.R, self.cfg.filter_width, ca.data_ptr(), state.frames, self.pool_stride, self.R,
                 ca.shape[1] * self.R, dt, st, state.t, self.carry_all[i].data_ptr())
            y = xs[i]
        state.t += n
        log_scale = prms[0][:, :, 0].clone()
        for p in prms[1:]:
            log_scale += p[:, :, 0]
        return (xs[0], log_scale, prms, xs) if want_params else (xs[0], log_scale)

    def invert(self, audio, cond, want_params: bool = False):
        """``start(cond)`` and one ``step`` over the whole of audio [B, T]."""
        cond = self._check_cond(cond)
        return self.step(self.start(cond), audio, want_params)


class SynthState:
    """One batch of streams of a ``FlowSynthesizer`` (which holds the device side: a synthesizer serves one state at a
    time).  ``t``: samples made so far; ``limit`` = frames * pool_stride.  A ``live`` state is fed its frames while it runs
    (``FlowSynthesizer.feed``): ``fed`` frames so far, ``limit`` = fed * pool_stride."""

    def __init__(self, batch: int, frames: int, limit: int, serial: int, live: bool = False):
        self.B, self.frames, self.limit, self.t, self._serial = batch, frames, limit, 0, serial
        self.live, self.fed = bool(live), frames


class FlowSynthesizer:
    """``num_flows`` flows (model.py:415-535) as a streaming synthesizer: ``start`` a batch of streams on their
    encodings, then ``step`` it chunk by chunk.  Per chunk and flow: one entry launch, one launch per layer group, one
    exit launch (+ one noise launch per chunk); the sequence of a (batch, chunk size) is captured as a hipGraph when it
    is used a second time and replayed from then on (SRWN_MODEL_GRAPHS=0: eager launches).  ``pool`` serves the same
    buffers as slots that streams join and leave while the batch runs (``SynthPool``).  ``start(..., live=True)`` begins
    streams that are handed their frames while they run (``feed`` / ``room``): the conditioning tables then serve as
    rings of ``max_frames`` frames and a stream has no bound on its length."""

    def __init__(self, flow_cfg: StackConfig, num_flows: int, max_batch: int = 1, max_chunk: int = 1600,
                 max_frames: int = 32, device="cuda"):
        K._need_gpu()
        _check_flow_cfg(flow_cfg)
        if min(int(num_flows), int(max_batch), int(max_chunk), int(max_frames)) < 1:
            raise ValueError("num_flows, max_batch, max_chunk and max_frames must be >= 1")
        cfg = replace(flow_cfg, head_mode="flow", shift_input=True, output_channels=2)
        self.cfg, self.F = cfg, int(num_flows)
        self.max_batch, self.max_chunk, self.max_frames = int(max_batch), int(max_chunk), int(max_frames)
        self.dev, self.dt = torch.device(device), cfg.dtype
        self.L, self.R, self.E, self.pool_stride = len(cfg.dilations), cfg.dilation_channels, cfg.cond_channels, int(cfg.pool_stride)
        self.weights = [FlowWeights(cfg, self.dev) for _ in range(self.F)]
        Bm, C, R = self.max_batch, self.max_chunk, self.R
        z = lambda *s, dt=self.dt: torch.zeros(s, dtype=dt, device=self.dev)
        self.top = z(Bm, C, R)                                # every flow's last layer in its turn, chunk rows only
        self.stacks = [StreamStack(w, Bm, C, store_z=False, top=self.top) for w in self.weights]
        self.groups, self.hist = self.stacks[0].groups, self.stacks[0].hist
        self.bufs, self.roll = [sk.bufs for sk in self.stacks], [sk.roll for sk in self.stacks]
        self.rows_c = Bm * self.max_frames
        self.cond_in = z(self.rows_c, self.weights[0].Ep)
        self.cond_all = [z(self.L, self.rows_c, R) for _ in range(self.F)]
        self.xbuf = [z(Bm, C, dt=torch.float32) for _ in range(self.F + 1)]           # noise, x_1 .. x_F
        self.carry_all = z(self.F, Bm, 2, dt=torch.float32)
        self.carry = [self.carry_all[i] for i in range(self.F)]
        self.seeds = torch.zeros(Bm, dtype=torch.int64, device=self.dev)
        self.temps = z(Bm, dt=torch.float32)
        self.clock = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.roll_all = torch.cat(self.roll, 0).contiguous()      # every flow's table in one (a pool join resets through it)
        self._graphs: Dict[tuple, object] = {}
        self._seen: set = set()
        self._serial = 0
        self._state: Optional[SynthState] = None
        self._pool: Optional["SynthPool"] = None
        self.use_graphs = os.environ.get("SRWN_MODEL_GRAPHS", "1") != "0"
        self.launches_per_chunk = 1 + self.F * (2 + len(self.groups))
        for w in self.weights:
            w.repack()

    def repack(self):
        for w in self.weights:
            w.repack()

    def inverter(self, max_batch: Optional[int] = None) -> "FlowInverter":
        """A ``FlowInverter`` on this synthesizer's own ``FlowWeights``: both directions serve one snapshot (after new
        parameters and ``repack`` here, call the inverter's ``repack`` too)."""
        return FlowInverter(self.cfg, self.F, max_batch=self.max_batch if max_batch is None else max_batch,
                            device=self.dev, weights=self.weights)

    # ------------------------------------------------------------------------------------------------
    def start(self, cond, seeds=0, temperature=1.0, live=False, batch=None) -> SynthState:
        """cond [B, frames <= max_frames, E] (encoding_w_condition) -> a state at clock 0: zero history, zero carry.
        seeds / temperature: one value per stream, or a scalar (seed s: stream b draws with s + b).
        live=True: the encoding arrives while the stream runs (``feed``); cond is None (`batch` streams, default 1) or the
        first frames, and the conditioning tables serve as rings of max_frames frames (``live_room``)."""
        if live:
            need = live_min_frames(max(self.hist), self.pool_stride)
            if self.max_frames < need:
                raise ValueError("a live stream needs a ring of max_frames >= ceil(%d / %d) + 1 = %d frames, this synthesizer "
                                 "holds %d" % (max(self.hist), self.pool_stride, need, self.max_frames))
            if cond is None:
                cond = torch.zeros((1 if batch is None else int(batch), 0, self.E), dtype=torch.float32)
        cond = torch.as_tensor(cond, dtype=torch.float32)
        if cond.dim() != 3 or cond.shape[2] != self.E:
            raise ValueError("cond must be [batch, frames, %d], got %s" % (self.E, tuple(cond.shape)))
        B, frames = int(cond.shape[0]), int(cond.shape[1])
        if not 1 <= B <= self.max_batch or not (0 if live else 1) <= frames <= self.max_frames:
            raise ValueError("cond: %d streams x %d frames; this synthesizer holds max_batch=%d, max_frames=%d"
                             % (B, frames, self.max_batch, self.max_frames))
        sd = np.asarray(seeds)
        sd = (int(sd) + np.arange(B)) if sd.ndim == 0 else sd.reshape(-1)
        tp = np.asarray(temperature, dtype=np.float64)
        tp = np.full(B, float(tp)) if tp.ndim == 0 else tp.reshape(-1)
        if sd.shape[0] != B or tp.shape[0] != B:
            raise ValueError("seeds / temperature: one value per stream (%d) or a scalar" % B)
        if not np.all(np.isfinite(tp)) or np.any(tp < 0):
            raise ValueError("temperature must be finite and >= 0")
        self.seeds[:B].copy_(torch.as_tensor(np.asarray([int(s) & 0x7fffffffffffffff for s in sd], dtype=np.int64)))
        self.temps[:B].copy_(torch.as_tensor(tp.astype(np.float32)))
        self.cond_in.zero_()
        st = K._stream()
        if not live:
            self.cond_in.view(self.max_batch, self.max_frames, -1)[:B, :frames, :self.E].copy_(cond.to(self.dev))
        for i, w in enumerate(self.weights):      # cb of every layer and frame (model.py:180), one product per flow
            if not live:
                call("srwn_pw_linear_ychunks", self.cond_in.data_ptr(), w.Ep, w.Ep, w.wptr(w.o_wc),
                     w.view("BC").reshape(-1).data_ptr(), self.cond_all[i].data_ptr(), self.R, self.R, self.rows_c * self.R,
                     self.L * self.R, self.L * self.R, self.rows_c, K.abi_dtype(self.dt), st)
            self.stacks[i].reset()
            self.carry[i].zero_()
        self.clock.zero_()
        self._serial += 1
        if self._pool is not None:      # the buffers serve one of the two at a time
            self._pool._open = False
            self._pool = None
        self._state = SynthState(B, 0 if live else frames, 0 if live else frames * self.pool_stride, self._serial, live)
        if live and frames:
            self.feed(self._state, cond)
        return self._state

    def _check_state(self, state):
        if state is not self._state or state._serial != self._serial:
            raise ValueError("this state is not the synthesizer's current one (start() began another)")

    def room(self, state: SynthState) -> int:
        """Frames a live state may be fed now (``live_room``); 0 for a state that got its encoding at ``start``."""
        self._check_state(state)
        if not state.live:
            return 0
        return live_room(state.fed, state.t, max(self.hist), self.pool_stride, self.max_frames)

    def _ring_feed(self, streams, first, counts, max_k):
        """srwn_cond_ring_feed, one launch per flow: frames [first_i, first_i + counts_i) of the named streams, staged in
        ``cond_in`` [max_batch, max_frames, Ep] (stream u's new frames in rows 0.. of its block), into every flow's ring."""
        n = len(streams)
        host = np.empty(2 * n, np.int64)           # one upload: first [n] int64 | streams [n] int32 | counts [n] int32
        host[:n] = first
        i32 = host[n:].view(np.int32)
        i32[:n], i32[n:] = streams, counts
        dev = torch.from_numpy(host).to(self.dev)
        base, st = dev.data_ptr(), K._stream()
        for i, w in enumerate(self.weights):
            call("srwn_cond_ring_feed", self.cond_in.data_ptr(), w.Ep, self.max_frames, w.Ep, w.wptr(w.o_wc),
                 w.view("BC").reshape(-1).data_ptr(), self.cond_all[i].data_ptr(), self.L, self.R, self.max_frames,
                 self.max_batch, base + 8 * n, base, base + 12 * n, n, int(max_k), K.abi_dtype(self.dt), st)

    def feed(self, state: SynthState, frames) -> None:
        """The next k frames of every stream of a live state: frames [B, k, E] (encoding_w_condition).  A device tensor is
        taken as it is: no host copy, no synchronisation.  Refuses (ValueError, state untouched) a state that is not live
        and k > ``room``.  Afterwards ``step`` may run up to fed * pool_stride."""
        self._check_state(state)
        if not state.live:
            raise ValueError("feed: this state got its whole encoding at start (start(..., live=True) begins a live one)")
        fr = torch.as_tensor(frames, dtype=torch.float32)
        if fr.dim() != 3 or fr.shape[0] != state.B or fr.shape[2] != self.E:
            raise ValueError("feed: frames must be [%d, k, %d], got %s" % (state.B, self.E, tuple(fr.shape)))
        k = int(fr.shape[1])
        if k == 0:
            return
        room = self.room(state)
        if k > room:
            raise ValueError("feed: %d frames, but the ring of %d has room for %d at t = %d with %d fed"
                             % (k, self.max_frames, room, state.t, state.fed))
        B = state.B
        self.cond_in.view(self.max_batch, self.max_frames, -1)[:B, :k, :self.E].copy_(fr)
        self._ring_feed(np.arange(B), np.full(B, state.fed), np.full(B, k), k)
        state.fed += k
        state.frames = state.fed
        state.limit = state.fed * self.pool_stride

    def pool(self) -> "SynthPool":
        """A ``SynthPool`` on this synthesizer's buffers: max_batch slots, each a stream at a clock of its own.  The current
        ``SynthState`` (and an earlier pool) ends here, as at ``start``; ``start`` closes the pool."""
        K._need_gpu()
        if self._pool is not None:
            self._pool._open = False
        self._serial += 1
        self._state = None
        self._pool = SynthPool(self)
        return self._pool

    def _launch_chunk(self, B: int, n: int, device_noise: bool, pool: Optional["SynthPool"] = None):
        """The 1 + F x (2 + G) launches of a chunk.  pool: the slot forms, on the pool's table instead of the clock."""
        st, dt, R, C = K._stream(), K.abi_dtype(self.dt), self.R, self.max_chunk
        slots = pool is not None
        sfx = "_slots" if slots else ""
        ck = pool.slots.data_ptr() if slots else self.clock.data_ptr()
        if device_noise:
            call("srwn_logistic_noise" + sfx, self.xbuf[0].data_ptr(), C, self.temps.data_ptr(), self.seeds.data_ptr(), ck, B, n, st)
        for i, w in enumerate(self.weights):
            v, ca = w.view, self.cond_all[i]
            call("srwn_flow_stream_in" + sfx, self.xbuf[i].data_ptr(), C, self.carry[i].data_ptr(), v("init_w").data_ptr(),
                 v("init_b").data_ptr(), ca[0].data_ptr(), self.max_frames, self.pool_stride, R, self.bufs[i][0].data_ptr(),
                 self.hist[0] + C, self.hist[0], B, n, C, R, dt, ck, st)
            above = [ca[l + 1].data_ptr() if l + 1 < self.L else None for l in range(self.L)]      # layer l adds layer l + 1's
            self.stacks[i].launch_groups(B, n, ck, slots, (above, self.max_frames, self.pool_stride, R))
            lastf = i + 1 == self.F
            tail = (ck, pool.arrive.data_ptr()) if slots else (ck,)
            call("srwn_flow_stream_out" + sfx, self.top.data_ptr(), C, v("flow_w").data_ptr(), v("flow_b").data_ptr(),
                 self.xbuf[i].data_ptr(), self.xbuf[i + 1].data_ptr(), C, self.carry[i].data_ptr(), 1 if lastf else 0,
                 self.roll[i].data_ptr(), len(self.groups), B, n, C, R, dt, *tail, 1 if lastf else 0, st)

    def step(self, state: SynthState, n: int, noise=None) -> torch.Tensor:
        """The next n samples of every stream: [B, n] fp32 in [-1, 1].  noise [B, n]: the first flow's input instead of the
        device draw.  Refuses (ValueError, state untouched) n outside 1..max_chunk and steps past frames * pool_stride."""
        self._check_state(state)
        n = int(n)
        if not 1 <= n <= self.max_chunk:
            raise ValueError("chunk of %d samples: 1..max_chunk = %d" % (n, self.max_chunk))
        if state.t + n > state.limit:
            raise ValueError("chunk of %d samples at %d: the encoding ends at frames * pool_stride = %d"
                             % (n, state.t, state.limit))
        B = state.B
        if noise is not None:
            nz = torch.as_tensor(noise, dtype=torch.float32)
            if tuple(nz.shape) != (B, n):
                raise ValueError("noise must be [%d, %d], got %s" % (B, n, tuple(nz.shape)))
            self.xbuf[0][:B, :n].copy_(nz.to(self.dev))
        K.run_cached_graph(self._graphs, self._seen, (B, n, noise is None), self.use_graphs,      # per (batch, chunk size)
                           lambda: self._launch_chunk(B, n, noise is None))
        state.t += n
        return self.xbuf[self.F][:B, :n].clone()


class SynthPool(SlotTable):
    """``FlowSynthesizer.pool()``: the synthesizer's ``max_batch`` rows as SLOTS, each holding a stream at a clock of its
    own (srwn.h, SrwnSynthSlot).  Streams ``join`` free slots with their encodings, seeds and temperatures, ``step`` runs
    every live slot with the launches of one synthesizer chunk, and a stream that reaches its end or ``leave``s frees its
    slot for the next one.  A stream has, bit for bit, the samples of a batch-of-one ``FlowSynthesizer`` run with its
    encoding, seed and temperature -- in any slot, whenever it joined, whatever the chunk sizes and the other slots."""

    def __init__(self, syn: "FlowSynthesizer"):
        K._need_gpu()
        self.syn, self.capacity = syn, syn.max_batch
        self.frames, self.pool_stride, self.E = syn.max_frames, syn.pool_stride, syn.E
        self._t = np.zeros(self.capacity, np.int64)          # host mirror of the device table (the kernel advances both)
        self._end = np.zeros(self.capacity, np.int64)
        self._active = np.zeros(self.capacity, bool)
        self._live = np.zeros(self.capacity, bool)           # live slots: fed while they run; t_end = fed * pool_stride
        self._closed = np.zeros(self.capacity, bool)         # ... until closed: no more frames will come
        self._fed = np.zeros(self.capacity, np.int64)
        self.slots = torch.zeros((self.capacity, 2), dtype=torch.int64, device=syn.dev)      # [t, t_end] per slot
        self.arrive = torch.zeros(1, dtype=torch.int32, device=syn.dev)      # the last flow's exit launch counts its workgroups here
        self._graphs: Dict[tuple, object] = {}
        self._seen: set = set()
        self._open = True

    # ---- inspection
    @property
    def t(self) -> np.ndarray:
        """Each slot's own time of its next sample."""
        return self._t.copy()

    def _check_open(self):
        if not self._open:
            raise ValueError("this pool is closed (the synthesizer started a batch or opened another pool)")

    def _upload(self):
        """The host mirrors -> the device table, after join and leave.  The exit launch's workgroup counter is put back to
        zero with it: a launch that completed left it at zero, one that failed may not have."""
        self.slots.copy_(torch.from_numpy(np.stack([self._t, self._end], 1)))
        self.arrive.zero_()

    def _check_join(self, cond, seeds, temperature, max_samples, slots, live=False):
        """Everything join refuses, before any device work: (encodings as float32 tensors, seeds, temperatures, the chosen
        slots, t_end per stream)."""
        self._check_open()
        if live:
            need = live_min_frames(max(self.syn.hist), self.pool_stride)
            if self.frames < need:
                raise ValueError("join: a live stream needs a ring of max_frames >= ceil(%d / %d) + 1 = %d frames, this "
                                 "synthesizer holds %d" % (max(self.syn.hist), self.pool_stride, need, self.frames))
            if max_samples is not None:
                raise ValueError("join: a live stream ends where close() finds it; max_samples is for bounded streams")
            if cond is None:
                cond = [None]
        if isinstance(cond, (torch.Tensor, np.ndarray)) and cond.ndim == 2:
            cond = [cond]
        cond = [torch.zeros((0, self.E)) if (live and c is None) else
                c.detach().to("cpu", torch.float32) if isinstance(c, torch.Tensor) else torch.as_tensor(np.asarray(c, dtype=np.float32))
                for c in cond]
        n = len(cond)
        if n < 1:
            raise ValueError("join: no streams")
        for i, c in enumerate(cond):
            if c.dim() != 2 or c.shape[1] != self.E or not (0 if live else 1) <= c.shape[0] <= self.frames:
                raise ValueError("join: cond %d must be [%d..%d frames, %d], got %s"
                                 % (i, 0 if live else 1, self.frames, self.E, tuple(c.shape)))
        sd = np.asarray(seeds)
        sd = [int(sd) + i for i in range(n)] if sd.ndim == 0 else [int(s) for s in per_stream(seeds, n, "seeds", default=0)]
        tp = [float(v) for v in per_stream(temperature, n, "temperatures", default=1.0)]
        if not np.all(np.isfinite(tp)) or any(v < 0 for v in tp):
            raise ValueError("join: temperature must be finite and >= 0")
        ends = []
        for c, m in zip(cond, per_stream(max_samples, n, "max_samples")):
            lim = int(c.shape[0]) * self.pool_stride
            if m is not None and int(m) < 0:
                raise ValueError("join: max_samples %d" % int(m))
            ends.append(lim if m is None else min(lim, int(m)))
        return cond, sd, tp, self._take_slots(n, slots), ends

    def join(self, cond, seeds=0, temperature=None, max_samples=None, slots=None, live=False) -> List[int]:
        """n streams into free slots (the lowest ones, or `slots`): cond n encodings [frames_i <= max_frames, E]; seeds one
        per stream or a scalar s (stream i draws with s + i); temperature None (1), a scalar or one per stream;
        max_samples None, one int or n entries: a stream ends at min(frames_i * pool_stride, max_samples).  Writes the
        joined slots' seeds, temperatures and rows of every flow's conditioning table (srwn_pw_linear_ychunks on those rows)
        and zeroes their history rows and carries (srwn_flow_stream_reset_slots); returns the slots.
        live=True: the streams are fed while they run (``feed``): cond holds each stream's first frames (None or an entry
        None: no frame yet), their table rows serve as rings of max_frames frames and are written by srwn_cond_ring_feed; a
        live stream that has used up its frames is STARVED, not ended: it stays active with ran = 0 until it is fed,
        closed (``close``: it ends where its frames end) or left."""
        cond, sd, tp, slots, ends = self._check_join(cond, seeds, temperature, max_samples, slots, live)
        syn, n = self.syn, len(cond)
        dev, Fm, st = syn.dev, syn.max_frames, K._stream()
        dst = torch.tensor(slots, dtype=torch.int64, device=dev)
        syn.seeds[dst] = torch.tensor([s & 0x7fffffffffffffff for s in sd], dtype=torch.int64).to(dev)
        syn.temps[dst] = torch.tensor(tp, dtype=torch.float32).to(dev)
        cin = syn.cond_in.view(syn.max_batch, Fm, -1)
        for u, c in zip(slots, cond):
            cin[u].zero_()
            cin[u, :c.shape[0], :self.E].copy_(c.to(dev))
        order = sorted(slots)
        runs, u0 = [], order[0]
        for a, b in zip(order, order[1:] + [None]):      # neighbouring slots share a product
            if b != a + 1:
                runs.append((u0, a + 1 - u0))
                u0 = b
        esz = syn.cond_in.element_size()
        if live:      # the first frames enter the rings as every later one does
            runs = []
            ks = [int(c.shape[0]) for c in cond]
            if max(ks) > 0:
                syn._ring_feed(np.asarray(slots), np.zeros(n, np.int64), np.asarray(ks), max(ks))
        for i, w in enumerate(syn.weights):
            for u0, k in runs:
                call("srwn_pw_linear_ychunks", syn.cond_in.data_ptr() + u0 * Fm * w.Ep * esz, w.Ep, w.Ep, w.wptr(w.o_wc),
                     w.view("BC").reshape(-1).data_ptr(), syn.cond_all[i].data_ptr() + u0 * Fm * syn.R * esz, syn.R, syn.R,
                     syn.rows_c * syn.R, syn.L * syn.R, syn.L * syn.R, k * Fm, K.abi_dtype(syn.dt), st)
        ids = dst.to(torch.int32)
        call("srwn_flow_stream_reset_slots", syn.roll_all.data_ptr(), syn.roll_all.shape[0], syn.carry_all.data_ptr(), syn.F,
             syn.max_batch * 2, ids.data_ptr(), n, self.capacity, syn.R, K.abi_dtype(syn.dt), st)
        for u, e, c in zip(slots, ends, cond):
            self._t[u], self._end[u] = 0, e
            self._active[u] = live or e > 0
            self._live[u], self._closed[u], self._fed[u] = live, False, int(c.shape[0]) if live else 0
        self._upload()
        return list(slots)

    # ---- live slots
    def room(self, slot: int) -> int:
        """Frames a live slot may be fed now (``live_room``); 0 for every other slot."""
        self._check_open()
        u, = self._slot_list(slot, "room")
        if not (self._active[u] and self._live[u]) or self._closed[u]:
            return 0
        return live_room(int(self._fed[u]), int(self._t[u]), max(self.syn.hist), self.pool_stride, self.frames)

    def feed(self, slots, frames) -> None:
        """The next frames of live slots: frames[i] [k_i, E] for slots[i] (device tensors are taken as they are).  One
        srwn_cond_ring_feed per flow however many slots are fed; each slot's t_end grows to fed * pool_stride, on the host
        mirror and the device table together.  Refuses (ValueError, nothing changed) a slot that is not a live, open stream
        and k_i > room(slot).  The other slots are not touched."""
        self._check_open()
        slots = self._slot_list(slots, "feed")
        if isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 2:
            frames = [frames]
        frames = [torch.as_tensor(f, dtype=torch.float32) for f in frames]
        if len(frames) != len(slots) or len(set(slots)) != len(slots):
            raise ValueError("feed: %d distinct slots need one [k, %d] each, got %d" % (len(slots), self.E, len(frames)))
        for u, f in zip(slots, frames):
            if not (self._active[u] and self._live[u]) or self._closed[u]:
                raise ValueError("feed: slot %d holds no live, open stream" % u)
            if f.dim() != 2 or f.shape[1] != self.E:
                raise ValueError("feed: frames of slot %d must be [k, %d], got %s" % (u, self.E, tuple(f.shape)))
            if f.shape[0] > self.room(u):
                raise ValueError("feed: %d frames for slot %d, but its ring of %d has room for %d at t = %d with %d fed"
                                 % (f.shape[0], u, self.frames, self.room(u), self._t[u], self._fed[u]))
        pairs = [(u, f) for u, f in zip(slots, frames) if f.shape[0] > 0]
        if not pairs:
            return
        syn = self.syn
        cin = syn.cond_in.view(syn.max_batch, syn.max_frames, -1)
        for u, f in pairs:
            cin[u, :f.shape[0], :self.E].copy_(f)
        ks = [int(f.shape[0]) for _, f in pairs]
        us = [u for u, _ in pairs]
        syn._ring_feed(np.asarray(us), self._fed[us].copy(), np.asarray(ks), max(ks))
        for u, k in zip(us, ks):
            self._fed[u] += k
            self._end[u] = self._fed[u] * self.pool_stride
        self._upload()

    def close(self, slots) -> None:
        """No more frames will come for the live streams in `slots`: each frees its slot at the end of what it was fed,
        like a bounded stream (at once when it is already there)."""
        self._check_open()
        for u in self._slot_list(slots, "close"):
            if self._active[u] and self._live[u]:
                self._closed[u] = True
                self._active[u] = self._t[u] < self._end[u]

    def leave(self, slots) -> None:
        """Ends the streams in `slots` (a slot already free stays free) and frees their slots."""
        self._check_open()
        for u in self._slot_list(slots, "leave"):
            self._active[u] = False
            self._live[u] = False
            self._end[u] = self._t[u]
        self._upload()

    def step(self, n: int, noise=None):
        """The next n samples of every live slot, with the launches of one synthesizer chunk: (audio [capacity, n] f32,
        ran [capacity] int64 numpy).  Slot u's samples are row u's first ran[u] entries; the rest of every row is zero.
        noise [capacity, n]: the first flow's input instead of the device draw (every slot).  Slots whose stream reached its
        end become free.  With no live slot nothing is launched."""
        self._check_open()
        syn, n = self.syn, int(n)
        if not 1 <= n <= syn.max_chunk:
            raise ValueError("chunk of %d samples: 1..max_chunk = %d" % (n, syn.max_chunk))
        B = self.capacity
        nz = None
        if noise is not None:
            nz = torch.as_tensor(noise, dtype=torch.float32)
            if tuple(nz.shape) != (B, n):
                raise ValueError("noise must be [capacity = %d, %d], got %s" % (B, n, tuple(nz.shape)))
        ran = np.clip(self._end - self._t, 0, n)
        if not ran.any():
            return torch.zeros((B, n), dtype=torch.float32, device=syn.dev), ran
        if nz is not None:
            syn.xbuf[0][:, :n].copy_(nz.to(syn.dev))
        K.run_cached_graph(self._graphs, self._seen, (n, noise is None), syn.use_graphs,      # per chunk size
                           lambda: syn._launch_chunk(B, n, noise is None, self))
        self._t += ran
        self._active &= (self._t < self._end) | (self._live & ~self._closed)      # a starved live slot stays
        return syn.xbuf[syn.F][:, :n].clone(), ran
