/* srwn.h -- C-ABI of libsrwn.so: MI355X (gfx950) kernels for the WaveNet residual-stack hot path.
 *
 * The reference (tachitachi/SR-WaveNet, TensorFlow 1.x Python) has NO native/FFI interface; its
 * seam is the Python call surface of ops.py / model.py.  Each entry point below names the
 * reference function (file:line under /root/reference) whose arithmetic it replaces; the host
 * mirror of that Python surface lives in sr-wavenet_amd/{ops,model}.py and binds this header
 * through the pybind11 module build.py generates from it (_srwn_pyb; ctypes on request:
 * SRWN_BINDING=ctypes) -- see INTEGRATION.md.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller; nothing is allocated or freed here;
 *  - `stream` is a hipStream_t passed as void*; launches are asynchronous on it; no call
 *    synchronises, so every entry point may be captured into a hipGraph;
 *  - return value: 0 = ok, >0 = hipError_t of the launch, <0 = argument error (SRWN_E_*);
 *    srwn_last_error() returns a thread-local message for the last non-zero return;
 *  - tensors are channels-last [B,T,C] / [rows,C] (ops.py:4); master weights are fp32 in the
 *    reference's own shapes ([K,Cin,Cout] conv kernels, ops.py:5; [1,Cin,Cout] tf.layers.conv1d);
 *  - `dtype` selects the activation/compute type: SRWN_F32 (exact fp32 MFMA, parity mode) or
 *    SRWN_BF16 (bf16 MFMA, fp32 accumulate, throughput mode);
 *  - "packed" weights are MFMA A-operand fragment images built by srwn_pack_a_index +
 *    srwn_pack_gather from the fp32 master weights (layout: csrc/srwn_common.h).
 */
#ifndef SRWN_H
#define SRWN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRWN_F32 0
#define SRWN_BF16 1

#define SRWN_E_DTYPE (-1)
#define SRWN_E_SHAPE (-2)
#define SRWN_E_NULL (-3)
#define SRWN_E_UNSUPPORTED (-4)

/* pw_linear prologue / epilogue selectors */
#define SRWN_PRO_NONE 0
#define SRWN_PRO_GATE 1 /* x -> x*sigmoid(x): rebuilds c = z*sigmoid(z) from stored z (ops.py:33,36) */
#define SRWN_EPI_NONE 0
#define SRWN_EPI_RELU 1
#define SRWN_EPI_MASK 2 /* y *= (aux > 0): relu backward against the saved activation */
#define SRWN_EPI_F32 4  /* y is fp32 regardless of dtype (mixture-of-logistics parameters need full precision) */

int srwn_version(void);
const char* srwn_last_error(void);

/* ---- mu-law companding: ops.py:82-93 (encode) and ops.py:96-104 (decode); bit-exact vs the
 *      oracle (log1p/pow evaluated in f64 and rounded once, every other step an IEEE f32 op). */
int srwn_mu_law_encode(const float* audio, int32_t* codes, int64_t n, int32_t quantization_channels, void* stream);
int srwn_mu_law_decode(const int32_t* codes, float* audio, int64_t n, int32_t quantization_channels, void* stream);

/* ---- weight packing (no reference counterpart: TF keeps [K,Cin,Cout] and lets cuDNN/Eigen relayout)
 * srwn_pack_a_index writes, for an A operand with `mt_count` 32-row tiles and k-steps
 * [ks_offset, ks_offset+ks_count) of a packed image whose k extent is `ks_total` steps, the int32
 * source index   src_offset + row*row_stride + k*k_stride   of every fragment element
 * (row = output channel, k = contraction index local to this call), or -1 where row >= rows_valid
 * or k >= k_valid (zero padding).  k-steps >= perm_from_ks (local) use the permuted k order.
 * idx image: [mt_count][ks_total][64 lanes][8] int32, written at dst_idx.
 * srwn_pack_gather then materialises dst[i] = (dtype) src[idx[i]] (0 where idx<0) in one launch. */
int srwn_pack_a_index(int32_t* dst_idx, int32_t src_offset, int32_t rows_valid, int32_t k_valid,
                      int32_t row_stride, int32_t k_stride, int32_t mt_count, int32_t ks_total,
                      int32_t ks_offset, int32_t ks_count, int32_t perm_from_ks, void* stream);
int srwn_pack_gather(const float* src, const int32_t* idx, void* dst, int64_t n, int32_t dtype, void* stream);
/* srwn_pack_gather and, in the same launch, the column sums of a [sum_rows, sum_cols] fp32 matrix (fp64 accumulate, rows
 * in order): sum_out[c] = sum_l sum_src[l*sum_cols + c].  The training step re-packs the weight images after every
 * optimizer step; the sum of the layers' skip biases -- the bias of the skip sum, model.py:50 -- rides along instead of
 * being a reduction launch in front of every forward pass.  sum_rows = 0: plain srwn_pack_gather. */
int srwn_pack_gather_rowsum(const float* src, const int32_t* idx, void* dst, int64_t n, int32_t dtype,
                            const float* sum_src, int32_t sum_rows, int32_t sum_cols, float* sum_out, void* stream);

/* ---- generic dilated causal conv: _DilatedCausalConv1d / DilatedCausalConv1d (ops.py:6-20)
 * y[b,t,o] = bias[o] + sum_k sum_i x[b, t-(K-1-k)*dilation - shift, i] * w[k,i,o]  (zero for t<0).
 * `shift` = 1 folds RightShift (ops.py:78-80) into the tap offsets.  x is fp32 (audio side);
 * y is `dtype_out`.  Plain-VALU kernel: used for the Cin=1 input conv (model.py:40,173) and the
 * ops-level API; the 64-channel hot conv lives inside srwn_residual_layer_fwd. */
int srwn_causal_conv1d_fwd(const float* x, const float* w, const float* bias, void* y, int32_t B, int32_t T,
                           int32_t Cin, int32_t Cout, int32_t K, int32_t dilation, int32_t shift,
                           int32_t dtype_out, void* stream);
/* gradient of the Cin=1 input conv wrt its kernel [K,1,R] and bias [R] (autodiff of model.py:40):
 * gw[k,o] = sum_{b,t} audio[b,t-(K-1-k)-shift] * g[b,t,o]; gb[o] = sum g.  `partials` is a
 * workspace of srwn_init_conv_wgrad_partials(B,T,R,K) floats; result written (not accumulated).
 * gw = gb = NULL: only the per-slab partials are written -- partials[slab][(K+1)*R] = [gw | gb] of each slab of rows,
 * srwn_init_conv_wgrad_partials / ((K+1)*R) slabs -- for the caller to sum (the training step does it as one more job
 * of its srwn_reduce_partials_multi launch instead of a launch of its own).
 * R in {32, 64, 128}; K <= 7: the first stage's reduction buffer takes 8192*(K+1) bytes of LDS whatever R, 64 KiB at
 * K = 7.  K = 8 passes the shape check and is refused as SRWN_E_UNSUPPORTED at every R; K > 8: SRWN_E_SHAPE. */
int64_t srwn_init_conv_wgrad_partials(int32_t B, int32_t T, int32_t R, int32_t K);
int srwn_init_conv_wgrad(const float* audio, const void* g, float* partials, float* gw, float* gb, int32_t B,
                         int32_t T, int32_t R, int32_t K, int32_t shift, int32_t dtype, void* stream);

/* ---- fused residual layer forward: ResidualDilationLayer (ops.py:23-46) for K=2 taps, with the
 * decoder's conditioning add (model.py:180-183; NN upsample ops.py:64-74 as t/pool_stride) fused in.
 * x is the layer's COMPLETE input (the conditioning bias of this layer already added); the kernel adds the NEXT
 * layer's bias to what it stores, so no consumer (taps, residual base, weight gradients, the generator's rings)
 * ever re-adds it:
 *   z   = tanh(conv_K(x) + bias_f)                          -> z_out  (saved for skip GEMM and backward)
 *   c   = z * sigmoid(z)                                     (ops.py:33: the gate conv result is discarded)
 *   h   = (x + c @ Wr + bias_r) * sqrt(.5) + cond_next[b, t/pool_stride, :]   -> h_out   (cond_next may be NULL)
 * The first layer's bias is added to the input conv's output by srwn_add_frame_bias.
 * The skip 1x1 (ops.py:44) is deferred to srwn_pw_linear over the stored z of all layers.
 * wconv: packed [R/32][K*R/16] (last tap permuted k order), wres: packed [R/32][R/16] (permuted).
 * cond rows are cond_row_stride elements apart (one [B*frames, L*R] product serves every layer). */
int srwn_residual_layer_fwd(const void* x, const void* cond, const void* wconv, const void* wres,
                            const float* bias_f, const float* bias_r, void* h_out, void* z_out, int32_t B,
                            int32_t T, int32_t R, int32_t K, int32_t dilation, int32_t cond_frames,
                            int32_t pool_stride, int32_t cond_row_stride, int32_t dtype, void* stream);

/* ---- several consecutive residual layers per launch (the stacking loops model.py:42-47, 176-189, 428-453 around
 * ResidualDilationLayer, ops.py:23-46).  Same arithmetic, operands and outputs as `nlayers` calls of
 * srwn_residual_layer_fwd (bit-identical results), but the layer outputs travel between layers in LDS:
 * layer g (dilation dilations[g]) reads x_{g} and stores z_g at z_out + g*layer_stride and x_{g+1} at
 * x_out + g*layer_stride (elements; the engine's [L,B,T,R] stacks).  wconv/wres/bias_f/bias_r/cond_next are HOST
 * arrays of nlayers device pointers (cond_next[g] = the conditioning bias of the layer above layer g, or NULL).
 * Requirement: sum(dilations)/gcd(dilations) <= 31 and nlayers <= 8 (srwn_group_plan cuts a stack accordingly):
 * the kernel works on the residue classes t = j*gcd + r, where the group's dilations are small, and recomputes a
 * halo of that many steps per segment.  seg_rows = 0 lets the library choose the segment length. */
int srwn_residual_group_fwd(const void* x0, void* x_out, void* z_out, int64_t layer_stride,
                            const void* const* wconv, const void* const* wres, const float* const* bias_f,
                            const float* const* bias_r, const void* const* cond_next, int32_t cond_frames,
                            int32_t pool_stride, int32_t cond_row_stride, const int32_t* dilations, int32_t nlayers,
                            int32_t B, int32_t T, int32_t R, int32_t K, int32_t seg_rows, int32_t dtype, void* stream);
/* the backward chain of such a group (autodiff of the same lines; TF builds it in AdamOptimizer.minimize, model.py:31),
 * top layer first, in one launch: for g = nlayers-1 .. 0
 *   df_g = (Wr_g . (G_{g+1} sqrt(.5)) + dcs_g) * d(z sigmoid z)/df (z_g)        -> df_out + g*layer_stride
 *   G_g  = G_{g+1} sqrt(.5) + sum_k Wf_g[k] . df_g[t + (K-1-k)*dilations[g]]     -> g_out  + g*layer_stride
 * with G_{nlayers} = g_top (NULL = 0: the teacher's last dense output is unused, model.py:45-50) and dcs = Ws . dtotal
 * of every layer from srwn_skip_dgrad_all (NULL for the flows of ParallelWaveNet, model.py:440-449: no skip path).
 * Same values as nlayers + 1 calls of srwn_residual_layer_bwd (identical in fp32; in bf16 the gradient handed from
 * layer to layer is the stored, rounded one).  wconvT / wresT: HOST arrays of nlayers device pointers. */
int srwn_residual_group_bwd(const void* g_top, void* g_out, void* df_out, const void* z, const void* dcs,
                            int64_t layer_stride, const void* const* wconvT, const void* const* wresT,
                            const int32_t* dilations, int32_t nlayers, int32_t B, int32_t T, int32_t R, int32_t K,
                            int32_t seg_rows, int32_t dtype, void* stream);
/* ---- layer weight gradients summed inside the backward group kernel, 8 waves, output-split ("wt" mode).
 * The two kernels of a group are given the SAME segment cut (srwn_group_wt_geometry).  srwn_residual_group_fwd_wt is
 * srwn_residual_group_fwd that also writes, per layer g of the group and per 32-step tile of every segment, the
 * TRANSPOSED layer input x_g and gate output c_g = z_g sigmoid(z_g) ("weight-gradient tiles", per 16 channels x 32 steps one MFMA fragment in lane order,
 * layer g at xT / cT + g*wt_layer_stride elements; steps a segment does not own are zero in xT).  With
 * store_inner_x = 0 only the group's top layer stores its output rows (x_out + (nlayers-1)*layer_stride): in this mode
 * nothing reads the inner layers' (their transposed copies feed the weight gradients).
 * srwn_residual_group_bwd_wt is the chain of srwn_residual_group_bwd which, per layer, additionally contracts over time
 *   part_r [g][slab][i][o]     = sum c_g[t,i] * G_{g+1}[t,o]      part_br[g][slab][o] = sum G_{g+1}[t,o]
 *   part_f [g][slab][k*R+i][o] = sum x_g[t-(1-k)*d_g,i] * df_g[t,o]   part_bf[g][slab][o] = sum df_g[t,o]
 * (the sums of srwn_wgrad_layers, in its layout; tf.gradients of ops.py:27,39) with the A operands loaded as MFMA
 * fragments from those tiles and df_g / G_{g+1} read from the kernel's own LDS image, the R x R outputs split into
 * 16 x 16 blocks over the eight waves.  df is not stored; G of the inner layers only with write_all_g (the conditioned
 * decoders sum it per frame, model.py:180); g_out always receives the group's bottom gradient.  One partial slab per
 * workgroup (`nslabs` from srwn_group_wt_geometry; slabs beyond it must stay zero); finish with srwn_reduce_partials,
 * sqrt(.5) on the residual pair.  Halo (sum(dilations)/gcd) <= 31.
 * part16 != 0 (dtype SRWN_BF16 only): part_f / part_r are written in the COMPUTE type instead of fp32 -- the same number
 * of elements per (layer, slab), as 16 x 16 blocks in lane order (layout SRWN_PARTIALS_BLK16 of SrwnReduceJob below):
 * half the bytes both ways (the 256 x 30 partials of config 2 are 0.38 GB per step in fp32, written here and read back by
 * the reduction) for one more bf16 rounding per segment a workgroup runs: a later segment re-reads the block, adds its
 * fp32 sum and rounds again, so k segments per workgroup round the running sum k times (measured cost in accuracy, by k:
 * DESIGN.md 4c; the engine passes fp32 slabs for a group with more segments than workgroups).  The two bias partials
 * stay fp32.
 * ic_audio != NULL (the stack's FIRST group, dcs given; with fp32 slabs or part16 blocks): the launch also leaves the partial sums
 * of the input conv's kernel and bias gradient (model.py:40; what srwn_init_conv_wgrad's first stage forms from g_out in a
 * launch of its own) -- ic_partials[slab][3 R] = [sum_t audio[t-1-ic_shift] G_0[t,:] | sum_t audio[t-ic_shift] G_0[t,:] |
 * sum_t G_0[t,:]] over rows the workgroup's segments own, fp32, 8 / (R/16) slabs per workgroup (the launch's waves split
 * the tiles between them): ic_partials holds nslabs * 8 / (R/16) slabs of 3 R floats, to be summed; the audio enters the
 * bf16 MFMA as a high and a low bf16 part (exact to 2^-17).  audio [B,T] fp32. */
int srwn_group_wt_geometry(const int32_t* dilations, int32_t nlayers, int32_t B, int32_t T, int32_t R, int32_t dtype,
                           int32_t seg_rows_in, int32_t* seg_rows, int32_t* tiles_per_seg, int64_t* elems_per_layer,
                           int32_t* nslabs);
int srwn_residual_group_fwd_wt(const void* x0, void* x_out, void* z_out, int64_t layer_stride, void* xT, void* cT,
                               int64_t wt_layer_stride, int32_t store_inner_x, const void* const* wconv, const void* const* wres,
                               const float* const* bias_f, const float* const* bias_r, const void* const* cond_next,
                               int32_t cond_frames, int32_t pool_stride, int32_t cond_row_stride,
                               const int32_t* dilations, int32_t nlayers, int32_t B, int32_t T, int32_t R, int32_t K,
                               int32_t seg_rows, int32_t dtype, void* stream);
/* the FIRST group of a stack with the stack's input conv fused in (model.py:40 / 172-173: DilatedCausalConv1d 1 -> R,
 * K = 2 taps, d = 1; RightShift, ops.py:78-80, as `shift` in {0, 1}): what srwn_causal_conv1d_fwd(audio, init_w, init_b)
 * would have written as the group's input is computed into the kernel's segment image in the same arithmetic (the
 * activations are bit-identical) and never reaches HBM -- one launch, a 2*R-byte-per-sample write and the read that
 * fetches it back less.  audio [B,T] fp32, init_w [2,1,R], init_b [R] fp32.  Otherwise srwn_residual_group_fwd_wt (xT / cT
 * required).  Not built for the conditioned decoders (their first layer's bias is added
 * to the input conv's output: srwn_add_frame_bias). */
int srwn_residual_group_fwd_ic(const float* audio, const float* init_w, const float* init_b, int32_t shift, void* x_out,
                               void* z_out, int64_t layer_stride, void* xT, void* cT, int64_t wt_layer_stride,
                               int32_t store_inner_x, const void* const* wconv, const void* const* wres,
                               const float* const* bias_f, const float* const* bias_r, const int32_t* dilations,
                               int32_t nlayers, int32_t B, int32_t T, int32_t R, int32_t K, int32_t seg_rows,
                               int32_t dtype, void* stream);
int srwn_residual_group_bwd_wt(const void* g_top, void* g_out, int32_t write_all_g, const void* z, const void* dcs,
                               int64_t layer_stride, const void* xT, const void* cT, int64_t wt_layer_stride,
                               const void* const* wconvT, const void* const* wresT, const int32_t* dilations,
                               int32_t nlayers, void* part_f, void* part_r, float* part_bf, float* part_br,
                               int32_t part16, const float* ic_audio, float* ic_partials, int32_t ic_shift,
                               int32_t nslabs, int32_t B, int32_t T, int32_t R, int32_t K, int32_t seg_rows,
                               int32_t dtype, void* stream);
/* the same cut chosen for a problem size (B clips of T steps, R channels, dtype): minimises the estimated run time of
 * the group kernels (tile rounds per layer + a fixed cost per launch) over all cuts into runs of <= max_layers layers. */
int32_t srwn_group_plan_auto(const int32_t* dilations, int32_t nlayers, int32_t B, int32_t T, int32_t R, int32_t dtype,
                             int32_t max_layers, int32_t* starts);
/* ---- the remaining free functions of ops.py (none on the timed path; fp32, plain VALU kernels):
 * log_prob_from_logits (ops.py:111-115) -> y [rows,C] and / or log_sum_exp (ops.py:117-122) -> lse [rows] (either NULL) */
int srwn_log_softmax(const float* x, float* y, float* lse, int64_t rows, int32_t C, void* stream);
/* categorical_sample (ops.py:106-109): one index per row drawn from softmax(logits) (tf.multinomial's stream is not
 * reproducible; this one is counter-based: the same seed gives the same draws) */
int srwn_categorical_sample(const float* logits, int32_t* out, int64_t rows, int32_t C, uint64_t seed, void* stream);
/* probs_logistic (ops.py:203-214): sigmoid((y-mu+h)/s) - sigmoid((y-mu-h)/s), h = 1/(num_classes-1),
 * s = max(scale, exp(log_scale_min)) */
int srwn_probs_logistic(const float* scale, const float* mu, const float* y, float* out, int64_t n,
                        int32_t num_classes, float log_scale_min, void* stream);
/* pieces of ResidualDilationLayer / ResidualDilationLayerNC for shapes outside the fused kernels (any filter_width, any
 * channel counts; ops.py:232-236 builds an 8-channel layer on a 1-channel input): z = tanh(f), c = z*sigmoid(z)
 * (ops.py:28,33,36); dense = (inputs + residual)*sqrt(.5) with a 1-channel input broadcast (ops.py:40); relu (ops.py:49,52) */
int srwn_tanh_gate(const float* f, float* z, float* c, int64_t n, void* stream);
/* the gated activation unit with SURVEY 8(b)'s gate_mode: z = tanh(f) and
 *   SRWN_GATE_REFERENCE: c = z * sigmoid(z)   -- the graph the reference RUNS (ops.py:33 overwrites the gate conv's result
 *                                                with sigmoid(filter_conv); g is not read and may be NULL) = srwn_tanh_gate
 *   SRWN_GATE_WAVENET:   c = z * sigmoid(g)   -- the canonical WaveNet unit ops.py:31-32 builds and then discards; g = the
 *                                                gate conv's output (srwn_causal_conv1d_fwd with the `_gate` kernel)
 * Forward, fp32, any shape: the ops-level ResidualDilationLayer(gate_mode="wavenet") of sr-wavenet_amd/ops.py runs on it.
 * The fused training kernels srwn_residual_layer_* / srwn_residual_group_* implement SRWN_GATE_REFERENCE (parity is judged
 * on the graph the reference executes, and its `_gate` variables receive no gradient there); SRWN_GATE_WAVENET trains
 * through srwn_wavenet_layer_fwd / srwn_wavenet_layer_bwd (one launch per layer, since srwn_version() 102). */
#define SRWN_GATE_REFERENCE 0
#define SRWN_GATE_WAVENET 1
int srwn_gated_activation(const float* f, const float* g, float* z, float* c, int64_t n, int32_t gate_mode, void* stream);
int srwn_residual_combine(const float* x, int32_t cin, const float* res, int32_t R, float* out, int64_t rows,
                          void* stream);
int srwn_relu(const float* x, float* y, int64_t n, void* stream);
/* discretized_mix_logistic_loss with sum_all=False (ops.py:174-175): out[row] = -log_sum_exp_m(log p_m(x) + log pi_m) */
int srwn_mol_nll_rows(const float* logits, int64_t ldl, const float* x, int32_t M, float* out, int64_t rows,
                      void* stream);

/* diagnostic hook (no reference counterpart).  Only the -DSRWN_DIAG build of this library (libsrwn_diag.so:
 * `python sr-wavenet_amd/build.py --diag`, loaded with SRWN_LIB_PATH) holds the stamped kernel instantiations: there,
 * while a device buffer of 1024 uint64 is registered, the bf16 group kernels, the skip sum and the one-launch head append
 * in-kernel clock stamps of workgroup 0 to it; NULL restores production code.  The shipped libsrwn.so accepts NULL and
 * returns SRWN_E_UNSUPPORTED for a buffer. */
int srwn_debug_stamp_buffer(void* device_buffer);
/* greedy cut of a stack's dilation list (model.py:9, teacher.py:57) into such groups: starts[0..n] (starts[n] = nlayers),
 * returns n.  `starts` needs nlayers + 1 entries. */
int32_t srwn_group_plan(const int32_t* dilations, int32_t nlayers, int32_t max_halo, int32_t max_layers,
                        int32_t* starts);

/* ---- pointwise linear ("channels GEMM"): tf.layers.conv1d kernel_size=1 (ops.py:39,44;
 * model.py:53,56,180) and the sum of all skip 1x1s (model.py:50) as one K = L*R contraction:
 *   y[row, n] = epi( bias[n] + sum_k pro(x[row, k]) * W[k, n] )
 * Input channel k lives at  x + (k / chunk_len)*x_chunk_stride + row*x_row_stride + k % chunk_len
 * (chunk = one layer's z tensor for the skip sum; chunk_len = Cin for an ordinary tensor).
 * wpack: packed [Cout_pad/32][Cin/16] natural k order.  Rows n >= cout_valid are not stored.
 * EPI_MASK multiplies by (aux[row, n] > 0) (aux row stride = aux_row_stride elements). */
int srwn_pw_linear(const void* x, int64_t x_row_stride, int64_t x_chunk_stride, int32_t chunk_len, int32_t Cin,
                   const void* wpack, const float* bias, void* y, int64_t y_row_stride, int32_t cout_pad,
                   int32_t cout_valid, int64_t rows, const void* aux, int64_t aux_row_stride, int32_t pro,
                   int32_t epi, int32_t dtype, void* stream);

/* the same product (no prologue / epilogue) with its outputs in chunks of y_chunk_len channels: channel n at
 * y + (n / y_chunk_len)*y_chunk_stride + row*y_row_stride + n % y_chunk_len -- the conditioning biases of all layers
 * (model.py:180: L*R outputs) stored layer by layer, [L][rows][R], so that a layer's rows are dense. */
int srwn_pw_linear_ychunks(const void* x, int64_t x_row_stride, int32_t Cin, const void* wpack, const float* bias, void* y,
                           int64_t y_row_stride, int32_t y_chunk_len, int64_t y_chunk_stride, int32_t cout_pad,
                           int32_t cout_valid, int64_t rows, int32_t dtype, void* stream);

/* the same product split over the contraction axis (few rows, long K): slice z of nsplit writes its fp32 partial to
 * y_partials + z*rows*y_row_stride (bias in slice 0); srwn_reduce_partials(nslabs = nsplit, n = rows*y_row_stride)
 * finishes it.  Used for the encoder's pooled skip sum (model.py:150: B*frames rows, K = L*encoder_channels). */
int srwn_pw_linear_ksplit(const void* x, int64_t x_row_stride, int64_t x_chunk_stride, int32_t chunk_len, int32_t Cin,
                          const void* wpack, const float* bias, float* y_partials, int64_t y_row_stride,
                          int32_t cout_pad, int32_t cout_valid, int64_t rows, int32_t nsplit, int32_t dtype,
                          void* stream);

/* ---- last 1x1 + softmax head: model.py:56 then the mu-law softmax-CE the reference carries at
 * model.py:100-112 (log-softmax as ops.py:111-115), per time step, fused in registers:
 *   logits = bias + x @ W;  loss_row = logsumexp(logits) - logits[target]
 *   dlogits = (softmax(logits) - onehot(target)) * grad_scale   -> dlogits (dtype), may be NULL
 * logits_out (fp32, [rows, cout_valid]) may be NULL.  Per-tile loss sums go to loss_partials
 * (srwn_softmax_ce_partials(rows) floats); srwn_reduce_loss sums them in a fixed order. */
int64_t srwn_softmax_ce_partials(int64_t rows);
int srwn_head_softmax_ce(const void* x, int64_t x_row_stride, int32_t Cin, const void* wpack, const float* bias,
                         const int32_t* targets, float* loss_partials, void* dlogits, float* logits_out,
                         int32_t cout_pad, int32_t cout_valid, int64_t rows, float grad_scale, int32_t dtype,
                         void* stream);
int srwn_reduce_loss(const float* loss_partials, int64_t n, float scale, float* loss_out, void* stream);

/* ---- the whole head of the softmax teacher, forward and backward, in one launch (bf16, S = cout_pad = 256):
 *   r1 = relu(r0 @ W1 + b1)                      model.py:53-54
 *   logits = r1 @ W2 + b2; loss_row / dlogits as srwn_head_softmax_ce      model.py:56, 100-112
 *   da1 = (dlogits @ W2^T) * (r1 > 0);  dtotal = (da1 @ W1^T) * (r0 > 0)   (autodiff of model.py:51-56)
 * A wave carries 32 rows through the four products in registers; r1, dlogits, da1, dtotal ([rows, 256] each) are
 * written for the weight-gradient passes.  w1 is the srwn_pack image of W1 in natural k order; w2_perm, w2T_perm,
 * w1T_perm are the images of W2, W2^T, W1^T in the accumulator's (permuted) k order.  loss_partials as
 * srwn_head_softmax_ce.  Other shapes/dtypes: SRWN_E_UNSUPPORTED (the four separate entry points remain). */
int srwn_head_chain(const void* r0, const void* w1, const void* w2_perm, const void* w2T_perm, const void* w1T_perm,
                    const float* b1, const float* b2, const int32_t* targets, float* loss_partials, void* r1,
                    void* dlogits, void* da1, void* dtotal, int32_t S, int32_t cout_pad, int32_t cout_valid,
                    int64_t rows, float grad_scale, int32_t dtype, void* stream);

/* ---- fused residual layer backward: autodiff of ResidualDilationLayer (ops.py:23-46); TF builds
 * these gradients in tf.train.AdamOptimizer.minimize (model.py:31).  One call per layer, top down:
 *   has_up  : G_{l+1}[t] = g_in[t]*sqrt(.5) + sum_k Wf_{l+1}[k] . df_up[t + (K-1-k)*dilation_up]  -> g_out
 *             (g_in = G_{l+2}, may be NULL = 0; wconvT_up packed [R/32][K*R/16], rows = in channel)
 *   has_down: dc = Wr_l . (G_{l+1} sqrt(.5)) + Ws_l . dtotal;  df_l = dc * d(z sigmoid z)/df      -> df_out
 *             (wresT packed permuted [R/32][R/16]; z = z_l; the skip term Ws_l . dtotal is either `dcs`
 *             = layer l's slice from srwn_skip_dgrad_all, or computed here from wskipT [R/32][S/16] + dtotal)
 * Layer L-1: has_up=0 (its dense output is unused, model.py:45-50).  Below layer 0: has_down=0.
 * Flow stacks of ParallelWaveNet (model.py:415-453) have no skip path: pass S=0 (dc = Wr_l . G sqrt(.5) only);
 * their layer L-1 runs with has_up=2: G_L (the flow head's gradient, srwn_flow_affine_bwd) is READ from g_out. */
int srwn_residual_layer_bwd(const void* g_in, const void* df_up, const void* wconvT_up, void* g_out,
                            const void* wresT, const void* wskipT, const void* dtotal, const void* dcs,
                            const void* z, void* df_out, int32_t B, int32_t T, int32_t R, int32_t S, int32_t K,
                            int32_t dilation_up, int32_t has_up, int32_t has_down, int32_t dtype, void* stream);

/* ---- weight gradients (the tf.gradients of every kernel on the path), batched over `nbatch` layers:
 *   partials[l][slab][i][o] = sum_{rows of slab} pro(in_l[row - shifts[l], i] + cond_l[b, (t-shift)/pool, i])
 *                                                 * dout_l[row, o]          (0 where t - shift < 0)
 *   bias_partials[l][slab][o] = sum_{rows of slab} dout_l[row, o]           (may be NULL)
 * in_l = in + l*in_batch_stride (elements), dout_l likewise (stride 0 = shared by all layers);
 * rows = B*T flattened, `T` delimits batch elements for the shift.  pro = SRWN_PRO_GATE rebuilds
 * c = z*sigmoid(z).  nslabs = srwn_wgrad_slabs(rows); partials need nbatch*nslabs*cin*cout floats.
 * srwn_reduce_partials then writes out[l*out_batch_stride + i] = scale * sum_slab partials[...]
 * (fixed order, f64 accumulate); partials_batched=0 re-reads batch entry 0 for every l. */
int32_t srwn_wgrad_slabs(int64_t rows);
int srwn_wgrad(const void* in, int64_t in_batch_stride, int32_t cin, const void* dout, int64_t dout_batch_stride,
               int32_t cout, const void* cond, int64_t cond_batch_stride, int32_t cond_frames, int32_t pool_stride,
               int32_t cond_row_stride, const int32_t* shifts /* host array [nbatch] or NULL */, int32_t nbatch, float* partials,
               float* bias_partials, int64_t rows, int32_t T, int32_t nslabs, int32_t pro, int32_t dtype,
               void* stream);
int srwn_reduce_partials(const float* partials, int32_t nslabs, int64_t n, int32_t nbatch, int32_t partials_batched,
                         float scale, float* out, int64_t out_batch_stride, void* stream);
/* Up to 16 such reductions as ONE launch (host array of jobs; each job's result is bit-identical to its own
 * srwn_reduce_partials call). */
#define SRWN_PARTIALS_F32 0   /* fp32 [batch][slab][n]: what srwn_reduce_partials takes */
#define SRWN_PARTIALS_BLK16 1 /* bf16 [batch][slab][n] where the n = rows*blk_cols elements of a [rows, blk_cols] matrix
                               * are stored as 16 x 16 blocks in MFMA-accumulator lane order: block (rb, cb) at
                               * (rb*(blk_cols/16) + cb)*256 elements, lane l's four values -- rows 16 rb + 4 (l >> 4) + 0..3
                               * of column 16 cb + (l & 15) -- at + 4 l (srwn_residual_group_bwd_wt with part16) */
#define SRWN_PARTIALS_SUM 2   /* fp32; ONE output: out[0] = scale * the sum of all nslabs*n values, in srwn_reduce_loss's
                               * order and precision (the loss partials of a training step: bit-equal to that launch) */
typedef struct SrwnReduceJob {
  const void* partials; int32_t nslabs; int64_t n; int32_t nbatch; int32_t partials_batched; float scale;
  float* out; int64_t out_batch_stride;
  int32_t layout; int32_t blk_cols;      /* SRWN_PARTIALS_*; blk_cols: BLK16 only (a multiple of 16) */
} SrwnReduceJob;
int srwn_reduce_partials_multi(const SrwnReduceJob* jobs, int32_t njobs, void* stream);

/* ---- adjoint of ResizeEmbeddingNearestNeighbor (ops.py:64-74): out[b,e,c] = sum_{t in frame e} g[b,t,c] */
/* x[b,t,c] += bias[b, t/pool_stride, c] in place (h = h + upsampled, model.py:181-183, for the first layer) */
int srwn_add_frame_bias(void* x, const void* bias, int64_t bias_row_stride, int32_t B, int32_t T, int32_t C,
                        int32_t frames, int32_t pool_stride, int32_t dtype, void* stream);
int srwn_frame_sum(const void* g, void* out, int32_t B, int32_t T, int32_t C, int32_t frames, int32_t pool_stride,
                   int32_t dtype, void* stream);
/* the same for `nbatch` layers in one launch: g + l*g_batch_stride -> out + l*out_batch_stride (elements), times
 * `scale` (1/pool_stride gives tf.nn.pool AVG, model.py:154) */
int srwn_frame_sum_batched(const void* g, int64_t g_batch_stride, void* out, int64_t out_batch_stride, int32_t nbatch,
                           int32_t B, int32_t T, int32_t C, int32_t frames, int32_t pool_stride, float scale,
                           int32_t dtype, void* stream);

/* ---- tf.train.AdamOptimizer update (model.py:31,117,382) on the flat fp32 parameter buffer:
 *   t = ++*step (device counter);  lr_t = lr*sqrt(1-b2^t)/(1-b1^t);  g = grads*grad_scale;
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  params -= lr_t * m / (sqrt(v) + eps) */
int srwn_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, int64_t* step, float lr,
                   float beta1, float beta2, float eps, float grad_scale, void* stream);

/* ---- time-pooled classifier head of class WaveNet (model.py:56-60; loss model.py:24-29).
 * tf.nn.pool AVG over the whole clip commutes with the last 1x1, so:
 *   srwn_time_mean   : out[b,c] = mean_t x[b,t,c]   (partials: B*srwn_time_mean_slabs(T)*C floats)
 *   srwn_pooled_head : logits = mean @ w2 + b2; probs = softmax (model.py:60); with labels also
 *                      loss = mean_b softmax_cross_entropy_with_logits_v2 (soft labels, model.py:29),
 *                      gw2/gb2 (written, [S,ldw]/[ldw]) and dmean = d loss / d mean  [B,S].  Any B (since
 *                      srwn_version() 103: the rows go through one workgroup's LDS in chunks, same bits for any
 *                      chunk size); C <= 16128
 *   srwn_bcast_mask  : da1[b,t,s] = (r1[b,t,s] > 0) ? dmean[b,s]*scale : 0  (scale = 1/T) */
int32_t srwn_time_mean_slabs(int32_t T);
int srwn_time_mean(const void* x, float* partials, float* out, int32_t B, int32_t T, int32_t C, int32_t dtype,
                   void* stream);
int srwn_pooled_head(const float* mean, const float* w2, const float* b2, const float* labels, float* probs,
                     float* loss, float* gw2, float* gb2, float* dmean, int32_t B, int32_t S, int32_t C,
                     int32_t ldw, void* stream);
int srwn_bcast_mask(const float* dmean, const void* r1, void* out, int32_t B, int32_t T, int32_t S, float scale,
                    int32_t dtype, void* stream);

/* ---- canonical WaveNet gate (SRWN_GATE_WAVENET), one launch per layer (since srwn_version() 102).  R in {32, 64},
 * K = 2, any dilation, dtype SRWN_BF16 or SRWN_F32.  Forward:
 *   z = tanh(conv_K(x, Wf) + bias_f)   s = sigmoid(conv_K(x, Wg) + bias_g)   c = z * s      -> z_out, s_out, c_out
 *   h = (x + c @ Wr + bias_r) * sqrt(.5) + cond_next[b, t/pool_stride, :]                  -> h_out (cond may be NULL)
 * (the same conditioning contract as srwn_residual_layer_fwd: x is the layer's complete input).  Both convs are one
 * K*R-deep product into 2R rows: wconv = the pack_conv image of Wf followed by that of Wg ([2R/32][K*R/16], natural k
 * order), wres = packed [R/32][R/16] (permuted).  The skip sum and the 1x1 weight gradients read c with SRWN_PRO_NONE. */
int srwn_wavenet_layer_fwd(const void* x, const void* cond, const void* wconv, const void* wres, const float* bias_f,
                           const float* bias_g, const float* bias_r, void* h_out, void* z_out, void* s_out, void* c_out,
                           int32_t B, int32_t T, int32_t R, int32_t K, int32_t dilation, int32_t cond_frames,
                           int32_t pool_stride, int32_t cond_row_stride, int32_t dtype, void* stream);
/* Backward, the chaining contract of srwn_residual_layer_bwd with D = [d f | d g] ([B,T,2R]) in place of df:
 *   has_up:   G_{l+1} = G_{l+2} sqrt(.5) + sum_k [Wf|Wg]_{l+1}[k] . D_{l+1}[t + (K-1-k) d_{l+1}]     -> g_out
 *             (g_in = G_{l+2} or NULL for zero; wconvT_up = the pack_conv_T images of Wf_{l+1} and Wg_{l+1} back to back)
 *   has_down: dc = Wr_l . (G_{l+1} sqrt(.5)) + Ws_l . dtotal;  D_l = [dc s (1 - z^2) | dc z s (1 - s)]  -> d_out
 *             (skip term: `dcs` from srwn_skip_dgrad_all, or wskipT [R/32][S/16] + dtotal [B*T,S]; z, s from the forward)
 * Layer L-1: has_up=0.  Below layer 0: has_down=0.  Weight gradients: srwn_wgrad over (x_l, D_l) with cin = R, cout = 2R
 * and one shift per tap, and over (c_l, G_{l+1}) with SRWN_PRO_NONE (srwn_wgrad_layers assumes the reference gate). */
int srwn_wavenet_layer_bwd(const void* g_in, const void* d_up, const void* wconvT_up, void* g_out, const void* wresT,
                           const void* wskipT, const void* dtotal, const void* dcs, const void* z, const void* s,
                           void* d_out, int32_t B, int32_t T, int32_t R, int32_t S, int32_t K, int32_t dilation_up,
                           int32_t has_up, int32_t has_down, int32_t dtype, void* stream);

/* ---- contrastive head of class SiameseWaveNet (model.py:660-797; since srwn_version() 101).  The two towers share
 * their weights, so they run as ONE batch of rows = 2P clips: rows 0..P-1 the left clips, P..2P-1 the right ones.  On
 * the time-mean of srwn_time_mean (the pool commutes with the last 1x1):
 *   emb[r,k] = b2[k] + sum_s mean[r,s]*w2[s,k]                        [rows,D]   (w2 [S,ldw], columns >= D ignored)
 *   dist[p]  = sqrt(1e-8 + |emb[p] - emb[P+p]|^2)                      [P]        (model.py:736)
 *   loss     = mean_p y_p*d_p^2/2 + (1-y_p)*max(0, margin-d_p)^2/2                (model.py:747-749; y = 1: "same")
 * with labels [P] (plain floats) also gw2/gb2 (written, [S,ldw]/[ldw]; gb2 is exactly 0) and dmean = d loss / d mean
 * [rows,S] (needs an even row count, loss and the gradient outputs).  labels == NULL: emb only, and dist when `dist` is
 * given (even row count).  One workgroup: rows*D + 2P floats must fit 64 KiB of LDS (else SRWN_E_SHAPE). */
int srwn_contrastive_head(const float* mean, const float* w2, const float* b2, const float* labels, float margin,
                          float* emb, float* dist, float* loss, float* gw2, float* gb2, float* dmean, int32_t rows,
                          int32_t S, int32_t D, int32_t ldw, void* stream);

/* ---- weight gradient of 256-wide products as ONE time-contraction GEMM (tf.gradients of ops.py:44,
 * model.py:53,56 kernels):  partials[slab][m][n] = sum_{rows of slab} pro(A[row][m]) * D[row][n], n < 256.
 * A is addressed in chunks of 64 channels: a + (m/64)*a_chunk_stride + row*a_row_stride + m%64
 * (the [L,rows,64] stack of z for all skip 1x1s at once, or a [rows,256] tensor with chunk stride 64).
 * bias_partials[slab][n] = column sums of D (may be NULL).  nslabs = srwn_wgrad256_slabs(rows, m_chunks);
 * finish with srwn_reduce_partials. */
int32_t srwn_wgrad256_slabs(int64_t rows, int32_t m_chunks);
/* the same GEMM for the reference scripts' widths: A chunks of `chunk_width` = 64 or 32 channels
 * (dilation_channels), D of `d_width` = 256 or 128 columns (skip_channels); m_chunks*chunk_width must be a
 * multiple of 64; partials [slab][m_chunks*chunk_width][d_width]. */
int32_t srwn_wgrad_wide_slabs(int64_t rows, int32_t m_chunks, int32_t chunk_width);
int srwn_wgrad_wide(const void* a, int64_t a_chunk_stride, int64_t a_row_stride, int32_t m_chunks, int32_t chunk_width,
                    const void* d, int64_t d_row_stride, int32_t d_width, float* partials, float* bias_partials,
                    int64_t rows, int32_t nslabs, int32_t pro, int32_t dtype, void* stream);
/* two such products of ONE shape as one launch (the head's two 1x1s, model.py:53,56: 46 us each alone -- 256 workgroups
 * of 4 MFMAs per barrier -- side by side their workgroups share the CUs and hide each other's waits) */
int srwn_wgrad_wide_pair(const void* a0, const void* d0, float* partials0, float* bias_partials0, const void* a1,
                         const void* d1, float* partials1, float* bias_partials1, int64_t a_chunk_stride,
                         int64_t a_row_stride, int32_t m_chunks, int32_t chunk_width, int64_t d_row_stride,
                         int32_t d_width, int64_t rows, int32_t nslabs, int32_t pro, int32_t dtype, void* stream);
int srwn_wgrad256(const void* a, int64_t a_chunk_stride, int64_t a_row_stride, int32_t m_chunks, const void* d,
                  int64_t d_row_stride, float* partials, float* bias_partials, int64_t rows, int32_t nslabs,
                  int32_t pro, int32_t dtype, void* stream);

/* ---- skip-path data gradient of every layer in one launch (autodiff of ops.py:44):
 *   dcs[l][row][n] = sum_s dtotal[row][s] * Ws_l[n][s],   dcs + l*dcs_layer_stride, rows of R elements.
 * wskipT_all: the nlayers packed images [R/32][S/16] (natural k order) laid out back to back.
 * srwn_residual_layer_bwd then takes dcs_l instead of recomputing Ws_l . dtotal (pass wskipT = dtotal = NULL). */
int srwn_skip_dgrad_all(const void* dtotal, const void* wskipT_all, void* dcs, int64_t dcs_layer_stride,
                        int32_t nlayers, int64_t rows, int32_t R, int32_t S, int32_t dtype, void* stream);

/* ---- all per-layer weight gradients of ResidualDilationLayer (ops.py:27,39) in one pass over the
 * saved tensors, batched over layers ([L][rows][64] stacks, `layer_stride` elements apart; R=64, K=2):
 *   part_f [l][slab][k*64+i][o] = sum x_l[t-(1-k)*d_l, i] * df_l[t, o]   (x_l + cond_l when cond != NULL)
 *   part_r [l][slab][n][m]      = sum c_l[t, n] * g_l[t, m]              (c = z sigmoid z; g_l = G_{l+1})
 *   part_bf[l][slab][o] = sum df_l[t,o];  part_br[l][slab][m] = sum g_l[t,m]
 * dilations: host array [nlayers].  Finish with srwn_reduce_partials (sqrt(.5) on the residual pair). */
int srwn_wgrad_layers(const void* x, const void* z, const void* df, const void* g, int64_t layer_stride,
                      const void* cond, int64_t cond_layer_stride, int32_t cond_frames, int32_t pool_stride,
                      int32_t cond_row_stride, const int32_t* dilations, int32_t nlayers, float* part_f,
                      float* part_r, float* part_bf, float* part_br, int64_t rows, int32_t T, int32_t nslabs,
                      int32_t R, int32_t K, int32_t dtype, void* stream);

/* ---- weight gradient of all skip 1x1s from the forward group kernel's transposed gate outputs (tf.gradients of
 * ops.py:44 summed as model.py:50):  out[l*64 + n][s] = sum_t c_l[t][n] * d[t][s].  cT / wt_layer_stride: the cT buffer
 * srwn_residual_group_fwd_wt wrote (layer l at cT + l * wt_layer_stride elements); st[l] / seg_rows[l]: the stride (gcd of
 * the dilations) and the segment length (srwn_group_wt_geometry) of the group layer l was run in -- they fix which
 * positions its tiles hold; d: dskip [B*T, d_row_stride] (256 columns used).  Partials in srwn_wgrad256's layout:
 * partials[slab][nlayers*64][256], bias_partials[slab][256] (column sums of d; may be NULL); nslabs from
 * srwn_wgrad_skip_wt_slabs.  part16 != 0: `partials` holds the same [nlayers*64, 256] matrix per slab in bf16, as 16 x 16
 * blocks in lane order (SRWN_PARTIALS_BLK16 with 256 columns: half the partial bytes both ways, one more bf16 rounding
 * per partial sum -- one only: a slab's segments are summed in registers before its single store).  bf16, R = 64, S = 256 (csrc/srwn_wgradt.hip); other shapes: srwn_wgrad_wide on z. */
int32_t srwn_wgrad_skip_wt_slabs(const int32_t* st, const int32_t* seg_rows, int32_t nlayers, int32_t T);
int srwn_wgrad_skip_wt(const void* cT, int64_t wt_layer_stride, const int32_t* st, const int32_t* seg_rows,
                       int32_t nlayers, const void* d, int64_t d_row_stride, void* partials, float* bias_partials,
                       int32_t part16, int32_t nslabs, int32_t B, int32_t T, int32_t R, int32_t S, int32_t dtype,
                       void* stream);

/* ---- queue-cached incremental generation (BASELINE config 5; the reference only has the O(T^2 L) loop
 * of teacher.py:140-171).  Persistent workgroups generate `nsteps` samples, 32 utterances per workgroup,
 * with the arithmetic of the training graph (RightShift input conv model.py:172-173, layers ops.py:23-46,
 * head model.py:50-56, softmax over C mu-law classes, decode ops.py:96-104), keeping per layer a ring of
 * the last d_l+1 layer inputs (`ring`: ceil(B/32) * srwn_generate_ring_elems elements of `dtype`; one
 * workgroup per group of 32 utterances).
 * wcr: per layer, back to back, [conv image R/32 x 2R/16 (tap 0 natural, tap 1 permuted k order) |
 * residual image R/32 x R/16 (permuted)];  wskip: [S/32][L*R/16] in PERMUTED k order (its B operand is the
 * gate tile in registers); w1/w2/biases as for the training kernels.
 * mode 0 = argmax, 1 = categorical sample (counter-based RNG on seed, utterance, step).
 * forced != NULL: teacher forcing -- step t consumes forced[u, t-1] instead of its own sample (parity test).
 * audio_out/codes_out/forced are [B, Tout]; logits_out (may be NULL) [B, Tout, C] fp32. */
int64_t srwn_generate_ring_elems(const int32_t* dilations, int32_t nlayers, int32_t R);
int srwn_generate(const void* wcr, const void* wskip, const void* w1, const void* w2, const float* bias_f,
                  const float* bias_r, const float* bs_sum, const float* b1, const float* b2, const float* init_w,
                  const float* init_b, void* ring, float* audio_out, int32_t* codes_out, float* logits_out,
                  const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                  int32_t nsteps, int32_t R, int32_t S, int32_t C, int32_t K, int32_t mode, uint64_t seed,
                  int32_t dtype, void* stream);

/* The latency-optimised body of srwn_generate / srwn_generate_mol for bf16 stacks of R = 64 or 32 residual and S = 256 or
 * 128 skip channels, K = 2: same arithmetic, same rings (handed over ZERO-FILLED: a step before the first delayed tap
 * exists reads the slot nobody has written), same outputs, same RNG (teacher.py:140-171 / generator.py:150-170 are the
 * loops it replaces), but a layer's channels are split over the four waves on 16x16x32 tiles instead of every wave
 * running the whole chain, and the weights stream from L2 into registers one layer ahead (csrc/srwn_gen16.hip).
 * Fragment images of 64 lanes x 8 elements, lane l = row (l & 15), k = 8 (l >> 4) + j.  wl: per layer [4 waves][conv
 * k-steps 0..2R/32-1 (k < R: delayed tap, k >= R: current tap) | residual k-steps 0..R/32-1 | skip (S/64 row blocks) x
 * (R/32 k-steps)]; wave w owns conv / residual rows 16w.. (none for w >= R/16: zero fragments) and skip rows (S/4)w..;
 * wh1: [4 waves][S/64 row blocks][S/32 k-steps], wave w, block rb = rows (S/4) w + 16 rb; wh2: [4 waves][4 row
 * blocks][S/32 k-steps], rows 16 (4 rb + w) -- a head with few outputs still splits over the waves; rows beyond
 * ceil(C/32)*32 zero.  srwn_generate16_image_elems(nlayers, 0 | 1 | 2, R, S) = elements of wl | wh1 | wh2. */
int64_t srwn_generate16_image_elems(int32_t nlayers, int32_t which, int32_t R, int32_t S);
int srwn_generate16(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const float* bias_r,
                    const float* bs_sum, const float* b1, const float* b2, const float* init_w, const float* init_b,
                    void* ring, float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                    const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R,
                    int32_t S, int32_t C, int32_t mode, uint64_t seed, void* stream);
/* ... and for the conditioned mixture-of-logistics decoder (the model generator.py:150-170 samples from; arguments as
 * srwn_generate_mol): cond [B*cond_frames, cond_ld] bf16 (cond_ld a multiple of 4) or NULL. */
int srwn_generate16_mol(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const float* bias_r,
                        const float* bs_sum, const float* b1, const float* b2, const float* init_w,
                        const float* init_b, void* ring, float* audio_out, int32_t* codes_out, float* logits_out,
                        const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                        int32_t nsteps, int32_t R, int32_t S, int32_t num_mixtures, const void* cond,
                        int32_t cond_frames, int32_t pool_stride, int64_t cond_ld, int32_t mode, uint64_t seed,
                        void* stream);

/* The same generator for the conditioned mixture-of-logistics decoder of WaveNetAutoEncoder (model.py:158-200; the
 * reference samples it with one whole-clip pass per sample, generator.py:150-170): cond [B*cond_frames, cond_ld] in
 * `dtype` holds the conditioning biases cb_l of every layer at columns [l*R, (l+1)*R) (model.py:180: one
 * srwn_pw_linear of encoding_w_condition); layer l adds row (u, t / pool_stride), rounded like the training kernel.
 * cond = NULL: unconditioned.  Head: 4*num_mixtures logits (w2 image / b2 padded to a multiple of 32 rows), sampled
 * as sample_from_discretized_mix_logistic (ops.py:178-201) with counter-based uniforms in (1e-5, 1-1e-5);
 * mode 0 returns the selected mixture's mean.  codes_out = selected mixture; logits_out [B, Tout, 4M] (may be NULL). */
int srwn_generate_mol(const void* wcr, const void* wskip, const void* w1, const void* w2, const float* bias_f,
                      const float* bias_r, const float* bs_sum, const float* b1, const float* b2, const float* init_w,
                      const float* init_b, void* ring, float* audio_out, int32_t* codes_out, float* logits_out,
                      const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                      int32_t nsteps, int32_t R, int32_t S, int32_t K, int32_t num_mixtures, const void* cond,
                      int32_t cond_frames, int32_t pool_stride, int64_t cond_ld, int32_t mode, uint64_t seed,
                      int32_t dtype, void* stream);

/* ---- resumable generation (since srwn_version() 104): the four generators above as one call of a longer run, so that a
 * stream is produced chunk by chunk, stopped and continued, or continued from a prompt (the loop of teacher.py:140-171 /
 * generator.py:150-170 runs from t = 0 to the end in one go; these split it anywhere).  Each *_resume entry point takes
 * the arguments of the call it extends, plus:
 *   t0     the absolute step of the launch's first sample: step j of the launch is step t = t0 + j for the ring slots
 *          (t mod (d_l+1)), the delayed-tap test t - d_l >= 0, the conditioning frame t / pool_stride and both samplers'
 *          counters (softmax: (seed, u, t); mixture: (seed, u, t*(M+1)+m)).  Rows j of audio_out / codes_out / logits_out
 *          and of forced are the launch's own ([B, Tout] with nsteps <= Tout, as before).
 *   carry  float [B][2] = (a[t0-1], a[t0-2]), the two audio samples the input conv with RightShift (model.py:172-173)
 *          reads at step t0; read at the start, and on return it holds (a[t0+n-1], a[t0+n-2]) for the next launch: the
 *          forced samples where the launch was teacher-forced (step j reads forced[j-1] for j >= 1, else carry[0], and
 *          forced[j-2] for j >= 2, carry[0] for j = 1, carry[1] for j = 0), the emitted samples where it ran free.
 *          NULL = zeros in, nothing written back (only with t0 = 0: a NULL carry with t0 > 0 is SRWN_E_NULL).
 * The ring must hold the state after step t0 - 1: what the previous launch of the run left, srwn_generate_ring_fill, or
 * zeros for t0 = 0.  The one-shot entry points are these with t0 = 0, carry = NULL, and return the same bits. */
int srwn_generate_resume(const void* wcr, const void* wskip, const void* w1, const void* w2, const float* bias_f,
                         const float* bias_r, const float* bs_sum, const float* b1, const float* b2, const float* init_w,
                         const float* init_b, void* ring, float* audio_out, int32_t* codes_out, float* logits_out,
                         const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                         int32_t nsteps, int32_t R, int32_t S, int32_t C, int32_t K, int32_t mode, uint64_t seed,
                         int32_t dtype, void* stream, int32_t t0, float* carry);
int srwn_generate_mol_resume(const void* wcr, const void* wskip, const void* w1, const void* w2, const float* bias_f,
                             const float* bias_r, const float* bs_sum, const float* b1, const float* b2,
                             const float* init_w, const float* init_b, void* ring, float* audio_out, int32_t* codes_out,
                             float* logits_out, const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B,
                             int32_t Tout, int32_t nsteps, int32_t R, int32_t S, int32_t K, int32_t num_mixtures,
                             const void* cond, int32_t cond_frames, int32_t pool_stride, int64_t cond_ld, int32_t mode,
                             uint64_t seed, int32_t dtype, void* stream, int32_t t0, float* carry);
int srwn_generate16_resume(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const float* bias_r,
                           const float* bs_sum, const float* b1, const float* b2, const float* init_w, const float* init_b,
                           void* ring, float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                           const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R,
                           int32_t S, int32_t C, int32_t mode, uint64_t seed, void* stream, int32_t t0, float* carry);
int srwn_generate16_mol_resume(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const float* bias_r,
                               const float* bs_sum, const float* b1, const float* b2, const float* init_w,
                               const float* init_b, void* ring, float* audio_out, int32_t* codes_out, float* logits_out,
                               const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                               int32_t nsteps, int32_t R, int32_t S, int32_t num_mixtures, const void* cond,
                               int32_t cond_frames, int32_t pool_stride, int64_t cond_ld, int32_t mode, uint64_t seed,
                               void* stream, int32_t t0, float* carry);
/* The rings after a prompt of P samples, from ONE parallel forward pass over it instead of P generation steps (the
 * teacher-forced loop of teacher.py:140-171 over the prompt): xs = the stored layer inputs of that pass, layer l at
 * xs + l * layer_stride elements, [B, T_src, R] rows (T_src >= P; for a conditioned stack they already hold cb_l, as the
 * rings do).  Writes every slot of every layer ring of all ceil(B/32) groups (layout of srwn_generate_ring_elems): slot s
 * of layer l <- x_l[t] for the single t in [P-1-d_l, P-1] with t = s (mod d_l+1); zero where t < 0 or the utterance is
 * >= B (the causal padding both bodies rely on).  Then a *_resume launch with t0 = P continues the prompt.  dtype bf16
 * or fp32, R in {32, 64}; xs 16-byte aligned, layer_stride a multiple of 16 bytes; xs may be NULL when P = 0. */
int srwn_generate_ring_fill(const void* xs, int64_t layer_stride, int32_t T_src, int32_t P, const int32_t* dilations,
                            int32_t nlayers, int32_t B, int32_t R, void* ring, int32_t dtype, void* stream);

/* ---- generation pools (since srwn_version() 105): B slots over one set of rings, each slot holding its own stream at its
 * own step, so that streams join and leave a running batch.  The rings follow ONE clock, the launch's `clock`: step j of
 * the launch writes ring position (clock + j) mod (d_l+1) and reads the delayed tap at (clock + j + 1) mod (d_l+1), for
 * every slot alike; the causal padding comes only from the rings (a join zero-fills or prompt-fills its slot's rows).
 * What depends on a stream's own position is read per slot from `slots` [B]:
 *   t      the slot's own step of its next sample: step j of the launch is the slot's step t_u = t + j for both samplers'
 *          counters -- softmax (seed, 0, t_u), mixture (seed, 0, t_u*(M+1)+m): a slot draws what a batch-of-one run with
 *          that seed draws, whichever slot it sits in -- and for the conditioning frame clamp(t_u / pool_stride, 0,
 *          cond_frames-1) of its rows [u*cond_frames, (u+1)*cond_frames) of cond;
 *   t_end  the slot runs while t_u < t_end (t_end <= t: idle).  audio_out / codes_out / logits_out rows and the carry are
 *          written only for steps that run; other rows keep what the caller put there.  On return t += min(nsteps,
 *          max(t_end - t, 0));
 *   seed   the samplers' seed.
 * Steps and limits are int32: 2^31 steps is 37 hours at 16 kHz. */
typedef struct SrwnGenSlot {
  int32_t t;
  int32_t t_end;
  uint64_t seed;
} SrwnGenSlot;
/* Each *_slots entry point takes the arguments of its *_resume twin without `seed`, and (clock, carry, slots) in place of
 * (t0, carry): carry [B][2] and slots [B] are required; `forced` and `mode` apply to the whole launch.  Idle columns keep
 * computing (their ring rows are rewritten by the next join).  Argument errors (SRWN_E_*) return before any launch. */
int srwn_generate_slots(const void* wcr, const void* wskip, const void* w1, const void* w2, const float* bias_f,
                        const float* bias_r, const float* bs_sum, const float* b1, const float* b2, const float* init_w,
                        const float* init_b, void* ring, float* audio_out, int32_t* codes_out, float* logits_out,
                        const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                        int32_t nsteps, int32_t R, int32_t S, int32_t C, int32_t K, int32_t mode, int32_t dtype,
                        void* stream, int32_t clock, float* carry, SrwnGenSlot* slots);
int srwn_generate_mol_slots(const void* wcr, const void* wskip, const void* w1, const void* w2, const float* bias_f,
                            const float* bias_r, const float* bs_sum, const float* b1, const float* b2,
                            const float* init_w, const float* init_b, void* ring, float* audio_out, int32_t* codes_out,
                            float* logits_out, const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B,
                            int32_t Tout, int32_t nsteps, int32_t R, int32_t S, int32_t K, int32_t num_mixtures,
                            const void* cond, int32_t cond_frames, int32_t pool_stride, int64_t cond_ld, int32_t mode,
                            int32_t dtype, void* stream, int32_t clock, float* carry, SrwnGenSlot* slots);
int srwn_generate16_slots(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const float* bias_r,
                          const float* bs_sum, const float* b1, const float* b2, const float* init_w, const float* init_b,
                          void* ring, float* audio_out, int32_t* codes_out, float* logits_out, const float* forced,
                          const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R,
                          int32_t S, int32_t C, int32_t mode, void* stream, int32_t clock, float* carry,
                          SrwnGenSlot* slots);
int srwn_generate16_mol_slots(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const float* bias_r,
                              const float* bs_sum, const float* b1, const float* b2, const float* init_w,
                              const float* init_b, void* ring, float* audio_out, int32_t* codes_out, float* logits_out,
                              const float* forced, const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout,
                              int32_t nsteps, int32_t R, int32_t S, int32_t num_mixtures, const void* cond,
                              int32_t cond_frames, int32_t pool_stride, int64_t cond_ld, int32_t mode, void* stream,
                              int32_t clock, float* carry, SrwnGenSlot* slots);
/* The rings of pool slots after prompts, from ONE parallel forward pass over n prompts (layout as srwn_generate_ring_fill:
 * layer l at xs + l * layer_stride, [n, T_src, R] rows): row i fills the rows of slot dst[i] of every layer ring so that a
 * slot launch at `clock` continues it at its local step P[i] -- local step tau of that stream sits at ring position
 * (clock - P[i] + tau) mod (d_l+1), zero for tau < 0 (P[i] = 0 clears the slot).  dst and P are device int32 [n]; a row
 * whose dst is outside [0, B) or whose P is outside [0, T_src] is skipped.  Rows of slots not named are not touched.
 * xs may be NULL when every P[i] is 0. */
int srwn_generate_ring_fill_slots(const void* xs, int64_t layer_stride, int32_t T_src, int32_t n, const int32_t* dst,
                                  const int32_t* P, int32_t clock, const int32_t* dilations, int32_t nlayers, int32_t B,
                                  int32_t R, void* ring, int32_t dtype, void* stream);

/* ---- sampling controls of the generators (since srwn_version() 106): per utterance (or pool slot) a temperature, a
 * top-k and a nucleus (top-p) cut; the defaults (1, 1, 0) mean "off".  Softmax head, mode 1, on the step's fp32 logits:
 *   1. z = logits / temperature;
 *   2. the classes are ordered by z descending, equal values by lower class first (the tie rule of mode 0);
 *   3. top_k > 0: the first top_k classes of that order are kept (0: all C);
 *   4. top_p < 1: of the kept classes, the shortest prefix of that order whose softmax mass is >= top_p times the kept mass
 *      (at least one class stays);
 *   5. the draw is mode 1's over what is left, in class order: the first class whose inclusive prefix sum of exp(z - max)
 *      over the kept classes (dropped ones count 0) exceeds uniform * total, with the step's own uniform ((seed, u, t); in
 *      pools (seed, 0, t_u)): no new random numbers.  top_k = 1 is mode 0's argmax whatever the uniform is.
 * Mixture-of-logistics head, mode 1: the temperature only -- mixture = argmax_m(logit_m / temperature - log(-log u1_m)),
 * sample = mean + temperature * exp(max(log_scale, -7)) * (log u2 - log(1 - u2)), clipped as before; top_k / top_p are
 * not read.  Mode 0 ignores the controls.
 * The array is data and the kernels sanitise it: a temperature that is not finite or not > 0 counts as 1; a top_k outside
 * [0, C] counts as 0; a top_p outside (0, 1] (NaN included) counts as 1.  Whatever it holds, codes stay in [0, C) and the
 * audio finite.  `reserved` is not read (write 0). */
typedef struct SrwnGenSampling {
  float temperature;
  float top_p;
  int32_t top_k;
  int32_t reserved;
} SrwnGenSampling;
/* Each *_sampled entry point takes the arguments of the *_resume / *_slots call it is named after, plus `sampling`: a DEVICE
 * array of B entries (one per utterance / per slot; a join writes its slot's entry as it writes the slot's carry), read
 * once per launch; NULL = all defaults.  An utterance whose entry is all defaults, an idle slot, and every utterance of a
 * launch with sampling = NULL run the code of the calls above and return their bits: those calls ARE these with NULL. */
int srwn_generate_resume_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2, const float*
                                 bias_f, const float* bias_r, const float* bs_sum, const float* b1, const float* b2,
                                 const float* init_w, const float* init_b, void* ring, float* audio_out, int32_t*
                                 codes_out, float* logits_out, const float* forced, const int32_t* dilations, int32_t
                                 nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R, int32_t S, int32_t C,
                                 int32_t K, int32_t mode, uint64_t seed, int32_t dtype, void* stream, int32_t t0,
                                 float* carry, const SrwnGenSampling* sampling);
int srwn_generate_mol_resume_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2, const float*
                                     bias_f, const float* bias_r, const float* bs_sum, const float* b1, const float*
                                     b2, const float* init_w, const float* init_b, void* ring, float* audio_out,
                                     int32_t* codes_out, float* logits_out, const float* forced, const int32_t*
                                     dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R,
                                     int32_t S, int32_t K, int32_t num_mixtures, const void* cond, int32_t
                                     cond_frames, int32_t pool_stride, int64_t cond_ld, int32_t mode, uint64_t seed,
                                     int32_t dtype, void* stream, int32_t t0, float* carry, const SrwnGenSampling*
                                     sampling);
int srwn_generate16_resume_sampled(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const float*
                                   bias_r, const float* bs_sum, const float* b1, const float* b2, const float* init_w,
                                   const float* init_b, void* ring, float* audio_out, int32_t* codes_out, float*
                                   logits_out, const float* forced, const int32_t* dilations, int32_t nlayers, int32_t
                                   B, int32_t Tout, int32_t nsteps, int32_t R, int32_t S, int32_t C, int32_t mode,
                                   uint64_t seed, void* stream, int32_t t0, float* carry, const SrwnGenSampling*
                                   sampling);
int srwn_generate16_mol_resume_sampled(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const
                                       float* bias_r, const float* bs_sum, const float* b1, const float* b2, const
                                       float* init_w, const float* init_b, void* ring, float* audio_out, int32_t*
                                       codes_out, float* logits_out, const float* forced, const int32_t* dilations,
                                       int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R, int32_t S,
                                       int32_t num_mixtures, const void* cond, int32_t cond_frames, int32_t
                                       pool_stride, int64_t cond_ld, int32_t mode, uint64_t seed, void* stream,
                                       int32_t t0, float* carry, const SrwnGenSampling* sampling);
int srwn_generate_slots_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2, const float*
                                bias_f, const float* bias_r, const float* bs_sum, const float* b1, const float* b2,
                                const float* init_w, const float* init_b, void* ring, float* audio_out, int32_t*
                                codes_out, float* logits_out, const float* forced, const int32_t* dilations, int32_t
                                nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R, int32_t S, int32_t C,
                                int32_t K, int32_t mode, int32_t dtype, void* stream, int32_t clock, float* carry,
                                SrwnGenSlot* slots, const SrwnGenSampling* sampling);
int srwn_generate_mol_slots_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2, const float*
                                    bias_f, const float* bias_r, const float* bs_sum, const float* b1, const float*
                                    b2, const float* init_w, const float* init_b, void* ring, float* audio_out,
                                    int32_t* codes_out, float* logits_out, const float* forced, const int32_t*
                                    dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R,
                                    int32_t S, int32_t K, int32_t num_mixtures, const void* cond, int32_t cond_frames,
                                    int32_t pool_stride, int64_t cond_ld, int32_t mode, int32_t dtype, void* stream,
                                    int32_t clock, float* carry, SrwnGenSlot* slots, const SrwnGenSampling* sampling);
int srwn_generate16_slots_sampled(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const float*
                                  bias_r, const float* bs_sum, const float* b1, const float* b2, const float* init_w,
                                  const float* init_b, void* ring, float* audio_out, int32_t* codes_out, float*
                                  logits_out, const float* forced, const int32_t* dilations, int32_t nlayers, int32_t
                                  B, int32_t Tout, int32_t nsteps, int32_t R, int32_t S, int32_t C, int32_t mode,
                                  void* stream, int32_t clock, float* carry, SrwnGenSlot* slots, const
                                  SrwnGenSampling* sampling);
int srwn_generate16_mol_slots_sampled(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const
                                      float* bias_r, const float* bs_sum, const float* b1, const float* b2, const
                                      float* init_w, const float* init_b, void* ring, float* audio_out, int32_t*
                                      codes_out, float* logits_out, const float* forced, const int32_t* dilations,
                                      int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R, int32_t S,
                                      int32_t num_mixtures, const void* cond, int32_t cond_frames, int32_t
                                      pool_stride, int64_t cond_ld, int32_t mode, void* stream, int32_t clock, float*
                                      carry, SrwnGenSlot* slots, const SrwnGenSampling* sampling);
/* The draw of steps 1-5 on rows the caller chooses (the device function the generators call): logits [rows, ld] fp32 (C
 * <= 256 columns used, ld >= C), sampling [rows] or NULL (defaults), uniforms [rows] in (0, 1), codes_out [rows]. */
int srwn_sample_filtered(const float* logits, int64_t ld, const SrwnGenSampling* sampling, const float* uniforms,
                         int32_t* codes_out, int64_t rows, int32_t C, void* stream);

/* ---- discretised mixture-of-logistics loss of the reference's live teacher:
 * discretized_mix_logistic_loss (ops.py:124-175, sum_all=True) on logits [rows, ldl] fp32 whose first 4*M
 * columns are (logit_probs, means, log_scales, coeffs) and targets x [rows] in [-1,1]:
 *   loss = -sum_rows logsumexp_m( log p_m(x) + log_softmax(logit_probs)_m )   (bin half-width 1/255, log-scale
 *   floor -7, the four tf.where branches of ops.py:169; the coeffs never reach the loss)
 * loss_partials: one float per 256 rows (sum with srwn_reduce_loss);  dlogits [rows, ldd] in `dtype`,
 * = d loss / d logits * grad_scale, columns >= 4*M written as 0. */
int srwn_mol_loss(const float* logits, int64_t ldl, const float* x, int32_t M, float* loss_partials, void* dlogits,
                  int64_t ldd, int64_t rows, float grad_scale, int32_t dtype, void* stream);

/* Same loss on the student's output (model.py:374): the teacher logits are constants (stop_gradient,
 * model.py:334), the gradient wanted is dx[row] = d loss / d x[row] * grad_scale (fp32). */
int srwn_mol_loss_dx(const float* logits, int64_t ldl, const float* x, int32_t M, float* loss_partials, float* dx,
                     int64_t rows, float grad_scale, void* stream);

/* ---- Parallel-WaveNet student (class ParallelWaveNet, model.py:290-537).
 * A flow (createPartialFlow/createFlow, model.py:415-487) is the conditioned residual stack above WITHOUT the skip
 * path, then  prm = relu(h_L) @ W2[R,2] + b2;  scale = exp(prm0), mean = prm1;  x_out = x_in*scale + mean.
 *   srwn_flow_affine_fwd: prm [rows,2] and x_out [rows] (fp32); ent_partials[srwn_flow_partials(rows)] = block sums
 *                         of prm0 = log scale (entropy = sum over flows + 2*rows, model.py:356)
 *   srwn_flow_affine_bwd: dprm0 = dx_out*x_in*scale + ent_grad, dprm1 = dx_out;  dx_in = dx_out*scale;
 *                         g [rows,R] (dtype) = (h_L > 0) * (dprm @ W2^T) = G_L for srwn_residual_layer_bwd(has_up=2);
 *                         w_partials[block][2R+2] = (relu(h_L)^T dprm | column sums of dprm): srwn_reduce_partials
 * ent_grad carries d(-alpha*entropy/B)/d prm0 = -alpha/B (model.py:376-379). */
int64_t srwn_flow_partials(int64_t rows);
int srwn_flow_affine_fwd(const void* h, const float* w2, const float* b2, const float* x_in, float* prm, float* x_out,
                         float* ent_partials, int64_t rows, int32_t R, int32_t dtype, void* stream);
int srwn_flow_affine_bwd(const void* h, const float* w2, const float* prm, const float* x_in, const float* dx_out,
                         float ent_grad, void* g, float* dx_in, float* w_partials, int64_t rows, int32_t R,
                         int32_t dtype, void* stream);

/* ---- out = tf.minimum(tf.maximum(x, lo), hi) (model.py:535) and its gradient dx = dy where lo <= x <= hi, else 0
 * (dx may alias dy). */
int srwn_clamp(const float* x, float* y, int64_t n, float lo, float hi, void* stream);
int srwn_clamp_bwd(const float* x, const float* dy, float* dx, int64_t n, float lo, float hi, void* stream);

/* ---- chunked synthesis with the student (since srwn_version() 107): the flows of model.py:415-535 as an inference-only
 * stream.  A batch of B streams is synthesised in chunks [t0, t0 + n) of absolute time, t0 read from a DEVICE clock (one
 * int64 per synthesizer state), so the same launch arguments -- and a captured graph -- serve every chunk of a size.
 * Per flow and stream the state is the carry (the flow input's samples x[t0-1], x[t0-2], fp32 [B,2]) and, for every
 * layer group (srwn_group_plan), a boundary buffer [B][hist + max_chunk][R] (dtype) whose first hist = sum of the group's
 * dilations rows hold the group's input rows of times [t0 - hist, t0) (zeros at the start) and whose next n rows hold
 * the chunk.  A tap or a conditioning frame is taken by absolute time: a tap at t < 0 is the conv's zero padding at every
 * layer (ops.py:9), the frame of time t is max(t, 0) / pool_stride, kept in row frame mod cond_frames of the table (a
 * ring, see 110 below; the identity while frame < cond_frames).  Every stored value has the bits the whole-clip entry
 * points give it.  Argument errors return SRWN_E_* before anything is launched: a null pointer
 * (-3), n < 1 or n > max_chunk or buffers too short (-2), R other than 32 / 64, K other than 2 or a group whose halo
 * (sum of dilations / their gcd) exceeds 31 (-4), an unknown dtype (-1).
 *
 *   srwn_flow_stream_in     model.py:423-424 + 431-435 for rows [hist, hist + n) of the flow's first boundary buffer:
 *                           RightShift + the K = 2 input conv (init_w [2,1,R], init_b [R], fp32) on x [B, x_stride]
 *                           fp32 (rows t < 0 of the chunk from the carry), rounded to dtype as srwn_causal_conv1d_fwd
 *                           rounds, then + cond0[b, frame] (the first layer's conditioning bias, rows of
 *                           cond_row_stride elements, cond_frames rows per stream) rounded as srwn_add_frame_bias.
 *   srwn_residual_group_fwd_stream
 *                           model.py:428-453 for one layer group (ops.py:23-46 per layer): srwn_residual_group_fwd on
 *                           the buffer x_in [B][in_clip_rows][R] = [hist history rows | n chunk rows], segments cut
 *                           over the chunk rows only, and ONLY the top layer's chunk rows stored, to rows
 *                           [out_hist, out_hist + n) of x_out [B][out_clip_rows][R] (the next group's buffer, or the
 *                           flow's top buffer with out_hist = 0).  No z, no inner layer's output.  cond_next[g] = the
 *                           conditioning bias of the layer above layer g, or NULL.  A group of one layer is allowed.
 *   srwn_flow_stream_out    model.py:451-452, 479-483 (+ 535 with clamp != 0) on rows [0, n) of the flow's top buffer
 *                           h [B][top_clip_rows][R]: x_out = x_in * exp(p0) + p1 in srwn_flow_affine_fwd's arithmetic
 *                           (x_in, x_out fp32 [B, x_stride]); renews the carry from x_in; moves rows [n, n + hist) of
 *                           every buffer of roll_table (nroll int64 triples {address, rows per stream, hist}, a device
 *                           array) to its front -- the next chunk's history; an overlapping move when n < hist, walked
 *                           front to back -- and, with advance_clock != 0 (the last flow), adds n to *clock.
 *   srwn_logistic_noise     the first flow's input (student.py:100 draws it on the host): noise[b, j] = temperature[b]
 *                           * (log u - log(1 - u)), u from the counter-based bits of (seed[b], *clock + j): splitmix64
 *                           as srwn_categorical_sample mixes it, the TOP 23 BITS k of the result, u = (k + 1/2) / 2^23.
 *                           So 2^-24 <= u <= 1 - 2^-24, both u and 1 - u are exact and positive in fp32 and every
 *                           draw is finite (|noise| <= 16.64).  Evaluated as +-log1p(|2u - 1| / min(u, 1 - u)), whose
 *                           operands are exact: a few ulp at every u, also where log u - log(1 - u) would cancel.
 *                           temperature, seed: device arrays [B] (fp32, uint64).  temperature 0 writes +0.
 *   srwn_logistic_from_bits out[i] = log u - log(1 - u) for k = bits[i] & 0x7fffff: the map above on bits the caller
 *                           chooses (tests: k = 0 and k = 2^23 - 1). */
int srwn_flow_stream_in(const float* x, int64_t x_stride, const float* carry, const float* init_w, const float* init_b,
                        const void* cond0, int32_t cond_frames, int32_t pool_stride, int64_t cond_row_stride, void* out,
                        int64_t out_clip_rows, int32_t out_hist, int32_t B, int32_t n, int32_t max_chunk, int32_t R,
                        int32_t dtype, const int64_t* clock, void* stream);
int srwn_residual_group_fwd_stream(const void* x_in, int64_t in_clip_rows, void* x_out, int64_t out_clip_rows,
                                   int32_t out_hist, const void* const* wconv, const void* const* wres,
                                   const float* const* bias_f, const float* const* bias_r,
                                   const void* const* cond_next, int32_t cond_frames, int32_t pool_stride,
                                   int32_t cond_row_stride, const int32_t* dilations, int32_t nlayers, int32_t B,
                                   int32_t n, int32_t max_chunk, int32_t R, int32_t K, int32_t dtype,
                                   const int64_t* clock, void* stream);
int srwn_flow_stream_out(const void* h, int64_t top_clip_rows, const float* flow_w, const float* flow_b,
                         const float* x_in, float* x_out, int64_t x_stride, float* carry, int32_t clamp,
                         const int64_t* roll_table, int32_t nroll, int32_t B, int32_t n, int32_t max_chunk, int32_t R,
                         int32_t dtype, int64_t* clock, int32_t advance_clock, void* stream);
int srwn_logistic_noise(float* noise, int64_t noise_stride, const float* temperature, const uint64_t* seed,
                        const int64_t* clock, int32_t B, int32_t n, void* stream);
int srwn_logistic_from_bits(const uint32_t* bits, float* out, int64_t n, void* stream);

/* ---- student synthesis pools (since srwn_version() 108): the four launches above for `capacity` SLOTS over one set of
 * flow buffers, every slot a stream at a clock of its own.  The device table slots[capacity] replaces the clock:
 *   t      absolute time of the slot's next sample          t_end   where its stream ends
 * A slot is live when t < t_end and owns ran = clamp(t_end - t, 0, n) rows of a chunk of n: rows [0, ran) of its chunk
 * are computed with time t + row (taps before time 0 are the zero padding, frames by t + row, noise counter t + row), so
 * a stream has the bits the clock forms give a batch of one, in any slot, whenever it joined and whatever the other slots
 * hold.  A slot with ran = 0 has no group segment and no history roll (its segments end at the table entry); the noise,
 * entry and exit launches still start its threads, and the exit launch writes its row of zeros.  The segment cut
 * of the group launch depends on (capacity, n, stride, halo) and the chip alone, so a captured graph serves every chunk
 * of its size.  temperature / seed stay device arrays [capacity].  Argument errors as above, plus capacity < 1 (-2).
 *
 *   srwn_logistic_noise_slots            noise[u, j] for j < ran(u), counter slots[u].t + j; other entries untouched.
 *   srwn_flow_stream_in_slots            rows [hist, hist + ran(u)) of slot u, frame of time slots[u].t + row.
 *   srwn_residual_group_fwd_stream_slots buffer row 0 of slot u sits at time slots[u].t - hist.
 *   srwn_flow_stream_out_slots           x_out[u, j] for j < ran(u), +0 for ran(u) <= j < n (free slots: a row of zeros);
 *                                        the carry and the history roll (by ran(u) rows) of the slots with ran > 0; with advance != 0 (the
 *                                        last flow) slots[u].t += ran(u) for the live slots, by the workgroup that finishes
 *                                        last (`arrive`: one device int32, zero before the first launch and zero again
 *                                        after every launch that completes; a caller re-zeroes it after a failed
 *                                        one), since every workgroup of the launch reads the table.
 *   srwn_flow_stream_reset_slots         what a join needs: zeroes rows [0, hist) of slot u of every buffer of roll_table
 *                                        (the tables of all flows, nroll triples) and carry[f][u][0..1] for f < ncarry
 *                                        (carry + f * carry_stride floats), for the nslots slots of the device array
 *                                        slot_ids (int32; ids outside [0, capacity) are ignored). */
typedef struct SrwnSynthSlot {
  int64_t t;
  int64_t t_end;
} SrwnSynthSlot;

int srwn_logistic_noise_slots(float* noise, int64_t noise_stride, const float* temperature, const uint64_t* seed,
                              const SrwnSynthSlot* slots, int32_t capacity, int32_t n, void* stream);
int srwn_flow_stream_in_slots(const float* x, int64_t x_stride, const float* carry, const float* init_w,
                              const float* init_b, const void* cond0, int32_t cond_frames, int32_t pool_stride,
                              int64_t cond_row_stride, void* out, int64_t out_clip_rows, int32_t out_hist,
                              int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t dtype,
                              const SrwnSynthSlot* slots, void* stream);
int srwn_residual_group_fwd_stream_slots(const void* x_in, int64_t in_clip_rows, void* x_out, int64_t out_clip_rows,
                                         int32_t out_hist, const void* const* wconv, const void* const* wres,
                                         const float* const* bias_f, const float* const* bias_r,
                                         const void* const* cond_next, int32_t cond_frames, int32_t pool_stride,
                                         int32_t cond_row_stride, const int32_t* dilations, int32_t nlayers,
                                         int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t K,
                                         int32_t dtype, const SrwnSynthSlot* slots, void* stream);
int srwn_flow_stream_out_slots(const void* h, int64_t top_clip_rows, const float* flow_w, const float* flow_b,
                               const float* x_in, float* x_out, int64_t x_stride, float* carry, int32_t clamp,
                               const int64_t* roll_table, int32_t nroll, int32_t capacity, int32_t n, int32_t max_chunk,
                               int32_t R, int32_t dtype, SrwnSynthSlot* slots, int32_t* arrive, int32_t advance,
                               void* stream);
int srwn_flow_stream_reset_slots(const int64_t* roll_table, int32_t nroll, float* carry, int32_t ncarry,
                                 int64_t carry_stride, const int32_t* slot_ids, int32_t nslots, int32_t capacity,
                                 int32_t R, int32_t dtype, void* stream);

/* ---- live synthesis (since srwn_version() 110): the conditioning tables of the four stream launches above (and of their
 * slot forms) are RINGS.  A table holds cond_frames rows per stream; frame q of a stream (q = time / pool_stride, 0 for a
 * time before the start) is looked up in row q mod cond_frames.  A caller that writes a stream's whole encoding once
 * (frames < cond_frames, as every caller before 110 does) sees the identity, and those entry points keep their
 * signatures and their bits.  A caller that keeps FEEDING a running stream writes frame q to row q mod cond_frames
 * while the stream runs, and may do so as long as no frame a later launch still reads is overwritten: a chunk starting
 * at time t recomputes the halo rows of a group back to t - hist, so with hist_max the largest history of the flow's
 * groups the oldest frame still read is max(t - hist_max, 0) / pool_stride, and after `fed` frames the ring has room for
 *     max(0, cond_frames - fed + max(t - hist_max, 0) / pool_stride)
 * more.  A launch then never spans cond_frames frames: the group kernel reduces the first frame of a segment modulo
 * cond_frames once, on the scalar side, and wraps a row with one compare and subtract (no 64-bit division per tile).
 * Rows a tile computes but never stores (padding rows, rows of idle slots) may read any row of the ring; the lookup
 * stays inside the table for them.
 *
 *   srwn_cond_ring_feed   for ONE flow: projects the new frames of n streams through the packed conditioning image of all
 *                         L layers (wpack: the image srwn_pw_linear_ychunks takes, Cin = the padded encoding width, a
 *                         multiple of 16; bias [L*R] fp32) and writes them into the ring table [L][capacity *
 *                         cond_frames][R] (dtype).  Entry i < n names stream streams[i] (int32, distinct), its first
 *                         new frame first_frame[i] (int64, absolute) and counts[i] (int32) frames, all DEVICE arrays;
 *                         frame j of the entry is read from row streams[i] * x_stream_rows + j of x (rows of
 *                         x_row_stride elements, dtype) and written to row streams[i] * cond_frames + (first_frame[i] +
 *                         j) mod cond_frames of every layer.  One launch however many streams are fed.  The rows it
 *                         writes have the bits srwn_pw_linear_ychunks writes for the same frame, image and dtype (one
 *                         device body serves both).  max_k bounds the counts (the grid is sized by it; a larger count is
 *                         cut at max_k).  Errors before any launch: a null pointer (-3); cond_frames < 1, max_k >
 *                         cond_frames (more frames at once than the ring holds), n > capacity (more streams than the table
 *                         holds), x_stream_rows < max_k, Cin not a multiple of 16 (-2); R other than 32 / 64 (-4); an
 *                         unknown dtype (-1).  The device arrays cannot be read before the launch: an entry whose stream
 *                         lies outside [0, capacity) or whose first frame is negative is skipped by the kernel, as
 *                         srwn_flow_stream_reset_slots skips such ids.  n = 0 or max_k = 0: nothing to do (0). */
int srwn_cond_ring_feed(const void* x, int64_t x_row_stride, int64_t x_stream_rows, int32_t Cin, const void* wpack,
                        const float* bias, void* table, int32_t L, int32_t R, int32_t cond_frames, int32_t capacity,
                        const int32_t* streams, const int64_t* first_frame, const int32_t* counts, int32_t n,
                        int32_t max_k, int32_t dtype, void* stream);

/* ---- live autoregressive decoding (since srwn_version() 112): the conditioned mixture-of-logistics decoder of
 * srwn_generate_mol_resume_sampled / srwn_generate16_mol_resume_sampled over a conditioning table that is a RING, so that
 * the encoder's frames can be fed while the decoder runs and a stream is not bounded by the table it started with.  The
 * two *_live_sampled entry points take the arguments of their *_mol_resume_sampled twins; `cond` is required and
 * cond_frames is the ring length: the table is [B * cond_frames, cond_ld] (the layout of the twins), and frame q = t /
 * pool_stride of stream u is looked up in row u * cond_frames + q mod cond_frames (the twins: min(q, cond_frames - 1)).
 * A step reads the row of its own frame only, so after `fed` frames a run at step t has room for
 *     cond_frames - fed + t / pool_stride
 * more (no history term: nothing older than the current frame is read again).  The latency body requests layer 0's
 * operands of step t + 1 during step t; after a launch's last step that row may belong to a frame not fed yet: the ring
 * lookup keeps it inside the table and its value is never used (the next launch requests it again).  Neither body reads
 * ahead otherwise.  Every other argument, the carry, the rings and the random draws are the twins': a live run over a
 * ring returns the bits of the twin over the whole table.  Kernels of their own; the twins' launches run the code they
 * ran before.  Errors before any launch: a null cond (-3); cond_frames < 1, pool_stride < 1, cond_ld < nlayers * R
 * (latency body: or not a multiple of 4) (-2); then the twins' checks.
 *
 *   srwn_cond_ring_scatter   the feed: rows [B * k, rows_ld] (dtype; row u * k + j = the conditioning biases of all
 *                                layers, srwn_pw_linear's output, of new frame first_frame + j of stream u) -> row
 *                                u * cond_frames + (first_frame + j) mod cond_frames of table [B * cond_frames, cond_ld];
 *                                `width` elements per row in 16-byte vectors.  One launch however many streams.  Errors
 *                                before any launch: a null pointer (-3); k > cond_frames, cond_frames < 1, first_frame <
 *                                0, a width, leading dimension or address that is not a whole number of vectors, width
 *                                beyond a leading dimension (-2); an unknown dtype (-1).  B = 0 or k = 0: nothing (0). */
int srwn_generate_mol_live_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2, const float*
                                   bias_f, const float* bias_r, const float* bs_sum, const float* b1, const float* b2,
                                   const float* init_w, const float* init_b, void* ring, float* audio_out, int32_t*
                                   codes_out, float* logits_out, const float* forced, const int32_t* dilations,
                                   int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R, int32_t S,
                                   int32_t K, int32_t num_mixtures, const void* cond, int32_t cond_frames, int32_t
                                   pool_stride, int64_t cond_ld, int32_t mode, uint64_t seed, int32_t dtype, void*
                                   stream, int32_t t0, float* carry, const SrwnGenSampling* sampling);
int srwn_generate16_mol_live_sampled(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const
                                     float* bias_r, const float* bs_sum, const float* b1, const float* b2, const
                                     float* init_w, const float* init_b, void* ring, float* audio_out, int32_t*
                                     codes_out, float* logits_out, const float* forced, const int32_t* dilations,
                                     int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R, int32_t S,
                                     int32_t num_mixtures, const void* cond, int32_t cond_frames, int32_t
                                     pool_stride, int64_t cond_ld, int32_t mode, uint64_t seed, void* stream,
                                     int32_t t0, float* carry, const SrwnGenSampling* sampling);
int srwn_cond_ring_scatter(const void* rows, int64_t rows_ld, void* table, int64_t cond_ld, int32_t B, int32_t k,
                               int64_t first_frame, int32_t cond_frames, int32_t width, int32_t dtype, void* stream);

/* ---- live slots in generation pools (since srwn_version() 114): the slot form of the conditioned mixture-of-logistics
 * decoder (srwn_generate_mol_slots_sampled / srwn_generate16_mol_slots_sampled) over per-slot conditioning RINGS, so that
 * a pool slot is fed its encoding while it runs.  The two *_live_slots_sampled entry points take the arguments of their
 * *_mol_slots_sampled twins; `cond` is required and cond_frames is the ring length of every slot: the table is
 * [B * cond_frames, cond_ld], and slot u at its OWN step t_u looks its frame q = t_u / pool_stride up in row
 * u * cond_frames + q mod cond_frames (a true modulus: an idle slot may hold any t).  A slot with t_end <= cond_frames *
 * pool_stride whose frames sit in rows 0.. (a bounded stream) reads what the twins read.  The host raises a live slot's
 * t_end to fed * pool_stride as it feeds it; a slot that reaches t_end inside a launch, or before it, idles as in the
 * twins -- except that an idle column does NOT store into the layer rings: its ring rows stay exactly as its last own
 * step left them (everything else of an idle column still computes on junk and is dropped).  The rings follow the pool's
 * clock, so before the launch in which such a slot runs again its columns are realigned:
 *
 *   srwn_generate_ring_rotate_slots  for i < n, slot u = slot_ids[i] and every layer l with depth D = d_l + 1:
 *                                new[(p + shift[i]) mod D] = old[p] for p in [0, D), over the slot's R elements, in the
 *                                ring layout of srwn_generate_ring_elems (slot u: group u / 32, row u mod 32).  shift[i] =
 *                                (clock of the slot's next own step) - (clock at which its last own step ended) >= 0.  In
 *                                place, any shift and dilation: one owner workgroup per (slot, layer) column, three
 *                                reversals of disjoint swaps.  Slots not listed, an entry outside [0, capacity) or with a
 *                                negative shift, and a shift that is 0 mod D keep their bits.  slot_ids (device, int32 [n])
 *                                must be distinct.  Errors before any launch: n < 0, n > 65535, capacity < 1, a layer count
 *                                outside 1..64, a dilation < 1, a ring not 16-byte aligned (-2); a null pointer (-3); R not
 *                                32 or 64 (-4); an unknown dtype (-1).  n = 0: nothing (0).
 *   srwn_cond_ring_scatter_slots    the feed of ragged slots: row i of rows [n_rows, rows_ld] (srwn_pw_linear's output
 *                                for one new frame) -> row dst_row[i] (device, int32 [n_rows]) of table [table_rows,
 *                                cond_ld]; the host computes dst_row = slot * cond_frames + (fed_slot + j) mod cond_frames.
 *                                `width` elements per row in 16-byte vectors; a destination outside the table is skipped;
 *                                the destinations must be distinct (two rows to one destination would race).
 *                                One launch however many slots and frames.  Errors before any launch: n_rows < 0 (-2, checked
 *                                first); a null pointer (-3); table_rows < 1, a width, leading dimension or address that is not a whole
 *                                number of vectors, width beyond a leading dimension (-2); an unknown dtype (-1).  n_rows =
 *                                0: nothing (0).
 *
 * Kernels of their own; every earlier launch runs the code it ran before.  Errors of the generators before any launch: a
 * null cond (-3); cond_frames < 1, pool_stride < 1, cond_ld < nlayers * R (latency body: or not a multiple of 4) (-2);
 * then the twins' checks. */
int srwn_generate_mol_live_slots_sampled(const void* wcr, const void* wskip, const void* w1, const void* w2, const float*
                                         bias_f, const float* bias_r, const float* bs_sum, const float* b1, const float*
                                         b2, const float* init_w, const float* init_b, void* ring, float* audio_out,
                                         int32_t* codes_out, float* logits_out, const float* forced, const int32_t*
                                         dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R,
                                         int32_t S, int32_t K, int32_t num_mixtures, const void* cond, int32_t
                                         cond_frames, int32_t pool_stride, int64_t cond_ld, int32_t mode, int32_t dtype,
                                         void* stream, int32_t clock, float* carry, SrwnGenSlot* slots, const
                                         SrwnGenSampling* sampling);
int srwn_generate16_mol_live_slots_sampled(const void* wl, const void* wh1, const void* wh2, const float* bias_f, const
                                           float* bias_r, const float* bs_sum, const float* b1, const float* b2, const
                                           float* init_w, const float* init_b, void* ring, float* audio_out, int32_t*
                                           codes_out, float* logits_out, const float* forced, const int32_t* dilations,
                                           int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R, int32_t
                                           S, int32_t num_mixtures, const void* cond, int32_t cond_frames, int32_t
                                           pool_stride, int64_t cond_ld, int32_t mode, void* stream, int32_t clock,
                                           float* carry, SrwnGenSlot* slots, const SrwnGenSampling* sampling);
int srwn_generate_ring_rotate_slots(void* ring, const int32_t* dilations, int32_t nlayers, int32_t capacity, int32_t R,
                                    const int32_t* slot_ids, const int32_t* shift, int32_t n, int32_t dtype, void* stream);
int srwn_cond_ring_scatter_slots(const void* rows, int64_t rows_ld, void* table, int64_t cond_ld, int32_t n_rows, const
                                 int32_t* dst_row, int32_t table_rows, int32_t width, int32_t dtype, void* stream);

/* ---- data gradient of _DilatedCausalConv1d (ops.py:6-10) wrt a narrow input (the 1-channel flow input,
 * model.py:423-424); `shift` is the adjoint of RightShift (ops.py:78-80):
 *   dx[b,u,i] (+)= scale * sum_k sum_o w[k,i,o] * dy[b, u + shift + (K-1-k)*dilation, o]   (0 beyond the clip)
 * dy [B,T,Cout] in `dtype`, w [K,Cin,Cout] fp32, dx [B,T,Cin] fp32 (accumulate != 0 adds into it). */
int srwn_causal_conv1d_dgrad(const void* dy, const float* w, float* dx, int32_t B, int32_t T, int32_t Cin,
                             int32_t Cout, int32_t K, int32_t dilation, int32_t shift, int32_t accumulate, float scale,
                             int32_t dtype, void* stream);

/* ---- STFT power loss (model.py:360-371): tf.contrib.signal.stft(x, 512, 256) -> frames without end padding
 * (srwn_stft_frames(T) = 1 + (T-512)/256), periodic Hann window, 512-point real DFT (257 bins);
 *   srwn_stft_power    : power[b,f] = mean_frames |X[b,n,f]|^2;  spec [B,frames,257,2] keeps (Re,Im) for the
 *                        backward (may be NULL); frame_power [B,frames,257] is scratch
 *   srwn_power_loss    : loss = gamma * sum (power_truth - power_out)^2 (tf.norm(.)**2);  dpower (may be NULL)
 *                        = d(loss*grad_scale)/d power_out
 *   srwn_stft_power_bwd: dx[b,t] (+)= sum_f dpower[b,f] * d power[b,f] / d x[b,t] */
int32_t srwn_stft_frames(int32_t T);
int srwn_stft_power(const float* x, float* spec, float* frame_power, float* power, int32_t B, int32_t T, void* stream);
int srwn_power_loss(const float* power_truth, const float* power_out, int64_t n, float gamma, float grad_scale,
                    float* dpower, float* loss, void* stream);
int srwn_stft_power_bwd(const float* spec, const float* dpower, float* dx, int32_t B, int32_t T, int32_t accumulate,
                        void* stream);

/* ---- tf.clip_by_global_norm(grads, clip_norm) (model.py:385) + the Adam update with the clip factor on device:
 *   srwn_sumsq      : partials[srwn_sumsq_partials(n)] = chunk sums of g^2 (call once per gradient buffer, into
 *                     consecutive slices of one partials array)
 *   srwn_clip_scale : norm = pre_scale*sqrt(sum partials); out[0] = pre_scale*clip_norm/max(norm, clip_norm);
 *                     out[1] = norm   (pre_scale = 1/world when the buffers hold an all-reduced SUM)
 *   srwn_adam_step_scaled: srwn_adam_step with grad_scale read from device memory; tick=0 shares one step
 *                     counter between several parameter buffers (tick it on the first call of a step only) */
/* y += alpha * scale_dev[0] * x: accumulates per-row clipped gradients of the slow path ParallelWaveNet.train
 * (model.py:599-632) with the clip factor of srwn_clip_scale left on the device */
int srwn_axpy_dev(float* y, const float* x, const float* scale_dev, float alpha, int64_t n, void* stream);
int64_t srwn_sumsq_partials(int64_t n);
int srwn_sumsq(const float* g, int64_t n, float* partials, void* stream);
int srwn_clip_scale(const float* partials, int64_t n, float clip_norm, float pre_scale, float* out, void* stream);
int srwn_adam_step_scaled(float* params, const float* grads, float* m, float* v, int64_t n, int64_t* step, float lr,
                          float beta1, float beta2, float eps, const float* grad_scale_dev, int32_t tick,
                          void* stream);

/* ---- WaveNetAutoEncoder pieces (model.py:75-285).  The encoder (createEncoder, model.py:136-156) is a chain of
 * ResidualDilationLayerNC (ops.py:48-58): relu -> tf.layers.conv1d(K, SAME; the dilation argument is never passed
 * on) -> relu, then 1x1 residual and 1x1 skip; skips summed, 1x1 to latent_channels, average-pooled.
 *
 * srwn_tap_linear: time-tap GEMM on MFMA for 128 or 256 output channels --
 *   y[row][n] = epi( bias[n] + frame_add[clip*frames + t/pool_stride][n]*frame_add_scale
 *                    + sum_{tap<ntaps} sum_i x[row + tap*tap_step][i] * W[tap*Cin + i][n] )
 *   rows = clips*T; a tap that leaves its clip contributes 0 (SAME padding of the K=2 conv: tap_step=+1; its
 *   data gradient: tap_step=-1 with the transposed kernel); wpack = MFMA image [cout/32][ntaps*Cin/16] (natural k);
 *   epi = SRWN_EPI_NONE / _RELU / _MASK (aux > 0); frame_add (fp32, may be NULL) is the broadcast of a per-frame
 *   term (the pooled skip path's gradient, the adjoint of tf.nn.pool AVG model.py:154). */
int srwn_tap_linear(const void* x, int64_t x_row_stride, int32_t ntaps, int32_t tap_step, int32_t T, int32_t Cin,
                    const void* wpack, const float* bias, void* y, int64_t y_row_stride, int32_t cout, int64_t rows,
                    const void* aux, int64_t aux_row_stride, const float* frame_add, int64_t frame_add_ld,
                    int32_t frames, int32_t pool_stride, float frame_add_scale, int32_t epi, int32_t dtype,
                    void* stream);
/* One ResidualDilationLayerNC of the encoder as ONE launch (ops.py:48-58; bf16, 128 channels, K = 2 taps at t and
 * t+1; other shapes: SRWN_E_UNSUPPORTED -- use srwn_tap_linear):
 *   a_out[t] = relu(bias_c + sum_k r_in[t+k] . Wconv[k])     (a tap beyond the clip contributes 0)
 *   r_out[t] = relu(bias_r + a_out[t] . Wr)                   (the relu'd input of the next layer; NULL: skipped --
 *                                                              the last layer's residual output is unused, model.py:144-150)
 * wconv = MFMA image [4][16] natural k (k = tap*128 + in channel), wres = image [4][8] in permuted k order (its B
 * operand is the first product's accumulator tile).  a_bits / r_bits (may be NULL): srwn_nc_mask_words(B,T) 64-bit
 * words receiving the relu masks of a_out / r_out in the layout srwn_nc_layer_bwd reads (word [tile*64 + lane], one bit
 * per accumulator register of the lane: opaque outside srwn_nc.hip). */
int64_t srwn_nc_mask_words(int32_t B, int32_t T);
int srwn_nc_layer_fwd(const void* r_in, const void* wconv, const void* wres, const float* bias_c, const float* bias_r,
                      void* a_out, void* r_out, uint64_t* a_bits, uint64_t* r_bits, int32_t B, int32_t T, int32_t C,
                      int32_t K, int32_t dtype, void* stream);
/* the same mask words for a [B,T,128] bf16 tensor written by another kernel (x > 0) */
int srwn_nc_mask_bits(const void* x, uint64_t* bits, int32_t B, int32_t T, int32_t C, int32_t dtype, void* stream);
/* Its data gradient, pairing the conv of layer l with the 1x1 of the layer below (autodiff of ops.py:50-57):
 *   dh_out[t]   = [r[t] > 0] . sum_k dpre_up[t-k] . Wconv[k]^T                                      (= d loss / d r_l)
 *   dpre_out[t] = [a[t] > 0] . (dh_out[t] . Wr_below^T + frame_add[clip*frames + t/pool]*scale)       (NULL: skipped)
 * r_bits / a_bits = mask words of the layer's relu'd input and of the activation under the 1x1 below;
 * wconvT = image [4][16] natural k (rows = in channel, k = tap*128 + out channel), wresT = image [4][8] permuted k;
 * frame_add (fp32, may be NULL) is the pooled skip path's gradient broadcast over its frame (model.py:154). */
int srwn_nc_layer_bwd(const void* dpre_up, const void* wconvT, const uint64_t* r_bits, void* dh_out, const void* wresT,
                      const float* frame_add, int64_t frame_add_ld, int32_t frames, int32_t pool_stride,
                      float frame_add_scale, const uint64_t* a_bits, void* dpre_out, int32_t B, int32_t T, int32_t C,
                      int32_t K, int32_t dtype, void* stream);
/* weight gradients of the encoder's ResidualDilationLayerNC chain (ops.py:48-58), all layers in one pass over the saved
 * tensors ([L][rows][128] stacks, `layer_stride` elements apart; 128 channels, K = 2 taps at t and t+1):
 *   part_w [l][slab][k*128+i][o] = sum r_l[t+k, i] * dpre_l[t, o]   (taps beyond the clip contribute 0)
 *   part_r [l][slab][n][m]       = sum a_l[t, n] * dh_l[t, m];  part_b / part_br = column sums of dpre_l / dh_l
 * Finish with srwn_reduce_partials. */
int srwn_wgrad_nc_layers(const void* r, const void* a, const void* dpre, const void* dh, int64_t layer_stride,
                         int32_t nlayers, float* part_w, float* part_r, float* part_b, float* part_br, int64_t rows,
                         int32_t T, int32_t nslabs, int32_t C, int32_t K, int32_t dtype, void* stream);
/* first encoder layer on the raw clip (model.py:141-142): a[b,t,c] = relu(bias[c] + sum_k w[k][c]*relu(x[b,t+k])) */
int srwn_nc_input_fwd(const float* x, const float* w, const float* bias, void* a, int32_t B, int32_t T, int32_t C,
                      int32_t K, int32_t dtype, void* stream);
/* ---- the encoder for inference (since srwn_version() 109; csrc/srwn_ncstream.hip): the whole chain above for B streams x
 * `nframes` frames in one launch -- a_0 = relu(nc_conv(relu(x))), r_0, then a_{l+1} = relu(conv(r_l) + b_l),
 * r_{l+1} = relu(a_{l+1} Wr_l + br_l) for every layer, on chip -- leaving only the per-frame means of a_1..a_L:
 * means [nlayers][B*nframes][128] bf16, the layout srwn_pw_linear_ksplit consumes (x_chunk_stride = B*nframes*128).
 *   x          audio window [B][ld] fp32 whose row 0 is a frame boundary; valid_rows = real samples in it,
 *              nframes*pool_stride <= valid_rows <= nframes*pool_stride + nlayers + 1 (and <= ld).  Rows at or beyond
 *              valid_rows are past the end of the clip: the input of every layer is zero there (SAME padding).
 *   nc_w/nc_b  'nc_conv' [2][128] / [128] fp32; nc_wr: its 1x1 as image [4][8] in permuted k order; nc_br [128]
 *   wconv/wres layer l's images at + l*stride elements ([4][16] natural k / [4][8] permuted k, as srwn_nc_layer_fwd);
 *              bias_c / bias_r [nlayers][128] fp32.  The last layer's residual 1x1 is never read.
 *   partials   workspace of srwn_nc_encode_partials(B, nframes, pool_stride, nlayers) floats (fixed-order segment sums)
 * A frame's result depends on its own window only: not on its place in the launch, the streams beside it or nframes.
 * bf16, 128 channels, K = 2, at most srwn_nc_encode_max_layers() layers; fp32 or other widths: SRWN_E_UNSUPPORTED (run
 * the layers one launch each); argument errors return before any launch. */
int32_t srwn_nc_encode_max_layers(void);
int64_t srwn_nc_encode_partials(int32_t B, int32_t nframes, int32_t pool_stride, int32_t nlayers);
int srwn_nc_encode_frames(const float* x, int64_t ld, const float* nc_w, const float* nc_b, const void* nc_wr,
                          const float* nc_br, const void* wconv, int64_t wconv_stride, const void* wres,
                          int64_t wres_stride, const float* bias_c, const float* bias_r, float* partials, void* means,
                          int32_t B, int32_t nframes, int32_t pool_stride, int32_t valid_rows, int32_t nlayers, int32_t C,
                          int32_t K, int32_t dtype, void* stream);
/* ---- encoder pools (since srwn_version() 111; csrc/srwn_ncstream.hip): the same chain (createEncoder, model.py:136-156)
 * over a LIST of frames of independent streams, each at a clock of its own.  A stream's audio lives in its row of a ring
 * [capacity][ring_len] fp32, sample s in column s mod ring_len; a frame reads its own pool_stride + nlayers + 1 samples
 * and nothing else, so a launch is any list of frames of any streams.
 *
 *   SrwnEncFrame                  one item of a launch (16 bytes, a DEVICE array): the row of the ring, the ring column
 *                                 of the frame's first sample (first_sample mod ring_len, reduced on the host), and the
 *                                 number of real samples from there on: pool_stride + nlayers + 1 for a frame whose
 *                                 look-ahead is complete, fewer (>= pool_stride) at the end of a clip, where the missing
 *                                 rows are the SAME padding.  Rows are counted from the frame's first sample and a row
 *                                 >= valid is never loaded, so a column still holding an older sample is unreachable.
 *   srwn_nc_encode_frame_list     srwn_nc_encode_frames with workgroup (segment, item) instead of (segment, frame,
 *                                 stream): means [nlayers][nitems][128] bf16 (srwn_pw_linear_ksplit with rows =
 *                                 nitems), partials = srwn_nc_encode_list_partials(nitems, pool_stride, nlayers)
 *                                 floats.  One device body serves both entries (two instantiations that differ in the
 *                                 addressing only; every sum keeps its fixed order), so item i has the bits of the same
 *                                 window as a one-frame srwn_nc_encode_frames call, whatever the other items hold.  The
 *                                 table cannot be read before the launch: an item whose stream lies outside [0,
 *                                 capacity), whose col lies outside [0, ring_len) or whose valid lies outside
 *                                 [pool_stride, pool_stride + nlayers + 1] is skipped and its row of means is zero, as
 *                                 srwn_cond_ring_feed skips such ids.  Errors before any launch: a null pointer (-3);
 *                                 ring_len < pool_stride + nlayers + 1, nitems < 0 or > 65535, capacity < 1,
 *                                 pool_stride < 1, nlayers outside 1..srwn_nc_encode_max_layers() (-2); C, K or a
 *                                 dtype the chain is not built for (-4; an unknown dtype -1); nitems = 0: nothing (0).
 *   srwn_audio_ring_put           new audio into the rings, one launch however many streams: entry i < n copies
 *                                 counts[i] floats from src + src_offset[i] to row streams[i], columns (first_col[i] +
 *                                 j) mod ring_len.  streams, src_offset, first_col, counts: int32 DEVICE arrays (they
 *                                 may share one upload with src); max_count bounds the counts (the grid is sized by it,
 *                                 a larger count is cut).  An entry whose stream lies outside [0, capacity), whose
 *                                 first_col lies outside [0, ring_len) or whose offset is negative is skipped.  Errors:
 *                                 a null pointer (-3); ring_len < 1, capacity < 1, n < 0 or > 65535, max_count < 0 or >
 *                                 ring_len (-2); n = 0 or max_count = 0: nothing (0). */
typedef struct SrwnEncFrame {
  int32_t stream;   /* row of the audio ring, 0 .. capacity-1 */
  int32_t col;      /* ring column of the frame's first sample */
  int32_t valid;    /* real samples from the frame's first sample on */
  int32_t reserved; /* 0 */
} SrwnEncFrame;
int64_t srwn_nc_encode_list_partials(int32_t nitems, int32_t pool_stride, int32_t nlayers);
int srwn_nc_encode_frame_list(const float* ring, int32_t ring_len, int32_t capacity, const SrwnEncFrame* frames,
                              int32_t nitems, const float* nc_w, const float* nc_b, const void* nc_wr,
                              const float* nc_br, const void* wconv, int64_t wconv_stride, const void* wres,
                              int64_t wres_stride, const float* bias_c, const float* bias_r, float* partials,
                              void* means, int32_t pool_stride, int32_t nlayers, int32_t C, int32_t K, int32_t dtype,
                              void* stream);
int srwn_audio_ring_put(float* ring, int32_t ring_len, int32_t capacity, const float* src, const int32_t* streams,
                        const int32_t* src_offset, const int32_t* first_col, const int32_t* counts, int32_t n,
                        int32_t max_count, void* stream);
/* small products on the [B*frames] axis (latent 1x1 model.py:152, gradient wrt the encoding through model.py:180):
 *   C[m][n] = (accumulate ? C : 0) + bias[n] + sum_k A(m,k)*B(k,n), chunked addressing on both operands:
 *   A(m,k) = a[(k/a_chunk)*a_chunk_stride + m*lda + k%a_chunk];  B(k,n) = b[(k/b_chunk)*b_chunk_stride + (k%b_chunk)*ldb_k + n*ldb_n]
 *   srwn_small_wgrad: c[k][n] = scale*sum_m a[m][k]*d[m][n], bias_out[n] = scale*sum_m d[m][n] (may be NULL) */
int srwn_small_gemm(const void* a, int64_t lda, int32_t a_chunk, int64_t a_chunk_stride, int32_t a_dtype,
                    const float* b, int64_t ldb_k, int64_t ldb_n, int32_t b_chunk, int64_t b_chunk_stride,
                    const float* bias, void* c, int64_t ldc, int32_t c_dtype, int32_t M, int32_t N, int32_t K,
                    int32_t accumulate, void* stream);
int srwn_small_wgrad(const float* a, int64_t lda, const float* d, int64_t ldd, float* c, float* bias_out, int32_t M,
                     int32_t K, int32_t N, float scale, void* stream);
/* sample_from_discretized_mix_logistic (ops.py:178-201) given the uniform draws u1 [rows,M], u2 [rows] in
 * (1e-5, 1-1e-5): Gumbel-max mixture choice, logistic sample, clip to [-1,1] -> out [rows] */
int srwn_mol_sample(const float* logits, int64_t ldl, int32_t M, const float* u1, const float* u2, float* out,
                    int64_t rows, void* stream);

/* ---- streaming classifier (since srwn_version() 113; csrc/srwn_recog.hip, csrc/srwn_group.hip): the causal stack of class
 * WaveNet (createNetwork, model.py:33-62: input conv 40, residual layers 42-47, skip sum 50-51, head 1x1s 53-56, the
 * sliding AVG pool 58 and the softmax 60) as an inference-only stream over audio of any length.  The input placeholder
 * of the reference graph is [None, None]: on T > input_size samples the VALID pool yields T - input_size + 1 rows, one
 * per window position; a stream emits the row of every `hop`-th position.  `window` is a multiple of `hop`; the stack
 * advances by whole hops at hop-aligned absolute times only (audio that does not fill a hop waits with the caller).
 *   H_j = sum of r1[t] over t in [j * hop, (j + 1) * hop)            fp32 [S], r1 = relu(W1 relu(sum_l skip_l + bs) + b1)
 *   e_j = softmax(((H_{j-nW+1} + ... + H_j) / window) @ W2 + b2)     nW = window / hop, j >= nW - 1, oldest block first
 * e_j is the graph's pooled output at position (j + 1) * hop - window.  State of a batch of B streams: a device clock
 * (int64 absolute time of the next chunk's first row), per layer group of srwn_group_plan a boundary buffer
 * [B][hist + max_chunk][R] (hist = the sum of the group's dilations), a carry [B] fp32 (the sample before the chunk) and
 * the ring [B][ring_rows][S] fp32 of hop sums, H_j in row j mod ring_rows; all zero at the stream's start.  A chunk is
 * n = k * hop rows, 1 <= n <= max_chunk.  R in {32, 64}, dtype SRWN_BF16 or SRWN_F32; no RightShift, no conditioning.
 *
 *   srwn_recog_stream_in    model.py:40 for rows [out_hist, out_hist + n) of the first boundary buffer: h0[t] = w0 x[t-1]
 *                           + w1 x[t] + b (init_w [2,1,R], init_b [R], fp32) on x [B, x_stride] fp32, x[-1] of the chunk
 *                           from carry[b]; arithmetic and rounding of srwn_causal_conv1d_fwd with shift 0.
 *   srwn_residual_group_fwd_stream_z
 *                           srwn_residual_group_fwd_stream (its arguments, its bits in x_out) that ALSO stores z of
 *                           every layer of the group for the chunk's own rows (never history or halo rows): chunk row t
 *                           of stream b of layer g at z_out + g * z_layer_stride + ((b * max_chunk) + t) * R, with the
 *                           bits srwn_residual_group_fwd gives that row on the whole clip.  z_layer_stride >= B *
 *                           max_chunk * R elements.  cond_next, cond_frames, pool_stride and
 *                           cond_row_stride mean what they mean to srwn_residual_group_fwd_stream (since srwn_version()
 *                           117; before: NULL only): the conditioning bias of the layer above layer g is added to layer
 *                           g's output, on the halo rows the launch recomputes too, from the ring row of each row's frame.
 *                           z is the tanh of a layer's filter conv and is stored for the chunk's own rows only, conditioned
 *                           or not: a row's z depends on the conditioning through the layer's input alone.
 *   srwn_pooled_stream_head model.py:50-54 and the hop sums of a chunk of k hops in one launch, one workgroup per
 *                           (stream, hop): per 32-row tile of the hop, in time order (the last one masked when hop % 32
 *                           != 0), the gate c = z sigmoid(z) rebuilt from the stored z as srwn_pw_linear's SRWN_PRO_GATE
 *                           does, r0 = relu(bs_sum + sum_l Ws_l c_l), r1 = relu(W1 r0 + b1) -- both rounded to dtype
 *                           where the training forward stores them, r0 exchanged through LDS -- and the tile's rows of
 *                           r1 summed neighbours first (rows 2i + 2i+1, then pairs of pairs ...), the tile sums added
 *                           to the hop's fp32 sum in time order.  H_j goes to ring row j mod ring_rows, j = *clock /
 *                           hop + i for hop i of the chunk.  z [nlayers][B][z_clip_rows][R] at z_layer_stride; wskip:
 *                           the packed skip image [S/32][nlayers * R / 16] (natural k order, k = l * R + n) and w1 the
 *                           packed head image [S/32][S/16], as srwn_pw_linear takes them.  S in {128, 256}.
 *   srwn_hop_sum            the parity twin of the head's last step: the same sums, in the same order, from r1
 *                           [B][r1_clip_rows][S] (dtype) that two srwn_pw_linear calls wrote.  S even.
 *   srwn_window_mean        mean[b * k + i][S] = (sum of the nW ring rows that end at hop j = *clock / hop + i, oldest
 *                           first) / window, zeros while j < nW - 1 (no window has filled: VALID).  ring_rows >= nW + k
 *                           - 1, S <= 256.  With logits != NULL also logits[b * k + i][C] = mean @ w2 + b2 (w2 [S, ldw],
 *                           fp32) in srwn_pooled_head's arithmetic; srwn_pooled_head (labels NULL, B * k rows) gives the
 *                           probabilities.
 *   srwn_recog_roll         moves rows [n, n + hist) of every buffer of roll_table (nroll int64 triples {address, rows per
 *                           stream, hist}, a device array) to its front as srwn_flow_stream_out does, sets carry[b] =
 *                           x[b][n - 1] and adds n to *clock.  The last launch of a chunk.
 * Errors: a null pointer (-3), a width that is not built (-4), a chunk or buffer that does not fit (-2), dtype (-1). */
int srwn_recog_stream_in(const float* x, int64_t x_stride, const float* carry, const float* init_w, const float* init_b,
                         void* out, int64_t out_clip_rows, int32_t out_hist, int32_t B, int32_t n, int32_t max_chunk,
                         int32_t R, int32_t dtype, void* stream);
int srwn_residual_group_fwd_stream_z(const void* x_in, int64_t in_clip_rows, void* x_out, int64_t out_clip_rows,
                                     int32_t out_hist, void* z_out, int64_t z_layer_stride, const void* const* wconv,
                                     const void* const* wres, const float* const* bias_f, const float* const* bias_r,
                                     const void* const* cond_next, int32_t cond_frames, int32_t pool_stride,
                                     int32_t cond_row_stride, const int32_t* dilations, int32_t nlayers, int32_t B,
                                     int32_t n, int32_t max_chunk, int32_t R, int32_t K, int32_t dtype,
                                     const int64_t* clock, void* stream);
int srwn_pooled_stream_head(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers, const void* wskip,
                            const float* bs_sum, const void* w1, const float* b1, float* ring, int32_t ring_rows,
                            const int64_t* clock, int32_t B, int32_t k, int32_t hop, int32_t max_chunk, int32_t R,
                            int32_t S, int32_t dtype, void* stream);
int srwn_hop_sum(const void* r1, int64_t r1_clip_rows, float* ring, int32_t ring_rows, const int64_t* clock, int32_t B,
                 int32_t k, int32_t hop, int32_t max_chunk, int32_t S, int32_t dtype, void* stream);
int srwn_window_mean(const float* ring, int32_t ring_rows, float* mean, const int64_t* clock, int32_t B, int32_t k,
                     int32_t hop, int32_t window, int32_t S, const float* w2, const float* b2, float* logits, int32_t C,
                     int32_t ldw, void* stream);
int srwn_recog_roll(const int64_t* roll_table, int32_t nroll, const float* x, int64_t x_stride, float* carry,
                    int64_t* clock, int32_t B, int32_t n, int32_t max_chunk, int32_t R, int32_t dtype, void* stream);

/* ---- classifier pools (since srwn_version() 115; csrc/srwn_recog.hip, csrc/srwn_group.hip): the launches of the streaming
 * classifier above (class WaveNet, createNetwork, model.py:33-62) for `capacity` SLOTS over one set of buffers, every slot a
 * stream at a clock of its own.  The device table slots[capacity] of SrwnSynthSlot replaces the clock, with the meaning it
 * has for the synthesis pools: t is the absolute time of the slot's next row, and the slot owns ran(u) = clamp(t_end - t,
 * 0, n) rows of a chunk of n = k * hop.  For the classifier t and ran are multiples of hop (t >= 0).  The HOST writes the
 * whole table before every step -- t = the samples the slot's stack has consumed, t_end = t + the whole hops the step
 * gives it -- and no launch modifies it: there is no device advance and no arrive counter.  A slot with ran = 0 (free, or
 * no whole hop waiting) has no group segment, no head workgroup that works, no roll; its rows of mean, logits and
 * probabilities are zeros / the softmax of the bias and are discarded by the caller.  A stream has the bits the clock
 * forms give a batch of one: in any slot, whenever it joined, however its audio was cut, whatever k the steps had and
 * whatever the other slots hold.  The segment cut of the group launch and every grid depend on (capacity, k) and the
 * chip alone, so a captured graph serves every step of its k.
 *
 * A join zeroes the history rows of the joined slots: srwn_flow_stream_reset_slots with the classifier's roll table and
 * ncarry = 0 (carry NULL).  The hop-sum ring needs NO reset: srwn_window_mean_slots emits zeros while j < nW - 1, and from
 * then on a window reads the rows j - nW + 1 .. j >= 0 only, every one of which this stream wrote (ring_rows >= nW + k -
 * 1 keeps them apart); what an earlier stream left in the slot's ring is never read.  The audio lives in the pool's audio
 * ring [capacity][ring_len] fp32, sample s of a slot in column s mod ring_len (the layout srwn_audio_ring_put writes);
 * ring_len >= max_chunk + 1, so that sample t - 1 is still there beside a whole chunk: there is no carry array.
 *
 *   srwn_recog_stream_in_slots      srwn_recog_stream_in for rows [out_hist, out_hist + ran(u)) of slot u: row i from the
 *                                   samples slots[u].t + i - 1 and slots[u].t + i of the audio ring (x[-1] = 0 at time
 *                                   0); arithmetic and rounding of the clock form.  Other rows are not touched.
 *   srwn_residual_group_fwd_stream_z_slots
 *                                   srwn_residual_group_fwd_stream_slots (its arguments, its bits in x_out) that also
 *                                   stores z of every layer of the group for the slot's own chunk rows [0, ran(u)), as
 *                                   srwn_residual_group_fwd_stream_z lays them out (slot u in the place of stream b);
 *                                   rows >= ran(u) of x_out and z_out are not touched.  R in {32, 64}, bf16 and fp32.
 *   srwn_pooled_stream_head_slots   srwn_pooled_stream_head with one workgroup per (slot u, hop i < k) that works only
 *                                   when (i + 1) * hop <= ran(u) and otherwise returns without touching the ring.  H_j
 *                                   goes to row j mod ring_rows of slot u's ring, j = slots[u].t / hop + i.  The
 *                                   arithmetic and the order of every sum are the clock form's (one device body).
 *   srwn_hop_sum_slots              the parity twin, as srwn_hop_sum is srwn_pooled_stream_head's.
 *   srwn_window_mean_slots          srwn_window_mean with row u * k + i from slot u's ring at j = slots[u].t / hop + i;
 *                                   the row is zero where j < nW - 1 or (i + 1) * hop > ran(u).  logits as in the clock
 *                                   form; srwn_pooled_head over capacity * k rows gives the probabilities.
 *   srwn_recog_roll_slots           the history roll of every buffer of roll_table by ran(u) rows (rows [ran, ran +
 *                                   hist) to the front), for the slots with ran > 0.  Nothing else: no carry, no clock.
 * Errors: a null pointer (-3), a width that is not built (-4), capacity < 1, a chunk, a buffer or a ring that does not fit
 * (-2; ring_len < max_chunk + 1 among them), dtype (-1). */
int srwn_recog_stream_in_slots(const float* audio_ring, int32_t ring_len, const float* init_w, const float* init_b,
                               void* out, int64_t out_clip_rows, int32_t out_hist, int32_t capacity, int32_t n,
                               int32_t max_chunk, int32_t R, int32_t dtype, const SrwnSynthSlot* slots, void* stream);
int srwn_residual_group_fwd_stream_z_slots(const void* x_in, int64_t in_clip_rows, void* x_out, int64_t out_clip_rows,
                                           int32_t out_hist, void* z_out, int64_t z_layer_stride,
                                           const void* const* wconv, const void* const* wres,
                                           const float* const* bias_f, const float* const* bias_r,
                                           const void* const* cond_next, int32_t cond_frames, int32_t pool_stride,
                                           int32_t cond_row_stride, const int32_t* dilations, int32_t nlayers,
                                           int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t K,
                                           int32_t dtype, const SrwnSynthSlot* slots, void* stream);
int srwn_pooled_stream_head_slots(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                                  const void* wskip, const float* bs_sum, const void* w1, const float* b1, float* ring,
                                  int32_t ring_rows, const SrwnSynthSlot* slots, int32_t capacity, int32_t k, int32_t hop,
                                  int32_t max_chunk, int32_t R, int32_t S, int32_t dtype, void* stream);
int srwn_hop_sum_slots(const void* r1, int64_t r1_clip_rows, float* ring, int32_t ring_rows, const SrwnSynthSlot* slots,
                       int32_t capacity, int32_t k, int32_t hop, int32_t max_chunk, int32_t S, int32_t dtype,
                       void* stream);
int srwn_window_mean_slots(const float* ring, int32_t ring_rows, float* mean, const SrwnSynthSlot* slots, int32_t capacity,
                           int32_t k, int32_t hop, int32_t window, int32_t S, const float* w2, const float* b2,
                           float* logits, int32_t C, int32_t ldw, void* stream);
int srwn_recog_roll_slots(const int64_t* roll_table, int32_t nroll, const SrwnSynthSlot* slots, int32_t capacity, int32_t n,
                          int32_t max_chunk, int32_t R, int32_t dtype, void* stream);

/* ---- streaming likelihood scorer (since srwn_version() 116; csrc/srwn_score.hip): the softmax teacher (class
 * WaveNetTeacher: createDecoder's stack, model.py:158-196, without conditioning, and the per-sample softmax over mu-law
 * codes, model.py:100-112) as an inference-only stream that leaves nll[t] = -log p(code[t] | audio[< t]) in nats for every
 * row of a chunk.  The stack runs through the streaming classifier's launches: srwn_recog_stream_in on the audio DELAYED BY
 * ONE SAMPLE (x'[0] = the last sample of the chunk before, 0 at the stream's start, x'[1:n] = chunk[:n-1]: with the K = 2
 * entry conv that is h0[t] = b + w0 a[t-2] + w1 a[t-1], the RightShift of model.py:172 folded into the staging), one
 * srwn_residual_group_fwd_stream_z per layer group, and srwn_recog_roll.  A chunk is any 1 <= n <= max_chunk rows; a row's
 * value depends on its own z rows only, so a stream has the same bits however its audio was cut, at any batch size and in
 * any row of the batch.  R in {32, 64}, S in {128, 256}, 1 <= C <= 256 classes, dtype SRWN_BF16 or SRWN_F32.
 *
 *   srwn_stream_score_head  model.py:50-56, the log-softmax and the gather of the target's column in one launch, one
 *                           workgroup per (stream, 32-row tile of the chunk; the last one masked when n % 32 != 0): the gate
 *                           c = z sigmoid(z) rebuilt from the stored z as srwn_pw_linear's SRWN_PRO_GATE does, r0 =
 *                           relu(bs_sum + sum_l Ws_l c_l), r1 = relu(W1 r0 + b1) -- both rounded to dtype where the
 *                           training forward stores them and exchanged through LDS -- logits = W2 r1 + b2 in fp32 (all
 *                           three products start at the bias and take their k-steps in order, as srwn_pw_linear does),
 *                           then per row, over the columns [0, C) ONLY (the padding of the last 32-column tile never enters
 *                           the max or the sum): m = max, nll = log(sum_c exp(l_c - m)) + m - l[code], 8 lanes per row,
 *                           lane j on the columns j, j + 8, ... in rising order, the lanes' values joined by an xor
 *                           butterfly.  z [nlayers][B][z_clip_rows][R] at z_layer_stride, chunk row t of stream b at row b *
 *                           z_clip_rows + t (what srwn_residual_group_fwd_stream_z stores); wskip: the packed skip image
 *                           [S/32][nlayers * R / 16] (natural k order, k = l * R + n), w1 the packed head image
 *                           [S/32][S/16] and w2 the packed image [Cp/32][S/16] of the last 1x1, Cp = 32 * ceil(C / 32), its
 *                           rows behind C zero, as srwn_pw_linear takes them; b2 [Cp] fp32, zero behind C.  codes
 *                           [B][out_stride] int32 in [0, C) (a value outside is clamped into it).  Outputs, row t of
 *                           stream b at b * out_stride + t: nll fp32; best (NULL: not wanted) int32, the argmax column,
 *                           the lowest one on ties; logits_out (NULL: not wanted) fp32 [B][out_stride][C].  Rows [n,
 *                           out_stride) of a stream are not touched.  Dynamic LDS: 32 x (S + 16 / sizeof(dtype)) elements
 *                           of dtype and 32 x 260 fp32 (66 560 bytes for S = 256 in fp32).
 *   srwn_nll_rows           the parity twin of the head's last step: the same reduction, by the same device routine on the
 *                           same lane-to-column map, of logits [B][logits_clip_rows][logits_ld] fp32 (logits_ld >= C) that
 *                           three srwn_pw_linear calls wrote (SRWN_PRO_GATE + SRWN_EPI_RELU over the stored z, SRWN_EPI_RELU,
 *                           SRWN_EPI_F32): nll, best and logits_out have the bits of srwn_stream_score_head.
 * Errors: a null pointer (-3; best and logits_out may be NULL), a width that is not built (-4), C outside [1, 256], B < 1, n
 * < 1 or a chunk or buffer that does not fit (-2), dtype (-1); all before any launch. */
int srwn_stream_score_head(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers, const void* wskip,
                           const float* bs_sum, const void* w1, const float* b1, const void* w2, const float* b2,
                           const int32_t* codes, float* nll, int32_t* best, float* logits_out, int64_t out_stride,
                           int32_t B, int32_t n, int32_t max_chunk, int32_t R, int32_t S, int32_t C, int32_t dtype,
                           void* stream);
int srwn_nll_rows(const float* logits, int64_t logits_ld, int64_t logits_clip_rows, const int32_t* codes, float* nll,
                  int32_t* best, float* logits_out, int64_t out_stride, int32_t B, int32_t n, int32_t C, void* stream);

/* ---- streaming likelihood scorer of the mixture-of-logistics decoder (since srwn_version() 117; csrc/srwn_score.hip): the
 * conditioned decoder of class WaveNetAutoEncoder and the mixture-of-logistics WaveNetTeacher (createDecoder, model.py:
 * 158-196, trained on discretized_mix_logistic_loss, ops.py:124-175) as an inference-only stream that leaves nll[t] = -log
 * p(audio[t] | audio[< t], encoding) in nats for every row of a chunk.  The stack runs through srwn_flow_stream_in on the
 * chunk's own audio (RightShift, the K = 2 entry conv and the first layer's conditioning bias at the device clock; its carry
 * [B][2] = the two samples before the chunk, staged by the caller), one srwn_residual_group_fwd_stream_z per layer group with
 * cond_next set, and srwn_recog_roll.  The conditioning table is a ring [B * cond_frames][nlayers * R] (dtype), frame q of
 * stream b in row b * cond_frames + q mod cond_frames, fed by srwn_pw_linear and srwn_cond_ring_scatter; the group launches
 * recompute their halo rows with their conditioning, so the room rule is the live synthesizer's (110 above): after `fed`
 * frames a stream at time t has room for max(0, cond_frames - fed + max(t - hist_max, 0) / pool_stride) more, hist_max the
 * largest history of the plan's groups.  1 <= M <= 16 mixtures: the 4M logits are Cp = 32 or 64 columns.
 *
 *   srwn_stream_mol_score_head  srwn_stream_score_head through the logits (one device body serves both kernels: the same
 *                           workgroups, fragment maps, k order and barriers), logits = W2 r1 + b2 in fp32 in LDS, then per
 *                           row the mixture-of-logistics negative log-likelihood of the TARGET sample x[b][t] (x [B][x_stride]
 *                           fp32, the chunk's own audio, not delayed) in srwn_mol_nll_rows' per-mixture arithmetic (the
 *                           branches on x < -0.999 / x > 0.999 / cdf_delta > 1e-5, max(log_scale, -7), the half bin 1/255,
 *                           log 127.5): 8 lanes per row, lane j on the mixtures j and j + 8 below M, the log-softmax of the
 *                           mixture logits and the final log-sum-exp joined by an xor butterfly.  Columns [3M, Cp) are never
 *                           read by the reduction.  w2: the packed image [Cp/32][S/16] of the last 1x1, rows behind 4M zero;
 *                           b2 [Cp] fp32.  Outputs, row t of stream b at b * out_stride + t: nll fp32; logits_out (NULL: not
 *                           wanted) fp32 [B][out_stride][4M].  Rows [n, out_stride) of a stream are not touched.  Dynamic
 *                           LDS: 32 x (S + 16 / sizeof(dtype)) elements of dtype and 32 x 68 fp32.
 *   srwn_mol_score_rows     the parity twin of the head's last step: the same reduction, by the same device routine on the
 *                           same lane-to-mixture map, of logits [B][logits_clip_rows][logits_ld] fp32 (logits_ld >= 4M) that
 *                           three srwn_pw_linear calls wrote (the last with SRWN_EPI_F32): nll and logits_out have the bits
 *                           of srwn_stream_mol_score_head.
 * Errors: a null pointer (-3; logits_out may be NULL), a width that is not built (-4), M outside [1, 16], B < 1, n < 1 or a
 * chunk or buffer that does not fit (-2), dtype (-1); all before any launch. */
int srwn_stream_mol_score_head(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                               const void* wskip, const float* bs_sum, const void* w1, const float* b1, const void* w2,
                               const float* b2, const float* x, int64_t x_stride, float* nll, float* logits_out,
                               int64_t out_stride, int32_t B, int32_t n, int32_t max_chunk, int32_t R, int32_t S, int32_t M,
                               int32_t dtype, void* stream);
int srwn_mol_score_rows(const float* logits, int64_t logits_ld, int64_t logits_clip_rows, const float* x, int64_t x_stride,
                        float* nll, float* logits_out, int64_t out_stride, int32_t B, int32_t n, int32_t M, void* stream);

/* ---- scorer pools (since srwn_version() 118; csrc/srwn_score.hip): the launches of the softmax streaming scorer above
 * (116) for `capacity` SLOTS over one set of buffers, every slot a stream at a clock of its own.  The device table
 * slots[capacity] of SrwnSynthSlot replaces the clock, with the meaning it has for the classifier pools (115): t is the
 * absolute time of the slot's next sample (t >= 0), and the slot owns ran(u) = clamp(t_end - t, 0, n) rows of a chunk of n
 * -- here ANY number of rows, not a multiple of anything.  The HOST writes the whole table before every step (t = the
 * samples the slot has scored, t_end = t + the samples the step gives it) and no launch modifies it.  A slot with ran = 0
 * touches nothing.  A step is the entry below, one srwn_residual_group_fwd_stream_z_slots per layer group, the head below
 * (or the twin: three srwn_pw_linear products over (capacity - 1) * max_chunk + n rows, in which stale rows ride along
 * and are never read, then srwn_nll_rows_slots) and srwn_recog_roll_slots; a join zeroes the history rows of the joined
 * slots with srwn_flow_stream_reset_slots (ncarry = 0).  A stream has the bits the clock forms give a batch of one: in any
 * slot, whenever it joined, however its audio was cut, whatever n the steps had and whatever the other slots hold.  Every
 * grid depends on (capacity, n) alone, so a captured graph serves every step of its n.
 *
 *   srwn_score_stream_in_slots    the pool's entry, one launch over the pool's audio ring [capacity][ring_len] fp32 (sample
 *                                 s of a slot in column s mod ring_len, the layout srwn_audio_ring_put writes).  For row i <
 *                                 ran(u) of slot u, s = slots[u].t + i: (a) row out_hist + i of the first boundary buffer
 *                                 `out` [capacity][out_clip_rows][R] = b + w0 a[s-2] + w1 a[s-1] in srwn_recog_stream_in's
 *                                 arithmetic and rounding on the delayed audio (the teacher's RightShift folded into the
 *                                 read: no staged delayed copy, no carry; samples before time 0 read as 0), and (b)
 *                                 codes[u * codes_stride + i] = the mu-law code of a[s] over C classes, the bits of
 *                                 srwn_mu_law_encode (one device routine serves both).  ring_len >= max_chunk + 2, so that
 *                                 a[t-2] is still there beside a whole chunk; codes_stride >= max_chunk.  2 <= C <= 256.
 *                                 Other rows of out and codes are not touched.
 *   srwn_stream_score_head_slots  srwn_stream_score_head with one workgroup per (slot u, 32-row tile i < ceil(n / 32)) that
 *                                 returns before its first barrier when 32 * i >= ran(u) and otherwise runs the clock form's
 *                                 body (one device body, the SLOTS instantiation of the same kernel template) with ran(u)
 *                                 in the place of n: a masked last tile re-reads the slot's last own row and stores
 *                                 nothing.  Rows >= ran(u) of nll, best and logits_out are not touched.
 *   srwn_nll_rows_slots           the parity twin's last step on the fp32 logits, as srwn_nll_rows is
 *                                 srwn_stream_score_head's: the same grid and the same early return.
 * Errors, all before any launch: empty work (capacity * n == 0) is done (0); a null pointer (-3; best and logits_out may be
 * NULL); a width or a class count that is not built (-4); capacity < 0, n < 0 or a chunk, a buffer or a ring that does
 * not fit (-2; ring_len < max_chunk + 2 among them); dtype (-1). */
int srwn_score_stream_in_slots(const float* audio_ring, int32_t ring_len, const float* init_w, const float* init_b, void* out,
                               int64_t out_clip_rows, int32_t out_hist, int32_t* codes, int64_t codes_stride,
                               int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t C, int32_t dtype,
                               const SrwnSynthSlot* slots, void* stream);
int srwn_stream_score_head_slots(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                                 const void* wskip, const float* bs_sum, const void* w1, const float* b1, const void* w2,
                                 const float* b2, const int32_t* codes, float* nll, int32_t* best, float* logits_out,
                                 int64_t out_stride, int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t S,
                                 int32_t C, int32_t dtype, const SrwnSynthSlot* slots, void* stream);
int srwn_nll_rows_slots(const float* logits, int64_t logits_ld, int64_t logits_clip_rows, const int32_t* codes, float* nll,
                        int32_t* best, float* logits_out, int64_t out_stride, int32_t capacity, int32_t n, int32_t C,
                        const SrwnSynthSlot* slots, void* stream);

/* ---- mixture-of-logistics scorer pools (since srwn_version() 119; csrc/srwn_score.hip): the launches of the streaming
 * likelihood scorer of the mixture-of-logistics decoder above (117) for `capacity` SLOTS over one set of buffers, every slot
 * a stream at a clock of its own AND with a conditioning ring of its own.  The device table slots[capacity] of SrwnSynthSlot
 * replaces the clock with the meaning it has for the scorer pools (118): t is the absolute time of the slot's next sample
 * (t >= 0), and the slot owns ran(u) = clamp(t_end - t, 0, n) rows of a chunk of n, any number.  The HOST writes the whole
 * table before every step (t = the samples the slot has scored, t_end = t + the samples the step gives it: at most what it
 * has received, and for a conditioned decoder at most fed(u) * pool_stride) and no launch modifies it.  A slot with ran = 0
 * touches nothing.  A step is the entry below, one srwn_residual_group_fwd_stream_z_slots per layer group with cond_next
 * set, the head below (or the twin: three srwn_pw_linear products over (capacity - 1) * max_chunk + n rows, in which stale
 * rows ride along and are never read, then srwn_mol_score_rows_slots) and srwn_recog_roll_slots; a join zeroes the history
 * rows of the joined slots with srwn_flow_stream_reset_slots (ncarry = 0).  The conditioning table is the ring of 117,
 * [capacity * cond_frames][nlayers * R]: frame q of slot u in row u * cond_frames + q mod cond_frames, fed by srwn_pw_linear
 * and srwn_cond_ring_scatter_slots (ragged: any number of frames per slot in one launch) under the room rule of 117 with the
 * slot's own fed and t.  A join need not clear a slot's ring rows: a stream reads only frames it was fed.  A stream has
 * the bits the clock forms give a batch of one: in any slot, whenever it joined, however its audio and its frames were cut,
 * whatever n the steps had and whatever the other slots hold.  Every grid depends on (capacity, n) alone, so a captured
 * graph serves every step of its n.
 *
 *   srwn_mol_score_stream_in_slots    the pool's entry, one launch over the pool's audio ring [capacity][ring_len] fp32
 *                                     (sample s of a slot in column s mod ring_len, the layout srwn_audio_ring_put writes).
 *                                     For row i < ran(u) of slot u, s = slots[u].t + i: (a) row out_hist + i of the first
 *                                     boundary buffer `out` [capacity][out_clip_rows][R] = round(b + w0 a[s-2] + w1 a[s-1])
 *                                     + cond0 row u * cond_frames + (s / pool_stride) mod cond_frames, rounded again: the
 *                                     RightShift, the K = 2 entry conv and the first layer's conditioning bias with the bits
 *                                     srwn_flow_stream_in_slots gives the same row for the same chunk in x, the two samples
 *                                     before it in carry and the same table (one device routine serves both; samples before
 *                                     time 0 read as 0; no carry buffer, no staged copy of the chunk), and (b) x_out[u *
 *                                     x_stride + i] = a[s], the row's target, not delayed, for the head below.  ring_len >=
 *                                     max_chunk + 2, so that a[s-2] is still there beside a whole chunk; x_stride >=
 *                                     max_chunk; cond0, cond_frames, pool_stride and cond_row_stride as srwn_flow_stream_in
 *                                     takes them (an unconditioned decoder passes its one zero row per slot with cond_frames
 *                                     = 1).  Other rows of out and x_out are not touched.
 *   srwn_stream_mol_score_head_slots  srwn_stream_mol_score_head with one workgroup per (slot u, 32-row tile i < ceil(n /
 *                                     32)) that returns before its first barrier when 32 * i >= ran(u) and otherwise runs the
 *                                     clock form's body (the SLOTS instantiation of the same kernel template) with ran(u) in
 *                                     the place of n: a masked last tile re-reads the slot's last own row and stores
 *                                     nothing.  Rows >= ran(u) of nll and logits_out are not touched.
 *   srwn_mol_score_rows_slots         the parity twin's last step on the fp32 logits, as srwn_mol_score_rows is
 *                                     srwn_stream_mol_score_head's: the same grid and the same early return.
 * Errors, all before any launch: empty work (capacity * n == 0) is done (0); a null pointer (-3; logits_out may be NULL); a
 * width that is not built (-4); M outside [1, 16], capacity < 0, n < 0 or a chunk, a buffer or a ring that does not fit
 * (-2; ring_len < max_chunk + 2 among them); dtype (-1). */
int srwn_mol_score_stream_in_slots(const float* audio_ring, int32_t ring_len, const float* init_w, const float* init_b,
                                   const void* cond0, int32_t cond_frames, int32_t pool_stride, int64_t cond_row_stride,
                                   void* out, int64_t out_clip_rows, int32_t out_hist, float* x_out, int64_t x_stride,
                                   int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t dtype,
                                   const SrwnSynthSlot* slots, void* stream);
int srwn_stream_mol_score_head_slots(const void* z, int64_t z_layer_stride, int64_t z_clip_rows, int32_t nlayers,
                                     const void* wskip, const float* bs_sum, const void* w1, const float* b1, const void* w2,
                                     const float* b2, const float* x, int64_t x_stride, float* nll, float* logits_out,
                                     int64_t out_stride, int32_t capacity, int32_t n, int32_t max_chunk, int32_t R, int32_t S,
                                     int32_t M, int32_t dtype, const SrwnSynthSlot* slots, void* stream);
int srwn_mol_score_rows_slots(const float* logits, int64_t logits_ld, int64_t logits_clip_rows, const float* x,
                              int64_t x_stride, float* nll, float* logits_out, int64_t out_stride, int32_t capacity, int32_t n,
                              int32_t M, const SrwnSynthSlot* slots, void* stream);

/* ---- streaming embedder (since srwn_version() 120; csrc/srwn_embed.hip): a tower of class SiameseWaveNet (model.py:660-797:
 * class WaveNet's network up to the last 1x1 and the average pool, model.py:689-731) as an inference-only stream that
 * scores every window position against an enrolled gallery with the reference's distance (model.py:736).  Everything up
 * to the hop sums is the streaming classifier's (113): srwn_recog_stream_in, srwn_residual_group_fwd_stream_z per layer
 * group, srwn_pooled_stream_head (or its twin) into the ring [B][ring_rows][S] of hop sums, and srwn_recog_roll last.  The
 * gallery is gallery [max_gallery][D] fp32 with its row count in DEVICE memory (n_gallery, one int32, clamped to [0,
 * max_gallery]): every workgroup reads it when it runs, so a captured graph keeps serving after rows were enrolled.
 *
 *   srwn_window_embed_match   one launch, one workgroup of 256 threads per row = (stream b, hop i < k of the step), row index
 *                             b * k + i, j = *clock / hop + i:
 *                             (a) mean [S] = (sum of the nW = window / hop ring rows that end at hop j, oldest first) / window,
 *                                 zeros while j < nW - 1 (such a row reads no ring row) -- srwn_window_mean's mean;
 *                             (b) emb[row][d] = b2[d] + sum_s mean[s] w2[s][d], d < D (w2 [S, ldw] fp32, one fmaf per s in
 *                                 order): bit for bit what srwn_window_mean writes to `logits` with C = D for the same ring;
 *                             (c) dist[row][n] = sqrt(1e-8 + sum_d (emb[row][d] - gallery[n][d])^2) for n < N = *n_gallery
 *                                 (dist [rows][max_gallery]; columns n >= N are not written).  Wave w of the workgroup takes the
 *                                 rows n = w, w + 4, ...; lane l adds the squares of d = l, l + 64, ... in order and a 64-lane
 *                                 xor butterfly adds the lanes, as srwn_contrastive_head scores a pair: a distance's bits
 *                                 depend on the two vectors and D alone, not on k, B, the row or N;
 *                             (d) nearest[row] = the argmin over n < N, the lowest index on ties, dmin[row] its distance;
 *                                 N = 0: nearest = -1, dmin = +inf.
 *                             The mean and the embedding stay in LDS.  ring_rows >= nW + k - 1.
 *   srwn_window_embed_match_slots
 *                             the same on a pool's table (115) in the clock's place: row u * k + i from slot u's ring at
 *                             j = slots[u].t / hop + i; the mean is zero too (and no ring row is read) where (i + 1) * hop >
 *                             ran(u) -- rows the caller discards.  One device body with the clock form.
 *   srwn_gallery_match        steps (c) and (d) alone on emb [rows][D] (the device routine of the fused kernel): the last step
 *                             of the parity twin behind srwn_window_mean(_slots) with logits, and a scorer of stored
 *                             embeddings.  rows = 0 is done (0).
 * Limits: S <= 256, 1 <= D <= 256, ldw >= D, 1 <= max_gallery <= 1024.  Errors, all before any launch, as srwn_window_mean
 * reports them: a null pointer (-3); a size that does not fit (-2: S or D outside [1, 256], ldw < D, max_gallery outside
 * [1, 1024], B, k or hop < 1, window not a multiple of hop, a ring of fewer than nW + k - 1 rows, rows < 0).  The kernels
 * are not built per width or dtype (everything here is fp32), so -4 and -1 do not occur. */
int srwn_window_embed_match(const float* ring, int32_t ring_rows, const int64_t* clock, int32_t B, int32_t k, int32_t hop,
                            int32_t window, int32_t S, const float* w2, const float* b2, int32_t D, int32_t ldw,
                            const float* gallery, const int32_t* n_gallery, int32_t max_gallery, float* emb, float* dist,
                            int32_t* nearest, float* dmin, void* stream);
int srwn_window_embed_match_slots(const float* ring, int32_t ring_rows, const SrwnSynthSlot* slots, int32_t capacity,
                                  int32_t k, int32_t hop, int32_t window, int32_t S, const float* w2, const float* b2,
                                  int32_t D, int32_t ldw, const float* gallery, const int32_t* n_gallery, int32_t max_gallery,
                                  float* emb, float* dist, int32_t* nearest, float* dmin, void* stream);
int srwn_gallery_match(const float* emb, int32_t rows, int32_t D, const float* gallery, const int32_t* n_gallery,
                       int32_t max_gallery, float* dist, int32_t* nearest, float* dmin, void* stream);

/* ---- student flow inversion (since srwn_version() 121; csrc/srwn_flow_inv.hip): one inverse-autoregressive flow of class
 * ParallelWaveNet (createFlow, model.py:456-487) run backwards, audio -> noise.  The flow computes
 *   x_out[t] = x_in[t] * exp(p0[t]) + p1[t],   (p0, p1)[t] = flow_b + relu(stack(RightShift(x_in), encoding)[t]) . flow_w,
 * where the stack reads x_in[< t] only, so given x_out = y the input is recovered one step at a time:
 *   h0[t]   = init_b + init_w[0] * x_in[t-2] + init_w[1] * x_in[t-1]   from the RECOVERED samples (zeros before the clip),
 *             rounded to the activation type, then layer 0's conditioning bias is added (srwn_flow_stream_in's rounding);
 *   layers  the L conditioned layers of the reference gate over rings of the last d_l + 1 layer inputs, with the
 *           arithmetic, the ring writes, the zero tap before the clip starts and the conditioning frame
 *           min(t / pool_stride, cond_frames - 1) of the conditioned generator (srwn_generate_mol); no skip path;
 *   head    (p0, p1) = flow_b + relu(x_L[t] rounded to the activation type) . flow_w in fp32 (srwn_flow_affine_fwd);
 *   inverse x_in[t] = (y[t] - p1) * expf(-p0).
 * One launch inverts ONE flow over the steps [t0, t0 + nsteps) of B streams; a student of F flows is F dependent launches,
 * the last flow first, each reading the x_in the launch before wrote.  sum_f p0_f[t] is log |d audio / d noise| at t.
 *   wcr     per layer [srwn conv image, last tap permuted | residual image] (the generators' layer images, without skip)
 *   flow_w  [R][2] fp32, flow_b [2] fp32 (srwn_flow_affine_fwd's w2 / b2); bias_f, bias_r [L][R]; init_w [2][R]; init_b [R]
 *   ring    srwn_generate_ring_elems(dilations, nlayers, R) elements per group of 32 streams, zero at t0 = 0
 *   y, x_in [B][Tout] fp32, prm [B][Tout][2] fp32 or NULL: rows j < nsteps <= Tout are the launch's own (as in
 *           srwn_generate_resume); y and x_in may not overlap
 *   cond    the conditioning biases: cb_l of stream u and frame f at element l * cond_layer_stride +
 *           (u * cond_frames + f) * cond_ld, R values of the activation type (cond_ld >= R)
 *   carry   float [B][2] = (x_in[t0-1], x_in[t0-2]) in, (x_in[t0+n-1], x_in[t0+n-2]) out; NULL = zeros in, nothing
 *           written (only with t0 = 0).  Any cut of a run into launches gives the bits of one launch.
 * Errors, all before any launch: B = 0 or nsteps = 0 is done (0); B, nsteps or t0 < 0, nsteps > Tout, nlayers outside
 * [1, 64], a dilation < 1, cond_frames or pool_stride < 1, cond_ld < R, cond_frames * pool_stride < t0 + nsteps, or layer
 * constants that do not fit the LDS of a workgroup (-2); a null pointer other than prm, or a NULL carry with t0 > 0 (-3);
 * R not 32 or 64, K not 2 (-4); a dtype other than SRWN_BF16 / SRWN_F32 (-1). */
int srwn_flow_invert(const void* wcr, const float* bias_f, const float* bias_r, const float* init_w, const float* init_b,
                     const float* flow_w, const float* flow_b, void* ring, const float* y, float* x_in, float* prm,
                     const int32_t* dilations, int32_t nlayers, int32_t B, int32_t Tout, int32_t nsteps, int32_t R, int32_t K,
                     const void* cond, int32_t cond_frames, int32_t pool_stride, int64_t cond_ld,
                     int64_t cond_layer_stride, int32_t dtype, void* stream, int32_t t0, float* carry);

/* ---- device-resident datasets (since srwn_version() 122; csrc/srwn_data.hip): the two launches that a BatchSampler
 * (sr-wavenet_amd/dataset.py) puts around the training step, inside its hipGraph.  The clips stay on the device; a replay
 * needs no upload and no host wait.
 *   state   int64 [2] = {seed, step} in device memory.  srwn_batch_draw only reads it; srwn_step_log ticks `step`, as
 *           srwn_adam_step ticks its own counter.
 * srwn_batch_draw draws the B records of the step and writes what the engines' set_inputs writes from a host batch.  Row b
 * is position p = (step * world + rank) * B + b of the sample sequence: epoch e = p / num_clips, place i = p % num_clips,
 * record perm(seed, e)(i) (shuffle != 0: a keyed bijection on [0, num_clips) -- four alternating Feistel rounds on the next
 * power of two, keyed by the splitmix64 finaliser of the samplers' uniforms, cycle-walked back into range) or i; crop 0 takes
 * samples [0, T) of the clip (tf.slice, nsynth.py:31), crop 1 an offset uniform on [0, clip_len - T] drawn from (seed, p).
 * dataset.draw_plan states the same function in Python.
 *   clips    [num_clips][clip_len] fp32;  labels [num_clips] int32, or NULL without one-hot rows
 *   audio0   [B][T] fp32: the cropped rows;  audio1 the same rows once more, or NULL (the auto-encoder's second buffer)
 *   codes    [B][T] int32 or NULL: the rows' mu-law codes at quantization_channels, with the bits of srwn_mu_law_encode
 *   onehot   NULL, or a matrix of onehot_dtype (SRWN_F32 / SRWN_BF16) with onehot_ld elements per row: rows
 *            [b * onehot_rows, (b + 1) * onehot_rows) get, in columns [onehot_col0, onehot_col0 + num_classes), the one-hot
 *            row of record b's label -- all zeros for a label outside [0, num_classes), as tf.one_hot; other columns are
 *            not touched.  (The classifier: onehot_rows 1, column 0, fp32 [B][C]; the auto-encoder: the frames of a clip,
 *            behind the latent columns of the decoder's conditioning input.)
 *   indices  [B] int32: the records drawn
 * Errors, all before any launch: B = 0 or T = 0 is done (0); a null clips, state, audio0 or indices, or one-hot rows without
 * labels (-3); num_clips or clip_len < 1, T > clip_len, B > 65535, rank outside [0, world), a crop other than 0 / 1,
 * quantization_channels < 2 with codes, one-hot columns that do not fit onehot_ld, a buffer that is not 4-byte aligned (-2);
 * a one-hot dtype other than SRWN_F32 / SRWN_BF16 (-1).
 * srwn_step_log is the step's last launch: log[step % capacity] = loss[0], then step += 1 (one thread).  The tick is here
 * because every workgroup of srwn_batch_draw reads `step`.  Errors: a null pointer (-3), capacity < 1 (-2). */
int srwn_batch_draw(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len, const int64_t* state,
                    int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank, int32_t world, float* audio0,
                    float* audio1, int32_t* codes, int32_t quantization_channels, void* onehot, int64_t onehot_ld,
                    int32_t onehot_rows, int32_t onehot_col0, int32_t num_classes, int32_t onehot_dtype, int32_t* indices,
                    void* stream);
int srwn_step_log(const float* loss, float* log, int32_t capacity, int64_t* state, void* stream);

/* ---- device-resident training for the student and the twin towers (since srwn_version() 123; csrc/srwn_draw.hip): the
 * launches a DistillSampler and a PairSampler (sr-wavenet_amd/dataset.py) put around a training step, inside its hipGraph.
 * The rules of the block above hold: `state` is int64 [2] = {seed, step} in device memory, the draws only read it and the
 * log launches tick `step`; rows are positions p = (step * world + rank) * B + b of the sample sequence, their records and
 * crop offsets are srwn_batch_draw's (dataset.draw_plan); every argument is checked before any launch.
 * srwn_distill_draw is the student step's first launch.
 *   audio0   [B][T] fp32: the cropped rows;  audio1, audio2 the same rows again, or NULL (the teacher encoder's input,
 *            StudentEngine.truth and the teacher decoder's audio)
 *   noise    [B][T] fp32 or NULL: temperature * (log u - log(1 - u)), u = (k + 1/2) / 2^23, with the 23-bit values k of
 *            dataset.noise_plan: row b has the seed s_b = mix64((seed ^ NOISE_SALT) + GOLDEN * (p + 1)) and entry j the
 *            bits mix64(s_b + GOLDEN * (j + 1)) >> 41 -- what srwn_logistic_noise draws for seed[b] = s_b at clock 0, by
 *            that kernel's evaluation and its rule for temperature 0
 *   cond_tables  a DEVICE array of num_tables (0..64) addresses of matrices of cond_dtype (SRWN_F32 / SRWN_BF16) with
 *            cond_ld elements per row (the teacher decoder's cond_in and every flow's): in each, rows [b * cond_rows,
 *            (b + 1) * cond_rows) get, in columns [cond_col0, cond_col0 + num_classes), the one-hot row of record b's label
 *            by srwn_batch_draw's tf.one_hot rule; other columns are not touched.  num_tables 0: no one-hot rows.
 *   indices  [B] int32: the records drawn
 * Errors: B = 0 or T = 0 is done (0); a null clips, state, audio0 or indices, or one-hot rows without labels or tables
 * (-3); num_clips or clip_len < 1, T > clip_len, B > 65535, rank outside [0, world), a crop other than 0 / 1, num_tables
 * outside [0, 64], one-hot columns that do not fit cond_ld, a buffer that is not 4-byte aligned (-2); a one-hot dtype other
 * than SRWN_F32 / SRWN_BF16 (-1).
 * srwn_cond_scatter writes enc [rows][latent] fp32 (EncoderStack.forward's encoding) into columns [0, latent) of the same
 * num_tables matrices, converted to cond_dtype (bf16: round to nearest even) -- the bits of cond_in[:, :latent].copy_(enc);
 * columns >= latent are not touched.  One launch.  Errors: nothing to do is done (0); a null pointer (-3); negative sizes,
 * cond_ld < latent, num_tables > 64 (-2); the dtype (-1).
 * srwn_distill_log is the student step's last launch (one thread): in double and in this order, every operation rounded
 * once, entropy = logs[0] + 2 n and loss = (beta * ce[0] - alpha * entropy + power[0]) / loss_div -- the arithmetic of
 * StudentEngine.losses() -- then loss_log[s] = (float)loss, power_log[s] = power[0], entropy_log[s] = (float)entropy at
 * s = step % capacity, then step += 1.  Errors: a null pointer (-3); capacity < 1, n < 0, loss_div 0 or NaN (-2).
 * srwn_pair_draw is the twins' first launch (dataset.pair_plan).  The left clip of pair b is the draw's record and offset
 * of position p.  With c its label, m the records of class c, q its place inside the class block of `order`: the coin
 * same = (h1 >> 32) < same_threshold (= floor(p_same * 2^32)), overridden where only one outcome exists (m = 1: different;
 * num_clips = m: same; num_clips = 1: the record itself); same: k = ((h2 >> 32) (m - 1)) >> 32, k += (k >= q), right =
 * order[class_start[c] + k]; different: k = ((h2 >> 32) (num_clips - m)) >> 32, right = order[k < class_start[c] ? k : k +
 * m]; h1, h2 and the right crop offset's h3 = mix64((seed ^ salt) + GOLDEN * (p + 1)) with the three PAIR salts.
 *   order [num_clips] int32: the stable argsort of the labels;  place [num_clips]: its inverse;  class_start
 *   [num_classes + 1]: where each class begins in `order`.  Every label must lie in [0, num_classes).
 *   audio [2P][T] fp32: the left clips in rows [0, P), the right ones in [P, 2P);  y [P] fp32: 1 where the labels agree,
 *   else 0 (model.py:747-749);  left, right [P] int32 and y_log [P] fp32: the draw, for the sampler.
 * Errors: P = 0 or T = 0 is done (0); a null pointer (-3); the draw's shape errors, P > 32767, num_classes < 1,
 * same_threshold outside [0, 2^32] (-2).
 * srwn_pair_log is the twins' last launch (one workgroup): loss_log[s] = loss[0] and dist_log[s][0..P) = dist[0..P) at
 * s = step % capacity, then step += 1.  Errors: a null pointer (-3); capacity or P < 1 (-2). */
int srwn_distill_draw(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len, const int64_t* state,
                      int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank, int32_t world, float* audio0,
                      float* audio1, float* audio2, float* noise, float temperature, const int64_t* cond_tables,
                      int32_t num_tables, int64_t cond_ld, int32_t cond_rows, int32_t cond_col0, int32_t num_classes,
                      int32_t cond_dtype, int32_t* indices, void* stream);
int srwn_cond_scatter(const float* enc, int64_t rows, int32_t latent, const int64_t* cond_tables, int32_t num_tables,
                      int64_t cond_ld, int32_t cond_dtype, void* stream);
int srwn_distill_log(const float* ce, const float* power, const float* logs, double alpha, double beta, int64_t n,
                     double loss_div, float* loss_log, float* power_log, float* entropy_log, int32_t capacity,
                     int64_t* state, void* stream);
int srwn_pair_draw(const float* clips, const int32_t* labels, const int32_t* order, const int32_t* place,
                   const int32_t* class_start, int32_t num_classes, int32_t num_clips, int64_t clip_len, const int64_t* state,
                   int32_t P, int32_t T, int64_t same_threshold, int32_t shuffle, int32_t crop, int32_t rank, int32_t world,
                   float* audio, float* y, int32_t* left, int32_t* right, float* y_log, void* stream);
int srwn_pair_log(const float* loss, const float* dist, int32_t P, float* loss_log, float* dist_log, int32_t capacity,
                  int64_t* state, void* stream);

/* ---- device-resident evaluation (since srwn_version() 124; csrc/srwn_eval.hip): the launch an EvalSampler
 * (sr-wavenet_amd/dataset.py) puts behind the classifier's forward pass when it sweeps a held-out set once, inside the
 * sweep's hipGraph.  The draw in front is srwn_batch_draw with shuffle 0, which only reads the state; this launch ticks it.
 *   state    int64 [3] = {seed, step, sweep} in device memory
 *   probs    [B][C] fp32: the pooled head's posteriors of the step's rows;  indices [B] int32: the draw's records
 *   labels   [num_clips] int32, every one inside [0, C)
 *   pred, rank_out [sweep_capacity][num_clips] int32;  nll [sweep_capacity][num_clips] fp32;
 *   confusion [sweep_capacity][C][C] int32 (label, then prediction);  seen [sweep_capacity] int32: the result slots
 * Row b of the step is position p = (step * world + rank) * B + b and is valid where p < num_clips (its record is p: one
 * sweep of ceil(num_clips / (B * world)) steps visits every record once across the ranks).  For every valid row the launch
 * writes, in slot sweep % sweep_capacity and at the row's record: pred, the first maximum of the row (`>` over rising
 * class index: on equal values the lower index); rank_out, the number of classes that come before the label's class in
 * that order (a greater probability, or an equal one at a lower index), so rank_out = 0 exactly where pred = label;
 * nll = (float)(-log((double)probs[label])), +inf for a probability of 0.  It adds 1 to confusion[label][pred] and to seen
 * with integer atomic adds.  At step 0 it first clears the slot's confusion and seen.  Invalid rows write nothing; records
 * the sweep has not reached keep what they held.  Last it ticks: step += 1, and where step reaches the sweep's steps,
 * step = 0 and sweep += 1.  One workgroup.  dataset.sweep_plan states the order in Python.
 * Errors, all before any launch: a null pointer (-3); C outside [1, 256], B < 1, num_clips < 1, rank outside [0, world),
 * sweep_capacity < 1 (-2). */
int srwn_eval_classes(const float* probs, const int32_t* indices, const int32_t* labels, int64_t* state, int32_t num_clips,
                      int32_t B, int32_t C, int32_t rank, int32_t world, int32_t sweep_capacity, int32_t* pred,
                      int32_t* rank_out, float* nll, int32_t* confusion, int32_t* seen, void* stream);

/* ---- device-resident evaluation of an embedding model (since srwn_version() 125; csrc/srwn_pair_eval.hip): the two launches
 * an EmbedSampler (sr-wavenet_amd/dataset.py) adds to a tower's forward pass when it sweeps a labelled held-out set: one
 * behind every step's forward pass, one behind the sweep's last step over all pairs of records.
 *   state      int64 [3] = {seed, step, sweep} in device memory, ticked as srwn_eval_classes ticks it
 *   slots_emb  [sweep_capacity][num_clips][D] fp32;  seen [sweep_capacity] int32;  labels [num_clips] int32
 *   nearest, same_nearest, rank_same [sweep_capacity][num_clips] int32;  nearest_dist, same_dist the same in fp32
 *   hist_same, hist_diff [sweep_capacity][bins] int64;  dist NULL or [num_clips][num_clips] fp32
 * srwn_embed_collect: row b of the step is position p = (step * world + rank) * B + b, valid where p < num_clips.  The launch
 * copies every valid row of emb [B][D] to record indices[b] of slot sweep % sweep_capacity, adds their number to the slot's
 * seen (from 0 at step 0) and ticks: step += 1, and where step reaches ceil(num_clips / (B * world)), step = 0 and
 * sweep += 1.  Invalid rows write nothing.  One workgroup.
 * srwn_pair_sweep: over the records of slot (sweep - 1) % sweep_capacity, the sweep just completed (nothing before the
 * first).  d(i, j) = sqrtf(1e-8f + ss) with the bits of srwn_contrastive_head and srwn_gallery_match: lane l of a 64-lane
 * wave forms ss_l by fmaf(df, df, ss) over k = l, l + 64, ... from 0, an xor butterfly 32, 16, 8, 4, 2, 1 adds the lanes;
 * dist[i][j] = d(i, j) for every i and j, the diagonal included.  a comes before b iff d_a < d_b, or d_a == d_b and a < b.
 * Per record i over j != i: nearest and nearest_dist are the first j and its distance (-1 and +inf for one record);
 * same_nearest and same_dist the first j with labels[j] == labels[i] (-1 and +inf without one); rank_same the number of j of
 * another label that come before same_nearest, -1 without one.  Over i < j: bin = min(bins - 1, (int)(d * scale)) is counted
 * in hist_same or hist_diff by the labels; a product that is not below bins, NaN included, goes to the last bin.  The entry
 * point clears the slot's two histograms with a one-workgroup launch in front of the row launch (one workgroup per
 * record), which adds its LDS counts to them with 64-bit integer atomic adds: no result depends on an execution order.
 * Errors, all before any launch: a null pointer other than dist (-3); D outside [1, 1024], num_clips outside [1, 4096],
 * B < 1, rank outside [0, world), sweep_capacity < 1, bins outside [1, 4096], a scale that is not finite and above 0 (-2). */
int srwn_embed_collect(const float* emb, const int32_t* indices, int64_t* state, int32_t num_clips, int32_t B, int32_t D,
                       int32_t rank, int32_t world, int32_t sweep_capacity, float* slots_emb, int32_t* seen, void* stream);
int srwn_pair_sweep(const float* slots_emb, const int32_t* labels, const int64_t* state, int32_t num_clips, int32_t D,
                    int32_t sweep_capacity, int32_t bins, float scale, int32_t* nearest, int32_t* same_nearest,
                    int32_t* rank_same, float* nearest_dist, float* same_dist, int64_t* hist_same, int64_t* hist_diff,
                    float* dist, void* stream);

/* ---- training controls (since srwn_version() 126; csrc/srwn_opt.hip): the update of srwn_adam_step / srwn_adam_step_scaled
 * with the learning rate read from a device table, the clip factor from device memory and an exponential moving average of
 * the parameters kept in the same pass.
 *   ctl           float32 [H][2] = {lr, ema_decay} per step, in device memory
 *   ctl_len       int32 [1] in device memory: H.  The launch reads it, so a table and a length rewritten in place steer a
 *                 captured graph without a new capture.  H is held to [1, ctl_capacity]
 *   ctl_capacity  the rows allocated behind ctl (host): no row at or past it is ever read
 *   ema           NULL, or float32 [n]: the shadow
 *   grad_scale_dev NULL, or the clip factor of srwn_clip_scale: g = grads * (grad_scale * grad_scale_dev[0])
 *   tick          as for srwn_adam_step_scaled; t below is the count after the tick (the count itself where tick = 0)
 * Rule, with row = min(t - 1, H - 1) (0 where t = 0):
 *   lr_t = (float)((double)ctl[row][0] * sqrt(1 - b2^t) / (1 - b1^t));
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  params -= lr_t * m / (sqrt(v) + eps)      (the bits of srwn_adam_step at
 *   lr = ctl[row][0])
 *   and where ema is given, tf's assign_moving_average on the parameter just written, as three separately rounded fp32
 *   operations in this order:  s = 1.0f - ctl[row][1];  diff = ema - params;  p = s * diff;  ema = ema - p
 * params, m and v do not depend on whether ema is given.  Errors, before any launch: a null params, grads, m, v, step, ctl
 * or ctl_len (-3); n < 0 or ctl_capacity < 1 (-2).  n == 0 returns 0. */
int srwn_adam_step_ctl(float* params, const float* grads, float* m, float* v, float* ema, int64_t n, int64_t* step,
                       const float* ctl, const int32_t* ctl_len, int32_t ctl_capacity, float beta1, float beta2, float eps,
                       float grad_scale, const float* grad_scale_dev, int32_t tick, void* stream);

/* ---- augmented draws (since srwn_version() 127; csrc/srwn_augment.hip): srwn_batch_draw and srwn_pair_draw with a random
 * time shift, a random gain and a background recording mixed in at a random volume, in the same one launch.  Everything the
 * plain entries say holds -- the state is only read, the records and crop offsets are dataset.draw_plan's and
 * dataset.pair_plan's, the outputs are the same buffers -- and the arguments in front of the augmentation block are theirs.
 *   max_shift        S: the shift is uniform on [-S, S], 0 <= S < T
 *   gain_lo, gain_hi, volume_lo, volume_hi   linear amplitude ranges, finite, 0 <= lo <= hi
 *   noise            NULL, or [noise_clips][noise_len] fp32 background recordings, noise_len >= T;  noise_clips 0: none
 *   noise_threshold  floor(noise_prob * 2^32): a row is mixed where its coin's 32 bits lie below it (and there is noise)
 * Row b (srwn_pair_draw_aug: pair b, side 0 its left clip and side 1 its right one; srwn_batch_draw_aug: side 0) at position
 * p takes six draws h = mix64((seed ^ salt) + GOLDEN * (2 p + side + 1)), one salt per quantity (dataset.augment_plan):
 *   shift = (((h >> 32) (2 S + 1)) >> 32) - S;   gain = lo + u (hi - lo) with u = (float)(h >> 40) * 2^-24 (exact), the
 *   subtraction, the product and the sum each rounded to fp32;   mix = (h >> 32) < noise_threshold;   noise record
 *   ((h >> 32) noise_clips) >> 32;   noise offset ((h >> 32) (noise_len - T + 1)) >> 32;   volume as gain.
 * With row[0..T) the cropped clip, the sample rule (dataset.augment_rows) is
 *   xs[j] = row[j - shift] where 0 <= j - shift < T, else +0;   n[j] = noise[record][offset + j] and v = volume where the
 *   row is mixed, else n[j] = +0 and v = +0;   y[j] = fp32(fp32(gain * xs[j]) + fp32(v * n[j])), no fused multiply-add;
 *   then y < -1 ? -1 : (y > 1 ? 1 : y), so a NaN passes.  Subnormal products are kept.
 * audio0, audio1 and the mu-law codes (srwn_pair_draw_aug: audio) all hold y; one-hot rows, indices, y, left, right and y_log
 * are the plain entries'.
 * Errors, all before any launch: the plain entry's, and max_shift outside [0, T), a range with a negative end, lo > hi or a
 * value that is not finite, noise_clips < 0, noise_len < T with noise_clips > 0, noise_threshold outside [0, 2^32], a noise
 * pointer that is not 4-byte aligned (-2); noise_clips > 0 with a null noise (-3). */
int srwn_batch_draw_aug(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len, const int64_t* state,
                        int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank, int32_t world, float* audio0,
                        float* audio1, int32_t* codes, int32_t quantization_channels, void* onehot, int64_t onehot_ld,
                        int32_t onehot_rows, int32_t onehot_col0, int32_t num_classes, int32_t onehot_dtype,
                        int32_t* indices, int32_t max_shift, float gain_lo, float gain_hi, const float* noise,
                        int32_t noise_clips, int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi,
                        void* stream);
int srwn_pair_draw_aug(const float* clips, const int32_t* labels, const int32_t* order, const int32_t* place,
                       const int32_t* class_start, int32_t num_classes, int32_t num_clips, int64_t clip_len,
                       const int64_t* state, int32_t P, int32_t T, int64_t same_threshold, int32_t shuffle, int32_t crop,
                       int32_t rank, int32_t world, float* audio, float* y, int32_t* left, int32_t* right, float* y_log,
                       int32_t max_shift, float gain_lo, float gain_hi, const float* noise, int32_t noise_clips,
                       int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi, void* stream);

/* ---- speed perturbation in the augmented draws (since srwn_version() 128; csrc/srwn_resample.hip): srwn_batch_draw_aug and
 * srwn_pair_draw_aug with every row resampled by a factor of its own, y(j) = x(j * s), before shift, gain, noise and clamp act
 * on it -- tempo and pitch move together, by 12 log2(s) semitones.  Everything the _aug entries say holds, and the arguments
 * in front of the resampling block are theirs.
 *   table            [SRWN_RESAMPLE_PHASES][taps] fp32, the polyphase low-pass dataset.resample_table states: tap k of phase
 *                    f sits k - (taps / 2 - 1) - f / SRWN_RESAMPLE_PHASES samples from the position.  Only read.
 *   taps             even, 2 .. 64
 *   step_lo, step_hi speeds as fixed-point steps with 24 fraction bits, round(s * 2^24): 2^23 <= step_lo <= step_hi <= 2^25
 * The row takes a seventh draw h = mix64((seed ^ salt) + GOLDEN * (2 p + side + 1)) (dataset.speed_plan; the other six do not
 * move): step = step_lo + (((h >> 32) (step_hi - step_lo + 1)) >> 32).  With row[0..T) the cropped clip and +0 outside it
 * (the record's samples beyond the crop window are never read), q = jj * step as an unsigned 64-bit integer, i = q >> 24 and
 * f = (q >> (24 - log2 SRWN_RESAMPLE_PHASES)) & (SRWN_RESAMPLE_PHASES - 1), the resampled row (dataset.resample_rows) is
 *   r[jj] = the sum over k = 0 .. taps - 1, in that order from +0, of fp32(table[f][k] * row[i - (taps / 2 - 1) + k]),
 * every product and every partial sum rounded to fp32, no fused multiply-add.  The _aug entries' sample rule then reads r
 * where it reads row: xs[j] = r[j - shift] where 0 <= j - shift < T, else +0.  All audio outputs and the codes hold y.
 * Errors, all before any launch: the _aug entry's, and taps odd or outside [2, 64], step_lo > step_hi, a step outside
 * [2^23, 2^25], a table that is not 4-byte aligned (-2); a null table (-3). */
#define SRWN_RESAMPLE_PHASES 4096
int srwn_batch_draw_warp(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len, const int64_t* state,
                         int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank, int32_t world, float* audio0,
                         float* audio1, int32_t* codes, int32_t quantization_channels, void* onehot, int64_t onehot_ld,
                         int32_t onehot_rows, int32_t onehot_col0, int32_t num_classes, int32_t onehot_dtype,
                         int32_t* indices, int32_t max_shift, float gain_lo, float gain_hi, const float* noise,
                         int32_t noise_clips, int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi,
                         const float* table, int32_t taps, int32_t step_lo, int32_t step_hi, void* stream);
int srwn_pair_draw_warp(const float* clips, const int32_t* labels, const int32_t* order, const int32_t* place,
                        const int32_t* class_start, int32_t num_classes, int32_t num_clips, int64_t clip_len,
                        const int64_t* state, int32_t P, int32_t T, int64_t same_threshold, int32_t shuffle, int32_t crop,
                        int32_t rank, int32_t world, float* audio, float* y, int32_t* left, int32_t* right, float* y_log,
                        int32_t max_shift, float gain_lo, float gain_hi, const float* noise, int32_t noise_clips,
                        int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi, const float* table,
                        int32_t taps, int32_t step_lo, int32_t step_hi, void* stream);

/* ---- room reverberation in the augmented draws (since srwn_version() 129; csrc/srwn_room.hip): srwn_batch_draw_warp and
 * srwn_pair_draw_warp with a row convolved with a room impulse response between resampling and shift, gain, noise and clamp.
 * Everything the _warp entries say holds, and the arguments in front of the room block are theirs, with one addition:
 * table == NULL with taps == 0 and step_lo == step_hi == 2^24 means "no resampling" -- the row is the cropped clip, as in the
 * _aug entries (through the table, phase 0 would turn a -0.0 into +0.0).
 *   rir              [rir_clips][rir_len] fp32, the impulse responses.  Only read.
 *   rir_clips        >= 1
 *   rir_len          K, 1 .. SRWN_ROOM_MAX_TAPS
 *   rir_threshold    floor(reverb_prob * 2^32), in [0, 2^32]
 * The row takes an eighth and a ninth draw h = mix64((seed ^ salt) + GOLDEN * (2 p + side + 1)) (dataset.reverb_plan; the
 * other seven do not move): it is reverberated where (h_coin >> 32) < rir_threshold, with the response
 * ((h_pick >> 32) rir_clips) >> 32.  With r[0..T) the resampled (or cropped) row and +0 outside it, and h that response,
 *   e[jj] = the sum over k = 0 .. K - 1, in that order from +0, of fp32(h[k] * r[jj - k]),
 * every product and every partial sum rounded to fp32, no fused multiply-add, subnormals kept (dataset.reverb_rows): the
 * tail beyond T is cut.  The sample rule then reads e where it reads r: xs[j] = e[j - shift] where 0 <= j - shift < T, else
 * +0; the noise is added dry.  A row whose coin is off has the bits the _warp (or, without a table, the _aug) entry gives it.
 * Errors, all before any launch: the _aug and _warp entries' (a null table with taps or another step: -3), and rir_clips < 1,
 * rir_len outside [1, SRWN_ROOM_MAX_TAPS], rir_threshold outside [0, 2^32], rir not 4-byte aligned (-2); a null rir (-3). */
#define SRWN_ROOM_MAX_TAPS 8192
int srwn_batch_draw_room(const float* clips, const int32_t* labels, int32_t num_clips, int64_t clip_len, const int64_t* state,
                         int32_t B, int32_t T, int32_t shuffle, int32_t crop, int32_t rank, int32_t world, float* audio0,
                         float* audio1, int32_t* codes, int32_t quantization_channels, void* onehot, int64_t onehot_ld,
                         int32_t onehot_rows, int32_t onehot_col0, int32_t num_classes, int32_t onehot_dtype,
                         int32_t* indices, int32_t max_shift, float gain_lo, float gain_hi, const float* noise,
                         int32_t noise_clips, int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi,
                         const float* table, int32_t taps, int32_t step_lo, int32_t step_hi, const float* rir,
                         int32_t rir_clips, int32_t rir_len, int64_t rir_threshold, void* stream);
int srwn_pair_draw_room(const float* clips, const int32_t* labels, const int32_t* order, const int32_t* place,
                        const int32_t* class_start, int32_t num_classes, int32_t num_clips, int64_t clip_len,
                        const int64_t* state, int32_t P, int32_t T, int64_t same_threshold, int32_t shuffle, int32_t crop,
                        int32_t rank, int32_t world, float* audio, float* y, int32_t* left, int32_t* right, float* y_log,
                        int32_t max_shift, float gain_lo, float gain_hi, const float* noise, int32_t noise_clips,
                        int64_t noise_len, int64_t noise_threshold, float volume_lo, float volume_hi, const float* table,
                        int32_t taps, int32_t step_lo, int32_t step_hi, const float* rir, int32_t rir_clips,
                        int32_t rir_len, int64_t rir_threshold, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRWN_H */
