// Device-resident evaluation of an embedding model (srwn.h, srwn_version() 125): the two launches an EmbedSampler
// (sr-wavenet_amd/dataset.py) adds to a tower's forward pass when it sweeps a labelled held-out set.
//
//   srwn_embed_collect  behind the forward pass of every step: reads {seed, step, sweep} from device memory, copies the
//                       step's valid rows of emb [B, D] to their records in result slot sweep % sweep_capacity and ticks the
//                       state exactly as srwn_eval_classes does.  Rows of the ragged tail write nothing.  One workgroup.
//   srwn_pair_sweep     once behind a sweep's last step, over all N x N pairs of the slot of the sweep just completed
//                       ((sweep - 1) % sweep_capacity, read from device memory: a captured sequence serves every sweep).
//                       One workgroup of 256 threads per record i:
//                         A  d(i, j) for every j into LDS (and, where asked for, into dist [N, N]),
//                         B  the pairs i < j into two LDS histograms (same label / other label) and the first j != i and
//                            the first j != i of i's label in the order (d, j),
//                         C  the number of j of another label in front of that same-label neighbour,
//                         D  the LDS histograms into the slot's with 64-bit integer atomic adds.
//                       A one-workgroup launch in front of it (the same entry point enqueues both) clears the slot's two
//                       histograms, so a second call into a slot counts afresh.
//
// d(i, j) has the bits of srwn_contrastive_head and srwn_gallery_match for the same two rows: lane l of a 64-lane wave adds
// the squares of k = l, l + 64, ... with one fmaf each from 0, an xor butterfly (32, 16, 8, 4, 2, 1) adds the lanes, then
// sqrtf(1e-8f + ss).  For D > 16 a wave takes a pair and does exactly that.  For D <= 16 (the embeddings a verification
// model is trained with: siamese.py's has two dimensions) every lane of that wave holds at most one square and 48 lanes
// hold none, so a THREAD takes a pair: it replays the butterfly as the tree it is -- node (level, r) is the sum over the
// lanes congruent to r modulo 2^level, node (level, r) = node (level + 1, r) + node (level + 1, r + 2^level), the leaves at
// level 6 are the lanes -- built for the power of two DP >= D: the subtrees without a lane below DP are left out and the
// leaves in [D, DP) are +0, which changes no bit of a non-negative (or NaN) partner.  (Trees of 32 and 64 leaves keep that
// many row offsets in scalar registers and spill them; the wave form serves those widths.)
// Everything counted is an integer; every selection is merged by the order, never by arrival: no result depends on the
// order in which waves or workgroups run.  No scratch (build.py refuses an object in which these kernels spill).
#include <cmath>
#include "srwn_common.h"
#include "srwn_host.h"
#include "../../include/srwn.h"

using namespace srwn;

namespace {

constexpr int kPairThreads = 256;
constexpr int kPairWave = 64;
constexpr int kPairWaves = kPairThreads / kPairWave;
constexpr int kPairMaxN = 4096;        // records of a set: drow [N] floats of LDS, one workgroup per record
constexpr int kPairMaxBins = 4096;     // 2 x bins LDS counters
constexpr int kPairMaxD = 1024;        // the record's own embedding in LDS
constexpr int kPairTreeD = 16;         // up to here a thread takes a pair

struct CollectArgs {
  const float* emb; const int32_t* indices; int64_t* state; float* slots; int32_t* seen;
  int32_t N, B, D, rank, world, capacity;
};

__global__ __launch_bounds__(kPairThreads) void embed_collect_kernel(const CollectArgs a) {
  const int tid = (int)threadIdx.x;
  // every thread reads the state here; thread 0 writes it behind the barrier
  const unsigned long long step = (unsigned long long)a.state[1], sweep = (unsigned long long)a.state[2];
  const int64_t slot = (int64_t)(sweep % (unsigned long long)a.capacity);
  const unsigned long long p0 = (step * (unsigned long long)a.world + (unsigned long long)a.rank) * (unsigned long long)a.B;
  // the valid rows are the first `valid` ones: positions rise with b
  const int valid = p0 >= (unsigned long long)a.N ? 0 : (int)min((unsigned long long)a.B, (unsigned long long)a.N - p0);
  float* const dst = a.slots + slot * (int64_t)a.N * a.D;
  const int64_t total = (int64_t)valid * a.D;
  for (int64_t q = tid; q < total; q += kPairThreads) {
    const int b = (int)(q / a.D), c = (int)(q % a.D);
    const int32_t rec = a.indices[b];
    if ((uint32_t)rec >= (uint32_t)a.N) continue;                 // (the draw's records are p % N: never taken)
    dst[(int64_t)rec * a.D + c] = a.emb[q];
  }
  __syncthreads();
  if (tid == 0) {
    a.seen[slot] = (step == 0ull ? 0 : a.seen[slot]) + valid;     // a sweep's first step starts the slot's count over
    const unsigned long long per = (unsigned long long)a.B * (unsigned long long)a.world;
    const unsigned long long steps = ((unsigned long long)a.N + per - 1ull) / per;
    if (step + 1ull >= steps) { a.state[1] = 0; a.state[2] = (int64_t)(sweep + 1ull); }
    else a.state[1] = (int64_t)(step + 1ull);
  }
}

struct PairArgs {
  const float* slots; const int32_t* labels; const int64_t* state;
  int32_t* nearest; int32_t* same_nearest; int32_t* rank_same; float* nearest_dist; float* same_dist;
  unsigned long long* hist_same; unsigned long long* hist_diff; float* dist;
  int32_t N, D, capacity, bins;
  float scale;
};

// the slot of the sweep just completed, or -1 before the first one
__device__ __forceinline__ int64_t pair_slot(const PairArgs& a) {
  const long long sweep = (long long)a.state[2];
  return sweep <= 0 ? -1 : (int64_t)((unsigned long long)(sweep - 1) % (unsigned long long)a.capacity);
}

__global__ __launch_bounds__(kPairThreads) void pair_clear_kernel(const PairArgs a) {
  const int64_t slot = pair_slot(a);
  if (slot < 0) return;
  for (int q = (int)threadIdx.x; q < a.bins; q += kPairThreads) {
    a.hist_same[slot * a.bins + q] = 0ull;
    a.hist_diff[slot * a.bins + q] = 0ull;
  }
}

// a before b in the order of the selections: the smaller distance, on equal distances the lower index; anything before none
__device__ __forceinline__ bool pair_before(float da, int a, float db, int b) {
  return b < 0 || da < db || (da == db && a < b);
}

// the butterfly of a wave whose lanes 0 .. D - 1 (D <= DP <= 16, DP a power of two) hold one square each, as a tree: the sum
// over the lanes congruent to r modulo 2^LEVEL.  A subtree's lowest lane is r, so r >= DP leaves it out at compile time
// (+0); a leaf in [D, DP) is +0 by a select on a load inside the row, so no branch is taken per pair.
template <int LEVEL, int DP>
__device__ __forceinline__ float pair_tree(const float* __restrict__ ei, const float* __restrict__ ej, int r, int D) {
  if (r >= DP) return 0.0f;
  if constexpr (LEVEL == 6) {
    const int k = min(r, D - 1);
    const float df = ei[k] - ej[k];
    return r < D ? fmaf(df, df, 0.0f) : 0.0f;
  } else {
    const float lo = pair_tree<LEVEL + 1, DP>(ei, ej, r, D);
    const float hi = pair_tree<LEVEL + 1, DP>(ei, ej, r + (1 << LEVEL), D);
    return lo + hi;
  }
}

__device__ __forceinline__ float pair_wave_sum64(float v) {      // every lane ends with the sum
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kPairWave);
  return v;
}

// the first of the wave's candidates in the order, in every lane
__device__ __forceinline__ void pair_wave_first(float& d, int& j) {
#pragma unroll
  for (int m = kPairWave / 2; m >= 1; m >>= 1) {
    const float od = __shfl_xor(d, m, kPairWave);
    const int oj = __shfl_xor(j, m, kPairWave);
    if (oj >= 0 && pair_before(od, oj, d, j)) { d = od; j = oj; }
  }
}

// DP: the power of two the tree of a thread's pair is built for (D <= DP <= 16); 0: a wave takes a pair (D > 16)
template <int DP>
__global__ __launch_bounds__(kPairThreads) void pair_sweep_kernel(const PairArgs a) {
  extern __shared__ float lds[];                                  // drow [N] | e [D] | hs [bins] | hd [bins]
  __shared__ float wd[2 * kPairWaves];
  __shared__ int wj[2 * kPairWaves];
  __shared__ float s_sd;
  __shared__ int s_sj, s_rank;
  const int64_t slot = pair_slot(a);
  if (slot < 0) return;
  const int tid = (int)threadIdx.x, lane = tid & (kPairWave - 1), wave = tid / kPairWave;
  const int N = a.N, D = a.D, bins = a.bins, i = (int)blockIdx.x;
  float* const drow = lds;
  float* const e = lds + N;
  unsigned* const hs = reinterpret_cast<unsigned*>(lds + N + D);
  unsigned* const hd = hs + bins;
  const float* const emb = a.slots + slot * (int64_t)N * D;
  for (int c = tid; c < D; c += kPairThreads) e[c] = emb[(int64_t)i * D + c];
  for (int q = tid; q < bins; q += kPairThreads) { hs[q] = 0u; hd[q] = 0u; }
  if (tid == 0) s_rank = 0;
  __syncthreads();
  // A: the row's distances, the diagonal by the same formula
  if constexpr (DP > 0) {
    for (int j = tid; j < N; j += kPairThreads)
      drow[j] = sqrtf(1e-8f + pair_tree<0, DP>(e, emb + (int64_t)j * D, 0, D));
  } else {
    for (int j = wave; j < N; j += kPairWaves) {                  // (wave-uniform)
      const float* g = emb + (int64_t)j * D;
      float ss = 0.0f;
      for (int k = lane; k < D; k += kPairWave) {
        const float df = e[k] - g[k];
        ss = fmaf(df, df, ss);
      }
      ss = pair_wave_sum64(ss);
      if (lane == 0) drow[j] = sqrtf(1e-8f + ss);
    }
  }
  __syncthreads();
  // B: the histograms of the pairs i < j, and the first j != i among all and among i's label
  const int32_t lab = a.labels[i];
  float bd = INFINITY, sd = INFINITY;
  int bj = -1, sj = -1;
  for (int j = tid; j < N; j += kPairThreads) {
    const float d = drow[j];
    if (a.dist) a.dist[(int64_t)i * N + j] = d;
    if (j == i) continue;
    const bool same = a.labels[j] == lab;
    if (j > i) {
      const float p = d * a.scale;
      const int bin = p < (float)bins ? (int)p : bins - 1;        // not below bins, NaN included: the last bin
      atomicAdd((same ? hs : hd) + bin, 1u);
    }
    if (pair_before(d, j, bd, bj)) { bd = d; bj = j; }
    if (same && pair_before(d, j, sd, sj)) { sd = d; sj = j; }
  }
  pair_wave_first(bd, bj);
  pair_wave_first(sd, sj);
  if (lane == 0) {
    wd[wave] = bd; wj[wave] = bj;
    wd[kPairWaves + wave] = sd; wj[kPairWaves + wave] = sj;
  }
  __syncthreads();
  if (tid == 0) {
    for (int h = 0; h < 2; ++h) {
      float d = wd[h * kPairWaves];
      int j = wj[h * kPairWaves];
      for (int w = 1; w < kPairWaves; ++w) {
        const float od = wd[h * kPairWaves + w];
        const int oj = wj[h * kPairWaves + w];
        if (oj >= 0 && pair_before(od, oj, d, j)) { d = od; j = oj; }
      }
      const int64_t o = slot * (int64_t)N + i;
      if (h == 0) { a.nearest[o] = j; a.nearest_dist[o] = j < 0 ? INFINITY : d; }
      else { a.same_nearest[o] = j; a.same_dist[o] = j < 0 ? INFINITY : d; s_sd = d; s_sj = j; }
    }
  }
  __syncthreads();
  // C: the records of another label in front of the same-label neighbour
  const float fd = s_sd;
  const int fj = s_sj;
  if (fj >= 0) {                                                  // (workgroup-uniform)
    int cnt = 0;
    for (int j = tid; j < N; j += kPairThreads)
      if (j != i && a.labels[j] != lab && pair_before(drow[j], j, fd, fj)) ++cnt;
#pragma unroll
    for (int m = kPairWave / 2; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, kPairWave);
    if (lane == 0) atomicAdd(&s_rank, cnt);
  }
  __syncthreads();
  if (tid == 0) a.rank_same[slot * (int64_t)N + i] = fj >= 0 ? s_rank : -1;
  // D: this record's counts into the slot's histograms
  for (int q = tid; q < bins; q += kPairThreads) {
    const unsigned ns = hs[q], nd = hd[q];
    if (ns) atomicAdd(a.hist_same + slot * bins + q, (unsigned long long)ns);
    if (nd) atomicAdd(a.hist_diff + slot * bins + q, (unsigned long long)nd);
  }
}

}  // namespace

extern "C" int srwn_embed_collect(const float* emb, const int32_t* indices, int64_t* state, int32_t num_clips, int32_t B,
                                  int32_t D, int32_t rank, int32_t world, int32_t sweep_capacity, float* slots_emb,
                                  int32_t* seen, void* stream) {
  if (!emb || !indices || !state || !slots_emb || !seen) return set_error(SRWN_E_NULL, "embed_collect: null pointer");
  if (D < 1 || D > kPairMaxD) return set_error(SRWN_E_SHAPE, "embed_collect: D=%d (1 to %d dimensions)", D, kPairMaxD);
  if (B < 1 || num_clips < 1 || num_clips > kPairMaxN)
    return set_error(SRWN_E_SHAPE, "embed_collect: %d clips (1 to %d), B=%d", num_clips, kPairMaxN, B);
  if (world < 1 || rank < 0 || rank >= world) return set_error(SRWN_E_SHAPE, "embed_collect: rank %d of %d", rank, world);
  if (sweep_capacity < 1) return set_error(SRWN_E_SHAPE, "embed_collect: sweep_capacity %d", sweep_capacity);
  CollectArgs a;
  a.emb = emb; a.indices = indices; a.state = state; a.slots = slots_emb; a.seen = seen;
  a.N = num_clips; a.B = B; a.D = D; a.rank = rank; a.world = world; a.capacity = sweep_capacity;
  hipLaunchKernelGGL(embed_collect_kernel, dim3(1), dim3(kPairThreads), 0, (hipStream_t)stream, a);
  return check_launch("embed_collect");
}

extern "C" int srwn_pair_sweep(const float* slots_emb, const int32_t* labels, const int64_t* state, int32_t num_clips,
                               int32_t D, int32_t sweep_capacity, int32_t bins, float scale, int32_t* nearest,
                               int32_t* same_nearest, int32_t* rank_same, float* nearest_dist, float* same_dist,
                               int64_t* hist_same, int64_t* hist_diff, float* dist, void* stream) {
  if (!slots_emb || !labels || !state || !nearest || !same_nearest || !rank_same || !nearest_dist || !same_dist ||
      !hist_same || !hist_diff)
    return set_error(SRWN_E_NULL, "pair_sweep: null pointer");
  if (D < 1 || D > kPairMaxD) return set_error(SRWN_E_SHAPE, "pair_sweep: D=%d (1 to %d dimensions)", D, kPairMaxD);
  if (num_clips < 1 || num_clips > kPairMaxN)
    return set_error(SRWN_E_SHAPE, "pair_sweep: %d clips (1 to %d)", num_clips, kPairMaxN);
  if (bins < 1 || bins > kPairMaxBins) return set_error(SRWN_E_SHAPE, "pair_sweep: bins=%d (1 to %d)", bins, kPairMaxBins);
  if (!(scale > 0.0f) || !std::isfinite(scale)) return set_error(SRWN_E_SHAPE, "pair_sweep: scale=%g (finite, above 0)", scale);
  if (sweep_capacity < 1) return set_error(SRWN_E_SHAPE, "pair_sweep: sweep_capacity %d", sweep_capacity);
  PairArgs a;
  a.slots = slots_emb; a.labels = labels; a.state = state;
  a.nearest = nearest; a.same_nearest = same_nearest; a.rank_same = rank_same; a.nearest_dist = nearest_dist;
  a.same_dist = same_dist; a.hist_same = reinterpret_cast<unsigned long long*>(hist_same);
  a.hist_diff = reinterpret_cast<unsigned long long*>(hist_diff); a.dist = dist;
  a.N = num_clips; a.D = D; a.capacity = sweep_capacity; a.bins = bins; a.scale = scale;
  hipLaunchKernelGGL(pair_clear_kernel, dim3(1), dim3(kPairThreads), 0, (hipStream_t)stream, a);
  if (const int rc = check_launch("pair_sweep (clear)")) return rc;
  const size_t lds = ((size_t)num_clips + (size_t)D + 2u * (size_t)bins) * sizeof(float);     // at most 52 KB
  const dim3 grid((unsigned)num_clips), block(kPairThreads);
  const hipStream_t st = (hipStream_t)stream;
  if (D > kPairTreeD) hipLaunchKernelGGL(pair_sweep_kernel<0>, grid, block, lds, st, a);
  else if (D > 8) hipLaunchKernelGGL(pair_sweep_kernel<16>, grid, block, lds, st, a);
  else if (D > 4) hipLaunchKernelGGL(pair_sweep_kernel<8>, grid, block, lds, st, a);
  else if (D > 2) hipLaunchKernelGGL(pair_sweep_kernel<4>, grid, block, lds, st, a);
  else hipLaunchKernelGGL(pair_sweep_kernel<2>, grid, block, lds, st, a);
  return check_launch("pair_sweep");
}
