// MoE routing and token alignment: what stands between the router's logits and the grouped expert GEMMs of moe_gemm.hip.
//
// topk_softmax (sgl-kernel/csrc/moe/moe_topk_softmax_kernels.cu, op signature sgl-kernel/python/sgl_kernel/moe.py:28-36):
//   one wave per token row, E <= 512 logits in 8 registers per lane (expert e in lane e % 64, register e / 64), row maximum and
//   sum by the lane-swap / DPP reductions of common.h, no LDS and no barrier.  The k winners are taken one at a time: the wave's
//   largest remaining logit, the LOWEST index among equals (the order of torch.topk over the softmax; selecting on the logit
//   instead of on exp(logit - max) / sum is the same order and cannot tie where the probabilities underflow), weight
//   exp(logit - max) / sum in f32, divided by the k weights' sum with renormalize.
//
// moe_align_block_size (sgl-kernel/csrc/moe/moe_align_kernel.cu, moe.py:6-25; layout: fused_moe.py:549-619): pairs
//   p = token * topk + j sorted by expert, every expert's run padded to a multiple of block_size with the value P = numel, one
//   experts_ids entry per block, the padded total in num_tokens_post_pad[0].  Beyond the reference: WITHIN an expert the pair
//   indices ascend (a stable counting sort; no position is handed out by an atomic, so the layout is the same on every run), and
//   ids outside [0, num_experts) -- the -1 of padded tokens and of expert parallelism -- are left out.
//   The unit of work is a wave that owns a contiguous range of pairs: it counts its range into a private LDS histogram (integer
//   LDS atomics: a count does not depend on their order), and after the scan it walks the range again 64 pairs at a time, where
//   the lanes that hold the same expert find their rank with one ballot per distinct expert (rank = lanes below with the same id)
//   on top of the wave's private running base for that expert.
//     P <= 4096 (decode): one 512-thread workgroup, 8 such waves, histogram -> scan -> scatter between barriers.
//     larger (prefill):   up to 256 waves in three launches: histograms to a [units][E] workspace, one workgroup that turns them
//                         into per-unit bases and lays out blocks and padding, and the scatter.
//   The scan: per expert a serial prefix over the units, then one wave scans the padded counts (ceil(E / 64) experts per lane,
//   __shfl_up over the lanes); block b's expert is found by bisection over the expert starts.
//   Nothing is read back to the host: every size the launches need is a function of P and E.
#include "common.h"

namespace {

constexpr int kTopkMaxE = 512, kTopkMax = 32;
constexpr int kAlignMaxE = 1024;
constexpr int kAlignSmallP = 4096;   // one workgroup up to here
constexpr int kSmallWaves = 8;
constexpr int kUnitPairs = 1024, kMaxUnits = 256;

// ---- topk_softmax -----------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(256) void topk_softmax_kernel(float* __restrict__ topk_w, int* __restrict__ topk_i,
                                                           const T* __restrict__ gate, int tokens, int E, int topk, int renorm) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= tokens) return;   // wave uniform, and the kernel has no barrier
  const T* g = gate + (int64_t)row * E;
  float x[8];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = lane + 64 * i;
    x[i] = e < E ? (float)g[e] : -INFINITY;
    mx = fmaxf(mx, x[i]);
  }
  mx = wave_reduce_max(mx);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += __expf(x[i] - mx);   // exp(-inf) = 0 for the lanes past E
  const float inv = 1.0f / wave_reduce_sum(s);

  float my_w = 0.f;
  int my_i = 0;
  for (int j = 0; j < topk; ++j) {
    float bv = -INFINITY;
    int bi = 1024;
#pragma unroll
    for (int i = 0; i < 8; ++i)   // ascending index and a strict compare: the lowest index among equals stays
      if (x[i] > bv) { bv = x[i]; bi = lane + 64 * i; }
    const float m = wave_reduce_max(bv);
    // the lowest index among the lanes that hold the maximum (indices are exact in f32)
    const int idx = (int)-wave_reduce_max(-(float)(bv == m ? bi : 1024));
    if (lane == j) { my_w = __expf(m - mx) * inv; my_i = idx; }
    if ((idx & 63) == lane) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i == (idx >> 6)) x[i] = -INFINITY;
    }
  }
  if (renorm) my_w = my_w / wave_reduce_sum(lane < topk ? my_w : 0.f);
  if (lane < topk) {
    topk_w[(int64_t)row * topk + lane] = my_w;
    topk_i[(int64_t)row * topk + lane] = my_i;
  }
}

// ---- moe_align_block_size ---------------------------------------------------------------------------------------------------

struct AlignParams {
  const int* ids;   // [P]
  int* sorted;      // [capacity]
  int* expert_ids;
  int* num_post_pad;
  int* cumsum;      // [E + 1]
  int* hist;        // [units][E], multi-workgroup form only
  int P, E, bs, capacity, pad_tail, units, chunk;
};

// counts of the valid ids of pairs [lo, hi) into the wave's own h[E] (LDS, zeroed)
__device__ __forceinline__ void wave_hist(const int* ids, int lo, int hi, int E, int* h, int lane) {
  for (int p = lo + lane; p < hi; p += 64) {
    const int e = ids[p];
    if ((unsigned)e < (unsigned)E) atomicAdd(&h[e], 1);
  }
}

// Stable scatter of pairs [lo, hi): base[e] (the wave's own, LDS) is where this wave's next pair of expert e goes.  64 pairs at a
// time, one round per distinct expert among them: its lanes read base[e] (one broadcast read), take base + the number of lower
// lanes of the round, and the lowest of them moves base on -- after the read in program order, and LDS serves a wave in order.
__device__ __forceinline__ void wave_scatter(const int* ids, int lo, int hi, int E, volatile int* base, int* sorted, int lane) {
  for (int p0 = lo; p0 < hi; p0 += 64) {
    const int p = p0 + lane;
    const int e = p < hi ? ids[p] : -1;
    const bool valid = (unsigned)e < (unsigned)E;
    uint64_t todo = __ballot(valid);
    while (todo) {   // wave uniform
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const int e0 = __builtin_amdgcn_readlane(e, leader);
      const uint64_t m = __ballot(valid && e == e0);
      if (valid && e == e0) {
        const int b = base[e0];
        sorted[b + __popcll(m & ((1ull << lane) - 1ull))] = p;
        if (lane == leader) base[e0] = b + __popcll(m);
      }
      todo &= ~m;
    }
  }
}

__device__ __forceinline__ int pad_to(int c, int bs) { return (c + bs - 1) / bs * bs; }

// The whole workgroup: counts[E] (LDS) -> start[E + 1] (LDS; start[E] = padded total), cumsum, the padding entries of every
// expert's run, the expert of every block, the total.  Ends in a barrier.
__device__ __forceinline__ void finish_layout(const AlignParams& p, const int* counts, int* start) {
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, E = p.E;
  if (tid < 64) {
    const int per = (E + 63) / 64, lo = lane * per;
    int sum = 0;
    for (int k = 0; k < per; ++k)
      if (lo + k < E) sum += pad_to(counts[lo + k], p.bs);
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(incl, d, 64);
      if (lane >= d) incl += y;
    }
    int run = incl - sum;
    for (int k = 0; k < per; ++k)
      if (lo + k < E) { start[lo + k] = run; run += pad_to(counts[lo + k], p.bs); }
    if (lane == 63) start[E] = incl;
  }
  __syncthreads();
  const int total = start[E];
  for (int e = tid; e < E; e += nthr) {
    p.cumsum[e] = start[e];
    for (int q = start[e] + counts[e]; q < start[e + 1]; ++q) p.sorted[q] = p.P;
  }
  if (tid == 0) { p.cumsum[E] = total; p.num_post_pad[0] = total; }
  for (int b = tid; b < total / p.bs; b += nthr) {
    // the one expert with start[e] <= b * bs < start[e + 1]: never an empty one
    const int x = b * p.bs;
    int lo = 0, hi = E - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (start[mid + 1] <= x) lo = mid + 1; else hi = mid;
    }
    p.expert_ids[b] = lo;
  }
  if (p.pad_tail)
    for (int q = total + tid; q < p.capacity; q += nthr) p.sorted[q] = p.P;
  __syncthreads();
}

__global__ __launch_bounds__(64 * kSmallWaves) void moe_align_small_kernel(const AlignParams p) {
  __shared__ int h[kSmallWaves * kAlignMaxE];
  __shared__ int counts[kAlignMaxE], start[kAlignMaxE + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, E = p.E;
  for (int i = tid; i < kSmallWaves * E; i += 64 * kSmallWaves) h[i] = 0;
  __syncthreads();
  const int chunk = (p.P + kSmallWaves - 1) / kSmallWaves;
  const int lo = min(w * chunk, p.P), hi = min(lo + chunk, p.P);
  wave_hist(p.ids, lo, hi, E, h + w * E, lane);
  __syncthreads();
  for (int e = tid; e < E; e += 64 * kSmallWaves) {   // exclusive prefix over the waves, in place
    int run = 0;
    for (int ww = 0; ww < kSmallWaves; ++ww) { const int c = h[ww * E + e]; h[ww * E + e] = run; run += c; }
    counts[e] = run;
  }
  __syncthreads();
  finish_layout(p, counts, start);
  for (int e = tid; e < E; e += 64 * kSmallWaves)
    for (int ww = 0; ww < kSmallWaves; ++ww) h[ww * E + e] += start[e];
  __syncthreads();
  wave_scatter(p.ids, lo, hi, E, h + w * E, p.sorted, lane);
}

__global__ __launch_bounds__(256) void moe_align_hist_kernel(const AlignParams p) {
  __shared__ int h[4 * kAlignMaxE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, E = p.E;
  for (int i = tid; i < 4 * E; i += 256) h[i] = 0;
  __syncthreads();
  const int u = blockIdx.x * 4 + w;
  const int lo = (int)min((int64_t)u * p.chunk, (int64_t)p.P), hi = min(lo + p.chunk, p.P);
  wave_hist(p.ids, lo, hi, E, h + w * E, lane);
  __syncthreads();
  for (int i = tid; i < 4 * E; i += 256) p.hist[(int64_t)blockIdx.x * 4 * E + i] = h[i];
}

__global__ __launch_bounds__(1024) void moe_align_scan_kernel(const AlignParams p) {
  __shared__ int counts[kAlignMaxE], start[kAlignMaxE + 1];
  for (int e = threadIdx.x; e < p.E; e += 1024) {   // exclusive prefix over the units, in place
    int run = 0;
    for (int u = 0; u < p.units; ++u) { const int c = p.hist[(int64_t)u * p.E + e]; p.hist[(int64_t)u * p.E + e] = run; run += c; }
    counts[e] = run;
  }
  __syncthreads();
  finish_layout(p, counts, start);
}

__global__ __launch_bounds__(256) void moe_align_scatter_kernel(const AlignParams p) {
  __shared__ int base[4 * kAlignMaxE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, E = p.E;
  for (int i = tid; i < 4 * E; i += 256) base[i] = p.cumsum[i % E] + p.hist[(int64_t)blockIdx.x * 4 * E + i];
  __syncthreads();
  const int u = blockIdx.x * 4 + w;
  const int lo = (int)min((int64_t)u * p.chunk, (int64_t)p.P), hi = min(lo + p.chunk, p.P);
  wave_scatter(p.ids, lo, hi, E, base + w * E, p.sorted, lane);
}

int align_units(int64_t P) {
  if (P <= kAlignSmallP) return 0;
  int64_t u = (P + kUnitPairs - 1) / kUnitPairs;
  if (u > kMaxUnits) u = kMaxUnits;
  return (int)((u + 3) / 4 * 4);
}

}  // namespace

extern "C" int sgl_mi355_topk_softmax(float* topk_weights, int* topk_ids, const void* gating_output, int num_tokens, int num_experts,
                                      int topk, int renormalize, int dtype, void* stream) {
  SGL_CHECK(num_tokens >= 0 && num_experts > 0 && topk > 0, "topk_softmax: bad shape (tokens=%d experts=%d topk=%d)", num_tokens,
            num_experts, topk);
  SGL_CHECK(num_experts <= kTopkMaxE, "topk_softmax: num_experts=%d above %d", num_experts, kTopkMaxE);
  SGL_CHECK(topk <= kTopkMax && topk <= num_experts, "topk_softmax: topk=%d above min(num_experts=%d, %d)", topk, num_experts, kTopkMax);
  SGL_CHECK(dtype == SGL_F32 || dtype == SGL_BF16 || dtype == SGL_F16, "topk_softmax: gating_output must be f32, bf16 or f16");
  if (num_tokens == 0) return SGL_MI355_OK;
  SGL_CHECK(topk_weights && topk_ids && gating_output, "topk_softmax: null pointer");
  const dim3 grid((num_tokens + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SGL_F32)
    hipLaunchKernelGGL(topk_softmax_kernel<float>, grid, block, 0, st, topk_weights, topk_ids, (const float*)gating_output, num_tokens,
                       num_experts, topk, renormalize);
  else if (dtype == SGL_BF16)
    hipLaunchKernelGGL(topk_softmax_kernel<__bf16>, grid, block, 0, st, topk_weights, topk_ids, (const __bf16*)gating_output,
                       num_tokens, num_experts, topk, renormalize);
  else
    hipLaunchKernelGGL(topk_softmax_kernel<_Float16>, grid, block, 0, st, topk_weights, topk_ids, (const _Float16*)gating_output,
                       num_tokens, num_experts, topk, renormalize);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

// int32 words of workspace sgl_mi355_moe_align_block_size needs (0: the one-workgroup form)
extern "C" int64_t sgl_mi355_moe_align_workspace_ints(int64_t num_pairs, int num_experts) {
  return (int64_t)align_units(num_pairs) * num_experts;
}

extern "C" int sgl_mi355_moe_align_block_size(const int* topk_ids, int64_t num_pairs, int num_experts, int block_size,
                                              int* sorted_token_ids, int64_t sorted_capacity, int* experts_ids,
                                              int* num_tokens_post_pad, int* cumsum_buffer, int pad_sorted_token_ids, int* workspace,
                                              int64_t workspace_ints, void* stream) {
  SGL_CHECK(num_experts > 0 && num_experts <= kAlignMaxE, "moe_align_block_size: num_experts=%d outside [1, %d]", num_experts,
            kAlignMaxE);
  SGL_CHECK(block_size > 0 && block_size <= 1024, "moe_align_block_size: block_size=%d outside [1, 1024]", block_size);
  const int64_t active = num_pairs < num_experts ? num_pairs : num_experts;
  SGL_CHECK(num_pairs >= 0 && num_pairs + active * (block_size - 1) < (1ll << 31), "moe_align_block_size: %lld pairs do not fit int32",
            (long long)num_pairs);
  SGL_CHECK(topk_ids && sorted_token_ids && experts_ids && num_tokens_post_pad && cumsum_buffer, "moe_align_block_size: null pointer");
  SGL_CHECK(sorted_capacity >= num_pairs + active * (block_size - 1),
            "moe_align_block_size: sorted_token_ids holds %lld entries, the worst case needs %lld", (long long)sorted_capacity,
            (long long)(num_pairs + active * (block_size - 1)));
  AlignParams p;
  p.ids = topk_ids; p.sorted = sorted_token_ids; p.expert_ids = experts_ids; p.num_post_pad = num_tokens_post_pad;
  p.cumsum = cumsum_buffer; p.hist = workspace;
  p.P = (int)num_pairs; p.E = num_experts; p.bs = block_size;
  p.capacity = (int)(sorted_capacity < (1ll << 31) - 1 ? sorted_capacity : (1ll << 31) - 1);
  p.pad_tail = pad_sorted_token_ids;
  p.units = align_units(num_pairs);
  p.chunk = p.units ? (int)((num_pairs + p.units - 1) / p.units) : 0;
  hipStream_t st = (hipStream_t)stream;
  if (p.units == 0) {
    hipLaunchKernelGGL(moe_align_small_kernel, dim3(1), dim3(64 * kSmallWaves), 0, st, p);
    SGL_HIP_LAUNCH_CHECK();
    return SGL_MI355_OK;
  }
  SGL_CHECK(workspace && workspace_ints >= (int64_t)p.units * num_experts,
            "moe_align_block_size: %lld pairs need a workspace of %lld int32 (sgl_mi355_moe_align_workspace_ints)", (long long)num_pairs,
            (long long)p.units * num_experts);
  hipLaunchKernelGGL(moe_align_hist_kernel, dim3(p.units / 4), dim3(256), 0, st, p);
  SGL_HIP_LAUNCH_CHECK();
  hipLaunchKernelGGL(moe_align_scan_kernel, dim3(1), dim3(1024), 0, st, p);
  SGL_HIP_LAUNCH_CHECK();
  hipLaunchKernelGGL(moe_align_scatter_kernel, dim3(p.units / 4), dim3(256), 0, st, p);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}
