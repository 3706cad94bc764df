// Grouped expert GEMMs of the fused MoE layer for unquantised 16-bit experts (bf16 / f16), and the sum over topk that ends it.
// Replaces invoke_fused_moe_kernel (python/sglang/srt/layers/moe/fused_moe_triton/fused_moe.py:622-780: the Triton
// fused_moe_kernel) as fused_experts_impl (fused_moe.py:1391-1631) calls it twice, the silu_and_mul between the two calls, and
// moe_sum_reduce (fused_moe.py:1299-1388).
//
//   out[pair][n] = epilogue( sum_k A[row(pair)][k] * W[e(pair)][n][k] )          pair = token * topk + j
//
// over the layout of moe_align_block_size (moe_align.hip): sorted_token_ids holds every expert's pairs padded to a multiple of
// block_size with the value P, experts_ids one expert per block.  A workgroup reads its block's expert and its rows' pairs from
// there and compares its block's first position with num_tokens_post_pad[0] ON THE DEVICE: the grid is sized on the host for the
// worst case (P + min(E, P) * (block_size - 1) positions), so a launch needs no value from the device, no synchronisation and no
// allocation, and a captured graph replays on new routing.  Padding rows load zeros and store nothing.  Every output element is
// written by one thread from one f32 sum in a fixed order: no atomics, the same bits on every run.
//
// Epilogues (one f32 -> 16-bit rounding each; the reference rounds the [M, topk, 2I] product first and silu_and_mul's result again):
//   SILU  (GEMM 1, W = w1[E][2I][K]): a workgroup's weight rows are gate rows n and the up rows I + n of the same columns, so a
//         lane holds both accumulators of an output and writes silu(gate) * up to a2[pair][n]; with
//         apply_router_weight_on_input both accumulators are multiplied by the pair's router weight first, as the reference
//         multiplies GEMM 1's product (the weight is on the INPUT: (w x) W1 = w (x W1)).  A rows are x[pair / topk], gathered,
//         never materialised; the [P, 2I] intermediate is never written.
//   PLAIN (GEMM 2, W = w2[E][H][I]): A rows are a2[pair]; out = acc * topk_weights[pair] unless the weight went in on the input.
//
// v_mfma_f32_16x16x32_{bf16,f16} takes 8 elements (16 bytes) of K per lane and operand: lane (a = lane & 15, g = lane >> 4) gives row
// a of the A and of the B fragment; which 8 of a step's 32 k the hardware pairs with lane group g does not matter as long as A and
// B agree, and both operands of every MFMA below hold THE SAME 16 contiguous bytes of K of their rows.  C: lane (a, g) holds
// column a (weight row), rows 4 g .. 4 g + 3 (pair of the block).  K % 32 == 0 and N % 32 == 0 (K is H or I, N is I or H).
//
// Streaming form (block_size 16; few pairs per expert, decode): the bytes of the active experts' weights are the cost, each read
//   once.  Workgroup = (block, slab of weight rows); its 4 waves split the 128-byte K slices (wave w: slices w, w + 4, ...).
//   Lane (a, g) reads bytes 32 g .. 32 g + 31 of the slice of weight row a with two non-temporal 16-byte loads (a wave's loads
//   cover whole 128-byte lines) straight into two B fragments, and the same bytes of its gathered A row into the A fragments.
//   The A fragments are used by TWO weight fragments per wave -- gate and up of 16 columns (SILU) or 32 columns (PLAIN) -- so the
//   L2 re-read of the gathered rows is half the weight bytes at most (the int8 / block-fp8 streaming forms re-read X once per 16
//   weight rows, which binds them at M = 32..64).  4 slices in flight in registers, no barrier in the loop; K % 64 == 32 leaves
//   a half slice whose lanes g >= 2 read the bytes of lanes g - 2 again and zero their weights.  One LDS reduction sums the four
//   waves' accumulators: wave w finishes row 4 g + w of every lane.
// Tile form (block_size 128; many pairs per expert, prefill): 128 pairs x 128 weight rows per 256-thread workgroup, 4 waves of
//   64 x 64 (4 x 4 sub-tiles), K slice = 128 bytes = two MFMA steps per sub-tile.  Two slice buffers in LDS (gathered A 16 KiB + W
//   16 KiB each = 64 KiB: two workgroups per CU), 16-byte chunks XOR-swizzled as tiled_gemm.hip's lds_off (conflict-free
//   ds_read_b128), staged through registers one slice ahead, one barrier per slice.  SILU: the 128 weight rows are 64 gate + 64
//   up rows ordered so that sub-tile columns j = 0, 1 of a wave are gate and j = 2, 3 the up rows of the same 32 outputs: 64 output
//   columns per workgroup.  Rows past N are clamped on the load and masked on the store.
#include "common.h"

namespace {

struct MoeGemmParams {
  const char* a;            // [rows][K] 16-bit
  const char* w;            // [E][NW][K] 16-bit, NW = 2 N (SILU) or N
  void* out;                // [P][N]
  const float* topk_w;      // [P] or null
  const int* sorted_ids;
  const int* expert_ids;
  const int* num_post_pad;
  int P, a_div, E, N, NW, K;
};

template <typename T>
__device__ __forceinline__ f32x4_t mma(const u32x4_t& a, const u32x4_t& b, const f32x4_t& c) {
  typedef typename ElemTraits<T>::vec8 vec8;
  return ElemTraits<T>::mfma16(__builtin_bit_cast(vec8, a), __builtin_bit_cast(vec8, b), c);
}

__device__ __forceinline__ float silu_mul(float g, float u) { return g / (1.0f + __expf(-g)) * u; }

// ---- streaming form ---------------------------------------------------------------------------------------------------------

template <typename T, bool SILU>
__global__ __launch_bounds__(256, 2) void moe_stream_kernel(const MoeGemmParams p) {
  constexpr int NF = 2, PD = 4;   // weight fragments per wave, slices in flight: PD x 4 (NF + 1) x 2 registers
  __shared__ __attribute__((aligned(16))) f32x4_t red[4][NF][64];
  const int blk = blockIdx.x;
  if (blk * 16 >= p.num_post_pad[0]) return;   // workgroup uniform, before any barrier
  const int e = p.expert_ids[blk];
  if ((unsigned)e >= (unsigned)p.E) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * (SILU ? 16 : 32);
  const int Kb = p.K * 2;
  const int KS = (Kb + 127) >> 7;     // 128-byte slices, the last one possibly half
  const int nsw = (KS - w + 3) / 4;   // this wave's slices: w, w + 4, ... (0 when KS <= w)

  const int pair = p.sorted_ids[blk * 16 + a];
  const bool live = (unsigned)pair < (unsigned)p.P;   // a padding row reads row 0 and contributes zeros
  const char* xrow = p.a + (int64_t)(live ? pair / p.a_div : 0) * Kb + 32 * g;
  const char* wrow[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int row = SILU ? f * p.N + n0 + a : n0 + 16 * f + a;   // SILU: gate row n, up row I + n (N == I)
    wrow[f] = p.w + ((int64_t)e * p.NW + row) * Kb + 32 * g;
  }

  u32x4_t wreg[PD][NF][2], xreg[PD][2];
  auto issue = [&](int slot, int i) __attribute__((always_inline)) {
    if (i >= nsw) return;   // wave uniform; the slot is never computed
    const int off = (w + 4 * i) * 128;
    // false only for lanes g >= 2 of a half slice (Kb - off == 64): they read what lanes g - 2 read and contribute zeros
    const bool in = off + 32 * g < Kb;
    const int o = in ? off : off - 64;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32x4_t v = __builtin_nontemporal_load((const u32x4_t*)(wrow[f] + o + 16 * h));
        wreg[slot][f][h] = in ? v : u32x4_t{0u, 0u, 0u, 0u};
      }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4_t v = *(const u32x4_t*)(xrow + o + 16 * h);
      xreg[slot][h] = live ? v : u32x4_t{0u, 0u, 0u, 0u};
    }
  };

  f32x4_t acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < PD; ++j) issue(j, j);
  for (int i0 = 0; i0 < nsw; i0 += PD) {
#pragma unroll
    for (int jj = 0; jj < PD; ++jj) {
      if (i0 + jj < nsw) {   // wave uniform
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int f = 0; f < NF; ++f) acc[f] = mma<T>(xreg[jj][h], wreg[jj][f][h], acc[f]);
        issue(jj, i0 + jj + PD);
      }
    }
  }

  // the four waves' partial sums, added in wave order; wave w finishes row 4 g + w of every lane's four
#pragma unroll
  for (int f = 0; f < NF; ++f) red[w][f][lane] = acc[f];
  __syncthreads();
  const int pr = p.sorted_ids[blk * 16 + 4 * g + w];
  if ((unsigned)pr >= (unsigned)p.P) return;
  float s[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    s[f] = ((const float*)&red[0][f][lane])[w];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) s[f] += ((const float*)&red[ww][f][lane])[w];
  }
  const float rw = p.topk_w ? p.topk_w[pr] : 1.0f;
  T* orow = (T*)p.out + (int64_t)pr * p.N + n0 + a;
  if constexpr (SILU) {
    orow[0] = (T)silu_mul(s[0] * rw, s[1] * rw);
  } else {
#pragma unroll
    for (int f = 0; f < NF; ++f) orow[16 * f] = (T)(s[f] * rw);
  }
}

// ---- tile form --------------------------------------------------------------------------------------------------------------

constexpr int BT = 128;                      // tile edge and bytes of K per slice
constexpr int OPERAND_BYTES = BT * BT;       // 16 KiB per operand per buffer
constexpr int BUF_BYTES = 2 * OPERAND_BYTES;
constexpr int TILE_SMEM = 2 * BUF_BYTES;     // 64 KiB: two workgroups per CU

// byte offset of 16-byte chunk c (0..7) of row r in a [128][128 B] swizzled image (tiled_gemm.hip's lds_off)
__device__ __forceinline__ int sw_off(int r, int c) { return r * BT + ((c ^ ((r >> 1) & 7)) << 4); }

// Row of W[e] behind row r of the workgroup's weight tile.  SILU: r = 64 (wave column) + 16 j + a, j = 0, 1: gate rows of output
// columns n0 + 32 (wave column) + 16 j + a, j = 2, 3: the up rows of the same columns.  Past N: clamped (masked on the store).
template <bool SILU>
__device__ __forceinline__ int tile_wrow(int r, int n0, int N) {
  if constexpr (!SILU) return min(n0 + r, N - 1);
  const int col = n0 + (r >> 6) * 32 + ((r >> 4) & 1) * 16 + (r & 15);
  return ((r >> 5) & 1) * N + min(col, N - 1);
}

template <typename T, bool SILU>
__global__ __launch_bounds__(256, 2) void moe_tile_kernel(const MoeGemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int blk = blockIdx.x;
  if (blk * BT >= p.num_post_pad[0]) return;   // workgroup uniform, before any barrier
  const int e = p.expert_ids[blk];
  if ((unsigned)e >= (unsigned)p.E) return;
  const int n0 = blockIdx.y * (SILU ? 64 : 128);
  const int Kb = p.K * 2;
  const int KS = (Kb + 127) >> 7;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
  const int a = lane & 15, g = lane >> 4;

  // staging: thread loads 16-byte chunk (tid & 7) of rows (tid >> 3) + 32 i of both operands
  const int ld_c = tid & 7, ld_r = tid >> 3;
  const char* xg[4];
  const char* wg[4];
  bool live[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pair = p.sorted_ids[blk * BT + ld_r + 32 * i];
    live[i] = (unsigned)pair < (unsigned)p.P;   // a padding row reads row 0 and stages zeros
    xg[i] = p.a + (int64_t)(live[i] ? pair / p.a_div : 0) * Kb + ld_c * 16;
    wg[i] = p.w + ((int64_t)e * p.NW + tile_wrow<SILU>(ld_r + 32 * i, n0, p.N)) * Kb + ld_c * 16;
  }
  u32x4_t xr[4], wr[4];
  auto gload = [&](int ks) __attribute__((always_inline)) {
    const int off = ks * BT;
    // false only for chunks 4..7 of a half slice (Kb - off == 64): read chunks 0..3 again, stage zeros for the weights
    const bool in = off + ld_c * 16 < Kb;
    const int o = in ? off : off - 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u32x4_t x = *(const u32x4_t*)(xg[i] + o);
      xr[i] = live[i] ? x : u32x4_t{0u, 0u, 0u, 0u};
      const u32x4_t v = *(const u32x4_t*)(wg[i] + o);
      wr[i] = in ? v : u32x4_t{0u, 0u, 0u, 0u};
    }
  };
  auto lstore = [&](int buf) __attribute__((always_inline)) {
    char* xa = smem + buf * BUF_BYTES;
    char* wa = xa + OPERAND_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(u32x4_t*)(xa + sw_off(ld_r + 32 * i, ld_c)) = xr[i];
      *(u32x4_t*)(wa + sw_off(ld_r + 32 * i, ld_c)) = wr[i];
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  gload(0);
  lstore(0);
  __syncthreads();
  for (int ks = 0; ks < KS; ++ks) {
    const int buf = ks & 1;
    // the next slice, unconditionally (the last iteration fetches its own slice again into the idle buffer): a branch here
    // splits the loop body and lets the compiler sink the MFMAs below the wait for these loads
    gload(min(ks + 1, KS - 1));
    __builtin_amdgcn_sched_barrier(0);   // issued before the MFMAs, so the whole slice covers their latency
    const char* xa = smem + buf * BUF_BYTES;
    const char* wa = xa + OPERAND_BYTES;
    u32x4_t af[4][2], bf[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        af[i][h] = *(const u32x4_t*)(xa + sw_off(wm + 16 * i + a, 4 * h + g));
        bf[i][h] = *(const u32x4_t*)(wa + sw_off(wn + 16 * i + a, 4 * h + g));
      }
    // step-major: 16 independent MFMAs between two that touch the same accumulator
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mma<T>(af[i][h], bf[j][h], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);   // the stores (and the wait for the global loads) stay behind the MFMAs
    lstore(buf ^ 1);   // the buffer the slice before was read from: every wave is past the last barrier
    __syncthreads();
  }

  // acc[i][j][r] -> pair of row wm + 16 i + 4 g + r, weight-tile row wn + 16 j + a
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int pr = p.sorted_ids[blk * BT + wm + 16 * i + 4 * g + r];
      if ((unsigned)pr >= (unsigned)p.P) continue;
      const float rw = p.topk_w ? p.topk_w[pr] : 1.0f;
      T* orow = (T*)p.out + (int64_t)pr * p.N;
      if constexpr (SILU) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = n0 + (wn >> 1) + 16 * j + a;   // N % 16 == 0: a 16-column unit is in or out as a whole
          if (n < p.N) orow[n] = (T)silu_mul(acc[i][j][r] * rw, acc[i][j + 2][r] * rw);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = n0 + wn + 16 * j + a;
          if (n < p.N) orow[n] = (T)(acc[i][j][r] * rw);
        }
      }
    }
}

// ---- moe_sum_reduce ---------------------------------------------------------------------------------------------------------

// out[t] = T( scale * sum_j y[t][j] ), f32, j ascending; with ids, a j whose id is outside [0, E) is skipped and its row never read
// (GEMM 2 never wrote it).  One thread per 8 columns.
template <typename T>
__global__ __launch_bounds__(256) void moe_sum_reduce_kernel(const T* __restrict__ y, T* __restrict__ out, const int* __restrict__ ids,
                                                             int tokens, int topk, int H, int E, float scale) {
  const int hv = H / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)tokens * hv) return;
  const int t = (int)(idx / hv), c = (int)(idx - (int64_t)t * hv) * 8;
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.f;
  for (int j = 0; j < topk; ++j) {
    if (ids && (unsigned)ids[(int64_t)t * topk + j] >= (unsigned)E) continue;
    const u32x4_t raw = *(const u32x4_t*)(y + ((int64_t)t * topk + j) * H + c);
    const typename ElemTraits<T>::vec8 v = __builtin_bit_cast(typename ElemTraits<T>::vec8, raw);
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] += (float)v[k];
  }
  typename ElemTraits<T>::vec8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = (T)(s[k] * scale);
  *(u32x4_t*)(out + (int64_t)t * H + c) = __builtin_bit_cast(u32x4_t, o);
}

// ---- host -------------------------------------------------------------------------------------------------------------------

// Pairs per expert (P / E) up to which the streaming form runs: the largest P / E of tools/bench_moe.py's sweep at which it beats
// the tile form on all three layers (profiles/moe_sweep.csv, stream_us against tile_us: x0.87 DeepSeek-V3 T = 128 at P / E = 4,
// x0.89 Qwen3-30B-A3B T = 128 and x0.63 Mixtral T = 32 at P / E = 8; at 16 the DeepSeek row T = 512 is x1.28 and every row above
// loses: a second 16-pair block reads its expert's weights a second time, a 128-pair block reads them once).
constexpr int kStreamMaxPairsPerExpert = 8;

template <typename T, bool SILU>
int moe_launch(const MoeGemmParams& p, int block_size, int64_t blocks, hipStream_t st) {
  if (block_size == 16) {
    hipLaunchKernelGGL((moe_stream_kernel<T, SILU>), dim3((unsigned)blocks, p.N / (SILU ? 16 : 32)), dim3(256), 0, st, p);
  } else {
    static bool attr_set = false;
    if (!attr_set) {
      (void)hipFuncSetAttribute((const void*)moe_tile_kernel<T, SILU>, hipFuncAttributeMaxDynamicSharedMemorySize, TILE_SMEM);
      attr_set = true;
    }
    hipLaunchKernelGGL((moe_tile_kernel<T, SILU>), dim3((unsigned)blocks, cdiv_i(p.N, SILU ? 64 : 128)), dim3(256), TILE_SMEM, st, p);
  }
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

}  // namespace

// Which form fused_experts runs for P pairs over E experts (host logic only): 0 = streaming (block_size 16), 1 = tile (128).
extern "C" int sgl_mi355_moe_gemm_form(int64_t num_pairs, int num_experts, int N, int K) {
  (void)N;
  (void)K;
  return num_pairs <= (int64_t)kStreamMaxPairsPerExpert * (num_experts > 0 ? num_experts : 1) ? 0 : 1;
}

extern "C" int sgl_mi355_moe_grouped_gemm(const void* a, const void* w, void* out, const float* topk_weights,
                                          const int* sorted_token_ids, const int* experts_ids, const int* num_tokens_post_pad,
                                          int64_t num_pairs, int a_rows_div, int num_experts, int N, int K, int block_size,
                                          int epilogue, int dtype, void* stream) {
  SGL_CHECK(num_pairs >= 0 && num_experts > 0 && N > 0 && K > 0 && a_rows_div > 0,
            "moe_grouped_gemm: bad shape (pairs=%lld experts=%d N=%d K=%d rows_div=%d)", (long long)num_pairs, num_experts, N, K,
            a_rows_div);
  SGL_CHECK(K % 32 == 0 && N % 32 == 0, "moe_grouped_gemm: N=%d and K=%d (hidden and intermediate size) must be multiples of 32", N, K);
  SGL_CHECK(block_size == 16 || block_size == 128, "moe_grouped_gemm: block_size=%d is neither 16 (streaming form) nor 128 (tile form)",
            block_size);
  SGL_CHECK(epilogue == 0 || epilogue == 1, "moe_grouped_gemm: epilogue=%d is neither 0 (router weight) nor 1 (SiluAndMul)", epilogue);
  SGL_CHECK(dtype == SGL_BF16 || dtype == SGL_F16, "moe_grouped_gemm: dtype must be bf16 or f16 (quantised experts are not served)");
  if (num_pairs == 0) return SGL_MI355_OK;
  SGL_CHECK(a && w && out && sorted_token_ids && experts_ids && num_tokens_post_pad, "moe_grouped_gemm: null pointer");
  SGL_CHECK(((uintptr_t)a % 16) == 0 && ((uintptr_t)w % 16) == 0, "moe_grouped_gemm: a and w must be 16-byte aligned");
  const int64_t active = num_pairs < num_experts ? num_pairs : num_experts;
  const int64_t blocks = (num_pairs + active * (block_size - 1) + block_size - 1) / block_size;
  SGL_CHECK(num_pairs + active * (block_size - 1) < (1ll << 31) && N / 16 <= 65535 && K < (1 << 29),
            "moe_grouped_gemm: grid too large (pairs=%lld N=%d K=%d)", (long long)num_pairs, N, K);
  MoeGemmParams p;
  p.a = (const char*)a; p.w = (const char*)w; p.out = out; p.topk_w = topk_weights;
  p.sorted_ids = sorted_token_ids; p.expert_ids = experts_ids; p.num_post_pad = num_tokens_post_pad;
  p.P = (int)num_pairs; p.a_div = a_rows_div; p.E = num_experts; p.N = N; p.NW = epilogue == 1 ? 2 * N : N; p.K = K;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SGL_BF16)
    return epilogue == 1 ? moe_launch<__bf16, true>(p, block_size, blocks, st) : moe_launch<__bf16, false>(p, block_size, blocks, st);
  return epilogue == 1 ? moe_launch<_Float16, true>(p, block_size, blocks, st) : moe_launch<_Float16, false>(p, block_size, blocks, st);
}

extern "C" int sgl_mi355_moe_sum_reduce(const void* y, void* out, const int* topk_ids, int num_tokens, int topk, int hidden,
                                        int num_experts, float routed_scaling_factor, int dtype, void* stream) {
  SGL_CHECK(num_tokens >= 0 && topk > 0 && hidden > 0, "moe_sum_reduce: bad shape (tokens=%d topk=%d hidden=%d)", num_tokens, topk, hidden);
  SGL_CHECK(hidden % 8 == 0, "moe_sum_reduce: hidden=%d must be a multiple of 8", hidden);
  SGL_CHECK(dtype == SGL_BF16 || dtype == SGL_F16, "moe_sum_reduce: dtype must be bf16 or f16");
  if (num_tokens == 0) return SGL_MI355_OK;
  SGL_CHECK(y && out, "moe_sum_reduce: null pointer");
  SGL_CHECK(((uintptr_t)y % 16) == 0 && ((uintptr_t)out % 16) == 0, "moe_sum_reduce: y and out must be 16-byte aligned");
  const int64_t threads = (int64_t)num_tokens * (hidden / 8);
  SGL_CHECK((threads + 255) / 256 < (1ll << 31), "moe_sum_reduce: grid too large");
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SGL_BF16)
    hipLaunchKernelGGL(moe_sum_reduce_kernel<__bf16>, grid, block, 0, st, (const __bf16*)y, (__bf16*)out, topk_ids, num_tokens, topk,
                       hidden, num_experts, routed_scaling_factor);
  else
    hipLaunchKernelGGL(moe_sum_reduce_kernel<_Float16>, grid, block, 0, st, (const _Float16*)y, (_Float16*)out, topk_ids, num_tokens,
                       topk, hidden, num_experts, routed_scaling_factor);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}
