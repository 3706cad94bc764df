// Fused int4 AWQ dequant + GEMM for M > 64:  y[m][n] = sum_k x[m][k] * W[k][n] (+ bias), W[k][n] EXACTLY awq_dequantize's value.
//
// Replaces, for 64 < M, the awq_unpack_nk + tiled-GEMM pair AWQLinearMethod.apply used (the reference's awq_dequantize +
// torch.matmul, python/sglang/srt/layers/quantization/awq.py:401-418): that pair reads K N / 2 bytes, writes 2 K N and reads them
// back on every call; this kernel reads the int4 image once per row tile and nothing else of W ever exists in memory.
//
// The M dimension is tiled (awq.hip's kernel is X-stationary: all of X in registers, which ends at 64 rows):
//   * workgroup tile 128 rows x 128 columns, 4 waves, two workgroups per CU; wave w owns all 128 rows and column units 2 w, 2 w + 1
//     (a unit = 16 columns): 8 x 2 accumulator tiles.  Every dequantised word feeds 8 MFMAs: with the 64 x 64 wave tile first
//     built (4 MFMAs per word) the bf16 dequantisation (~20 VALU ops per word) outweighed the MFMAs and bf16 lost to the unfused
//     path at M = 256 on qkv / o_proj.  256-row workgroup tiles were built too and measured slower at every M (fewer, fatter
//     workgroups; same L2 traffic for X), so there is one tile shape.
//   * W never touches LDS.  A (unit, 128-k block) of qpacked is 1 KiB in B-fragment order: one 16-byte buffer load per lane, and
//     word s of lane (a, g), through AwqDequant<T>::run, IS the B operand of k-step s.  PD blocks of packed words + sz words are
//     in flight in registers; loads past the last unit / block are predicated off by an out-of-range offset.
//   * X goes through LDS: a 128 x 128-k slice (32 KiB, rows XOR-swizzled in 16-byte chunks as awq.hip's ximg, so the
//     A-fragment ds_read_b128s are conflict free), double buffered: slice i + 1 is loaded into registers before block i's
//     MFMAs and stored behind them; ONE barrier per k-block.  Rows past M are clamped on the load and zeroed.
//   * per k-step a wave does 8 ds_read_b128 (A) and 2 dequantised words (B) for 16 MFMAs: 8 KiB of LDS reads per 16 x 16 cycles
//     of MFMA issue; eight waves per CU, two per SIMD: 128 B / cycle if the MFMAs ran back to back, what a CU's LDS delivers --
//     the kernel runs at a third of the MFMA rate (X traffic from L2 binds first), so LDS is a third used.
//   * split-K over grid.y in whole k-blocks for few-tile shapes: raw f32 partial sums [kranges][M][N], finished by
//     awq_slab_reduce_kernel (bias there); a single range stores T with the bias in the epilogue.
#include "common.h"
#include "awq_dequant.h"

namespace {

struct AwqTiledParams {
  const char* x;            // [M][K] T
  int64_t x_stride;         // elements
  const uint32_t* qpacked;  // [N/16][KB][64][4]
  const uint32_t* sz;       // [K/G][N]
  void* y;
  int64_t y_stride;
  const void* bias;
  float* slabs;   // [kranges][M][N] (null: one k-range, T outputs)
  int M, N, G, KB;
  int mtiles;     // row tiles (blockIdx.x = row tile + mtiles * column tile: the row tiles of one W column
                  // tile run side by side and share its bytes in L2)
  int bpr;        // k-blocks per k-range
  int stream_w;   // one row tile: every W byte is read once (nt)
};

// k-blocks of W in flight per wave.  Two measured latency bound wherever W comes from HBM (one row tile: 3 - 5 us per k-block
// against 0.85 us of MFMA issue); four with more than one sz word per unit and block spilled in the first build, so two stay there.
constexpr int awq_tiled_pd(int sg) { return sg == 1 ? 4 : 2; }
constexpr int kTiledMinBpr = 3;  // shortest k-range, in k-blocks

template <typename T, int SG>
__global__ __launch_bounds__(256, 2) void awq_tiled_gemm_kernel(const AwqTiledParams p) {
  typedef ElemTraits<T> Tr;
  typedef typename Tr::vec8 vec8;
  constexpr int PD = awq_tiled_pd(SG);
  static_assert(PD % 2 == 0, "the LDS buffer of a block is the parity of its register slot");
  constexpr int BM = 128;
  constexpr int SLICE = BM * 256;  // bytes of one X slice
  constexpr int XI = 8;            // 16-byte chunks per thread and slice (128 x 16 chunks over 256 threads)
  constexpr int RPP = 16;          // rows per staging pass, so row & 15 == lr & 15 in every pass
  extern __shared__ __attribute__((aligned(16))) char xlds[];  // [2][BM][256 B]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = lane & 15, g = lane >> 4;
  const int rt = blockIdx.x % p.mtiles, ct = blockIdx.x / p.mtiles;
  const int kr = blockIdx.y;
  const int b0 = kr * p.bpr;
  const int nb = min(p.bpr, p.KB - b0);  // k-blocks of this range (>= 1)
  const int row0 = rt * BM;
  const int ntiles = p.N / 16;

  // ---- X: global -> registers -> swizzled LDS slice ----
  const int lc = tid & 15, lr = tid >> 4;  // 16-byte chunk lc of rows lr + RPP i
  u32x4_t xr[XI];
  auto load_x = [&](int b) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int m = row0 + lr + RPP * i;
      const u32x4_t v = *(const u32x4_t*)((const T*)p.x + (int64_t)min(m, p.M - 1) * p.x_stride + 128 * b + 8 * lc);
      xr[i] = m < p.M ? v : u32x4_t{0u, 0u, 0u, 0u};
    }
  };
  auto store_x = [&](int buf) __attribute__((always_inline)) {
    char* xb = xlds + buf * SLICE + (((lc ^ lr) & 15) << 4);
#pragma unroll
    for (int i = 0; i < XI; ++i) *(u32x4_t*)(xb + (lr + RPP * i) * 256) = xr[i];
  };

  // ---- W: packed words + sz words of PD k-blocks in registers ----
  const int64_t wbytes64 = (int64_t)ntiles * p.KB * 1024;
  const auto wrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.qpacked, 0, (unsigned)min(wbytes64, (int64_t)0xFFFFFFF0ll), 0x00020000);
  u32x4_t wreg[PD][2];
  uint32_t szreg[PD][2][SG];
  auto issue = [&](int slot, int i) __attribute__((always_inline)) {
    const bool bok = i < nb;
    const int b = b0 + (bok ? i : 0);  // scale loads stay in range; weight loads past the end are predicated off
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = 8 * ct + 2 * w + u;
      const int tc = min(t, ntiles - 1);
      const unsigned off = (bok && t < ntiles) ? (unsigned)((((int64_t)t * p.KB + b) * 64 + lane) * 16) : 0xFFFFFFF0u;
      if (p.stream_w) wreg[slot][u] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, off, 0, 2));
      else wreg[slot][u] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, off, 0, 0));
#pragma unroll
      for (int q = 0; q < SG; ++q) {
        const int grp = (128 * b + (128 / SG) * q) / p.G;
        szreg[slot][u][q] = p.sz[(int64_t)grp * p.N + 16 * tc + a];
      }
    }
  };

  f32x4_t acc[8][2];  // [row tile][column unit]: rows 16 mt + 4 g + r, column 16 (8 ct + 2 w + u) + a
#pragma unroll
  for (int mt = 0; mt < 8; ++mt)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[mt][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int buf, int slot) __attribute__((always_inline)) {
    const char* xb = xlds + buf * SLICE + a * 256;
    AwqDequant<T> dq[2];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      vec8 af[8];
#pragma unroll
      for (int mt = 0; mt < 8; ++mt)
        af[mt] = __builtin_bit_cast(vec8, *(const u32x4_t*)(xb + mt * 16 * 256 + ((((4 * s + g) ^ a) & 15) << 4)));
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (s % (4 / SG) == 0) dq[u].setup(szreg[slot][u][(s * SG) / 4]);
        const vec8 wf = dq[u].run(wreg[slot][u][s]);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) acc[mt][u] = Tr::mfma16(af[mt], wf, acc[mt][u]);
      }
    }
  };

#pragma unroll
  for (int j = 0; j < PD; ++j) issue(j, j);
  load_x(b0);
  store_x(0);
  __syncthreads();
  for (int i0 = 0; i0 < nb; i0 += PD) {
#pragma unroll
    for (int jj = 0; jj < PD; ++jj) {
      const int i = i0 + jj;
      if (i < nb) {  // uniform over the workgroup
        const bool more = i + 1 < nb;
        if (more) load_x(b0 + i + 1);  // in flight under this block's MFMAs
        compute(jj & 1, jj);
        issue(jj, i + PD);
        if (more) store_x((jj + 1) & 1);  // the buffer block i - 1 was read from: every wave is past the last barrier
        __syncthreads();
      }
    }
  }

  // ---- epilogue: 16 lanes write 16 consecutive columns of a row ----
  const bool has_bias = p.bias != nullptr && p.slabs == nullptr;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int t = 8 * ct + 2 * w + u;
    if (t >= ntiles) continue;
    const int n = 16 * t + a;
    const float bv = has_bias ? (float)((const T*)p.bias)[n] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 8; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = row0 + 16 * mt + 4 * g + r;
        if (m >= p.M) continue;
        if (p.slabs != nullptr) p.slabs[((int64_t)kr * p.M + m) * p.N + n] = acc[mt][u][r];
        else ((T*)p.y)[(int64_t)m * p.y_stride + n] = (T)(acc[mt][u][r] + bv);
      }
  }
}

template <typename T, int SG>
int awq_tiled_launch(AwqTiledParams p, int kranges, hipStream_t st) {
  constexpr int smem = 2 * 128 * 256;  // 64 KiB
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)awq_tiled_gemm_kernel<T, SG>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    attr_set = true;
  }
  p.mtiles = (p.M + 127) / 128;
  p.stream_w = p.mtiles == 1;
  hipLaunchKernelGGL((awq_tiled_gemm_kernel<T, SG>), dim3(p.mtiles * ((p.N + 127) / 128), kranges), dim3(256), smem, st, p);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

template <typename T>
int awq_tiled_dispatch(const AwqTiledParams& p, int kranges, hipStream_t st) {
  const int sg = p.G % 128 == 0 ? 1 : 128 / p.G;
  if (sg == 1) return awq_tiled_launch<T, 1>(p, kranges, st);
  if (sg == 2) return awq_tiled_launch<T, 2>(p, kranges, st);
  return awq_tiled_launch<T, 4>(p, kranges, st);
}

// k-blocks per k-range, for launches with fewer tiles than workgroup slots: the range length that minimises a two-term estimate of the time,
//   rounds of resident workgroups x blocks per range x kBlockUs  +  ranges x (one f32 [M, N] slab written and read back at ~3 TB/s),
// plus the reduce launch.  (The starting rule -- one workgroup per CU, whatever the slabs cost -- lost to the unfused path at
// M = 256 on o_proj / down_proj: ten slabs of 256 x 3584 floats are 24 us of traffic around 4 us of MFMAs.  The constants are
// estimates from that sweep, not fitted.)
int awq_tiled_bpr(int M, int N, int KB) {
  const int64_t tiles = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
  const int cus = 2 * awq_cus();   // two 128-row workgroups per CU
  if (tiles >= cus) return KB;
  constexpr double kBlockUs = 1.5, kReduceUs = 4.0;
  const double slab_us = (double)M * N * 8.0 / 3.0e6;
  int best = KB;
  double best_us = KB * kBlockUs;
  for (int bpr = KB - 1; bpr >= kTiledMinBpr; --bpr) {
    const int kr = (KB + bpr - 1) / bpr;
    const double us = (double)((tiles * kr + cus - 1) / cus) * bpr * kBlockUs + kr * slab_us + kReduceUs;
    if (us < best_us) { best = bpr; best_us = us; }
  }
  return best;
}

}  // namespace

// Split-K ranges of sgl_mi355_awq_gemm_tiled (f32 [M, N] slabs of workspace it wants; 1: none).
extern "C" int sgl_mi355_awq_gemm_tiled_kranges(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K < 128) return 1;
  const int bpr = awq_tiled_bpr(M, N, K / 128);
  return (K / 128 + bpr - 1) / bpr;
}

// y [M, N] = x [M, K] . dequant(qpacked, sz) (+ bias) for M > 64; arguments as sgl_mi355_awq_gemm; workspace: kranges x M x N floats
// when sgl_mi355_awq_gemm_tiled_kranges(M, N, K) > 1.  No allocation, no synchronisation: capturable in a HIP graph.
extern "C" int sgl_mi355_awq_gemm_tiled(const void* x, int64_t x_stride_elems, const void* qpacked, const void* sz, void* y,
                                        int64_t y_stride_elems, const void* bias, int M, int N, int K, int group_size, int dtype,
                                        float* workspace, int64_t workspace_floats, void* stream) {
  SGL_CHECK(M > 64 && N > 0 && K > 0 && group_size > 0, "awq_gemm_tiled: bad shape (M=%d must exceed 64: sgl_mi355_awq_gemm serves the rest)", M);
  SGL_CHECK(x && qpacked && sz && y, "awq_gemm_tiled: null pointer");
  SGL_CHECK(K % 128 == 0 && N % 16 == 0, "awq_gemm_tiled: needs K %% 128 == 0 and N %% 16 == 0 (K=%d N=%d)", K, N);
  SGL_CHECK(K % group_size == 0 && (group_size % 128 == 0 || group_size == 64 || group_size == 32),
            "awq_gemm_tiled: group_size=%d must be 32, 64 or a multiple of 128 dividing K", group_size);
  SGL_CHECK(dtype == SGL_BF16 || dtype == SGL_F16, "awq_gemm_tiled: dtype must be bf16 or f16");
  SGL_CHECK(x_stride_elems % 8 == 0 && x_stride_elems >= K && ((uintptr_t)x % 16) == 0 && ((uintptr_t)qpacked % 16) == 0,
            "awq_gemm_tiled: x rows and qpacked must be 16-byte aligned");
  SGL_CHECK(y_stride_elems >= N, "awq_gemm_tiled: y row stride %lld below N=%d", (long long)y_stride_elems, N);
  SGL_CHECK((int64_t)K * N / 2 < 0xFFFFFFF0ll, "awq_gemm_tiled: weight larger than 4 GiB");
  const int KB = K / 128;
  AwqTiledParams p;
  p.bpr = awq_tiled_bpr(M, N, KB);
  const int kranges = (KB + p.bpr - 1) / p.bpr;
  p.x = (const char*)x; p.x_stride = x_stride_elems;
  p.qpacked = (const uint32_t*)qpacked; p.sz = (const uint32_t*)sz;
  p.y = y; p.y_stride = y_stride_elems; p.bias = bias; p.slabs = nullptr;
  p.M = M; p.N = N; p.G = group_size; p.KB = KB;
  if (kranges > 1) {
    SGL_CHECK(workspace != nullptr && workspace_floats >= (int64_t)kranges * M * N,
              "awq_gemm_tiled: M=%d N=%d K=%d needs a workspace of %d x M x N floats", M, N, K, kranges);
    p.slabs = workspace;
  }
  hipStream_t st = (hipStream_t)stream;
  const int rc = dtype == SGL_BF16 ? awq_tiled_dispatch<__bf16>(p, kranges, st) : awq_tiled_dispatch<_Float16>(p, kranges, st);
  if (rc != SGL_MI355_OK || kranges == 1) return rc;
  const int64_t items = (int64_t)M * (N / 4);
  const unsigned blocks = (unsigned)((items + 255) / 256 > 2048 ? 2048 : (items + 255) / 256);
  if (dtype == SGL_BF16)
    hipLaunchKernelGGL((awq_slab_reduce_kernel<__bf16>), dim3(blocks), dim3(256), 0, st, p.slabs, kranges, (const __bf16*)bias,
                       (__bf16*)y, y_stride_elems, M, N);
  else
    hipLaunchKernelGGL((awq_slab_reduce_kernel<_Float16>), dim3(blocks), dim3(256), 0, st, p.slabs, kranges, (const _Float16*)bias,
                       (_Float16*)y, y_stride_elems, M, N);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}
