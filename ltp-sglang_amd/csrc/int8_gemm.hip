// int8 w8a8 GEMM (static per-channel symmetric int8 weights, dynamic per-token symmetric int8 activations: the "quantized.w8a8"
// Llama / Qwen checkpoints):
//
//   Y[m][n] = float( sum_k X[m][k] W[n][k] ) * sa[m] * sb[n]  (+ bias[n])
//
// Replaces int8_scaled_mm (sgl-kernel/csrc/gemm/int8_gemm_kernel.cu:663-730: CUTLASS sm75 / sm80 / sm89 / sm90 int8 kernels).
// X [M, K] and W [N, K] int8 row-major (row strides in bytes, multiples of 16), sa / sb f32, int32 accumulation, one conversion
// to bf16 / f16 at the end.  K % 64 == 0, K < 131072 (K products of magnitude <= 2^14 stay inside int32), N % 16 == 0, any M >= 1.
// No allocation, no host synchronisation: capturable in a HIP graph.
//
// v_mfma_i32_16x16x64_i8 takes 16 bytes of K per lane and operand: lane (a = lane & 15, g = lane >> 4) gives row a of the A
// and of the B fragment.  Which 16 of a step's 64 K positions the hardware pairs with lane group g does not matter as long as A
// and B agree, and they do: both operands of every MFMA below hold THE SAME 16 contiguous bytes of K of their rows.  The C
// layout is the f32 one: lane (a, g) holds column a (weight row), rows 4 g .. 4 g + 3 (token).
//
// The integer sum is exact, so it does not depend on how K is split over waves, workgroups or kernels, and every path ends in ONE
// epilogue function (int8_epilogue: cvt, * sa, * sb, + bias, round; no contraction): the same sum gives the same bits whichever
// form produced it.
//
// Streaming form (M <= 64): decode is a weight stream.  A workgroup owns 16 NT weight rows; its 4 waves split the 128-byte K
//   slices (wave w: slices w, w + 4, ...).  Lane (a, g) reads bytes 32 g .. 32 g + 31 of the slice of weight row a with two
//   non-temporal 16-byte loads (the wave's loads cover whole 128-byte lines) straight into two B fragments, and the same bytes
//   of up to four 16-row X fragments (L2 resident) into the A fragments; PD slices in flight in registers, no barrier in the
//   loop.  K % 128 == 64 leaves a half slice: its lanes g >= 2 read the bytes of lanes g - 2 again and zero their weights.
//   One LDS reduction sums the four waves' int32 accumulators, the epilogue follows.
//   NT = 1 (grid N / 16) except for M > 32 with N / 32 >= 256: there every workgroup re-reads all of X (up to 64 x K bytes) from
//   L2 for 16 K bytes of weights per row fragment -- four times the weight bytes at M = 64 -- and 32 rows halve that while the
//   grid still covers every CU; below that N the idle CUs would cost more than the L2 traffic saves.
//
// Tile form (M > 64): 128 x 128 outputs per 256-thread workgroup, 4 waves of 64 x 64 (4 x 4 sub-tiles), K slice = 128 bytes =
//   two MFMA steps per sub-tile; two slice buffers in LDS (X 16 KiB + W 16 KiB each, 16-byte chunks XOR-swizzled as
//   tiled_gemm.hip's lds_off: conflict-free ds_read_b128), staged through registers one slice ahead, one barrier per slice.
//   Rows / columns past M / N are clamped on the load and masked on the store; a half slice at the end of K stages zeros for the
//   weights' missing chunks.  XCD-aware bijective block remap as tiled_gemm_kernel.
//   Split-K (64 < M <= 512, at most half as many tiles as CUs): grid.y workgroups per tile take contiguous slice ranges and write
//   raw int32 partial tiles to [S][M][N] slabs in the caller's workspace (bytes are bytes: the f32 scratch holds int32 here, so
//   the sum stays exact); int8_splitk_reduce_kernel adds them and runs the epilogue.
#include "common.h"

namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));

struct Int8GemmParams {
  const char* x;     // [M][K] int8
  int64_t x_stride;  // bytes
  const char* w;     // [N][K] int8
  int64_t w_stride;  // bytes
  void* y;
  int64_t y_stride;  // elements
  const float* sa;   // [M]
  const float* sb;   // [N]
  const void* bias;  // [N] of the output type, or null
  int* slabs;        // split-K: [ksplit][M][N] int32 partial sums
  int M, N, K;
  int tiles_m, tiles_n, ksplit;
};

constexpr int kCUs = 256;   // MI355X; the form and split choices are host logic that needs no device

// one 64-byte K step of a 16 x 16 sub-tile
__device__ __forceinline__ i32x4_t mma(const u32x4_t& a, const u32x4_t& b, const i32x4_t& c) {
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4_t, a), __builtin_bit_cast(i32x4_t, b), c, 0, 0, 0);
}

// The one epilogue of every path.  Five separately rounded steps; contraction is off so that no compiler version or call site
// fuses "* sb + bias" into an FMA.
template <typename OutT>
__device__ __forceinline__ OutT int8_epilogue(int acc, float sa, float sb, const OutT* bias, int n) {
#pragma clang fp contract(off)
  float v = (float)acc;
  v = v * sa;
  v = v * sb;
  if (bias) v = v + (float)bias[n];
  return (OutT)v;
}

// ---- streaming form ---------------------------------------------------------------------------------------------------------

// K slices in flight per wave: PD x 8 (NT + MT) registers
constexpr int stream_pd(int mt) { return mt <= 2 ? 4 : 2; }

template <typename OutT, int MT, int NT>
__global__ __launch_bounds__(256, 2) void int8_stream_kernel(const Int8GemmParams p) {
  constexpr int PD = stream_pd(MT);
  __shared__ __attribute__((aligned(16))) i32x4_t red[4][MT * NT][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT);
  const int KS = (p.K + 127) >> 7;       // 128-byte slices, the last one possibly half
  const int nsw = (KS - w + 3) / 4;      // this wave's slices: w, w + 4, ... (0 when KS <= w)

  const char* wrow[NT];
  const char* xrow[MT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wrow[nt] = p.w + (int64_t)min(n0 + 16 * nt + a, p.N - 1) * p.w_stride + 32 * g;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = p.x + (int64_t)min(16 * mt + a, p.M - 1) * p.x_stride + 32 * g;

  u32x4_t wreg[PD][NT][2], xreg[PD][MT][2];
  auto issue = [&](int slot, int i) __attribute__((always_inline)) {
    if (i >= nsw) return;   // wave uniform; the slot is never computed
    const int off = (w + 4 * i) * 128;
    // false only for lanes g >= 2 of a half slice (K - off == 64): they read what lanes g - 2 read and contribute zeros
    const bool in = off + 32 * g < p.K;
    const int o = in ? off : off - 64;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32x4_t v = __builtin_nontemporal_load((const u32x4_t*)(wrow[nt] + o + 16 * h));
        wreg[slot][nt][h] = in ? v : u32x4_t{0u, 0u, 0u, 0u};
      }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int h = 0; h < 2; ++h) xreg[slot][mt][h] = *(const u32x4_t*)(xrow[mt] + o + 16 * h);
  };

  i32x4_t acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = i32x4_t{0, 0, 0, 0};

#pragma unroll
  for (int j = 0; j < PD; ++j) issue(j, j);
  for (int i0 = 0; i0 < nsw; i0 += PD) {
#pragma unroll
    for (int jj = 0; jj < PD; ++jj) {
      if (i0 + jj < nsw) {   // wave uniform
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mma(xreg[jj][mt][h], wreg[jj][nt][h], acc[mt][nt]);
        issue(jj, i0 + jj + PD);
      }
    }
  }

  // the four waves' partial sums; wave w finishes fragments w, w + 4, ...
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) red[w][mt * NT + nt][lane] = acc[mt][nt];
  __syncthreads();
  for (int f = w; f < MT * NT; f += 4) {
    i32x4_t sum = red[0][f][lane];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) sum += red[ww][f][lane];
    const int n = n0 + 16 * (f % NT) + a;
    if (n >= p.N) continue;
    const float sb = p.sb[n];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * (f / NT) + 4 * g + r;
      if (m < p.M) ((OutT*)p.y)[(int64_t)m * p.y_stride + n] = int8_epilogue<OutT>(sum[r], p.sa[m], sb, (const OutT*)p.bias, n);
    }
  }
}

// ---- tile form --------------------------------------------------------------------------------------------------------------

constexpr int BT = 128;                      // tile edge and bytes of K per slice
constexpr int OPERAND_BYTES = BT * BT;       // 16 KiB per operand per buffer
constexpr int BUF_BYTES = 2 * OPERAND_BYTES;
constexpr int TILE_SMEM = 2 * BUF_BYTES;     // 64 KiB: two workgroups per CU

// byte offset of 16-byte chunk c (0..7) of row r in a [128][128 B] swizzled image (tiled_gemm.hip's lds_off)
__device__ __forceinline__ int sw_off(int r, int c) { return r * BT + ((c ^ ((r >> 1) & 7)) << 4); }

template <typename OutT>
__global__ __launch_bounds__(256, 2) void int8_tile_kernel(const Int8GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // XCD-aware bijective remap of the linear tile id (8 XCDs, round-robin dispatch): the workgroups of one XCD's contiguous
  // range share X row panels in that XCD's L2
  const int nwg = p.tiles_m * p.tiles_n;
  const int bid = blockIdx.x;
  const int q = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
  const int wgid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + bid / 8;
  const int tm = wgid / p.tiles_n, tn = wgid - tm * p.tiles_n;
  const int m0 = tm * BT, n0 = tn * BT;
  // this workgroup's slices: [ks0, ks1), never empty (ksplit <= KS)
  const int KS = (p.K + 127) >> 7;
  const int split = blockIdx.y;
  const int ks0 = (int)((int64_t)split * KS / p.ksplit), ks1 = (int)((int64_t)(split + 1) * KS / p.ksplit);

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
  const int a = lane & 15, g = lane >> 4;

  // staging: thread loads 16-byte chunk (tid & 7) of rows (tid >> 3) + 32 i of both operands
  const int ld_c = tid & 7, ld_r = tid >> 3;
  const char* xg[4];
  const char* wg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xg[i] = p.x + (int64_t)min(m0 + ld_r + 32 * i, p.M - 1) * p.x_stride + ld_c * 16;
    wg[i] = p.w + (int64_t)min(n0 + ld_r + 32 * i, p.N - 1) * p.w_stride + ld_c * 16;
  }
  u32x4_t xr[4], wr[4];
  auto gload = [&](int ks) __attribute__((always_inline)) {
    const int off = ks * BT;
    // false only for chunks 4..7 of a half slice (K - off == 64): read chunks 0..3 again, stage zeros for the weights
    const bool in = off + ld_c * 16 < p.K;
    const int o = in ? off : off - 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xr[i] = *(const u32x4_t*)(xg[i] + o);
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

  i32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = i32x4_t{0, 0, 0, 0};

  gload(ks0);
  lstore(0);
  __syncthreads();
  for (int ks = ks0; ks < ks1; ++ks) {
    const int buf = (ks - ks0) & 1;
    // the next slice, unconditionally (the last iteration fetches its own slice again into the idle buffer): a branch here
    // splits the loop body and lets the compiler sink the MFMAs below the wait for these loads
    gload(min(ks + 1, ks1 - 1));
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
        for (int j = 0; j < 4; ++j) acc[i][j] = mma(af[i][h], bf[j][h], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);   // the stores (and the wait for the global loads) stay behind the MFMAs
    lstore(buf ^ 1);   // the buffer the slice before was read from: every wave is past the last barrier
    __syncthreads();
  }

  // acc[i][j][r] -> row m0 + wm + 16 i + 4 g + r, column n0 + wn + 16 j + a
  int* slab = p.slabs ? p.slabs + (int64_t)split * p.M * p.N : nullptr;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn + 16 * j + a;
    if (n >= p.N) continue;   // N % 16 == 0: a 16-column unit is in or out as a whole
    const float sb = p.sb[n];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * i + 4 * g + r;
        if (m >= p.M) continue;
        if (slab) slab[(int64_t)m * p.N + n] = acc[i][j][r];
        else ((OutT*)p.y)[(int64_t)m * p.y_stride + n] = int8_epilogue<OutT>(acc[i][j][r], p.sa[m], sb, (const OutT*)p.bias, n);
      }
  }
}

// sum of the split-K slabs and the epilogue: one thread per four consecutive columns of a row
template <typename OutT>
__global__ __launch_bounds__(256) void int8_splitk_reduce_kernel(const Int8GemmParams p) {
  const int nq = p.N / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.M * nq) return;
  const int m = (int)(idx / nq), n = (int)(idx - (int64_t)m * nq) * 4;
  const int64_t slab = (int64_t)p.M * p.N;
  const int* src = p.slabs + (int64_t)m * p.N + n;
  i32x4_t sum = *(const i32x4_t*)src;
  for (int s = 1; s < p.ksplit; ++s) sum += *(const i32x4_t*)(src + s * slab);
  const float sa = p.sa[m];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    ((OutT*)p.y)[(int64_t)m * p.y_stride + n + r] = int8_epilogue<OutT>(sum[r], sa, p.sb[n + r], (const OutT*)p.bias, n + r);
}

// ---- host -------------------------------------------------------------------------------------------------------------------

constexpr int kStreamMaxM = 64;
constexpr int kSplitMaxM = 512;

// Split-K ranges of the tile form: only where the tiles leave at least half the CUs idle, at least four slices (512 bytes of K)
// per range, at most 8 ranges, and only if the slabs fit the scratch (whose last 512 words belong to another kernel).
int tile_ksplit(int M, int N, int K, int64_t ws_floats) {
  const int64_t tiles = (int64_t)cdiv_i(M, BT) * cdiv_i(N, BT);
  if (M > kSplitMaxM || tiles * 2 > kCUs) return 1;
  int s = (int)(kCUs / tiles);
  if (s > 8) s = 8;
  if (s > cdiv_i(K, BT) / 4) s = cdiv_i(K, BT) / 4;
  while (s > 1 && (int64_t)s * M * N > ws_floats - 512) --s;
  return s > 1 ? s : 1;
}

template <typename OutT>
int tile_launch(Int8GemmParams p, float* ws, int64_t ws_floats, hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)int8_tile_kernel<OutT>, hipFuncAttributeMaxDynamicSharedMemorySize, TILE_SMEM);
    attr_set = true;
  }
  p.tiles_m = cdiv_i(p.M, BT);
  p.tiles_n = cdiv_i(p.N, BT);
  p.ksplit = ws ? tile_ksplit(p.M, p.N, p.K, ws_floats) : 1;
  p.slabs = p.ksplit > 1 ? (int*)ws : nullptr;
  hipLaunchKernelGGL((int8_tile_kernel<OutT>), dim3(p.tiles_m * p.tiles_n, p.ksplit), dim3(256), TILE_SMEM, st, p);
  SGL_HIP_LAUNCH_CHECK();
  if (p.ksplit > 1) {
    const int64_t threads = (int64_t)p.M * (p.N / 4);
    hipLaunchKernelGGL((int8_splitk_reduce_kernel<OutT>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p);
    SGL_HIP_LAUNCH_CHECK();
  }
  return SGL_MI355_OK;
}

template <typename OutT, int MT, int NT>
int stream_launch_mt(const Int8GemmParams& p, hipStream_t st) {
  hipLaunchKernelGGL((int8_stream_kernel<OutT, MT, NT>), dim3(p.N / (16 * NT)), dim3(256), 0, st, p);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

template <typename OutT>
int stream_launch(const Int8GemmParams& p, hipStream_t st) {
  const int mt = cdiv_i(p.M, 16);
  if (mt >= 3 && p.N % 32 == 0 && p.N / 32 >= kCUs)   // 32 weight rows per workgroup (see the head of the file)
    return mt == 3 ? stream_launch_mt<OutT, 3, 2>(p, st) : stream_launch_mt<OutT, 4, 2>(p, st);
  switch (mt) {
    case 1: return stream_launch_mt<OutT, 1, 1>(p, st);
    case 2: return stream_launch_mt<OutT, 2, 1>(p, st);
    case 3: return stream_launch_mt<OutT, 3, 1>(p, st);
    default: return stream_launch_mt<OutT, 4, 1>(p, st);
  }
}

}  // namespace

// Which form sgl_mi355_int8_gemm runs for this shape (host logic only): 0 = streaming (M <= 64), 1 = tile.
extern "C" int sgl_mi355_int8_gemm_form(int M, int N, int K) {
  (void)N;
  (void)K;
  return M <= kStreamMaxM ? 0 : 1;
}

extern "C" int sgl_mi355_int8_gemm(const void* x, int64_t x_stride_b, const void* w, int64_t w_stride_b, void* y, int64_t y_stride,
                                   const float* scales_a, const float* scales_b, const void* bias, int M, int N, int K,
                                   int out_dtype, float* workspace, int64_t workspace_floats, void* stream) {
  SGL_CHECK(M >= 0 && N > 0 && K > 0, "int8_gemm: bad shape (M=%d N=%d K=%d)", M, N, K);
  SGL_CHECK(K % 64 == 0, "int8_gemm: K=%d must be a multiple of 64 (one int8 MFMA step)", K);
  SGL_CHECK(K < 131072, "int8_gemm: K=%d must be below 131072 (int32 accumulation)", K);
  SGL_CHECK(N % 16 == 0, "int8_gemm: N=%d must be a multiple of 16", N);
  SGL_CHECK(out_dtype == SGL_BF16 || out_dtype == SGL_F16, "int8_gemm: out_dtype must be bf16 or f16");
  if (M == 0) return SGL_MI355_OK;
  SGL_CHECK(x && w && y && scales_a && scales_b, "int8_gemm: null pointer");
  SGL_CHECK(x_stride_b >= K && w_stride_b >= K && x_stride_b % 16 == 0 && w_stride_b % 16 == 0 && ((uintptr_t)x % 16) == 0 &&
                ((uintptr_t)w % 16) == 0,
            "int8_gemm: x and w rows must be 16-byte aligned and at least K bytes apart");
  SGL_CHECK(y_stride >= N, "int8_gemm: y row stride %lld below N=%d", (long long)y_stride, N);
  SGL_CHECK(workspace_floats >= 0 && ((uintptr_t)workspace % 16) == 0, "int8_gemm: workspace must be 16-byte aligned");
  SGL_CHECK((int64_t)cdiv_i(M, 128) * cdiv_i(N, 128) < (1ll << 31) && (int64_t)M * N / 1024 < (1ll << 31), "int8_gemm: grid too large");
  Int8GemmParams p;
  p.x = (const char*)x; p.x_stride = x_stride_b;
  p.w = (const char*)w; p.w_stride = w_stride_b;
  p.y = y; p.y_stride = y_stride;
  p.sa = scales_a; p.sb = scales_b; p.bias = bias;
  p.slabs = nullptr;
  p.M = M; p.N = N; p.K = K;
  p.tiles_m = p.tiles_n = 0; p.ksplit = 1;
  hipStream_t st = (hipStream_t)stream;
  if (sgl_mi355_int8_gemm_form(M, N, K) == 0)
    return out_dtype == SGL_BF16 ? stream_launch<__bf16>(p, st) : stream_launch<_Float16>(p, st);
  return out_dtype == SGL_BF16 ? tile_launch<__bf16>(p, workspace, workspace_floats, st)
                               : tile_launch<_Float16>(p, workspace, workspace_floats, st);
}
