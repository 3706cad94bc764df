// Block-scaled fp8 GEMM (DeepSeek-V3 / Qwen3-FP8 style checkpoints: one f32 weight scale per 128 x 128 block, one activation
// scale per token and 128-wide K group):
//
//   Y[m][n] = sum_kb ( sum_{k in block kb} X[m][k] W[n][k] ) * sx[m][kb] * sw[n / 128][kb]  (+ bias[n])
//
// Replaces fp8_blockwise_scaled_mm (sgl-kernel/csrc/gemm/fp8_blockwise_gemm_kernel.cu:345-383: CUTLASS sm90 / sm100 / sm120
// block-scaled kernels).  X [M, K] and W [N, K] e4m3fn row-major, f32 accumulation, one round-to-nearest-even conversion to
// bf16 / f16 at the end.  K % 128 == 0, N % 16 == 0 (a partial last 128-column block has its own scale row), any M >= 1.
// No workspace, no allocation, no host synchronisation: capturable in a HIP graph.
//
// The scale changes every 128 elements of K, so it cannot wait for an epilogue.  v_mfma_scale_f32_16x16x128_f8f6f4 consumes
// exactly one scale block of K per instruction, so a scale block is ONE MFMA per 16 x 16 output sub-tile, and both forms below
// share one inner step (the "block step"):
//
//   t   = mfma_scale_16x16x128(a_frags, b_frags, C = 0)      unit E8M0 scales: the raw block sum, exact in f32 for fp8 inputs
//   acc += t * s,   s[r] = sx[row_r][kb] * sw                 4 v_mul per 16-row sub-tile and block, 4 v_fma per MFMA
//
// In the 16 x 16 C layout lane (a = lane & 15, g = lane >> 4) holds column a, rows 4 g .. 4 g + 3: four sx values per row
// sub-tile; a wave's columns lie inside one 128-column block, so sw is wave uniform (a scalar load, one value per K block).
// The FMAs of one MFMA's result are issued behind the NEXT row of MFMAs (the last row of block kb behind the first MFMAs of block
// kb + 1), so the vector port works under the matrix pipe, not after it.
//
// Tile form (M > 64): 128 x 128 outputs per 256-thread workgroup, 4 waves of 64 x 64 (4 x 4 sub-tiles), K slice = 128 bytes =
//   one scale block; two slice buffers in LDS (X 16 KiB + W 16 KiB, 16-byte chunks XOR-swizzled as tiled_gemm.hip's lds_off:
//   conflict-free ds_read_b128 fragment reads) with the tile's 128 row scales of the slice beside them (512 B), all staged
//   through registers one slice ahead; one barrier per slice.  Rows / columns past M / N are clamped on the load and masked on
//   the store; the N tail is whole 16-column units.  XCD-aware bijective block remap as tiled_gemm_kernel.
//   Budget: LDS 2 x (32 KiB + 512 B) = 65 KiB per workgroup, two workgroups per CU (130 of 160 KiB).  VGPRs: 64 accumulators
//   + 64 fragments + 32 staging + 16 MFMA results + scales: under the 256 that __launch_bounds__(256, 2) allows (the
//   compiler's figure is in DESIGN.md section 3.3); 8 waves per CU, 2 per SIMD; no scratch.
//
// Streaming form (M <= 64): decode is a weight stream and 128-wide tiles would put N / 128 workgroups on 256 CUs.  A workgroup
//   owns 16 weight rows (grid N / 16); its 4 waves split the K blocks (wave w: blocks w, w + 4, ...).  Lane (a, g) reads bytes
//   32 g .. 32 g + 31 of block kb of weight row a with two non-temporal 16-byte loads -- the wave's pair of loads covers the
//   whole 128-byte aligned run of each of the 16 rows -- straight into the B fragment (both operands come from global memory
//   here, so the lanes take the hardware's own K order); up to four 16-row X fragments come from global memory the same way
//   (X is L2 resident); lane l fetches sx of row l (the four values a lane needs per fragment come back by ds_bpermute, so a
//   block's row scales cost one register) and the scalar sw per block; PD blocks in flight in registers, no barrier in the
//   loop.  One LDS reduction (16 KiB) sums the four waves' accumulators in a fixed order; the epilogue follows.
//   Budget: at most 16 accumulators + 16 results + PD x (8 W + 8 MT X + 2 scales) registers (PD = 4 up to 32 rows, 2 above);
//   114 .. 192 VGPRs by the compiler's count, two workgroups per CU and more; no scratch.
#include "common.h"

namespace {

struct BlockGemmParams {
  const char* x;   // [M][K] e4m3fn
  int64_t x_stride;  // bytes
  const char* w;   // [N][K] e4m3fn
  int64_t w_stride;  // bytes
  void* y;
  int64_t y_stride;  // elements
  const float* sx;   // [M][KB], element strides sx_m / sx_k
  int64_t sx_m, sx_k;
  const float* sw;   // [ceil(N / 128)][KB], element strides sw_n / sw_k
  int64_t sw_n, sw_k;
  const void* bias;
  int M, N, KB;
  int tiles_m, tiles_n;
};

typedef int i32x8_t __attribute__((ext_vector_type(8)));

// raw sum over one 128-element K block of a 16 x 16 sub-tile (unit E8M0 scales, C = 0)
__device__ __forceinline__ f32x4_t block_sum(const u32x4_t& a0, const u32x4_t& a1, const u32x4_t& b0, const u32x4_t& b1) {
  const i32x8_t av = {(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
  const i32x8_t bv = {(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
}

__device__ __forceinline__ void fold(f32x4_t& acc, const f32x4_t& t, const f32x4_t& s) {
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = fmaf(t[r], s[r], acc[r]);
}

constexpr int BT = 128;                     // tile edge and bytes of K per slice
constexpr int OPERAND_BYTES = BT * BT;      // 16 KiB per operand per buffer
constexpr int BUF_BYTES = 2 * OPERAND_BYTES + BT * 4;   // X, W, 128 row scales
constexpr int TILE_SMEM = 2 * BUF_BYTES;    // 66 560 bytes

// byte offset of 16-byte chunk c (0..7) of row r in a [128][128 B] swizzled image (tiled_gemm.hip's lds_off)
__device__ __forceinline__ int sw_off(int r, int c) { return r * BT + ((c ^ ((r >> 1) & 7)) << 4); }

template <typename OutT>
__global__ __launch_bounds__(256, 2) void fp8_block_tile_kernel(const BlockGemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // XCD-aware bijective remap of the linear block id (8 XCDs, round-robin dispatch): the workgroups of one XCD's contiguous
  // range share X row panels in that XCD's L2
  const int nwg = p.tiles_m * p.tiles_n;
  const int bid = blockIdx.x;
  const int q = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
  const int wgid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + bid / 8;
  const int tm = wgid / p.tiles_n, tn = wgid - tm * p.tiles_n;
  const int m0 = tm * BT, n0 = tn * BT;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = (w >> 1) * 64, wn = (w & 1) * 64;
  const int a = lane & 15, g = lane >> 4;

  // staging: thread loads 16-byte chunk (tid & 7) of rows (tid >> 3) + 32 i of both operands; thread t the scale of row t & 127
  const int ld_c = tid & 7, ld_r = tid >> 3;
  const char* xg[4];
  const char* wg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xg[i] = p.x + (int64_t)min(m0 + ld_r + 32 * i, p.M - 1) * p.x_stride + ld_c * 16;
    wg[i] = p.w + (int64_t)min(n0 + ld_r + 32 * i, p.N - 1) * p.w_stride + ld_c * 16;
  }
  const float* sxg = p.sx + (int64_t)min(m0 + (tid & 127), p.M - 1) * p.sx_m;
  const float* swg = p.sw + (int64_t)tn * p.sw_n;   // wave uniform: a scalar load per block
  u32x4_t xr[4], wr[4];
  float sxr, swn;
  auto gload = [&](int kb) __attribute__((always_inline)) {
    const int64_t off = (int64_t)kb * BT;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xr[i] = *(const u32x4_t*)(xg[i] + off);
      wr[i] = *(const u32x4_t*)(wg[i] + off);
    }
    sxr = sxg[(int64_t)kb * p.sx_k];
    swn = swg[(int64_t)kb * p.sw_k];
  };
  auto lstore = [&](int buf) __attribute__((always_inline)) {
    char* xa = smem + buf * BUF_BYTES;
    char* wa = xa + OPERAND_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(u32x4_t*)(xa + sw_off(ld_r + 32 * i, ld_c)) = xr[i];
      *(u32x4_t*)(wa + sw_off(ld_r + 32 * i, ld_c)) = wr[i];
    }
    *(float*)(wa + OPERAND_BYTES + (tid & 127) * 4) = sxr;   // threads t and t + 128 hold the same value: no branch in the loop
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // results and scales of the row of sub-tiles whose FMAs are still owed (0 * 0 the first time round)
  f32x4_t tp[4], sp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) tp[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  gload(0);
  lstore(0);
  float swc = swn;   // sw of the slice being computed
  __syncthreads();
  for (int kb = 0; kb < p.KB; ++kb) {
    const int buf = kb & 1;
    // the next slice, unconditionally (the last iteration fetches its own slice again into the idle buffer): a branch here
    // splits the loop body, and the compiler then sinks the MFMAs below the LDS stores and the wait for these loads
    gload(min(kb + 1, p.KB - 1));
    __builtin_amdgcn_sched_barrier(0);   // issued before the block step, so the whole step covers their latency
    const char* xa = smem + buf * BUF_BYTES;
    const char* wa = xa + OPERAND_BYTES;
    const char* sa = wa + OPERAND_BYTES;
    u32x4_t af[4][2], bf[4][2];
    f32x4_t s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        af[i][h] = *(const u32x4_t*)(xa + sw_off(wm + 16 * i + a, 4 * h + g));
        bf[i][h] = *(const u32x4_t*)(wa + sw_off(wn + 16 * i + a, 4 * h + g));
      }
      s[i] = *(const f32x4_t*)(sa + (wm + 16 * i + 4 * g) * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) s[i][r] *= swc;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4_t t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = block_sum(af[i][0], af[i][1], bf[j][0], bf[j][1]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        fold(acc[(i + 3) & 3][j], tp[j], sp);   // the row before: row 3 of the previous block when i == 0
        tp[j] = t[j];
      }
      sp = s[i];
    }
    __builtin_amdgcn_sched_barrier(0);   // the stores (and the wait for the global loads) stay behind the block step
    lstore(buf ^ 1);   // the buffer slice kb - 1 was read from: every wave is past the last barrier
    swc = swn;
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) fold(acc[3][j], tp[j], sp);

  // epilogue: acc[i][j][r] -> row m0 + wm + 16 i + 4 g + r, column n0 + wn + 16 j + a (16 lanes write 32 consecutive bytes)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn + 16 * j + a;
    if (n >= p.N) continue;   // N % 16 == 0: a 16-column unit is in or out as a whole
    const float bv = p.bias ? (float)((const OutT*)p.bias)[n] : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * i + 4 * g + r;
        if (m < p.M) ((OutT*)p.y)[(int64_t)m * p.y_stride + n] = (OutT)(acc[i][j][r] + bv);
      }
  }
}

// K blocks in flight per wave: PD x (8 MT + 10) registers
constexpr int stream_pd(int mt) { return mt <= 2 ? 4 : 2; }

template <typename OutT, int MT>
__global__ __launch_bounds__(256, 2) void fp8_block_stream_kernel(const BlockGemmParams p) {
  constexpr int PD = stream_pd(MT);
  __shared__ __attribute__((aligned(16))) f32x4_t red[4][MT][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nbw = (p.KB - w + 3) / 4;   // this wave's blocks: w, w + 4, ... (0 when KB <= w)

  const char* wrow = p.w + (int64_t)(n0 + a) * p.w_stride + 32 * g;
  const char* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = p.x + (int64_t)min(16 * mt + a, p.M - 1) * p.x_stride + 32 * g;
  // lane l fetches the scale of row l; the four a lane needs per row fragment come back through ds_bpermute (registers only)
  const float* sxrow = p.sx + (int64_t)min(lane, p.M - 1) * p.sx_m;
  const float* swg = p.sw + (int64_t)(n0 / 128) * p.sw_n;

  u32x4_t wreg[PD][2], xreg[PD][MT][2];
  float sreg[PD], swreg[PD];
  auto issue = [&](int slot, int i) __attribute__((always_inline)) {
    if (i >= nbw) return;   // wave uniform; the slot is never computed
    const int kb = w + 4 * i;
    const int64_t off = (int64_t)kb * 128;
    wreg[slot][0] = __builtin_nontemporal_load((const u32x4_t*)(wrow + off));
    wreg[slot][1] = __builtin_nontemporal_load((const u32x4_t*)(wrow + off + 16));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      xreg[slot][mt][0] = *(const u32x4_t*)(xrow[mt] + off);
      xreg[slot][mt][1] = *(const u32x4_t*)(xrow[mt] + off + 16);
    }
    sreg[slot] = sxrow[(int64_t)kb * p.sx_k];
    swreg[slot] = swg[(int64_t)kb * p.sw_k];
  };

  f32x4_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int j = 0; j < PD; ++j) issue(j, j);
  for (int i0 = 0; i0 < nbw; i0 += PD) {
#pragma unroll
    for (int jj = 0; jj < PD; ++jj) {
      if (i0 + jj < nbw) {   // wave uniform
        f32x4_t t[MT], s[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          t[mt] = block_sum(xreg[jj][mt][0], xreg[jj][mt][1], wreg[jj][0], wreg[jj][1]);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            s[mt][r] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((16 * mt + 4 * g + r) * 4, __builtin_bit_cast(int, sreg[jj]))) * swreg[jj];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) fold(acc[mt], t[mt], s[mt]);
        issue(jj, i0 + jj + PD);
      }
    }
  }

  // the four waves' partial sums, added in wave order by wave mt for row fragment mt
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) red[w][mt][lane] = acc[mt];
  __syncthreads();
  if (w >= MT) return;
  f32x4_t sum = red[0][w][lane];
#pragma unroll
  for (int ww = 1; ww < 4; ++ww) {
    const f32x4_t v = red[ww][w][lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[r] += v[r];
  }
  const int n = n0 + a;
  const float bv = p.bias ? (float)((const OutT*)p.bias)[n] : 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = 16 * w + 4 * g + r;
    if (m < p.M) ((OutT*)p.y)[(int64_t)m * p.y_stride + n] = (OutT)(sum[r] + bv);
  }
}

template <typename OutT>
int tile_launch(BlockGemmParams p, hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)fp8_block_tile_kernel<OutT>, hipFuncAttributeMaxDynamicSharedMemorySize, TILE_SMEM);
    attr_set = true;
  }
  p.tiles_m = (p.M + BT - 1) / BT;
  p.tiles_n = (p.N + BT - 1) / BT;
  hipLaunchKernelGGL((fp8_block_tile_kernel<OutT>), dim3(p.tiles_m * p.tiles_n), dim3(256), TILE_SMEM, st, p);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

template <typename OutT, int MT>
int stream_launch_mt(const BlockGemmParams& p, hipStream_t st) {
  hipLaunchKernelGGL((fp8_block_stream_kernel<OutT, MT>), dim3(p.N / 16), dim3(256), 0, st, p);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

template <typename OutT>
int stream_launch(const BlockGemmParams& p, hipStream_t st) {
  switch ((p.M + 15) / 16) {
    case 1: return stream_launch_mt<OutT, 1>(p, st);
    case 2: return stream_launch_mt<OutT, 2>(p, st);
    case 3: return stream_launch_mt<OutT, 3>(p, st);
    default: return stream_launch_mt<OutT, 4>(p, st);
  }
}

constexpr int kStreamMaxM = 64;

}  // namespace

// Which form sgl_mi355_fp8_blockwise_gemm runs for this shape (host logic only): 0 = streaming (M <= 64), 1 = tile.
extern "C" int sgl_mi355_fp8_blockwise_gemm_form(int M, int N, int K) {
  (void)N;
  (void)K;
  return M <= kStreamMaxM ? 0 : 1;
}

extern "C" int sgl_mi355_fp8_blockwise_gemm(const void* x, int64_t x_stride_b, const void* w, int64_t w_stride_b, void* y,
                                            int64_t y_stride, const float* sx, int64_t sx_stride_m, int64_t sx_stride_k,
                                            const float* sw, int64_t sw_stride_n, int64_t sw_stride_k, const void* bias, int M,
                                            int N, int K, int out_dtype, void* stream) {
  SGL_CHECK(M >= 0 && N > 0 && K > 0, "fp8_blockwise_gemm: bad shape (M=%d N=%d K=%d)", M, N, K);
  SGL_CHECK(K % 128 == 0, "fp8_blockwise_gemm: K=%d must be a multiple of the 128-wide scale block", K);
  SGL_CHECK(N % 16 == 0, "fp8_blockwise_gemm: N=%d must be a multiple of 16", N);
  SGL_CHECK(out_dtype == SGL_BF16 || out_dtype == SGL_F16, "fp8_blockwise_gemm: out_dtype must be bf16 or f16");
  if (M == 0) return SGL_MI355_OK;
  SGL_CHECK(x && w && y && sx && sw, "fp8_blockwise_gemm: null pointer");
  SGL_CHECK(x_stride_b >= K && w_stride_b >= K && x_stride_b % 16 == 0 && w_stride_b % 16 == 0 && ((uintptr_t)x % 16) == 0 &&
                ((uintptr_t)w % 16) == 0,
            "fp8_blockwise_gemm: x and w rows must be 16-byte aligned and at least K bytes apart");
  SGL_CHECK(y_stride >= N, "fp8_blockwise_gemm: y row stride %lld below N=%d", (long long)y_stride, N);
  SGL_CHECK(sx_stride_m >= 0 && sx_stride_k >= 0 && sw_stride_n >= 0 && sw_stride_k >= 0, "fp8_blockwise_gemm: negative scale stride");
  SGL_CHECK((int64_t)((M + 127) / 128) * ((N + 127) / 128) < (1ll << 31), "fp8_blockwise_gemm: grid too large");
  BlockGemmParams p;
  p.x = (const char*)x; p.x_stride = x_stride_b;
  p.w = (const char*)w; p.w_stride = w_stride_b;
  p.y = y; p.y_stride = y_stride;
  p.sx = sx; p.sx_m = sx_stride_m; p.sx_k = sx_stride_k;
  p.sw = sw; p.sw_n = sw_stride_n; p.sw_k = sw_stride_k;
  p.bias = bias;
  p.M = M; p.N = N; p.KB = K / 128;
  p.tiles_m = p.tiles_n = 0;
  hipStream_t st = (hipStream_t)stream;
  if (sgl_mi355_fp8_blockwise_gemm_form(M, N, K) == 0)
    return out_dtype == SGL_BF16 ? stream_launch<__bf16>(p, st) : stream_launch<_Float16>(p, st);
  return out_dtype == SGL_BF16 ? tile_launch<__bf16>(p, st) : tile_launch<_Float16>(p, st);
}
