// NVFP4 (w4a16) linear: fused fp4 dequant + GEMM with 16-bit activations, and the dense dequantisation.
//
// Replaces what PetitNvFp4LinearMethod.apply reaches through apply_petit_nvfp4_linear
// (python/sglang/srt/layers/quantization/petit.py:238-252, petit_utils.py:78-104): mul_nvfp4_a16 of the petit_kernel wheel,
// which is not part of the reference -- so nothing here is a port.  The product, for ModelOpt NVFP4 checkpoint tensors
// (petit.py:134-224):
//   W[n][k] = e2m1(nibble(n, k)) * float(weight_scale[n][k / 16])
//   y[m][n] = T( f32(sum_k x[m][k] W[n][k]) * weight_scale_2 (+ bias[n]) )        T = bf16 / f16, f32 accumulation
// weight uint8 [N, K/2]: byte j of a row = element 2j in the low nibble, 2j + 1 in the high one; a nibble = sign (bit 3) and an
// index into {0, .5, 1, 1.5, 2, 3, 4, 6}; weight_scale float8_e4m3fn [N, K/16]; weight_scale_2 one f32 (a DEVICE scalar).
// The reference wrapper adds the bias in place to the rounded output (petit_utils.py:101-102: two roundings); this build adds
// it in f32 and ROUNDS ONCE, as every epilogue of gemm_epilogue.h does.
//
// Dequantisation in registers, bit-exact: W[n][k] has at most 2 + 4 significant bits, |W| <= 6 * 448 and >= 2^-10 when non-zero,
// so it is exactly representable (and normal) in f16 and in bf16, and the MFMA operand equals it for every nibble and every
// finite scale byte (subnormal, zero and negative e4m3 bytes included; 0x7F / 0xFF = NaN are outside the contract):
//   f16:  v_cvt_scalef32_pk_f16_fp4 (byte j of the packed word -> elements 2j, 2j + 1 as packed f16) with the scale operand 1.0,
//         then v_pk_mul_f16 by the group scale (e4m3 -> f32 -> f16, both exact; broadcast by op_sel): 8 VALU ops per 8 weights;
//   bf16: v_cvt_scalef32_pk_f32_fp4 (scale 1.0), two v_mul_f32 by the group scale, v_cvt_pk_bf16_f32: 16 ops per 8 weights
//         (every step exact: the f32 product has 6 significant bits).
// The conversion's f32 scale operand is always the constant 1.0 here: whether the instruction multiplies by the whole f32 or only
// by its exponent (2^(E - 127)), 1.0 means "times one", so exactness does not rest on that reading.
//
// Load-time re-layout (the role repack_nvfp4 / process_nvfp4_scales play in petit_utils.py:61-75), MFMA-fragment order:
//   qpacked uint32 [N/16][K/128][64 lanes][4]: word s of lane (a = n % 16, g) of tile n / 16, block k / 128 holds
//           W[n][128 b + 32 s + 8 g + e], e = 0..7, nibble e at bits 4 e -- i.e. the checkpoint's own four bytes, moved whole:
//           a wave-wide 16-byte load IS the B operand of four v_mfma_f32_16x16x32 k-steps (1 KiB contiguous per (tile, block));
//   spacked uint32 [N/16][K/128][32]: word (h = g / 2) * 16 + a holds the four scale bytes lane (a, g) needs for the block,
//           byte s = weight_scale[n][8 b + 2 s + h] (a lane's 8 k of step s lie in ONE group of 16).  128 bytes per (tile, block),
//           one coalesced 4-byte load per lane; lanes g and g ^ 1 read the same word, so HBM sees 1024 + 128 bytes per 2048
//           weights: the format's own 9/16 byte per weight.
//
// Two forms behind sgl_mi355_nvfp4_gemm (sgl_mi355_nvfp4_gemm_form):
//   0, M <= 64: weight streaming, X-stationary (the structure of awq.hip): one 512-thread workgroup per CU; wave w keeps the A
//      fragments of k-blocks w, w + 8, .. of its k-range (4096 k for M <= 32, 2048 k for 33..64 rows) in registers for the whole
//      launch; the workgroup walks 16-column tiles with non-temporal weight loads, PD tiles in flight; the eight waves' partial
//      sums meet in LDS.  More than one k-range: f32 slabs in the workspace + nvfp4_slab_reduce_kernel.
//   1, M > 64: 128 x 128 workgroup tile, 4 waves (the structure of awq_tiled.hip): X slices double buffered in swizzled LDS, W
//      never touches LDS (packed words + scale words of PD k-blocks in registers, dequantised into B operands), every
//      dequantised word feeds 8 MFMAs; split-K over grid.y where the tiles are fewer than the CUs.
// The global scale is applied to the f32 sum in the epilogue (or in the slab reduce), before the bias.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2_t;

template <int B>
__device__ __forceinline__ float e4m3_byte(uint32_t sw) {  // float(byte B of sw as OCP e4m3fn): exact
  return __builtin_amdgcn_cvt_f32_fp8((int)sw, B);
}

// the four group scales of a lane's 128-k block (byte s of the spacked word serves k-step s), in the type the dequantisation
// multiplies by
template <typename T>
struct Nvfp4Scales;
template <>
struct Nvfp4Scales<_Float16> {
  _Float16 v[4];
  __device__ __forceinline__ void set(uint32_t sw) {
    v[0] = (_Float16)e4m3_byte<0>(sw); v[1] = (_Float16)e4m3_byte<1>(sw);
    v[2] = (_Float16)e4m3_byte<2>(sw); v[3] = (_Float16)e4m3_byte<3>(sw);
  }
};
template <>
struct Nvfp4Scales<__bf16> {
  float v[4];
  __device__ __forceinline__ void set(uint32_t sw) {
    v[0] = e4m3_byte<0>(sw); v[1] = e4m3_byte<1>(sw); v[2] = e4m3_byte<2>(sw); v[3] = e4m3_byte<3>(sw);
  }
};

// 8 weights of one packed word (nibble e at bits 4 e) times their group scale -> MFMA operand, exact (header)
__device__ __forceinline__ f16x8_t nvfp4_word(uint32_t wq, _Float16 s) {
  const f16x2_t s2 = {s, s};
  struct P { f16x2_t v[4]; } pk;
  pk.v[0] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(wq, 1.0f, 0) * s2;
  pk.v[1] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(wq, 1.0f, 1) * s2;
  pk.v[2] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(wq, 1.0f, 2) * s2;
  pk.v[3] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(wq, 1.0f, 3) * s2;
  return __builtin_bit_cast(f16x8_t, pk);
}
__device__ __forceinline__ bf16x8_t nvfp4_word(uint32_t wq, float s) {
  const f32x2_t e0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wq, 1.0f, 0);
  const f32x2_t e1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wq, 1.0f, 1);
  const f32x2_t e2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wq, 1.0f, 2);
  const f32x2_t e3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wq, 1.0f, 3);
  struct P { __bf16 v[8]; } pk;
  pk.v[0] = (__bf16)(e0[0] * s); pk.v[1] = (__bf16)(e0[1] * s);
  pk.v[2] = (__bf16)(e1[0] * s); pk.v[3] = (__bf16)(e1[1] * s);
  pk.v[4] = (__bf16)(e2[0] * s); pk.v[5] = (__bf16)(e2[1] * s);
  pk.v[6] = (__bf16)(e3[0] * s); pk.v[7] = (__bf16)(e3[1] * s);
  return __builtin_bit_cast(bf16x8_t, pk);
}

struct Nvfp4Params {
  const char* x;            // [M][K] T
  int64_t x_stride;         // elements
  const uint32_t* qpacked;  // [N/16][KB][64][4]
  const uint32_t* spacked;  // [N/16][KB][32]
  void* y;
  int64_t y_stride;
  const float* gscale;      // device scalar: weight_scale_2
  const void* bias;
  float* slabs;             // [kranges][M][N] raw f32 sums (null: one k-range, T outputs)
  int M, N, KB;             // KB = K / 128
  int mtiles, bpr, stream_w;  // tile form: row tiles, k-blocks per k-range, one row tile (every W byte read once: nt loads)
};

__device__ __forceinline__ unsigned nvfp4_w_offset(const Nvfp4Params& p, bool ok, int t, int b, int lane) {
  // loads past the last tile / block are predicated off by an out-of-range buffer offset (they return 0)
  return ok ? (unsigned)((((int64_t)t * p.KB + b) * 64 + lane) * 16) : 0xFFFFFFF0u;
}
__device__ __forceinline__ auto nvfp4_w_rsrc(const Nvfp4Params& p) {
  const int64_t wbytes = (int64_t)(p.N / 16) * p.KB * 1024;  // < 0xFFFFFFF0 (checked by the entry point)
  return __builtin_amdgcn_make_buffer_rsrc((void*)p.qpacked, 0, (unsigned)wbytes, 0x00020000);
}
// the lane's scale word of (tile t, block b): both in range by construction of the callers
__device__ __forceinline__ uint32_t nvfp4_scale_word(const Nvfp4Params& p, int t, int b, int lane) {
  return p.spacked[((int64_t)t * p.KB + b) * 32 + ((lane >> 5) << 4) + (lane & 15)];
}

// ------------------------------------------------------------------------------------------------------------------------
// Form 0: weight streaming, M <= 64
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kStreamWaves = 8;
constexpr int kStreamMaxM = 64;
// k-blocks per wave and k-range: 4 while the A fragments of 32 rows fit (128 VGPRs), 2 for 33..64 rows
constexpr int stream_bpw(int mt) { return mt >= 4 ? 2 : 4; }

// MT: 16-row tiles of X; PD: column tiles in flight; TPP: column tiles per phase (one pair of barriers per phase)
template <typename T, int MT, int PD, int TPP>
__global__ __launch_bounds__(kStreamWaves * 64, 1) void nvfp4_stream_kernel(const Nvfp4Params p, int ntiles) {
  typedef ElemTraits<T> Tr;
  typedef typename Tr::vec8 vec8;
  static_assert(TPP == 1 || TPP % PD == 0, "static slot indices");
  constexpr int BPW = stream_bpw(MT);
  constexpr int EPT = (MT * 16 + 31) / 32;  // output rows per thread and tile (512 threads cover 32 rows x 16 columns)
  __shared__ float red[TPP][kStreamWaves][MT * 16][16];
  __shared__ __attribute__((aligned(16))) char ximg[kStreamWaves * 4096];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = lane & 15, g = lane >> 4;
  const int kr = blockIdx.y;
  const int b0 = kr * (kStreamWaves * BPW);
  const int nb = min(kStreamWaves * BPW, p.KB - b0);  // k-blocks of this range (>= 1)
  const int G_ = gridDim.x;
  const int cnt = (ntiles - (int)blockIdx.x + G_ - 1) / G_;  // tiles of this workgroup: blockIdx.x + j * G_

  // ---- A fragments of this wave's k-blocks, once: coalesced 256-byte row pieces -> swizzled wave-private LDS image ->
  // registers (lane (a, g) holds X[16 mt + a][128 b + 32 s + 8 g .. + 7]); rows past M and blocks past the range are zero ----
  char* xl = ximg + w * 4096;                // 16 rows x 256 B
  const int lc = lane & 15, lr = lane >> 4;  // staging: 16-byte chunk lc of row lr + 4 i
  vec8 xf[MT][BPW][4];
#pragma unroll
  for (int bi = 0; bi < BPW; ++bi) {
    const bool bok = w + kStreamWaves * bi < nb;
    const int b = b0 + (bok ? w + kStreamWaves * bi : 0);
    u32x4_t xr[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mt * 16 + lr + 4 * i;
        const u32x4_t v = *(const u32x4_t*)((const T*)p.x + (int64_t)min(m, p.M - 1) * p.x_stride + 128 * b + 8 * lc);
        xr[mt][i] = (m < p.M && bok) ? v : u32x4_t{0u, 0u, 0u, 0u};
      }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = lr + 4 * i;
        *(u32x4_t*)(xl + row * 256 + (((lc ^ row) & 15) << 4)) = xr[mt][i];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
        xf[mt][bi][s] = __builtin_bit_cast(vec8, *(const u32x4_t*)(xl + a * 256 + ((((4 * s + g) ^ a) & 15) << 4)));
    }
  }

  const auto wrsrc = nvfp4_w_rsrc(p);
  u32x4_t wreg[PD][BPW];
  uint32_t sreg[PD][BPW];
  auto issue = [&](int slot, int j) {
    const int t = blockIdx.x + j * G_;
    const int tc = min(t, ntiles - 1);  // scale loads stay in range; weight loads past the end are predicated off
#pragma unroll
    for (int bi = 0; bi < BPW; ++bi) {
      const bool bok = w + kStreamWaves * bi < nb;
      const int b = b0 + (bok ? w + kStreamWaves * bi : 0);
      wreg[slot][bi] = __builtin_bit_cast(
          u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, nvfp4_w_offset(p, j < cnt && bok, t, b, lane), 0, 2));  // nt: read once
      sreg[slot][bi] = nvfp4_scale_word(p, tc, b, lane);
    }
  };
#pragma unroll
  for (int j = 0; j < PD; ++j) issue(j, j);

  const int em0 = tid >> 4, en = tid & 15;  // this thread's output elements of every tile: rows em0 + 32 e, column en
  const float gs = *p.gscale;
  const bool has_bias = p.bias != nullptr && p.slabs == nullptr;

  for (int j0 = 0; j0 < cnt; j0 += TPP) {
#pragma unroll
    for (int jj = 0; jj < TPP; ++jj) {
      const int j = j0 + jj;
      const int slot = (TPP == 1) ? 0 : (jj % PD);
      f32x4_t acc[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int bi = 0; bi < BPW; ++bi) {
        const u32x4_t wq = wreg[slot][bi];
        Nvfp4Scales<T> sc;
        sc.set(sreg[slot][bi]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const vec8 wfrag = nvfp4_word(wq[s], sc.v[s]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[mt] = Tr::mfma16(xf[mt][bi][s], wfrag, acc[mt]);
        }
      }
      if constexpr (TPP > 1) issue(slot, j + PD);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[jj][w][mt * 16 + 4 * g + r][a] = acc[mt][r];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int em = em0 + 32 * e;
      if (em >= MT * 16) continue;
#pragma unroll
      for (int jj = 0; jj < TPP; ++jj) {
        const int j = j0 + jj;
        const int n = (blockIdx.x + j * G_) * 16 + en;
        float v = 0.f;
#pragma unroll
        for (int ww = 0; ww < kStreamWaves; ++ww) v += red[jj][ww][em][en];
        if (!(j < cnt && em < p.M && n < p.N)) continue;
        if (p.slabs != nullptr) {
          p.slabs[((int64_t)kr * p.M + em) * p.N + n] = v;
        } else {
          v *= gs;
          if (has_bias) v += (float)((const T*)p.bias)[n];
          ((T*)p.y)[(int64_t)em * p.y_stride + n] = (T)v;
        }
      }
    }
    if (TPP > 1) __syncthreads();  // the next phase overwrites red
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// Form 1: 128 x 128 tile, M > 64
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kTilePD = 4;      // k-blocks of W in flight per wave (packed words + scale words in registers)
constexpr int kTileMinBpr = 3;  // shortest k-range, in k-blocks

template <typename T>
__global__ __launch_bounds__(256, 2) void nvfp4_tile_kernel(const Nvfp4Params p) {
  typedef ElemTraits<T> Tr;
  typedef typename Tr::vec8 vec8;
  constexpr int PD = kTilePD;
  static_assert(PD % 2 == 0, "the LDS buffer of a block is the parity of its register slot");
  constexpr int BM = 128;
  constexpr int SLICE = BM * 256;  // bytes of one X slice (128 rows x 128 k)
  constexpr int XI = 8;            // 16-byte chunks per thread and slice
  constexpr int RPP = 16;          // rows per staging pass, so row & 15 == lr & 15 in every pass
  extern __shared__ __attribute__((aligned(16))) char xlds[];  // [2][BM][256 B]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = lane & 15, g = lane >> 4;
  const int rt = blockIdx.x % p.mtiles, ct = blockIdx.x / p.mtiles;  // the row tiles of one W column tile run side by side
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

  // ---- W: packed words + scale words of PD k-blocks in registers; wave w owns column units 2 w, 2 w + 1 of the tile ----
  const auto wrsrc = nvfp4_w_rsrc(p);
  u32x4_t wreg[PD][2];
  uint32_t sreg[PD][2];
  auto issue = [&](int slot, int i) __attribute__((always_inline)) {
    const bool bok = i < nb;
    const int b = b0 + (bok ? i : 0);  // scale loads stay in range; weight loads past the end are predicated off
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = 8 * ct + 2 * w + u;
      const unsigned off = nvfp4_w_offset(p, bok && t < ntiles, t, b, lane);
      if (p.stream_w) wreg[slot][u] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, off, 0, 2));
      else wreg[slot][u] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, off, 0, 0));
      sreg[slot][u] = nvfp4_scale_word(p, min(t, ntiles - 1), b, lane);
    }
  };

  f32x4_t acc[8][2];  // [row tile][column unit]: rows 16 mt + 4 g + r, column 16 (8 ct + 2 w + u) + a
#pragma unroll
  for (int mt = 0; mt < 8; ++mt)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[mt][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int buf, int slot) __attribute__((always_inline)) {
    const char* xb = xlds + buf * SLICE + a * 256;
    Nvfp4Scales<T> sc[2];
    sc[0].set(sreg[slot][0]);
    sc[1].set(sreg[slot][1]);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      vec8 af[8];
#pragma unroll
      for (int mt = 0; mt < 8; ++mt)
        af[mt] = __builtin_bit_cast(vec8, *(const u32x4_t*)(xb + mt * 16 * 256 + ((((4 * s + g) ^ a) & 15) << 4)));
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const vec8 wf = nvfp4_word(wreg[slot][u][s], sc[u].v[s]);
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
  const float gs = *p.gscale;
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
        else ((T*)p.y)[(int64_t)m * p.y_stride + n] = (T)(acc[mt][u][r] * gs + bv);
      }
  }
}

// y[m][n] = T(sum_kr slabs[kr][m][n] * weight_scale_2 + bias[n])
template <typename T>
__global__ __launch_bounds__(256) void nvfp4_slab_reduce_kernel(const float* __restrict__ slabs, int S, const float* __restrict__ gscale,
                                                                const T* bias, T* out, int64_t out_stride, int M, int N) {
  const float gs = *gscale;
  const int64_t total = (int64_t)M * (N / 4);
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int m = (int)(idx / (N / 4)), n = (int)(idx - (int64_t)m * (N / 4)) * 4;
    f32x4_t v = *(const f32x4_t*)(slabs + (int64_t)m * N + n);
    for (int sI = 1; sI < S; ++sI) v += *(const f32x4_t*)(slabs + ((int64_t)sI * M + m) * N + n);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float r = v[c] * gs;
      if (bias) r += (float)bias[n + c];
      out[(int64_t)m * out_stride + n + c] = (T)r;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// load-time re-layout and the dense dequantisation
// ------------------------------------------------------------------------------------------------------------------------
// weight as uint32 [N][K/8]: word k / 8 of row n holds elements 8 (k / 8) .. + 7, nibble e at bits 4 e -- already the packed word
__global__ __launch_bounds__(256) void nvfp4_repack_w_kernel(const uint32_t* __restrict__ weight, uint32_t* __restrict__ qpacked,
                                                             int K, int N) {
  const int KB = K / 128;
  const int64_t total = (int64_t)(N / 16) * KB * 256;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int s = (int)(o & 3), lane = (int)((o >> 2) & 63);
    const int64_t tb = o >> 8;
    const int b = (int)(tb % KB), t = (int)(tb / KB);
    const int a = lane & 15, g = lane >> 4;
    qpacked[o] = weight[(int64_t)(16 * t + a) * (K / 8) + 16 * b + 4 * s + g];
  }
}

__global__ __launch_bounds__(256) void nvfp4_repack_s_kernel(const uint8_t* __restrict__ scale, uint32_t* __restrict__ spacked, int K,
                                                             int N) {
  const int KB = K / 128;
  const int64_t total = (int64_t)(N / 16) * KB * 32;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int a = (int)(o & 15), h = (int)((o >> 4) & 1);
    const int64_t tb = o >> 5;
    const int b = (int)(tb % KB), t = (int)(tb / KB);
    const uint8_t* row = scale + (int64_t)(16 * t + a) * (K / 16) + 8 * b + h;
    spacked[o] = (uint32_t)row[0] | ((uint32_t)row[2] << 8) | ((uint32_t)row[4] << 16) | ((uint32_t)row[6] << 24);
  }
}

// checkpoint tensors -> dense W [N][K]: one scale group (16 weights: two words, one scale byte, 32 bytes out) per thread and
// step, through the GEMMs' own nvfp4_word.  gscale null: the exact W; else T(W * *gscale), one rounding of the exact product.
template <typename T>
__global__ __launch_bounds__(256) void nvfp4_dequant_kernel(const uint32_t* __restrict__ weight, const uint8_t* __restrict__ scale,
                                                            const float* __restrict__ gscale, T* __restrict__ out, int64_t groups) {
  typedef typename ElemTraits<T>::vec8 vec8;
  const float gs = gscale != nullptr ? *gscale : 1.0f;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < groups; idx += (int64_t)gridDim.x * 256) {
    const uint32_t w0 = weight[2 * idx], w1 = weight[2 * idx + 1];
    Nvfp4Scales<T> sc;
    sc.set((uint32_t)scale[idx]);  // bytes 1..3 are zero: only v[0] is used
    vec8 v0 = nvfp4_word(w0, sc.v[0]), v1 = nvfp4_word(w1, sc.v[0]);
    if (gscale != nullptr) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v0[e] = (T)((float)v0[e] * gs);
        v1[e] = (T)((float)v1[e] * gs);
      }
    }
    *(vec8*)(out + idx * 16) = v0;
    *(vec8*)(out + idx * 16 + 8) = v1;
  }
}

int nvfp4_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
  }
  return cus;
}

int stream_kranges(int M, int KB) {
  const int blocks = kStreamWaves * stream_bpw(M > 32 ? 4 : 2);  // 128-k blocks per k-range
  return (KB + blocks - 1) / blocks;
}

// k-blocks per k-range of the tile form, for launches with fewer tiles than workgroup slots: the range length that minimises
//   rounds of resident workgroups x blocks per range x kBlockUs  +  ranges x (one f32 [M, N] slab written and read back at ~3 TB/s)
// plus the reduce launch (awq_tiled.hip's rule and constants: the same tile, the same slabs; estimates, not fitted).
int tile_bpr(int M, int N, int KB) {
  const int64_t tiles = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
  const int slots = 2 * nvfp4_cus();  // two 128-row workgroups per CU
  if (tiles >= slots) return KB;
  constexpr double kBlockUs = 1.5, kReduceUs = 4.0;
  const double slab_us = (double)M * N * 8.0 / 3.0e6;
  int best = KB;
  double best_us = KB * kBlockUs;
  for (int bpr = KB - 1; bpr >= kTileMinBpr; --bpr) {
    const int kr = (KB + bpr - 1) / bpr;
    const double us = (double)((tiles * kr + slots - 1) / slots) * bpr * kBlockUs + kr * slab_us + kReduceUs;
    if (us < best_us) { best = bpr; best_us = us; }
  }
  return best;
}

template <typename T, int MT>
void stream_launch(const Nvfp4Params& p, int kranges, hipStream_t st) {
  const int cus = nvfp4_cus();
  const int per_range = cus / kranges > 0 ? cus / kranges : 1;
  const int ntiles = p.N / 16;
  const int gx = ntiles < per_range ? ntiles : per_range;
  const dim3 grid(gx, kranges);
  if (ntiles <= gx)
    hipLaunchKernelGGL((nvfp4_stream_kernel<T, MT, 1, 1>), grid, dim3(kStreamWaves * 64), 0, st, p, ntiles);
  else
    hipLaunchKernelGGL((nvfp4_stream_kernel<T, MT, 2, (MT >= 4 ? 2 : 4)>), grid, dim3(kStreamWaves * 64), 0, st, p, ntiles);
}

template <typename T>
void stream_dispatch(const Nvfp4Params& p, int kranges, hipStream_t st) {
  if (p.M <= 16) stream_launch<T, 1>(p, kranges, st);
  else if (p.M <= 32) stream_launch<T, 2>(p, kranges, st);
  else stream_launch<T, 4>(p, kranges, st);
}

template <typename T>
void tile_launch(Nvfp4Params p, int kranges, hipStream_t st) {
  constexpr int smem = 2 * 128 * 256;  // 64 KiB
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)nvfp4_tile_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    attr_set = true;
  }
  p.mtiles = (p.M + 127) / 128;
  p.stream_w = p.mtiles == 1;
  hipLaunchKernelGGL((nvfp4_tile_kernel<T>), dim3(p.mtiles * ((p.N + 127) / 128), kranges), dim3(256), smem, st, p);
}

unsigned grid_for(int64_t items, unsigned cap) {
  const int64_t b = (items + 255) / 256;
  return (unsigned)(b > cap ? cap : (b < 1 ? 1 : b));
}

}  // namespace

// Which kernel sgl_mi355_nvfp4_gemm runs (host logic only): 0 = weight-streaming form, 1 = 128 x 128 tile form.
extern "C" int sgl_mi355_nvfp4_gemm_form(int M, int N, int K) {
  (void)N;
  (void)K;
  return M <= kStreamMaxM ? 0 : 1;
}

// Split-K ranges of sgl_mi355_nvfp4_gemm (f32 [M, N] slabs of workspace it wants; 1: none).
extern "C" int sgl_mi355_nvfp4_gemm_kranges(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K < 128) return 1;
  const int KB = K / 128;
  if (sgl_mi355_nvfp4_gemm_form(M, N, K) == 0) return stream_kranges(M, KB);
  const int bpr = tile_bpr(M, N, KB);
  return (KB + bpr - 1) / bpr;
}

// weight uint8 [N, K/2] + weight_scale e4m3 [N, K/16]  ->  qpacked (K N / 2 bytes), spacked (K N / 16 bytes); layouts above.
extern "C" int sgl_mi355_nvfp4_repack(const void* weight, const void* weight_scale, void* qpacked, void* spacked, int N, int K,
                                      void* stream) {
  SGL_CHECK(N > 0 && K > 0, "nvfp4_repack: bad shape");
  SGL_CHECK(K % 128 == 0 && N % 16 == 0, "nvfp4_repack: needs K %% 128 == 0 and N %% 16 == 0 (K=%d N=%d)", K, N);
  SGL_CHECK(weight && weight_scale && qpacked && spacked, "nvfp4_repack: null pointer");
  SGL_CHECK(((uintptr_t)weight % 4) == 0 && ((uintptr_t)qpacked % 16) == 0 && ((uintptr_t)spacked % 4) == 0,
            "nvfp4_repack: weight / spacked must be 4-byte and qpacked 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t tw = (int64_t)K * N / 8, ts = (int64_t)K * N / 64;
  hipLaunchKernelGGL(nvfp4_repack_w_kernel, dim3(grid_for(tw, 16384)), dim3(256), 0, st, (const uint32_t*)weight, (uint32_t*)qpacked, K, N);
  SGL_HIP_LAUNCH_CHECK();
  hipLaunchKernelGGL(nvfp4_repack_s_kernel, dim3(grid_for(ts, 16384)), dim3(256), 0, st, (const uint8_t*)weight_scale,
                     (uint32_t*)spacked, K, N);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

// Dense W [N, K] (row-major, bf16 / f16) from the checkpoint tensors; any K % 16 == 0.  global_scale null: WITHOUT
// weight_scale_2, bit-exact; else a device pointer to it and out = T(W * weight_scale_2).
extern "C" int sgl_mi355_nvfp4_dequantize(const void* weight, const void* weight_scale, const float* global_scale, void* out, int N,
                                          int K, int dtype, void* stream) {
  SGL_CHECK(N >= 0 && K >= 0, "nvfp4_dequantize: negative shape");
  if (N == 0 || K == 0) return SGL_MI355_OK;
  SGL_CHECK(K % 16 == 0, "nvfp4_dequantize: K=%d is not a multiple of the group size 16", K);
  SGL_CHECK(weight && weight_scale && out, "nvfp4_dequantize: null pointer");
  SGL_CHECK(dtype == SGL_BF16 || dtype == SGL_F16, "nvfp4_dequantize: dtype must be bf16 or f16");
  SGL_CHECK(((uintptr_t)weight % 4) == 0 && ((uintptr_t)out % 16) == 0, "nvfp4_dequantize: weight must be 4-byte and out 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t groups = (int64_t)N * (K / 16);
  const unsigned blocks = grid_for(groups, 16384);
  if (dtype == SGL_F16)
    hipLaunchKernelGGL((nvfp4_dequant_kernel<_Float16>), dim3(blocks), dim3(256), 0, st, (const uint32_t*)weight,
                       (const uint8_t*)weight_scale, global_scale, (_Float16*)out, groups);
  else
    hipLaunchKernelGGL((nvfp4_dequant_kernel<__bf16>), dim3(blocks), dim3(256), 0, st, (const uint32_t*)weight,
                       (const uint8_t*)weight_scale, global_scale, (__bf16*)out, groups);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

// y [M, N] = T( f32(x [M, K] . dequant(qpacked, spacked)^T) * *global_scale (+ bias) ); apply_petit_nvfp4_linear,
// petit_utils.py:78-104.  Any M (0: no launch); x rows may be padded.  workspace: kranges x M x N floats when
// sgl_mi355_nvfp4_gemm_kranges(M, N, K) > 1.  No allocation, no synchronisation, global_scale is never read on the host.
extern "C" int sgl_mi355_nvfp4_gemm(const void* x, int64_t x_stride_elems, const void* qpacked, const void* spacked, void* y,
                                    int64_t y_stride_elems, const float* global_scale, const void* bias, int M, int N, int K,
                                    int dtype, float* workspace, int64_t workspace_floats, void* stream) {
  SGL_CHECK(M >= 0 && N > 0 && K > 0, "nvfp4_gemm: bad shape");
  SGL_CHECK(K % 128 == 0 && N % 16 == 0, "nvfp4_gemm: needs K %% 128 == 0 and N %% 16 == 0 (K=%d N=%d)", K, N);
  SGL_CHECK(global_scale != nullptr, "nvfp4_gemm: global_scale (weight_scale_2, a device scalar) is null");
  if (M == 0) return SGL_MI355_OK;
  SGL_CHECK(x && qpacked && spacked && y, "nvfp4_gemm: null pointer");
  SGL_CHECK(dtype == SGL_BF16 || dtype == SGL_F16, "nvfp4_gemm: dtype must be bf16 or f16");
  SGL_CHECK(x_stride_elems % 8 == 0 && x_stride_elems >= K && ((uintptr_t)x % 16) == 0 && ((uintptr_t)qpacked % 16) == 0 &&
                ((uintptr_t)spacked % 4) == 0,
            "nvfp4_gemm: x rows and qpacked must be 16-byte aligned (x row stride >= K)");
  SGL_CHECK(y_stride_elems >= N, "nvfp4_gemm: y row stride %lld below N=%d", (long long)y_stride_elems, N);
  SGL_CHECK((int64_t)K * N / 2 < 0xFFFFFFF0ll, "nvfp4_gemm: weight larger than 4 GiB");
  const int KB = K / 128;
  const int form = sgl_mi355_nvfp4_gemm_form(M, N, K);
  Nvfp4Params p;
  p.x = (const char*)x; p.x_stride = x_stride_elems;
  p.qpacked = (const uint32_t*)qpacked; p.spacked = (const uint32_t*)spacked;
  p.y = y; p.y_stride = y_stride_elems; p.gscale = global_scale; p.bias = bias; p.slabs = nullptr;
  p.M = M; p.N = N; p.KB = KB;
  p.mtiles = 1; p.stream_w = 1;
  p.bpr = form == 0 ? KB : tile_bpr(M, N, KB);
  const int kranges = form == 0 ? stream_kranges(M, KB) : (KB + p.bpr - 1) / p.bpr;
  if (kranges > 1) {
    SGL_CHECK(workspace != nullptr && workspace_floats >= (int64_t)kranges * M * N && ((uintptr_t)workspace % 16) == 0,
              "nvfp4_gemm: M=%d N=%d K=%d needs a 16-byte aligned workspace of %d x M x N floats", M, N, K, kranges);
    p.slabs = workspace;
  }
  hipStream_t st = (hipStream_t)stream;
  if (form == 0) {
    if (dtype == SGL_BF16) stream_dispatch<__bf16>(p, kranges, st); else stream_dispatch<_Float16>(p, kranges, st);
  } else {
    if (dtype == SGL_BF16) tile_launch<__bf16>(p, kranges, st); else tile_launch<_Float16>(p, kranges, st);
  }
  SGL_HIP_LAUNCH_CHECK();
  if (kranges == 1) return SGL_MI355_OK;
  const unsigned blocks = grid_for((int64_t)M * (N / 4), 2048);
  if (dtype == SGL_BF16)
    hipLaunchKernelGGL((nvfp4_slab_reduce_kernel<__bf16>), dim3(blocks), dim3(256), 0, st, p.slabs, kranges, global_scale,
                       (const __bf16*)bias, (__bf16*)y, y_stride_elems, M, N);
  else
    hipLaunchKernelGGL((nvfp4_slab_reduce_kernel<_Float16>), dim3(blocks), dim3(256), 0, st, p.slabs, kranges, global_scale,
                       (const _Float16*)bias, (_Float16*)y, y_stride_elems, M, N);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}
