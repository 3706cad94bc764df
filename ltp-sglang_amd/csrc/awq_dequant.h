// Pieces shared by the int4 AWQ GEMMs (awq.hip: M <= 64, X-stationary; awq_tiled.hip: M > 64, tiled): the in-register
// dequantisation that reproduces awq_dequantize bit for bit, the split-K slab reduce and the CU count.
#pragma once
#include "common.h"

namespace {

template <int B>
__device__ __forceinline__ float cvt_ubyte(uint32_t x) {  // float(byte B of x): one VALU op, no shift / mask
  float f;
  if constexpr (B == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(x));
  else if constexpr (B == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(x));
  else if constexpr (B == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(x));
  else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(x));
  return f;
}

template <typename T>
struct AwqDequant;
// (szw: zero << 16 | scale bits)  ->  per-lane constants of one scale group, then 8 weights of one packed word
template <>
struct AwqDequant<_Float16> {
  f16x2_t s2, nz0, nz1;   // scale, -(1024 + z), -(64 + z) in both halves
  // (one uint32_t, never an element of a u32x2_t: `bit_cast<f16x2_t>(v[1])[0]` of a two-word vector compiles to word 0's half with
  // ROCm 7.2's hipcc -- tools/microbench/buffer_b64_halves.hip)
  __device__ __forceinline__ void setup(uint32_t szw) {
    const f16x2_t c = __builtin_bit_cast(f16x2_t, szw);
    s2 = f16x2_t{c[0], c[0]};      // op_sel on the sz word: no instruction
    nz0 = f16x2_t{c[1], c[1]};     // 0xE400 | z
    const f16x2_t d = __builtin_bit_cast(f16x2_t, ((szw >> 12) & 0xF0u) | 0xD400u);   // -(64 + z): z in mantissa bits 4..7
    nz1 = f16x2_t{d[0], d[0]};
  }
  __device__ __forceinline__ f16x8_t run(uint32_t wq) const {
    f16x2_t o[4];
    const uint32_t w8 = wq >> 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t pr;  // i even: (1024 + q[2i], 1024 + q[2i+1]); i odd: (64 + q[2i], 64 + q[2i+1]); one v_and_or_b32 each
      if (i & 1) asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(pr) : "v"(i < 2 ? wq : w8), "s"(0x00F000F0u), "v"(0x54005400u));
      else asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(pr) : "v"(i < 2 ? wq : w8), "s"(0x000F000Fu), "v"(0x64006400u));
      const f16x2_t d = __builtin_bit_cast(f16x2_t, pr) + ((i & 1) ? nz1 : nz0);   // exact small integers
      o[i] = d * s2;                                                              // one rounding: T(d * s)
    }
    struct P { f16x2_t v[4]; } pk{{o[0], o[1], o[2], o[3]}};
    return __builtin_bit_cast(f16x8_t, pk);
  }
};
template <>
struct AwqDequant<__bf16> {
  float sf, nzs;
  __device__ __forceinline__ void setup(uint32_t szw) {
    sf = (float)__builtin_bit_cast(__bf16, (uint16_t)(szw & 0xFFFFu));
    nzs = -(float)(szw >> 16) * sf;  // exact: 4-bit zero point x 8-bit scale
  }
  __device__ __forceinline__ bf16x8_t run(uint32_t wq) const {
    const uint32_t lo = wq & 0x0F0F0F0Fu, hi = (wq >> 4) & 0x0F0F0F0Fu;  // nibbles 0,2,4,6 = e 0,4,1,5 / 1,3,5,7 = e 2,6,3,7
    const float e0 = cvt_ubyte<0>(lo), e4 = cvt_ubyte<1>(lo);
    const float e1 = cvt_ubyte<2>(lo), e5 = cvt_ubyte<3>(lo);
    const float e2 = cvt_ubyte<0>(hi), e6 = cvt_ubyte<1>(hi);
    const float e3 = cvt_ubyte<2>(hi), e7 = cvt_ubyte<3>(hi);
    struct P { __bf16 v[8]; } pk;
    pk.v[0] = (__bf16)fmaf(e0, sf, nzs); pk.v[1] = (__bf16)fmaf(e1, sf, nzs);
    pk.v[2] = (__bf16)fmaf(e2, sf, nzs); pk.v[3] = (__bf16)fmaf(e3, sf, nzs);
    pk.v[4] = (__bf16)fmaf(e4, sf, nzs); pk.v[5] = (__bf16)fmaf(e5, sf, nzs);
    pk.v[6] = (__bf16)fmaf(e6, sf, nzs); pk.v[7] = (__bf16)fmaf(e7, sf, nzs);
    return __builtin_bit_cast(bf16x8_t, pk);
  }
};

// y[m][n] = T(sum_kr slabs[kr][m][n] + bias[n])
template <typename T>
__global__ __launch_bounds__(256) void awq_slab_reduce_kernel(const float* __restrict__ slabs, int S, const T* bias, T* out,
                                                              int64_t out_stride, int M, int N) {
  const int64_t total = (int64_t)M * (N / 4);
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int m = (int)(idx / (N / 4)), n = (int)(idx - (int64_t)m * (N / 4)) * 4;
    f32x4_t v = *(const f32x4_t*)(slabs + (int64_t)m * N + n);
    for (int sI = 1; sI < S; ++sI) v += *(const f32x4_t*)(slabs + ((int64_t)sI * M + m) * N + n);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float r = v[c];
      if (bias) r += (float)bias[n + c];
      out[(int64_t)m * out_stride + n + c] = (T)r;
    }
  }
}

inline int awq_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
  }
  return cus;
}

}  // namespace
