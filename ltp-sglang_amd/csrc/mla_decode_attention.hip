// Split-KV decode attention over a latent (MLA) KV pool, stage 1, gfx950: DeepSeek-V2 / V3 / R1 decode in the absorbed form.
//
// Every query head of the rank attends over ONE shared row per token, kv_lora_rank + qk_rope_head_dim = 512 + 64 = 576 columns
// (MLATokenToKVPool, python/sglang/srt/mem_cache/memory_pool.py:708-853); the value is the first 512 columns of the same row.
// Replaces, for that shape, what the reference runs through decode_attention_fwd -> _fwd_grouped_kernel_stage1 with
// Lk == 576 -> BLOCK_DMODEL 512 + BLOCK_DPE 64 (python/sglang/srt/layers/attention/triton_ops/decode_attention.py:244-462).
// Same contract as the GQA stage 1 (decode_attention.hip): attn_logits f32 [bs, Hq, max_kv_splits, 512] = acc / l,
// attn_lse = m + log l, the same split_len rule and request_range; decode_attn_stage2 merges unchanged.
//
// Design
//  * unit = (request, kv split, head block).  A head block is WH 16-head groups, WH = 1 / 2 / 4 for Hq <= 16 / <= 32 / more, so
//    Hq = 128 is two 64-head blocks.  Heads past Hq in the last group are computed on zero queries and never stored.  Grid =
//    (head blocks, bs, max_kv_splits): the split index is the SLOWEST dimension, not the middle one, because the GQA kernel
//    measured that never-live splits interleaved with live ones double a bs-128 launch (decode_attention.hip, launch_mfma).
//  * ONE KV tile per workgroup, used twice: 32 tokens x 576 columns gathered through kv_indices with 16-byte loads,
//    register-staged (9 loads per lane) and issued one tile ahead of the compute; double-buffered in LDS (2 x 36 KiB); all four
//    waves read their QK^T A-fragments (ds_read_b128) and their transposed PV fragments (ds_read_b64_tr_b16 over columns 0-511)
//    from that one image -- no V byte is loaded separately -- with one workgroup barrier per tile (a wave can only overwrite
//    buffer i & 1 two barriers after it was read).
//    Gather mapping, where the resource report forced a deviation: with 72 consecutive lanes on one contiguous 1 152-byte row
//    (chunk = i x 256 + tid) every one of a lane's nine loads has its own row, slot id, dead-row test and swizzled LDS address;
//    kept live across the loop that is > 50 registers and the WH = 2 instantiation spilled (256 VGPRs, 96 bytes of scratch).
//    Here a lane owns ONE row of the tile (tid >> 3) and in load i the chunk 8 i + (tid & 7): eight lanes cover one whole
//    128-byte line, the nine loads of the lane walk its row back to back, and the lane needs one slot id and one LDS base.
//  * Bank layout.  The row stride is 288 dwords = 32 mod 64 banks: an even row starts at bank 0, an odd row at bank 32, so in units
//    of 16-byte slots (16 per 256-byte bank line) chunk c of row r sits in slot 8 (r & 1) + c mod 16.  Chunk c of row r is stored at
//    chunk c ^ f(r), f(r) = (r & 6) | ((r >> 3) & 1) -- only the low three bits move, and 72 = 9 x 8, so the row stays in place.
//      - K fragments: the 16 lanes of one ds_read_b128 phase read chunk 4 ks + g of rows a = 0..15.  (a & 1, f(a)) takes 16
//        different values (f(a) runs through all 8 values over the 8 rows of one parity), so the 16 slots are all different.
//      - transposed V fragments: the 32 lanes of one ds_read_b64_tr_b16 phase read the chunk pair {2n, 2n + 1} of rows 0..7 (or
//        8..15).  The pair of row r lands on slot pair (n ^ (f(r) >> 1)) of its parity's half; f(r) >> 1 = (r >> 1) & 3 is different
//        for the four rows of one parity, so the eight rows take the sixteen slots once each.
//  * waves as a WH x WD grid over (16-head group, slice of the 512 output columns), WD = 4 / WH.  A wave keeps its group's Q
//    fragments in registers (16 heads x 576 columns = 72 VGPRs) and its own online-softmax state.  S^T = K Q^T with
//    v_mfma_f32_16x16x32 (2 token halves x 18 k-steps = 36 MFMAs per tile); the accumulator after the in-register softmax is
//    already the B operand of O^T = V^T P^T (head on lane & 15, 4 + 4 tokens in registers), 32 / WD MFMAs for the wave's 512 / WD
//    columns.  The WD waves of a head group compute the same scores from the same LDS bytes with the same instructions, so their
//    softmax states are bit-identical and no cross-wave merge exists.
//  * wave count: FOUR, from the compiler's resource report (DESIGN.md has the table; scratch 0 everywhere).  With eight waves and
//    WD = 2 a 64-head block would spend 4 x (2 x 36 + 32) = 416 MFMAs and 8 x 36 + 8 x 16 = 416 KiB of LDS reads per tile; with four
//    waves and WD = 1 the same block spends 4 x (36 + 32) = 272 MFMAs and 4 x (36 + 32) = 272 KiB -- no redundant score at all at 64
//    heads per block; the 128 accumulator registers live in AGPRs and the workgroup runs alone on its CU (one wave per SIMD).
//    The redundancy that remains: 36 MFMAs per tile per extra wave of a head group, i.e. 72 at 32 heads (WD = 2: 2 x 36 of
//    2 x (2 x 36 + 16) = 176) and 108 at <= 16 heads (WD = 4: 3 x 36 of 4 x (36 + 8) = 176), where the launch is a gather.
//  * logit_cap as in the GQA kernel (softcap_log2); k_scale / v_scale do not apply (16-bit pool).  Both index modes of
//    request_range work; the in-launch merge is not offered (it is limited to Hq x Dv <= 16 384).
#include "decode_params.h"

namespace {

constexpr int kD = 576, kDv = 512;
constexpr int kRowB = kD * 2;           // 1 152 bytes per latent row
constexpr int kCPR = kRowB / 16;        // 72 16-byte chunks per row
constexpr int kImgB = kTile * kRowB;    // 36 KiB per LDS image
constexpr int kKS = kD / 32;            // 18 QK^T k-steps
constexpr int kNW = 4;                  // waves per workgroup
constexpr int kNCH = kTile * kCPR / (kNW * 64);  // 9 staged chunks per lane per tile
static_assert(kNCH * kNW * 64 == kTile * kCPR, "the tile must be a whole number of workgroup-wide loads");

__device__ __forceinline__ int mla_swz(int row) { return (row & 6) | ((row >> 3) & 1); }

template <typename T, int WH>
__global__ __launch_bounds__(kNW * 64, WH == 4 ? 1 : 2) void mla_decode_stage1(const DecodeParams p) {
  using Tr = ElemTraits<T>;
  using vec8 = typename Tr::vec8;
  constexpr int WD = kNW / WH;
  constexpr int NT = kDv / 16 / WD;  // PV output column tiles of this wave
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wh = w / WD, wd = w - wh * WD;
  const int a = lane & 15;  // MFMA n index: q head within the group
  const int g = lane >> 4;  // MFMA k/m group
  const int b = blockIdx.y, split = blockIdx.z;

  const int32_t* idx_row;
  int seq_len;
  request_range(p, b, idx_row, seq_len);
  const int nsplit = max(1, min(p.num_kv_splits[b], p.max_kv_splits));
  if (split >= nsplit) return;
  const int per = split_len(seq_len, nsplit);
  const int start = split * per;
  const int end = min(start + per, seq_len);
  if (start >= end) return;
  const int ntiles = (end - start + kTile - 1) / kTile;

  // Q fragments: B operand of S^T = K Q^T, lane (a, g) holds Q[head][32 ks + 8 g .. + 8]
  const int head = (blockIdx.x * WH + wh) * 16 + a;
  const bool live_head = head < p.hq;
  vec8 qf[kKS];
  {
    const T* qrow = (const T*)p.q + (int64_t)b * p.q_stride_t + (int64_t)min(head, p.hq - 1) * kD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      if (live_head) {
        qf[ks] = *(const vec8*)(qrow + 32 * ks);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[ks][j] = (T)0.0f;
      }
    }
  }

  const char* kbase = (const char*)p.k_buf;
  const int64_t kst = p.k_stride_t * 2;
  const float scale_log2 = p.sm_scale * kLog2e;
  const bool use_cap = p.logit_cap > 0.0f;
  // a row is read once per head block: with one head block nothing re-reads it (non-temporal); with two the second block's
  // read may still find it in a cache
  const bool stream_once = gridDim.x == 1;

  float m_i = -INFINITY, l_i = 0.0f;
  f32x4_t acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // gather mapping: lane t of the workgroup owns row t >> 3 of the tile and, in load i, the 16-byte chunk 8 i + (t & 7) -- eight
  // lanes cover one 128-byte line of a row and the nine loads of a lane walk its row, so a lane needs ONE slot id, one dead-row
  // test and one LDS base (the swizzle moves only the low three chunk bits: load i lands at base + 128 i)
  const int srow = tid >> 3;
  const int ssub = tid & 7;
  const int st_off = srow * kRowB + ((ssub ^ mla_swz(srow)) << 4);
  u32x4_t stg[kNCH];
  auto load_idx = [&](int t) -> int {
    const int tok = start + t * kTile + srow;
    return (t < ntiles && tok < end) ? idx_row[tok] : 0;
  };
  auto issue = [&](int id) {
    const char* src = kbase + (int64_t)id * kst + ssub * 16;
#pragma unroll
    for (int i = 0; i < kNCH; ++i)
      stg[i] = stream_once ? __builtin_nontemporal_load((const u32x4_t*)(src + 128 * i)) : *(const u32x4_t*)(src + 128 * i);
  };

  issue(load_idx(0));
  int idx_next = load_idx(1);

  // fragment addressing: chunk c of row r lives at c ^ f(r); f moves the low three bits only, so a lane needs two K bases (k-step
  // parity) and four V bases (column tile mod 4) per image and every other term is an instruction immediate
  const int fk = mla_swz(a);
  const int k_off0 = a * kRowB + ((((fk >> 2) << 2) | (g ^ (fk & 3))) << 4);
  const int k_off1 = a * kRowB + (((((fk >> 2) ^ 1) << 2) | (g ^ (fk & 3))) << 4);
  const int vrow = 4 * g + (a >> 2);
  const int fv = mla_swz(vrow);
  const int v_off = vrow * kRowB + ((a & 1) << 3) + wd * (NT * 32) + (((((a >> 1) & 1) ^ (fv & 1))) << 4);
  const int v_j[4] = {v_off + (((0 ^ (fv >> 1)) << 1) << 4), v_off + (((1 ^ (fv >> 1)) << 1) << 4),
                      v_off + (((2 ^ (fv >> 1)) << 1) << 4), v_off + (((3 ^ (fv >> 1)) << 1) << 4)};

  for (int tile = 0; tile < ntiles; ++tile) {
    const int tok0 = start + tile * kTile;
    char* img = smem + (tile & 1) * kImgB;
    // ---- staged registers -> the swizzled LDS image of this tile ----
    {
      const bool dead = tok0 + srow >= end;  // 0 * garbage must stay 0
#pragma unroll
      for (int i = 0; i < kNCH; ++i) *(u32x4_t*)(img + st_off + 128 * i) = dead ? u32x4_t{0u, 0u, 0u, 0u} : stg[i];
    }
    // ---- issue the gather of the next tile, prefetch the slot id two tiles ahead ----
    if (tile + 1 < ntiles) issue(idx_next);
    idx_next = load_idx(tile + 2);
    __syncthreads();

    // ---- S^T = K Q^T for two 16-token halves (two independent MFMA chains) ----
    f32x4_t s[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      const char* kp = img + ((ks & 1) ? k_off1 : k_off0) + (ks >> 1) * 128;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const vec8 kf = *(const vec8*)(kp + tt * 16 * kRowB);
        s[tt] = Tr::mfma16(kf, qf[ks], s[tt]);
      }
    }
    // ---- online softmax; lane (a, g) holds head a, tokens 16 tt + 4 g + r ----
    float x[2][4];
    if (use_cap) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[tt][r] = softcap_log2(s[tt][r] * p.sm_scale, p.logit_cap);
    } else {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[tt][r] = s[tt][r];
    }
    const float cs = use_cap ? 1.0f : scale_log2;  // the exponent is x * cs - m (cs > 0)
    float mt = -INFINITY;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tok = tok0 + 16 * tt + 4 * g + r;
        x[tt][r] = (tok < end) ? x[tt][r] : -INFINITY;
        mt = fmaxf(mt, x[tt][r]);
      }
    }
    mt = pair32_max(pair16_max(mt));          // over the four lane groups of a head
    const float m_new = fmaxf(m_i, mt * cs);  // finite: every tile holds >= 1 valid token
    const float alpha = __builtin_amdgcn_exp2f(m_i - m_new);
    float lsum = 0.0f;
    vec8 pf;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(x[tt][r], cs, -m_new));
        lsum += pv;
        pf[4 * tt + r] = Tr::from_f32(pv);  // P is rounded to the V dtype before PV (decode_attention.py:373)
      }
    }
    l_i = l_i * alpha + lsum;  // per-lane partial; the 4 g-lanes of a head are summed once at the end
    m_i = m_new;
    // ---- O^T += V^T P^T over this wave's 512 / WD columns, V read transposed out of the same image ----
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      acc[n] *= alpha;
      const char* vp = img + v_j[n & 3] + (n >> 2) * 128;
      const s16x4_t t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)vp);
      const s16x4_t t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)(vp + 16 * kRowB));
      const s16x8_t t01 = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
      acc[n] = Tr::mfma16(__builtin_bit_cast(vec8, t01), pf, acc[n]);
    }
  }

  // ---- the wave's slice of the split partial, straight from the accumulator layout ----
  l_i = pair32_sum(pair16_sum(l_i));
  if (live_head) {
    const int64_t slot = ((int64_t)b * p.hq + head) * p.max_kv_splits + split;
    const float inv = 1.0f / l_i;
    float* dst = p.attn_logits + slot * kDv + wd * (NT * 16) + 4 * g;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      f32x4_t o = acc[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] *= inv;
      *(f32x4_t*)(dst + 16 * n) = o;
    }
    if (wd == 0 && g == 0) p.attn_lse[slot] = m_i * kLn2 + __logf(l_i);
  }
}

template <typename T, int WH>
int launch_wh(const DecodeParams& p, hipStream_t st) {
  constexpr int smem = 2 * kImgB;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mla_decode_stage1<T, WH>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    attr_set = true;
  }
  const dim3 grid((p.hq + 16 * WH - 1) / (16 * WH), p.bs, p.max_kv_splits);
  hipLaunchKernelGGL((mla_decode_stage1<T, WH>), grid, dim3(kNW * 64), smem, st, p);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

template <typename T>
int launch_t(const DecodeParams& p, hipStream_t st) {
  if (p.hq <= 16) return launch_wh<T, 1>(p, st);
  if (p.hq <= 32) return launch_wh<T, 2>(p, st);
  return launch_wh<T, 4>(p, st);
}

}  // namespace

int launch_mla_decode(const DecodeParams& p, int dtype, hipStream_t st) {
  return dtype == SGL_BF16 ? launch_t<__bf16>(p, st) : launch_t<_Float16>(p, st);
}
