// Extend (prefill / chunked-prefill / RadixAttention-hit) attention over a latent (MLA) KV pool, gfx950: DeepSeek-V2 / V3 / R1 in
// the absorbed form, the prefill twin of mla_decode_attention.hip.
//
// Every query head attends over ONE shared 576-column row per token (kv_lora_rank 512 + qk_rope_head_dim 64); the value is the
// first 512 columns of the same row.  Replaces, for that shape, what the reference runs through extend_attention_fwd with
// Lq == 576 -> BLOCK_DMODEL 512 + BLOCK_DPE 64 (python/sglang/srt/layers/attention/triton_ops/extend_attention.py:336-338), called
// as attn_mqa(q, k, k_nope) with q [T, Hq, 576], k [T, 1, 576], v [T, 1, 512] (python/sglang/srt/models/deepseek_v2.py:1275-1277).
// Contract of extend_attention_fwd (extend_attention.py:306-438) for this shape: both index modes of ExtendParams, is_causal 0 / 1,
// logit_cap; no custom mask, no sliding window, no fp8 pool (the entry refuses them).
//
// Design (the decode kernel's 64-head form, WH = 4 / WD = 1, with (token, head) pairs in place of heads)
//  * rows.  A query row is a (token, head) pair; a request's rows are flattened as t x Hq + h and cut into blocks of 64.  A
//    workgroup is (request, row block): four waves, each owning one 16-row group (72 VGPRs of Q fragments), its own online-softmax
//    state and all 512 output columns (128 accumulator registers, in AGPRs); one workgroup per CU.  Rows past ext_len x Hq in the
//    last block are computed on zero queries and never stored.  With Hq a multiple of 16 a 16-row group lies inside one token;
//    with Hq = 8 it spans two, so the causal limit is a PER-LANE value taken from the lane's own row (row / Hq), never a wave scalar.
//  * ONE key stream per request: keys [0, pre) are pool rows taken through kv_indices (or req_to_token), keys [pre, pre + ext) are
//    the k_extend rows q0 + n - pre.  Tiles of 32 keys run over the concatenation and may straddle the seam: in the gather mapping
//    a lane owns one row of the tile (tid >> 3) and in load i the 16-byte chunk 8 i + (tid & 7), so it picks the row's source once.
//    Staging is the decode kernel's: 16-byte loads, register-staged (9 per lane) one tile ahead of the compute, the row's slot id
//    two tiles ahead; double-buffered in LDS as one swizzled 36 KiB image (chunk c of row r at c ^ f(r), see mla_decode_attention.hip
//    for the bank argument); QK^T A-fragments by ds_read_b128 and the transposed PV fragments by ds_read_b64_tr_b16 over columns
//    0-511 of the SAME image -- no V byte is loaded separately; one workgroup barrier per tile.  The loads are ordinary (cached)
//    loads: every row block of a request, Hq / 64 of them per token, reads the same rows.
//  * causal bound.  A row block whose last token is t1 walks ceil((pre + t1 + 1) / 32) tiles when causal, ceil((pre + ext) / 32)
//    when not; tiles wholly beyond the diagonal are never loaded.  Only tiles that reach past the diagonal of the block's FIRST
//    token, or past the end of the stream, take the masking pass (one block-uniform branch); masking sets -inf before the maximum,
//    so dead keys contribute an exact 0.  Key 0 is visible to every row, so every running maximum is finite after tile 0.
//  * arithmetic as in decode: S^T = K Q^T with v_mfma_f32_16x16x32 (2 key halves x 18 k-steps), f32 online softmax in registers,
//    the score accumulator is the B operand of O^T = V^T P^T (32 MFMAs per tile and wave); at the end a row is divided by its sum
//    and stored in the query dtype straight into o_extend.  Per tile and workgroup: 4 x (36 + 32) = 272 MFMAs and 272 KiB of LDS
//    reads for a 36 KiB image -- no redundant score.
//  * no split-KV and no stage 2: a prefill has T x Hq / 64 workgroups.  A short extend over a long prefix is served correctly
//    but with little parallelism.
//  * grid = (ceil(max_len_extend x Hq / 64), batch) with an early exit past the request's rows; blockIdx.x is reversed, so the
//    last row blocks, which walk the most keys under causal masking, are dispatched first (longest first).
#include "extend_params.h"

namespace {

constexpr int kD = 576, kDv = 512;
constexpr int kTile = 32;               // keys per tile
constexpr int kRowB = kD * 2;           // 1 152 bytes per latent row
constexpr int kCPR = kRowB / 16;        // 72 16-byte chunks per row
constexpr int kImgB = kTile * kRowB;    // 36 KiB per LDS image
constexpr int kKS = kD / 32;            // 18 QK^T k-steps
constexpr int kNW = 4;                  // waves per workgroup
constexpr int kRows = 16 * kNW;         // query rows per workgroup
constexpr int kNT = kDv / 16;           // 32 PV output column tiles per wave
constexpr int kNCH = kTile * kCPR / (kNW * 64);  // 9 staged chunks per lane per tile
static_assert(kNCH * kNW * 64 == kTile * kCPR, "the tile must be a whole number of workgroup-wide loads");

__device__ __forceinline__ int mla_swz(int row) { return (row & 6) | ((row >> 3) & 1); }

__device__ __forceinline__ float softcap_log2(float s_scaled, float cap) {
  // cap * tanh(x / cap) in log2 units, tanh(y) = 2 * sigmoid(2 y) - 1 (extend_attention.py:36-38)
  const float y = s_scaled / cap;
  const float t = 2.0f / (1.0f + __expf(-2.0f * y)) - 1.0f;
  return cap * t * kLog2e;
}

template <typename T>
__global__ __launch_bounds__(kNW * 64, 1) void mla_extend_kernel(const ExtendParams p) {
  using Tr = ElemTraits<T>;
  using vec8 = typename Tr::vec8;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = lane & 15;  // MFMA n index: query row within the wave's group
  const int g = lane >> 4;  // MFMA k/m group
  const int b = blockIdx.y;
  const int rb = gridDim.x - 1 - blockIdx.x;  // longest key ranges first

  const int q0 = p.qo_indptr ? p.qo_indptr[b] : p.extend_start_loc[b];
  const int ext = p.qo_indptr ? p.qo_indptr[b + 1] - q0 : p.extend_seq_lens[b];
  const int nrows = ext * p.hq;
  const int row0 = rb * kRows;
  if (row0 >= nrows) return;  // also a request without new tokens
  int pre;
  const int32_t* idx_row;
  if (p.kv_indptr) {  // mode by indptr: kv_indices may legitimately be NULL when no request has a prefix
    const int s0 = p.kv_indptr[b];
    pre = p.kv_indptr[b + 1] - s0;
    idx_row = p.kv_indices + s0;
  } else {
    pre = (int)p.seq_lens[b] - ext;
    idx_row = p.req_to_token + p.req_pool_indices[b] * p.req_to_token_stride;
  }

  // ---- the block's key range and the lane's own limit ----
  const int total = pre + ext;
  const int t_first = row0 / p.hq;
  const int t_last = (min(row0 + kRows, nrows) - 1) / p.hq;
  const int nkeys = p.is_causal ? pre + t_last + 1 : total;       // keys any row of this block may see (> pre)
  const int mask_from = p.is_causal ? pre + t_first + 1 : total;  // keys below are seen by every row of the block
  const int ntiles = (nkeys + kTile - 1) / kTile;
  const int row = row0 + 16 * w + a;
  const bool live_row = row < nrows;
  const int tok = min(row, nrows - 1) / p.hq;  // the lane's token inside the extend part
  const int head = min(row, nrows - 1) - tok * p.hq;
  const int lim = p.is_causal ? pre + tok + 1 : total;  // the lane's row sees keys [0, lim)

  // Q fragments: B operand of S^T = K Q^T, lane (a, g) holds Q[row][32 ks + 8 g .. + 8]
  vec8 qf[kKS];
  {
    const T* qrow = (const T*)p.q + (int64_t)(q0 + tok) * p.q_stride_t + (int64_t)head * kD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      if (live_row) {
        qf[ks] = *(const vec8*)(qrow + 32 * ks);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[ks][j] = (T)0.0f;
      }
    }
  }

  const char* kpool = (const char*)p.k_buf;
  const char* kext = (const char*)p.ke + (int64_t)q0 * p.ke_stride_t * 2;
  const int64_t kpst = p.k_stride_t * 2, kest = p.ke_stride_t * 2;
  const float scale_log2 = p.sm_scale * kLog2e;
  const bool use_cap = p.logit_cap > 0.0f;

  float m_i = -INFINITY, l_i = 0.0f;
  f32x4_t acc[kNT];
#pragma unroll
  for (int n = 0; n < kNT; ++n) acc[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // gather mapping: lane t of the workgroup owns row t >> 3 of the tile and, in load i, the 16-byte chunk 8 i + (t & 7) -- eight
  // lanes cover one 128-byte line of a row and the nine loads of a lane walk its row, so a lane needs ONE row id (a pool slot
  // before the seam, a k_extend row after it), one source select, one dead-row test and one LDS base
  const int srow = tid >> 3;
  const int ssub = tid & 7;
  const int st_off = srow * kRowB + ((ssub ^ mla_swz(srow)) << 4);
  u32x4_t stg[kNCH];
  auto load_id = [&](int t) -> int {  // (tiles past the last one: key >= nkeys > pre, nothing is read)
    const int key = t * kTile + srow;
    return key < pre ? idx_row[key] : min(key, nkeys - 1) - pre;
  };
  auto issue = [&](int t, int id) {
    const char* src = (t * kTile + srow < pre ? kpool + (int64_t)id * kpst : kext + (int64_t)id * kest) + ssub * 16;
#pragma unroll
    for (int i = 0; i < kNCH; ++i) stg[i] = *(const u32x4_t*)(src + 128 * i);
  };

  issue(0, load_id(0));
  int id_next = load_id(1);

  // fragment addressing: chunk c of row r lives at c ^ f(r); f moves the low three bits only, so a lane needs two K bases (k-step
  // parity) and four V bases (column tile mod 4) per image and every other term is an instruction immediate
  const int fk = mla_swz(a);
  const int k_off0 = a * kRowB + ((((fk >> 2) << 2) | (g ^ (fk & 3))) << 4);
  const int k_off1 = a * kRowB + (((((fk >> 2) ^ 1) << 2) | (g ^ (fk & 3))) << 4);
  const int vrow = 4 * g + (a >> 2);
  const int fv = mla_swz(vrow);
  const int v_off = vrow * kRowB + ((a & 1) << 3) + (((((a >> 1) & 1) ^ (fv & 1))) << 4);
  const int v_j[4] = {v_off + (((0 ^ (fv >> 1)) << 1) << 4), v_off + (((1 ^ (fv >> 1)) << 1) << 4),
                      v_off + (((2 ^ (fv >> 1)) << 1) << 4), v_off + (((3 ^ (fv >> 1)) << 1) << 4)};

  for (int tile = 0; tile < ntiles; ++tile) {
    const int key0 = tile * kTile;
    char* img = smem + (tile & 1) * kImgB;
    // ---- staged registers -> the swizzled LDS image of this tile ----
    {
      const bool dead = key0 + srow >= nkeys;  // 0 * garbage must stay 0
#pragma unroll
      for (int i = 0; i < kNCH; ++i) *(u32x4_t*)(img + st_off + 128 * i) = dead ? u32x4_t{0u, 0u, 0u, 0u} : stg[i];
    }
    // ---- issue the gather of the next tile, prefetch the row id two tiles ahead ----
    if (tile + 1 < ntiles) issue(tile + 1, id_next);
    id_next = load_id(tile + 2);
    __syncthreads();

    // ---- S^T = K Q^T for two 16-key halves (two independent MFMA chains) ----
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
    // ---- online softmax; lane (a, g) holds row a, keys 16 tt + 4 g + r ----
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
    if (key0 + kTile > mask_from) {  // block-uniform: the diagonal of the block's first token or the end of the stream is in reach
      const int rel = lim - key0 - 4 * g;  // key 16 tt + r of this lane is seen iff 16 tt + r < rel
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[tt][r] = (16 * tt + r < rel) ? x[tt][r] : -INFINITY;
    }
    float mt = -INFINITY;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mt = fmaxf(mt, x[tt][r]);
    mt = pair32_max(pair16_max(mt));          // over the four lane groups of a row
    const float m_new = fmaxf(m_i, mt * cs);  // finite from tile 0 on (key 0 is seen by every row); a later tile may be all -inf
    const float alpha = __builtin_amdgcn_exp2f(m_i - m_new);
    float lsum = 0.0f;
    vec8 pf;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(x[tt][r], cs, -m_new));
        lsum += pv;
        pf[4 * tt + r] = Tr::from_f32(pv);  // P is rounded to the V dtype before PV (extend_attention.py:200,281)
      }
    }
    l_i = l_i * alpha + lsum;  // per-lane partial; the 4 g-lanes of a row are summed once at the end
    m_i = m_new;
    // ---- O^T += V^T P^T over all 512 columns, V read transposed out of the same image ----
#pragma unroll
    for (int n = 0; n < kNT; ++n) {
      acc[n] *= alpha;
      const char* vp = img + v_j[n & 3] + (n >> 2) * 128;
      const s16x4_t t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)vp);
      const s16x4_t t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3)))*)(vp + 16 * kRowB));
      const s16x8_t t01 = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
      acc[n] = Tr::mfma16(__builtin_bit_cast(vec8, t01), pf, acc[n]);
    }
  }

  // ---- o = acc / l ; lane (a, g) owns query row a, columns 16 n + 4 g + [0, 4) ----
  l_i = pair32_sum(pair16_sum(l_i));
  if (live_row) {
    const float inv = 1.0f / l_i;  // l > 0: key 0 is seen by every row
    T* orow = (T*)p.o + (int64_t)(q0 + tok) * p.o_stride_t + (int64_t)head * kDv + 4 * g;
#pragma unroll
    for (int n = 0; n < kNT; ++n) {
      typename Tr::vec4 ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) ov[r] = Tr::from_f32(acc[n][r] * inv);
      *(typename Tr::vec4*)(orow + 16 * n) = ov;
    }
  }
}

template <typename T>
int launch_t(const ExtendParams& p, int max_len_extend, hipStream_t st) {
  constexpr int smem = 2 * kImgB;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mla_extend_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    attr_set = true;
  }
  const int64_t nblk = ((int64_t)max_len_extend * p.hq + kRows - 1) / kRows;
  if (nblk <= 0 || p.bs <= 0) return SGL_MI355_OK;
  if (nblk >= (1ll << 31) || p.bs > 65535) {
    snprintf(g_sgl_mi355_err, sizeof(g_sgl_mi355_err), "extend_attention: grid too large");
    return SGL_MI355_EINVAL;
  }
  hipLaunchKernelGGL((mla_extend_kernel<T>), dim3((unsigned)nblk, (unsigned)p.bs), dim3(kNW * 64), smem, st, p);
  SGL_HIP_LAUNCH_CHECK();
  return SGL_MI355_OK;
}

}  // namespace

int launch_mla_extend(const ExtendParams& p, int max_len_extend, int dtype, hipStream_t st) {
  return dtype == SGL_BF16 ? launch_t<__bf16>(p, max_len_extend, st) : launch_t<_Float16>(p, max_len_extend, st);
}
