// Launch parameters and the split rules shared by the decode-attention translation units (decode_attention.hip: the GQA kernels,
// stage 2 and the C-ABI entries; mla_decode_attention.hip: the 576 / 512 latent-KV kernel).  Field meanings follow
// decode_attention_fwd (python/sglang/srt/layers/attention/triton_ops/decode_attention.py:677-728) and decode_attention_cpu
// (sgl-kernel/csrc/cpu/decode.cpp:1375-1575).
#pragma once
#include "common.h"

struct DecodeParams {
  const void* q;
  int64_t q_stride_t;  // elements between tokens of q; heads are contiguous [Hq, D]
  const void* k_buf;
  const void* v_buf;
  int64_t k_stride_t, k_stride_h, v_stride_t, v_stride_h;  // elements
  void* o;
  int64_t o_stride_t;
  // index mode A (Triton backend metadata): kv_indptr/kv_indices
  const int32_t* kv_indptr;
  const int32_t* kv_indices;
  // index mode B (CPU op schema): req_to_token[req_pool_indices[b], :seq_lens[b]]
  const int32_t* req_to_token;
  int64_t req_to_token_stride;
  const int64_t* req_pool_indices;
  const int64_t* seq_lens;
  float* attn_logits;
  float* attn_lse;
  const int32_t* num_kv_splits;
  int max_kv_splits;
  int bs, hq, hkv, group, dv;
  float sm_scale, logit_cap;
  int kv_fp8;             // K/V pool rows are e4m3fn bytes (kv_cache_dtype fp8_e4m3, memory_pool.py:385-395), else the q dtype
  float k_scale, v_scale;  // K_true = K_fp8 * k_scale, V_true = V_fp8 * v_scale (radix_attention.py:73-76); 1 for 16-bit pools
  // in-launch stage 2 (MODE 0): the last workgroup of a request to finish merges its splits and quantises the row
  int32_t* merge_cnt;  // [bs], zero on entry, left zero; NULL = off
  void* mq_o;          // optional T [bs, Hq * Dv]
  void* mq_q;          // optional e4m3 [bs, Hq * Dv] with mq_s f32 [bs]
  float* mq_s;
  // Cascade shared-prefix decode: all `bs` requests share the first prefix_len slots of their sequences.
  //   prefix pass  a launch of the EXTEND kernel (extend_attention.hip, ExtendParams::casc_*): the bs decode queries are the
  //                query block, the shared rows the keys, staged once per (kv head, 32 requests, split) in LDS for all 4 x 32
  //                (head, request) pairs of a workgroup; prefix_splits split partials (O = acc / l, LSE) per (request, head)
  //                go to the TOP split slots [max_kv_splits - prefix_splits, max_kv_splits).  (Round 2 first ran the prefix as
  //                16-column chunks of this kernel -- every chunk re-read the rows, 19.6 us at 64 x 1536 -- and then had the
  //                merging workgroup of every request read prefix + suffix partials, +2 us per prefix split.)
  //   suffix pass  (CASC = 2, prefix_splits > 0): the ordinary kernel over every request's private slots, except that split 0
  //                of every (request, kv head) CONTINUES the online softmax from the prefix state (the LSE-weighted sum of the
  //                prefix partials is its initial (m, l, acc) -- the math of merge_state, merge_attn_states.cu, applied before
  //                instead of after), so the in-launch merge sees suffix slots only.
  int prefix_len, prefix_splits;
  // Flat unit list (round 5, SCHED kernels; csrc/kv_index.hip decode_schedule_kernel): the (request, split) units of the launch as a
  // list sorted by length, longest first -- grid y walks the list, so the dispatcher starts the long units first and fills the
  // chip's slots with short ones as they free up (ragged batches), and the grid carries no never-live workgroups.
  // sched: {T, units, total tokens, capacity}, then per unit {request, split | splits << 16, kv_indptr[request], its length}.
  // sched_chunks = grid y = the capacity the host sized the list for.
  const int32_t* sched;
  int sched_chunks;
#ifdef SGL_DEC_TIMELINE
  long long* tl;   // tools/debug/dec_timeline.py: s_memrealtime stamps [workgroup (linear)][wave][8]
#endif
};

// mla_decode_attention.hip: stage 1 of the 576 / 512 latent-KV (MLA) decode, one kv head, V = the first 512 columns of K.
// dtype: SGL_BF16 / SGL_F16.  Returns SGL_MI355_OK after a launch; the caller (decode_entry) has checked the shape and aliasing.
int launch_mla_decode(const DecodeParams& p, int dtype, hipStream_t st);

namespace {

constexpr int kTile = 32;  // tokens per wave tile == reference _MIN_BLOCK_KV (decode_attention.py:35)
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ void request_range(const DecodeParams& p, int b, const int32_t*& idx_row, int& seq_len) {
  if (p.kv_indptr != nullptr) {
    const int s0 = p.kv_indptr[b];
    seq_len = p.kv_indptr[b + 1] - s0;
    idx_row = p.kv_indices + s0;
  } else {
    seq_len = (int)p.seq_lens[b];
    idx_row = p.req_to_token + p.req_pool_indices[b] * p.req_to_token_stride;
  }
}

__device__ __forceinline__ int split_len(int seq_len, int nsplit) {
  // decode_attention.py:90-94: ceil(ceil(seq/splits)/MIN_BLOCK_KV)*MIN_BLOCK_KV
  const int per = (seq_len + nsplit - 1) / nsplit;
  return (per + kTile - 1) / kTile * kTile;
}

__device__ __forceinline__ float softcap_log2(float s_scaled, float cap) {
  // cap * tanh(x / cap), tanh(y) = 2*sigmoid(2y) - 1 (decode_attention.py:38-41)
  const float y = s_scaled / cap;
  const float t = 2.0f / (1.0f + __expf(-2.0f * y)) - 1.0f;
  return cap * t * kLog2e;
}

}  // namespace
