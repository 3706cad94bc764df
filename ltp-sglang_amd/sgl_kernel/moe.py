"""MoE ops: routing, token alignment, the grouped expert GEMM and the sum over topk (csrc/moe_align.hip, csrc/moe_gemm.hip).

topk_softmax and moe_align_block_size carry the parameter names, order and defaults of sgl-kernel/python/sgl_kernel/moe.py:6-36.
No op synchronises with the host; the only allocation is moe_align_block_size's histogram workspace above 4096 pairs, taken from
torch's caching allocator before the launch (capturable like every other torch.empty)."""
from typing import Optional

import torch

from .._cabi import check, current_stream, dtype_code, lib, ptr


def _cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("MoE ops take GPU tensors only (there is no CPU path)")


def topk_softmax(topk_weights: torch.Tensor, topk_ids: torch.Tensor, gating_output: torch.Tensor, renormalize: bool = False) -> None:
    """softmax over the experts in f32, then top-k (ties: the lower index); in-place outputs topk_weights f32 [T, topk] and
    topk_ids int32 [T, topk]; gating_output [T, E] f32 / bf16 / f16, E <= 512, topk <= min(E, 32)."""
    _cuda(topk_weights, topk_ids, gating_output)
    if topk_weights.dtype != torch.float32 or topk_ids.dtype != torch.int32:
        raise RuntimeError("topk_softmax: topk_weights must be float32 and topk_ids int32")
    if gating_output.dim() != 2 or topk_weights.shape != topk_ids.shape or topk_ids.shape[0] != gating_output.shape[0]:
        raise RuntimeError("topk_softmax: gating_output [T, E] and topk_weights / topk_ids [T, topk] expected")
    if not (topk_weights.is_contiguous() and topk_ids.is_contiguous() and gating_output.is_contiguous()):
        raise RuntimeError("topk_softmax: tensors must be contiguous")
    t, e = gating_output.shape
    check(lib.sgl_mi355_topk_softmax(ptr(topk_weights), ptr(topk_ids), ptr(gating_output), t, e, topk_ids.shape[1],
                                     int(bool(renormalize)), dtype_code(gating_output.dtype), current_stream()))


def moe_align_block_size(topk_ids, num_experts, block_size, sorted_token_ids, experts_ids, num_tokens_post_pad, cumsum_buffer,
                         pad_sorted_token_ids=False):
    """The sorted layout of fused_moe.py:549-619 into the caller's int32 buffers; within an expert the pair indices ascend, and
    ids outside [0, num_experts) are left out.  cumsum_buffer: at least num_experts + 1 entries."""
    _cuda(topk_ids, sorted_token_ids, experts_ids, num_tokens_post_pad, cumsum_buffer)
    for t in (topk_ids, sorted_token_ids, experts_ids, num_tokens_post_pad, cumsum_buffer):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError("moe_align_block_size: every tensor must be contiguous int32")
    pairs = topk_ids.numel()
    active = min(pairs, num_experts)
    if cumsum_buffer.numel() < num_experts + 1 or experts_ids.numel() * block_size < pairs + active * (block_size - 1):
        raise RuntimeError("moe_align_block_size: cumsum_buffer or experts_ids too small for the worst case")
    ws_n = int(lib.sgl_mi355_moe_align_workspace_ints(pairs, int(num_experts)))
    ws = torch.empty(ws_n, dtype=torch.int32, device=topk_ids.device) if ws_n else None
    check(lib.sgl_mi355_moe_align_block_size(ptr(topk_ids), pairs, int(num_experts), int(block_size), ptr(sorted_token_ids),
                                             sorted_token_ids.numel(), ptr(experts_ids), ptr(num_tokens_post_pad), ptr(cumsum_buffer),
                                             int(bool(pad_sorted_token_ids)), ptr(ws), ws_n, current_stream()))


def moe_gemm_form(num_pairs: int, num_experts: int, n: int, k: int) -> int:
    """Which grouped GEMM fused_experts runs: 0 = weight-streaming form (block_size 16), 1 = 128 x 128 tile form (block_size 128)."""
    return int(lib.sgl_mi355_moe_gemm_form(int(num_pairs), int(num_experts), int(n), int(k)))


def moe_grouped_gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, topk_weights: Optional[torch.Tensor],
                     sorted_token_ids: torch.Tensor, experts_ids: torch.Tensor, num_tokens_post_pad: torch.Tensor, block_size: int,
                     a_rows_div: int, silu_and_mul: bool) -> None:
    """out[p] = epilogue(a[p // a_rows_div] @ w[expert of pair p].T) for every pair of the layout; out [P, N].
    silu_and_mul: w [E, 2 N, K] (gate rows, then up rows) and out = silu(gate) * up; else w [E, N, K].  topk_weights (f32, one per
    pair), when given, multiplies the f32 sums (gate and up, before the silu) ahead of the one rounding.  block_size 16 / 128
    selects the streaming / tile form."""
    _cuda(a, w, out, topk_weights, sorted_token_ids, experts_ids, num_tokens_post_pad)
    if not (a.is_contiguous() and w.is_contiguous() and out.is_contiguous()) or a.dtype != w.dtype or out.dtype != a.dtype:
        raise RuntimeError("moe_grouped_gemm: a, w and out must be contiguous and of one dtype")
    if a.dim() != 2 or w.dim() != 3 or out.dim() != 2 or w.shape[2] != a.shape[1]:
        raise RuntimeError("moe_grouped_gemm: a [rows, K], w [E, N, K] and out [P, N] expected")
    e, nw, k = w.shape
    pairs, n = out.shape
    if nw != (2 * n if silu_and_mul else n) or a.shape[0] * a_rows_div < pairs:
        raise RuntimeError("moe_grouped_gemm: shapes of a, w and out do not match")
    if topk_weights is not None and (topk_weights.dtype != torch.float32 or not topk_weights.is_contiguous()
                                     or topk_weights.numel() != pairs):
        raise RuntimeError("moe_grouped_gemm: topk_weights must be contiguous float32 with one entry per pair")
    for t in (sorted_token_ids, experts_ids, num_tokens_post_pad):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError("moe_grouped_gemm: the layout tensors must be contiguous int32")
    active = min(pairs, e)
    if sorted_token_ids.numel() < pairs + active * (block_size - 1) or experts_ids.numel() * block_size < pairs + active * (block_size - 1):
        raise RuntimeError("moe_grouped_gemm: the layout tensors are smaller than the worst case of this launch's grid")
    check(lib.sgl_mi355_moe_grouped_gemm(ptr(a), ptr(w), ptr(out), ptr(topk_weights), ptr(sorted_token_ids), ptr(experts_ids),
                                         ptr(num_tokens_post_pad), pairs, int(a_rows_div), e, n, k, int(block_size),
                                         int(bool(silu_and_mul)), dtype_code(a.dtype), current_stream()))


def moe_sum_reduce(y: torch.Tensor, out: torch.Tensor, routed_scaling_factor: float, topk_ids: Optional[torch.Tensor] = None,
                   num_experts: int = 0) -> None:
    """out[t] = round(routed_scaling_factor * sum_j y[t][j]) in f32, j ascending; y [T, topk, H], out [T, H].  With topk_ids
    (int32 [T, topk]) every j whose id is outside [0, num_experts) is skipped."""
    _cuda(y, out, topk_ids)
    if y.dim() != 3 or tuple(out.shape) != (y.shape[0], y.shape[2]) or y.dtype != out.dtype:
        raise RuntimeError("moe_sum_reduce: y [T, topk, H] and out [T, H] of one dtype expected")
    if not (y.is_contiguous() and out.is_contiguous()):
        raise RuntimeError("moe_sum_reduce: tensors must be contiguous")
    if topk_ids is not None and (topk_ids.dtype != torch.int32 or not topk_ids.is_contiguous() or topk_ids.numel() != y.shape[0] * y.shape[1]):
        raise RuntimeError("moe_sum_reduce: topk_ids must be contiguous int32 [T, topk]")
    check(lib.sgl_mi355_moe_sum_reduce(ptr(y), ptr(out), ptr(topk_ids), y.shape[0], y.shape[1], y.shape[2], int(num_experts),
                                       float(routed_scaling_factor), dtype_code(y.dtype), current_stream()))
