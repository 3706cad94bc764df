"""Fused MoE for unquantised 16-bit experts (python/sglang/srt/layers/moe/fused_moe_triton/fused_moe.py: moe_align_block_size
549-619, fused_experts 1224-1296, fused_experts_impl 1391-1631, fused_moe 1634-1714) on the HIP kernels of csrc/moe_align.hip and
csrc/moe_gemm.hip.

One linear chain of launches: align -> grouped GEMM 1 with SiluAndMul in its epilogue -> grouped GEMM 2 times the router weight ->
sum over topk.  No launch depends on a value read back from the device, so the whole of fused_experts is capturable in
torch.cuda.graph and a replay follows new routing.  w1 [E, 2 I, H] (rows [0, I) gate, [I, 2 I) up), w2 [E, H, I]."""
from typing import List, Optional, Tuple

import torch

from ....sgl_kernel import moe as _ops


def moe_align_block_size(topk_ids: torch.Tensor, block_size: int, num_experts: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(sorted_token_ids, expert_ids, num_tokens_post_padded) of fused_moe.py:549-619: every expert's pairs (ascending) padded to
    a multiple of block_size with topk_ids.numel(), one expert id per block, the padded total.  Ids outside [0, num_experts) are
    left out.  Entries past num_tokens_post_padded[0] are undefined."""
    max_num_tokens_padded = topk_ids.numel() + (num_experts + 1) * (block_size - 1)
    sorted_ids = torch.empty((max_num_tokens_padded,), dtype=torch.int32, device=topk_ids.device)
    max_num_m_blocks = (max_num_tokens_padded + block_size - 1) // block_size
    expert_ids = torch.empty((max_num_m_blocks,), dtype=torch.int32, device=topk_ids.device)
    num_tokens_post_pad = torch.empty((1), dtype=torch.int32, device=topk_ids.device)
    cumsum_buffer = torch.empty((num_experts + 2,), dtype=torch.int32, device=topk_ids.device)
    _ops.moe_align_block_size(topk_ids, num_experts, block_size, sorted_ids, expert_ids, num_tokens_post_pad, cumsum_buffer, False)
    return sorted_ids, expert_ids, num_tokens_post_pad


# tools/bench_moe.py times both GEMM forms on one shape through this: 16 / 128 overrides moe_gemm_form's choice (None: no override)
_FORCE_BLOCK_SIZE = None


def _reject_quantised(**flags) -> None:
    for name, value in flags.items():
        if value is not None and value is not False:
            raise NotImplementedError(f"fused_experts: {name} is not served: this build has unquantised bf16 / f16 experts only")


def fused_experts(
    hidden_states: torch.Tensor,
    w1: torch.Tensor,
    w2: torch.Tensor,
    topk_output,
    inplace: bool = False,
    activation: str = "silu",
    apply_router_weight_on_input: bool = False,
    use_fp8_w8a8: bool = False,
    use_int8_w8a8: bool = False,
    use_int8_w8a16: bool = False,
    use_int4_w4a16: bool = False,
    per_channel_quant: bool = False,
    w1_scale: Optional[torch.Tensor] = None,
    w2_scale: Optional[torch.Tensor] = None,
    w1_zp: Optional[torch.Tensor] = None,
    w2_zp: Optional[torch.Tensor] = None,
    a1_scale: Optional[torch.Tensor] = None,
    a2_scale: Optional[torch.Tensor] = None,
    block_shape: Optional[List[int]] = None,
    no_combine: bool = False,
    routed_scaling_factor: Optional[float] = None,
):
    _reject_quantised(use_fp8_w8a8=use_fp8_w8a8, use_int8_w8a8=use_int8_w8a8, use_int8_w8a16=use_int8_w8a16,
                      use_int4_w4a16=use_int4_w4a16, per_channel_quant=per_channel_quant, w1_scale=w1_scale, w2_scale=w2_scale,
                      w1_zp=w1_zp, w2_zp=w2_zp, a1_scale=a1_scale, a2_scale=a2_scale, block_shape=block_shape)
    if activation != "silu":
        raise ValueError(f"Unsupported activation: {activation=} (silu only)")
    topk_weights, topk_ids = topk_output[0], topk_output[1]
    assert not (inplace and no_combine), "no combine + inplace makes no sense"
    assert hidden_states.dim() == 2 and hidden_states.is_contiguous(), "Hidden_states must be contiguous"
    assert w1.is_contiguous(), "Expert weights1 must be contiguous"
    assert w2.is_contiguous(), "Expert weights2 must be contiguous"
    assert topk_weights.shape == topk_ids.shape, "topk shape mismatch"
    if hidden_states.dtype not in (torch.bfloat16, torch.float16) or w1.dtype != hidden_states.dtype or w2.dtype != hidden_states.dtype:
        raise RuntimeError("fused_experts: hidden_states, w1 and w2 must all be bfloat16 or all float16")
    T, H = hidden_states.shape
    E, N2, _ = w1.shape
    I = N2 // 2
    assert w1.shape[2] == H, "Hidden size mismatch"
    assert N2 == 2 * I and tuple(w2.shape) == (E, H, I), "w1 [E, 2I, H] and w2 [E, H, I] expected"
    if H % 32 != 0 or I % 32 != 0:
        raise RuntimeError(f"fused_experts: hidden size {H} and intermediate size {I} must be multiples of 32")
    topk = topk_ids.shape[1]
    assert topk_ids.shape[0] == T, "Number of tokens mismatch"
    if apply_router_weight_on_input:
        assert topk == 1, "Only support topk=1 when `apply_router_weight_on_input` is True"
    scale = 1.0 if routed_scaling_factor is None else float(routed_scaling_factor)
    dev, dtype = hidden_states.device, hidden_states.dtype

    if no_combine:
        out = torch.empty((T, topk, H), device=dev, dtype=dtype)
    elif inplace:
        out = hidden_states
    else:
        out = torch.empty_like(hidden_states)
    if T == 0:
        return out

    ids = topk_ids if topk_ids.dtype == torch.int32 else topk_ids.to(torch.int32)
    ids = ids.contiguous()
    weights = topk_weights.to(torch.float32).contiguous().view(-1)
    P = T * topk
    block_size = _FORCE_BLOCK_SIZE or (16 if _ops.moe_gemm_form(P, E, I, H) == 0 else 128)
    sorted_ids, expert_ids, num_post_pad = moe_align_block_size(ids, block_size, E)

    a2 = torch.empty((P, I), device=dev, dtype=dtype)
    _ops.moe_grouped_gemm(hidden_states, w1, a2, weights if apply_router_weight_on_input else None, sorted_ids, expert_ids,
                          num_post_pad, block_size, topk, True)
    direct = no_combine or (topk == 1 and scale == 1.0)   # GEMM 2 writes the result itself (fused_moe.py:1561-1565, 1592-1593)
    y = out.view(P, H) if direct else torch.empty((P, H), device=dev, dtype=dtype)
    _ops.moe_grouped_gemm(a2, w2, y, None if apply_router_weight_on_input else weights, sorted_ids, expert_ids, num_post_pad,
                          block_size, 1, False)
    if not direct:
        _ops.moe_sum_reduce(y.view(T, topk, H), out, scale, ids, E)
    return out


def fused_moe(
    hidden_states: torch.Tensor,
    w1: torch.Tensor,
    w2: torch.Tensor,
    topk_output,
    inplace: bool = False,
    activation: str = "silu",
    apply_router_weight_on_input: bool = False,
    use_fp8_w8a8: bool = False,
    use_int8_w8a8: bool = False,
    use_int8_w8a16: bool = False,
    use_int4_w4a16: bool = False,
    per_channel_quant: bool = False,
    w1_scale: Optional[torch.Tensor] = None,
    w2_scale: Optional[torch.Tensor] = None,
    w1_zp: Optional[torch.Tensor] = None,
    w2_zp: Optional[torch.Tensor] = None,
    a1_scale: Optional[torch.Tensor] = None,
    a2_scale: Optional[torch.Tensor] = None,
    block_shape: Optional[List[int]] = None,
    no_combine: bool = False,
    routed_scaling_factor: Optional[float] = None,
) -> torch.Tensor:
    """A Mixture-of-Experts layer over the expert weights w1 and w2 and a top-k gating result (fused_moe.py:1634-1714)."""
    return fused_experts(
        hidden_states, w1, w2, topk_output, inplace=inplace, activation=activation,
        apply_router_weight_on_input=apply_router_weight_on_input, use_fp8_w8a8=use_fp8_w8a8, use_int8_w8a8=use_int8_w8a8,
        use_int8_w8a16=use_int8_w8a16, use_int4_w4a16=use_int4_w4a16, per_channel_quant=per_channel_quant, w1_scale=w1_scale,
        w2_scale=w2_scale, w1_zp=w1_zp, w2_zp=w2_zp, a1_scale=a1_scale, a2_scale=a2_scale, block_shape=block_shape,
        no_combine=no_combine, routed_scaling_factor=routed_scaling_factor,
    )
