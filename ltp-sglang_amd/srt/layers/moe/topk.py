"""Standard top-k routing (python/sglang/srt/layers/moe/topk.py:93-103, 335-361) on the HIP topk_softmax kernel."""
from typing import NamedTuple

import torch

from ....sgl_kernel.moe import topk_softmax


class StandardTopKOutput(NamedTuple):
    """Standard top-k output format (topk.py:93-98)."""

    topk_weights: torch.Tensor
    topk_ids: torch.Tensor
    router_logits: torch.Tensor


def fused_topk(hidden_states: torch.Tensor, gating_output: torch.Tensor, topk: int, renormalize: bool):
    """(topk_weights f32 [M, topk], topk_ids int32 [M, topk]): softmax over the experts, then top-k (topk.py:335-361)."""
    assert hidden_states.shape[0] == gating_output.shape[0], "Number of tokens mismatch"
    M, _ = hidden_states.shape
    topk_weights = torch.empty(M, topk, dtype=torch.float32, device=hidden_states.device)
    topk_ids = torch.empty(M, topk, dtype=torch.int32, device=hidden_states.device)
    topk_softmax(topk_weights, topk_ids, gating_output, renormalize)
    return topk_weights, topk_ids
