"""int8 helper with the reference's name (python/sglang/srt/layers/quantization/int8_kernel.py, imported at w8a8_int8.py:28)."""
from typing import Tuple

import torch

from ....sgl_kernel import sgl_per_token_quant_int8


def per_token_quant_int8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [..., K] bf16 / f16 -> (x_q int8 like x, scale f32 [..., 1]): per row absmax = max(max |x|, 1e-10), scale = absmax / 127,
    x_q = round_half_away_from_zero(x * (127 / absmax)), all in f32."""
    assert x.is_contiguous(), "`x` is not contiguous"
    x_q = torch.empty_like(x, device=x.device, dtype=torch.int8)
    scale = torch.empty(x.shape[:-1] + (1,), device=x.device, dtype=torch.float32)
    sgl_per_token_quant_int8(x.view(-1, x.shape[-1]), x_q.view(-1, x.shape[-1]), scale.view(-1, 1))
    return x_q, scale
