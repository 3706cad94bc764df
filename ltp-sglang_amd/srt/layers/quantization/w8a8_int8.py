"""W8A8Int8Config / W8A8Int8LinearMethod: static per-channel symmetric int8 weights, dynamic per-token symmetric int8 activations
(python/sglang/srt/layers/quantization/w8a8_int8.py:178-386; linear only -- W8A8Int8MoEMethod and the NPU classes are out of
scope)."""
import re
from typing import Any, Dict, List, Optional

import torch
from torch.nn.parameter import Parameter

from ....sgl_kernel import int8_scaled_mm
from .base_config import LinearMethodBase, QuantizationConfig
from .int8_kernel import per_token_quant_int8
from .unquant import UnquantizedLinearMethod


def per_channel_quant_int8(weight: torch.Tensor):
    """[N, K] half/float weight -> (int8 [N, K], scale f32 [N, 1]): the per-row form of per_token_quant_int8's arithmetic, for
    weights that arrive unquantised (the sibling of per_channel_quant_fp8)."""
    wf = weight.float()
    absmax = wf.abs().amax(dim=1, keepdim=True).clamp(min=1e-10)
    v = wf * (torch.full_like(absmax, 127.0) / absmax)
    return (v.sign() * (v.abs() + 0.5).floor()).to(torch.int8), absmax / 127.0


class W8A8Int8Config(QuantizationConfig):
    def __init__(self, quant_config: Optional[Dict[str, Any]] = None):
        super().__init__()
        quant_config = quant_config or {}
        self.quant_description = quant_config
        self.is_dynamic = quant_config.get("is_dynamic", False)
        self.ignore = quant_config.get("ignore") or []
        self.packed_modules_mapping = quant_config.get("packed_modules_mapping") or {}

    @classmethod
    def get_name(cls) -> str:
        return "w8a8_int8"

    def get_supported_act_dtypes(self) -> List[torch.dtype]:
        return [torch.float16, torch.bfloat16]

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> "W8A8Int8Config":
        return cls(config)

    def _ignored(self, name: str) -> bool:   # check_equal_or_regex_match, compressed_tensors/utils.py:76-84,155-173
        return any(re.match(t[3:], name) if t.startswith("re:") else t == name for t in self.ignore)

    def get_quant_method(self, layer: torch.nn.Module, prefix: str):
        from ..linear import LinearBase

        # should_ignore_layer (compressed_tensors/utils.py:21-73): a fused layer is ignored when its checkpoint shards are
        proj = prefix.split(".")[-1]
        if proj in self.packed_modules_mapping and not self._ignored(prefix):
            shards = [self._ignored(prefix.replace(proj, s)) for s in self.packed_modules_mapping[proj]]
            if any(shards) != all(shards):
                raise ValueError(f"Found a different quantization schemes for {proj} in {prefix}. vLLM requires all to use the same scheme.")
            ignored = all(shards)
        else:
            ignored = self._ignored(prefix)
        if ignored:
            return UnquantizedLinearMethod()
        return W8A8Int8LinearMethod(self) if isinstance(layer, LinearBase) else None


class W8A8Int8LinearMethod(LinearMethodBase):
    def __init__(self, quantization_config: W8A8Int8Config):
        self.quantization_config = quantization_config

    def create_weights(self, layer, input_size_per_partition: int, output_partition_sizes: List[int], input_size: int,
                       output_size: int, params_dtype: torch.dtype, **extra_weight_attrs):
        n = sum(output_partition_sizes)
        layer.logical_widths = output_partition_sizes
        layer.register_parameter("weight", Parameter(torch.empty(n, input_size_per_partition, dtype=torch.int8), requires_grad=False))
        layer.register_parameter("weight_scale", Parameter(torch.empty((n, 1), dtype=torch.float32), requires_grad=False))

    def process_weights_after_loading(self, layer) -> None:
        # stored as the [K, N] column-major view so that apply() hands int8_scaled_mm its mat_b (w8a8_int8.py:332-333)
        layer.weight = Parameter(layer.weight.data.t(), requires_grad=False)
        layer.weight_scale = Parameter(layer.weight_scale.data, requires_grad=False)

    def apply(self, layer, x: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        x_q, x_scale = per_token_quant_int8(x2)
        out = int8_scaled_mm(x_q, layer.weight, x_scale, layer.weight_scale, out_dtype=x.dtype, bias=bias)
        return out.view(x.shape[:-1] + (out.shape[-1],))
