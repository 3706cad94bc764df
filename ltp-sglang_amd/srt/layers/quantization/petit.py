"""PetitNvFp4Config / PetitNvFp4LinearMethod: ModelOpt NVFP4 checkpoints as w4a16 -- fp4 (e2m1) weights with one e4m3 scale per
16 inputs and one f32 scale per tensor, 16-bit activations (python/sglang/srt/layers/quantization/petit.py:33-252; on a ROCm host
the reference sends every ``quant_method: modelopt`` FP4 checkpoint here, :107-110).  The arithmetic is this package's HIP
(petit_utils.py); the w4a4 ``modelopt_fp4`` method and MoE are out of scope."""
import logging
import re
from typing import Any, Dict, List, Optional

import torch
from torch.nn.parameter import Parameter

from .base_config import LinearMethodBase, QuantizationConfig, QuantizeMethodBase
from .petit_utils import apply_petit_nvfp4_linear, prepare_nvfp4_layer_for_petit, verify_petit_nvfp4_supported

logger = logging.getLogger(__name__)


class PetitNvFp4Config(QuantizationConfig):
    """Config class for Petit FP4."""

    def __init__(self, is_checkpoint_nvfp4_serialized: bool = False, kv_cache_quant_algo: str = None, group_size: int = None,
                 exclude_modules: List[str] = None) -> None:
        super().__init__()
        self.is_checkpoint_nvfp4_serialized = is_checkpoint_nvfp4_serialized
        if is_checkpoint_nvfp4_serialized:
            logger.warning("Detected nvfp4 checkpoint. Please note that the format is experimental and subject to change.")
        self.group_size = group_size
        self.kv_cache_quant_algo = kv_cache_quant_algo
        self.exclude_modules = exclude_modules

    @classmethod
    def get_name(cls) -> str:
        return "petit_nvfp4"

    @classmethod
    def get_supported_act_dtypes(cls) -> List[torch.dtype]:
        return [torch.bfloat16, torch.half]

    @classmethod
    def get_config_filenames(cls) -> List[str]:
        return ["hf_quant_config.json"]

    @classmethod
    def from_config(cls, config: Dict[str, Any]) -> "PetitNvFp4Config":
        quant_config = cls.get_from_keys(config, ["quantization"])
        quant_method = quant_config["quant_algo"]
        group_size = quant_config.get("group_size", None)
        verify_petit_nvfp4_supported(quant_method, group_size)
        kv_cache_quant_algo = quant_config["kv_cache_quant_algo"] or "auto"
        exclude_modules = quant_config.get("exclude_modules", None)
        if not (group_size and kv_cache_quant_algo and exclude_modules is not None):
            logger.warning(f"group_size: {group_size},kv_cache_quant_algo: {kv_cache_quant_algo},exclude_modules: {exclude_modules}")
            raise ValueError("NVFP4 quantization requires group size and kv_cache_quant_algo specified in hf_quant_config.json")
        return cls("NVFP4" in quant_method, kv_cache_quant_algo, group_size, exclude_modules)

    @classmethod
    def override_quantization_method(cls, hf_quant_cfg, user_quant) -> Optional[str]:
        return cls.get_name() if cls.is_petit_nvfp4_compatible(hf_quant_cfg) else None

    @classmethod
    def is_petit_nvfp4_compatible(cls, quant_config: Dict[str, Any]) -> bool:
        # petit.py:107-110 also asks is_hip(): this build has no other host
        return quant_config.get("quant_method", "").lower() == "modelopt"

    def is_layer_excluded(self, prefix: str, exclude_modules: list) -> bool:
        """``*`` in a pattern matches any run of characters; everything else is literal (petit.py:112-117)."""
        return any(re.fullmatch(".*".join(re.escape(part) for part in pattern.split("*")), prefix) for pattern in exclude_modules)

    def get_quant_method(self, layer: torch.nn.Module, prefix: str) -> Optional[QuantizeMethodBase]:
        from ..linear import LinearBase
        from .unquant import UnquantizedLinearMethod

        if isinstance(layer, LinearBase):
            exclude = self.exclude_modules or []
            if prefix in exclude or self.is_layer_excluded(prefix, exclude):   # is_layer_skipped (utils.py:21-56) or a pattern
                return UnquantizedLinearMethod()
            return PetitNvFp4LinearMethod(self)
        return None

    def get_scaled_act_names(self) -> List[str]:
        return []


class PetitNvFp4LinearMethod(LinearMethodBase):
    """NVFP4 linear.  Checkpoint tensors (petit.py:134-224), N = sum(output_partition_sizes), P = number of partitions:

        weight          uint8          [N, K/2]     two e2m1 values per byte, the even input in the low nibble
        weight_scale    float8_e4m3fn  [N, K/16]    one scale per 16 inputs
        weight_scale_2  float32        [P]          per-tensor scale of every merged partition -> their max
        input_scale     float32        [P]          loaded, folded into ``alpha``, then dropped: the activations stay 16-bit
    """

    def __init__(self, quant_config: PetitNvFp4Config):
        self.quant_config = quant_config

    def create_weights(self, layer, input_size_per_partition: int, output_partition_sizes: List[int], input_size: int,
                       output_size: int, params_dtype: torch.dtype, **extra_weight_attrs):
        if not self.quant_config.is_checkpoint_nvfp4_serialized:
            raise ValueError("NVFP4 quantization was selected,  dynamic quantization is not supported.")
        n = sum(output_partition_sizes)
        layer.logical_widths = output_partition_sizes
        layer.input_size_per_partition = input_size_per_partition
        layer.output_size_per_partition = n
        if input_size_per_partition % 16 != 0:
            raise ValueError("Unsupported model when in features size is not multiple of 16")
        parts = len(output_partition_sizes)
        groups = input_size_per_partition // self.quant_config.group_size
        layer.register_parameter("weight", Parameter(torch.empty(n, input_size_per_partition // 2, dtype=torch.uint8), requires_grad=False))
        layer.register_parameter("input_scale", Parameter(torch.empty(parts, dtype=torch.float32), requires_grad=False))
        layer.register_parameter("weight_scale_2", Parameter(torch.empty(parts, dtype=torch.float32), requires_grad=False))
        layer.register_parameter("weight_scale", Parameter(torch.empty(n, groups, dtype=torch.float8_e4m3fn), requires_grad=False))

    def process_weights_after_loading(self, layer) -> None:
        input_scale = layer.input_scale.max().to(torch.float32)
        weight_scale_2 = layer.weight_scale_2.max().to(torch.float32)
        layer.weight_scale_2 = Parameter(weight_scale_2, requires_grad=False)
        layer.alpha = Parameter(input_scale * weight_scale_2, requires_grad=False)
        prepare_nvfp4_layer_for_petit(layer)
        del layer.input_scale

    def apply(self, layer, x: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        return apply_petit_nvfp4_linear(input=x, weight=layer.weight, weight_scale=layer.weight_scale,
                                        weight_scale_2=layer.weight_scale_2, size_n=layer.output_size_per_partition,
                                        size_k=layer.input_size_per_partition, bias=bias,
                                        packed=getattr(layer, "nvfp4_packed", None))
