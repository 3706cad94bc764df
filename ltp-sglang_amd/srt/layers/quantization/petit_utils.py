"""Helpers of the petit_nvfp4 method (python/sglang/srt/layers/quantization/petit_utils.py:36-104).  The reference forwards to the
petit_kernel wheel (repack_nvfp4, process_nvfp4_scales, mul_nvfp4_a16); here the same three steps are this package's HIP
kernels: ``nvfp4_repack``, ``nvfp4_gemm`` and, for large M or shapes the fused kernel does not take, ``nvfp4_dequantize`` +
``dense_linear``."""
from typing import Optional, Tuple

import torch

from ....sgl_kernel import dense_linear, nvfp4_dequantize, nvfp4_gemm, nvfp4_repack

# Largest M routed to the fused kernel.  The rule is awq.py's: the largest M of tools/bench_nvfp4.py's sweep at which nvfp4_gemm
# beats nvfp4_dequantize + dense_linear on all four Llama-3-8B shapes in both dtypes (profiles/nvfp4_sweep.csv: x0.16 - x0.48 of
# the unfused time up to 64 rows, x0.36 - x0.84 at 128, x0.46 - x0.83 at 256; at 512 it still wins on seven of the eight
# (x0.65 - x0.89) but ties on gate_up in bf16 (x0.99 / x1.01 in the two runs); at 1024 it loses on qkv, o_proj and gate_up).
FUSED_MAX_M = 256


def _check_petit_nvfp4_supported(quant_method: str, group_size: Optional[int]) -> Tuple[bool, Optional[str]]:
    if quant_method != "NVFP4":
        return (False, "Petit currently only supports: NVFP4 quantizations in sglang. Please check the "
                       "`hf_quant_config.json` file for your model's quant configuration.")
    if group_size is not None and group_size != 16:
        return (False, "Petit currently only supports: group_size=16 quantizations.")
    return (True, None)


def verify_petit_nvfp4_supported(quant_method: str, group_size: Optional[int]) -> None:
    supported, error_msg = _check_petit_nvfp4_supported(quant_method, group_size)
    if not supported:
        raise ValueError(error_msg)


def prepare_nvfp4_layer_for_petit(layer: torch.nn.Module) -> None:
    """Load-time re-layout (petit_utils.py:61-75).  The reference overwrites ``weight`` / ``weight_scale`` with the wheel's
    layout; here the checkpoint tensors stay (nvfp4_dequantize reads them for large M) and the MFMA-fragment image is kept beside
    them as ``layer.nvfp4_packed = (qpacked, spacked)``, or None where the fused kernel does not take the shape (K % 128, N % 16)."""
    n, k = layer.output_size_per_partition, layer.input_size_per_partition
    layer.weight = torch.nn.Parameter(layer.weight.data.contiguous(), requires_grad=False)
    layer.weight_scale = torch.nn.Parameter(layer.weight_scale.data.contiguous(), requires_grad=False)
    layer.nvfp4_packed = None
    if layer.weight.is_cuda and k % 128 == 0 and n % 16 == 0:
        layer.nvfp4_packed = nvfp4_repack(layer.weight.data, layer.weight_scale.data)


def apply_petit_nvfp4_linear(input: torch.Tensor, weight: torch.Tensor, weight_scale: torch.Tensor, weight_scale_2: torch.Tensor,
                             size_n: int, size_k: int, bias: Optional[torch.Tensor] = None,
                             packed: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """y = (x @ W^T) * weight_scale_2 (+ bias), W[n][k] = e2m1 nibble * e4m3 group scale (petit_utils.py:78-104); ``weight`` /
    ``weight_scale`` are the checkpoint tensors, ``packed`` the image of prepare_nvfp4_layer_for_petit.

    * M <= FUSED_MAX_M with a packed image: ``nvfp4_gemm`` -- exact weights, f32 accumulation, the global scale and the bias
      applied in f32, ONE rounding to x's dtype (the reference adds the bias to the rounded product: two).
    * larger M, or no image (K % 128 != 0 or N % 16 != 0): ``nvfp4_dequantize`` with the global scale folded in (no extra pass
      over anything) + ``dense_linear``.  Rounding of this route: each weight is rounded once to x's dtype as
      T(W * weight_scale_2) (relative 2^-9 bf16 / 2^-12 f16; the unscaled W alone would be exact), f32 accumulation, bias in f32,
      one rounding of the output."""
    x2d = input.reshape(-1, input.shape[-1]).contiguous()
    out_shape = input.shape[:-1] + (size_n,)
    if x2d.shape[1] != size_k:
        raise ValueError(f"apply_petit_nvfp4_linear: input has {x2d.shape[1]} features, the layer {size_k}")
    if packed is not None and x2d.shape[0] <= FUSED_MAX_M:
        return nvfp4_gemm(x2d, packed[0], packed[1], weight_scale_2, bias).reshape(out_shape)
    w_nk = nvfp4_dequantize(weight, weight_scale, x2d.dtype, weight_scale_2)
    return dense_linear(x2d, w_nk, bias).reshape(out_shape)
