"""CPU: the host side of the block-wise fp8 linear -- C-ABI symbols and argument errors of sgl_mi355_fp8_blockwise_gemm, its form
choice, Fp8Config's weight_block_size validation and the torch op's schema (no kernel is launched)."""
import ctypes

import pytest

P = ctypes.c_void_p(64)   # a non-null, 16-byte aligned pointer: never dereferenced, every call below returns before a launch


def _call(lib, M, N, K, x=P, dtype=0):
    return lib.sgl_mi355_fp8_blockwise_gemm(x, K, P, K, P, N, P, K // 128, 1, P, K // 128, 1, None, M, N, K, dtype, None)


def test_symbols_and_argument_errors(pkg):
    from ltp_sglang_amd import _cabi

    names = [p[0] for p in _cabi.parse_header()]
    raw = ctypes.CDLL(_cabi.LIB_PATH)
    for n in ("sgl_mi355_fp8_blockwise_gemm", "sgl_mi355_fp8_blockwise_gemm_form"):
        assert n in names and hasattr(raw, n)
    lib = _cabi.lib
    for args, msg in (((4, 128, 192), "K=192"), ((4, 24, 128), "N=24"), ((4, 128, 128, None), "null pointer"),
                      ((4, 128, 128, P, 2), "out_dtype")):
        assert _call(lib, *args) == 1 and msg in _cabi.last_error(), (args, _cabi.last_error())
    assert _call(lib, 0, 128, 128) == 0   # empty batch: no launch
    form = lib.sgl_mi355_fp8_blockwise_gemm_form
    assert [form(m, 4096, 4096) for m in (1, 64, 65, 4096)] == [0, 0, 1, 1]


def test_fp8_config_weight_block_size(pkg):
    from ltp_sglang_amd.srt.layers.quantization.fp8 import Fp8Config, Fp8LinearMethod

    cfg = Fp8Config.from_config({"quant_method": "fp8", "activation_scheme": "dynamic", "weight_block_size": [128, 128]})
    assert cfg.weight_block_size == [128, 128] and Fp8LinearMethod(cfg).block_quant
    assert not Fp8LinearMethod(Fp8Config.from_config({"quant_method": "fp8", "activation_scheme": "static"})).block_quant
    for kw in (dict(activation_scheme="static", weight_block_size=[128, 128]), dict(weight_block_size=[128]),
               dict(is_checkpoint_fp8_serialized=False, weight_block_size=[128, 128])):
        with pytest.raises(ValueError):
            Fp8Config(**{"is_checkpoint_fp8_serialized": True, **kw})


def test_torch_op_schema(pkg):
    import torch

    from ltp_sglang_amd import sgl_kernel  # noqa: F401  (registers)

    want = "sgl_kernel::fp8_blockwise_scaled_mm(Tensor mat_a, Tensor mat_b, Tensor scales_a, Tensor scales_b, ScalarType out_dtype) -> Tensor"
    assert str(torch.ops.sgl_kernel.fp8_blockwise_scaled_mm.default._schema) == want
