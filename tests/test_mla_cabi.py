"""CPU: sgl_mi355_decode_attention's argument rules around the 576 / 512 MLA shape through the status + message convention (no
launch here), and the aliasing of MLATokenToKVPool's value view."""
import ctypes

import torch


def _decode(lib, k, v, hd, dv, kv_dtype=0):
    p = ctypes.c_void_p(16)
    return lib.sgl_mi355_decode_attention(p, 16 * hd, k, v, hd, hd, hd, hd, p, 16 * dv, p, p, None, 0, None, None, p, p, p, 8,
                                          2, 16, 1, hd, dv, 0.1, 0.0, 0, kv_dtype, 1.0, 1.0, None)


def test_mla_decode_argument_errors(pkg):
    from ltp_sglang_amd import _cabi

    k, v = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    assert _decode(_cabi.lib, k, v, 576, 512) == 1 and "first 512 columns of the key buffer" in _cabi.last_error()
    assert _decode(_cabi.lib, k, k, 576, 512, kv_dtype=_cabi.FP8_E4M3) == 1 and "fp8_e4m3 latent cache" in _cabi.last_error()
    assert _decode(_cabi.lib, k, v, 288, 256) == 1 and "outside (0, 256]" in _cabi.last_error()


def test_mla_pool_value_is_a_view_of_the_key(pkg):
    from ltp_sglang_amd.srt.mem_cache.memory_pool import MLATokenToKVPool

    pool = MLATokenToKVPool(7, 1, torch.bfloat16, 512, 64, 2, "cpu", False)
    k, v = pool.get_kv_buffer(1)
    assert tuple(k.shape) == (8, 1, 576) and v.shape[-1] == 512
    assert v.data_ptr() == k.data_ptr() and v.stride(0) == k.stride(0)
