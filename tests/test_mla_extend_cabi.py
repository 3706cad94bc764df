"""CPU: sgl_mi355_extend_attention's argument rules around the 576 / 512 MLA shape through the status + message convention.  Every
call here is refused or returns before a launch; the pointers are dummies."""
import ctypes

import pytest

K, KB = 4096, 1 << 20   # k_extend / k_buffer
OTHER = 8192


def _extend(lib, hd, dv, v_ext=K, v_buf=KB, tokens=16, mask=None, window=-1):
    p = ctypes.c_void_p(16)
    c = ctypes.c_void_p
    return lib.sgl_mi355_extend_attention(p, c(K), c(v_ext), p, 16 * hd, hd, hd, 16 * dv, c(KB), c(v_buf), hd, hd, hd, hd, p, p, p, None, 0,
                                          None, None, None, None, 2, tokens, 8, 16, 1, hd, dv, 0.1, 0.0, 1, 0, 0, 1.0, 1.0,
                                          mask, p if mask else None, 1, window, None)


@pytest.mark.parametrize("kwargs, message", [
    (dict(v_ext=OTHER), "first 512 columns of k_extend"),
    (dict(v_buf=OTHER), "first 512 columns of the key buffer"),
    (dict(mask=ctypes.c_void_p(64)), "(576, 512) on one kv head (MLA) take no custom_mask"),
    (dict(window=64), "(576, 512) on one kv head (MLA) take no sliding window"),
    (dict(hd=288, dv=256), "outside (0, 256]"),
], ids=["v_extend", "v_buffer", "custom_mask", "window", "288_256"])
def test_mla_extend_argument_errors(kwargs, message, pkg):
    from ltp_sglang_amd import _cabi

    args = dict(hd=576, dv=512)
    args.update(kwargs)
    assert _extend(_cabi.lib, **args) == 1 and message in _cabi.last_error()


def test_mla_extend_zero_tokens_is_a_no_op(pkg):
    from ltp_sglang_amd import _cabi

    assert _extend(_cabi.lib, 576, 512, tokens=0) == 0
