"""CPU: sgl_mi355_nvfp4_gemm rejects bad arguments through the status + message convention, and the form rule (no launch here)."""
import ctypes


def test_nvfp4_gemm_argument_errors_and_form(pkg):
    from ltp_sglang_amd import _cabi, sgl_kernel

    p = ctypes.c_void_p(16)
    rc = _cabi.lib.sgl_mi355_nvfp4_gemm(p, 192, p, p, p, 16, p, None, 4, 16, 192, 0, None, 0, None)
    assert rc == 1 and "K % 128" in _cabi.last_error()
    rc = _cabi.lib.sgl_mi355_nvfp4_gemm(p, 128, p, p, p, 16, None, None, 4, 16, 128, 0, None, 0, None)
    assert rc == 1 and "global_scale" in _cabi.last_error()
    assert sgl_kernel.nvfp4_gemm_form(64, 4096, 4096) == 0
    assert sgl_kernel.nvfp4_gemm_form(65, 4096, 4096) == 1
