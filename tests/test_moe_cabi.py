"""CPU: the MoE entry points' argument rules through the status + message convention, the form choice (host logic), and the loud
refusal of quantised experts.  No kernel is launched here."""
import ctypes

import pytest
import torch


def test_moe_entry_points_reject_bad_arguments(pkg):
    from ltp_sglang_amd import _cabi

    lib, p = _cabi.lib, ctypes.c_void_p(4096)
    gemm = lib.sgl_mi355_moe_grouped_gemm
    cases = [
        (lambda: lib.sgl_mi355_topk_softmax(None, p, p, 4, 8, 2, 0, 2, None), "topk_softmax: null"),
        (lambda: lib.sgl_mi355_topk_softmax(p, p, p, 4, 64, 33, 0, 2, None), "topk=33"),
        (lambda: lib.sgl_mi355_topk_softmax(p, p, p, 4, 513, 2, 0, 2, None), "num_experts=513"),
        (lambda: lib.sgl_mi355_moe_align_block_size(p, 8, 8, 16, None, 1024, p, p, p, 0, None, 0, None), "moe_align_block_size: null"),
        (lambda: gemm(p, None, p, None, p, p, p, 8, 2, 8, 64, 128, 16, 1, 0, None), "moe_grouped_gemm: null"),
        (lambda: gemm(p, p, p, None, p, p, p, 8, 2, 8, 64, 144, 16, 1, 0, None), "multiples of 32"),   # H = 144
        (lambda: gemm(p, p, p, None, p, p, p, 8, 1, 8, 144, 64, 16, 0, 0, None), "multiples of 32"),
        (lambda: gemm(p, p, p, None, p, p, p, 8, 2, 8, 64, 128, 64, 1, 0, None), "block_size=64"),
        (lambda: lib.sgl_mi355_moe_sum_reduce(p, None, None, 4, 2, 64, 8, 1.0, 0, None), "moe_sum_reduce: null"),
    ]
    for call, message in cases:
        assert call() == 1 and message in _cabi.last_error(), message


def test_moe_gemm_form_is_host_logic(pkg):
    from ltp_sglang_amd.sgl_kernel import moe_gemm_form

    assert moe_gemm_form(256, 256, 256, 7168) == 0
    assert moe_gemm_form(65536, 8, 1792, 4096) == 1
    assert moe_gemm_form(8 * 60, 60, 96, 160) == 0 and moe_gemm_form(8 * 60 + 1, 60, 96, 160) == 1   # the threshold is on P / E


@pytest.mark.parametrize("flag", [dict(use_fp8_w8a8=True), dict(use_int4_w4a16=True), dict(block_shape=[128, 128]),
                                  dict(w1_scale=torch.ones(1))])
def test_fused_experts_refuses_quantised_experts(pkg, flag):
    from ltp_sglang_amd.srt.layers.moe.fused_moe import fused_experts

    x, w1, w2 = torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(4, 64, 64, dtype=torch.bfloat16), torch.zeros(4, 64, 32, dtype=torch.bfloat16)
    topk = (torch.ones(2, 1), torch.zeros(2, 1, dtype=torch.int32), None)
    with pytest.raises(NotImplementedError, match=next(iter(flag))):
        fused_experts(x, w1, w2, topk, **flag)
