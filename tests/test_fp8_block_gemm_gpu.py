"""sgl_kernel.fp8_blockwise_scaled_mm (block-scaled fp8 GEMM: streaming form for M <= 64, tile form above) against the float64
product of the block-wise dequantised operands, and Fp8LinearMethod's block_quant route to it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def sk(pkg):
    from ltp_sglang_amd import sgl_kernel

    return sgl_kernel


def _m_major(s):
    return s.t().contiguous().t()


def _run(sk, x, w, sx, sw, dtype, bias=None, sx_m_major=False, sw_copy=False):
    """x [M, K], w [N, K] fp8; sx [M, K/128]; sw [ceil(N/128), K/128] (the checkpoint's weight_scale_inv layout)."""
    sx, sw = sx.to(DEV), sw.to(DEV)
    return sk.fp8_blockwise_scaled_mm(x.to(DEV), w.to(DEV).T, _m_major(sx) if sx_m_major else sx, sw.T.contiguous() if sw_copy else sw.T,
                                      dtype, None if bias is None else bias.to(DEV)).cpu()


def _ref(x, w, sx, sw, bias=None):
    xd = x.double() * sx.double().repeat_interleave(128, dim=1)
    wd = w.double() * sw.double().repeat_interleave(128, dim=0)[: w.shape[0]].repeat_interleave(128, dim=1)
    ref = xd @ wd.T
    return ref if bias is None else ref + bias.double()


def _random_case(m, k, n, dtype, bias, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=gen).to(torch.float8_e4m3fn)
    w = torch.randn(n, k, generator=gen).to(torch.float8_e4m3fn)
    sx = torch.rand(m, k // 128, generator=gen) * 0.02 + 1e-3
    sw = torch.rand((n + 127) // 128, k // 128, generator=gen) * 0.02 + 1e-3
    return x, w, sx, sw, (torch.randn(n, generator=gen).to(dtype) if bias else None)


@pytest.mark.parametrize("m,k,n,dtype,bias,sx_m_major", [
    (1, 128, 128, torch.bfloat16, False, False),    # one block; one live row of a streaming fragment
    (16, 384, 144, torch.float16, True, True),      # 16-column tail with its own scale row; 3 K blocks for 4 waves
    (64, 1024, 256, torch.bfloat16, True, False),   # last streaming M; four full row fragments; two K blocks per wave
    (65, 128, 128, torch.float16, False, True),     # first tile-form M; ragged row tile; single slice
    (129, 384, 144, torch.bfloat16, True, False),   # full row tile + one-row tile; N tail
    (257, 1024, 384, torch.float16, True, True),    # 3 x 3 tiles: the XCD remap
])
def test_blockwise_mm_vs_float64(m, k, n, dtype, bias, sx_m_major, sk):
    """Gate of test_awq_tiled_gemm_gpu.py for this product type (fp8 operands, f32 accumulation, one rounding to the output type)."""
    assert sk.fp8_blockwise_gemm_form(m, n, k) == (0 if m <= 64 else 1)
    x, w, sx, sw, b = _random_case(m, k, n, dtype, bias, seed=m + k)
    y = _run(sk, x, w, sx, sw, dtype, b, sx_m_major)
    ref = _ref(x, w, sx, sw, b)
    err = (y.double() - ref).abs().max().item()
    tol = (2e-2 if dtype == torch.bfloat16 else 3e-3) * max(1.0, ref.abs().max().item())
    print(f"max |y - ref| = {err:.3e}, gate {tol:.3e}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("m,k", [(7, 256), (64, 1024), (65, 256), (130, 1024)])
def test_blockwise_mm_exact_small_integers(m, k, sk):
    """fp8 values in -2..2, power-of-two scales 2^-3..2^1: every block sum and running sum is exact in f32 (|sum| <= 8 * 128 * 4 * 4
    in multiples of 2^-6: 20 bits), so a wrong lane, scale row, K-block index, tail column or wave reduction is a non-zero difference."""
    n = 144
    gen = torch.Generator().manual_seed(11)
    x = torch.randint(-2, 3, (m, k), generator=gen).float().to(torch.float8_e4m3fn)
    w = torch.randint(-2, 3, (n, k), generator=gen).float().to(torch.float8_e4m3fn)
    sx = 2.0 ** torch.randint(-3, 2, (m, k // 128), generator=gen).float()
    sw = 2.0 ** torch.randint(-3, 2, (2, k // 128), generator=gen).float()
    assert torch.equal(_run(sk, x, w, sx, sw, torch.float16), _ref(x, w, sx, sw).to(torch.float16))


@pytest.mark.parametrize("m", [32, 200])
def test_blockwise_mm_scale_layouts_bit_identical(m, sk):
    x, w, sx, sw, b = _random_case(m, 512, 272, torch.bfloat16, True, seed=m)
    y = _run(sk, x, w, sx, sw, torch.bfloat16, b)
    assert torch.equal(y, _run(sk, x, w, sx, sw, torch.bfloat16, b, sx_m_major=True))
    assert torch.equal(y, _run(sk, x, w, sx, sw, torch.bfloat16, b, sw_copy=True))


@pytest.mark.parametrize("m", [32, 200])
def test_fp8_block_linear_method_route(m, sk, pkg):
    """apply() on a block-quantised layer is per_token_group_quant_fp8 + fp8_blockwise_scaled_mm on the layer's tensors, bit for bit."""
    from ltp_sglang_amd.srt.layers.quantization.fp8 import Fp8Config, Fp8LinearMethod
    from ltp_sglang_amd.srt.layers.quantization.fp8_kernel import per_token_group_quant_fp8
    k, n = 512, 384
    _, w, _, sw, b = _random_case(m, k, n, torch.bfloat16, True, seed=3)
    meth = Fp8LinearMethod(Fp8Config.from_config({"quant_method": "fp8", "activation_scheme": "dynamic", "weight_block_size": [128, 128]}))
    layer = torch.nn.Module()
    meth.create_weights(layer, k, [n], k, n, torch.bfloat16)
    assert tuple(layer.weight_scale_inv.shape) == (3, 4) and layer.weight.dtype == torch.float8_e4m3fn
    layer.weight.data, layer.weight_scale_inv.data = w.to(DEV), sw.to(DEV)
    meth.process_weights_after_loading(layer)
    x = torch.randn(2, m // 2, k, generator=torch.Generator().manual_seed(m)).to(torch.bfloat16).to(DEV)
    xq, xs = per_token_group_quant_fp8(x.view(m, k), 128)
    want = sk.fp8_blockwise_scaled_mm(xq, layer.weight.T, xs, layer.weight_scale_inv.T, torch.bfloat16, b.to(DEV))
    got = meth.apply(layer, x, b.to(DEV))
    assert got.shape == (2, m // 2, n) and torch.equal(got.view(m, n), want)
