"""sgl_kernel.int8_scaled_mm (int8 w8a8 GEMM: streaming form for M <= 64, tile form with split-K above) against the float64 product,
per_token_quant_int8 against its formula in f32 torch, and W8A8Int8LinearMethod's route to both."""
import ctypes

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def sk(pkg):
    from ltp_sglang_amd import sgl_kernel

    return sgl_kernel


def _ref(x, w, sa, sb):
    """The scaled product without bias; the integer product is exact in float64."""
    return (x.double() @ w.double().T) * sa.double().view(-1, 1) * sb.double().view(1, -1)


def _case(m, k, n, dtype, bias, seed):
    """int8 over the full range; scales in [0.5, 1.5) * 2^-7, so |ref| <= K * 2^14 * 2.25 * 2^-14 < 65504 for K <= 2112."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-128, 128, (m, k), generator=gen, dtype=torch.int8)
    w = torch.randint(-128, 128, (n, k), generator=gen, dtype=torch.int8)
    sa, sb = ((torch.rand(r, generator=gen) + 0.5) * 2.0 ** -7 for r in (m, n))
    return x, w, sa, sb, (torch.randn(n, generator=gen).to(dtype) if bias else None)


def _run(sk, x, w, sa, sb, dtype, bias=None, pad=0):
    xd = x.to(DEV)
    if pad:   # rows `pad` bytes apart beyond K
        xd = torch.zeros(x.shape[0], x.shape[1] + pad, dtype=torch.int8, device=DEV)
        xd[:, : x.shape[1]] = x.to(DEV)
        xd = xd[:, : x.shape[1]]
    return sk.int8_scaled_mm(xd, w.to(DEV).t(), sa.to(DEV), sb.to(DEV), dtype, None if bias is None else bias.to(DEV)).cpu()


@gpu
@pytest.mark.parametrize("m,k,n,dtype,bias,pad", [
    (1, 64, 16, torch.bfloat16, False, 0),       # one MFMA step (a half slice), one live row
    (16, 192, 48, torch.float16, True, 64),      # 2 slices for 4 waves, the second half; N tail
    (64, 1024, 256, torch.bfloat16, True, 0),    # last streaming M; full row fragments
    (48, 128, 8192, torch.float16, True, 0),     # streaming form with 32 weight rows per workgroup
    (65, 64, 16, torch.float16, False, 16),      # first tile M; ragged row tile; single half slice
    (129, 448, 144, torch.bfloat16, True, 0),    # full tile plus a one-row tile; half-slice K tail; N tail
    (257, 1024, 384, torch.float16, True, 64),   # 3 x 3 tiles, the block remap; two split-K ranges
    (100, 2112, 48, torch.bfloat16, False, 0),   # one tile, four uneven split-K ranges, the last ending in a half slice
])
def test_int8_scaled_mm_vs_float64(m, k, n, dtype, bias, pad, sk):
    """|y - ref| <= u |ref| (half an ulp of the output) + 2^-21 (|p| + |bias|) (the epilogue's four f32 roundings) + 2^-25 (f16's
    subnormal spacing), per element."""
    assert sk.int8_gemm_form(m, n, k) == (0 if m <= 64 else 1)
    x, w, sa, sb, b = _case(m, k, n, dtype, bias, seed=m + k)
    p = _ref(x, w, sa, sb)
    babs = 0.0 if b is None else b.double().abs()
    ref = p if b is None else p + b.double()
    assert ref.abs().max().item() < 65504
    gate = (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11) * ref.abs() + 2.0 ** -21 * (p.abs() + babs) + 2.0 ** -25
    err = (_run(sk, x, w, sa, sb, dtype, b, pad).double() - ref).abs()
    print(f"max err / gate = {(err / gate).max().item():.3f}")
    assert (err <= gate).all(), (err / gate).max().item()


@gpu
@pytest.mark.parametrize("m", [8, 72])
def test_int8_scaled_mm_signedness_and_range(m, sk):
    """Sums of 2^26 and -127 * 2^19: an unsigned or saturating path, or a 16-bit intermediate, cannot produce them."""
    k, n = 4096, 16
    x = torch.full((m, k), -128, dtype=torch.int8)
    w = torch.full((n, k), -128, dtype=torch.int8)
    w[1::2] = 127
    s = torch.full((max(m, n),), 2.0 ** -20)
    y = _run(sk, x, w, s[:m], s[:n], torch.float16)
    assert torch.equal(y, _ref(x, w, s[:m], s[:n]).to(torch.float16))


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_int8_scaled_mm_form_independent(dtype, sk):
    """The same rows through the streaming form, the tile form with split-K (M = 128) and without (M = 576): the same bits."""
    x, w, sa, sb, b = _case(576, 1024, 256, dtype, True, seed=5)
    y576 = _run(sk, x, w, sa, sb, dtype, b)
    y128 = _run(sk, x[:128], w, sa[:128], sb, dtype, b)
    y64 = _run(sk, x[:64], w, sa[:64], sb, dtype, b)
    assert torch.equal(y128[:64], y64) and torch.equal(y576[:128], y128)


@gpu
@pytest.mark.parametrize("m,k,dtype", [
    (1, 64, torch.float16), (37, 64, torch.bfloat16), (4, 8192, torch.bfloat16),   # the register-resident row kernel
    (513, 64, torch.float16), (2049, 64, torch.bfloat16),                          # workgroup per row; wave per row
])
def test_per_token_quant_int8(m, k, dtype, pkg):
    from ltp_sglang_amd.srt.layers.quantization.int8_kernel import per_token_quant_int8

    x = torch.randn(m, k, generator=torch.Generator().manual_seed(m)).to(dtype)
    x[m // 2] = 0                                  # all-zero row: scale 1e-10 / 127, q = 0
    x[m - 1, :2] = torch.tensor([9.0, -9.0])       # +-absmax: q = +-127, never -128
    q, s = per_token_quant_int8(x.to(DEV))
    xf = x.float()
    absmax = xf.abs().amax(dim=1, keepdim=True).clamp(min=1e-10)
    v = xf * (torch.full_like(absmax, 127.0) / absmax)
    assert torch.equal(s.cpu(), absmax / torch.full_like(absmax, 127.0))
    assert torch.equal(q.cpu(), (v.sign() * (v.abs() + 0.5).floor()).to(torch.int8))
    if m > 1:
        assert q[m - 1, :2].tolist() == [127, -127] and q.min().item() == -127


@gpu
@pytest.mark.parametrize("m", [32, 200])
def test_w8a8_int8_linear_method_route(m, sk, pkg):
    """apply() is per_token_quant_int8 + int8_scaled_mm on the layer's tensors, bit for bit."""
    from ltp_sglang_amd.srt.layers.linear import LinearBase
    from ltp_sglang_amd.srt.layers.quantization import get_quantization_config
    from ltp_sglang_amd.srt.layers.quantization.int8_kernel import per_token_quant_int8
    from ltp_sglang_amd.srt.layers.quantization.unquant import UnquantizedLinearMethod
    from ltp_sglang_amd.srt.layers.quantization.w8a8_int8 import W8A8Int8Config, W8A8Int8LinearMethod

    assert get_quantization_config("w8a8_int8") is W8A8Int8Config and W8A8Int8Config.get_name() == "w8a8_int8"
    cfg = W8A8Int8Config.from_config({"ignore": ["lm_head"]})
    lin = LinearBase(64, 16, quant_config=cfg, prefix="model.layers.0.mlp.down_proj")
    assert isinstance(lin.quant_method, W8A8Int8LinearMethod)
    assert isinstance(LinearBase(64, 16, quant_config=cfg, prefix="lm_head").quant_method, UnquantizedLinearMethod)
    k, n = 512, 384
    _, w, _, sb, b = _case(m, k, n, torch.bfloat16, True, seed=3)
    meth, layer = lin.quant_method, torch.nn.Module()
    meth.create_weights(layer, k, [n], k, n, torch.bfloat16)
    assert layer.weight.dtype == torch.int8 and tuple(layer.weight.shape) == (n, k) and tuple(layer.weight_scale.shape) == (n, 1)
    layer.weight.data, layer.weight_scale.data = w.to(DEV), sb.view(n, 1).to(DEV)
    meth.process_weights_after_loading(layer)
    x = torch.randn(2, m // 2, k, generator=torch.Generator().manual_seed(m)).to(torch.bfloat16).to(DEV)
    xq, xs = per_token_quant_int8(x.view(m, k))
    want = sk.int8_scaled_mm(xq, layer.weight, xs, layer.weight_scale, torch.bfloat16, b.to(DEV))
    got = meth.apply(layer, x, b.to(DEV))
    assert got.shape == (2, m // 2, n) and torch.equal(got.view(m, n), want)


def test_int8_gemm_argument_errors(pkg):
    """CPU: the launcher's domain checks return before any launch; the form boundary; the wrapper's first check."""
    from ltp_sglang_amd import _cabi, sgl_kernel

    P = ctypes.c_void_p(64)   # non-null, 16-byte aligned, never dereferenced
    for (m, n, k, dt), msg in (((4, 16, 96, 0), "K=96"), ((4, 24, 64, 0), "N=24"), ((4, 16, 131072, 0), "below 131072"),
                               ((4, 16, 64, 3), "out_dtype")):
        assert _cabi.lib.sgl_mi355_int8_gemm(P, k, P, k, P, n, P, P, None, m, n, k, dt, None, 0, None) == 1
        assert msg in _cabi.last_error(), _cabi.last_error()
    assert [sgl_kernel.int8_gemm_form(m, 4096, 4096) for m in (1, 64, 65, 4096)] == [0, 0, 1, 1]
    a = torch.zeros(4, 64, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="mat_a must be a CUDA tensor"):
        sgl_kernel.int8_scaled_mm(a, a.t(), torch.ones(4), torch.ones(4), torch.float16)
    want = "sgl_kernel::int8_scaled_mm(Tensor mat_a, Tensor mat_b, Tensor scales_a, Tensor scales_b, ScalarType out_dtype, Tensor? bias) -> Tensor"
    assert str(torch.ops.sgl_kernel.int8_scaled_mm.default._schema) == want
