"""The M > 64 half of sgl_kernel.awq_gemm (the tiled int4 dequant-GEMM) against the float64 product of the oracle's dequantised
weights, and AWQLinearMethod.apply's route to it."""
import pytest
import torch

from oracle import quant as oq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def sk(pkg):
    from ltp_sglang_amd import sgl_kernel

    return sgl_kernel


def _awq_case(k, n, g, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    qw = torch.randint(-2**31, 2**31 - 1, (k, n // 8), generator=gen, dtype=torch.int32)
    qz = torch.randint(-2**31, 2**31 - 1, (k // g, n // 8), generator=gen, dtype=torch.int32)
    sc = (torch.rand(k // g, n, generator=gen) * 0.02 + 1e-3).to(dtype)
    return qw, qz, sc


@pytest.mark.parametrize("m,k,n,g,dtype,bias,split", [
    (65, 128, 16, 128, torch.float16, False, False),     # first M past the old limit; one k-block, one unit, ragged M and N tile
    (129, 384, 144, 32, torch.bfloat16, True, False),    # 128-row tile + 1-row tile, N tail, four scale groups, 3 k-blocks
    (200, 512, 272, 64, torch.float16, True, False),     # two scale groups per block, N tail of one unit past two tiles
    (257, 1024, 128, 256, torch.bfloat16, False, False), # two full row tiles + a 1-row tile, group spanning two blocks
    (65, 2048, 128, 128, torch.float16, True, True),     # one output tile: split-K through slabs + reduce
    (300, 3584, 256, 128, torch.bfloat16, True, True),   # 28 k-blocks: ragged last k-range
])
def test_awq_gemm_tiled_vs_float64(m, k, n, g, dtype, bias, split, sk):
    """Same gate as test_awq_gemm_vs_oracle applies to the M <= 64 kernel: same product, weights and accumulate type."""
    if split:
        assert sk.awq_gemm_tiled_kranges(m, n, k) > 1
    qw, qz, sc = _awq_case(k, n, g, dtype, seed=m + k)
    gen = torch.Generator().manual_seed(m)
    x = torch.randn(m, k, generator=gen).to(dtype)
    b = torch.randn(n, generator=gen).to(dtype) if bias else None
    qp, sz = sk.awq_repack(qw.to(DEV), sc.to(DEV), qz.to(DEV))
    y = sk.awq_gemm(x.to(DEV), qp, sz, g, None if b is None else b.to(DEV))
    ref = x.double() @ oq.awq_dequantize(qw, sc, qz, g).double()
    if b is not None:
        ref = ref + b.double()
    err = (y.cpu().double() - ref).abs().max().item()
    tol = (2e-2 if dtype == torch.bfloat16 else 3e-3) * max(1.0, ref.abs().max().item())
    print(f"max |y - ref| = {err:.3e}, gate {tol:.3e}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("m,k", [(65, 768), (130, 768), (260, 4608)])
def test_awq_gemm_tiled_exact_small_integers(m, k, sk):
    """Power-of-two scales, activations in {-2..2}: every product and partial sum is exact in f32 (|sum| <= 4608 * 60 in multiples
    of 1/8), so a wrong nibble, zero point, group index, fragment lane, k-range boundary or slab shows as a non-zero difference."""
    n, g = 96, 128
    gen = torch.Generator().manual_seed(11)
    qw = torch.randint(-2**31, 2**31 - 1, (k, n // 8), generator=gen, dtype=torch.int32)
    qz = torch.randint(-2**31, 2**31 - 1, (k // g, n // 8), generator=gen, dtype=torch.int32)
    sc = (2.0 ** torch.randint(-3, 2, (k // g, n), generator=gen).float()).to(torch.float16)
    x = torch.randint(-2, 3, (m, k), generator=gen).to(torch.float16)
    qp, sz = sk.awq_repack(qw.to(DEV), sc.to(DEV), qz.to(DEV))
    y = sk.awq_gemm(x.to(DEV), qp, sz, g)
    ref = (x.double() @ oq.awq_dequantize(qw, sc, qz, g).double()).to(torch.float16)
    assert torch.equal(y.cpu(), ref)


def test_awq_gemm_tiled_row_stride(sk):
    m, k, n, g = 150, 256, 64, 128
    qw, qz, sc = (t.to(DEV) for t in _awq_case(k, n, g, torch.bfloat16, seed=7))
    wide = torch.randn(m, k + 64, generator=torch.Generator().manual_seed(7)).to(torch.bfloat16).to(DEV)
    qp, sz = sk.awq_repack(qw, sc, qz)
    x = wide[:, :k]
    assert x.stride(0) == k + 64
    assert torch.equal(sk.awq_gemm(x, qp, sz, g), sk.awq_gemm(x.contiguous(), qp, sz, g))


@pytest.mark.parametrize("m", [80, 200])
def test_awq_linear_method_reaches_tiled_gemm(m, sk, pkg):
    """apply() must be awq_gemm on the layer's packed weight, bit for bit: the public route reaches the kernel."""
    from ltp_sglang_amd.srt.layers.quantization.awq import AWQConfig, AWQLinearMethod
    k, n, g = 1024, 256, 128
    qw, qz, sc = _awq_case(k, n, g, torch.bfloat16, seed=3)
    layer = torch.nn.Module()
    meth = AWQLinearMethod(AWQConfig(4, g, True))
    meth.create_weights(layer, k, [n], k, n, torch.bfloat16)
    layer.qweight.data, layer.qzeros.data, layer.scales.data = qw.to(DEV), qz.to(DEV), sc.to(DEV)
    meth.process_weights_after_loading(layer)
    gen = torch.Generator().manual_seed(m)
    x = torch.randn(m, k, generator=gen).to(torch.bfloat16).to(DEV)
    bias = torch.randn(n, generator=gen).to(torch.bfloat16).to(DEV)
    assert torch.equal(meth.apply(layer, x, bias), sk.awq_gemm(x, layer._awq_packed[0], layer._awq_packed[1], g, bias))
