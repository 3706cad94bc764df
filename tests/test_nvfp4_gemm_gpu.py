"""NVFP4 (w4a16): sgl_kernel.nvfp4_dequantize / nvfp4_repack / nvfp4_gemm against a float64 product formed here from the checkpoint
tensors, and the petit_nvfp4 method's route to them."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
F16, BF16 = torch.float16, torch.bfloat16


@pytest.fixture(scope="module")
def sk(pkg):
    from ltp_sglang_amd import sgl_kernel

    return sgl_kernel


def _dense(weight, weight_scale):
    """W [N, K] in float32 (exact): low nibble first, one scale per 16 inputs."""
    nib = torch.stack((weight & 0xF, weight >> 4), dim=-1).reshape(weight.shape[0], -1).long()
    return E2M1[nib] * weight_scale.float().repeat_interleave(16, 1)


def _case(n, k, gen, scale_bytes=(0x08, 0x41)):
    """random weight bytes; scale bytes 0x08..0x40 are the e4m3 values in [2^-6, 2]"""
    w = torch.randint(0, 256, (n, k // 2), generator=gen, dtype=torch.uint8)
    s = torch.randint(scale_bytes[0], scale_bytes[1], (n, k // 16), generator=gen, dtype=torch.uint8).view(torch.float8_e4m3fn)
    return w, s


def _gate(y, ref, dtype):
    err = (y.cpu().double() - ref).abs().max().item()
    tol = (2e-2 if dtype == BF16 else 3e-3) * max(1.0, ref.abs().max().item())
    print(f"max |y - ref| = {err:.3e}, gate {tol:.3e}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_nvfp4_dequantize_bit_exact(dtype, sk):
    """Every finite scale byte (subnormals, zeros, negatives) and every weight byte; W is exactly representable in both dtypes."""
    gen = torch.Generator().manual_seed(1)
    finite = [b for b in range(256) if b & 0x7F != 0x7F]
    sb = torch.tensor(finite + [0x38, 0xB8], dtype=torch.uint8)[torch.randperm(256, generator=gen)]
    s = sb.reshape(32, 8).view(torch.float8_e4m3fn)
    w = (torch.randperm(2048, generator=gen) % 256).to(torch.uint8).reshape(32, 64)
    ref = _dense(w, s)
    assert torch.equal(ref.to(dtype).float(), ref)
    assert torch.equal(sk.nvfp4_dequantize(w.to(DEV), s.to(DEV), dtype).cpu(), ref.to(dtype))


@pytest.mark.parametrize("m,k,n,dtype,bias,split", [
    (1, 128, 16, F16, False, False),       # streaming form: one row, one k-block, one column tile
    (17, 384, 144, BF16, True, False),     # two 16-row tiles, 3 k-blocks over 8 waves
    (64, 2176, 256, F16, True, True),      # four row tiles: 17 k-blocks = two k-ranges through slabs
    (32, 256, 8208, BF16, True, False),    # 513 column tiles walked by 256 workgroups, ragged last phase
    (40, 4224, 1392, F16, True, True),     # three k-ranges x 85 workgroups walking 87 tiles
    (65, 128, 16, BF16, False, False),     # tile form: a full tile's first row past 64, one k-block, ragged N
    (129, 384, 144, F16, True, False),     # a 128-row tile + a 1-row tile, N tail past a tile
    (300, 1024, 256, BF16, True, True),    # ragged row tile, split-K with a short last range
])
def test_nvfp4_gemm_vs_float64(m, k, n, dtype, bias, split, sk):
    """The gate test_awq_tiled_gemm_gpu.py applies to the same kind of product (exact weights, f32 accumulation, one rounding)."""
    assert sk.nvfp4_gemm_form(m, n, k) == (0 if m <= 64 else 1)
    assert (sk.nvfp4_gemm_kranges(m, n, k) > 1) == split
    gen = torch.Generator().manual_seed(m + k)
    w, s = _case(n, k, gen)
    gs = torch.tensor(0.009)
    x = torch.randn(m, k, generator=gen).to(dtype)
    b = torch.randn(n, generator=gen).to(dtype) if bias else None
    qp, sp = sk.nvfp4_repack(w.to(DEV), s.to(DEV))
    y = sk.nvfp4_gemm(x.to(DEV), qp, sp, gs.to(DEV), None if b is None else b.to(DEV))
    ref = x.double() @ _dense(w, s).double().T * gs.double()
    _gate(y, ref if b is None else ref + b.double(), dtype)


@pytest.mark.parametrize("m", [8, 65, 260])
@pytest.mark.parametrize("k", [768, 4608])
def test_nvfp4_gemm_exact_small_integers(m, k, sk):
    """Power-of-two scales in [2^-3, 2], weight_scale_2 = 1/4, x in {-2..2}: every product is a multiple of 2^-4 and
    |sum| <= 4608 * 2 * 12 < 2^17, so all partial sums are exact in f32 in any order and the output is the reference rounded once:
    a wrong nibble, sign, group index, fragment lane, k-range boundary or slab shows as a non-zero difference."""
    n = 96
    gen = torch.Generator().manual_seed(11)
    w, s = _case(n, k, gen, scale_bytes=(0x20, 0x41))
    s = (s.view(torch.uint8) & 0x78).view(torch.float8_e4m3fn)   # mantissa cleared: 2^-3 .. 2
    x = torch.randint(-2, 3, (m, k), generator=gen).to(F16)
    qp, sp = sk.nvfp4_repack(w.to(DEV), s.to(DEV))
    y = sk.nvfp4_gemm(x.to(DEV), qp, sp, torch.tensor(0.25, device=DEV))
    assert torch.equal(y.cpu(), (x.double() @ _dense(w, s).double().T * 0.25).to(F16))


@pytest.mark.parametrize("m", [20, 150])
def test_nvfp4_gemm_row_stride(m, sk):
    k, n = 256, 64
    gen = torch.Generator().manual_seed(7)
    w, s = _case(n, k, gen)
    qp, sp = sk.nvfp4_repack(w.to(DEV), s.to(DEV))
    gs = torch.tensor(0.009, device=DEV)
    x = torch.randn(m, k + 64, generator=gen).to(BF16).to(DEV)[:, :k]
    assert x.stride(0) == k + 64
    assert torch.equal(sk.nvfp4_gemm(x, qp, sp, gs), sk.nvfp4_gemm(x.contiguous(), qp, sp, gs))


@pytest.mark.parametrize("m,k", [(520, 512), (8, 192)])
def test_petit_nvfp4_unfused_route(m, k, sk, pkg):
    """M past FUSED_MAX_M, and a K the fused kernel does not take: nvfp4_dequantize (global scale folded in) + dense_linear."""
    from ltp_sglang_amd.srt.layers.quantization import petit_utils

    assert m > petit_utils.FUSED_MAX_M or k % 128 != 0
    n = 64
    gen = torch.Generator().manual_seed(m)
    w, s = _case(n, k, gen)
    gs = torch.tensor(0.009)
    x = torch.randn(m, k, generator=gen).to(BF16)
    bias = torch.randn(n, generator=gen).to(BF16)
    packed = sk.nvfp4_repack(w.to(DEV), s.to(DEV)) if k % 128 == 0 else None
    y = petit_utils.apply_petit_nvfp4_linear(x.to(DEV), w.to(DEV), s.to(DEV), gs.to(DEV), n, k, bias.to(DEV), packed)
    _gate(y, x.double() @ _dense(w, s).double().T * gs.double() + bias.double(), BF16)


@pytest.mark.parametrize("xshape", [(8,), (200,), (2, 4)])
def test_petit_nvfp4_public_route(xshape, sk, pkg):
    from ltp_sglang_amd.srt.layers.quantization import get_quantization_config
    from ltp_sglang_amd.srt.layers.quantization.petit import PetitNvFp4Config, PetitNvFp4LinearMethod

    assert get_quantization_config("petit_nvfp4") is PetitNvFp4Config
    quant = {"quant_algo": "NVFP4", "group_size": 16, "kv_cache_quant_algo": None, "exclude_modules": ["lm_head"]}
    cfg = PetitNvFp4Config.from_config({"quantization": quant})
    for bad in ({"group_size": 32}, {"quant_algo": "FP8"}):
        with pytest.raises(ValueError):
            PetitNvFp4Config.from_config({"quantization": {**quant, **bad}})
    k, parts = 512, [128, 64]
    n = sum(parts)
    layer = torch.nn.Module()
    meth = PetitNvFp4LinearMethod(cfg)
    meth.create_weights(layer, k, parts, k, n, BF16)
    got = {name: (tuple(p.shape), p.dtype) for name, p in layer.named_parameters()}
    assert got == {"weight": ((n, k // 2), torch.uint8), "input_scale": ((2,), torch.float32),
                   "weight_scale_2": ((2,), torch.float32), "weight_scale": ((n, k // 16), torch.float8_e4m3fn)}
    gen = torch.Generator().manual_seed(5)
    w, s = _case(n, k, gen)
    layer.weight.data, layer.weight_scale.data = w.to(DEV), s.to(DEV)
    layer.weight_scale_2.data = torch.tensor([0.006, 0.009], device=DEV)
    layer.input_scale.data = torch.tensor([0.5, 0.25], device=DEV)
    meth.process_weights_after_loading(layer)
    assert not hasattr(layer, "input_scale") and layer.weight_scale_2.item() == pytest.approx(0.009)
    x = torch.randn(*xshape, k, generator=gen).to(BF16)
    bias = torch.randn(n, generator=gen).to(BF16)
    y = meth.apply(layer, x.to(DEV), bias.to(DEV))
    assert y.shape == (*xshape, n)
    qp, sp = layer.nvfp4_packed
    assert torch.equal(y.reshape(-1, n), sk.nvfp4_gemm(x.reshape(-1, k).to(DEV), qp, sp, layer.weight_scale_2, bias.to(DEV)))
    ref = x.reshape(-1, k).double() @ _dense(w, s).double().T * torch.tensor(0.009).double() + bias.double()
    _gate(y.reshape(-1, n), ref, BF16)
