"""GPU: the 576 / 512 latent-KV (MLA) extend kernel through sgl_kernel.extend_attention_fwd and HipAttnBackend.forward_extend.

Tolerances are the project's extend tolerances against the float64 oracle (test_extend_attention_gpu.py): bf16 2e-2, f16 3e-3."""
import functools
from types import SimpleNamespace

import pytest
import torch

from oracle import attention as oa

pytestmark = pytest.mark.gpu

TOL_F64 = {torch.bfloat16: 2e-2, torch.float16: 3e-3}
# (prefix, extend): a tile edge on both sides of the seam, a tile that straddles it, a row block that ends mid-token-range, a
# diagonal that crosses tile boundaries, a request with nothing to do
LENS = [(0, 1), (0, 33), (31, 5), (32, 32), (33, 70), (97, 3), (5, 0)]
POOL, D, DV = 512, 576, 512
SCALE = 192 ** -0.5


@functools.lru_cache(maxsize=None)
def _problem(hq, dtype):
    """One batch over a permuted 512-row pool whose unreferenced rows (except row 0) are NaN."""
    g = torch.Generator().manual_seed(hq)
    pre = torch.tensor([p for p, _ in LENS])
    ext = torch.tensor([e for _, e in LENS])
    npre, t = int(pre.sum()), int(ext.sum())
    perm = torch.randperm(POOL - 1, generator=g) + 1
    slots, new = perm[:npre].int(), perm[npre: npre + t]   # cached prefix rows / the rows the new tokens go to
    kv = torch.randn(POOL, 1, D, generator=g).to(dtype)
    dead = torch.ones(POOL, dtype=torch.bool)
    dead[slots.long()] = False
    dead[0] = False
    kv[dead] = float("nan")
    q = torch.randn(t, hq, D, generator=g).to(dtype)
    k = torch.randn(t, 1, D, generator=g).to(dtype)
    kv_indptr = torch.zeros(len(LENS) + 1, dtype=torch.int32)
    kv_indptr[1:] = torch.cumsum(pre, 0)
    qo_indptr = torch.zeros(len(LENS) + 1, dtype=torch.int32)
    qo_indptr[1:] = torch.cumsum(ext, 0)
    return SimpleNamespace(q=q, k=k, kv=kv, slots=slots, new=new, pre=pre, ext=ext, kv_indptr=kv_indptr, qo_indptr=qo_indptr)


@functools.lru_cache(maxsize=None)
def _ref(hq, dtype, causal, logit_cap=0.0):
    P = _problem(hq, dtype)
    return oa.extend_attention_masked_f64(P.q, P.k, P.k[..., :DV], P.kv, P.kv[..., :DV], P.qo_indptr, P.kv_indptr, P.slots, None, None,
                                          SCALE, is_causal=causal, logit_cap=logit_cap)


def _run(P, dtype, causal, logit_cap=0.0):
    from ltp_sglang_amd import sgl_kernel

    dev = torch.device("cuda:0")
    kv, k = P.kv.to(dev), P.k.to(dev)
    o = torch.full((P.q.shape[0], P.q.shape[1], DV), float("nan"), dtype=dtype, device=dev)
    sgl_kernel.extend_attention_fwd(P.q.to(dev), k, k[..., :DV], o, kv, kv[..., :DV], P.qo_indptr.to(dev), P.kv_indptr.to(dev),
                                    P.slots.to(dev), None, causal, None, int(P.ext.max()), SCALE, logit_cap)
    torch.cuda.synchronize()
    return o.cpu()


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("hq", [8, 16, 128])
def test_mla_extend_matches_f64(hq, dtype, causal, pkg):
    o = _run(_problem(hq, dtype), dtype, causal)
    assert torch.isfinite(o.float()).all()
    err = (o.double() - _ref(hq, dtype, causal)).abs().max().item()
    print(f"mla extend hq={hq} {dtype} causal={causal}: max |err| = {err:.3e}")
    assert err <= TOL_F64[dtype]


def test_mla_extend_logit_cap(pkg):
    o = _run(_problem(16, torch.bfloat16), torch.bfloat16, True, logit_cap=30.0)
    err = (o.double() - _ref(16, torch.bfloat16, True, 30.0)).abs().max().item()
    print(f"mla extend logit_cap=30: max |err| = {err:.3e}")
    assert err <= TOL_F64[torch.bfloat16]


def test_backend_extend_over_mla_pool(pkg):
    from ltp_sglang_amd import sgl_kernel
    from ltp_sglang_amd.srt.layers.attention.hip_backend import HipAttnBackend
    from ltp_sglang_amd.srt.layers.radix_attention import RadixAttention
    from ltp_sglang_amd.srt.mem_cache.memory_pool import MLATokenToKVPool
    from ltp_sglang_amd.srt.model_executor.forward_batch_info import ForwardBatch, ForwardMode

    dev, hq, bs, dtype = "cuda:0", 16, len(LENS), torch.bfloat16
    P = _problem(hq, dtype)
    pool = MLATokenToKVPool(POOL - 1, 1, dtype, DV, D - DV, 1, dev, False)
    layer = RadixAttention(hq, D, SCALE, 1, 0, v_head_dim=DV)
    pool.kv_buffer[0].copy_(P.kv.to(dev))   # the rows at out_cache_loc are NaN until the forward writes them
    seq = P.pre + P.ext
    r2t = torch.zeros(bs, int(seq.max()), dtype=torch.int32)
    for i, (p, e) in enumerate(LENS):
        r2t[i, :p] = P.slots[P.kv_indptr[i]: P.kv_indptr[i + 1]]
        r2t[i, p: p + e] = P.new[P.qo_indptr[i]: P.qo_indptr[i + 1]].int()
    r2t = r2t.to(dev)
    runner = SimpleNamespace(device=dev, gpu_id=0, req_to_token_pool=SimpleNamespace(size=bs, req_to_token=r2t),
                             token_to_kv_pool=pool, sliding_window_size=None,
                             model_config=SimpleNamespace(num_attention_heads=hq, get_num_kv_heads=lambda tp: 1, context_len=r2t.shape[1],
                                                          is_encoder_decoder=False))
    backend = HipAttnBackend(runner)
    t = P.q.shape[0]
    fb = ForwardBatch.init_new(ForwardMode.EXTEND, torch.arange(bs, device=dev), seq.to(dev), P.new.to(dev),
                               torch.zeros(t, dtype=torch.int64, device=dev), None, pool, backend,
                               extend_prefix_lens=P.pre.to(dev), extend_seq_lens=P.ext.to(dev), seq_lens_cpu=seq)
    backend.init_forward_metadata(fb)
    q, k = P.q.to(dev), P.k.to(dev)
    v = k[..., :DV].clone()   # a separate copy of k_nope, as the reference's caller passes
    got = backend.forward_extend(q.reshape(t, -1), k, v, layer, fb, save_kv_cache=True).view(t, hq, DV)
    torch.cuda.synchronize()
    assert torch.equal(pool.kv_buffer[0][P.new.to(dev)].view(torch.int16), k.view(torch.int16))
    assert torch.equal(got.cpu().view(torch.int16), _run(P, dtype, True).view(torch.int16))
    assert (got.cpu().double() - _ref(hq, dtype, True)).abs().max().item() <= TOL_F64[dtype]
    # the native-op signature (prefix addressed through req_to_token) reaches the same kernel
    o2 = torch.full_like(got, float("nan"))
    sgl_kernel.extend_attention(q, k, k[..., :DV], o2, pool.get_key_buffer(0), pool.get_value_buffer(0), r2t, fb.req_pool_indices,
                                fb.seq_lens, fb.extend_seq_lens, fb.extend_start_loc, int(P.ext.max()), SCALE, 0.0)
    assert torch.equal(o2.view(torch.int16), got.view(torch.int16))
