"""GPU: the 576 / 512 latent-KV (MLA) decode kernel, the latent pool write and MLATokenToKVPool behind HipAttnBackend.

Tolerances are the project's decode tolerances against the float64 oracle (test_decode_attention_gpu.py): bf16 2e-2, f16 3e-3."""
import functools
from types import SimpleNamespace

import pytest
import torch

from oracle import attention as oa

pytestmark = pytest.mark.gpu

TOL_F64 = {torch.bfloat16: 2e-2, torch.float16: 3e-3}
SEQ = [1, 31, 32, 33, 97, 300]   # a tile edge on both sides, empty splits, five live splits of 64
POOL, D, DV, MAX_SPLITS = 512, 576, 512, 8
SCALE = 192 ** -0.5


@functools.lru_cache(maxsize=None)
def _problem(hq, dtype, logit_cap=0.0):
    """One batch over a permuted 512-row pool whose unreferenced rows (except row 0) are NaN, and its float64 reference."""
    g = torch.Generator().manual_seed(hq)
    bs, total = len(SEQ), sum(SEQ)
    slots = torch.randperm(POOL, generator=g)[:total].int()
    kv = torch.randn(POOL, 1, D, generator=g).to(dtype)
    dead = torch.ones(POOL, dtype=torch.bool)
    dead[slots.long()] = False
    dead[0] = False
    kv[dead] = float("nan")
    q = torch.randn(bs, hq, D, generator=g).to(dtype)
    seq = torch.tensor(SEQ, dtype=torch.int64)
    r2t = torch.zeros(bs, max(SEQ), dtype=torch.int32)
    kv_indptr = torch.zeros(bs + 1, dtype=torch.int32)
    kv_indptr[1:] = torch.cumsum(seq, 0)
    for i in range(bs):
        r2t[i, : SEQ[i]] = slots[kv_indptr[i]: kv_indptr[i + 1]]
    ref = oa.decode_attention_f64(q, kv, kv[..., :DV], r2t, torch.arange(bs), seq, SCALE, logit_cap)
    return SimpleNamespace(q=q, kv=kv, slots=slots, kv_indptr=kv_indptr, r2t=r2t, seq=seq, ref=ref)


def _run(P, hq, dtype, splits, logit_cap=0.0):
    from ltp_sglang_amd import sgl_kernel

    dev = torch.device("cuda:0")
    bs = len(SEQ)
    kv = P.kv.to(dev)
    o = torch.full((bs, hq, DV), float("nan"), dtype=dtype, device=dev)
    logits = torch.full((bs, hq, MAX_SPLITS, DV), float("nan"), dtype=torch.float32, device=dev)
    lse = torch.full((bs, hq, MAX_SPLITS), float("nan"), dtype=torch.float32, device=dev)
    sgl_kernel.decode_attention_fwd(P.q.to(dev), kv, kv[..., :DV], o, P.kv_indptr.to(dev), P.slots.to(dev), logits, lse,
                                    torch.tensor(splits, dtype=torch.int32, device=dev), MAX_SPLITS, SCALE, logit_cap)
    torch.cuda.synchronize()
    return o.cpu()


@pytest.mark.parametrize("split_mode", ["one", "ragged", "max"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("hq", [8, 16, 32, 64, 128])
def test_mla_decode_matches_f64(hq, dtype, split_mode, pkg):
    bs = len(SEQ)
    splits = {"one": [1] * bs, "ragged": [(i % 8) + 1 for i in range(bs)], "max": [MAX_SPLITS] * bs}[split_mode]
    P = _problem(hq, dtype)
    o = _run(P, hq, dtype, splits)
    assert torch.isfinite(o.float()).all()
    err = (o.double() - P.ref).abs().max().item()
    print(f"mla decode hq={hq} {dtype} {split_mode}: max |err| = {err:.3e}")
    assert err <= TOL_F64[dtype]


def test_mla_decode_logit_cap(pkg):
    P = _problem(16, torch.bfloat16, 30.0)
    o = _run(P, 16, torch.bfloat16, [2, 1, 3, 4, 8, 5], logit_cap=30.0)
    assert (o.double() - P.ref).abs().max().item() <= TOL_F64[torch.bfloat16]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_set_mla_kv_buffer_byte_exact(dtype, pkg):
    from ltp_sglang_amd import sgl_kernel

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    n = 37
    buf = torch.randn(101, 1, D, generator=g).to(dtype).to(dev)
    loc = torch.randperm(101, generator=g)[:n].to(dev)
    nope = torch.randn(n, 1, DV + 64, generator=g).to(dtype).to(dev)[..., 8:8 + DV]   # row strides != widths
    rope = torch.randn(n, 1, 96, generator=g).to(dtype).to(dev)[..., 16:16 + 64]
    want = buf.clone()
    want[loc, 0, :DV] = nope[:, 0]
    want[loc, 0, DV:] = rope[:, 0]
    sgl_kernel.set_mla_kv_buffer(buf, loc, nope, rope)
    assert torch.equal(buf.view(torch.int16), want.view(torch.int16))


def test_backend_decode_over_mla_pool(pkg):
    from ltp_sglang_amd import sgl_kernel
    from ltp_sglang_amd.srt.layers.attention.hip_backend import HipAttnBackend
    from ltp_sglang_amd.srt.layers.radix_attention import RadixAttention
    from ltp_sglang_amd.srt.mem_cache.memory_pool import MLATokenToKVPool
    from ltp_sglang_amd.srt.model_executor.forward_batch_info import ForwardBatch, ForwardMode

    dev, hq, bs = "cuda:0", 16, len(SEQ)
    P = _problem(hq, torch.bfloat16)
    pool = MLATokenToKVPool(POOL - 1, 1, torch.bfloat16, DV, D - DV, 1, dev, False)
    layer = RadixAttention(hq, D, SCALE, 1, 0, v_head_dim=DV)
    new = P.slots[(P.kv_indptr[1:] - 1).long()].long().to(dev)   # the last token of every request is the step's new one
    pool.kv_buffer[0].copy_(P.kv.to(dev))
    pool.kv_buffer[0][new] = 0
    rows = P.kv.to(dev)[new]
    pool.set_mla_kv_buffer(layer, new, rows[..., :DV], rows[..., DV:])
    assert torch.equal(pool.kv_buffer[0].view(torch.int16), P.kv.to(dev).view(torch.int16))
    r2t = P.r2t.to(dev)
    runner = SimpleNamespace(device=dev, gpu_id=0, req_to_token_pool=SimpleNamespace(size=bs, req_to_token=r2t),
                             token_to_kv_pool=pool, sliding_window_size=None,
                             model_config=SimpleNamespace(num_attention_heads=hq, get_num_kv_heads=lambda tp: 1, context_len=r2t.shape[1],
                                                          is_encoder_decoder=False),
                             server_args=SimpleNamespace(triton_attention_num_kv_splits=MAX_SPLITS, speculative_num_draft_tokens=None,
                                                         speculative_num_steps=None))
    backend = HipAttnBackend(runner)
    fb = ForwardBatch(forward_mode=ForwardMode.DECODE, batch_size=bs, input_ids=torch.zeros(bs, dtype=torch.int64, device=dev),
                      req_pool_indices=torch.arange(bs, device=dev), seq_lens=P.seq.to(dev), out_cache_loc=new,
                      seq_lens_sum=sum(SEQ), token_to_kv_pool=pool, attn_backend=backend)
    backend.init_forward_metadata(fb)
    q = P.q.to(dev)
    got = backend.forward_decode(q.reshape(bs, -1), None, None, layer, fb, save_kv_cache=False).view(bs, hq, DV)
    md = backend.forward_metadata
    o = torch.empty(bs, hq, DV, dtype=torch.bfloat16, device=dev)
    sgl_kernel.decode_attention_fwd(q, pool.get_key_buffer(0), pool.get_value_buffer(0), o, md.kv_indptr, md.kv_indices,
                                    torch.empty_like(md.attn_logits), torch.empty_like(md.attn_lse), md.num_kv_splits, MAX_SPLITS, SCALE)
    assert torch.equal(got.view(torch.int16), o.view(torch.int16))
    assert (got.cpu().double() - P.ref).abs().max().item() <= TOL_F64[torch.bfloat16]
