"""GPU: the fused MoE path for 16-bit experts against plain CPU float64 -- topk_softmax, moe_align_block_size, fused_experts in both
GEMM forms and its variants, and a captured graph replayed on new routing."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


# ---- topk_softmax -------------------------------------------------------------------------------------------------------------

def _distinct_logits(T, E, dtype, seed):
    """per row a seeded permutation of E distinct values in [-8, 8), multiples of 1/32: exact in every dtype here"""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.arange(E, dtype=torch.float64) - E // 2) * ((512 // E) / 32.0)
    return torch.stack([vals[torch.randperm(E, generator=g)] for _ in range(T)]).to(dtype)


@pytest.mark.parametrize("T,E,topk,dtype,renorm", [(1, 8, 2, "f32", False), (33, 60, 4, "bf16", True), (7, 256, 8, "f16", False),
                                                   (5, 512, 32, "f32", True), (5, 512, 32, "bf16", False)])
def test_topk_softmax(pkg, T, E, topk, dtype, renorm):
    from ltp_sglang_amd.sgl_kernel import topk_softmax

    logits = _distinct_logits(T, E, DTYPES[dtype], 7)
    logits = torch.cat([logits, torch.full((1, E), 0.25, dtype=logits.dtype)])   # one all-equal row: ids 0 .. topk - 1
    w = torch.empty(T + 1, topk, dtype=torch.float32, device=DEV)
    ids = torch.empty(T + 1, topk, dtype=torch.int32, device=DEV)
    topk_softmax(w, ids, logits.to(DEV), renorm)
    ref_w, ref_i = torch.softmax(logits.double(), dim=-1).topk(topk, dim=-1)
    if renorm:
        ref_w = ref_w / ref_w.sum(-1, keepdim=True)
    assert torch.equal(ids.cpu()[:T].long(), ref_i[:T])
    assert ids.cpu()[T].tolist() == list(range(topk))
    rel = ((w.cpu().double() - ref_w).abs() / ref_w).max().item()
    print(f"topk_softmax max relative weight error {rel:.3e}")
    assert rel <= 2.0 ** -15


# ---- moe_align_block_size -----------------------------------------------------------------------------------------------------

def _align_ids(T, topk, E, forced, invalid):
    g = torch.Generator().manual_seed(T * 131 + E)
    ids = torch.randint(0, E, (T, topk), generator=g, dtype=torch.int32)
    if forced == "16/15":   # expert 0: exactly one full block, expert 1: 15, expert 2: 1, the others none
        ids[:, 0], ids[:, 1] = 0, 1
        ids[3, 1] = 2
    elif forced == "16/17":  # expert 0: exactly 16, expert 1: one past a block, the others none
        ids[:, 0], ids[:, 1] = 0, 1
        ids[16, 0] = 1
    if invalid:
        ids.view(-1)[torch.randperm(T * topk, generator=g)[: T * topk // 10]] = -1
    return ids


@pytest.mark.parametrize("T,topk,E,bs,forced,invalid", [(1, 2, 8, 16, None, False), (16, 2, 8, 16, "16/15", False),
                                                        (17, 2, 8, 16, "16/17", False), (64, 8, 256, 16, None, False),
                                                        (3000, 8, 60, 128, None, False), (300, 8, 60, 16, None, True),
                                                        (3000, 8, 60, 128, None, True)])
def test_moe_align_block_size(pkg, T, topk, E, bs, forced, invalid):
    from ltp_sglang_amd.srt.layers.moe.fused_moe import moe_align_block_size

    ids = _align_ids(T, topk, E, forced, invalid)
    P = ids.numel()
    sorted_ids, expert_ids, post_pad = (t.cpu() for t in moe_align_block_size(ids.to(DEV), bs, E))
    flat = ids.view(-1).long()
    counts = torch.bincount(flat[flat >= 0], minlength=E)
    padded = (counts + bs - 1) // bs * bs
    total = int(padded.sum())
    assert int(post_pad[0]) == total
    assert torch.equal(expert_ids[: total // bs].long(), torch.repeat_interleave(torch.arange(E), padded // bs))
    want = torch.full((total,), P, dtype=torch.int64)   # every expert's pairs ascending, then the padding value
    starts = torch.cumsum(padded, 0) - padded
    for e in range(E):
        want[starts[e]: starts[e] + counts[e]] = torch.nonzero(flat == e).view(-1)
    assert torch.equal(sorted_ids[:total].long(), want)


# ---- fused_experts ------------------------------------------------------------------------------------------------------------

CASES = {   # name: (T, E, topk, H, I, form)
    "one_token": (1, 8, 2, 128, 64, 0),
    "topk1": (5, 8, 1, 64, 32, 0),
    "odd_sizes": (19, 60, 4, 160, 96, 0),
    "forced_16_17_0": (40, 4, 2, 256, 128, 1),
    "tile": (700, 4, 2, 192, 160, 1),
}


def _routing(T, E, topk, seed, name=""):
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).int()
    if name == "forced_16_17_0":   # expert 0: 16 pairs, expert 1: 17, expert 2: none, expert 3 the rest (twice in a token where needed)
        ids = torch.tensor([[0, 3]] * 16 + [[1, 3]] * 17 + [[3, 3]] * 7, dtype=torch.int32)
    w = torch.softmax(torch.randn(T, E, generator=g), -1).gather(1, ids.long().clamp(min=0)).float()
    return w, ids


def _inputs(name, dtype, seed=0):
    T, E, topk, H, I, _ = CASES[name]
    g = torch.Generator().manual_seed(seed + 1)
    x = (0.5 * torch.randn(T, H, generator=g)).to(dtype)
    w1 = (0.05 * torch.randn(E, 2 * I, H, generator=g)).to(dtype)
    w2 = (0.05 * torch.randn(E, H, I, generator=g)).to(dtype)
    return x, w1, w2


def _reference(x, w1, w2, tw, ids, dtype, scale=1.0, on_input=False, combine=True, emulate=False):
    """float64 (emulate=False), or f32 matmuls of the 16-bit values rounded to dtype at the four places fused_experts_impl stores
    16-bit: GEMM 1's output, silu_and_mul's, weight * GEMM 2's output, the scaled sum.  A pair with id -1 contributes nothing."""
    ft = torch.float32 if emulate else torch.float64
    rnd = (lambda t: t.to(dtype).to(ft)) if emulate else (lambda t: t)
    T, topk = ids.shape
    I = w2.shape[2]
    y = torch.zeros(T, topk, w2.shape[1], dtype=ft)
    for t in range(T):
        for j in range(topk):
            e = int(ids[t, j])
            if e < 0:
                continue
            c1 = x[t].to(ft) @ w1[e].to(ft).T
            c1 = rnd(c1 * tw[t, j].to(ft) if on_input else c1)
            act = rnd(torch.nn.functional.silu(c1[:I]) * c1[I:])
            c3 = act @ w2[e].to(ft).T
            y[t, j] = rnd(c3 if on_input else c3 * tw[t, j].to(ft))
    if not combine:
        return y.double()
    return rnd(y.sum(1) * scale).double() if (topk > 1 or scale != 1.0) else y[:, 0].double()


def _check(out, exact, emu, dtype):
    """as close to exact arithmetic as the reference's own rounding is (tests/test_model_gpu.py's criterion)"""
    hip = out.cpu().double()
    ulp = 2.0 ** (math.floor(math.log2(exact.abs().max().item())) - (7 if dtype == torch.bfloat16 else 10))
    e_hip, e_emu = (hip - exact).abs(), (emu - exact).abs()
    print(f"max |hip - exact| {e_hip.max():.3e} (emu {e_emu.max():.3e}, ulp {ulp:.3e}); mean {e_hip.mean():.3e} (emu {e_emu.mean():.3e})")
    assert e_hip.max() <= 1.25 * e_emu.max() + ulp
    assert e_hip.mean() <= 1.10 * e_emu.mean()


def _run(name, dtype, ids=None, seed=0, refs=True, **kw):
    from ltp_sglang_amd.sgl_kernel import moe_gemm_form
    from ltp_sglang_amd.srt.layers.moe.fused_moe import fused_experts
    from ltp_sglang_amd.srt.layers.moe.topk import StandardTopKOutput

    T, E, topk, H, I, form = CASES[name]
    assert moe_gemm_form(T * topk, E, I, H) == form
    x, w1, w2 = _inputs(name, dtype, seed)
    tw, rids = _routing(T, E, topk, seed + 2, name)
    ids = rids if ids is None else ids
    xd = x.to(DEV)
    out = fused_experts(xd, w1.to(DEV), w2.to(DEV), StandardTopKOutput(tw.to(DEV), ids.to(DEV), None), **kw)
    if not refs:
        return out
    ref_kw = dict(scale=kw.get("routed_scaling_factor") or 1.0, on_input=kw.get("apply_router_weight_on_input", False),
                  combine=not kw.get("no_combine", False))
    exact = _reference(x, w1, w2, tw, ids, dtype, **ref_kw)
    emu = _reference(x, w1, w2, tw, ids, dtype, emulate=True, **ref_kw)
    return out, xd, exact, emu


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_experts(pkg, name, dtype):
    out, _, exact, emu = _run(name, DTYPES[dtype])
    assert out.shape == exact.shape
    _check(out, exact, emu, DTYPES[dtype])
    assert torch.equal(out, _run(name, DTYPES[dtype], refs=False))   # no atomics, no order left to chance


@pytest.mark.parametrize("name,dtype,kw", [
    ("odd_sizes", "bf16", dict(inplace=True)),
    ("tile", "f16", dict(no_combine=True)),
    ("topk1", "bf16", dict(apply_router_weight_on_input=True)),
    ("odd_sizes", "f16", dict(routed_scaling_factor=2.5)),
    ("topk1", "f16", dict(routed_scaling_factor=2.5)),
])
def test_fused_experts_variants(pkg, name, dtype, kw):
    out, xd, exact, emu = _run(name, DTYPES[dtype], **kw)
    T, _, topk, H, _, _ = CASES[name]
    assert tuple(out.shape) == ((T, topk, H) if kw.get("no_combine") else (T, H))
    assert (out.data_ptr() == xd.data_ptr()) == bool(kw.get("inplace"))
    _check(out, exact, emu, DTYPES[dtype])


@pytest.mark.parametrize("name,dtype", [("odd_sizes", "bf16"), ("tile", "bf16")])
def test_fused_experts_skips_invalid_ids(pkg, name, dtype):
    T, E, topk = CASES[name][:3]
    ids = _routing(T, E, topk, 2)[1]
    g = torch.Generator().manual_seed(5)
    ids.view(-1)[torch.randperm(T * topk, generator=g)[: T * topk // 10]] = -1
    out, _, exact, emu = _run(name, DTYPES[dtype], ids=ids)
    _check(out, exact, emu, DTYPES[dtype])


def test_fused_experts_graph_replays_on_new_routing(pkg):
    """The device-side num_tokens_post_pad and the worst-case grid: one capture, replayed after the gating logits changed."""
    from ltp_sglang_amd.srt.layers.moe.fused_moe import fused_experts
    from ltp_sglang_amd.srt.layers.moe.topk import StandardTopKOutput, fused_topk

    name, dtype = "odd_sizes", torch.bfloat16
    T, E, topk, H, I, _ = CASES[name]
    x, w1, w2 = _inputs(name, dtype)
    xd, w1d, w2d = x.to(DEV), w1.to(DEV), w2.to(DEV)
    g = torch.Generator().manual_seed(11)
    draws = [torch.randn(T, E, generator=g), 3.0 * torch.randn(T, E, generator=g)]
    gating = draws[0].to(DEV)

    def layer():
        tw, ids = fused_topk(xd, gating, topk, True)
        return fused_experts(xd, w1d, w2d, StandardTopKOutput(tw, ids, gating)), tw, ids

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, _, _ = layer()
    gating.copy_(draws[1].to(DEV))
    for _ in range(3):
        graph.replay()
    replayed = out_g.clone()
    eager, tw, ids = layer()
    assert not torch.equal(ids.cpu(), fused_topk(xd, draws[0].to(DEV), topk, True)[1].cpu())   # the routing did change
    assert torch.equal(replayed, eager)
    exact = _reference(x, w1, w2, tw.cpu(), ids.cpu(), dtype)
    emu = _reference(x, w1, w2, tw.cpu(), ids.cpu(), dtype, emulate=True)
    _check(replayed, exact, emu, dtype)
