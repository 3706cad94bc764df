"""Kernel-level timing of fused_experts (bf16 experts, uniform random routing) at three MoE layers' shapes:
  bench_moe.py [--out CSV] [--ts 1,32,...] [--models deepseek_v3_tp8,...]
Timing as tools/bench_int8.py: the call captured in a HIP graph that walks over several copies of the expert weights (together
larger than the last-level cache), warmed up, replayed; the median counts.  Every timing is taken twice, the two forms alternating,
and both values and their spread go into the CSV.  Per row:
  stream / tile   us per fused_experts with the streaming (block_size 16) / tile (block_size 128) grouped GEMMs forced
  form            what moe_gemm_form picks for this shape
  loop            what the tree would otherwise force: a Python loop over the experts of dense_linear -> silu_and_mul -> dense_linear and
                  an index_add_, timed eagerly with a host clock around a device synchronise (it reads the routing on the host and
                  cannot be captured)
  hbm_us          the bytes of the DISTINCT ACTIVE experts' weights over 8 TB/s: the floor of a small T
  tflops          2 * P * 3 * H * I over the time of the chosen form (the bare bf16 MFMA rate is 1 650 TFLOP/s)"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools.bench_block_fp8 import graph_time

from ltp_sglang_amd import sgl_kernel as K
from ltp_sglang_amd.srt.layers.moe import fused_moe as FM
from ltp_sglang_amd.srt.layers.moe.topk import StandardTopKOutput, fused_topk

MODELS = {   # name: (E, topk, H, I)
    "deepseek_v3_tp8": (256, 8, 7168, 256),
    "qwen3_30b_a3b": (128, 8, 2048, 768),
    "mixtral_8x7b_tp8": (8, 2, 4096, 14336 // 8),
}
HEADER = ("model,T,E,topk,H,I,form,stream_us_1,stream_us_2,tile_us_1,tile_us_2,spread_pct,loop_us_1,loop_us_2,active_experts,"
          "hbm_us,tflops")


def expert_loop(x, w1, w2, tw, ids):
    out = torch.zeros_like(x, dtype=torch.float32)
    for e in torch.unique(ids).tolist():   # host sync: the routing decides the launches
        tok, slot = torch.nonzero(ids == e, as_tuple=True)
        h = K.silu_and_mul(K.dense_linear(x[tok].contiguous(), w1[e]))
        out.index_add_(0, tok, K.dense_linear(h, w2[e]).float() * tw[tok, slot].unsqueeze(1))
    return out.to(x.dtype)


def host_time(f, reps=3):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return sorted(ts)[len(ts) // 2]


def sweep(out, ts, models):
    dev = "cuda:0"
    rows = [HEADER]
    print(HEADER, flush=True)
    for name in models:
        E, topk, H, I = MODELS[name]
        copies = max(2, min(6, int(1.2e9 // (E * 3 * H * I * 2)) + 1))
        ws = [(torch.randn(E, 2 * I, H, device=dev, dtype=torch.bfloat16) * 0.05, torch.randn(E, H, I, device=dev, dtype=torch.bfloat16) * 0.05)
              for _ in range(copies)]
        for T in ts:
            gen = torch.Generator(device=dev).manual_seed(T)
            x = torch.randn(T, H, generator=gen, device=dev).to(torch.bfloat16) * 0.5
            tw, ids = fused_topk(x, torch.randn(T, E, generator=gen, device=dev), topk, True)
            top = StandardTopKOutput(tw, ids, None)

            def timed(block_size):
                FM._FORCE_BLOCK_SIZE = block_size
                try:
                    return graph_time([(lambda w=w: FM.fused_experts(x, w[0], w[1], top)) for w in ws])
                finally:
                    FM._FORCE_BLOCK_SIZE = None

            st, ti, lo = [], [], []
            for _ in range(2):   # alternating: a drift of the machine shows as spread, not as a difference between the forms
                st.append(timed(16))
                ti.append(timed(128))
                lo.append(host_time(lambda: expert_loop(x, ws[0][0], ws[0][1], tw, ids)))
            form = K.moe_gemm_form(T * topk, E, I, H)
            best = min(ti) if form else min(st)
            spread = max((max(v) - min(v)) / min(v) for v in (st, ti)) * 100.0
            active = int(torch.unique(ids).numel())
            hbm_us = active * 3 * H * I * 2 / 8e12 * 1e6
            rows.append(f"{name},{T},{E},{topk},{H},{I},{form},{st[0]:.1f},{st[1]:.1f},{ti[0]:.1f},{ti[1]:.1f},{spread:.1f},{lo[0]:.0f},"
                        f"{lo[1]:.0f},{active},{hbm_us:.1f},{2.0 * T * topk * 3 * H * I / best / 1e6:.1f}")
            print(rows[-1], flush=True)
        del ws
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--ts", default="1,32,128,512,2048,8192")
    ap.add_argument("--models", default=",".join(MODELS))
    a = ap.parse_args()
    sweep(a.out, [int(v) for v in a.ts.split(",")], a.models.split(","))
