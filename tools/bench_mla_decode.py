"""Kernel-level timing of the MLA (576 / 512 latent-KV) decode attention, stage 1 + stage 2 launched:
  bench_mla_decode.py [--out CSV] [--label L] [--hqs 16,32,64,128] [--bss 1,32,128] [--ctxs 2048,8192] [--max-kv-splits 16]
bf16; the split counts are the backend's (decode_metadata, balance rule, at most --max-kv-splits).  Timing as tools/bench_nvfp4.py: the
call captured in a HIP graph that walks over several disjoint, randomly permuted slot sets of one pool, warmed up, replayed; the median
counts.  Per row: microseconds; the launch's algorithmic bytes (every KV row once, q, the split partials written by stage 1 and read by
stage 2, o) and FLOP (2 x Hq x (576 + 512) per token) over that time; the share of the larger of the two bounds (bytes at 8 TB/s, FLOP
at the bare bf16 MFMA rate tools/microbench/mfma_rate.hip measured, 1 650 TFLOP/s taken) and which bound that is.  The Hq 16 rows
also time the GQA kernel (Hq 16, Hkv 1, D 128) on 4.5 x the tokens as a yardstick for the memory-bound end and give both kernels'
achieved KV bytes/s (the GQA kernel reads a 256-byte K row AND a 256-byte V row per token).  Run it twice (--label 1 / 2) into one
CSV: the spread between the runs is the noise."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools.bench_block_fp8 import graph_time

from ltp_sglang_amd import sgl_kernel as K

HEADER = ("run,Hq,bs,ctx,splits,us,TB_per_s,TFLOP_per_s,bound,share_of_bound,kv_TB_per_s,gqa_us,gqa_kv_TB_per_s")
HBM_BPS, MFMA_FLOPS = 8.0e12, 1.65e15


def _calls(hq, hkv, d, dv, bs, ctx, max_splits, shared_kv, copies, gen):
    """`copies` closures running decode_attention_fwd over disjoint slot sets; -> (closures, splits of request 0)."""
    dev = "cuda:0"
    dt = torch.bfloat16
    rows = copies * bs * ctx + 1
    k = torch.randn(rows, hkv, d, generator=gen, device=dev, dtype=torch.float32).to(dt)
    v = k[..., :dv] if shared_kv else torch.randn(rows, hkv, dv, generator=gen, device=dev, dtype=torch.float32).to(dt)
    perm = (torch.randperm(rows - 1, generator=gen, device=dev) + 1).int()
    seq = torch.full((bs,), ctx, dtype=torch.int64, device=dev)
    kv_indptr = torch.zeros(bs + 1, dtype=torch.int32, device=dev)
    nsplit = torch.zeros(bs, dtype=torch.int32, device=dev)
    # (the MLA kernel's unit is a head block of up to 64 heads: HipAttnBackend gives the split rule 16 heads per block)
    split_heads = 16 * (1 if hq <= 32 else (hq + 63) // 64) if shared_kv else hq
    K.decode_metadata(kv_indptr, nsplit, seq, 1, split_heads, hkv, max_splits, torch.cuda.get_device_properties(0).multi_processor_count, 2)
    logits = torch.empty(bs, hq, max_splits, dv, dtype=torch.float32, device=dev)
    lse = torch.empty(bs, hq, max_splits, dtype=torch.float32, device=dev)
    o = torch.empty(bs, hq, dv, dtype=dt, device=dev)
    fs = []
    for c in range(copies):
        q = torch.randn(bs, hq, d, generator=gen, device=dev, dtype=torch.float32).to(dt)
        idx = perm[c * bs * ctx:(c + 1) * bs * ctx].contiguous()
        fs.append(lambda q=q, idx=idx: K.decode_attention_fwd(q, k, v, o, kv_indptr, idx, logits, lse, nsplit, max_splits, d ** -0.5))
    return fs, int(nsplit[0])


def sweep(out, label, hqs, bss, ctxs, max_splits):
    rows = [HEADER]
    print(HEADER, flush=True)
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    for ctx in ctxs:
        for bs in bss:
            copies = max(2, min(6, int(1.5e9 // (bs * ctx * 1152))))
            for hq in hqs:
                fs, ns = _calls(hq, 1, 576, 512, bs, ctx, max_splits, True, copies, gen)
                us = graph_time(fs)
                kv_bytes = bs * ctx * 1152
                nbytes = kv_bytes + bs * hq * (576 * 2 + 512 * 2) + 2 * bs * hq * ns * (512 + 1) * 4
                flop = 2.0 * bs * ctx * hq * (576 + 512)
                tb, tf = nbytes / us / 1e6, flop / us / 1e6
                by_bytes, by_flop = nbytes / HBM_BPS * 1e6, flop / MFMA_FLOPS * 1e6
                bound = "bytes" if by_bytes >= by_flop else "flop"
                gqa_us = gqa_tb = ""
                if hq == 16:   # the memory-bound yardstick
                    gctx = ctx * 9 // 2
                    gcopies = max(2, min(6, int(1.5e9 // (bs * gctx * 512))))
                    del fs
                    gfs, _ = _calls(16, 1, 128, 128, bs, gctx, max_splits, False, gcopies, gen)
                    g = graph_time(gfs)
                    gqa_us, gqa_tb = f"{g:.1f}", f"{bs * gctx * 512 / g / 1e6:.3f}"
                    del gfs
                rows.append(f"{label},{hq},{bs},{ctx},{ns},{us:.1f},{tb:.3f},{tf:.1f},{bound},{max(by_bytes, by_flop) / us:.3f},"
                            f"{kv_bytes / us / 1e6:.3f},{gqa_us},{gqa_tb}")
                print(rows[-1], flush=True)
    if out:
        new = not os.path.exists(out)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write("\n".join(rows[0 if new else 1:]) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--label", default="1")
    ap.add_argument("--hqs", default="16,32,64,128")
    ap.add_argument("--bss", default="1,32,128")
    ap.add_argument("--ctxs", default="2048,8192")
    ap.add_argument("--max-kv-splits", type=int, default=16)
    a = ap.parse_args()
    ints = lambda s: [int(v) for v in s.split(",")]
    sweep(a.out, a.label, ints(a.hqs), ints(a.bss), ints(a.ctxs), a.max_kv_splits)
