"""Kernel-level timing of the MLA (576 / 512 latent-KV) extend attention, causal, bf16:
  bench_mla_extend.py [--out CSV] [--label L] [--hqs 16,128] [--cases 1x0+2048,4x0+2048,4x2048+512,1x0+8192]
A case is BATCH x PREFIX + NEW tokens per request.  Timing as tools/bench_mla_decode.py: the call captured in a HIP graph that walks
over several disjoint copies of the inputs (own q, k_extend, o and randomly permuted prefix slots of one pool), warmed up, replayed;
the median counts.  Per row: microseconds; workgroups of the launch (row blocks of 64 (token, head) pairs); FLOP counted as
2 x (576 + 512) per VISIBLE (row, key) pair -- the masked half of a diagonal tile and the padding of a last tile are computed but not
counted -- over that time, and its share of the bare bf16 MFMA rate tools/microbench/mfma_rate.hip measured (1 650 TFLOP/s taken);
the algorithmic bytes (q, o, every new row and every prefix row once) over that time for completeness: every case here is FLOP-bound
by that count.  Run it twice (--label 1 / 2) into one CSV: the spread between the runs is the noise."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools.bench_block_fp8 import graph_time

from ltp_sglang_amd import sgl_kernel as K

HEADER = "run,Hq,bs,prefix,new,workgroups,us,TFLOP_per_s,share_of_mfma_rate,TB_per_s"
MFMA_FLOPS = 1.65e15
D, DV = 576, 512


def _calls(hq, bs, pre, ext, copies, gen):
    dev, dt = "cuda:0", torch.bfloat16
    t = bs * ext
    rows = copies * bs * pre + 1
    pool = torch.randn(rows, 1, D, generator=gen, device=dev, dtype=torch.float32).to(dt) if pre else None
    perm = (torch.randperm(rows - 1, generator=gen, device=dev) + 1).int()
    qo_indptr = torch.arange(0, (bs + 1) * ext, ext, dtype=torch.int32, device=dev)
    kv_indptr = torch.arange(0, (bs + 1) * pre, pre, dtype=torch.int32, device=dev) if pre else torch.zeros(bs + 1, dtype=torch.int32, device=dev)
    fs = []
    for c in range(copies):
        q = torch.randn(t, hq, D, generator=gen, device=dev, dtype=torch.float32).to(dt)
        k = torch.randn(t, 1, D, generator=gen, device=dev, dtype=torch.float32).to(dt)
        o = torch.empty(t, hq, DV, dtype=dt, device=dev)
        idx = perm[c * bs * pre:(c + 1) * bs * pre].contiguous()
        fs.append(lambda q=q, k=k, o=o, idx=idx: K.extend_attention_fwd(
            q, k, k[..., :DV], o, pool, None if pool is None else pool[..., :DV], qo_indptr, kv_indptr, idx, None, True, None, ext,
            192 ** -0.5))
    return fs


def sweep(out, label, hqs, cases):
    rows = [HEADER]
    print(HEADER, flush=True)
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    for bs, pre, ext in cases:
        for hq in hqs:
            copies = max(2, min(4, int(1.5e9 // (bs * ext * hq * (D + DV) * 2))))
            fs = _calls(hq, bs, pre, ext, copies, gen)
            us = graph_time(fs)
            del fs
            pairs = bs * hq * (ext * pre + ext * (ext + 1) // 2)
            flop = 2.0 * (D + DV) * pairs
            nbytes = bs * ext * hq * (D + DV) * 2 + bs * (pre + ext) * D * 2
            rows.append(f"{label},{hq},{bs},{pre},{ext},{bs * ((ext * hq + 63) // 64)},{us:.1f},{flop / us / 1e6:.1f},"
                        f"{flop / MFMA_FLOPS * 1e6 / us:.3f},{nbytes / us / 1e6:.3f}")
            print(rows[-1], flush=True)
    if out:
        new = not os.path.exists(out)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write("\n".join(rows[0 if new else 1:]) + "\n")


def _case(s):
    bs, rest = s.split("x")
    pre, ext = rest.split("+")
    return int(bs), int(pre), int(ext)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--label", default="1")
    ap.add_argument("--hqs", default="16,128")
    ap.add_argument("--cases", default="1x0+2048,4x0+2048,4x2048+512,1x0+8192")
    a = ap.parse_args()
    sweep(a.out, a.label, [int(v) for v in a.hqs.split(",")], [_case(c) for c in a.cases.split(",")])
