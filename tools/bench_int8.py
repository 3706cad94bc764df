"""Kernel-level timing of the int8 w8a8 linear at the Llama-3-8B projection shapes:
  bench_int8.py [--out CSV] [--label L] [--ms 1,32,...]
int8_scaled_mm against this tree's fp8_scaled_mm on the same shape -- the same operand bytes and the same MFMA count per byte.
Timing as tools/bench_block_fp8.py: each path captured in a HIP graph that walks over several copies of the weight, warmed up,
replayed; the median counts.  A row is bound by bytes (x + w + y + scales over 8 TB/s) or by ops (2 M N K over 5 POP/s int8),
whichever takes longer; the CSV says which and gives the achieved rate of that kind."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools.bench_block_fp8 import LLAMA3_8B, graph_time

from ltp_sglang_amd import sgl_kernel as K

HEADER = "run,shape,M,N,K,form,int8_us,fp8_us,int8_over_fp8,bound,int8_TB_per_s,int8_TOP_per_s"


def sweep(out, label, ms, copies=6):
    dev = "cuda:0"
    rows = [HEADER]
    print(HEADER, flush=True)
    for name, n, k in LLAMA3_8B:
        gen = torch.Generator(device=dev).manual_seed(0)
        ws = []
        for _ in range(max(2, min(copies, int(1.0e9 // (n * k))))):
            w8 = torch.randint(-128, 128, (n, k), generator=gen, device=dev, dtype=torch.int8)
            ws.append((w8, torch.randn(n, k, generator=gen, device=dev).to(torch.float8_e4m3fn),
                       torch.rand(n, generator=gen, device=dev) * 0.02 + 1e-3))
        for m in ms:
            x8 = torch.randint(-128, 128, (m, k), generator=gen, device=dev, dtype=torch.int8)
            xf = torch.randn(m, k, generator=gen, device=dev).to(torch.float8_e4m3fn)
            sx = torch.rand(m, generator=gen, device=dev) * 0.02 + 1e-3
            i8 = graph_time([(lambda w=w: K.int8_scaled_mm(x8, w[0].T, sx, w[2], torch.bfloat16)) for w in ws])
            f8 = graph_time([(lambda w=w: K.fp8_scaled_mm(xf, w[1].T, sx, w[2], torch.bfloat16)) for w in ws])
            nbytes = m * k + n * k + 2 * m * n + 4 * (m + n)
            ops = 2.0 * m * n * k
            bound = "bytes" if nbytes / 8e12 >= ops / 5e15 else "ops"
            rows.append(f"{label},{name},{m},{n},{k},{K.int8_gemm_form(m, n, k)},{i8:.1f},{f8:.1f},{i8 / f8:.2f},{bound},"
                        f"{nbytes / i8 / 1e6:.3f},{ops / i8 / 1e6:.1f}")
            print(rows[-1], flush=True)
        del ws
    if out:
        new = not os.path.exists(out)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write("\n".join(rows[0 if new else 1:]) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--label", default="1")
    ap.add_argument("--ms", default="1,32,64,128,512,4096")
    a = ap.parse_args()
    sweep(a.out, a.label, [int(v) for v in a.ms.split(",")])
