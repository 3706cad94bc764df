"""Kernel-level timing of the NVFP4 (w4a16) linear at the Llama-3-8B projection shapes:
  bench_nvfp4.py [--out CSV] [--label L] [--ms 1,32,...] [--dtypes bf16,f16]
The fused nvfp4_gemm against the unfused route of the same method (nvfp4_dequantize + dense_linear, the weight re-materialised
on every call as PetitNvFp4LinearMethod.apply does above FUSED_MAX_M) and against this tree's fp8_scaled_mm on the same shape (one
byte per weight where NVFP4 streams 9/16).  Timing as tools/bench_int8.py: each path captured in a HIP graph that walks over
several copies of the weight, warmed up, replayed; the median counts.  fused_TB_per_s is the fused kernel's own bytes (x + 9/16
byte per weight + y) over its time.  Run it twice (--label 1 / 2) into one CSV: the spread between the runs is the noise."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tools.bench_block_fp8 import LLAMA3_8B, graph_time

from ltp_sglang_amd import sgl_kernel as K

HEADER = ("run,shape,dtype,M,N,K,form,kranges,fused_us,unfused_us,fp8_us,fused_over_unfused,fused_over_fp8,fused_TB_per_s")
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def sweep(out, label, ms, dtypes, copies=6):
    dev = "cuda:0"
    rows = [HEADER]
    print(HEADER, flush=True)
    for name, n, k in LLAMA3_8B:
        gen = torch.Generator(device=dev).manual_seed(0)
        gs = torch.tensor(0.009, device=dev)
        ws = []
        for _ in range(max(2, min(copies, int(1.0e9 // (n * k))))):
            w = torch.randint(0, 256, (n, k // 2), generator=gen, device=dev, dtype=torch.uint8)
            s = torch.randint(0x08, 0x41, (n, k // 16), generator=gen, device=dev, dtype=torch.uint8).view(torch.float8_e4m3fn)
            ws.append((w, s, K.nvfp4_repack(w, s), torch.randn(n, k, generator=gen, device=dev).to(torch.float8_e4m3fn),
                       torch.rand(n, generator=gen, device=dev) * 0.02 + 1e-3))
        for dname in dtypes:
            dt = DTYPES[dname]
            for m in ms:
                x = torch.randn(m, k, generator=gen, device=dev).to(dt)
                xf = torch.randn(m, k, generator=gen, device=dev).to(torch.float8_e4m3fn)
                sx = torch.rand(m, generator=gen, device=dev) * 0.02 + 1e-3
                fused = graph_time([(lambda w=w: K.nvfp4_gemm(x, w[2][0], w[2][1], gs)) for w in ws])
                unf = graph_time([(lambda w=w: K.dense_linear(x, K.nvfp4_dequantize(w[0], w[1], dt, gs))) for w in ws])
                f8 = graph_time([(lambda w=w: K.fp8_scaled_mm(xf, w[3].T, sx, w[4], dt)) for w in ws])
                nbytes = 2 * m * k + n * k * 9 // 16 + 2 * m * n
                rows.append(f"{label},{name},{dname},{m},{n},{k},{K.nvfp4_gemm_form(m, n, k)},{K.nvfp4_gemm_kranges(m, n, k)},"
                            f"{fused:.1f},{unf:.1f},{f8:.1f},{fused / unf:.2f},{fused / f8:.2f},{nbytes / fused / 1e6:.3f}")
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
    ap.add_argument("--ms", default="1,32,64,128,256,512,1024,4096")
    ap.add_argument("--dtypes", default="bf16,f16")
    a = ap.parse_args()
    sweep(a.out, a.label, [int(v) for v in a.ms.split(",")], a.dtypes.split(","))
