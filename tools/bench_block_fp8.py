"""Kernel-level timing of the block-wise fp8 linear at the Llama-3-8B projection shapes:
  bench_block_fp8.py [--out CSV] [--label L] [--ms 1,32,...]
fp8_blockwise_scaled_mm against this tree's fp8_scaled_mm on the same shape -- the same operand bytes and the same MFMA work, but a
per-row x per-column scale applied once after the K loop.  Each path is captured in a HIP graph that walks over several copies of
the weight (a model's layers do not find their weights in the caches), warmed up, and replayed `reps` times; the median counts.
A row is bound by bytes (x + w + y + scales over 8 TB/s) or by FLOPs (2 M N K over 5 PFLOP/s fp8), whichever takes longer; the
CSV says which and gives the achieved rate of that kind."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from __graft_entry__ import load_package

load_package()
from ltp_sglang_amd import sgl_kernel as K

LLAMA3_8B = [("qkv", 6144, 4096), ("o_proj", 4096, 4096), ("gate_up", 28672, 4096), ("down", 4096, 14336)]
HEADER = "run,shape,M,N,K,form,block_us,scaled_us,block_over_scaled,bound,block_TB_per_s,block_TFLOP_per_s"


def graph_time(fs, reps=10):
    """Median time in us of one call of the list `fs`, replayed as one captured graph."""
    for f in fs:
        f()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=st):
        for f in fs:
            f()
    gr.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / len(fs))
    return sorted(ts)[len(ts) // 2]


def sweep(out, label, ms, copies=6):
    dev = "cuda:0"
    rows = [HEADER]
    print(HEADER, flush=True)
    for name, n, k in LLAMA3_8B:
        gen = torch.Generator(device=dev).manual_seed(0)
        ws = []
        for _ in range(max(2, min(copies, int(1.0e9 // (n * k))))):
            w = torch.randn(n, k, generator=gen, device=dev).to(torch.float8_e4m3fn)
            ws.append((w, torch.rand(n // 128, k // 128, generator=gen, device=dev) * 0.02 + 1e-3,
                       torch.rand(n, generator=gen, device=dev) * 0.02 + 1e-3))
        for m in ms:
            x = torch.randn(m, k, generator=gen, device=dev).to(torch.float8_e4m3fn)
            sxb = torch.rand(m, k // 128, generator=gen, device=dev) * 0.02 + 1e-3
            sxr = torch.rand(m, generator=gen, device=dev) * 0.02 + 1e-3
            blk = graph_time([(lambda w=w: K.fp8_blockwise_scaled_mm(x, w[0].T, sxb, w[1].T, torch.bfloat16)) for w in ws])
            sca = graph_time([(lambda w=w: K.fp8_scaled_mm(x, w[0].T, sxr, w[2], torch.bfloat16)) for w in ws])
            nbytes = m * k + n * k + 2 * m * n + 4 * (m + n // 128) * (k // 128)
            flops = 2.0 * m * n * k
            bound = "bytes" if nbytes / 8e12 >= flops / 5e15 else "flops"
            rows.append(f"{label},{name},{m},{n},{k},{K.fp8_blockwise_gemm_form(m, n, k)},{blk:.1f},{sca:.1f},{blk / sca:.2f},{bound},"
                        f"{nbytes / blk / 1e6:.3f},{flops / blk / 1e6:.1f}")
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
