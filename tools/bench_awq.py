"""Kernel-level timing of the AWQ int4 linear at the Qwen2-7B shapes.
  bench_awq.py [f16]                     M = 32: fused dequant-GEMM vs the reference's unfused structure (awq_dequantize + transpose + GEMM)
  bench_awq.py sweep [--out CSV] [--label L]   M = 128 .. 8192, f16 and bf16: the tiled fused kernel vs awq_unpack_nk + dense_linear"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from __graft_entry__ import load_package
load_package()
from ltp_sglang_amd import sgl_kernel as K, _cabi
from ltp_sglang_amd._cabi import check, lib, ptr, current_stream

def graph_time(fs, iters=10):
    for f in fs: f()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(); st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for f in fs: f()
    torch.cuda.current_stream().wait_stream(st)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=st):
        for f in fs: f()
    gr.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); gr.replay(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / len(fs))
    ts.sort(); return ts[len(ts) // 2]

def run(m, k, n, g=128, dtype=torch.bfloat16, copies=8):
    dev = "cuda:0"
    copies = max(2, min(copies, int(1.0e9 // (k * n // 2))))
    gen = torch.Generator(device=dev).manual_seed(0)
    ws = []
    for _ in range(copies):
        qw = torch.randint(-2**31, 2**31 - 1, (k, n // 8), generator=gen, dtype=torch.int32, device=dev)
        qz = torch.randint(-2**31, 2**31 - 1, (k // g, n // 8), generator=gen, dtype=torch.int32, device=dev)
        sc = (torch.rand(k // g, n, generator=gen, device=dev) * 0.01).to(dtype)
        ws.append((qw, qz, sc) + K.awq_repack(qw, sc, qz))
    x = torch.randn(m, k, device=dev).to(dtype)
    fused = graph_time([(lambda w=w: K.awq_gemm(x, w[3], w[4], g)) for w in ws])
    if os.environ.get("AWQ_BENCH_FUSED_ONLY"):
        print(f"M={m} K={k} N={n}: fused {fused*1e3:7.1f} us ({k*n/2/fused/1e6:6.0f} GB/s of int4)", flush=True)
        return
    def unfused(w):
        wkn = K.awq_dequantize(w[0], w[2], w[1])
        wnk = torch.empty((n, k), dtype=dtype, device=dev)
        check(lib.sgl_mi355_transpose_2d(ptr(wnk), ptr(wkn), k, n, current_stream()))
        return K.dense_linear(x, wnk)
    unf = graph_time([(lambda w=w: unfused(w)) for w in ws[:2]], iters=5)
    print(f"M={m} K={k} N={n}: fused {fused*1e3:7.1f} us ({k*n/2/fused/1e6:6.0f} GB/s of int4)   dequant+GEMM {unf*1e3:8.1f} us   x{unf/fused:.1f}", flush=True)

QWEN2_7B = [("qkv", 3584, 4608), ("o_proj", 3584, 3584), ("gate_up", 3584, 37888), ("down", 18944, 3584)]


def sweep(out=None, label="1", ms=(128, 256, 512, 1024, 2048, 4096, 8192), g=128, reps=7, inner=6):
    """Fused vs awq_unpack_nk + dense_linear, alternating in one process, each timed with device events around `inner` calls that
    walk over several copies of the weight (a model's layers do not find their weights in the caches); median of `reps`.
    Bytes: what the fused kernel has to move once (int4 + sz + x + y) against 8 TB/s; FLOP = 2 M N K."""
    dev = "cuda:0"
    rows = ["run,shape,dtype,M,K,N,kranges,fused_us,unfused_us,unfused_over_fused,fused_TB_per_s,fused_pct_of_8TBps,fused_TFLOP_per_s"]
    print(rows[0], flush=True)
    for dtype in (torch.float16, torch.bfloat16):
        for name, k, n in QWEN2_7B:
            gen = torch.Generator(device=dev).manual_seed(0)
            ws = []
            for _ in range(max(2, min(inner, int(1.0e9 // (k * n // 2))))):
                qw = torch.randint(-2**31, 2**31 - 1, (k, n // 8), generator=gen, dtype=torch.int32, device=dev)
                qz = torch.randint(-2**31, 2**31 - 1, (k // g, n // 8), generator=gen, dtype=torch.int32, device=dev)
                sc = (torch.rand(k // g, n, generator=gen, device=dev) * 0.01).to(dtype)
                ws.append(K.awq_repack(qw, sc, qz))
                del qw, qz, sc
            for m in ms:
                x = torch.randn(m, k, device=dev).to(dtype)
                paths = {"fused": lambda w: K.awq_gemm(x, w[0], w[1], g),
                         "unfused": lambda w: K.dense_linear(x, K.awq_unpack_nk(w[0], w[1], g, dtype))}
                times = {"fused": [], "unfused": []}
                for rep in range(reps + 1):      # rep 0 warms both paths
                    for tag, f in paths.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for j in range(inner):
                            f(ws[j % len(ws)])
                        e1.record()
                        torch.cuda.synchronize()
                        if rep:
                            times[tag].append(e0.elapsed_time(e1) * 1e3 / inner)
                fu, un = (sorted(times[t])[reps // 2] for t in ("fused", "unfused"))
                nbytes = k * n // 2 + (k // g) * n * 4 + 2 * m * k + 2 * m * n
                rows.append(f"{label},{name},{str(dtype)[6:]},{m},{k},{n},{K.awq_gemm_tiled_kranges(m, n, k)},{fu:.1f},{un:.1f},{un / fu:.2f},"
                            f"{nbytes / fu / 1e6:.3f},{nbytes / fu / 1e6 / 8 * 100:.1f},{2.0 * m * n * k / fu / 1e6:.1f}")
                print(rows[-1], flush=True)
            del ws
    if out:
        new = not os.path.exists(out)
        with open(out, "a") as f:
            f.write("\n".join(rows[0 if new else 1:]) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "sweep":
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("mode")
        ap.add_argument("--out")
        ap.add_argument("--label", default="1")
        a = ap.parse_args()
        sweep(a.out, a.label)
        sys.exit(0)
    dt = torch.float16 if len(sys.argv) > 1 and sys.argv[1] == "f16" else torch.bfloat16
    print(dt)
    for k, n in [(3584, 4608), (3584, 3584), (3584, 37888), (18944, 3584), (4096, 6144), (4096, 28672), (14336, 4096)]:
        run(32, k, n, dtype=dt)
