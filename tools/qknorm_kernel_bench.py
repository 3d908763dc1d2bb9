"""GPU: the Qwen3 per-head norm kernels against the RoPE launch they stand in for, at one shape (default: the headline's row count
M = 11780 with 32 + 8 heads of D = 128 inside the fused q|k|v buffer).  Each launch is timed with device events over --iters calls
on --bufs rotating buffers (more bytes than the L2 + MALL hold, so the reads come from HBM), the variants alternating in one process.
Prints one JSON line per kernel: us per launch, the bytes the algorithm needs (computed here from the shape) and GB/s.
Kernel-only times: run under `rocprofv3 --kernel-trace --stats -- python tools/qknorm_kernel_bench.py`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=11780)
    ap.add_argument("--hq", type=int, default=32)
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--lora", type=int, default=0, help="extra LoRA-A columns behind q|k|v (the leading dimension grows by this)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--bufs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from slam_llm_amd import ops
    from slam_llm_amd.host_tables import rope_tables
    dev = torch.device("cuda:0")
    M, Hq, Hkv, D = args.rows, args.hq, args.hkv, args.d
    H, N = Hq + Hkv, (Hq + 2 * Hkv) * D + args.lora
    g = torch.Generator(device=dev).manual_seed(0)
    bufs = [torch.randn(M, N, generator=g, device=dev).to(torch.bfloat16) for _ in range(args.bufs)]
    grads = [torch.randn(M, N, generator=g, device=dev).to(torch.bfloat16) for _ in range(args.bufs)]
    wq, wk = 1 + 0.1 * torch.randn(D, generator=g, device=dev), 1 + 0.1 * torch.randn(D, generator=g, device=dev)
    cos, sin = [t.to(dev) for t in rope_tables(M, D, 1e6)]
    rstd, x = ops.head_rmsnorm_rope(bufs[0].clone(), 0, 1, M, Hq, Hkv, D, wq, wk, 1e-6, cos, sin, stash=True)
    qk = 2.0 * M * H * D        # bytes of the q|k columns, once
    variants = {
        # name: (launch on buffer i, algorithmic bytes)
        "rope_inplace": (lambda i: ops.rope_inplace(bufs[i], 0, 1, M, H, D, cos, sin), 2 * qk),
        "head_rmsnorm_rope(eval)": (lambda i: ops.head_rmsnorm_rope(bufs[i], 0, 1, M, Hq, Hkv, D, wq, wk, 1e-6, cos, sin), 2 * qk),
        "head_rmsnorm_rope(train, stash)": (lambda i: ops.head_rmsnorm_rope(bufs[i], 0, 1, M, Hq, Hkv, D, wq, wk, 1e-6, cos, sin, stash=True),
                                            3 * qk + 4.0 * M * H),
        "head_rmsnorm_bwd": (lambda i: ops.head_rmsnorm_bwd(grads[i], 0, x, rstd, Hq, Hkv, D, wq, wk), 3 * qk + 4.0 * M * H),
    }
    best = {k: float("inf") for k in variants}
    for _ in range(args.rounds):        # alternate the variants: drift of the clock hits all of them alike
        for name, (fn, _) in variants.items():
            for i in range(args.bufs):
                fn(i)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for it in range(args.iters):
                fn(it % args.bufs)
            t1.record()
            torch.cuda.synchronize()
            best[name] = min(best[name], t0.elapsed_time(t1) * 1e3 / args.iters)
    for name, (_, nbytes) in variants.items():
        print(json.dumps(dict(kernel=name, rows=M, heads=f"{Hq}+{Hkv}", D=D, ld=N, us=round(best[name], 2), bytes=int(nbytes),
                              gb_per_s=round(nbytes / best[name] * 1e-3, 1),
                              vs_rope=round(best[name] / best["rope_inplace"], 3))))


if __name__ == "__main__":
    main()
