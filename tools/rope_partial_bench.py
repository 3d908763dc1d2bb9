"""GPU: the partial-rotary launch (slam_head_rope_partial) against rope_inplace at one shape (default: the headline's row count
M = 11780 with 32 heads of D = 128, rot = 96, inside a buffer of 40 heads' width).  Each launch is timed with device events over --iters
calls on --bufs rotating buffers (more bytes than the L2 + MALL hold, so the reads come from HBM), the variants alternating in one
process.  Prints one JSON line per variant: us per launch, the bytes the algorithm needs (computed here from the shape: the partial
launch neither reads nor writes dims [rot, D)) and GB/s.
Kernel-only times: run under `rocprofv3 --kernel-trace --stats -- python tools/rope_partial_bench.py`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=11780)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--rot", type=int, default=96)
    ap.add_argument("--extra", type=int, default=8 * 128, help="columns behind the rotated heads (v heads, LoRA-A columns)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--bufs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from slam_llm_amd import ops
    from slam_llm_amd.host_tables import rope_tables
    dev = torch.device("cuda:0")
    M, H, D, rot = args.rows, args.heads, args.d, args.rot
    N = H * D + args.extra
    g = torch.Generator(device=dev).manual_seed(0)
    bufs = [torch.randn(M, N, generator=g, device=dev).to(torch.bfloat16) for _ in range(args.bufs)]
    cos, sin = [t.to(dev) for t in rope_tables(M, D, 1e4)]
    pcos, psin = [t.to(dev) for t in rope_tables(M, D, 1e4, rot_dim=rot)]
    full, part = 4.0 * M * H * D, 4.0 * M * H * rot     # bf16 read once + written once
    variants = {
        "rope_inplace": (lambda i: ops.rope_inplace(bufs[i], 0, 1, M, H, D, cos, sin), full),
        f"head_rope_partial(rot={rot})": (lambda i: ops.rope_inplace(bufs[i], 0, 1, M, H, D, pcos, psin, rot_dim=rot), part),
        f"head_rope_partial(rot={rot}, inverse)": (lambda i: ops.rope_inplace(bufs[i], 0, 1, M, H, D, pcos, psin, rot_dim=rot, inverse=True), part),
        f"head_rope_partial(rot={D})": (lambda i: ops.head_rope_partial(bufs[i], 0, 1, M, H, D, D, cos, sin), full),
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
        print(json.dumps(dict(kernel=name, rows=M, heads=H, D=D, ld=N, us=round(best[name], 2), bytes=int(nbytes),
                              gb_per_s=round(nbytes / best[name] * 1e-3, 1), vs_rope=round(best[name] / best["rope_inplace"], 3))))


if __name__ == "__main__":
    main()
