#!/usr/bin/env python3
"""FP8 base GEMM (ops/hip/gemm_fp8.hip) against the bf16 routes, in one
process with interleaved rounds, on the training shapes: the forward
layout x @ W^T and the dgrad layout dy @ (W^T)^T of every projection
family, at 24k and 64k rows.

Per shape: F.linear (hipBLASLt bf16), ops.gemm_nt (hand-written bf16),
ops.gemm_fp8_nt on operands quantized beforehand, and quant_fp8_rows of
the activation + gemm_fp8_nt (what a training step pays; the weight is
quantized once). Times are the best of the rounds; TF/s counts 2*M*N*K.

  python tools/bench_fp8_gemm.py [--rows 24576,65536] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from datatunerx_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="24576,65536")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()

assert torch.cuda.is_available() and ops.have_ext(), "needs the GPU"
dev = torch.device("cuda:0")
torch.manual_seed(0)

# (name, N, K) of W [N,K]; the dgrad of a family is the NT GEMM on W^T [K,N]
FAMILIES = [("qkvo", 4096, 4096), ("gateup", 11008, 4096),
            ("down", 4096, 11008)]


def timeit(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def rand(m, k):
    return (torch.rand((m, k), device=dev) * 2 - 1).to(torch.bfloat16)


results = []
for m in (int(r) for r in args.rows.split(",")):
    for fam, n_w, k_w in FAMILIES:
        for layout, n, k in (("fwd", n_w, k_w), ("dgrad", k_w, n_w)):
            a, b = rand(m, k), rand(n, k)
            a8, sa = ops.quant_fp8_rows(a)
            b8, sb = ops.quant_fp8_rows(b)
            # the fp8 product against the fp32 product of the SAME fp8
            # operands (kernel error), and against the bf16 product
            # (quantization error), on the first 256 rows
            got = ops.gemm_fp8_nt(a8, sa, b8, sb)[:256].float()
            deq = (a8[:256].float() * sa[:256, None]) @ \
                (b8.float() * sb[:, None]).t()
            exact = a[:256].float() @ b.float().t()
            e_k = float((got - deq).norm() / deq.norm())
            e_q = float((got - exact).norm() / exact.norm())
            del got, deq, exact
            routes = {
                "linear_bf16": lambda: torch.nn.functional.linear(a, b),
                "gemm_nt_bf16": lambda: ops.gemm_nt(a, b),
                "fp8_gemm": lambda: ops.gemm_fp8_nt(a8, sa, b8, sb),
                "fp8_quant+gemm": lambda: ops.gemm_fp8_nt(
                    *ops.quant_fp8_rows(a), b8, sb),
            }
            for fn in routes.values():
                for _ in range(3):
                    fn()
            best = {r: float("inf") for r in routes}
            for _ in range(args.rounds):          # interleaved rounds
                for r, fn in routes.items():
                    best[r] = min(best[r], timeit(fn, args.iters))
            fl = 2.0 * m * n * k
            rec = {"family": fam, "layout": layout, "M": m, "N": n, "K": k,
                   "rel_err_kernel": e_k, "rel_err_vs_bf16": e_q,
                   "ms": {r: t * 1e3 for r, t in best.items()},
                   "tflops": {r: fl / t / 1e12 for r, t in best.items()}}
            results.append(rec)
            print(f"{fam:6s} {layout:5s} M={m} N={n} K={k} "
                  f"err kernel {e_k:.1e} vs-bf16 {e_q:.1e} | " +
                  "  ".join(f"{r} {t*1e3:.3f} ms {fl/t/1e12:.0f} TF/s"
                            for r, t in best.items()), flush=True)
            del a, b, a8, b8, routes
            torch.cuda.empty_cache()

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
