"""Quantized decode kernels vs the paths they replace, one process, arms
interleaved: bf16 gemv / qgemv int8 / qgemv int4 at M = 1, and for
M in {2, 8, 16} the MFMA qgemv against dequant + F.linear (what a
quantized layer did before) and against bf16 F.linear (context).

Every arm rotates over enough distinct weight copies that no call finds
its weight in the L2 / Infinity Cache (the decode step streams ~all
weights once per token), so GB/s is an HBM figure: weight bytes of the
arm's own format over the median per-call time (device events around
one pass over all copies, arms alternating inside every repetition).

Run on the GPU box: python tools/bench_qgemv.py [--out FILE.json]
"""

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datatunerx_amd import ops  # noqa: E402

SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008), (32000, 4096),
          (1024, 4096)]
GROUP = 64
FOOTPRINT = 768 << 20        # bytes the smallest (int4) arm cycles through


def make_weights(N, K, copies, dev):
    g = torch.Generator(device=dev).manual_seed(N * 7 + K)
    w = (torch.randn(N, K, device=dev, generator=g) * 0.3).to(torch.bfloat16)
    q8 = torch.randint(-127, 128, (N, K), device=dev, generator=g,
                       dtype=torch.int8)
    s8 = torch.rand(N, device=dev, generator=g) * 0.01 + 1e-3
    q4 = torch.randint(0, 256, (N, K // 2), device=dev, generator=g,
                       dtype=torch.uint8)
    s4 = torch.rand(N, K // GROUP, device=dev, generator=g) * 0.1 + 1e-2
    rep = lambda t: [t.clone() for _ in range(copies)]   # noqa: E731
    return {"bf16": rep(w), "q8": rep(q8), "s8": rep(s8), "q4": rep(q4),
            "s4": rep(s4)}


def arms_for(M, W):
    """name -> (fn(i) running copy i, weight bytes per call)."""
    N, K = W["bf16"][0].shape
    b16, b8, b4 = 2 * N * K, N * K + 4 * N, N * K // 2 + 4 * N * (K // GROUP)
    a = {}
    if M == 1:
        a["gemv bf16"] = (lambda x, i: ops.gemv(x, W["bf16"][i]), b16)
    else:
        a["linear bf16"] = (lambda x, i: F.linear(x, W["bf16"][i]), b16)
        a["dequant+linear int8"] = (
            lambda x, i: F.linear(x, ops.dequant_int8(W["q8"][i],
                                                      W["s8"][i])), b8)
        a["dequant+linear int4"] = (
            lambda x, i: F.linear(x, ops.dequant_int4(W["q4"][i], W["s4"][i],
                                                      GROUP)), b4)
    a["qgemv int8"] = (lambda x, i: ops.qlinear(x, W["q8"][i], W["s8"][i],
                                                8), b8)
    a["qgemv int4"] = (lambda x, i: ops.qlinear(x, W["q4"][i], W["s4"][i],
                                                4, GROUP), b4)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10,
                    help="graph replays per timed window")
    ap.add_argument("--batches", default="1,2,8,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_qgemv needs a GPU"
    dev = torch.device("cuda")
    rows = []
    for N, K in SHAPES:
        copies = max(4, min(96, -(-FOOTPRINT // (N * K // 2))))
        W = make_weights(N, K, copies, dev)
        for M in [int(b) for b in args.batches.split(",")]:
            x = (torch.randn(M, K, device=dev) * 0.3).to(torch.bfloat16)
            if M == 1:
                x = x.view(1, 1, K)
            arms = arms_for(M, W)
            times = {n: [] for n in arms}
            graphs = {}
            for n, (fn, _) in arms.items():      # warm every arm/shape
                for i in range(min(copies, 4)):
                    fn(x, i)
                torch.cuda.synchronize()
                # one pass over all copies as a hipGraph: these kernels
                # run for microseconds, an eager loop would time the
                # Python launch rate (and decode replays a graph anyway)
                graphs[n] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[n]):
                    for i in range(copies):
                        fn(x, i)
                graphs[n].replay()
            torch.cuda.synchronize()
            for _ in range(args.reps):
                for n in arms:                   # arms alternate per rep
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _i in range(args.inner):
                        graphs[n].replay()
                    e1.record()
                    e1.synchronize()
                    times[n].append(e0.elapsed_time(e1) * 1e3 /
                                    (copies * args.inner))
            del graphs
            for n, (_, nbytes) in arms.items():
                us = statistics.median(times[n])
                row = {"N": N, "K": K, "M": M, "arm": n,
                       "us": round(us, 2),
                       "us_min": round(min(times[n]), 2),
                       "us_max": round(max(times[n]), 2),
                       "weight_GBps": round(nbytes / us / 1e3, 1),
                       "copies": copies}
                rows.append(row)
                print(json.dumps(row), flush=True)
        del W
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
