"""Gathered multi-adapter LoRA update (ops.mlora_add: shrink + expand,
8 adapters, a different one per row) against the single-adapter path it
stands in for at decode (ops.lora_contract + ops.lora_expand_add, one
adapter for all rows), same M, one process, arms interleaved.

Every arm rotates over enough distinct adapter copies that a call does
not find its adapter in the L2 / Infinity Cache (in a decode step the
base-weight stream evicts it between tokens). Timing: device events
around a hipGraph of one pass over all copies — the kernels run for
microseconds, an eager loop would time the launch rate.

Run on the GPU box: python tools/bench_mlora.py [--out FILE.json]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datatunerx_amd import ops  # noqa: E402

SHAPES = [(4096, 4096), (4096, 1024), (4096, 11008), (11008, 4096)]  # (K, N)
RANKS = [8, 16, 64]
G = 8
FOOTPRINT = 320 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10,
                    help="graph replays per timed window")
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mlora needs a GPU"
    dev = torch.device("cuda")
    rows = []
    for K, N in SHAPES:
        for R in RANKS:
            g = torch.Generator(device=dev).manual_seed(K + 3 * N + R)
            # copies sized on the SINGLE adapter (the smaller arm)
            copies = max(4, min(128, -(-FOOTPRINT // (2 * R * (K + N)))))
            mk = lambda *s: (torch.randn(*s, device=dev, generator=g)  # noqa: E731
                             * 0.05).to(torch.bfloat16)
            stacks = [(mk(G, R, K), mk(G, R, N)) for _ in range(copies)]
            singles = [(mk(R, K), mk(N, R)) for _ in range(copies)]
            scale = torch.full((G,), 2.0, device=dev)
            for M in [int(b) for b in args.batches.split(",")]:
                x = (torch.randn(M, K, device=dev, generator=g) * 0.3) \
                    .to(torch.bfloat16)
                y = (torch.randn(M, N, device=dev, generator=g) * 0.3) \
                    .to(torch.bfloat16)
                idx = (torch.arange(M, device=dev) % G).to(torch.int32)
                assert ops.mlora_supported(M, N, K, R)

                def multi(i):
                    ops.mlora_add(y, x, stacks[i][0], stacks[i][1], scale,
                                  idx)

                def single(i):
                    t = ops.lora_contract(x, singles[i][0])
                    ops.lora_expand_add(y, t, singles[i][1], 2.0)

                arms = {"mlora (8 adapters)": multi,
                        "lora_contract+expand (1 adapter)": single}
                graphs, times = {}, {n: [] for n in arms}
                for n, fn in arms.items():
                    for i in range(min(copies, 4)):
                        fn(i)
                    torch.cuda.synchronize()
                    graphs[n] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs[n]):
                        for i in range(copies):
                            fn(i)
                    graphs[n].replay()
                torch.cuda.synchronize()
                for _ in range(args.reps):
                    for n in arms:               # arms alternate per rep
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
                us = {n: statistics.median(t) for n, t in times.items()}
                names = list(arms)
                row = {"K": K, "N": N, "R": R, "M": M,
                       "mlora_us": round(us[names[0]], 2),
                       "mlora_us_min": round(min(times[names[0]]), 2),
                       "mlora_us_max": round(max(times[names[0]]), 2),
                       "single_us": round(us[names[1]], 2),
                       "single_us_min": round(min(times[names[1]]), 2),
                       "single_us_max": round(max(times[names[1]]), 2),
                       "ratio": round(us[names[0]] / us[names[1]], 2),
                       "copies": copies}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del stacks, singles
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
