"""bf16 decode GEMMs at 1..16 rows: the weight-streaming kernel
(ops/hip/skinny.hip) against the library path it replaces, one process,
arms interleaved, in the method of tools/bench_qgemv.py.

  - M in {2, 8, 16} over the five N x K shapes: skinny vs F.linear
    (gemv and skinny at M = 1 are context)
  - q/k/v: one grouped launch vs three single launches vs three F.linear
  - gate/up: skinny_swiglu vs two F.linear + swiglu_fwd

Every arm rotates over enough distinct weight copies that no call finds
its weight in the L2 / Infinity Cache, so GB/s is an HBM figure: weight
bytes over the median per-call time (device events around graph replays
of one pass over all copies, arms alternating inside every repetition;
7 windows, median with min and max).

Run on the GPU box: python tools/bench_skinny.py [--out FILE.json]
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
FOOTPRINT = 1536 << 20       # bytes of weights an arm cycles through


def weights(N, K, copies, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(N * 7 + K + seed)
    w = (torch.randn(N, K, device=dev, generator=g) * 0.3).to(torch.bfloat16)
    return [w.clone() for _ in range(copies)]


def measure(arms, x, copies, reps, inner):
    """arms: name -> (fn(x, i) over copy i, weight bytes per call).
    Returns name -> list of per-call microseconds, one per window."""
    graphs = {}
    for n, (fn, _) in arms.items():          # warm every arm, then capture
        for i in range(min(copies, 4)):
            fn(x, i)
        torch.cuda.synchronize()
        graphs[n] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[n]):
            for i in range(copies):
                fn(x, i)
        graphs[n].replay()
    torch.cuda.synchronize()
    times = {n: [] for n in arms}
    for _ in range(reps):
        for n in arms:                       # arms alternate per window
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(inner):
                graphs[n].replay()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / (copies * inner))
    return times


def report(rows, tag, arms, times, copies):
    for n, (_, nbytes) in arms.items():
        us = statistics.median(times[n])
        row = dict(tag, arm=n, us=round(us, 2), us_min=round(min(times[n]), 2),
                   us_max=round(max(times[n]), 2),
                   weight_GBps=round(nbytes / us / 1e3, 1), copies=copies)
        rows.append(row)
        print(json.dumps(row), flush=True)


def ncopies(nbytes):
    return max(4, min(96, -(-FOOTPRINT // nbytes)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10,
                    help="graph replays per timed window")
    ap.add_argument("--batches", default="1,2,8,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_skinny needs a GPU"
    dev = torch.device("cuda")
    rows = []

    def acts(M, K):
        return (torch.randn(M, K, device=dev) * 0.3).to(torch.bfloat16)

    for N, K in SHAPES:
        nb = 2 * N * K
        copies = ncopies(nb)
        W = weights(N, K, copies, dev)
        for M in [int(b) for b in args.batches.split(",")]:
            x = acts(M, K)
            arms = {"skinny": (lambda x, i: ops.skinny_linear(x, W[i]), nb)}
            if M == 1:
                arms["gemv"] = (lambda x, i: ops.gemv(x, W[i]), nb)
            else:
                arms["linear"] = (lambda x, i: F.linear(x, W[i]), nb)
            report(rows, {"N": N, "K": K, "M": M}, arms,
                   measure(arms, x, copies, args.reps, args.inner), copies)
        del W
        torch.cuda.empty_cache()

    # q/k/v of a GQA layer: one grouped launch against separate calls
    K, Ns = 4096, (4096, 1024, 1024)
    nb = 2 * K * sum(Ns)
    copies = ncopies(nb)
    Ws = [weights(n, K, copies, dev, seed=j) for j, n in enumerate(Ns)]
    for M in (1, 8):
        x = acts(M, K)
        arms = {
            "skinny grouped": (lambda x, i: ops.skinny_linear_multi(
                x, [w[i] for w in Ws]), nb),
            "skinny x3": (lambda x, i: [ops.skinny_linear(x, w[i])
                                        for w in Ws], nb),
            "linear x3": (lambda x, i: [F.linear(x, w[i]) for w in Ws], nb)}
        report(rows, {"N": "4096+1024+1024", "K": K, "M": M}, arms,
               measure(arms, x, copies, args.reps, args.inner), copies)
    del Ws
    torch.cuda.empty_cache()

    # gate/up + SwiGLU
    N, K = 11008, 4096
    nb = 4 * N * K
    copies = ncopies(nb)
    Wg, Wu = weights(N, K, copies, dev), weights(N, K, copies, dev, seed=1)
    for M in (1, 8):
        x = acts(M, K)
        arms = {
            "skinny_swiglu": (lambda x, i: ops.skinny_swiglu(x, Wg[i], Wu[i]),
                              nb),
            "linear x2 + swiglu_fwd": (lambda x, i: ops.swiglu_fwd(
                F.linear(x, Wg[i]), F.linear(x, Wu[i])), nb)}
        report(rows, {"N": "11008 gate/up", "K": K, "M": M}, arms,
               measure(arms, x, copies, args.reps, args.inner), copies)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
