#!/usr/bin/env python3
"""Probe for the frozen-base GEMMs at the bench's mb 64 shapes: the dgrad
of a frozen projection as dy @ W against F.linear(dy, W^T) on a cached
transposed copy, the same for the accumulating dgrads (addmm_), and
torch.addmm(res, x, W.t()) against ops.gemm_nt_add (hipBLASLt, C != D).

One process, device events, arms interleaved, 7 windows of 5 calls per
arm; median and min-max per arm. Not a test.

  python tools/bench_basegemm.py [--windows 7] [--iters 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from datatunerx_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--iters", type=int, default=5)
args = ap.parse_args()

assert torch.cuda.is_available() and ops.have_ext()
dev = torch.device("cuda:0")
torch.manual_seed(0)

# (family, M, N, K): the weight is [N,K]; forward x [M,K] -> y [M,N]
SHAPES = [
    ("qkvo", 65536, 4096, 4096),
    ("gate/up", 65536, 11008, 4096),
    ("down", 65536, 4096, 11008),
    ("lm_head", 65472, 32000, 4096),
]


def rnd(*shape):
    return (torch.rand(shape, device=dev) * 2 - 1).to(torch.bfloat16)


def window(fn, iters):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters          # ms per call


def interleaved(arms):
    """arms: {name: fn}. Warm every arm, then args.windows rounds with the
    arms taking turns. -> {name: (median, min, max)} in ms."""
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in arms}
    for _ in range(args.windows):
        for name, fn in arms.items():
            t[name].append(window(fn, args.iters))
    return {name: (statistics.median(v), min(v), max(v))
            for name, v in t.items()}


def report(probe, family, M, N, K, res):
    fl = 2.0 * M * N * K
    for arm, (med, lo, hi) in res.items():
        print(json.dumps({
            "probe": probe, "family": family, "M": M, "N": N, "K": K,
            "arm": arm, "ms_median": round(med, 4), "ms_min": round(lo, 4),
            "ms_max": round(hi, 4), "tflops_median": round(fl / med / 1e9, 1),
        }), flush=True)


print(json.dumps({"workspace_bytes":
                  ops._load_ext().gemm_nt_add_workspace_bytes()}),
      flush=True)

for family, M, N, K in SHAPES:
    w = rnd(N, K)
    wt = w.t().contiguous()
    dy = rnd(M, N)
    # (a) plain dgrad dx[M,K] = dy[M,N] @ W[N,K]
    res = interleaved({"dy@W": lambda: dy @ w,
                       "linear(dy,Wt)": lambda: F.linear(dy, wt)})
    report("a_dgrad", family, M, N, K, res)
    # (b) accumulating dgrad, beta = 1 in place
    acc = rnd(M, K)
    res = interleaved({"addmm_(dy,W)": lambda: acc.addmm_(dy, w),
                       "addmm_(dy,Wt.t())": lambda: acc.addmm_(dy, wt.t())})
    report("b_dgrad_acc", family, M, N, K, res)
    del dy, acc, wt
    torch.cuda.empty_cache()
    if family in ("qkvo", "down"):
        # (c) forward with the residual: o_proj and down_proj only
        x, r = rnd(M, K), rnd(M, N)
        got = ops.gemm_nt_add(x[:256], w, r[:256]).float()
        want = x[:256].float() @ w.float().t() + r[:256].float()
        err = float((got - want).abs().max() / want.abs().max())
        res = interleaved({
            "torch.addmm": lambda: torch.addmm(r, x, w.t()),
            "gemm_nt_add": lambda: ops.gemm_nt_add(x, w, r),
            "F.linear(floor)": lambda: F.linear(x, w)})
        report("c_residual", family, M, N, K, res)
        print(json.dumps({"probe": "c_residual", "family": family,
                          "gemm_nt_add_rel_err": err}), flush=True)
        del x, r
    del w
    torch.cuda.empty_cache()
