#!/usr/bin/env python3
"""Attention kernel microbench on the training shape.

Reports ms + effective TF/s per kernel (causal ~halves the useful
flops; we count the causal flops actually computed: full tiles below
the diagonal + masked diagonal tiles).

  python tools/bench_attn.py --batch 64        # the bench.py shape
  python tools/bench_attn.py --batch 4 --seq 4096 --docs 8
      # sequence packing: 8 equal documents per row through the
      # document-masked kernels, next to plain causal at the same S

For per-kernel times run it under the profiler, in a run of its own:
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_attn.py --batch 64
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datatunerx_amd import ops
from datatunerx_amd.ops import _dtx_hip

assert torch.cuda.is_available()
dev = torch.device("cuda:0")
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16,
                help="batch size (bench.py's Llama-2-7B shape is 64)")
ap.add_argument("--seq", type=int, default=1024, help="row length S")
ap.add_argument("--docs", type=int, default=0,
                help="N > 0: also time the document-masked kernels with "
                     "N equal documents per row (S %% N == 0)")
args = ap.parse_args()
B, H, S, D = args.batch, 32, args.seq, 128
scale = D ** -0.5

q = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
k = torch.randn_like(q)
v = torch.randn_like(q)
do = torch.randn_like(q)


def bench(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


# causal: ~1/2 the S^2 work
fwd_fl = 4 * B * H * S * S * D * 0.5
bwd_dkdv_fl = fwd_fl / 2 * 4          # useful matmuls: S, dP, dV, dK
bwd_dq_fl = fwd_fl / 2 * 3

t = bench(lambda: ops.attn_fwd(q, k, v, True, scale))
print(f"attn_fwd (incl V-transpose): {t*1e3:7.3f} ms  {fwd_fl/t/1e12:6.0f} TF/s")

t = bench(lambda: _dtx_hip.attn_fwd(q, k, v, True, scale))
print(f"attn_fwd (kernel only):      {t*1e3:7.3f} ms  {fwd_fl/t/1e12:6.0f} TF/s")

o, lse = ops.attn_fwd(q, k, v, True, scale)
t = bench(lambda: _dtx_hip.attn_bwd(q, k, v, o, do, lse, True, scale))
print(f"attn_bwd (all):              {t*1e3:7.3f} ms  {(bwd_dkdv_fl+bwd_dq_fl)/t/1e12:6.0f} TF/s")

t = bench(lambda: _dtx_hip.transpose_sd(q))
gb = q.numel() * 2 * 2 / 1e9
print(f"transpose_sd:                {t*1e3:7.3f} ms  {gb/t/1e3:6.2f} TB/s")

if args.docs > 0:
    N = args.docs
    assert S % N == 0, "--docs must divide --seq"
    L = S // N
    ds = (torch.arange(S, device=dev, dtype=torch.int32) // L * L)
    ds = ds.expand(B, S).contiguous()
    de = ops.doc_end_from_start(ds)
    # N causal triangles of side L instead of one of side S
    frac = 1.0 / N
    t_f0 = bench(lambda: _dtx_hip.attn_fwd(q, k, v, True, scale))
    t_b0 = bench(lambda: _dtx_hip.attn_bwd(q, k, v, o, do, lse, True, scale))
    t_f = bench(lambda: _dtx_hip.attn_fwd(q, k, v, True, scale, ds))
    od, lsed = _dtx_hip.attn_fwd(q, k, v, True, scale, ds)
    t_b = bench(lambda: _dtx_hip.attn_bwd(q, k, v, od, do, lsed, True,
                                          scale, ds, de))
    print(f"--- {N} documents of {L} per row (useful flops x{frac:.3f})")
    print(f"attn_fwd docs (kernel only): {t_f*1e3:7.3f} ms  "
          f"{fwd_fl*frac/t_f/1e12:6.0f} TF/s  "
          f"plain causal {t_f0*1e3:7.3f} ms  ratio {t_f0/t_f:5.2f}x")
    print(f"attn_bwd docs (all):         {t_b*1e3:7.3f} ms  "
          f"{(bwd_dkdv_fl+bwd_dq_fl)*frac/t_b/1e12:6.0f} TF/s  "
          f"plain causal {t_b0*1e3:7.3f} ms  ratio {t_b0/t_b:5.2f}x")
