"""Decode attention over the bf16 KV cache: the per-query-head kernel
(_EXT.attn_decode) against the GQA-shared one (_EXT.attn_decode_gqa), timed
interleaved in one process.

  python tools/bench_gqa_decode.py [--out TABLE.md]

Per cell (G, capacity, B, live length): ROUNDS rounds, each timing CALLS
calls of the old kernel and then CALLS calls of the new one between device
events. The calls of a round walk a ring of caches of at least 512 MiB in
all, so no call finds its rows in L2 or the Infinity Cache from the call
before (a model's layers each have their own cache). Reported: the median
round of each kernel in microseconds a call, new / old, and the spread
(max - min) / median of each kernel's rounds; a difference inside the
spread is no difference. GB/s counts the live K and V rows once per kv
head: what the shared kernel has to read.

Needs a GPU: it measures and has no CPU path.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datatunerx_amd import ops  # noqa: E402

GROUPS = [(32, 8), (28, 4), (32, 4)]         # G = 4 (llama3), 7 (qwen2), 8
CAPS = [2048, 8192, 32768]
BATCHES = [1, 8, 16]
D = 128
ROUNDS, CALLS, RING_BYTES = 7, 20, 512 << 20


def time_calls(fn, ring, lens, scale):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for i in range(CALLS):
        q, k, v = ring[i % len(ring)]
        fn(q, k, v, scale, lens)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def cell(Hq, Hkv, cap, B, live, dev):
    g = torch.Generator(device=dev).manual_seed(cap + B + Hq)
    kv_bytes = 2 * B * cap * Hkv * D * 2
    ring = []
    for _ in range(max(2, min(64, -(-RING_BYTES // kv_bytes)))):
        mk = lambda *s: (torch.randn(*s, generator=g, device=dev) * 0.5).to(
            torch.bfloat16)
        ring.append((mk(B, 1, Hq, D), mk(B, cap, Hkv, D), mk(B, cap, Hkv, D)))
    lens = torch.full((B,), live, dtype=torch.int32, device=dev)
    scale = D ** -0.5
    fns = {"old": ops._EXT.attn_decode, "new": ops._EXT.attn_decode_gqa}
    q, k, v = ring[0]
    o_old, o_new = (fns[n](q, k, v, scale, lens)[0].float() for n in fns)
    err = float((o_old - o_new).abs().max())
    for fn in fns.values():                  # warm-up over the whole ring
        time_calls(fn, ring, lens, scale)
    t = {n: [] for n in fns}
    for _ in range(ROUNDS):
        for n, fn in fns.items():
            t[n].append(time_calls(fn, ring, lens, scale))
    med = {n: statistics.median(x) for n, x in t.items()}
    spread = {n: (max(x) - min(x)) / med[n] for n, x in t.items()}
    live_bytes = 2 * B * live * Hkv * D * 2
    return {"G": Hq // Hkv, "Hq": Hq, "Hkv": Hkv, "cap": cap, "B": B,
            "live": live, "old_us": med["old"], "new_us": med["new"],
            "ratio": med["new"] / med["old"], "spread_old": spread["old"],
            "spread_new": spread["new"],
            "new_gbps": live_bytes / med["new"] / 1e3, "max_abs_diff": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None,
                    help="also write the table as markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.have_ext():
        sys.exit("bench_gqa_decode: needs a GPU and the HIP extension")
    dev = torch.device("cuda", 0)
    rows = []
    for Hq, Hkv in GROUPS:
        for cap in CAPS:
            for B in BATCHES:
                for live in (cap, cap // 8):
                    r = cell(Hq, Hkv, cap, B, live, dev)
                    rows.append(r)
                    print(json.dumps(r), flush=True)
    if args.out is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("| G (Hq/Hkv) | capacity | B | live | old us | new us | "
                "new/old | spread old / new | new GB/s |\n"
                "|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['G']} ({r['Hq']}/{r['Hkv']}) | {r['cap']} | "
                    f"{r['B']} | {r['live']} | {r['old_us']:.1f} | "
                    f"{r['new_us']:.1f} | {r['ratio']:.2f} | "
                    f"{r['spread_old']:.2f} / {r['spread_new']:.2f} | "
                    f"{r['new_gbps']:.0f} |\n")


if __name__ == "__main__":
    main()
