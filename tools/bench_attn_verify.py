"""Verify attention (ops.attn_verify, T query rows over the bf16 KV cache)
against what a T-token step had before it: T calls of the routed
single-token decode kernel (ops.attn_fwd, S = 1) and the prefill kernel on
the same shape (_EXT.attn_fwd over the live prefix), timed interleaved in
one process.

  python tools/bench_attn_verify.py [--out TABLE.md]

B = 1, D = 128, capacity 8192. Per cell (heads, live length, T): ROUNDS
rounds, each timing CALLS calls of every path between device events. The
calls of a round walk a ring of caches of at least 512 MiB in all, so no
call finds its rows in L2 or the Infinity Cache from the call before (a
model's layers each have their own cache). Reported: the median round of
each path in microseconds a T-token step, and the spread (max - min) /
median of the verify kernel's rounds.

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

HEADS = [(32, 8), (32, 32)]
LIVES = [512, 2048, 8192]
TS = [2, 4, 8]
D, CAP = 128, 8192
ROUNDS, CALLS, RING_BYTES = 7, 20, 512 << 20


def time_calls(fn, ring):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for i in range(CALLS):
        fn(*ring[i % len(ring)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def cell(Hq, Hkv, live, T, dev):
    g = torch.Generator(device=dev).manual_seed(live + T + Hq)
    mk = lambda *s: (torch.randn(*s, generator=g, device=dev) * 0.5).to(
        torch.bfloat16)
    n_ring = max(2, min(64, -(-RING_BYTES // (2 * CAP * Hkv * D * 2))))
    ring = [(mk(1, T, Hq, D), mk(1, CAP, Hkv, D), mk(1, CAP, Hkv, D))
            for _ in range(n_ring)]
    scale = D ** -0.5
    len_t = torch.tensor([live], dtype=torch.int32, device=dev)
    lens1 = [torch.tensor([live - T + t + 1], dtype=torch.int32, device=dev)
             for t in range(T)]

    def verify(q, k, v):
        return ops.attn_verify(q, k, v, scale, len_t)

    def singles(q, k, v):
        return [ops.attn_fwd(q[:, t:t + 1], k, v, True, scale, lens1[t])
                for t in range(T)]

    def prefill(q, k, v):
        return ops._EXT.attn_fwd(q, k[:, :live], v[:, :live], True, scale)

    fns = {"verify": verify, "singles": singles, "prefill": prefill}
    o = verify(*ring[0])[0].float()
    o1 = torch.cat([x[0] for x in singles(*ring[0])], 1).float()
    err = float((o - o1).abs().max())
    for fn in fns.values():                  # warm-up over the whole ring
        time_calls(fn, ring)
    t = {n: [] for n in fns}
    for _ in range(ROUNDS):
        for n, fn in fns.items():
            t[n].append(time_calls(fn, ring))
    med = {n: statistics.median(x) for n, x in t.items()}
    return {"Hq": Hq, "Hkv": Hkv, "live": live, "T": T,
            "verify_us": med["verify"], "singles_us": med["singles"],
            "prefill_us": med["prefill"],
            "spread_verify": (max(t["verify"]) - min(t["verify"])) /
            med["verify"], "max_abs_diff_vs_singles": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None,
                    help="also write the table as markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.have_ext():
        sys.exit("bench_attn_verify: needs a GPU and the HIP extension")
    dev = torch.device("cuda", 0)
    rows = []
    for Hq, Hkv in HEADS:
        for live in LIVES:
            for T in TS:
                if not ops.attn_verify_supported(T, Hq, Hkv, D):
                    continue
                rows.append(cell(Hq, Hkv, live, T, dev))
                print(json.dumps(rows[-1]), flush=True)
    if args.out is None:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("| Hq/Hkv | live | T | verify us | T singles us | prefill "
                "kernel us | verify / singles | spread verify |\n"
                "|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['Hq']}/{r['Hkv']} | {r['live']} | {r['T']} | "
                    f"{r['verify_us']:.1f} | {r['singles_us']:.1f} | "
                    f"{r['prefill_us']:.1f} | "
                    f"{r['verify_us'] / r['singles_us']:.2f} | "
                    f"{r['spread_verify']:.2f} |\n")


if __name__ == "__main__":
    main()
