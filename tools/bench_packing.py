#!/usr/bin/env python3
"""Padded against packed training throughput, in real (non-pad) tokens/s.

Trains Llama-2-7B LoRA for a few optimizer steps on a seeded synthetic
instruction set whose lengths are uniform in 16..512 (block_size 1024),
once with the default collator (each micro-batch right-padded to its
longest example) and once with --packing (whole examples bin-packed into
rows of block_size, attention masked by document). Both runs see the same
examples; the figure of merit is the number of real tokens consumed per
second of timed steps, since pad positions are work nobody asked for.

  python tools/bench_packing.py --steps 40 --warmup 4 --examples 2048
      # a timed window of several seconds per mode (profiles/README.md)
  python tools/bench_packing.py --model llama-mini --steps 2 --warmup 1
      # plumbing check at a toy size (measures overheads only)

The token accounting alone predicts fill_packed / fill_padded; the script
prints both fills next to the measured ratio.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datatunerx_amd.data.dataset import SFTDataset  # noqa: E402
from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM  # noqa: E402
from datatunerx_amd.train.trainer import SFTTrainer, TrainerConfig  # noqa: E402


def synthetic(n, lo, hi, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    ex = []
    for L in torch.randint(lo, hi + 1, (n,), generator=g).tolist():
        ids = torch.randint(3, vocab, (L,), generator=g)
        labels = ids.clone()
        labels[:max(1, L // 4)] = -100          # prompt part
        ex.append({"input_ids": ids.tolist(), "labels": labels.tolist()})
    return SFTDataset(ex)


def run(name, packing, ds, args, device):
    cfg = (LlamaConfig.llama2_7b() if name == "llama2-7b"
           else LlamaConfig.mini(max_position_embeddings=args.block_size))
    with torch.device(device):
        model = LlamaForCausalLM(cfg, lora=True, dtype=torch.bfloat16)
    model.init_random(seed=1234)
    tcfg = TrainerConfig(output_dir=args.out, micro_batch_size=args.batch,
                         max_steps=args.steps + args.warmup,
                         logging_steps=0, packing=packing,
                         cutoff_len=args.block_size)
    tr = SFTTrainer(model, ds, tcfg, device=device)
    model.train()
    it = iter(tr.train_loader)
    real = computed = 0
    t0 = 0.0
    for step in range(args.steps + args.warmup):
        if step == args.warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        mb = next(it)
        if step >= args.warmup:
            computed += mb["input_ids"].numel()
            # synthetic ids start at 3; 0 is the pad id in both collators
            real += int((mb["input_ids"] != 0).sum())
        tr.train_step([mb])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del tr, model
    torch.cuda.empty_cache()
    return {"mode": "packed" if packing else "padded",
            "real_tokens": real, "computed_tokens": computed,
            "fill": round(real / computed, 4), "seconds": round(dt, 3),
            "real_tokens_per_s": round(real / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2-7b",
                    choices=["llama2-7b", "llama-mini"])
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--block_size", type=int, default=1024)
    ap.add_argument("--examples", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="output/bench_packing")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_packing needs a GPU"
    device = torch.device("cuda:0")
    vocab = 32000 if args.model == "llama2-7b" else 512
    ds = synthetic(args.examples, 16, 512, vocab, args.seed)
    res = [run(args.model, p, ds, args, device) for p in (False, True)]
    for r in res:
        print(json.dumps(r))
    pad, pk = res
    print(json.dumps({
        "speedup_real_tokens_per_s":
            round(pk["real_tokens_per_s"] / pad["real_tokens_per_s"], 3),
        "predicted_by_fill": round(pk["fill"] / pad["fill"], 3)}))


if __name__ == "__main__":
    main()
