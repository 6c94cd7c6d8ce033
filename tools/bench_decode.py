"""Serving decode throughput: prefill a prompt, then time N decoded
tokens through the hipGraph-captured token step — single stream by
default, `--batch N` for the batched graphed step, `--quantization
int8|int4` for the weight-streaming quantized path (ops.qlinear).
`--quantization all` runs bf16, int8 and int4 in one process,
alternating the arms, and reports peak allocated memory per arm.

Run on the GPU box: python tools/bench_decode.py [--no-graph]
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM  # noqa: E402
from datatunerx_amd.serve.engine import InferenceEngine  # noqa: E402


def build(dev, quantization, graph):
    torch.cuda.reset_peak_memory_stats()
    model = LlamaForCausalLM(LlamaConfig.llama2_7b(), lora=False,
                             dtype=torch.bfloat16)
    model.to(dev)
    model.init_random(seed=0)
    if quantization:
        from datatunerx_amd.models.quant import quantize_model_
        quantize_model_(model, 4 if quantization == "int4" else 8,
                        lora_base=True)
        torch.cuda.empty_cache()
    model.eval()
    return InferenceEngine(model, template="vanilla", device=dev,
                           graph_decode=graph)


def run(eng, tokens, batch):
    """One timed generation; returns decoded tokens per second (all
    rows). Random weights never emit a stop token reliably, so count
    what was actually produced."""
    prompt = list(range(5, 5 + 96))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if batch > 1:
        outs = eng.generate_batch([prompt] * batch, max_new_tokens=tokens)
        n = sum(len(o) for o in outs)
    else:
        n = len(eng.generate(prompt, max_new_tokens=tokens))
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quantization", default=None,
                    choices=("int8", "int4", "all"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    arms = [None, "int8", "int4"] if args.quantization == "all" \
        else [args.quantization]
    engines, mem = {}, {}
    for q in arms:
        # memory of this arm alone: relative to what earlier arms hold
        base = torch.cuda.memory_allocated()
        engines[q] = build(dev, q, not args.no_graph)
        run(engines[q], 8, args.batch)     # warmup (captures the graph)
        mem[q] = (torch.cuda.memory_allocated() - base,
                  torch.cuda.max_memory_allocated() - base)
    rates = {q: [] for q in arms}
    for _ in range(args.reps):
        for q in arms:                     # arms alternate per repetition
            rates[q].append(run(engines[q], args.tokens, args.batch))
    for q in arms:
        tps = statistics.median(r for r, _ in rates[q])
        n = rates[q][0][1]
        print(f"{q or 'bf16'} graph={not args.no_graph} "
              f"batch={args.batch}: {n} tokens, {tps:.1f} tok/s "
              f"(min {min(r for r, _ in rates[q]):.1f}, "
              f"max {max(r for r, _ in rates[q]):.1f}); allocated "
              f"{mem[q][0] / 2**30:.2f} GiB steady, "
              f"{mem[q][1] / 2**30:.2f} GiB peak (build + warmup)",
              flush=True)


if __name__ == "__main__":
    main()
