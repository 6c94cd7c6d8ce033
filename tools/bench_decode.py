"""Serving decode throughput: prefill a prompt, then time N decoded
tokens through the hipGraph-captured token step — single stream by
default, `--batch N` for the batched graphed step, `--quantization
int8|int4` for the weight-streaming quantized path (ops.qlinear).
`--quantization all` runs bf16, int8 and int4 in one process,
alternating the arms, and reports peak allocated memory per arm.

Adapters (r = 8 on q_proj / v_proj, random): `--single-adapter` serves
one the single-adapter way (unmerged LoRA modules); `--adapters N` is
multi-adapter mode with N stacked adapters, row i of the batch using
adapter i mod N; `--compare-adapters` runs single / multi 1 / multi 8 in
one process, alternating, for the chosen --quantization.

Sampling: `--temperature T` (with `--top-p`, `--top-k`) samples every
row instead of taking the argmax; `--mixed` alternates greedy and
sampled rows in one batch (rows 0, 2, ... greedy), which needs an
engine that samples on the device. Seeds are fixed (row i: seed i).

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


def _random_adapter(g, dev, K, N, r=8):
    a = (torch.randn(r, K, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    b = (torch.randn(N, r, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    return a, b


def _attach_random_adapters(model, n, dev):
    """Multi-adapter mode without checkpoint directories: q_proj / v_proj
    of every layer get a stack of n random r = 8 adapters."""
    from datatunerx_amd.models.multilora import (AdapterRegistry,
                                                 MultiLoRALinear)
    g = torch.Generator(device=dev).manual_seed(1)
    for layer in model.layers:
        for name in ("q_proj", "v_proj"):
            base = getattr(layer.self_attn, name)
            mod = MultiLoRALinear(base, n, 8)
            for i in range(n):
                a, b = _random_adapter(g, dev, base.in_features,
                                       base.out_features)
                mod.set_adapter(i, a, b, 4.0)
            setattr(layer.self_attn, name, mod)
    model.adapters = AdapterRegistry([f"a{i}" for i in range(n)],
                                     [8] * n, 8, ("q_proj", "v_proj"))


def build(dev, quantization, graph, adapters=0):
    """adapters: 0 none, -1 one adapter the single-adapter way (LoRA
    modules, unmerged), N > 0 multi-adapter mode with N stacked."""
    torch.cuda.reset_peak_memory_stats()
    model = LlamaForCausalLM(LlamaConfig.llama2_7b(), lora=adapters < 0,
                             dtype=torch.bfloat16)
    model.to(dev)
    model.init_random(seed=0)
    if adapters < 0:
        g = torch.Generator(device=dev).manual_seed(1)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if "lora_B" in n:
                    p.copy_((torch.randn(p.shape, generator=g, device=dev)
                             * 0.02).to(p.dtype))
    elif adapters > 0:
        _attach_random_adapters(model, adapters, dev)
    if quantization:
        from datatunerx_amd.models.quant import quantize_model_
        quantize_model_(model, 4 if quantization == "int4" else 8,
                        lora_base=True)
        torch.cuda.empty_cache()
    model.eval()
    return InferenceEngine(model, template="vanilla", device=dev,
                           graph_decode=graph)


def sampling_kwargs(args, batch):
    """generate / generate_batch keywords for the sampling flags ({}:
    greedy, the calls as they always were)."""
    if not args.temperature > 0:
        return {}
    if batch == 1:
        return {"temperature": args.temperature, "top_p": args.top_p,
                "top_k": args.top_k, "seed": 0}
    temps = [0.0 if args.mixed and i % 2 == 0 else args.temperature
             for i in range(batch)]
    return {"temperature": temps, "top_p": args.top_p,
            "top_k": args.top_k, "seed": list(range(batch))}


def run(eng, tokens, batch, skw=None):
    """One timed generation; returns decoded tokens per second (all
    rows). Random weights never emit a stop token reliably, so count
    what was actually produced. skw: sampling_kwargs()."""
    skw = skw or {}
    prompt = list(range(5, 5 + 96))
    reg = getattr(eng.model, "adapters", None)
    names = ([reg.names[i % len(reg)] for i in range(batch)]
             if reg is not None else None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if batch > 1:
        kw = dict(skw, **({"adapters": names} if names else {}))
        outs = eng.generate_batch([prompt] * batch, max_new_tokens=tokens,
                                  **kw)
        n = sum(len(o) for o in outs)
    else:
        kw = dict(skw, **({"adapter": names[0]} if names else {}))
        n = len(eng.generate(prompt, max_new_tokens=tokens, **kw))
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
    ap.add_argument("--adapters", type=int, default=0,
                    help="multi-adapter mode with N random adapters; row i "
                         "of the batch uses adapter i mod N")
    ap.add_argument("--single-adapter", action="store_true",
                    help="one adapter served the single-adapter way")
    ap.add_argument("--compare-adapters", action="store_true",
                    help="single adapter / multi 1 / multi 8, interleaved")
    ap.add_argument("--temperature", type=float, default=0.0,
                    help="sample every row at this temperature (0: greedy)")
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--mixed", action="store_true",
                    help="rows alternate greedy and sampled (needs "
                         "--temperature and --batch > 1)")
    args = ap.parse_args()
    if args.mixed and not (args.temperature > 0 and args.batch > 1):
        ap.error("--mixed needs --temperature > 0 and --batch > 1")
    skw = sampling_kwargs(args, args.batch)
    dev = torch.device("cuda")
    if args.compare_adapters:
        compare_adapters(args, dev)
        return
    arms = [None, "int8", "int4"] if args.quantization == "all" \
        else [args.quantization]
    adapters = -1 if args.single_adapter else args.adapters
    if adapters:
        print(f"adapters: {'single' if adapters < 0 else adapters}",
              flush=True)
    engines, mem = {}, {}
    for q in arms:
        # memory of this arm alone: relative to what earlier arms hold
        base = torch.cuda.memory_allocated()
        engines[q] = build(dev, q, not args.no_graph, adapters)
        run(engines[q], 8, args.batch, skw)    # warmup (captures the graph)
        mem[q] = (torch.cuda.memory_allocated() - base,
                  torch.cuda.max_memory_allocated() - base)
    rates = {q: [] for q in arms}
    for _ in range(args.reps):
        for q in arms:                     # arms alternate per repetition
            rates[q].append(run(engines[q], args.tokens, args.batch, skw))
    for q in arms:
        tps = statistics.median(r for r, _ in rates[q])
        n = rates[q][0][1]
        mode = ("mixed " if args.mixed else "sampled ") if skw else ""
        print(f"{q or 'bf16'} graph={not args.no_graph} "
              f"{mode}batch={args.batch}: {n} tokens, {tps:.1f} tok/s "
              f"(min {min(r for r, _ in rates[q]):.1f}, "
              f"max {max(r for r, _ in rates[q]):.1f}); allocated "
              f"{mem[q][0] / 2**30:.2f} GiB steady, "
              f"{mem[q][1] / 2**30:.2f} GiB peak (build + warmup)",
              flush=True)


def compare_adapters(args, dev):
    """(a) one adapter as LoRA modules, (b) multi mode with 1 adapter,
    (c) multi mode with 8 distinct adapters — same base, same process,
    arms alternating per repetition."""
    q = None if args.quantization in (None, "all") else args.quantization
    arms = {"single adapter (LoRA modules)": -1, "multi, 1 adapter": 1,
            "multi, 8 adapters": 8}
    engines, mem = {}, {}
    for name, n in arms.items():
        base = torch.cuda.memory_allocated()
        engines[name] = build(dev, q, not args.no_graph, n)
        run(engines[name], 8, args.batch)          # warmup + capture
        mem[name] = torch.cuda.memory_allocated() - base
    rates = {name: [] for name in arms}
    for _ in range(args.reps):
        for name in arms:
            rates[name].append(run(engines[name], args.tokens,
                                   args.batch)[0])
    ref = statistics.median(rates["single adapter (LoRA modules)"])
    for name in arms:
        tps = statistics.median(rates[name])
        print(f"{q or 'bf16'} batch={args.batch} {name}: {tps:.1f} tok/s "
              f"(min {min(rates[name]):.1f}, max {max(rates[name]):.1f}), "
              f"{tps / ref:.3f}x single; engine "
              f"{mem[name] / 2**30:.2f} GiB", flush=True)


if __name__ == "__main__":
    main()
