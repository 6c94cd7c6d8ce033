"""Multi-adapter serving: one base model, a stack of LoRA adapters, and
the adapter chosen per request (per row of a decode batch).

`MultiLoRALinear` wraps a frozen projection (bf16 `FrozenLinear`, or a
`QuantFrozenLinear` after quantization) and holds every adapter's A / B
for that projection in one stack, zero-padded to a common rank. A decode
step ([B,1,K], B <= 16) adds the low-rank term with the gathered kernel
(ops.mlora_add): the adapter index of each row is read on the device, so
one captured decode graph serves every assignment of adapters. Prefill
and CPU calls run the existing lora_contract / lora_expand_add ops once
per sequence on that adapter's slice of the stack.

Which adapter a row uses travels WITH the call (`adapters=` down from the
engine): engines on separate streams share one model, so there is no
model-global "current adapter".
"""

from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from .. import ops
from .lora import FrozenLinear

MAX_RANK = ops.MLORA_RANKS[-1]


class AdapterSelection:
    """Adapter index per sequence of one model call: `dev` is an int32
    [B] tensor on the model's device (what the decode kernel reads),
    `host` the same indices as a tuple (what the eager prefill path
    branches on; None for a graph's static buffer, whose content only
    the device knows). -1 selects the base model."""

    __slots__ = ("dev", "host")

    def __init__(self, dev: torch.Tensor, host: Optional[Sequence[int]]):
        self.dev = dev
        self.host = None if host is None else tuple(int(i) for i in host)


class AdapterRegistry:
    """name -> index of the stacks built by attach_adapters_."""

    def __init__(self, names: Sequence[str], ranks: Sequence[int],
                 rank: int, targets: Sequence[str]):
        self.names = tuple(names)
        self.ranks = tuple(ranks)           # each adapter's own r
        self.rank = rank                    # the stacks' padded R
        self.targets = tuple(targets)       # union of target modules
        self._index = {n: i for i, n in enumerate(self.names)}

    def __len__(self):
        return len(self.names)

    def __contains__(self, name):
        return name in self._index

    def as_dict(self) -> Dict[str, int]:
        return dict(self._index)

    def index(self, name: Optional[str]) -> int:
        """None -> -1 (base model); unknown names raise ValueError."""
        if name is None:
            return -1
        try:
            return self._index[name]
        except (KeyError, TypeError):
            raise ValueError(
                f"unknown adapter {name!r} (loaded: "
                f"{', '.join(self.names) or 'none'})") from None

    def select(self, names: Sequence[Optional[str]], device,
               pad_to: int = 0) -> AdapterSelection:
        """Selection for a batch; rows past len(names) up to pad_to get
        -1 (dummy padding rows of a fixed-size graphed batch)."""
        idx = [self.index(n) for n in names]
        idx += [-1] * (pad_to - len(idx))
        return AdapterSelection(
            torch.tensor(idx, dtype=torch.int32, device=device), idx)


class MultiLoRALinear(nn.Module):
    """Inference-only projection with a stack of G unmerged adapters:
    y[b] = base(x[b]) + scale[g] * (x[b] @ A[g]^T) @ Bt[g], g = the
    adapter of sequence b (none for g < 0). Buffers: A [G,R,K],
    Bt [G,R,N] (lora_B pre-transposed), scale [G] f32; an adapter that
    does not target this projection has zero A/Bt and scale 0. `base`
    is a child module so quantize_model_ converts it in place."""

    def __init__(self, base: nn.Module, n_adapters: int, rank: int):
        super().__init__()
        if rank not in ops.MLORA_RANKS:
            raise ValueError(f"stack rank must be one of {ops.MLORA_RANKS}, "
                             f"got {rank}")
        self.base = base
        self.in_features = base.in_features
        self.out_features = base.out_features
        self.rank = rank
        w = base.weight
        kw = dict(device=w.device, dtype=w.dtype)
        self.register_buffer(
            "A", torch.zeros(n_adapters, rank, self.in_features, **kw))
        self.register_buffer(
            "Bt", torch.zeros(n_adapters, rank, self.out_features, **kw))
        self.register_buffer(
            "scale", torch.zeros(n_adapters, dtype=torch.float32,
                                 device=w.device))
        # host copy of "adapter g targets this projection" (prefill
        # skips the others without a device read)
        self.targeted = [False] * n_adapters
        self.scales_host = [0.0] * n_adapters

    @torch.no_grad()
    def set_adapter(self, g: int, lora_A: torch.Tensor,
                    lora_B: torch.Tensor, scale: float):
        """lora_A [r,K], lora_B [N,r] (PEFT layouts), r <= the stack's
        rank; the remaining ranks stay zero."""
        r = lora_A.shape[0]
        if tuple(lora_A.shape) != (r, self.in_features) or \
                tuple(lora_B.shape) != (self.out_features, r):
            raise ValueError(
                f"adapter tensors {tuple(lora_A.shape)} / "
                f"{tuple(lora_B.shape)} do not fit a projection "
                f"{self.in_features} -> {self.out_features}")
        if r > self.rank:
            raise ValueError(f"adapter rank {r} above the stack's "
                             f"{self.rank}")
        self.A[g].zero_()
        self.Bt[g].zero_()
        self.A[g, :r].copy_(lora_A.to(self.A.dtype))
        self.Bt[g, :r].copy_(lora_B.t().to(self.Bt.dtype))
        self.scale[g] = float(scale)
        self.scales_host[g] = float(scale)
        self.targeted[g] = True

    # Rounding order. A sequence that uses an adapter here is computed as
    # the single-adapter modules compute it (LoRALinearModule,
    # QuantLoRALinear): y = bf16(base(x)), the low-rank update rounds y
    # once more, and the residual is added after the update. A sequence
    # without one is computed as the bare base module computes it, which
    # for a FrozenLinear folds the residual into the GEMM epilogue. So
    # serving an adapter from a stack gives what serving it alone gives,
    # rounding step for rounding step — "batched == per request" stays
    # meaningful. Prefill picks the order per sequence; a decode step is
    # one batched call and uses the adapter order for every row (for a
    # row without adapter that is the order of the single-row GEMV path:
    # y, then + residual).

    def _base(self, x, residual=None):
        """base(x) (+ residual) exactly as the bare base module does it."""
        if residual is not None and isinstance(self.base, FrozenLinear):
            return self.base(x, residual)      # residual in GEMM epilogue
        y = self.base(x)
        return y if residual is None else y + residual

    def _decode_path(self, x, adapters) -> bool:
        if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3
                and x.shape[1] == 1 and self.A.dtype == torch.bfloat16
                and adapters.dev.is_cuda
                and adapters.dev.numel() == x.shape[0]):
            return False
        return ops.mlora_supported(x.shape[0], self.out_features,
                                   self.in_features, self.rank)

    def forward(self, x, adapters: Optional[AdapterSelection] = None,
                residual=None):
        if adapters is None:
            return self._base(x, residual)
        if self._decode_path(x, adapters):
            B = x.shape[0]
            y = self.base(x).contiguous()
            ops.mlora_add(y.view(B, self.out_features),
                          x.contiguous().view(B, self.in_features),
                          self.A, self.Bt, self.scale, adapters.dev)
            return y if residual is None else y + residual
        return self._per_sequence(x, adapters, residual)

    def _update_sequence(self, yb, xb, g):
        """yb [S,N] += scale[g] * (xb [S,K] @ A[g]^T) @ Bt[g], in place,
        with the single-adapter LoRA ops; a matmul only for GPU shapes
        those kernels do not take (not bf16, K or N not in whole 16-byte
        pieces)."""
        K, N = self.in_features, self.out_features
        if (not xb.is_cuda) or (
                xb.dtype == torch.bfloat16 and self.A.dtype == torch.bfloat16
                and K % 8 == 0 and N % 8 == 0):
            if xb.is_cuda:
                xb = xb.contiguous()
            t = ops.lora_contract(xb, self.A[g])
            ops.lora_expand_add_t(yb, t, self.Bt[g], self.scales_host[g])
        else:
            d = (xb.float() @ self.A[g].float().t()) @ self.Bt[g].float()
            yb.add_((self.scales_host[g] * d).to(yb.dtype))

    def _per_sequence(self, x, adapters, residual):
        """Prefill / CPU / shapes outside the decode contract: the
        single-adapter LoRA ops once per sequence, on host indices."""
        if adapters.host is None:
            raise ValueError(
                "MultiLoRALinear: this call is outside the decode kernel's "
                "contract and needs host-side adapter indices")
        idx = adapters.host
        if x.dim() < 2 or len(idx) != x.shape[0]:
            raise ValueError(
                f"adapter selection of {len(idx)} rows for input "
                f"{tuple(x.shape)}")
        K, N = self.in_features, self.out_features
        live = [b for b, g in enumerate(idx)
                if 0 <= g < len(self.targeted) and self.targeted[g]]
        if not live:
            return self._base(x, residual)
        if residual is None or len(live) == len(idx):
            y = self.base(x).contiguous()
            for b in live:
                self._update_sequence(y[b].view(-1, N),
                                      x[b].reshape(-1, K), idx[b])
            return y if residual is None else y + residual
        # mixed, with a residual: the sequences without an adapter keep
        # the base module's fused result, the others are redone in the
        # adapter order
        y = self._base(x, residual).contiguous()
        for b in live:
            yb = self.base(x[b:b + 1]).contiguous()
            self._update_sequence(yb[0].view(-1, N), x[b].reshape(-1, K),
                                  idx[b])
            y[b] = (yb + residual[b:b + 1])[0]
        return y


def _read_adapter(adapter_dir: str, prefix: str):
    """(r, alpha, targets, {module: {"A": t, "B": t}}) of a PEFT adapter
    directory (the layout save_adapter writes and load_adapter reads)."""
    from safetensors.torch import load_file
    with open(os.path.join(adapter_dir, "adapter_config.json")) as f:
        ac = json.load(f)
    r = int(ac.get("r", 8))
    alpha = float(ac.get("lora_alpha", 32))
    targets = tuple(ac.get("target_modules") or ("q_proj", "v_proj"))
    sd = load_file(os.path.join(adapter_dir, "adapter_model.safetensors"))
    mods: Dict[str, Dict[str, torch.Tensor]] = {}
    for key, tensor in sd.items():
        if not key.startswith(prefix):
            continue
        rest = key[len(prefix):]
        for suffix, slot in ((".lora_A.weight", "A"),
                             (".lora_B.weight", "B")):
            if rest.endswith(suffix):
                mods.setdefault(rest[:-len(suffix)], {})[slot] = tensor
    return r, alpha, targets, mods


def stack_rank(max_r: int) -> int:
    """Smallest rank the gathered kernel takes that holds max_r."""
    for R in ops.MLORA_RANKS:
        if max_r <= R:
            return R
    raise ValueError(f"adapter rank {max_r} is above the supported "
                     f"maximum {MAX_RANK}")


@torch.no_grad()
def attach_adapters_(model: nn.Module, adapters: Dict[str, str],
                     prefix: str = "base_model.model.") -> AdapterRegistry:
    """Load the named PEFT adapter directories into `model` (a
    LlamaForCausalLM built with lora=False): every projection in the
    union of the adapters' target modules becomes a MultiLoRALinear
    holding all of them, ranks zero-padded to a common R. Returns the
    name -> index registry (also set as `model.adapters`)."""
    from .llama import LlamaForCausalLM
    if not isinstance(model, LlamaForCausalLM):
        raise ValueError(
            "multi-adapter serving supports llama models, not "
            f"{type(model).__name__}")
    if not adapters:
        raise ValueError("attach_adapters_: no adapters given")
    # a mapping, or (name, dir) pairs (which can carry a repeated name)
    items = list(adapters.items() if hasattr(adapters, "items")
                 else adapters)
    names: List[str] = []
    for n, _d in items:
        if not isinstance(n, str) or not n.strip():
            raise ValueError(f"empty adapter name {n!r}")
        if n in names:
            raise ValueError(f"duplicate adapter name {n!r}")
        names.append(n)
    adapters = dict(items)
    loaded = [_read_adapter(adapters[n], prefix) for n in names]
    for n, (r, _a, _t, _m) in zip(names, loaded):
        if r < 1 or r > MAX_RANK:
            raise ValueError(f"adapter {n!r}: rank {r} is outside 1.."
                             f"{MAX_RANK}")
    R = stack_rank(max(r for r, _a, _t, _m in loaded))
    union: List[str] = []
    for _r, _a, targets, _m in loaded:
        for t in targets:
            if t not in union:
                union.append(t)
    G = len(names)
    n_loaded = [0] * G
    used = [set() for _ in range(G)]
    for parent_name, parent in list(model.named_modules()):
        if not parent_name.startswith("layers."):
            continue
        for child_name, child in list(parent.named_children()):
            if child_name not in union or not isinstance(child, FrozenLinear):
                continue
            full = f"{parent_name}.{child_name}"
            mod = MultiLoRALinear(child, G, R)
            for g, (r, alpha, targets, mods) in enumerate(loaded):
                ab = mods.get(full)
                if ab is None or child_name not in targets:
                    continue
                if "A" not in ab or "B" not in ab:
                    raise ValueError(
                        f"adapter {names[g]!r}: {full} lacks lora_A or "
                        "lora_B")
                try:
                    mod.set_adapter(g, ab["A"], ab["B"], alpha / r)
                except ValueError as e:
                    raise ValueError(
                        f"adapter {names[g]!r}, {full}: {e}") from None
                n_loaded[g] += 2
                used[g].add(full)
            setattr(parent, child_name, mod)
    for g, (_r, _a, targets, mods) in enumerate(loaded):
        stray = sorted(m for m in mods if m not in used[g]
                       and m.rsplit(".", 1)[-1] in targets)
        if stray:
            raise ValueError(
                f"adapter {names[g]!r} does not fit the model: no frozen "
                f"projection {stray[0]!r}")
    for n, k in zip(names, n_loaded):
        if k == 0:
            raise ValueError(
                f"adapter {n!r} ({adapters[n]}) loaded no tensors into "
                "this model")
    reg = AdapterRegistry(names, [r for r, _a, _t, _m in loaded], R, union)
    model.adapters = reg
    return reg
