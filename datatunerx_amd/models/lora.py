"""LoRA modules + HF-PEFT-compatible adapter checkpoint layout.

Adapter layout contract (what the reference produces via PEFT
`trainer.save_model` — cmd/tuning/train.py:300, SURVEY.md §5
Checkpoint/resume): a directory with `adapter_config.json` and
`adapter_model.safetensors` whose keys are
`base_model.model.<module_path>.lora_A.weight` ([r, in]) and
`...lora_B.weight` ([out, r]) — the exact names/shapes PEFT writes
(layout-verified by tests; peft itself is not in this offline image).
"""

from __future__ import annotations

import json
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import (SKINNY_MAX_ROWS, gemm_fp8_supported, gemm_nt_supported,
                   quant_fp8_rows, skinny_decode_rows, skinny_linear)
from ..ops.autograd import FrozenGemm
from ..ops.autograd import LoRALinear as _FusedLoRAFn


def dgrad_wt_pays(n: int, k: int) -> bool:
    """Shape families [n,k] of frozen weights whose dgrad is faster
    against a cached W^T (F.linear(dy, W^T), the library's forward
    layout) than as dy @ W. A family that does not clear the probe's
    spread (tools/bench_basegemm.py, recorded in profiles/README.md)
    is refused here and builds no copy."""
    return True


_TENSOR_DATA = torch.Tensor.data


class _DataTrackedParameter(nn.Parameter):
    """A frozen weight whose W^T is cached. torch gives `weight.data` a
    version counter of its own, so `weight.data.mul_(2)` or
    `weight.data.copy_(...)` leave `weight._version` where it was; this
    class counts every use of `.data` instead, and the count is part of
    the cache key. A use that only reads costs one rebuild of the copy,
    never a stale one. _weight_t gives a plain nn.Parameter this class
    when it first caches its transpose; nothing else about the
    parameter changes (same storage, same flags, still an
    nn.Parameter)."""

    @property
    def data(self):
        self.__dict__["_data_uses"] = self.__dict__.get("_data_uses", 0) + 1
        return _TENSOR_DATA.__get__(self)

    @data.setter
    def data(self, value):
        self.__dict__["_data_uses"] = self.__dict__.get("_data_uses", 0) + 1
        _TENSOR_DATA.__set__(self, value)


def _weight_t(mod: nn.Module, any_device: bool = False):
    """Cached W^T [K,N] of a frozen base weight [N,K], or None. With it
    the dgrad dx = dy @ W runs as F.linear(dy, W^T): the library's
    forward layout, both operands contraction-contiguous, which it runs
    faster than the "NN" form of dy @ W. Frozen weights never change and
    288 GB of HBM3E make the persistent duplicate cheap (one extra bf16
    copy of the frozen projections and the lm_head).

    Built only for a CUDA bf16 weight with requires_grad == False, with
    grad mode on and DTX_DGRAD_WT != 0: serving and eval (no_grad) and
    full-parameter training never build it. The cache is a plain
    attribute (no parameter, no buffer: absent from state_dict() and
    adapter checkpoints) keyed on the weight's data_ptr(), its _version
    and its count of `.data` uses (_DataTrackedParameter), so
    init_random, a checkpoint load, .to() or any in-place write, through
    `weight.data` too, rebuilds it. any_device lifts the CUDA/bf16
    condition (tests)."""
    w = mod.weight
    if (w.requires_grad or not torch.is_grad_enabled()
            or os.environ.get("DTX_DGRAD_WT", "1") == "0"):
        return None
    if not any_device and not (w.is_cuda and w.dtype == torch.bfloat16):
        return None
    if not dgrad_wt_pays(*w.shape):
        return None
    return _cached(mod, "_wt", lambda: w.detach().t().contiguous())


def _cached(mod: nn.Module, slot: str, build):
    """mod.__dict__[slot] = (key, build()), rebuilt when the weight's
    data_ptr(), _version or count of `.data` uses changed."""
    w = mod.weight
    if type(w) is nn.Parameter:
        w.__class__ = _DataTrackedParameter
    key = (w.data_ptr(), w._version, w.__dict__.get("_data_uses", 0))
    cached = mod.__dict__.get(slot)
    if cached is None or cached[0] != key:
        cached = (key, build())
        mod.__dict__[slot] = cached
    return cached[1]


BASE_GEMM_MODES = ("bf16", "fp8")
FP8_MAX_FEATURES = 16384     # quant_fp8_rows holds a row in registers


def set_base_gemm(model: nn.Module, mode: str) -> None:
    """Choose how the frozen base projections of `model` multiply: "bf16"
    (default) or "fp8" (ops/hip/gemm_fp8.hip). The lm_head keeps bf16:
    logits are not computed in fp8."""
    if mode not in BASE_GEMM_MODES:
        raise ValueError(f"base_gemm must be one of {BASE_GEMM_MODES}, "
                         f"got {mode!r}")
    for name, mod in model.named_modules():
        if isinstance(mod, (FrozenLinear, LoRALinearModule)):
            head = "lm_head" in name.split(".")
            mod.base_gemm = "bf16" if head else mode


def _weight_fp8(mod: nn.Module, x):
    """The fp8 route of one module for the activation x, or None: the
    cached (w8, sw, wt8, swt) = quant_fp8_rows(W), quant_fp8_rows(W^T) of
    its frozen weight. THE routing predicate of the fp8 base GEMMs: mode
    fp8 on this module (set_base_gemm; never the lm_head), a frozen bf16
    weight, more than 16 activation rows (the decode kernels keep theirs),
    both dimensions within the quantizer's row limit and, on the GPU,
    [N,K] and [K,N] inside the kernel's support. The cache lives beside
    _wt under the same rules (keyed like it, no parameter, no buffer,
    dropped by __getstate__); a routed module builds no bf16 W^T."""
    w = mod.weight
    n, k = w.shape
    if (getattr(mod, "base_gemm", "bf16") != "fp8" or w.requires_grad
            or w.dtype != torch.bfloat16 or x.dtype != torch.bfloat16
            or x.numel() // x.shape[-1] <= SKINNY_MAX_ROWS
            or max(n, k) > FP8_MAX_FEATURES or n % 8 or k % 8):
        return None
    if w.is_cuda and not (gemm_fp8_supported(n, k)
                          and gemm_fp8_supported(k, n)):
        return None
    return _cached(mod, "_w8", lambda: (
        *quant_fp8_rows(w.detach()),
        *quant_fp8_rows(w.detach().t().contiguous())))


def base_operands(mod: nn.Module, x):
    """(wt, f8) for the autograd nodes: the fp8 operands when the module
    routes there (and then no W^T), else the cached bf16 W^T or None."""
    f8 = _weight_fp8(mod, x)
    return (None, f8) if f8 is not None else (_weight_t(mod), None)


def _state_without_wt(self):
    """__getstate__ of the modules _weight_t caches on: copy.deepcopy and
    whole-module pickling take the module without its cached W^T (the
    copy rebuilds its own on first use)."""
    state = self.__dict__.copy()
    state.pop("_wt", None)
    state.pop("_w8", None)
    return state


def fp8_operands(mods, x):
    """The fp8 operands of the modules that share x inside ONE autograd
    node (q/k/v, gate/up), or None: the node takes the fp8 route for all
    of them or for none."""
    f8 = tuple(_weight_fp8(m, x) for m in mods)
    return None if None in f8 else f8


def _custom_gemm(w, wt) -> bool:
    """Route this projection through the hand-written NT MFMA GEMM
    (gemm.hip), forward and dgrad? Opt-in with DTX_CUSTOM_GEMM=1: the
    kernel measures 1.25-1.33 PF/s on the mb24 training shapes vs the
    tuned hipBLASLt picks' 1.47-1.67 (tools/bench_mygemm.py, within-probe
    A/B), so it stays off until it wins. Needs both [N,K] and [K,N]
    inside the kernel's support and, for the dgrad, the cached W^T."""
    if os.environ.get("DTX_CUSTOM_GEMM", "0") != "1":
        return False
    if wt is None and torch.is_grad_enabled():
        return False
    n, k = w.shape
    return (w.is_cuda and w.dtype == torch.bfloat16
            and gemm_nt_supported(n, k) and gemm_nt_supported(k, n))


class FrozenLinear(nn.Module):
    """Bias-free frozen linear (Llama projections are bias-free)."""

    __getstate__ = _state_without_wt

    def __init__(self, in_features: int, out_features: int,
                 dtype=torch.bfloat16):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(
            torch.empty(out_features, in_features, dtype=dtype),
            requires_grad=False)

    def forward(self, x, residual=None):
        if x.is_cuda and x.numel() == x.shape[-1]:
            from ..ops import gemv
            y = gemv(x, self.weight)         # decode: streaming GEMV
            return y if residual is None else y + residual
        if not self.weight.requires_grad and skinny_decode_rows(x, 2):
            # batched decode (2-16 rows, no grad): the weight-streaming
            # kernel, the residual in its epilogue
            return skinny_linear(x, self.weight, residual)
        if not self.weight.requires_grad:
            # one node: residual add in the GEMM epilogue without a copy
            # of the residual, dgrad against the cached W^T
            wt, f8 = base_operands(self, x)
            return FrozenGemm.apply(x, self.weight, wt, residual,
                                    _custom_gemm(self.weight, wt), f8)
        # trainable base (full-parameter training): torch's own nodes
        if residual is not None:
            # fold the residual add into the GEMM epilogue (addmm,
            # beta=1): one kernel instead of linear + elementwise add
            xs = x.shape
            x2 = x.reshape(-1, xs[-1])
            r2 = residual.reshape(-1, self.out_features)
            return torch.addmm(r2, x2, self.weight.t()).reshape(
                *xs[:-1], self.out_features)
        return F.linear(x, self.weight)


def draw_dropout_seed() -> int:
    """Per-call seed of the fused LoRA dropout, drawn from torch's
    generator so dropout stays reproducible under torch.manual_seed."""
    return int(torch.randint(0, 2**31 - 1, (1,)).item())


class LoRALinearModule(nn.Module):
    """Frozen base weight + trainable LoRA A/B (HF layouts: A [r,in],
    B [out,r]); scale = alpha / r (reference defaults r=8 alpha=32 —
    cmd/tuning/parser.py:138-149). Training with dropout > 0 hands the
    fused node one (seed, keep) per call; how the mask reaches each
    kernel is decided in the op layer (ops.lora_expand_add_t), never
    here."""

    __getstate__ = _state_without_wt

    def __init__(self, in_features: int, out_features: int, r: int = 8,
                 alpha: float = 32.0, dropout: float = 0.0,
                 dtype=torch.bfloat16):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.r, self.alpha, self.dropout = r, alpha, dropout
        self.scale = alpha / r
        self.weight = nn.Parameter(
            torch.empty(out_features, in_features, dtype=dtype),
            requires_grad=False)
        self.lora_A = nn.Parameter(torch.empty(r, in_features, dtype=dtype))
        self.lora_B = nn.Parameter(torch.zeros(out_features, r, dtype=dtype))
        nn.init.kaiming_uniform_(self.lora_A, a=math.sqrt(5))

    def forward(self, x):
        wt, f8 = base_operands(self, x)
        seed, keep = 0, 1.0
        if self.training and self.dropout > 0.0:
            seed, keep = draw_dropout_seed(), 1.0 - self.dropout
        return _FusedLoRAFn.apply(x, self.weight, self.lora_A, self.lora_B,
                                  self.scale, wt, seed, keep,
                                  _custom_gemm(self.weight, wt), f8)

    def merged_weight(self):
        """W + s·B@A — used by the serving engine (no adapter overhead)."""
        return (self.weight.float()
                + self.scale * (self.lora_B.float() @ self.lora_A.float())
                ).to(self.weight.dtype)


def lora_state_dict(model: nn.Module, prefix: str = "base_model.model."):
    out = {}
    for name, mod in model.named_modules():
        if isinstance(mod, LoRALinearModule):
            out[f"{prefix}{name}.lora_A.weight"] = mod.lora_A.detach().cpu()
            out[f"{prefix}{name}.lora_B.weight"] = mod.lora_B.detach().cpu()
    return out


def save_adapter(model: nn.Module, out_dir: str, *, r: int, alpha: float,
                 dropout: float, target_modules: list[str],
                 base_model_name_or_path: str = ""):
    """Write HF-PEFT adapter layout (adapter_config.json +
    adapter_model.safetensors)."""
    os.makedirs(out_dir, exist_ok=True)
    from safetensors.torch import save_file
    sd = {k: v.contiguous() for k, v in lora_state_dict(model).items()}
    save_file(sd, os.path.join(out_dir, "adapter_model.safetensors"))
    cfg = {
        "peft_type": "LORA",
        "task_type": "CAUSAL_LM",
        "r": r,
        "lora_alpha": alpha,
        "lora_dropout": dropout,
        "target_modules": target_modules,
        "base_model_name_or_path": base_model_name_or_path,
        "bias": "none",
        "fan_in_fan_out": False,
        "inference_mode": False,
        "modules_to_save": None,
    }
    with open(os.path.join(out_dir, "adapter_config.json"), "w") as f:
        json.dump(cfg, f, indent=2)


def load_adapter(model: nn.Module, adapter_dir: str,
                 prefix: str = "base_model.model."):
    from safetensors.torch import load_file
    sd = load_file(os.path.join(adapter_dir, "adapter_model.safetensors"))
    mods = {n: m for n, m in model.named_modules()
            if isinstance(m, LoRALinearModule)}
    n_loaded = 0
    for key, tensor in sd.items():
        if not key.startswith(prefix):
            continue
        rest = key[len(prefix):]
        for suffix, attr in ((".lora_A.weight", "lora_A"),
                             (".lora_B.weight", "lora_B")):
            if rest.endswith(suffix):
                mod_name = rest[: -len(suffix)]
                if mod_name in mods:
                    getattr(mods[mod_name], attr).data.copy_(
                        tensor.to(getattr(mods[mod_name], attr).dtype))
                    n_loaded += 1
    return n_loaded
