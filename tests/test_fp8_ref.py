"""FP8 base GEMMs without a GPU: the reference quantizer, the mode switch
(flag, CR field, refusals) and a LoRA run on the CPU twins that shows which
modules take the route and what they cache."""

import pytest
import torch

from datatunerx_amd.api.types import Hyperparameter
from datatunerx_amd.api.validation import ValidationError, validate_ as validate
from datatunerx_amd.data.dataset import SFTDataset
from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
from datatunerx_amd.models.lora import FrozenLinear, LoRALinearModule
from datatunerx_amd.ops import reference as ref
from datatunerx_amd.train.args import get_train_args
from datatunerx_amd.train.trainer import SFTTrainer, TrainerConfig


def test_reference_quant_round_trips_representable_rows():
    # every e4m3 value once per row, times a power-of-two row scale: the
    # row's absmax is 448 * scale, so quantizing recovers the codes exactly
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn)
    codes = codes[~codes.float().isnan()].float()
    x = (codes[None, :] * torch.tensor([[0.25], [1.0], [8.0]])).bfloat16()
    q, s = ref.quant_fp8_rows(x)
    assert torch.equal(s, torch.tensor([0.25, 1.0, 8.0]))
    assert torch.equal(q.float(), codes.expand(3, -1))
    assert float(q.float().abs().max()) == 448.0
    assert torch.equal((q.float() * s[:, None]).bfloat16(), x)


def hp(**params):
    return Hyperparameter.from_dict({
        "kind": "Hyperparameter", "metadata": {"name": "h"},
        "spec": {"parameters": params}})


def test_mode_switch_accepts_and_refuses():
    assert get_train_args(["--base_gemm", "fp8"])[1].base_gemm == "fp8"
    assert get_train_args([])[1].base_gemm == "bf16"
    with pytest.raises(ValueError, match="base_gemm"):
        get_train_args(["--base_gemm", "fp8", "--finetuning_type", "full"])
    with pytest.raises(ValueError, match="base_gemm"):
        get_train_args(["--base_gemm", "fp16"])
    validate(hp(baseGemm="fp8"))
    with pytest.raises(ValidationError, match="baseGemm"):
        validate(hp(baseGemm="fp16"))
    with pytest.raises(ValidationError, match="baseGemm"):
        validate(hp(baseGemm="fp8", PEFT=False))


def test_lora_run_on_cpu_takes_the_fp8_route(tmp_path):
    cfg = LlamaConfig.tiny(lora_dropout=0.0)
    model = LlamaForCausalLM(cfg, lora=True,
                             dtype=torch.bfloat16).init_random()
    ds = SFTDataset.synthetic(8, 32, cfg.vocab_size)
    tcfg = TrainerConfig(output_dir=str(tmp_path), max_steps=2,
                         micro_batch_size=2, logging_steps=1,
                         base_gemm="fp8")
    loss = SFTTrainer(model, ds, tcfg,
                      device=torch.device("cpu")).train()
    assert loss == loss and abs(loss) != float("inf")
    routed = [m for n, m in model.named_modules()
              if isinstance(m, (FrozenLinear, LoRALinearModule))
              and n != "lm_head"]
    assert len(routed) == 7 * cfg.num_hidden_layers
    for m in routed:
        w8, sw, wt8, swt = m.__dict__["_w8"][1]
        assert w8.dtype == wt8.dtype == torch.float8_e4m3fn
        assert w8.shape == m.weight.shape and wt8.shape == w8.t().shape
        assert sw.shape == (w8.shape[0],) and swt.shape == (w8.shape[1],)
        assert "_wt" not in m.__dict__
    assert "_w8" not in model.lm_head.__dict__
    assert not any("_w8" in k for k in model.state_dict())
