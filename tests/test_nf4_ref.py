"""NF4 base weights on the CPU: the format (levels, nearest-level rule,
nibble order), its error against linear int4, and the way from the public
switches (build_model, the server flag, serveConfig, the Hyperparameter
`nf4` parameter) down to modules that hold the codebook."""

import pytest
import torch

from datatunerx_amd.models.quant import (NF4_CODE, QuantFrozenLinear,
                                         dequantize_int4, dequantize_nf4,
                                         quantize_int4, quantize_nf4)


def test_levels_requantize_to_their_index():
    code = torch.tensor(NF4_CODE)
    assert len(NF4_CODE) == 16 and NF4_CODE[7] == 0.0
    assert (code[1:] > code[:-1]).all()
    for absmax in (1e-3, 0.37, 5.0):
        w = (code * absmax).repeat(4).view(1, 64)   # one group, all levels
        packed, am = quantize_nf4(w, 64)
        idx = torch.stack([packed & 0xF, packed >> 4], dim=2).view(-1)
        assert idx.tolist() == list(range(16)) * 4
        assert torch.equal(am, torch.full((1, 1), absmax))
        assert torch.equal(dequantize_nf4(packed, am, torch.float32), w)


def test_dequant_quant_is_a_fixed_point():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(16, 128, generator=g) * 0.3).to(torch.bfloat16)
    p1, a1 = quantize_nf4(w, 32)
    d1 = dequantize_nf4(p1, a1, torch.float32, 32)
    p2, a2 = quantize_nf4(d1, 32)
    assert torch.equal(p1, p2) and torch.equal(a1, a2)
    assert torch.equal(dequantize_nf4(p2, a2, torch.float32, 32), d1)


def test_packed_layout_even_k_in_low_nibble():
    w = torch.zeros(1, 64)
    w[0, 0], w[0, 1], w[0, 2], w[0, 3] = -2.0, 2.0, 1.0, 0.0
    packed, absmax = quantize_nf4(w, 64)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (1, 32)
    assert absmax.item() == 2.0
    # k0 = -1 (idx 0), k1 = +1 (15), k2 = 0.5 (nearest 0.4407: 12), k3 = 0 (7)
    assert packed[0, 0].item() == 0 | 15 << 4
    assert packed[0, 1].item() == 12 | 7 << 4
    assert (packed[0, 2:] == (7 | 7 << 4)).all()


def test_nf4_error_below_int4():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(64, 256, generator=g) * 0.3).to(torch.bfloat16)

    def rms(d):
        return (d - w.float()).pow(2).mean().sqrt().item()

    e_nf4 = rms(dequantize_nf4(*quantize_nf4(w), torch.float32))
    e_int4 = rms(dequantize_int4(*quantize_int4(w), torch.float32))
    print(f"rms error nf4 / int4 = {e_nf4 / e_int4:.3f}")
    assert e_nf4 < e_int4


def test_build_model_nf4_generates():
    from datatunerx_amd.models.lora import FrozenLinear, LoRALinearModule
    from datatunerx_amd.serve.engine import InferenceEngine, build_model
    cpu = torch.device("cpu")
    model = build_model("llama-tiny", cpu, quantization="nf4")
    assert not any(isinstance(m, (FrozenLinear, LoRALinearModule))
                   for m in model.modules())
    quant = [m for m in model.modules() if isinstance(m, QuantFrozenLinear)]
    assert quant and all(m.bits == 4 and m.codebook == "nf4" for m in quant)
    eng = InferenceEngine(model, device=cpu)
    out = eng.generate(list(range(4, 12)), max_new_tokens=4)
    assert 0 < len(out) <= 4
    assert out == eng.generate(list(range(4, 12)), max_new_tokens=4)


def test_switches_accept_nf4():
    from datatunerx_amd.api.controllers import FinetuneController
    from datatunerx_amd.api.types import (Finetune, FinetuneJob,
                                          Hyperparameter)
    from datatunerx_amd.api.validation import ValidationError, validate_
    from datatunerx_amd.serve import server
    args = server.parse_args(["--quantization", "nf4", "--model",
                              "llama-tiny"])
    assert args.quantization == "nf4"
    spec = {"fineTune": {"finetuneSpec": {
        "llm": "llama-tiny", "dataset": "ds",
        "hyperparameter": {"hyperparameterRef": "hp"}, "node": 1}}}
    validate_(FinetuneJob(name="q", spec={
        **spec, "serveConfig": {"quantization": "nf4"}}))
    with pytest.raises(ValidationError, match="tensorParallel"):
        validate_(FinetuneJob(name="tp", spec={
            **spec, "serveConfig": {"quantization": "nf4",
                                    "tensorParallel": 2}}))
    validate_(Hyperparameter(name="h", spec={"parameters": {"nf4": True}}))
    with pytest.raises(ValidationError, match="mutually exclusive"):
        validate_(Hyperparameter(name="h2", spec={
            "parameters": {"nf4": True, "int4": True}}))
    ctl = FinetuneController.__new__(FinetuneController)
    ctl.cfg = type("Cfg", (), {"default_model": "llama-tiny",
                               "metrics_export_address": "",
                               "storage_path": ""})()
    a = ctl.build_args(Finetune(name="f", spec={"llm": "llama-tiny"}),
                       {"nf4": True}, None, "out")
    assert a[a.index("--quantization") + 1] == "nf4"
