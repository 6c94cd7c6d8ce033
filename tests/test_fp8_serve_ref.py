"""FP8 serving on the CPU: the e4m3 module against the fp8 contract, and the
base_gemm switch through engine, server flag, admission and reconciler."""

import pytest
import torch

from datatunerx_amd import ops
from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
from datatunerx_amd.models.lora import FrozenLinear, LoRALinearModule
from datatunerx_amd.models.quant import QuantFrozenLinear, quantize_model_
from datatunerx_amd.ops import reference as ref
from test_quant_serve import _FakeSupervisor, _job

BF, F8 = torch.bfloat16, torch.float8_e4m3fn
CPU = torch.device("cpu")


@pytest.mark.parametrize("M", [3, 40])
def test_e4m3_frozen_linear_is_the_reference_definition(M):
    g = torch.Generator().manual_seed(M)
    w = (torch.randn(24, 128, generator=g) / 8).to(BF)
    x = torch.randn(M, 128, generator=g).to(BF)
    m = QuantFrozenLinear.from_weight(w, bits=8, codebook="e4m3")
    w8, sw = ref.quant_fp8_rows(w)
    assert m.qweight.dtype == F8 and torch.equal(m.scale, sw)
    assert torch.equal(m.qweight.view(torch.uint8), w8.view(torch.uint8))
    x8, sa = ref.quant_fp8_rows(x)
    want = ((x8.float() @ w8.float().t()) * sa[:, None] * sw).to(BF)
    assert torch.equal(m(x), want)
    assert torch.equal(ops.qlinear(x, w8, sw, 8, codebook="e4m3"), want)
    assert ops.qlinear_supported(16, 24, 128, 8, codebook="e4m3")
    assert not ops.qlinear_supported(4, 24, 192, 8, codebook="e4m3")


def test_quantize_model_e4m3_drops_bf16_and_keeps_lm_head():
    model = LlamaForCausalLM(LlamaConfig.tiny(), lora=True, dtype=BF)
    model.init_random()
    head = model.lm_head.weight.clone()
    quantize_model_(model, 8, lora_base=True, codebook="e4m3")
    assert type(model.lm_head) is FrozenLinear
    assert torch.equal(model.lm_head.weight, head)
    assert [n for n, m in model.named_modules()
            if isinstance(m, (FrozenLinear, LoRALinearModule))] == ["lm_head"]
    for m in model.modules():
        if isinstance(m, QuantFrozenLinear):
            assert m.qweight.dtype == F8 and m.codebook == "e4m3"
            assert {n for n, _ in m.named_buffers()} == {"qweight", "scale"}
            assert "weight" not in dict(m.named_parameters())


def test_build_model_base_gemm_fp8_generates():
    from datatunerx_amd.serve.engine import InferenceEngine, build_model
    model = build_model("llama-tiny", CPU, base_gemm="fp8")
    eng = InferenceEngine(model, device=CPU)
    out = eng.generate(list(range(4, 12)), max_new_tokens=4)
    assert out == eng.generate(list(range(4, 12)), max_new_tokens=4)
    with pytest.raises(ValueError, match="mutually exclusive"):
        build_model("llama-tiny", CPU, base_gemm="fp8", quantization="int8")


def test_server_base_gemm_flag(monkeypatch):
    from datatunerx_amd.serve import server
    assert server.parse_args(["--base-gemm", "fp8"]).base_gemm == "fp8"
    assert server.parse_args([]).base_gemm == "bf16"
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="tensor-parallel"):
        server.main(["--base-gemm", "fp8", "--model", "llama-tiny"])


@pytest.mark.parametrize("cfg,bad", [
    ({"baseGemm": "fp8"}, None),
    ({"baseGemm": "fp4"}, "baseGemm must be"),
    ({"baseGemm": "fp8", "quantization": "int8"}, "mutually exclusive"),
    ({"baseGemm": "fp8", "tensorParallel": 2}, "tensorParallel")])
def test_validation_serve_base_gemm(cfg, bad):
    from datatunerx_amd.api.validation import ValidationError, validate_
    if bad is None:
        return validate_(_job("j", cfg))
    with pytest.raises(ValidationError, match=bad):
        validate_(_job("j", cfg))


def test_reconcile_serve_passes_base_gemm(tmp_path):
    from datatunerx_amd.api.controllers import (FinetuneJobController,
                                                ManagerConfig, PortAllocator)
    from datatunerx_amd.api.store import Store
    store = Store(str(tmp_path / "state"))
    cfg = ManagerConfig(state_dir=str(tmp_path / "state"),
                        work_dir=str(tmp_path / "work"), cpu_mode=True)
    sup = _FakeSupervisor()
    ctl = FinetuneJobController(store, None, sup, cfg, PortAllocator(34600))
    job = _job("f8serve", {"baseGemm": "fp8"})
    job.status["state"] = "Serve"
    store.create(job)
    ctl._reconcile_serve(job)
    argv, = sup.calls
    assert argv[argv.index("--base-gemm") + 1] == "fp8"
