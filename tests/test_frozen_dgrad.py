"""Dgrad of the frozen projections against a cached W^T: the cache
(models.lora._weight_t) and the autograd nodes that take it. CPU in fp32
with the helper's device condition lifted through its test-only argument,
plus one GPU case in bf16.
"""

import pytest
import torch
import torch.nn.functional as F

from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
from datatunerx_amd.models.lora import (FrozenLinear, LoRALinearModule,
                                        _weight_t)
from datatunerx_amd.ops.autograd import (FrozenGemm, LoRALinear,
                                         PairedFrozenGemm, QKVProj)


def frozen(n=24, k=16, seed=0):
    lin = FrozenLinear(k, n, dtype=torch.float32)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(n, k, generator=g))
    return lin


# ------------------------------------------------------------------ cache
def test_cache_built_once_and_reused():
    lin = frozen()
    wt = _weight_t(lin, any_device=True)
    assert wt.shape == (16, 24) and wt.is_contiguous()
    assert torch.equal(wt, lin.weight.t())
    again = _weight_t(lin, any_device=True)
    assert again.data_ptr() == wt.data_ptr()
    assert not wt.requires_grad


def test_cache_rebuilt_after_copy():
    lin = frozen()
    _weight_t(lin, any_device=True)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(24, 16))
    assert torch.equal(_weight_t(lin, any_device=True), lin.weight.t())
    with torch.no_grad():
        lin.weight.mul_(2)
    assert torch.equal(_weight_t(lin, any_device=True), lin.weight.t())


def test_cache_rebuilt_after_data_mul():
    """An in-place write through `.data`: torch gives `weight.data` a
    version counter of its own, so weight._version and data_ptr() stay
    as they were; the key's count of `.data` uses sees it."""
    lin = frozen()
    _weight_t(lin, any_device=True)
    version = lin.weight._version
    lin.weight.data.mul_(2)
    assert lin.weight._version == version
    assert torch.equal(_weight_t(lin, any_device=True), lin.weight.t())
    lin.weight.data.copy_(torch.randn(24, 16))
    assert torch.equal(_weight_t(lin, any_device=True), lin.weight.t())
    # still an ordinary parameter of the module
    assert isinstance(lin.weight, torch.nn.Parameter)
    assert set(lin.state_dict()) == {"weight"}
    assert type(lin.state_dict()["weight"]) is torch.Tensor
    wt = _weight_t(lin, any_device=True)
    assert _weight_t(lin, any_device=True).data_ptr() == wt.data_ptr()


def test_cache_not_in_state_dict():
    lin = frozen()
    _weight_t(lin, any_device=True)
    assert set(lin.state_dict()) == {"weight"}
    assert [n for n, _ in lin.named_buffers()] == []
    assert [n for n, _ in lin.named_parameters()] == ["weight"]


def test_cache_conditions(monkeypatch):
    lin = frozen()
    assert _weight_t(lin) is None              # CPU fp32: device condition
    with torch.no_grad():
        assert _weight_t(lin, any_device=True) is None
    monkeypatch.setenv("DTX_DGRAD_WT", "0")
    assert _weight_t(lin, any_device=True) is None
    monkeypatch.delenv("DTX_DGRAD_WT")
    lin.weight.requires_grad_(True)
    assert _weight_t(lin, any_device=True) is None
    assert "_wt" not in lin.__dict__           # none of these built it
    lin.weight.requires_grad_(False)
    assert _weight_t(lin, any_device=True) is not None


# ------------------------------------------------------------------ nodes
def rel_close(a, b, tol, name):
    a, b = a.float(), b.float()
    err = (a - b).abs().max() / b.abs().max().clamp(min=1e-6)
    assert err < tol, f"{name}: rel err {err:.3e}"


def bf16_close(got, want, name, rtol=2e-2):
    """assert_close of tests/test_ops_gpu.py."""
    got, want = got.float(), want.float()
    denom = want.abs().max().clamp(min=1e-3)
    err = (got - want).abs().max() / denom
    assert err < rtol, f"{name}: rel err {err:.4f} (max {denom:.3f})"


class Case:
    """One shape's tensors, made once per (device, dtype, keep)."""

    def __init__(self, dev, dtype, M, K, N, r, keep):
        g = torch.Generator().manual_seed(3)

        def mk(*s, scale=1.0):
            return (torch.randn(*s, generator=g) * scale).to(dev, dtype)
        self.x = mk(M, K)
        self.w = [mk(N, K, scale=K ** -0.5) for _ in range(3)]
        self.wt = [w.t().contiguous() for w in self.w]
        self.a = [mk(r, K, scale=K ** -0.5) for _ in range(2)]
        self.b = [mk(N, r, scale=0.3) for _ in range(2)]
        self.res = mk(M, N)
        self.dy = [mk(M, N) for _ in range(3)]
        self.keep, self.scale = keep, 4.0


def run_node(c, node, use_wt, x_grad=True, custom=False):
    """(outputs, grads by name) of one node; wt given or None. custom:
    the hand-written GEMM (FrozenGemm and LoRALinear only)."""
    x = c.x.clone().requires_grad_(x_grad)
    wt = c.wt if use_wt else [None] * 3
    a = [t.clone().requires_grad_(True) for t in c.a]
    b = [t.clone().requires_grad_(True) for t in c.b]
    res = c.res.clone().requires_grad_(True)
    grads = {}
    if node == "frozen":
        ys = (FrozenGemm.apply(x, c.w[0], wt[0], None, custom),)
    elif node == "frozen_res":
        ys = (FrozenGemm.apply(x, c.w[0], wt[0], res, custom),)
    elif node == "paired":
        ys = PairedFrozenGemm.apply(x, c.w[0], c.w[1], wt[0], wt[1])
    elif node == "qkv":
        ys = QKVProj.apply(x, c.w[0], a[0], b[0], c.w[1], c.w[2], a[1],
                           b[1], c.scale, 11, 12, c.keep, *wt)
    elif node == "lora":
        ys = (LoRALinear.apply(x, c.w[0], a[0], b[0], c.scale, wt[0], 11,
                               c.keep, custom),)
    torch.autograd.backward(ys, c.dy[:len(ys)])
    grads["x"] = x.grad
    if node == "frozen_res":
        grads["res"] = res.grad
    if node in ("qkv", "lora"):
        for i in range(2 if node == "qkv" else 1):
            grads[f"a{i}"], grads[f"b{i}"] = a[i].grad, b[i].grad
    return ys, grads


NODES = ["frozen", "frozen_res", "paired", "qkv", "lora"]


@pytest.fixture(scope="module")
def cpu_cases():
    dev = torch.device("cpu")
    return {keep: Case(dev, torch.float32, 37, 48, 40, 8, keep)
            for keep in (1.0, 0.9)}


@pytest.mark.parametrize("keep", [1.0, 0.9])
@pytest.mark.parametrize("node", NODES)
def test_nodes_wt_matches_plain_cpu(cpu_cases, node, keep):
    c = cpu_cases[keep]
    ys, g = run_node(c, node, use_wt=True)
    ys0, g0 = run_node(c, node, use_wt=False)
    for i, (y, y0) in enumerate(zip(ys, ys0)):
        rel_close(y, y0, 1e-5, f"{node} y{i}")
    assert set(g) == set(g0)
    for name in g:
        rel_close(g[name], g0[name], 1e-5, f"{node} d{name}")
    if node == "frozen_res":
        assert torch.equal(g["res"], c.dy[0])


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [1.0, 0.9])
def test_nodes_wt_matches_plain_gpu(keep):
    c = Case(torch.device("cuda:0"), torch.bfloat16, 200, 512, 512, 8, keep)
    for node in NODES:
        ys, g = run_node(c, node, use_wt=True)
        ys0, g0 = run_node(c, node, use_wt=False)
        for i, (y, y0) in enumerate(zip(ys, ys0)):
            bf16_close(y, y0, f"{node} y{i}")
        assert set(g) == set(g0)
        for name in g:
            bf16_close(g[name], g0[name], f"{node} d{name}")
        if node == "frozen_res":
            assert torch.equal(g["res"], c.dy[0])


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [1.0, 0.9])
def test_custom_gemm_nodes_match_plain_gpu(keep):
    """custom=True (DTX_CUSTOM_GEMM=1): forward, fused residual and dgrad
    on the hand-written MFMA kernel, against the library path."""
    c = Case(torch.device("cuda:0"), torch.bfloat16, 200, 512, 512, 8, keep)
    for node in ("frozen", "frozen_res", "lora"):
        ys, g = run_node(c, node, use_wt=True, custom=True)
        ys0, g0 = run_node(c, node, use_wt=False)
        bf16_close(ys[0], ys0[0], f"custom {node} y")
        assert set(g) == set(g0)
        for name in g:
            bf16_close(g[name], g0[name], f"custom {node} d{name}")


def test_custom_gemm_knob(monkeypatch):
    """_custom_gemm: off by default, needs the cached W^T in grad mode (so
    DTX_DGRAD_WT=0 switches it off there) and a CUDA bf16 weight."""
    from datatunerx_amd.models.lora import _custom_gemm
    w = torch.zeros(512, 512)
    wt = w.t().contiguous()
    assert not _custom_gemm(w, wt)
    monkeypatch.setenv("DTX_CUSTOM_GEMM", "1")
    assert not _custom_gemm(w, wt)             # CPU fp32 weight
    assert not _custom_gemm(w, None)


# -------------------------------------------------------- needs_input_grad
@pytest.mark.parametrize("node,n_linear,n_addmm", [("qkv", 1, 2),
                                                   ("lora", 1, 0)])
def test_no_dx_when_input_needs_no_grad(cpu_cases, monkeypatch, node,
                                        n_linear, n_addmm):
    c = cpu_cases[0.9]
    calls = {"linear": 0, "addmm_": 0}
    real_linear, real_addmm_ = F.linear, torch.Tensor.addmm_

    def linear(*a, **k):
        calls["linear"] += 1
        return real_linear(*a, **k)

    def addmm_(*a, **k):
        calls["addmm_"] += 1
        return real_addmm_(*a, **k)

    monkeypatch.setattr(F, "linear", linear)
    monkeypatch.setattr(torch.Tensor, "addmm_", addmm_)
    _, g = run_node(c, node, use_wt=True, x_grad=True)
    with_dx = dict(calls)
    calls.update(linear=0, addmm_=0)
    _, g0 = run_node(c, node, use_wt=True, x_grad=False)
    assert g["x"] is not None and g0["x"] is None
    for name in g:
        if name != "x":
            assert torch.equal(g[name], g0[name]), name
    # the base dgrads are the only linear / addmm_ calls that go away
    assert with_dx["linear"] - calls["linear"] == n_linear
    assert with_dx["addmm_"] == n_addmm and calls["addmm_"] == 0


# -------------------------------------------------------------- end to end
def test_tiny_llama_step_matches_plain(monkeypatch):
    """One training step of a 2-layer tiny Llama on the CPU: loss and all
    adapter gradients with the W^T path equal the DTX_DGRAD_WT=0 run."""
    import datatunerx_amd.models.lora as lora_mod
    import datatunerx_amd.models.llama as llama_mod

    cfg = LlamaConfig.tiny(lora_dropout=0.1)
    cfg.num_hidden_layers = 2
    m = LlamaForCausalLM(cfg, lora=True, dtype=torch.float32).init_random()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "lora_B" in n:                  # zero B hides dA and the dx
                p.normal_(std=0.05)            # term from the comparison
    ids = torch.randint(3, cfg.vocab_size, (2, 40),
                        generator=torch.Generator().manual_seed(1))

    def step():
        for p in m.parameters():
            p.grad = None
        torch.manual_seed(5)                   # the dropout seeds
        loss = m(ids, labels=ids.clone())
        loss.backward()
        return loss.detach(), {n: p.grad.clone()
                               for n, p in m.trainable_parameters()}

    built = []
    real = lora_mod._weight_t

    def lifted(mod):
        wt = real(mod, any_device=True)
        built.append(wt is not None)
        return wt

    monkeypatch.setattr(lora_mod, "_weight_t", lifted)
    monkeypatch.setattr(llama_mod, "_weight_t", lifted)
    loss, grads = step()
    n_proj = sum(isinstance(mod, (FrozenLinear, LoRALinearModule))
                 for mod in m.modules())
    assert built and all(built) and len(built) == n_proj
    monkeypatch.setenv("DTX_DGRAD_WT", "0")
    built.clear()
    loss0, grads0 = step()
    assert built and not any(built)
    rel_close(loss, loss0, 1e-5, "loss")
    assert grads.keys() == grads0.keys() and len(grads) == 8
    for n in grads:
        rel_close(grads[n], grads0[n], 1e-5, n)


# ------------------------------------------------- the cache and the module
def test_module_copies_leave_the_cache_behind():
    """deepcopy and whole-module pickling carry the weight (tracked class
    or not) and drop the cached transpose, which the copy rebuilds."""
    import copy
    import io
    lin = frozen()
    wt = _weight_t(lin, any_device=True)
    dup = copy.deepcopy(lin)
    buf = io.BytesIO()
    torch.save(lin, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    assert "_wt" in lin.__dict__
    for other in (dup, loaded):
        assert "_wt" not in other.__dict__
        assert isinstance(other.weight, torch.nn.Parameter)
        assert torch.equal(other.weight, lin.weight)
        assert not other.weight.requires_grad
        wt2 = _weight_t(other, any_device=True)
        assert torch.equal(wt2, wt) and wt2.data_ptr() != wt.data_ptr()
        other.weight.data.mul_(2)
        assert torch.equal(_weight_t(other, any_device=True),
                           other.weight.t())
