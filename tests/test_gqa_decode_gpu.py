"""GQA-shared bf16 decode (attn_decode_gqa.hip): the kernel against fp64
attention over the live rows, attn_fwd's routing, the binding contract and
a graphed decode step of a GQA model with the kernel on and off."""

import pytest
import torch

import kernel_check as kc
from datatunerx_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
if torch.cuda.is_available():
    assert ops.have_ext(), "HIP extension must be built for GPU tests"
CAP = 4224     # 17 chunks of 256 rows (two tiles a wave), the last of 128


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------- 1. kernel
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (8, 2), (7, 1), (12, 4), (16, 1)])
def test_decode_matches_fp64(Hq, Hkv, D):
    q, k, v, _ = kc.attn_inputs(3, Hq, Hkv, 1, CAP, D, seed=Hq + D)
    v = (v.float() * 4).to(torch.bfloat16)       # K at 0.5, V at 2.0
    assert ops._EXT.attn_decode_gqa_nsplit(CAP, Hkv, D) >= 3
    chunk = ops._EXT.attn_decode_gqa_chunk(CAP, Hkv, D)
    qg, kg, vg = q.to(DEV), k.to(DEV), v.to(DEV)
    report = {}

    def check(o, lse, b, n, tag):
        want = kc.attn_ref64(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n],
                             causal=False)
        kc.check_attn({"o": o, "lse": lse}, want, ("o",), tag=tag,
                      report=report)

    q1, k1, v1 = qg[1:2], kg[1:2], vg[1:2]
    for n in (1, 31, 32, 33, chunk - 1, chunk, chunk + 1, CAP):
        o, lse = ops.attn_decode_gqa(q1, k1, v1, len_dev=_i32([n]))
        check(o, lse, 1, n, f"len {n} ")
    # the B = 1 prefix view of a larger cache, no len_dev and no copy
    n = chunk + 33
    o, lse = ops.attn_decode_gqa(q1, k1[:, :n], v1[:, :n])
    check(o, lse, 1, n, f"prefix view {n} ")

    lens = [1, CAP, chunk + 1]
    o3, lse3 = ops.attn_decode_gqa(qg, kg, vg, len_dev=_i32(lens))
    for b, n in enumerate(lens):
        check(o3[b:b + 1], lse3[b:b + 1], b, n, f"batch row {b} ")
    # the same row alone: the split plan and so the bits ignore the batch
    o1, lse1 = ops.attn_decode_gqa(q1, k1, v1, len_dev=_i32([CAP]))
    assert torch.equal(o1, o3[1:2]) and torch.equal(lse1, lse3[1:2])
    # dead rows are neither read into the math nor multiplied by p = 0
    outs = []
    for fill in (0.0, float("nan")):
        kf, vf = kg.clone(), vg.clone()
        for b, n in enumerate(lens):
            kf[b, n:] = fill
            vf[b, n:] = fill
        outs.append(ops.attn_decode_gqa(qg, kf, vf, len_dev=_i32(lens)))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], o3)
    print(f"[gqa_decode] Hq={Hq} Hkv={Hkv} D={D}: worst o err/bound "
          f"{max(report.values()):.4f}")


# ------------------------------------------------------------ 2. routing
def test_routing(monkeypatch):
    # G = 4 routes by default from a capacity of 8192 rows
    q, k, v, _ = kc.attn_inputs(2, 8, 2, 1, 8192, 64, seed=1)
    ld = _i32([200, 8192])

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    qg, kg, vg = q.to(DEV), k.to(DEV), v.to(DEV)
    scale = 64 ** -0.5
    monkeypatch.delenv("DTX_GQA_DECODE", raising=False)
    new = ops.attn_decode_gqa(qg, kg, vg, len_dev=ld)
    old = ops._EXT.attn_decode(qg, kg, vg, scale, ld)
    assert same(ops.attn_fwd(qg, kg, vg, len_dev=ld), new)
    mha = (qg, kg.repeat_interleave(4, dim=2), vg.repeat_interleave(4, dim=2))
    old_mha = ops._EXT.attn_decode(*mha, scale, ld)
    assert same(ops.attn_fwd(*mha, len_dev=ld), old_mha)
    small = (qg, kg[:, :384].contiguous(), vg[:, :384].contiguous())
    ld_s = _i32([200, 384])                  # G = 4 below 8192: measured loss
    assert same(ops.attn_fwd(*small, len_dev=ld_s),
                ops._EXT.attn_decode(*small, scale, ld_s))
    monkeypatch.setenv("DTX_GQA_DECODE", "1")    # forced wherever supported
    assert same(ops.attn_fwd(*small, len_dev=ld_s),
                ops.attn_decode_gqa(*small, len_dev=ld_s))
    assert same(ops.attn_fwd(*mha, len_dev=ld), old_mha)
    monkeypatch.setenv("DTX_GQA_DECODE", "0")
    assert same(ops.attn_fwd(qg, kg, vg, len_dev=ld), old)
    assert same(ops.attn_fwd(*mha, len_dev=ld), old_mha)
    cpu = ops.attn_decode_gqa(q, k, v, len_dev=ld.cpu())
    assert same(cpu, ops.attn_fwd(q, k, v, len_dev=ld.cpu()))


# --------------------------------------------------- 3. binding contract
def _args(Hq=2, Hkv=1, D=64, B=1, Skv=8):
    """All-zero inputs: whatever a missing check would let through reads
    and writes inside these allocations."""
    q = torch.zeros(B, 1, Hq, D, dtype=torch.bfloat16, device=DEV)
    k = torch.zeros(B, Skv, Hkv, D, dtype=torch.bfloat16, device=DEV)
    return [q, k, k.clone()]


def test_binding_contract():
    a = _args()
    o, lse = ops.attn_decode_gqa(*a)
    assert o.shape == a[0].shape and lse.shape == (1, 2, 1)
    assert not o.any()                       # V is all zero
    o, lse = ops.attn_decode_gqa(*_args(B=0))
    assert o.shape == (0, 1, 2, 64) and lse.shape == (0, 2, 1)

    f32k = _args()
    f32k[1] = f32k[1].float()
    strided = _args(B=2, Skv=16)             # a batched prefix view
    strided[1], strided[2] = strided[1][:, :8], strided[2][:, :8]
    b3 = _args(B=3)
    refused = [
        (_args(Hq=2, Hkv=2), {}, "GQA group"),
        (_args(Hq=17, Hkv=1), {}, "GQA group"),
        (_args(D=96), {}, "D must be"),
        (f32k, {}, "k must be bf16"),
        (strided, {}, "contiguous"),
        (b3, {"len_dev": _i32([1, 1])}, r"\[1\] or \[B\]"),
        (b3, {"len_dev": torch.ones(3, dtype=torch.int64, device=DEV)},
         "len_dev must be int32"),
    ]
    for args, kw, match in refused:
        with pytest.raises(RuntimeError, match=match):
            ops.attn_decode_gqa(*args, **kw)
    assert ops.gqa_decode_supported(32, 8, 128)
    assert ops.gqa_decode_supported(28, 4, 128)
    assert not ops.gqa_decode_supported(4, 4, 64)
    assert not ops.gqa_decode_supported(17, 1, 64)
    assert not ops.gqa_decode_supported(8, 2, 96)


# ------------------------------------------------------- 4. in the model
def test_graphed_decode_logits(monkeypatch):
    """llama-mini with one kv head (G = 4, D = 64): prefill, then graphed
    decode steps at B = 2, the shared kernel (forced: this capacity is
    outside the default routing) against the per-head one.
    Logits, not tokens: two correct kernels may break a near-tie apart."""
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import _GraphedDecoder
    from test_skinny_gpu import check
    cfg = LlamaConfig.mini(num_key_value_heads=1)
    assert ops.gqa_decode_supported(cfg.num_attention_heads, 1, cfg.head_dim)
    with torch.device(DEV):
        model = LlamaForCausalLM(cfg, lora=False, dtype=torch.bfloat16)
    model.init_random(seed=3)
    model.eval()
    prompts = [list(range(4, 41)), list(range(50, 63))]
    steps = torch.tensor([[7, 9], [11, 13], [15, 17]], device=DEV)
    logits = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("DTX_GQA_DECODE", knob)
        gd = _GraphedDecoder(model, cfg, DEV, 2, 64)
        with torch.no_grad():
            for i, p in enumerate(prompts):
                model(torch.tensor([p], device=DEV), pos0=0,
                      kv_caches=[c.row_view(i) for c in gd.caches])
        gd.set_state([len(p) for p in prompts])
        logits[knob] = []
        for cur in steps:
            gd.step(cur.view(2, 1))
            logits[knob].append(gd.logits[:, -1].float().cpu())
    for i, (new, old) in enumerate(zip(logits["1"], logits["0"])):
        check(new, old, f"graphed step {i} logits")
