"""int8 KV cache on the GPU (kvq.hip): the fused quantize-append against
the quantizer's definition, the GQA-shared decode kernel against fp64
attention over exactly the numbers it reads, the binding contract and the
engine option."""

import pytest
import torch

import kernel_check as kc
import kv_int8_cases as cases
from datatunerx_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CAP = 640       # 5 chunks at D = 128, 3 at D = 64


def _dev(ts):
    return tuple(t.to(DEV) for t in ts)


# ------------------------------------------------------------- 1. append
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("start", [0, 5])
def test_append_host_mode(D, start):
    B, S, Hkv, Bc, max_s = 2, 3, 2, 3, 9
    k, v = cases.kv_rows(B, S, Hkv, D, seed=D + start)
    cache = cases.empty_cache(Bc, max_s, Hkv, D, DEV)
    ops.kv_quant_append(k.to(DEV), v.to(DEV), *cache, start=start)
    slots = [b * max_s + start + s for b in range(B) for s in range(S)]
    cases.check_append(cache, k, v, slots, f"host D={D} start={start}")


@pytest.mark.parametrize("D", [64, 128])
def test_append_device_mode(D):
    Hkv, Bc, max_s = 2, 3, 9
    k, v = cases.kv_rows(3, 1, Hkv, D, seed=D)
    cache = cases.empty_cache(Bc, max_s, Hkv, D, DEV)
    wpos = torch.tensor([4, 9, 26], device=DEV)
    ops.kv_quant_append(k.to(DEV), v.to(DEV), *cache, wpos=wpos)
    cases.check_append(cache, k, v, [4, 9, 26], f"wpos D={D}")
    before = [t.clone() for t in cache]
    for bad in (Bc * max_s, -1):
        ops.kv_quant_append(k[:1].to(DEV), v[:1].to(DEV), *cache,
                            wpos=torch.tensor([bad], device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(before, cache))


# ------------------------------------------------------------- 2. decode
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (8, 2), (16, 2), (16, 1)])
def test_decode_matches_fp64(Hq, Hkv, D):
    B = 3
    q, k, v, _ = kc.attn_inputs(B, Hq, Hkv, 1, CAP, D, seed=Hq + D)
    v = (v.float() * 4).to(torch.bfloat16)       # K at 0.5, V at 2.0
    cache = cases.empty_cache(B, CAP, Hkv, D, "cpu")
    ops.kv_quant_append(k, v, *cache)            # the reference quantizer
    k8, v8, ks, vs = cache
    kd = k8.double() * ks.double().permute(0, 2, 1)[..., None]
    vd = v8.double() * vs.double().permute(0, 2, 1)[..., None]
    assert ops._EXT.attn_decode_q8_nsplit(CAP, Hkv, D) >= 3
    qg, cg = q.to(DEV), _dev(cache)
    report = {}

    def check(o, lse, b, n, tag):
        want = kc.attn_ref64(q[b:b + 1], kd[b:b + 1, :n], vd[b:b + 1, :n],
                             causal=False)
        kc.check_attn({"o": o, "lse": lse}, want, ("o",), tag=tag,
                      report=report)

    row1 = tuple(t[1:2] for t in cg)
    for n in (1, 31, 33, 129, CAP):          # 129: chunks 2.. are empty
        ld = torch.tensor([n], dtype=torch.int32, device=DEV)
        o, lse = ops.attn_decode_q8(qg[1:2], *row1, len_dev=ld)
        check(o, lse, 1, n, f"len {n} ")
        oh, lh = ops.attn_decode_q8(qg[1:2], *row1, length=n)
        assert torch.equal(o, oh) and torch.equal(lse, lh)
    lens = [1, CAP, 129]
    o3, lse3 = ops.attn_decode_q8(qg, *cg, len_dev=torch.tensor(
        lens, dtype=torch.int32, device=DEV))
    for b, n in enumerate(lens):
        check(o3[b:b + 1], lse3[b:b + 1], b, n, f"batch row {b} ")
    # the same row alone: the split plan and so the bits ignore the batch
    o1, lse1 = ops.attn_decode_q8(qg[1:2], *row1)
    assert torch.equal(o1, o3[1:2]) and torch.equal(lse1, lse3[1:2])
    print(f"[kv_int8] Hq={Hq} Hkv={Hkv} D={D}: worst o err/bound "
          f"{max(report.values()):.4f}")


# --------------------------------------------------- 3. binding contract
def _decode_args(Hq=2, Hkv=2, D=64, B=1, Bc=1, max_s=8):
    q = torch.zeros(B, 1, Hq, D, dtype=torch.bfloat16, device=DEV)
    k8 = torch.zeros(Bc, max_s, Hkv, D, dtype=torch.int8, device=DEV)
    ks = torch.ones(Bc, Hkv, max_s, device=DEV)
    return [q, k8, k8.clone(), ks, ks.clone()]


def test_binding_contract():
    a = _decode_args()
    o, lse = ops.attn_decode_q8(*a)
    assert o.shape == a[0].shape and lse.shape == (1, 2, 1)
    assert not o.any()                       # V is all zero
    k = torch.zeros(1, 1, 2, 64, dtype=torch.bfloat16, device=DEV)
    ops.kv_quant_append(k, k, *a[1:])
    assert float(a[3][0, 0, 0]) == pytest.approx(1e-8 / 127, rel=1e-6)

    bf = _decode_args()
    bf[1] = bf[1].to(torch.bfloat16)
    wrong = _decode_args()                   # scales [1,4,8] for Hkv = 2
    wrong[3] = torch.ones(1, 4, 8, device=DEV)
    b3 = _decode_args(B=3, Bc=3)
    two = torch.ones(2, dtype=torch.int32, device=DEV)
    refused = [
        (ops.attn_decode_q8, _decode_args(Hq=32, Hkv=1), {}, "GQA group"),
        (ops.attn_decode_q8, _decode_args(D=96), {}, "D must be"),
        (ops.attn_decode_q8, bf, {}, "k8 must be int8"),
        (ops.attn_decode_q8, wrong, {}, "ks must be"),
        (ops.attn_decode_q8, b3, {"len_dev": two}, r"\[1\] or \[B\]"),
        (ops.attn_decode_q8, _decode_args(), {"length": 9}, "length"),
        (ops.kv_quant_append, [k.expand(1, 3, 2, 64).contiguous()] * 2
         + a[1:], {"start": 6}, "rows 6"),
        (ops.kv_quant_append, [k, k] + wrong[1:], {}, "ks must be"),
    ]
    for fn, args, kw, match in refused:
        with pytest.raises(RuntimeError, match=match):
            fn(*args, **kw)
    assert not ops.kv_int8_supported(32, 1, 128)
    assert not ops.kv_int8_supported(4, 4, 96)
    assert ops.kv_int8_supported(32, 8, 128)


# ------------------------------------------------------------- 4. engine
def test_engine_int8_gpu():
    """Ragged batch == per-request generation on the int8 cache, and the
    graphed step replays: two requests of different length through one
    graphed engine reproduce the eager engine's tokens."""
    from datatunerx_amd.serve.engine import InferenceEngine
    model = cases.tiny_llama(DEV, torch.bfloat16)
    eager, cls = cases.check_engine_batch(model, DEV, graph_decode=False)
    graphed = InferenceEngine(model, template="vanilla", device=DEV,
                              kv_cache="int8")
    for text in ("hello world", "a much longer prompt with many words in"):
        p = eager.tok.encode(text, add_special_tokens=True)
        want = eager.generate(p, max_new_tokens=12)
        assert graphed.generate(p, max_new_tokens=12) == want
    assert graphed._graphed is not None
    assert all(type(c) is cls for c in graphed._graphed.caches)
