"""int8 KV cache on the CPU: the fp32 twins of kvq.hip and the engine
option (ops/reference.py, serve/engine.py)."""

import pytest
import torch

import kernel_check as kc
import kv_int8_cases as cases
from datatunerx_amd import ops
from datatunerx_amd.serve.engine import (InferenceEngine, Int8KVCache,
                                         KVCache, _DecodeState)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("start", [0, 5])
def test_append_host_mode(D, start):
    B, S, Hkv, Bc, max_s = 2, 3, 2, 3, 9
    k, v = cases.kv_rows(B, S, Hkv, D, seed=D + start)
    cache = cases.empty_cache(Bc, max_s, Hkv, D, "cpu")
    ops.kv_quant_append(k, v, *cache, start=start)
    slots = [b * max_s + start + s for b in range(B) for s in range(S)]
    cases.check_append(cache, k, v, slots, f"cpu host D={D} start={start}")


def test_append_device_mode():
    Hkv, D, Bc, max_s = 2, 64, 3, 9
    k, v = cases.kv_rows(3, 1, Hkv, D, seed=1)
    cache = cases.empty_cache(Bc, max_s, Hkv, D, "cpu")
    ops.kv_quant_append(k, v, *cache, wpos=torch.tensor([4, 9, 26]))
    cases.check_append(cache, k, v, [4, 9, 26], "cpu wpos")
    before = [t.clone() for t in cache]
    ops.kv_quant_append(k[:1], v[:1], *cache, wpos=torch.tensor([27]))
    assert all(torch.equal(a, b) for a, b in zip(before, cache))


@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (8, 2)])
def test_decode_matches_fp64(Hq, Hkv):
    D, max_s, lens = 64, 40, [1, 33, 40]
    q, k, v, _ = kc.attn_inputs(3, Hq, Hkv, 1, max_s, D, seed=Hq)
    v = (v.float() * 4).to(torch.bfloat16)       # K at 0.5, V at 2.0
    cache = cases.empty_cache(3, max_s, Hkv, D, "cpu")
    ops.kv_quant_append(k, v, *cache)
    k8, v8, ks, vs = cache
    o, lse = ops.attn_decode_q8(q, *cache, len_dev=torch.tensor(
        lens, dtype=torch.int32))
    for b, n in enumerate(lens):
        kd = k8[b:b + 1, :n].double() * ks[b, :, :n].t()[None, :, :, None]
        vd = v8[b:b + 1, :n].double() * vs[b, :, :n].t()[None, :, :, None]
        want = kc.attn_ref64(q[b:b + 1], kd, vd, causal=False)
        kc.check_attn({"o": o[b:b + 1], "lse": lse[b:b + 1]}, want, ("o",),
                      tag=f"cpu q8 len {n} ")
    one, _ = ops.attn_decode_q8(q[1:2], *(t[1:2] for t in cache), length=33)
    assert torch.equal(one, o[1:2])


def test_engine_int8_cpu():
    model = cases.tiny_llama("cpu", torch.float32)
    eng, cls = cases.check_engine_batch(model, torch.device("cpu"))
    st = _DecodeState(2, 2, 16, 64, 1, "cpu", torch.float32, kv_cache="int8")
    assert type(st.caches[0]) is cls is Int8KVCache
    with pytest.raises(ValueError, match="non-empty"):
        c = st.caches[0].row_view(0)
        c.update(torch.zeros(1, 2, 2, 64), torch.zeros(1, 2, 2, 64))
        c.update(torch.zeros(1, 2, 2, 64), torch.zeros(1, 2, 2, 64))


def test_engine_keyword():
    """bf16 (the default) builds today's KVCache and no int8 tensor; an
    int8 engine refuses a model outside the kernels' contract."""
    model = cases.tiny_llama("cpu", torch.float32)
    for kw in ({}, {"kv_cache": "bf16"}):
        eng = InferenceEngine(model, template="vanilla", **kw)
        st = eng._batch_state(2, 4, 4, greedy=True)
        assert all(type(c) is KVCache for c in st.caches)
        assert not any(t.dtype == torch.int8 for c in st.caches
                       for t in vars(c).values() if torch.is_tensor(t))
    with pytest.raises(ValueError, match="kv_cache"):
        InferenceEngine(model, template="vanilla", kv_cache="fp8")
    wide = cases.tiny_llama("cpu", torch.float32, heads=2, kv_heads=2)
    wide.cfg.head_dim_override = 96
    with pytest.raises(ValueError, match="head_dim"):
        InferenceEngine(wide, template="vanilla", kv_cache="int8")
    assert ops.kv_int8_supported(32, 8, 128)
    assert not ops.kv_int8_supported(32, 1, 128)
