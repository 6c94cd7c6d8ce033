"""Shared by test_kv_int8_gpu.py and test_kv_int8_ref.py: the checks of
the int8 KV cache's quantizer against its definition, and the engine
cases. A plain helper module, imported by name like kernel_check."""

import torch

import kernel_check as kc

SENTINEL8, SENTINEL_S = 77, -5.0


def empty_cache(Bc, max_s, Hkv, D, device):
    """A cache pre-filled with sentinels: (k8, v8, ks, vs)."""
    k8 = torch.full((Bc, max_s, Hkv, D), SENTINEL8, dtype=torch.int8,
                    device=device)
    ks = torch.full((Bc, Hkv, max_s), SENTINEL_S, dtype=torch.float32,
                    device=device)
    return k8, k8.clone(), ks, ks.clone()


def kv_rows(B, S, Hkv, D, seed, zero_row=True):
    """bf16 k, v [B,S,Hkv,D] ~ N(0, 1); row (0, 0, 0) of k all zero."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.randn(B, S, Hkv, D, generator=gen).to(torch.bfloat16)
    v = torch.randn(B, S, Hkv, D, generator=gen).to(torch.bfloat16)
    if zero_row:
        k[0, 0, 0] = 0
    return k, v


def check_rows(x, q, s, tag):
    """x bf16 [N,Hkv,D], q int8 [N,Hkv,D], s f32 [N,Hkv]: the quantizer's
    definition in fp64. scale within 2 fp32 ulp of max(absmax, 1e-8)/127,
    |q| <= 127, |q s - x| <= s/2 (1 + 2^-20), the absmax element at +-127."""
    xd, qd, sd = x.cpu().to(kc.F64), q.cpu().to(kc.F64), s.cpu().to(kc.F64)
    absmax = xd.abs().amax(dim=-1)
    want = absmax.clamp(min=1e-8) / 127.0
    r_s = ((sd - want).abs() / (2 * kc.ulp32(want))).max()
    r_q = ((qd * sd[..., None] - xd).abs()
           / (sd[..., None] / 2 * (1 + 2.0 ** -20))).max()
    print(f"[kv_int8] {tag}: scale err/bound {float(r_s):.4f}, "
          f"element err/bound {float(r_q):.8f}")
    assert r_s <= 1.0, f"{tag}: scale at {float(r_s):.3f} of 2 ulp"
    assert qd.abs().max() <= 127
    assert r_q <= 1.0, f"{tag}: element at {float(r_q):.8f} of its bound"
    top = qd.abs().gather(-1, xd.abs().argmax(dim=-1, keepdim=True))[..., 0]
    assert torch.equal(top[absmax > 0],
                       torch.full_like(top[absmax > 0], 127.0)), tag
    assert torch.equal(qd[absmax == 0], torch.zeros_like(qd[absmax == 0]))


def check_append(cache, k, v, slots, tag):
    """The cache rows at the flat `slots` (one per (b, s) row of k, v, in
    order) hold k, v quantized; every other slot keeps the sentinel."""
    k8, v8, ks, vs = (t.cpu() for t in cache)
    Bc, max_s, Hkv, D = k8.shape
    slots = torch.as_tensor(slots)
    for x, x8, xs, name in ((k, k8, ks, "k"), (v, v8, vs, "v")):
        flat8 = x8.view(-1, Hkv, D)
        flats = xs.permute(0, 2, 1).reshape(-1, Hkv)
        check_rows(x.reshape(-1, Hkv, D), flat8[slots], flats[slots],
                   f"{tag} {name}")
        rest = torch.ones(Bc * max_s, dtype=torch.bool)
        rest[slots] = False
        assert (flat8[rest] == SENTINEL8).all(), f"{tag}: {name}8 overwritten"
        assert (flats[rest] == SENTINEL_S).all(), f"{tag}: {name}s overwritten"


def tiny_llama(device, dtype, heads=4, kv_heads=2):
    """The model of test_batched_decode_matches_sequential_gpu."""
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=512, hidden_size=64 * heads,
                      intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=heads,
                      num_key_value_heads=kv_heads,
                      max_position_embeddings=256)
    with torch.device(device):
        model = LlamaForCausalLM(cfg, lora=False, dtype=dtype)
    model.init_random()
    return model.eval()


def check_engine_batch(model, device, **kw):
    """generate_batch over 3 ragged prompts == per-request generate."""
    from datatunerx_amd.serve.engine import InferenceEngine, Int8KVCache
    eng = InferenceEngine(model, template="vanilla", device=device,
                          kv_cache="int8", **kw)
    prompts = [eng.tok.encode(t, add_special_tokens=True)
               for t in ("hello world",
                         "a much longer prompt with many words in", "x")]
    batched = eng.generate_batch(prompts, max_new_tokens=12)
    seq = [eng.generate(p, max_new_tokens=12) for p in prompts]
    assert batched == seq
    assert all(len(o) > 0 for o in seq)
    return eng, Int8KVCache
