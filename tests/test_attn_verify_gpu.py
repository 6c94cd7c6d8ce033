"""Multi-token verify attention (attn_verify.hip): the kernel against fp64
causal attention over each row's live prefix, the binding contract and
attn_fwd's routing, and a graphed verify step of llama-mini against
single-token graphed steps."""

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
@pytest.mark.parametrize("T,Hq,Hkv", [
    (2, 1, 1), (16, 1, 1), (4, 8, 2), (5, 8, 2), (8, 8, 2), (3, 7, 1),
    (2, 16, 1)])
def test_verify_matches_fp64(T, Hq, Hkv, D):
    q, k, v, _ = kc.attn_inputs(3, Hq, Hkv, T, CAP, D, seed=T + Hq + D)
    v = (v.float() * 4).to(torch.bfloat16)       # K at 0.5, V at 2.0
    assert ops.attn_verify_supported(T, Hq, Hkv, D)
    assert ops._EXT.attn_verify_nsplit(CAP, Hkv, D) >= 3
    chunk = ops._EXT.attn_verify_chunk(CAP, Hkv, D)
    qg, kg, vg = q.to(DEV), k.to(DEV), v.to(DEV)
    report = {}

    def check(o, lse, b, n, tag):
        want = kc.attn_ref64(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n],
                             causal=True)
        kc.check_attn({"o": o, "lse": lse}, want, ("o",), tag=tag,
                      report=report)

    q1, k1, v1 = qg[1:2], kg[1:2], vg[1:2]
    straddle = [chunk + t for t in range(1, T)]  # early queries end at chunk
    for n in [T, T + 1, 31 + T, 32 + T, 33 + T, *straddle, chunk, CAP]:
        o, lse = ops.attn_verify(q1, k1, v1, len_dev=_i32([n]))
        assert o.shape == q1.shape and lse.shape == (1, Hq, T)
        check(o, lse, 1, n, f"len {n} ")
    # the B = 1 prefix view of a larger cache, no len_dev and no copy
    n = chunk + 33
    o, lse = ops.attn_verify(q1, k1[:, :n], v1[:, :n])
    check(o, lse, 1, n, f"prefix view {n} ")

    lens = [T, CAP, chunk + 1]
    o3, lse3 = ops.attn_verify(qg, kg, vg, len_dev=_i32(lens))
    for b, n in enumerate(lens):
        check(o3[b:b + 1], lse3[b:b + 1], b, n, f"batch row {b} ")
    # the same row alone: the split plan and so the bits ignore the batch
    o1, lse1 = ops.attn_verify(q1, k1, v1, len_dev=_i32([CAP]))
    assert torch.equal(o1, o3[1:2]) and torch.equal(lse1, lse3[1:2])
    # dead rows are neither read into the math nor multiplied by p = 0
    outs = []
    for fill in (0.0, float("nan")):
        kf, vf = kg.clone(), vg.clone()
        for b, n in enumerate(lens):
            kf[b, n:] = fill
            vf[b, n:] = fill
        outs.append(ops.attn_verify(qg, kf, vf, len_dev=_i32(lens)))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], o3)
    print(f"[attn_verify] T={T} Hq={Hq} Hkv={Hkv} D={D}: worst o err/bound "
          f"{max(report.values()):.4f}")


# --------------------------------------------------- 2. binding contract
def _args(T=2, Hq=2, Hkv=1, D=64, B=1, Skv=32):
    """All-zero inputs: whatever a missing check would let through reads
    and writes inside these allocations."""
    q = torch.zeros(B, T, Hq, D, dtype=torch.bfloat16, device=DEV)
    k = torch.zeros(B, Skv, Hkv, D, dtype=torch.bfloat16, device=DEV)
    return [q, k, k.clone()]


def test_binding_contract():
    b3 = _args(B=3)
    refused = [
        (_args(T=3, Hq=12), {}, "T \\* Hq / Hkv <= 32"),
        (_args(T=17, Hq=1), {}, "1 <= T <= 16"),
        (_args(D=96), {}, "D in \\{64, 128\\}"),
        (b3, {"len_dev": _i32([2, 2])}, r"\[1\] or \[B\]"),
        (b3, {"len_dev": torch.full((3,), 2, dtype=torch.int64, device=DEV)},
         "len_dev must be int32"),
    ]
    for args, kw, match in refused:
        with pytest.raises(RuntimeError, match=match):
            ops.attn_verify(*args, **kw)
    assert ops.attn_verify_supported(8, 32, 8, 128)
    assert not ops.attn_verify_supported(9, 32, 8, 128)
    assert not ops.attn_verify_supported(2, 6, 4, 64)
    # attn_fwd routes S > 1 with len_dev here, and refuses what cannot go
    q, k, v, _ = kc.attn_inputs(2, 8, 2, 3, 300, 64, seed=1)
    q, k, v, ld = q.to(DEV), k.to(DEV), v.to(DEV), _i32([7, 300])
    got, want = ops.attn_fwd(q, k, v, len_dev=ld), \
        ops.attn_verify(q, k, v, len_dev=ld)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    cpu = ops.attn_fwd(q.cpu(), k.cpu(), v.cpu(), len_dev=ld.cpu())
    kc.assert_abs(got[1], cpu[1], kc.LSE_ATOL, name="routed lse vs cpu")
    wide = _args(T=3, Hq=12, Skv=16)
    with pytest.raises(ValueError, match="attn_verify_supported"):
        ops.attn_fwd(*wide, len_dev=_i32([16]))


# ------------------------------------------------------- 3. in the model
def test_graphed_verify_logits(monkeypatch):
    """llama-mini with one kv head (G = 4, D = 64, 16 columns at T = 4):
    after a prefill, one graphed verify step on x0 x1 r2 r3 against
    single-token graphed steps on the same tokens; then, keeping 2 of the
    4 rows, a step on x2..x5 (the rows of r2 r3 lie stale behind the live
    length) and, keeping all 4, one on x6..x9. Logits with
    test_graphed_decode_logits's comparison, not tokens: two correct
    kernels may break a near-tie apart. The step's RoPE (per-row pos_dev,
    S > 1) is checked on its own first.

    The single-token steps run with the arithmetic of the verify step,
    so that what is compared is the multi-token step itself (slots,
    positions, per-query limits, stale rows): a two-row decoder carrying
    the sequence in both rows, since one row takes the VALU gemv and two
    to sixteen rows the skinny MFMA GEMMs whose row bits do not depend on
    the row count, and the GQA-shared MFMA decode kernel (forced, as in
    test_graphed_decode_logits: this capacity is outside its default
    routing). Against a one-row decoder the projections alone put every
    position near the bound on MI355X, the first step at 0.93, 0.91, 0.87
    and 1.08 of it, position 0 with the same visible rows included."""
    monkeypatch.setenv("DTX_GQA_DECODE", "1")
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import _GraphedDecoder
    from test_skinny_gpu import check
    T, P = 4, 37
    x = kc.attn_inputs(1, 4, 1, T, 1, 64, seed=5)[0]
    cos, sin = ops.rope_tables(64, 64)
    want, bud = kc.rope_ref64(x, cos, sin, P + torch.arange(T).view(1, T))
    got = ops.rope_fwd(x.to(DEV), cos.to(DEV), sin.to(DEV), 0, _i32([P]))
    kc.assert_elems(got, want, 2.0 ** -8 * bud, name="rope pos_dev S=4")

    cfg = LlamaConfig.mini(num_key_value_heads=1)
    with torch.device(DEV):
        model = LlamaForCausalLM(cfg, lora=False, dtype=torch.bfloat16)
    model.init_random(seed=3)
    model.eval()
    prompt = torch.tensor([list(range(4, 4 + P))], device=DEV)
    toks = [7, 9, 11, 13, 15, 17, 19, 21, 23, 25]
    one = _GraphedDecoder(model, cfg, DEV, 2, 64)
    ver = _GraphedDecoder(model, cfg, DEV, 1, 64, width=T)
    for gd in (one, ver):
        for i in range(gd.B):
            with torch.no_grad():
                model(prompt, pos0=0,
                      kv_caches=[c.row_view(i) for c in gd.caches])
        gd.set_state([P] * gd.B)

    def singles(seq):
        out = []
        for t in seq:
            one.step(torch.tensor([[t], [t]], device=DEV))
            out.append(one.logits[0, -1].float().cpu())
        return out

    single = singles(toks)
    one.set_state([P + 2] * 2)               # back to x0 x1, then r2 r3
    rejected = [101, 103]
    first = single[:2] + singles(rejected)
    steps = [(toks[:2] + rejected, first, 2), (toks[2:6], single[2:6], 4),
             (toks[6:10], single[6:10], 4)]
    for n, (inp, want, keep) in enumerate(steps):
        ver.step(torch.tensor([inp]))
        for i in range(T):
            check(ver.logits[0, i].float().cpu(), want[i],
                  f"verify step {n} logits {i}")
        assert ver.out.tolist() == ver.logits[0].argmax(-1).tolist()
        ver.advance(keep)
