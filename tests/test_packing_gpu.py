"""Sequence packing on the GPU: the DOCS instantiations of the attention
forward / dq / dkdv kernels and of the RoPE kernel against the fp32
reference with doc_start, plus bit-reproducibility, isolation between
documents, agreement with the plain causal kernel per document, and the
model / trainer plumbing. Metric and bounds are those of
tests/test_ops_gpu.py (max error relative to the reference's max); the
comparisons with a reference also get the row-wise bound of
tests/kernel_check.py against fp64."""

import math

import pytest
import torch

import kernel_check as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    from datatunerx_amd.ops import reference as ref
    DEV = torch.device("cuda:0")
    assert ops.have_ext(), "HIP extension must be built for GPU tests"


def assert_close(got, want, rtol=2e-2, name=""):
    got, want = got.float(), want.float()
    denom = want.abs().max().clamp(min=1e-3)
    err = (got - want).abs().max() / denom
    assert err < rtol, f"{name}: rel err {err:.4f} (max {denom:.3f})"


# (B, Hq, Hkv, S, D, document lengths per batch row)
CASES = {
    "one_doc_sub_tile": (1, 2, 2, 24, 128, [[24]]),
    "len1_and_wave_edges": (1, 2, 2, 200, 128, [[1, 31, 32, 33, 64, 39]]),
    "second_stage_qblock_edge": (1, 2, 2, 320, 128, [[129, 127, 64]]),
    "span_qblocks_gqa4": (1, 4, 1, 600, 128, [[300, 300]]),
    "d64_ragged_per_row": (2, 2, 2, 100, 64, [[60, 40], [7, 93]]),
    "dead_subdiagonal_tiles": (1, 2, 2, 520, 128, [[8] * 65]),
}
ISOLATION = ["len1_and_wave_edges", "second_stage_qblock_edge"]


def doc_start_of(lens_rows, S):
    rows = []
    for lens in lens_rows:
        assert sum(lens) == S
        row, a = [], 0
        for n in lens:
            row += [a] * n
            a += n
        rows.append(row)
    return torch.tensor(rows, dtype=torch.int32)


def run_packed(t):
    """Forward + backward of the DOCS kernels on the tensors in t."""
    scale = 1.0 / math.sqrt(t["q"].shape[-1])
    o, lse = ops.attn_fwd(t["q"], t["k"], t["v"], True, scale,
                          doc_start=t["ds"])
    dq, dk, dv = ops.attn_bwd(t["q"], t["k"], t["v"], o, t["do"], lse,
                              True, scale, doc_start=t["ds"])
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


_CACHE = {}


def case(name):
    """Inputs, GPU results, the fp32 reference and the fp64 reference (with
    its budgets) of a case, computed once and shared (read-only) by every
    test that needs them."""
    if name in _CACHE:
        return _CACHE[name]
    B, Hq, Hkv, S, D, lens = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(
        torch.bfloat16).to(DEV)
    t = {"q": mk(B, S, Hq, D), "k": mk(B, S, Hkv, D), "v": mk(B, S, Hkv, D),
         "do": mk(B, S, Hq, D), "ds": doc_start_of(lens, S).to(DEV)}
    got = run_packed(t)
    c = {k: v.cpu() for k, v in t.items()}
    o_r, lse_r = ref.attn_fwd(c["q"].float(), c["k"].float(),
                              c["v"].float(), True, None, c["ds"])
    dq_r, dk_r, dv_r = ref.attn_bwd(c["q"].float(), c["k"].float(),
                                    c["v"].float(), o_r, c["do"].float(),
                                    lse_r, True, None, c["ds"])
    want = {"o": o_r, "lse": lse_r, "dq": dq_r, "dk": dk_r, "dv": dv_r}
    want["f64"] = kc.attn_ref64(c["q"], c["k"], c["v"], c["do"], True,
                                doc_start=c["ds"])
    _CACHE[name] = (t, got, want)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_attn_docs_vs_reference(name):
    _, got, want = case(name)
    assert_close(got["o"].cpu(), want["o"], rtol=2e-2, name="o")
    assert_close(got["lse"].cpu(), want["lse"], rtol=1e-2, name="lse")
    for k in ("dq", "dk", "dv"):
        assert_close(got[k].cpu(), want[k], rtol=3e-2, name=k)
    kc.check_attn(got, want["f64"], tag=name + " ")


@pytest.mark.parametrize("name", list(CASES))
def test_attn_docs_backward_is_bit_reproducible(name):
    t, got, _ = case(name)
    scale = 1.0 / math.sqrt(t["q"].shape[-1])
    again = ops.attn_bwd(t["q"], t["k"], t["v"], got["o"], t["do"],
                         got["lse"], True, scale, doc_start=t["ds"])
    for k, a in zip(("dq", "dk", "dv"), again):
        assert torch.equal(a, got[k]), k


@pytest.mark.parametrize("name", ISOLATION)
def test_attn_docs_isolation(name):
    """Fresh values in one middle document leave every other document's
    outputs bit-equal: no leak across a boundary, no wrongly skipped
    tile, even inside the tolerance."""
    t, got, _ = case(name)
    lens = CASES[name][5][0]
    mid = len(lens) // 2
    a = sum(lens[:mid])
    b = a + lens[mid]
    g = torch.Generator().manual_seed(99)
    t2 = dict(t)
    for k in ("q", "k", "v", "do"):
        x = t[k].clone()
        x[:, a:b] = (torch.randn(x[:, a:b].shape, generator=g) * 0.5).to(
            torch.bfloat16).to(DEV)
        t2[k] = x
    got2 = run_packed(t2)
    S = t["q"].shape[1]
    keep = torch.ones(S, dtype=torch.bool)
    keep[a:b] = False
    keep = keep.to(DEV)
    for k in ("o", "dq", "dk", "dv"):
        assert torch.equal(got2[k][:, keep], got[k][:, keep]), k
        assert not torch.equal(got2[k][:, a:b], got[k][:, a:b]), k
    assert torch.equal(got2["lse"][:, :, keep], got["lse"][:, :, keep])


@pytest.mark.parametrize("name", list(CASES))
def test_attn_docs_vs_plain_kernel_per_document(name):
    t, got, _ = case(name)
    B, Hq, Hkv, S, D, lens_rows = CASES[name]
    scale = 1.0 / math.sqrt(D)
    for bi, lens in enumerate(lens_rows):
        a = 0
        for n in lens:
            sl = slice(a, a + n)
            q, k, v, do = (t[x][bi:bi + 1, sl].contiguous()
                           for x in ("q", "k", "v", "do"))
            o, lse = ops.attn_fwd(q, k, v, True, scale)
            dq, dk, dv = ops.attn_bwd(q, k, v, o, do, lse, True, scale)
            tag = f"row {bi} doc at {a} len {n}"
            assert_close(got["o"][bi:bi + 1, sl], o, rtol=3e-2,
                         name="o " + tag)
            assert_close(got["lse"][bi:bi + 1, :, sl], lse, rtol=3e-2,
                         name="lse " + tag)
            for key, x in (("dq", dq), ("dk", dk), ("dv", dv)):
                assert_close(got[key][bi:bi + 1, sl], x, rtol=3e-2,
                             name=key + " " + tag)
            a += n


def test_attn_docs_misuse_is_an_error():
    q = torch.zeros(1, 8, 2, 64, dtype=torch.bfloat16, device=DEV)
    kv = torch.zeros(1, 16, 2, 64, dtype=torch.bfloat16, device=DEV)
    ds = torch.zeros(1, 8, dtype=torch.int32, device=DEV)
    from datatunerx_amd.ops import _dtx_hip
    with pytest.raises(RuntimeError):
        _dtx_hip.attn_fwd(q, q, q, False, 0.125, ds)
    with pytest.raises(RuntimeError):
        _dtx_hip.attn_fwd(q, kv, kv, True, 0.125, ds)
    with pytest.raises(RuntimeError):
        _dtx_hip.attn_fwd(q, q, q, True, 0.125, ds[:, :4].contiguous())
    with pytest.raises(RuntimeError):
        _dtx_hip.attn_fwd(q, q, q, True, 0.125, ds.long())
    with pytest.raises(RuntimeError):
        _dtx_hip.attn_fwd(q, q, q, True, 0.125, ds.cpu())


@pytest.mark.parametrize("D", [64, 128])
def test_rope_docs(D):
    B, S, H = 2, 100, 4
    g = torch.Generator().manual_seed(D)
    cos, sin = ref.rope_tables(256, D)
    x = torch.randn(B, S, H, D, generator=g).to(torch.bfloat16)
    dy = torch.randn(B, S, H, D, generator=g).to(torch.bfloat16)
    ds = doc_start_of([[60, 40], [7, 93]], S)
    y = ops.rope_fwd(x.to(DEV), cos.to(DEV), sin.to(DEV), pos0=3,
                     doc_start=ds.to(DEV))
    dx = ops.rope_bwd(dy.to(DEV), cos.to(DEV), sin.to(DEV), pos0=3,
                      doc_start=ds.to(DEV))
    assert_close(y.cpu(), ref.rope_fwd(x.float(), cos, sin, 3, ds),
                 rtol=2e-2, name="rope fwd")
    assert_close(dx.cpu(), ref.rope_bwd(dy.float(), cos, sin, 3, ds),
                 rtol=2e-2, name="rope bwd")
    pos = 3 + torch.arange(S).view(1, S) - ds.long()
    for got, src, bwd in ((y, x, False), (dx, dy, True)):
        w64, bud = kc.rope_ref64(src, cos, sin, pos, backward=bwd)
        kc.assert_elems(got, w64, 2.0 ** -8 * bud, name="rope docs")


def _mini(seed=0):
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig.mini()
    with torch.device(DEV):
        model = LlamaForCausalLM(cfg, lora=True, dtype=torch.bfloat16)
    model.init_random(seed=seed)
    return cfg, model


def test_model_packed_loss_matches_unpacked():
    cfg, model = _mini()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "lora_B" in n:
                p.copy_((torch.randn(p.shape, generator=g) * 0.05)
                        .to(p.dtype))
    model.eval()
    lens, S = [40, 100, 60], 256
    docs = [torch.randint(3, cfg.vocab_size, (n,), generator=g)
            for n in lens]
    ids = torch.zeros(1, S, dtype=torch.long)
    labels = torch.full((1, S), -100, dtype=torch.long)
    ids[0, :sum(lens)] = torch.cat(docs)
    labels[0, :sum(lens)] = torch.cat(docs)
    ds = doc_start_of([lens + [S - sum(lens)]], S)
    labels[0, torch.unique(ds).long()] = -100
    with torch.no_grad():
        packed = float(model(ids.to(DEV), labels=labels.to(DEV),
                             doc_start=ds.to(DEV)))
        total = 0.0
        for d in docs:
            d = d[None].to(DEV)
            total += float(model(d, labels=d)) * (d.shape[1] - 1)
    alone = total / (sum(lens) - len(lens))
    print(f"packed {packed:.5f} unpacked {alone:.5f}")
    assert math.isfinite(packed)
    assert abs(packed - alone) / alone < 3e-2


def test_trainer_step_with_packing(tmp_path):
    from datatunerx_amd.data.dataset import SFTDataset
    from datatunerx_amd.train.trainer import SFTTrainer, TrainerConfig
    cfg, model = _mini()
    g = torch.Generator().manual_seed(6)
    ex = []
    for n in torch.randint(16, 129, (24,), generator=g).tolist():
        ids = torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist()
        ex.append({"input_ids": ids, "labels": list(ids)})
    tcfg = TrainerConfig(output_dir=str(tmp_path), micro_batch_size=2,
                         max_steps=1, packing=True, cutoff_len=256,
                         logging_steps=0)
    tr = SFTTrainer(model, SFTDataset(ex), tcfg, device=DEV)
    model.train()
    mb = next(iter(tr.train_loader))
    assert mb["input_ids"].shape == (2, 256)
    assert mb["doc_start"].dtype == torch.int32
    loss = tr._micro_loss(mb)
    loss.backward()
    assert math.isfinite(float(loss.detach()))
    # the optimizer's hooks fold every gradient into its flat fp32 buffer
    named = dict(zip((n for n, _ in tr.opt.named), tr.opt.offsets))
    for n, p in tr.opt.named:
        gr = tr.opt.grad[named[n]:named[n] + p.numel()]
        assert bool(torch.isfinite(gr).all()), n
        if "lora_B" in n:           # B starts at zero, so dA is zero
            assert float(gr.abs().max()) > 0.0, n
    tr.opt.step(1e-4)
    assert any(float(p.detach().abs().max()) > 0 for n, p in tr.opt.named
               if "lora_B" in n)
