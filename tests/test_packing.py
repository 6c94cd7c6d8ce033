"""Sequence packing on the CPU: the packer, the document map contract, the
fp32 reference ops with doc_start, the model equivalence (packed row ==
its documents run alone), stage=pt document maps, and the flag plumbing."""

import pytest
import torch

from datatunerx_amd import ops
from datatunerx_amd.data.dataset import (IGNORE_INDEX, ByteTokenizer,
                                         PackedDataset, SFTDataset,
                                         collate_packed, first_fit)
from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
from datatunerx_amd.ops import reference as ref

CUTOFF = 1024


def _lengths():
    return torch.randint(16, 513, (2000,),
                         generator=torch.Generator().manual_seed(0)).tolist()


def _dataset(lengths):
    """Example i holds i+3 in the first slot and a running counter after
    it, so a row can be cut back into its examples without the packer's
    help."""
    ex = []
    for i, n in enumerate(lengths):
        ids = [i + 3] + list(range(1, n))
        ex.append({"input_ids": ids, "labels": list(ids)})
    return SFTDataset(ex)


@pytest.fixture(scope="module")
def packed():
    lengths = _lengths()
    return lengths, PackedDataset.from_dataset(_dataset(lengths), CUTOFF)


def test_packer_every_example_once_unsplit(packed):
    lengths, p = packed
    seen = []
    for row in p.rows:
        ids, ds = row["input_ids"], row["doc_start"]
        assert len(ids) == len(ds) == len(row["labels"]) <= CUTOFF
        starts = sorted(set(ds))
        in_row = []
        for a, b in zip(starts, starts[1:] + [len(ids)]):
            i = ids[a] - 3
            assert b - a == lengths[i], "example split or merged"
            assert ids[a + 1:b] == list(range(1, lengths[i]))
            in_row.append(i)
        assert in_row == sorted(in_row), "dataset order within a row"
        seen += in_row
    assert sorted(seen) == list(range(len(lengths)))


def test_packer_doc_start_invariants_and_labels(packed):
    _, p = packed
    for row in p.rows:
        ds = torch.tensor(row["doc_start"])
        s = torch.arange(len(ds))
        assert bool((ds[1:] >= ds[:-1]).all())
        assert bool((ds <= s).all())
        assert bool((ds[ds] == ds).all())
        labels = torch.tensor(row["labels"])
        first = torch.unique(ds)
        assert bool((labels[first] == IGNORE_INDEX).all())
        other = torch.ones(len(ds), dtype=torch.bool)
        other[first] = False
        assert bool((labels[other] == torch.tensor(row["input_ids"])[other])
                    .all()), "only first-token labels change"


def test_packer_deterministic_and_seeded(packed):
    lengths, p = packed
    again = PackedDataset.from_dataset(_dataset(lengths), CUTOFF)
    assert again.rows == p.rows
    other = PackedDataset.from_dataset(_dataset(lengths), CUTOFF, seed=1)
    assert other.rows != p.rows


def test_packer_fill(packed):
    lengths, p = packed
    fill = sum(lengths) / (len(p) * CUTOFF)
    assert fill >= 0.97, fill


def test_first_fit_is_first_fit():
    """The tree descent picks the LOWEST bin with room (checked against
    the quadratic definition), and 50k examples pack in seconds."""
    g = torch.Generator().manual_seed(1)
    lengths = torch.randint(1, 65, (300,), generator=g).tolist()
    free, want = [], []
    for i, n in enumerate(lengths):
        for b, f in enumerate(free):
            if f >= n:
                break
        else:
            b = len(free)
            free.append(64)
            want.append([])
        free[b] -= n
        want[b].append(i)
    assert first_fit(lengths, 64) == want
    big = torch.randint(16, 513, (50000,), generator=g).tolist()
    bins = first_fit(big, CUTOFF)
    assert sum(len(b) for b in bins) == 50000
    with pytest.raises(ValueError):
        first_fit([5, 70], 64)


def test_collate_packed_pads_to_cutoff(packed):
    _, p = packed
    mb = collate_packed([p[0], p[1]], pad_token_id=0, cutoff_len=CUTOFF)
    assert mb["input_ids"].shape == mb["labels"].shape == (2, CUTOFF)
    assert mb["doc_start"].shape == (2, CUTOFF)
    assert mb["doc_start"].dtype == torch.int32
    for i in range(2):
        n = len(p[i]["input_ids"])
        assert bool((mb["doc_start"][i, n:] == n).all())
        assert bool((mb["labels"][i, n:] == IGNORE_INDEX).all())
        assert mb["doc_start"][i, :n].tolist() == p[i]["doc_start"]


# ------------------------------------------------------------ reference ops
def _doc_start(lens, S):
    ds, a = [], 0
    for n in lens:
        ds += [a] * n
        a += n
    ds += [a] * (S - a)
    return torch.tensor([ds], dtype=torch.int32)


def test_doc_end_from_start():
    ds = _doc_start([5, 17, 9], 32)
    de = ops.doc_end_from_start(ds)
    want = [5] * 5 + [22] * 17 + [31] * 9 + [32]
    assert de.dtype == torch.int32 and de.tolist() == [want]


def test_reference_rope_restarts_per_document():
    torch.manual_seed(0)
    lens, S, H, D = [5, 17, 9], 32, 2, 16
    cos, sin = ref.rope_tables(64, D)
    x = torch.randn(1, S, H, D)
    ds = _doc_start(lens, S)
    y = ops.rope_fwd(x, cos, sin, 2, doc_start=ds)
    dx = ops.rope_bwd(x, cos, sin, 2, doc_start=ds)
    a = 0
    for n in lens + [1]:
        assert torch.equal(y[:, a:a + n],
                           ref.rope_fwd(x[:, a:a + n], cos, sin, 2))
        assert torch.equal(dx[:, a:a + n],
                           ref.rope_bwd(x[:, a:a + n], cos, sin, 2))
        a += n


def test_reference_attention_is_per_document():
    torch.manual_seed(0)
    lens, S, Hq, Hkv, D = [5, 17, 9], 32, 4, 2, 16
    q, do = torch.randn(1, S, Hq, D), torch.randn(1, S, Hq, D)
    k, v = torch.randn(1, S, Hkv, D), torch.randn(1, S, Hkv, D)
    ds = _doc_start(lens, S)
    o, lse = ops.attn_fwd(q, k, v, True, doc_start=ds)
    dq, dk, dv = ops.attn_bwd(q, k, v, o, do, lse, True, doc_start=ds)
    a = 0
    for n in lens + [1]:
        sl = slice(a, a + n)
        o1, lse1 = ref.attn_fwd(q[:, sl], k[:, sl], v[:, sl], True)
        g1 = ref.attn_bwd(q[:, sl], k[:, sl], v[:, sl], o1, do[:, sl],
                          lse1, True)
        assert torch.allclose(o[:, sl], o1, atol=1e-6)
        assert torch.allclose(lse[:, :, sl], lse1, atol=1e-6)
        for got, want in zip((dq, dk, dv), g1):
            assert torch.allclose(got[:, sl], want, atol=1e-6)
        a += n


def test_misuse_raises():
    q = torch.randn(1, 8, 2, 16)
    kv = torch.randn(1, 12, 2, 16)
    ds = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.attn_fwd(q, q, q, causal=False, doc_start=ds)
    with pytest.raises(ValueError):
        ops.attn_fwd(q, kv, kv, causal=True, doc_start=ds)
    with pytest.raises(ValueError):
        ops.attn_fwd(q[:, :1], q[:, :1], q[:, :1], True,
                     doc_start=ds[:, :1])
    with pytest.raises(ValueError):
        ops.attn_fwd(q, q, q, True, len_dev=torch.tensor([8]),
                     doc_start=ds)
    cos, sin = ref.rope_tables(16, 16)
    with pytest.raises(ValueError):
        ops.rope_fwd(q, cos, sin, 0, pos_dev=torch.tensor([1]),
                     doc_start=ds)
    with pytest.raises(ValueError):
        ops.attn_fwd(q, q, q, True, doc_start=ds.long())


# ------------------------------------------------------- model equivalence
@pytest.mark.parametrize("ckpt", [False, True])
def test_packed_row_equals_documents_alone(ckpt):
    lens, S = [5, 17, 9], 32
    cfg = LlamaConfig.tiny(gradient_checkpointing=ckpt)
    model = LlamaForCausalLM(cfg, lora=True, dtype=torch.float32)
    model.init_random()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "lora_B" in n:       # zero-init B would zero every A grad
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    model.train()
    docs = [torch.randint(3, cfg.vocab_size, (n,), generator=g)
            for n in lens]
    ids = torch.zeros(1, S, dtype=torch.long)
    ids[0, :sum(lens)] = torch.cat(docs)
    labels = torch.full((1, S), IGNORE_INDEX, dtype=torch.long)
    labels[0, :sum(lens)] = torch.cat(docs)
    ds = _doc_start(lens, S)
    labels[0, torch.unique(ds).long()] = IGNORE_INDEX

    names = [n for n, _ in model.trainable_parameters()]
    params = [p for _, p in model.trainable_parameters()]
    assert any("lora_A" in n for n in names)

    logits_p = model(ids, doc_start=ds)
    loss_p = model(ids, labels=labels, doc_start=ds)
    grads_p = torch.autograd.grad(loss_p, params)

    a, total, n_tok = 0, 0.0, 0
    for d in docs:
        n = len(d)
        logits_1 = model(d[None])
        assert torch.allclose(logits_p[0, a:a + n], logits_1[0],
                              atol=1e-5, rtol=0), (a, n)
        total = total + model(d[None], labels=d[None]) * (n - 1)
        n_tok += n - 1
        a += n
    loss_1 = total / n_tok
    assert abs(float(loss_p.detach()) - float(loss_1.detach())) < 1e-5
    grads_1 = torch.autograd.grad(loss_1, params)
    for name, gp, g1 in zip(names, grads_p, grads_1):
        assert torch.allclose(gp, g1, atol=1e-5, rtol=0), name
    assert any(float(gp.abs().max()) > 1e-4 for gp in grads_p)


def test_gpt2_restarts_positions_per_document():
    from datatunerx_amd.models import GPT2Config, GPT2ForCausalLM
    lens, S = [5, 17, 9], 32
    model = GPT2ForCausalLM(GPT2Config.tiny(), dtype=torch.float32)
    model.init_random()
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(3, 200, (1, S), generator=g)
    out = model(ids, doc_start=_doc_start(lens, S))
    a = 0
    for n in lens:
        one = model(ids[:, a:a + n])
        assert torch.allclose(out[:, a:a + n], one, atol=1e-5, rtol=0)
        a += n


# ---------------------------------------------------------------- stage=pt
def test_pt_doc_start_restarts_after_eos_and_at_block_start():
    tok = ByteTokenizer()
    rows = [{"instruction": "abcdefgh", "response": ""},
            {"instruction": "ijklmnopqrst", "response": ""},
            {"instruction": "uvw", "response": ""},
            {"instruction": "xyzxyzxyzxyz", "response": ""}]
    plain = SFTDataset.from_rows_pt(rows, tok, cutoff_len=16)
    ds = SFTDataset.from_rows_pt(rows, tok, cutoff_len=16, packing=True)
    assert len(ds) == len(plain) == 2
    for ex, ex0 in zip(ds.examples, plain.examples):
        ids = ex["input_ids"]
        assert ids == ex0["input_ids"], "blocks are built as before"
        assert "doc_start" not in ex0
        want, start = [], 0
        for j, t in enumerate(ids):
            want.append(start)
            if t == tok.eos_token_id:
                start = j + 1
        assert ex["doc_start"] == want
        for j, lab in enumerate(ex["labels"]):
            assert lab == (IGNORE_INDEX if j in set(want) else ids[j])
    # block 0: 8 bytes + eos, then a document cut by the block edge;
    # block 1 starts mid-document and so opens a document at 0
    assert ds[0]["doc_start"] == [0] * 9 + [9] * 7
    assert ds[1]["doc_start"] == [0] * 6 + [6] * 4 + [10] * 6
    # such a dataset is already rows: the packer takes it as is
    p = PackedDataset.from_dataset(ds, 16)
    assert p.rows == ds.examples


# ---------------------------------------------------------------- plumbing
def test_args_packing_flag():
    from datatunerx_amd.train.args import get_train_args
    assert get_train_args([])[1].packing is False
    assert get_train_args(["--packing"])[1].packing is True
    assert get_train_args(["--packing", "true"])[1].packing is True
    assert get_train_args(["--packing", "--stage", "pt"])[1].stage == "pt"
    with pytest.raises(ValueError):
        get_train_args(["--stage", "dpo", "--packing"])


def test_dpo_trainer_refuses_packing():
    from datatunerx_amd.data.preference import PreferenceDataset
    from datatunerx_amd.train.trainer import DPOTrainer, TrainerConfig
    cfg = LlamaConfig.tiny()
    model = LlamaForCausalLM(cfg, lora=True, dtype=torch.float32)
    ds = PreferenceDataset.synthetic(4, 16, cfg.vocab_size)
    with pytest.raises(ValueError):
        DPOTrainer(model, ds, TrainerConfig(packing=True))


def test_build_args_and_validation():
    from datatunerx_amd.api.controllers import FinetuneController
    from datatunerx_amd.api.types import Finetune, Hyperparameter
    from datatunerx_amd.api.validation import ValidationError
    from datatunerx_amd.api.validation import validate_ as validate
    ctl = FinetuneController.__new__(FinetuneController)
    ctl.cfg = type("Cfg", (), {"default_model": "llama-tiny",
                               "metrics_export_address": "",
                               "storage_path": ""})()
    ft = Finetune(name="f", spec={"llm": "llama-tiny"})
    a = ctl.build_args(ft, {"packing": True}, None, "out")
    assert "--packing" in a
    assert "--packing" not in ctl.build_args(ft, {}, None, "out")
    assert "--packing" not in ctl.build_args(ft, {"packing": False}, None,
                                             "out")

    def hp(params):
        return Hyperparameter(name="h", spec={"parameters": params})
    validate(hp({"packing": True, "stage": "sft"}))
    validate(hp({"packing": False, "stage": "dpo"}))
    with pytest.raises(ValidationError):
        validate(hp({"packing": "yes"}))
    with pytest.raises(ValidationError):
        validate(hp({"packing": 1}))
    with pytest.raises(ValidationError):
        validate(hp({"packing": True, "stage": "dpo"}))


def test_trainer_step_count_follows_packed_rows(tmp_path):
    from datatunerx_amd.train.trainer import SFTTrainer, TrainerConfig
    cfg = LlamaConfig.tiny()
    model = LlamaForCausalLM(cfg, lora=True, dtype=torch.float32)
    model.init_random()
    g = torch.Generator().manual_seed(0)
    ex = []
    for n in torch.randint(4, 33, (40,), generator=g).tolist():
        ids = torch.randint(3, cfg.vocab_size, (n,), generator=g).tolist()
        ex.append({"input_ids": ids, "labels": list(ids)})
    ds = SFTDataset(ex)
    tcfg = TrainerConfig(output_dir=str(tmp_path), micro_batch_size=2,
                         packing=True, cutoff_len=64, logging_steps=0)
    tr = SFTTrainer(model, ds, tcfg, device=torch.device("cpu"))
    rows = len(PackedDataset.from_dataset(ds, 64, seed=tcfg.seed))
    assert rows < len(ds) // 2
    assert tr.total_steps == max(1, rows // 2)
    mb = next(iter(tr.train_loader))
    assert mb["input_ids"].shape == (2, 64) and "doc_start" in mb
    loss = tr.train_step([mb])
    assert loss == loss
