"""ops.sample on the CPU: the RNG's known answers, the fp32 reference
against the independent fp64 oracle of tests/sample_cases.py, the drawn
distribution, and the engine's host sampling path (seed / top_k)."""

import pytest
import torch

import sample_cases as sc

from datatunerx_amd import ops
from datatunerx_amd.ops import reference as ref


def test_rng_known_answers():
    known = {(0, 0): 14819496, (5, 7): 8574860,
             (20261021, 0): 11964014, (20261021, 1): 10584903,
             (2 ** 63 - 1, 2 ** 31 - 1): 10451417}
    seed = torch.tensor([s for s, _ in known], dtype=torch.int64)
    off = torch.tensor([o for _, o in known], dtype=torch.int32)
    assert ref.sample_rng(seed, off).tolist() == list(known.values())
    # keyed by the row's own (seed, offset): not by its position or B
    assert int(ref.sample_rng(seed[3:4], off[3:4])) == 10584903


@pytest.mark.parametrize("idx", range(len(sc.CASES)))
def test_reference_against_fp64_oracle(idx):
    d = sc.build_case(idx)
    assert d["half_gap"] >= sc.MARGIN and d["margin"] >= sc.MARGIN
    assert d["last_share"] >= 2 * sc.MARGIN
    B = len(d["us"])
    logits = d["logits"].unsqueeze(0).expand(B, -1)
    out = ops.sample(logits, *sc.params(B, d["T"], d["top_p"], d["top_k"]),
                     u=torch.tensor(d["us"], dtype=torch.float32))
    assert out.dtype == torch.int64
    assert out.tolist() == d["expect"]
    # the oracle's own inverse CDF agrees with how the rows were built
    orc = d["oracle"]
    assert [orc.draw(d["members"], u) for u in d["us"]] == d["expect"]


def test_reference_greedy_topk1_and_rows_mix():
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(6, 520, generator=g) * 2).to(torch.bfloat16)
    x[1, [7, 300]] = 9.0
    x[2] = 0.25
    x[3, ::2] = float("-inf")
    want = x.float().argmax(-1)
    assert want[1] == 7 and want[2] == 0
    assert torch.equal(ops.sample(x, *sc.params(6, 0.0, 0.5, 3)), want)
    assert torch.equal(ops.sample(x, *sc.params(6, 1.3, 1.0, 1, seed=4)),
                       want)
    T = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    par = sc.params(6, 0.0, 0.9, 0, seed=8)
    mixed = ops.sample(x, T, *par[1:])
    assert torch.equal(mixed[0::2], want[0::2])
    # a row alone gives the row's token
    for i in range(6):
        one = ops.sample(x[i:i + 1], T[i:i + 1],
                         *[t[i:i + 1] for t in par[1:]])
        assert int(one) == int(mixed[i])
    with pytest.raises(ValueError, match="top_k"):
        ops.sample(x, T, par[1], par[2].long(), par[3], par[4])
    with pytest.raises(ValueError, match="seed"):
        ops.sample(x, T, par[1], par[2], par[3][:2], par[4])


@pytest.mark.parametrize("i", range(len(sc.DIST_SETTINGS)))
def test_reference_distribution(i):
    logits, T, top_p, top_k, members, pm = sc.dist_case(i)
    B = sc.DIST_ROWS
    rows = logits.unsqueeze(0).expand(B, -1)
    t, p, k, _, _ = sc.params(B, T, top_p, top_k)
    ar = torch.arange(B)
    for name, (seed, off) in {
            "seeds": (1234 + ar, torch.zeros(B, dtype=torch.int32)),
            "offsets": (torch.full((B,), 77, dtype=torch.int64),
                        ar.to(torch.int32))}.items():
        out = ops.sample(rows, t, p, k, seed, off)
        chi, bins = sc.chi_square(out, members, pm)
        limit = sc.chi_square_limit(bins)
        print(f"setting {i} {name}: chi2 {chi:.1f} limit {limit:.1f}")
        assert chi < limit, (name, chi, limit, bins)


# ------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def engine():
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import InferenceEngine
    m = LlamaForCausalLM(LlamaConfig.tiny(), lora=False,
                         dtype=torch.float32)
    m.init_random(seed=3)
    eng = InferenceEngine(m, template="vanilla", device=torch.device("cpu"))
    assert eng.device_sampling is False
    return eng


PROMPT = list(range(5, 25))


def test_engine_seed_reproduces(engine):
    a = engine.generate(PROMPT, 12, temperature=1.0, top_p=0.95, seed=11)
    b = engine.generate(PROMPT, 12, temperature=1.0, top_p=0.95, seed=11)
    c = engine.generate(PROMPT, 12, temperature=1.0, top_p=0.95, seed=12)
    assert a == b and len(a) > 0
    assert a != c
    # the batched host path draws the same tokens: token n at offset n
    rows = engine.generate_batch([PROMPT, PROMPT], 12, temperature=1.0,
                                 top_p=0.95, seed=[11, 12])
    assert rows == [a, c]
    text = engine.chat([{"role": "user", "content": "hi"}], 8, 1.0, 0.9,
                       seed=5)
    assert text == engine.chat([{"role": "user", "content": "hi"}], 8, 1.0,
                               0.9, seed=5)
    assert "".join(engine.chat_stream(
        [{"role": "user", "content": "hi"}], 8, 1.0, 0.9, seed=5)) == text


def test_engine_top_k_1_is_greedy(engine):
    greedy = engine.generate(PROMPT, 10)
    assert engine.generate(PROMPT, 10, temperature=1.5, top_k=1) == greedy
    assert engine.generate(PROMPT, 10, temperature=0.0, seed=3) == greedy


def test_engine_plain_requests_stay_on_the_host_sampler(engine,
                                                        monkeypatch):
    calls, op_calls = [], []
    real, real_op = engine._sample, ops.sample

    def spy(logits, temperature, top_p, *extra):
        calls.append(extra)
        return real(logits, temperature, top_p, *extra)

    def op_spy(*a, **kw):
        op_calls.append(1)
        return real_op(*a, **kw)

    monkeypatch.setattr(engine, "_sample", spy)
    monkeypatch.setattr(ops, "sample", op_spy)
    engine.generate(PROMPT, 4, temperature=0.9, top_p=0.9)
    assert len(calls) >= 1 and all(e == () for e in calls)
    assert not op_calls             # the torch-RNG sampler, untouched
    del calls[:]
    engine.generate(PROMPT, 4, temperature=0.9, top_p=0.9, seed=1)
    assert [e[2] for e in calls] == list(range(len(calls)))   # offsets
    assert len(op_calls) == len(calls) >= 1


def test_engine_mixed_batch_is_still_refused_on_cpu(engine):
    with pytest.raises(ValueError, match="share"):
        engine.chat_batch([
            {"messages": [{"role": "user", "content": "a"}],
             "max_tokens": 4, "temperature": 0.0},
            {"messages": [{"role": "user", "content": "b"}],
             "max_tokens": 4, "temperature": 0.9, "seed": 1}])
    # one setting, per-request seeds and top_k: fine
    reqs = [{"messages": [{"role": "user", "content": c}], "max_tokens": 5,
             "temperature": 0.9, "top_p": 0.9, "seed": s, "top_k": 20}
            for c, s in (("a", 1), ("b", 2))]
    outs = engine.chat_batch(reqs)
    assert outs == engine.chat_batch(reqs)
    assert outs[0] == engine.chat(reqs[0]["messages"], 5, 0.9, 0.9,
                                  top_k=20, seed=1)
