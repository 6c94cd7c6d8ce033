"""Speculative decoding on the CPU: the prompt-lookup drafts, the engine's
verify loop on the tiny fp32 model against plain greedy decoding, and the
refusals of the switch."""

import pytest
import torch

from datatunerx_amd.serve.engine import InferenceEngine
from datatunerx_amd.serve.lookup import prompt_lookup

CPU = torch.device("cpu")


@pytest.mark.parametrize("ids,k,want", [
    # the 3-gram (1 2 3) wins over the later 1-gram match of 3 at index 6
    ([1, 2, 3, 7, 8, 9, 3, 5, 1, 2, 3], 3, [7, 8, 9]),
    # the latest occurrence of (1 2) wins: 5 follows it, not 4
    ([1, 2, 4, 1, 2, 5, 1, 2], 1, [5]),
    # no longer n-gram repeats: down to the last token alone
    ([6, 9, 1, 6, 2, 9], 2, [1, 6]),
    ([1, 2, 3, 4], 4, []),                       # nothing repeats
    ([5], 4, []),
    ([7, 8, 9, 7, 8], 4, [9, 7, 8]),             # cut at the end of the ids
    ([4, 4, 4, 4], 2, [4]),                      # overlap: one follower
])
def test_prompt_lookup(ids, k, want):
    assert prompt_lookup(ids, k) == want


# Seed 16 of the tiny model, picked among seeds 1..20 on the CPU: plain
# greedy decoding has no near-tie over the tokens compared here (the
# smallest margin between the two best logits is 0.0054 after PROMPT and
# 0.0254 after LONG; the test prints both and asserts them above 1e-3, far
# more than fp32 summation order moves a logit of this model), so the
# K + 1-token verify pass and the one-token pass must pick the same tokens.
SEED, N_NEW = 16, 40
PROMPT = [5, 6, 7, 8, 9, 10, 11, 12] * 3 + [5, 6, 7]
LONG = [5, 6, 7, 8, 9, 10, 11, 12] * 30             # 16 positions left


@pytest.fixture(scope="module")
def model():
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    m = LlamaForCausalLM(LlamaConfig.tiny(), lora=False, dtype=torch.float32)
    m.init_random(seed=SEED)
    return m.eval()


def test_engine_matches_greedy(model):
    plain = InferenceEngine(model, template="vanilla", device=CPU)
    spec = InferenceEngine(model, template="vanilla", device=CPU,
                           speculative=4)
    want = plain.generate(PROMPT, N_NEW)
    # the context ends before the budget: the last steps run one token at
    # a time and stop where plain decoding stops
    want_long = plain.generate(LONG, 30)
    for prompt, new in ((PROMPT, want), (LONG, want_long)):
        with torch.no_grad():
            top = model(torch.tensor([prompt + new]))[
                0, len(prompt) - 1:-1].topk(2).values
        margin = float((top[:, 0] - top[:, 1]).min())
        print(f"smallest greedy margin {margin:.4f}")
        assert margin > 1e-3
    assert spec.generate(PROMPT, N_NEW) == want and len(want) == N_NEW
    st = dict(spec.spec_stats)
    print(f"spec_stats {st}")
    # tokens: what the verify steps accepted. The first token comes from
    # the prefill; the last step may accept past the budget
    assert 0 < st["verify_steps"] < N_NEW - 1 <= st["tokens"]
    assert spec.generate(PROMPT, 7) == want[:7]     # a budget ends mid-step
    assert spec.generate(LONG, 30) == want_long and len(want_long) == 16
    # a sampled request takes the plain path
    before = dict(spec.spec_stats)
    kw = dict(temperature=0.9, top_p=0.95, seed=7)
    assert spec.generate(PROMPT, 12, **kw) == plain.generate(PROMPT, 12, **kw)
    assert spec.spec_stats == before


def test_server_speculates(model, monkeypatch):
    """The fronts as main() builds them: with the batching front every
    chat request runs on its engine, so that engine carries the switch
    and /health counts its verify steps; the pool, left with /score,
    carries none. Without the front the pool's engines carry it."""
    import json
    import threading
    import urllib.request
    from http.server import ThreadingHTTPServer

    from datatunerx_amd.serve import server
    args = server.parse_args(["--speculative", "4", "--template", "vanilla"])
    monkeypatch.setenv("DTX_SERVE_BATCH", "0")
    monkeypatch.setenv("DTX_SERVE_CONCURRENCY", "2")
    pool, batcher = server.build_fronts(model, None, args, CPU)
    assert batcher is None and [e.speculative for e in pool.engines] == [4, 4]
    assert server.spec_stats(pool.engines) == {"verify_steps": 0, "tokens": 0}
    monkeypatch.delenv("DTX_SERVE_BATCH")
    pool, batcher = server.build_fronts(model, None, args, CPU)
    assert batcher.engine.speculative == 4
    assert [e.speculative for e in pool.engines] == [0, 0]
    httpd = ThreadingHTTPServer(("127.0.0.1", 0),
                                server.build_handler(pool, batcher))
    url = f"http://127.0.0.1:{httpd.server_address[1]}"
    threading.Thread(target=httpd.serve_forever, daemon=True).start()

    def health():
        with urllib.request.urlopen(url + "/health", timeout=60) as r:
            return json.load(r)

    try:
        assert health() == {"status": "ok", "verify_steps": 0, "tokens": 0}
        seen = 0
        for stream in (False, True):
            req = urllib.request.Request(url + "/chat/completions", json.dumps({
                "messages": [{"role": "user", "content": "abcdefgh " * 4}],
                "max_tokens": 24, "temperature": 0.0,
                "stream": stream}).encode())
            with urllib.request.urlopen(req, timeout=120) as r:
                r.read()
            h = health()
            assert h["tokens"] >= h["verify_steps"] > seen
            seen = h["verify_steps"]
    finally:
        httpd.shutdown()


def test_refusals(model):
    with pytest.raises(ValueError, match="bf16"):
        InferenceEngine(model, template="vanilla", device=CPU,
                        kv_cache="int8", speculative=4)
    for k in (16, -1):
        with pytest.raises(ValueError, match="0..15"):
            InferenceEngine(model, template="vanilla", device=CPU,
                            speculative=k)
    from datatunerx_amd.api.types import FinetuneJob
    from datatunerx_amd.api.validation import ValidationError, validate_

    def job(serve_cfg):
        return FinetuneJob(name="spec", spec={
            "fineTune": {"finetuneSpec": {
                "llm": "llama-tiny", "dataset": "ds",
                "hyperparameter": {"hyperparameterRef": "hp"}, "node": 1}},
            "serveConfig": serve_cfg})

    validate_(job({"speculative": 4}))
    validate_(job({"speculative": 0, "tensorParallel": 2}))
    for bad in (16, -1, "4", True):
        with pytest.raises(ValidationError, match="speculative"):
            validate_(job({"speculative": bad}))
    with pytest.raises(ValidationError, match="tensorParallel"):
        validate_(job({"speculative": 4, "tensorParallel": 2}))
    from datatunerx_amd.serve import server
    with pytest.raises(SystemExit, match="--speculative is not supported"):
        server.main(["--speculative", "4", "--kv-cache", "int8",
                     "--model", "llama-tiny"])
