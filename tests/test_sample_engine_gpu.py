"""Device sampling in the serving engine: requests with different
temperature / top_p / top_k / seed share one graphed batch, a seeded
request is reproducible whatever it shares the batch with, and the
batching front and the HTTP API pass the parameters through."""

import json
import threading
import urllib.error
import urllib.request

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def engine():
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import InferenceEngine
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=512, hidden_size=256,
                      intermediate_size=512, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2,
                      max_position_embeddings=256)
    with torch.device(DEV):
        model = LlamaForCausalLM(cfg, lora=False, dtype=torch.bfloat16)
    model.init_random()
    model.eval()
    eng = InferenceEngine(model, template="vanilla", device=DEV)
    assert eng.device_sampling is True
    return eng


def _msgs(text):
    return [{"role": "user", "content": text}]


SAMPLED = [dict(temperature=0.8, top_p=0.9, seed=11),
           dict(temperature=1.2, top_p=1.0, top_k=20, seed=12),
           dict(temperature=0.5, top_p=0.7, top_k=5, seed=13),
           dict(temperature=1.0, top_p=0.95, seed=14)]


def _requests():
    """Eight requests: greedy ones (even rows) among sampled ones with
    four different settings."""
    texts = ["hello world", "a much longer prompt with many words in",
             "x", "short one", "tell me more", "why", "another prompt",
             "the last of them"]
    reqs = []
    for i, t in enumerate(texts):
        r = {"messages": _msgs(t), "max_tokens": 8}
        if i % 2:
            r.update(SAMPLED[i // 2])
        reqs.append(r)
    return reqs


def test_mixed_batch_shares_one_generation(engine):
    from datatunerx_amd.serve.engine import InferenceEngine
    assert InferenceEngine.MAX_BATCH >= 8
    reqs = _requests()
    outs = engine.chat_batch(reqs)
    assert len(outs) == 8
    for r, o in zip(reqs, outs):
        if "temperature" not in r:
            assert o == engine.chat(r["messages"], 8)
    # the sampled rows are reproducible too: same seeds, same texts
    assert engine.chat_batch(reqs) == outs
    streamed = [""] * 8
    for i, d in engine.chat_batch_stream(reqs):
        if d is not None:
            streamed[i] += d
    assert streamed == outs


def test_sampled_batch_runs_the_graphed_decoder(engine):
    from datatunerx_amd.serve.engine import _GraphedDecoder
    st = engine._batch_state(3, 12, 8, greedy=False)
    assert isinstance(st, _GraphedDecoder)
    assert st is engine._bgraphed
    out = engine.generate_batch([[5, 6, 7], [9, 10]], 6, temperature=0.9,
                                top_p=0.9, seed=[1, 2])
    assert all(0 < len(o) <= 6 for o in out)


def test_seeded_request_is_reproducible_across_company(engine):
    """The same seeded request alone in the MAX_BATCH graph, in row 5
    among seven requests with other parameters, and repeated."""
    L, n = 12, 10
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(4, 500, (L,), generator=g).tolist()
               for _ in range(8)]
    mine = dict(temperature=0.9, top_p=0.9, top_k=50, seed=4242)
    alone = engine.generate_batch([prompts[5]], n, **mine)[0]
    assert engine._bgraphed, "batched graphed step did not engage"
    assert len(alone) >= 2
    temps = [0.0, 1.3, 0.7, 0.0, 1.0, mine["temperature"], 0.6, 1.1]
    top_ps = [1.0, 0.8, 1.0, 1.0, 0.5, mine["top_p"], 0.99, 0.9]
    top_ks = [0, 0, 3, 0, 100, mine["top_k"], 0, 7]
    seeds = [None, 1, 2, None, 3, mine["seed"], 4, 5]
    for _ in range(2):
        outs = engine.generate_batch(prompts, n, temperature=temps,
                                     top_p=top_ps, top_k=top_ks, seed=seeds)
        assert outs[5] == alone
    assert engine.generate_batch([prompts[5]], n, **mine)[0] == alone
    # another seed draws other tokens
    other = engine.generate_batch([prompts[5]], n,
                                  **dict(mine, seed=4243))[0]
    assert other != alone
    # single stream (B = 1 graph): reproducible, and top_k = 1 is greedy
    one = engine.generate(prompts[5], n, adapter=None, **mine)
    assert engine.generate(prompts[5], n, adapter=None, **mine) == one
    assert engine.generate(prompts[5], n, temperature=1.5, top_k=1) == \
        engine.generate(prompts[5], n)


class _Counting:
    """Engine wrapper that counts the calls the front makes."""

    def __init__(self, engine, with_attr=True):
        self._e = engine
        self.calls = []
        if with_attr:
            self.device_sampling = engine.device_sampling

    def chat(self, *a, **kw):
        self.calls.append(("chat", 1))
        return self._e.chat(*a, **kw)

    def chat_batch(self, requests):
        self.calls.append(("chat_batch", len(requests)))
        return self._e.chat_batch(requests)

    def chat_batch_stream(self, requests):
        self.calls.append(("chat_batch_stream", len(requests)))
        yield from self._e.chat_batch_stream(requests)


class _Stub:
    """Host-sampling engine stand-in: no device_sampling attribute."""

    def __init__(self):
        self.calls = []

    def chat(self, messages, max_tokens, temperature, top_p, **kw):
        self.calls.append([(temperature, top_p)])
        return "one"

    def chat_batch(self, requests):
        self.calls.append([(r["temperature"], r["top_p"])
                           for r in requests])
        return ["b"] * len(requests)


def _five(front):
    temps = (0.0, 0.0, 0.8, 0.0, 0.8)
    res = [None] * 5

    def one(i, t):
        try:
            res[i] = front.chat(_msgs("hello there"), 6, t, 1.0)
        except Exception as e:                   # pragma: no cover
            res[i] = e
    ts = [threading.Thread(target=one, args=(i, t))
          for i, t in enumerate(temps)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(isinstance(r, Exception) or r is None for r in res), res
    return res


def test_front_batches_mixed_requests_on_a_device_sampling_engine(engine):
    from datatunerx_amd.serve.server import BatchingFront
    # the worker leaves its collection loop as soon as the batch is full
    eng = _Counting(engine)
    res = _five(BatchingFront(eng, max_batch=5, linger=30.0))
    assert eng.calls in ([("chat_batch", 5)], [("chat_batch_stream", 5)])
    want = engine.chat(_msgs("hello there"), 6)
    assert [res[i] for i in (0, 1, 3)] == [want] * 3
    # ... and still splits them for an engine that samples on the host
    stub = _Stub()
    _five(BatchingFront(stub, max_batch=5, linger=30.0))
    assert sorted(len(c) for c in stub.calls) == [2, 3]
    assert all(len(set(c)) == 1 for c in stub.calls)


def test_top_k_and_seed_arrive_through_http(engine, monkeypatch):
    from http.server import ThreadingHTTPServer

    from datatunerx_amd.serve.server import build_handler
    seen = []
    real = engine.chat

    def spy(*a, **kw):
        seen.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(engine, "chat", spy)
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), build_handler(engine))
    port = httpd.server_address[1]
    threading.Thread(target=httpd.serve_forever, daemon=True).start()

    def post(**extra):
        body = {"messages": _msgs("hello"), "max_tokens": 6,
                "temperature": 0.9, "top_p": 0.9}
        body.update(extra)
        req = urllib.request.Request(
            f"http://127.0.0.1:{port}/v1/chat/completions",
            data=json.dumps(body).encode(),
            headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=120) as r:
            return json.load(r)["choices"][0]["message"]["content"]

    try:
        a = post(top_k=5, seed=7)
        assert seen[-1] == {"top_k": 5, "seed": 7}
        assert post(top_k=5, seed=7) == a
        post(seed=None)
        assert seen[-1] == {}
        for bad in ({"seed": "abc"}, {"seed": 1.5}, {"top_k": "many"},
                    {"top_k": -1}):
            with pytest.raises(urllib.error.HTTPError) as ei:
                post(**bad)
            assert ei.value.code == 400
    finally:
        httpd.shutdown()
