"""Inference engine for the inference-compare service.

Replaces the reference's Ray Serve `LlamaDeployment` app (baked into the
checkpoint image — finetunejob_controller.go:378-384):
native PyTorch-ROCm decode through the same fused HIP kernels as
training, with a preallocated KV cache. Single-token decode is
WEIGHT-bandwidth-bound, so throughput scales by request BATCHING
(ragged batched decode, hipGraph-captured batched token step) rather
than by streams; per-stream engine pools cover mixed workloads and the
TP path for 13B is in parallel/tp.py. The serve process is per-job and
torn down after scoring.
"""

from __future__ import annotations

import copy
import json
import math
import os
import random
from typing import List, Optional

import torch

from ..data.dataset import ByteTokenizer
from ..data.templates import get_template
from ..models import (GPT2Config, GPT2ForCausalLM, LlamaConfig,
                      LlamaForCausalLM, load_adapter)


class KVCache:
    """BSHD cache ([B, max_s, Hkv, D]) matching the attention kernels'
    native layout — appends along dim 1.

    update() returns (k, v, len_dev) in one of two modes. Host mode (no
    counters, or S > 1): append at the host counter `cur`; the returned
    tensors are the length-exact prefix and len_dev is None. Device mode
    (counters given and S == 1): one token per row written at wpos[b];
    the returned tensors are full-capacity and len_dev is len32, the
    per-row live length the decode kernel reads on device — no host
    value enters the step, so it replays from a hipGraph. wpos (int64
    [B], an index into the cache flattened to [B * max_s] slots) and
    len32 (int32 [B]) belong to a _DecodeState and are shared by every
    layer's cache."""

    def __init__(self, B, Hkv, max_s, D, device, dtype,
                 wpos=None, len32=None):
        self.k = torch.zeros(B, max_s, Hkv, D, device=device, dtype=dtype)
        self.v = torch.zeros(B, max_s, Hkv, D, device=device, dtype=dtype)
        self.cur = 0
        self.wpos, self.len32 = wpos, len32

    def row_view(self, i):
        """Host-mode B = 1 cache over row i's storage: ragged rows
        prefill one at a time through it."""
        row = copy.copy(self)
        row.k, row.v = self.k[i:i + 1], self.v[i:i + 1]
        row.cur, row.wpos, row.len32 = 0, None, None
        return row

    def update(self, k, v):
        S = k.shape[1]
        if self.wpos is not None and S == 1:
            # one flat index_copy_ for every B: an advanced-index put at
            # (row, pos) costs single-stream decode 2 % (64 writes a
            # token at 7B; profiles/README.md, serving decode)
            self.k.view(-1, *k.shape[2:]).index_copy_(0, self.wpos, k[:, 0])
            self.v.view(-1, *v.shape[2:]).index_copy_(0, self.wpos, v[:, 0])
            return self.k, self.v, self.len32
        # a right-padded batched prefill lands here too: per-row len32
        # bounds every later read and decode overwrites the first pad
        # slot, so pad K/V beyond a row's real length is never consumed
        # (pads sit AFTER real tokens: no real query attends one)
        start, self.cur = self.cur, self.cur + S
        self.k[:, start:self.cur] = k
        self.v[:, start:self.cur] = v
        if self.k.shape[0] == 1 and k.is_cuda:
            # the GPU decode kernel takes the dense prefix view directly
            # (no per-token copy)
            return self.k[:, :self.cur], self.v[:, :self.cur], None
        if start == 0:
            return k, v, None            # the prefix IS what came in
        # batch>1 / CPU paths want contiguous
        return (self.k[:, :self.cur].contiguous(),
                self.v[:, :self.cur].contiguous(), None)


class _DecodeState:
    """Counters and layer caches of one ragged decode batch. Row b's
    next token is written at index pos[b] (pos32 feeds rope, wpos ==
    b * max_s + pos is the flat cache slot) and attends len32[b] keys;
    every method keeps len32 == pos + 1, so a device-mode update never
    attends an empty row. Batched decode shares one weight stream across
    the batch — single-stream decode is WEIGHT-bandwidth-bound, so this
    is the scaling axis for serving throughput.

    The rows' sampling parameters are device state too (temperature,
    top_p, top_k, seed, and offset: the number of tokens the row has
    sampled, its RNG counter), so ops.sample draws every row of a step
    with that row's own setting; all-zero (the start) is greedy."""

    def __init__(self, B, Hkv, max_s, D, layers, device, dtype):
        self.B, self.max_s = B, max_s
        self._row0 = torch.arange(B, device=device) * max_s
        self.wpos = self._row0.clone()
        self.pos32 = torch.zeros(B, dtype=torch.int32, device=device)
        self.len32 = torch.ones(B, dtype=torch.int32, device=device)
        self.temperature = torch.zeros(B, dtype=torch.float32,
                                       device=device)
        self.top_p = torch.ones(B, dtype=torch.float32, device=device)
        self.top_k = torch.zeros(B, dtype=torch.int32, device=device)
        self.seed = torch.zeros(B, dtype=torch.int64, device=device)
        self.offset = torch.zeros(B, dtype=torch.int32, device=device)
        self.caches = [KVCache(B, Hkv, max_s, D, device, dtype,
                               wpos=self.wpos, len32=self.len32)
                       for _ in range(layers)]

    def set_state(self, lens):
        """After prefill: row b holds lens[b] tokens."""
        pos = torch.tensor(lens, dtype=torch.long,
                           device=self.wpos.device)
        self.wpos.copy_(self._row0 + pos)
        self.pos32.copy_(pos)
        self.len32.copy_(pos + 1)

    def set_sampling(self, samp, offset: int = 1):
        """Per-row sampling parameters (a _Sampling of B rows). offset:
        tokens every row has sampled already — 1 after prefill, whose
        first token is drawn with offset 0."""
        self.temperature.copy_(torch.tensor(samp.temperature,
                                            dtype=torch.float32))
        self.top_p.copy_(torch.tensor(samp.top_p, dtype=torch.float32))
        self.top_k.copy_(torch.tensor(samp.top_k, dtype=torch.int32))
        self.seed.copy_(torch.tensor(samp.seed, dtype=torch.int64))
        self.offset.fill_(offset)

    def sample_args(self):
        return (self.temperature, self.top_p, self.top_k, self.seed,
                self.offset)

    def reset(self):
        """Empty rows. No cache zeroing needed: prefill overwrites rows
        up to their length and attention never reads past len32."""
        self.set_state([0] * self.B)
        for c in self.caches:
            c.cur = 0

    def advance(self):
        self.wpos += 1
        self.pos32 += 1
        self.len32 += 1
        self.offset += 1


class _GraphedDecoder(_DecodeState):
    """hipGraph-captured decode step (torch.cuda.CUDAGraph) at fixed
    batch B and cache capacity max_s: the whole token forward replays
    as one graph — positions, cache lengths and the adapter of each row
    are device tensors the captured kernels read at replay, so ONE graph
    serves every sequence length and adapter assignment. Built once per
    engine (under the capture lock) and reset per request; a batch pads
    to B with dummy rows. The graph's static outputs are `logits`
    [B, 1, V] and `out` [B]: the greedy argmax, or with `sample` the
    token ops.sample draws for each row from the state's sampling
    buffers (a row at temperature 0 gets the same argmax, bit for bit),
    so one graph serves every mix of greedy and sampled rows."""

    def __init__(self, model, cfg, device, B, max_s, sample=False):
        super().__init__(B, cfg.num_key_value_heads, max_s, cfg.head_dim,
                         cfg.num_hidden_layers, device,
                         next(model.parameters()).dtype)
        self.input = torch.ones(B, 1, dtype=torch.long, device=device)
        # -1 = base model / dummy row
        self.adapter_idx, akw = _graph_adapter_buffer(model, B, device)

        def forward():
            logits = model(self.input, pos_dev=self.pos32,
                           kv_caches=self.caches, **akw)
            if sample:
                from .. import ops
                return logits, ops.sample(logits[:, -1],
                                          *self.sample_args())
            return logits, logits[:, -1].argmax(-1)

        with torch.no_grad():
            for _ in range(3):          # warmup: allocator + kernels
                forward()
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.logits, self.out = forward()

    def set_adapters(self, idx):
        """idx: one adapter index per row of the padded batch."""
        if self.adapter_idx is not None:
            self.adapter_idx.copy_(torch.tensor(idx, dtype=torch.int32))

    def step(self, cur):
        """cur: this step's input tokens — [B, 1] int64 on device, or a
        host int when B == 1. Refreshes `logits` and `out`."""
        self.input[:] = cur
        self.graph.replay()
        self.advance()


def builtin_config(name: str, **lora_kw):
    """Resolve a builtin model name to ("llama"|"gpt2", config) without
    allocating weights — the single registry the engine, TP server and
    tests share. Raises ValueError on unknown names."""
    if name in ("llama2-7b", "llama-2-7b"):
        return "llama", LlamaConfig.llama2_7b(**lora_kw)
    if name in ("llama2-13b", "llama-2-13b"):
        return "llama", LlamaConfig.llama2_13b(**lora_kw)
    if name in ("llama3-8b", "llama-3-8b"):
        return "llama", LlamaConfig.llama3_8b(**lora_kw)
    if name == "llama-tiny":
        return "llama", LlamaConfig.tiny(**lora_kw)
    if name == "llama-mini":
        return "llama", LlamaConfig.mini(**lora_kw)
    if name in ("gpt2-small", "gpt2"):
        return "gpt2", GPT2Config.small(**lora_kw)
    if name == "gpt2-tiny":
        return "gpt2", GPT2Config.tiny(**lora_kw)
    raise ValueError(f"unknown model {name!r}")


QUANTIZATIONS = {"int8": 8, "int4": 4}


def _graph_adapter_buffer(model, rows: int, device):
    """(int32 [rows] index buffer filled with -1, model kwargs) for a
    graphed decoder over a multi-adapter model; (None, {}) otherwise —
    such a model captures exactly as before."""
    if getattr(model, "adapters", None) is None:
        return None, {}
    from ..models.multilora import AdapterSelection
    buf = torch.full((rows,), -1, dtype=torch.int32, device=device)
    return buf, {"adapters": AdapterSelection(buf, None)}


def build_model(name: str, device, adapter_dir: Optional[str] = None,
                lora_kw: Optional[dict] = None,
                quantization: Optional[str] = None,
                adapters: Optional[dict] = None):
    """quantization: None | "int8" | "int4" — weight-only quantize every
    projection (LoRA bases included, adapters kept unmerged in bf16)
    AFTER weights and adapter are loaded, so the service runs the model
    a quantized job trained against; decode then streams the integer
    weights (ops.qlinear) instead of bf16.

    adapters: {name: adapter_dir, ...} — multi-adapter serving: the
    model is built WITHOUT LoRA modules and every targeted projection
    gets a stack of all the adapters (models/multilora.py); the name ->
    index registry hangs on the model as `model.adapters` and requests
    pick an adapter by name. Mutually exclusive with adapter_dir."""
    if adapters is not None and adapter_dir:
        raise ValueError("build_model: give either adapter_dir (one "
                         "adapter) or adapters (named stack), not both")
    if adapters is not None and not adapters:
        raise ValueError("build_model: adapters is empty")
    if quantization is not None and quantization not in QUANTIZATIONS:
        raise ValueError(
            f"unknown quantization {quantization!r} "
            f"(expected one of {sorted(QUANTIZATIONS)})")
    dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
    lora_kw = dict(lora_kw or {})
    if adapter_dir and not lora_kw:
        # adapt the LoRA geometry to the checkpoint's adapter_config.json
        cfg_path = os.path.join(adapter_dir, "adapter_config.json")
        if os.path.exists(cfg_path):
            with open(cfg_path) as f:
                ac = json.load(f)
            lora_kw = {"lora_r": int(ac.get("r", 8)),
                       "lora_alpha": float(ac.get("lora_alpha", 32)),
                       "lora_targets": tuple(ac.get("target_modules") or
                                             ("q_proj", "v_proj"))}
    from ..models.hf_io import (is_hf_model_dir, load_hf_config,
                                load_hf_weights)
    hf_dir = is_hf_model_dir(name)
    if hf_dir:
        family, cfg = "llama", load_hf_config(name, **lora_kw)
        lora = bool(adapter_dir)
    else:
        family, cfg = builtin_config(name, **lora_kw)
        lora = adapters is None     # a named stack replaces LoRA modules
    if adapters is not None and family != "llama":
        raise ValueError(
            f"multi-adapter serving supports llama models, not {name!r}")
    with torch.device(device):
        if family == "llama":
            model = LlamaForCausalLM(cfg, lora=lora, dtype=dtype)
        else:
            model = GPT2ForCausalLM(cfg, dtype=dtype)
    if hf_dir:
        load_hf_weights(model, name)   # real local weights
    else:
        model.init_random()      # builtin names: random-init (no network)
    if adapter_dir:
        load_adapter(model, adapter_dir)
    if adapters is not None:
        from ..models.multilora import attach_adapters_
        attach_adapters_(model, adapters)
    if quantization is not None:
        if not isinstance(model, LlamaForCausalLM):
            raise ValueError(
                f"quantized serving supports llama models, not {name!r} "
                "(its layers are not FrozenLinear)")
        from ..models.quant import quantize_model_
        quantize_model_(model, QUANTIZATIONS[quantization], lora_base=True)
    model.eval()
    return model


class _Sampling:
    """Per-row sampling parameters of one generation: lists of
    temperature, top_p, top_k and seed (one entry a row), and `plain`:
    the row named neither a seed nor a top_k, so a host-sampling engine
    draws it from the torch RNG the way it always did."""

    def __init__(self, temperature, top_p, top_k, seed, plain):
        self.temperature, self.top_p = temperature, top_p
        self.top_k, self.seed, self.plain = top_k, seed, plain

    def __len__(self):
        return len(self.temperature)

    @property
    def greedy(self) -> bool:
        return not any(t > 0 for t in self.temperature)

    def padded(self, n: int):
        """Extended to n rows with greedy dummy rows."""
        k = n - len(self)
        return _Sampling(self.temperature + [0.0] * k,
                         self.top_p + [1.0] * k, self.top_k + [0] * k,
                         self.seed + [0] * k, self.plain + [True] * k)

    def tensors(self, device, offset: int = 0):
        """ops.sample's parameter tensors, every row at `offset`."""
        n = len(self)
        return (torch.tensor(self.temperature, dtype=torch.float32,
                             device=device),
                torch.tensor(self.top_p, dtype=torch.float32,
                             device=device),
                torch.tensor(self.top_k, dtype=torch.int32, device=device),
                torch.tensor(self.seed, dtype=torch.int64, device=device),
                torch.full((n,), offset, dtype=torch.int32, device=device))


class InferenceEngine:
    """One generation context over a (shared, read-only) model. For
    concurrent serving, build several engines over the SAME model
    (serve/server.py EnginePool): each holds its own KV caches, hip
    graph and HIP stream, so batch-1 decodes overlap on the GPU instead
    of queueing on one engine lock (decode is latency-bound, not
    occupancy-bound)."""

    MAX_BATCH = int(os.environ.get("DTX_SERVE_MAX_BATCH", "8"))

    def __init__(self, model, tokenizer=None, template: str = "llama2",
                 device=None, graph_decode: bool = True,
                 own_stream: bool = False):
        self.model = model
        self.tok = tokenizer or ByteTokenizer()
        self.template = template
        self.device = device or next(model.parameters()).device
        self.is_llama = isinstance(model, LlamaForCausalLM)
        import torch.distributed as dist
        self._graphed = None
        self._bgraphed = None
        self._stream = (torch.cuda.Stream(device=self.device)
                        if own_stream and self.device.type == "cuda"
                        else None)
        self._graph_ok = (graph_decode and self.is_llama and
                          self.device.type == "cuda" and
                          not dist.is_initialized() and
                          os.environ.get("DTX_NO_GRAPH") != "1")
        # Sampling on the device (ops.sample inside the decode step, each
        # row with its own parameters): llama on one GPU, with logits the
        # kernel takes. Everywhere else the host sampler, as before.
        from .. import ops
        vocab = getattr(getattr(model, "cfg", None), "vocab_size", 0)
        self.device_sampling = (
            self.is_llama and self.device.type == "cuda" and
            not dist.is_initialized() and
            next(model.parameters()).dtype == torch.bfloat16 and
            vocab % 8 == 0 and 0 < vocab <= ops.sample_max_vocab())
        # seeds of the requests that name none
        self._seed_rng = random.Random()
        # stop set: tokenizer eos (may be a LIST in llama3-style
        # config.json), plus any template stop_words that the tokenizer
        # encodes to a single special id (llama3's <|eot_id|> ends a
        # turn but is distinct from eos)
        eos = getattr(self.tok, "eos_token_id", None)
        self._stop_ids = set(eos) if isinstance(eos, (list, tuple)) \
            else ({eos} if eos is not None else set())
        extra = getattr(self.tok, "stop_token_ids", None)
        if extra:
            self._stop_ids.update(int(i) for i in extra)
        try:
            tmpl = get_template(template)
            for w in tmpl.stop_words:
                ids = self.tok.encode(w, add_special_tokens=False) \
                    if hasattr(self.tok, "encode") else []
                if len(ids) == 1:
                    self._stop_ids.add(int(ids[0]))
        except (KeyError, TypeError):
            pass

    # ---------------------------------------------------- adapters
    def _adapter_index(self, adapter: Optional[str]) -> int:
        """Registry index of a request's adapter (-1: base model).
        Raises ValueError for a name the model does not hold — before
        any GPU work of the request."""
        if adapter is None:
            return -1
        reg = getattr(self.model, "adapters", None)
        if reg is None:
            raise ValueError(
                f"unknown adapter {adapter!r}: this model was built "
                "without named adapters")
        return reg.index(adapter)

    def _selection(self, idx):
        """Model kwargs for per-sequence adapter indices: {} when every
        sequence runs the base model."""
        if all(g < 0 for g in idx):
            return {}
        from ..models.multilora import AdapterSelection
        return {"adapters": AdapterSelection(
            torch.tensor(list(idx), dtype=torch.int32,
                         device=self.device), idx)}

    def _is_stop(self, tok_id) -> bool:
        return int(tok_id) in self._stop_ids

    def _stream_ctx(self):
        import contextlib
        if self._stream is None:
            return contextlib.nullcontext()
        return torch.cuda.stream(self._stream)

    # hip graph CAPTURE must never run concurrently with another
    # engine's capture or in-flight kernels (capture mode is
    # context-global); all captures serialize on this lock. Replays of
    # distinct graphs on distinct streams are concurrency-safe.
    _capture_lock = __import__("threading").Lock()

    def _capture(self, B, max_s):
        """A new graphed decoder, or None when its capture fails (the
        caller decides what that turns off)."""
        try:
            with InferenceEngine._capture_lock, self._stream_ctx():
                return _GraphedDecoder(self.model, self.model.cfg,
                                       self.device, B, max_s,
                                       sample=self.device_sampling)
        except Exception:
            return None

    def _get_graphed(self):
        """Single-stream decoder at full context; a failed capture turns
        graph decode off for the engine."""
        if self._graphed is None and self._graph_ok:
            self._graphed = self._capture(
                1, self.model.cfg.max_position_embeddings)
            self._graph_ok = self._graphed is not None
        return self._graphed

    def _get_batched_graphed(self, max_s):
        """MAX_BATCH-row decoder; a failed capture turns off only the
        batched graph (`_bgraphed` False: not tried again)."""
        if self._bgraphed is None and self._graph_ok:
            self._bgraphed = self._capture(InferenceEngine.MAX_BATCH,
                                           max_s) or False
        return self._bgraphed or None

    def warmup(self):
        """Build the graphed decoder + run one tiny generation NOW (a
        pool builds engines sequentially before serving concurrent
        requests, so no capture happens mid-traffic)."""
        with self._stream_ctx():
            self._get_graphed()
            list(self.generate([1], max_new_tokens=2))
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    # ------------------------------------------------------------ chat
    def _encode_messages(self, messages: List[dict]) -> List[int]:
        """[{role, content}] -> prompt ids through the engine's template:
        the last system message, completed user/assistant turns as
        history, the last unanswered user message as the query."""
        system, history, pending = "", [], None
        for m in messages:
            if m["role"] == "system":
                system = m["content"]
            elif m["role"] == "user":
                pending = m["content"]
            elif m["role"] == "assistant" and pending is not None:
                history.append((pending, m["content"]))
                pending = None
        src, _ = get_template(self.template).encode_oneturn(
            self.tok, pending or "", "", history, system)
        return src

    def _delta(self, ids, sent: str, final: bool = False):
        """(new text, all text sent) for a stream that decoded `ids` and
        already sent `sent`. Until final, trailing U+FFFD is held back:
        a multi-byte UTF-8 char split across tokens decodes as a
        replacement char until the rest arrives; emitting it early would
        make the concatenated stream differ from the one-shot decode."""
        text = self.tok.decode(ids)
        if not final:
            text = text.rstrip("\ufffd")
        if len(text) <= len(sent):
            return "", sent
        return text[len(sent):], text

    def chat(self, messages: List[dict], max_tokens: int = 64,
             temperature: float = 0.0, top_p: float = 1.0,
             adapter: Optional[str] = None, top_k: int = 0,
             seed: Optional[int] = None) -> str:
        """messages: [{role, content}] -> completion text. adapter: name
        of an attached adapter (None: the base model). top_k: sample
        among the k most likely tokens (0: all). seed: makes a sampled
        completion reproducible — the same request with the same seed
        returns the same tokens, whatever it shares a batch with."""
        self._adapter_index(adapter)
        with self._stream_ctx():
            ids = self.generate(self._encode_messages(messages),
                                max_tokens, temperature, top_p,
                                adapter=adapter, top_k=top_k, seed=seed)
            return self.tok.decode(ids)

    def chat_stream(self, messages: List[dict], max_tokens: int = 64,
                    temperature: float = 0.0, top_p: float = 1.0,
                    adapter: Optional[str] = None, top_k: int = 0,
                    seed: Optional[int] = None):
        """Like chat() but yields text DELTAS as tokens decode (the
        serving endpoint streams these as SSE chunks). Token-identical
        to chat(): same generate loop, so TP followers running chat()
        stay in collective lockstep with a streaming front rank."""
        self._adapter_index(adapter)
        ids, sent = [], ""
        for tok_id in self.generate_stream(
                self._encode_messages(messages), max_tokens, temperature,
                top_p, adapter=adapter, top_k=top_k, seed=seed):
            ids.append(tok_id)
            delta, sent = self._delta(ids, sent)
            if delta:
                yield delta
        delta, sent = self._delta(ids, sent, final=True)
        if delta:
            yield delta

    @torch.no_grad()
    def generate(self, prompt_ids: List[int], max_new_tokens: int = 64,
                 temperature: float = 0.0, top_p: float = 1.0,
                 adapter: Optional[str] = None, top_k: int = 0,
                 seed: Optional[int] = None) -> List[int]:
        return list(self.generate_stream(prompt_ids, max_new_tokens,
                                         temperature, top_p,
                                         adapter=adapter, top_k=top_k,
                                         seed=seed))

    @torch.no_grad()
    def generate_stream(self, prompt_ids: List[int],
                        max_new_tokens: int = 64, temperature: float = 0.0,
                        top_p: float = 1.0, adapter: Optional[str] = None,
                        top_k: int = 0, seed: Optional[int] = None):
        gi = self._adapter_index(adapter)
        samp = self._sampling(1, temperature, top_p, top_k, seed)
        with self._stream_ctx():
            yield from self._generate_stream(prompt_ids, max_new_tokens,
                                             samp, gi)

    # ------------------------------------------------------- sampling
    def _sampling(self, n: int, temperature, top_p, top_k=0, seed=None):
        """_Sampling of n rows; each argument is a scalar or a per-row
        list. A sampled row that names no seed gets one from the
        engine's own generator — except a plain row (no seed, no top_k)
        of a host-sampling engine, which stays on the torch RNG."""
        def rows(v, cast, name):
            if isinstance(v, (list, tuple)):
                if len(v) != n:
                    raise ValueError(
                        f"{len(v)} {name} values for {n} prompts")
                return [cast(x) for x in v]
            return [cast(v)] * n

        t = rows(temperature, float, "temperature")
        p = rows(top_p, float, "top_p")
        k = rows(top_k, lambda x: max(int(x or 0), 0), "top_k")
        s = rows(seed, lambda x: None if x is None else int(x), "seed")
        plain = [si is None and ki == 0 for si, ki in zip(s, k)]
        for i in range(n):
            if s[i] is None:
                drawn = t[i] > 0 and (self.device_sampling or not plain[i])
                s[i] = self._seed_rng.getrandbits(63) if drawn else 0
            else:       # any Python int, as the int64 with the same bits
                s[i] = (s[i] + (1 << 63)) % (1 << 64) - (1 << 63)
        return _Sampling(t, p, k, s, plain)

    def _device_sample(self, logits, samp, offset: int) -> torch.Tensor:
        """ops.sample over the rows of logits [B, V] on the GPU, every
        row with its own parameters and all at token counter `offset`."""
        from .. import ops
        return ops.sample(logits, *samp.tensors(self.device, offset))

    def _host_sample(self, logits, samp, i: int, offset: int) -> int:
        """Row i's token `offset` from its logits [V] on a host-sampling
        engine: plain rows through the torch RNG as ever, rows with a
        seed or a top_k through ops.sample's CPU reference."""
        if samp.plain[i]:
            return self._sample(logits, samp.temperature[i], samp.top_p[i])
        return self._sample(logits, samp.temperature[i], samp.top_p[i],
                            samp.top_k[i], samp.seed[i], offset)

    @torch.no_grad()
    def _generate_stream(self, prompt_ids: List[int], max_new_tokens: int,
                         samp, gi: int = -1):
        """samp: the request's _Sampling (one row). Token n is drawn with
        RNG offset n on every path."""
        if not prompt_ids:
            raise ValueError("empty prompt")
        akw = self._selection([gi])
        limit = getattr(self.model.cfg, "max_position_embeddings", 1 << 30)
        if len(prompt_ids) >= limit:
            raise ValueError(
                f"prompt length {len(prompt_ids)} exceeds the model "
                f"context ({limit} positions)")
        ids = torch.tensor([prompt_ids], dtype=torch.long,
                           device=self.device)
        dev = self.device_sampling

        def pick(logits, n):        # logits [1, S, V] -> token n
            if dev:
                return int(self._device_sample(logits[:, -1], samp, n))
            return self._host_sample(logits[0, -1], samp, 0, n)

        n_out = 0
        gd = self._get_graphed() if self.is_llama else None
        if gd is not None and len(prompt_ids) + max_new_tokens + 1 < \
                gd.max_s:
            # hipGraph-replayed decode: prefill eagerly into the graph's
            # caches, then one graph replay per token
            gd.reset()
            gd.set_adapters([gi])
            gd.set_sampling(samp)
            logits = self.model(ids, pos0=0, kv_caches=gd.caches, **akw)
            gd.set_state([len(prompt_ids)])
            nxt = pick(logits, 0)
            for _ in range(max_new_tokens):
                if self._is_stop(nxt):
                    break
                yield nxt
                n_out += 1
                if len(prompt_ids) + n_out + 1 >= gd.max_s:
                    break
                gd.step(nxt)
                # device sampling: the graph drew the token (gd.out, the
                # same kernel as the eager path). Host sampling: from
                # the logits, one tie-breaking rule for graphed and eager
                nxt = int(gd.out[0]) if dev else pick(gd.logits, n_out)
            return
        if self.is_llama:
            cfg = self.model.cfg
            max_s = min(cfg.max_position_embeddings,
                        len(prompt_ids) + max_new_tokens + 8)
            caches = [KVCache(1, cfg.num_key_value_heads, max_s,
                              cfg.head_dim, self.device,
                              next(self.model.parameters()).dtype)
                      for _ in range(cfg.num_hidden_layers)]
            pos = 0
            cur = ids
            for n in range(max_new_tokens):
                logits = self.model(cur, pos0=pos, kv_caches=caches,
                                    **akw)
                pos += cur.shape[1]
                if pos >= max_s:
                    break
                nxt = pick(logits, n)
                if self._is_stop(nxt):
                    break
                yield nxt
                cur = torch.tensor([[nxt]], dtype=torch.long,
                                   device=self.device)
        else:
            seq = list(prompt_ids)
            for n in range(max_new_tokens):
                cur = torch.tensor([seq], dtype=torch.long,
                                   device=self.device)
                logits = self.model(cur)
                nxt = pick(logits, n)
                if self._is_stop(nxt):
                    break
                yield nxt
                seq.append(nxt)

    def _sample(self, logits: torch.Tensor, temperature: float,
                top_p: float, top_k: int = 0, seed: Optional[int] = None,
                offset: int = 0) -> int:
        """The host sampler. With neither seed nor top_k: the torch RNG.
        With either: ops.sample's CPU reference on this row, keyed by
        (seed, offset), so a seed means the same on every engine."""
        import torch.distributed as dist
        tp = dist.is_initialized() and dist.get_world_size() > 1
        comm_dev = (self.device if tp and dist.get_backend() == "nccl"
                    else torch.device("cpu"))
        if tp and dist.get_rank() != 0:
            # follower ranks take rank 0's choice (RNG is per-process)
            t = torch.zeros(1, dtype=torch.long, device=comm_dev)
            dist.broadcast(t, src=0)
            return int(t)
        if seed is not None or top_k > 0:
            from .. import ops
            nxt = int(ops.sample(
                logits.detach().float().cpu().view(1, -1),
                torch.tensor([temperature], dtype=torch.float32),
                torch.tensor([top_p], dtype=torch.float32),
                torch.tensor([top_k], dtype=torch.int32),
                torch.tensor([seed or 0], dtype=torch.int64),
                torch.tensor([offset], dtype=torch.int32))[0])
        elif temperature <= 0.0:
            nxt = int(logits.argmax())
        else:
            probs = torch.softmax(logits.float() / temperature, dim=-1)
            if top_p < 1.0:
                sp, si = probs.sort(descending=True)
                cum = sp.cumsum(0)
                keep = cum <= top_p
                keep[0] = True
                probs = torch.zeros_like(probs).scatter_(0, si[keep],
                                                         sp[keep])
                probs /= probs.sum()
            nxt = int(torch.multinomial(probs, 1))
        if tp:
            dist.broadcast(torch.tensor([nxt], dtype=torch.long,
                                        device=comm_dev), src=0)
        return nxt

    # ------------------------------------------------- batched decode
    @torch.no_grad()
    def generate_batch(self, prompts: List[List[int]],
                       max_new_tokens: int = 64,
                       temperature=0.0, top_p=1.0,
                       adapters: Optional[List[Optional[str]]] = None,
                       top_k=0, seed=None) -> List[List[int]]:
        """Ragged batched generation: per-row prefill, then ONE decode
        step per token for the whole batch (the weight stream is read
        once per step instead of once per request). adapters: one
        adapter name (or None: base model) per prompt — rows of one
        batch may use different adapters. temperature, top_p, top_k and
        seed: each a scalar for the whole batch or one value per
        prompt."""
        self._adapter_indices(adapters, len(prompts))
        samp = self._sampling(len(prompts), temperature, top_p, top_k,
                              seed)
        with self._stream_ctx():
            return self._generate_batch(prompts, max_new_tokens, samp,
                                        adapters=adapters)

    def _adapter_indices(self, adapters, n: int):
        if adapters is None:
            return [-1] * n
        if len(adapters) != n:
            raise ValueError(f"{len(adapters)} adapters for {n} prompts")
        return [self._adapter_index(a) for a in adapters]

    @torch.no_grad()
    def _generate_batch(self, prompts, max_new_tokens, samp, budgets=None,
                        adapters=None):
        outs = [[] for _ in prompts]
        for emitted in self._generate_batch_steps(
                prompts, max_new_tokens, samp, budgets, adapters):
            for i, t in emitted:
                outs[i].append(t)
        return outs

    def _batch_state(self, n, lmax, max_new_tokens, greedy):
        """Decode state for n prompts of at most lmax tokens: the
        graphed MAX_BATCH-row decoder when the batch fits it (on GPU;
        greedy batches only unless the engine samples on the device),
        else eager state of exactly n rows."""
        cfg = self.model.cfg
        if (greedy or self.device_sampling) and \
                self.device.type == "cuda" and \
                n <= InferenceEngine.MAX_BATCH:
            cap = min(cfg.max_position_embeddings,
                      int(os.environ.get("DTX_SERVE_MAXS", "2048")))
            gd = self._get_batched_graphed(cap) \
                if lmax + max_new_tokens + 8 < cap else None
            if gd is not None:
                gd.reset()
                return gd
        max_s = min(cfg.max_position_embeddings,
                    lmax + max_new_tokens + 8)
        return _DecodeState(n, cfg.num_key_value_heads, max_s,
                            cfg.head_dim, cfg.num_hidden_layers,
                            self.device,
                            next(self.model.parameters()).dtype)

    def _batch_prefill(self, st, prompts, aidx, samp):
        """Prefill every row into st's caches and hand the row lengths
        over to its counters. Returns each row's first sampled token
        (token 0 of its request)."""
        B, lens = len(prompts), [len(p) for p in prompts]
        last = [None] * B           # each row's logits at its last token
        if B > 1 and self.device.type == "cuda":
            # ONE right-padded batched prefill (pads never attended:
            # causal + pads-after-real; len32 bounds decode reads)
            padded = torch.zeros(B, max(lens), dtype=torch.long,
                                 device=self.device)
            for i, ids in enumerate(prompts):
                padded[i, :len(ids)] = torch.tensor(ids,
                                                    dtype=torch.long)
            logits = self.model(padded, pos0=0, kv_caches=st.caches,
                                **self._selection(aidx))
            for i in range(B):
                last[i] = logits[i, lens[i] - 1]
        else:
            for i, ids in enumerate(prompts):
                row = [c.row_view(i) for c in st.caches]
                t = torch.tensor([ids], dtype=torch.long,
                                 device=self.device)
                logits = self.model(t, pos0=0, kv_caches=row,
                                    **self._selection([aidx[i]]))
                last[i] = logits[0, -1]
        if self.device_sampling:
            # one call over the rows' last positions
            nxt = self._device_sample(torch.stack(last), samp, 0).tolist()
        else:
            nxt = [self._host_sample(last[i], samp, i, 0)
                   for i in range(B)]
        st.set_state(lens)
        return nxt

    def _batch_step(self, st, cur, akw, samp, n):
        """Token n of every row from the [B, 1] input `cur`: (tokens on
        the host, the next step's input)."""
        if isinstance(st, _GraphedDecoder):
            st.step(cur)
            return st.out.tolist(), st.out.view(-1, 1)
        logits = self.model(cur, kv_caches=st.caches, pos_dev=st.pos32,
                            **akw)
        if self.device_sampling:
            from .. import ops
            out = ops.sample(logits[:, -1], *st.sample_args())
            st.advance()
            return out.tolist(), out.view(-1, 1)
        st.advance()
        if not samp.greedy:
            toks = [self._host_sample(logits[i, -1], samp, i, n)
                    for i in range(st.B)]
        else:
            toks = logits[:, -1].argmax(-1).tolist()
        return toks, torch.tensor(toks, dtype=torch.long,
                                  device=self.device).view(-1, 1)

    def _emit(self, toks, done, count, budgets):
        """One step's [(row, token)] emissions. A row is done at a stop
        token or at its budget; dummy rows (beyond budgets) never emit."""
        emitted = []
        for i, t in enumerate(toks):
            if done[i]:
                continue
            if self._is_stop(t):
                done[i] = True
            elif i < len(budgets):
                if count[i] < budgets[i]:
                    emitted.append((i, t))
                    count[i] += 1
                if count[i] >= budgets[i]:
                    done[i] = True
        return emitted

    @torch.no_grad()
    def _generate_batch_steps(self, prompts, max_new_tokens, samp,
                              budgets=None, adapters=None):
        """Yields, per decode step, the [(row, token)] emissions.
        samp: the rows' _Sampling. budgets: optional per-row max_tokens
        (rows stop emitting — and count as done — at their own budget).
        adapters: optional per-row adapter names."""
        assert self.is_llama, "batched decode is the Llama path"
        aidx = self._adapter_indices(adapters, len(prompts))
        lens = [len(p) for p in prompts]
        if not prompts or min(lens) == 0:
            raise ValueError("empty prompt in batch")
        n_live = len(prompts)
        st = self._batch_state(n_live, max(lens), max_new_tokens,
                               greedy=samp.greedy)
        # a graphed decoder has a fixed batch: pad with greedy dummy
        # rows on the base model
        prompts = list(prompts) + \
            [[self.tok.bos_token_id]] * (st.B - n_live)
        aidx = aidx + [-1] * (st.B - n_live)
        samp = samp.padded(st.B)
        if isinstance(st, _GraphedDecoder):
            st.set_adapters(aidx)
        st.set_sampling(samp)
        if budgets is None:
            budgets = [max_new_tokens] * n_live
        count, done = [0] * n_live, [False] * st.B
        nxt = self._batch_prefill(st, prompts, aidx, samp)
        yield self._emit(nxt, done, count, budgets)
        cur = torch.tensor(nxt, dtype=torch.long,
                           device=self.device).view(-1, 1)
        akw = self._selection(aidx)
        cap = st.max_s - max(lens) - 2
        for n in range(1, 1 + min(max_new_tokens - 1, cap)):
            if all(done[:n_live]):
                break
            toks, cur = self._batch_step(st, cur, akw, samp, n)
            yield self._emit(toks, done, count, budgets)

    def _encode_requests(self, requests):
        """(prompts, budgets, _Sampling) of a batch of chat requests.
        Requests with different sampling parameters share a batch only
        where the engine samples on the device."""
        prompts = [self._encode_messages(r.get("messages", []))
                   for r in requests]
        budgets = [int(r.get("max_tokens", 64)) for r in requests]
        temps = [float(r.get("temperature", 0.0)) for r in requests]
        top_ps = [float(r.get("top_p", 1.0)) for r in requests]
        if not self.device_sampling and \
                len(set(zip(temps, top_ps))) > 1:
            # the host sampler draws a whole batch with ONE setting;
            # the BatchingFront groups requests by it before batching
            raise ValueError("batched requests must share "
                             "temperature/top_p")
        samp = self._sampling(len(requests), temps, top_ps,
                              [r.get("top_k", 0) for r in requests],
                              [r.get("seed") for r in requests])
        return prompts, budgets, samp

    def _request_adapters(self, requests):
        """Per-request "adapter" names (None when no request names one);
        unknown names raise ValueError here, before the generation."""
        names = [r.get("adapter") for r in requests]
        if all(n is None for n in names):
            return None
        self._adapter_indices(names, len(names))
        return names

    def chat_batch(self, requests: List[dict]) -> List[str]:
        """requests: [{messages, max_tokens, temperature, top_p, top_k,
        seed, adapter}] -> completion texts (one batched generation; the
        optional "adapter", and on a device-sampling engine the sampling
        parameters, are chosen per request)."""
        prompts, budgets, samp = self._encode_requests(requests)
        names = self._request_adapters(requests)
        with self._stream_ctx():
            outs = self._generate_batch(prompts, max(budgets), samp,
                                        budgets=budgets, adapters=names)
        return [self.tok.decode(o) for o in outs]

    def chat_batch_stream(self, requests: List[dict]):
        """Batched STREAMING generation: yields (row_index, text_delta)
        as tokens decode, then (row_index, None) when a row finishes.
        Deltas per row concatenate to exactly chat_batch()'s text (the
        same U+FFFD holdback as chat_stream)."""
        prompts, budgets, samp = self._encode_requests(requests)
        names = self._request_adapters(requests)
        n = len(requests)
        ids = [[] for _ in range(n)]
        sent = [""] * n
        with self._stream_ctx():
            for emitted in self._generate_batch_steps(
                    prompts, max(budgets), samp, budgets=budgets,
                    adapters=names):
                for i, t in emitted:      # at most one token per row
                    ids[i].append(t)
                    delta, sent[i] = self._delta(ids[i], sent[i])
                    if delta:
                        yield i, delta
        for i in range(n):
            delta, sent[i] = self._delta(ids[i], sent[i], final=True)
            if delta:
                yield i, delta
            yield i, None

    # ----------------------------------------------------------- score
    @torch.no_grad()
    def perplexity(self, texts: List[str],
                   adapter: Optional[str] = None) -> float:
        gi = self._adapter_index(adapter)
        with self._stream_ctx():
            return self._perplexity(texts, gi)

    def _perplexity(self, texts: List[str], gi: int = -1) -> float:
        """Mean perplexity over texts (built-in Scoring metric)."""
        akw = self._selection([gi])
        losses = []
        for t in texts:
            ids = [self.tok.bos_token_id] + self.tok.encode(t)
            ids = ids[:512]
            if len(ids) < 2:
                continue
            x = torch.tensor([ids], dtype=torch.long, device=self.device)
            loss = self.model(x, labels=x, **akw)
            losses.append(float(loss))
        if not losses:
            return float("inf")
        mean = sum(losses) / len(losses)
        return math.exp(min(mean, 30.0))
