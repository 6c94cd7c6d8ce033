"""Controller/state-machine tests against the file store with real
(CPU, tiny-model) trainer and serve processes — the envtest-style
integration the reference never had (SURVEY.md §4 a/b)."""

import os
import time

import pytest
import yaml

from datatunerx_amd.api.controllers import ManagerConfig
from datatunerx_amd.api.manager import Manager
from datatunerx_amd.api.store import Store
from datatunerx_amd.api.types import (Dataset, Finetune, FinetuneExperiment,
                                      FinetuneJob, Hyperparameter, LLM,
                                      LLMCheckpoint, Scoring,
                                      merge_hyperparameters)

_PORT = [31000 + (os.getpid() % 500) * 7]
_MANAGERS = []


def mk_manager(tmp_path, n_gpus=0):
    _PORT[0] += 50
    cfg = ManagerConfig(state_dir=str(tmp_path / "state"),
                        work_dir=str(tmp_path / "work"),
                        n_gpus=8, cpu_mode=True, base_port=_PORT[0],
                        storage_path=str(tmp_path / "storage"))
    mgr = Manager(cfg)
    _MANAGERS.append(mgr)
    return mgr


@pytest.fixture(autouse=True)
def _kill_spawned_processes():
    """Kill (by exact pid, from store statuses) every process a test's
    manager spawned, even when the test fails mid-pipeline."""
    yield
    while _MANAGERS:
        mgr = _MANAGERS.pop()
        pids = []
        for cls in (Finetune, FinetuneJob):
            for obj in mgr.store.list(cls):
                info = obj.status.get("trainJobInfo") or {}
                pids += info.get("pids", [])
                sinfo = obj.status.get("serveInfo") or {}
                if sinfo.get("pid"):
                    pids.append(sinfo["pid"])
        for pid in pids:
            try:
                os.kill(pid, 15)
            except OSError:
                pass


def seed_resources(store, hp_params=None):
    store.create(LLM(name="llama-tiny", spec={"family": "llama"}))
    params = {"learningRate": "1e-3", "epochs": 1, "blockSize": 64,
              "batchSize": 2, "loRA_R": 4, "loRA_Alpha": 8,
              "loRA_Dropout": "0.0", "scheduler": "cosine",
              "optimizer": "adamw_torch", "maxSteps": 2,
              "syntheticExamples": 16}
    params.update(hp_params or {})
    store.create(Hyperparameter(name="hp", spec={"parameters": params}))
    store.create(Dataset(name="ds", spec={
        "datasetMetadata": {"datasetInfo": {
            "subsets": [{"splits": {"train": {"file": ""}}}],
            "features": [{"name": "instruction", "mapTo": "instruction"},
                         {"name": "response", "mapTo": "response"}],
        }}}))


def finetune_spec():
    return {"llm": "llama-tiny", "dataset": "ds",
            "hyperparameter": {"hyperparameterRef": "hp"}, "node": 1}


def test_hyperparameter_override_merge():
    base = {"learningRate": "1e-4", "epochs": 2, "int4": False}
    ov = {"learningRate": "5e-5", "epochs": None}
    out = merge_hyperparameters(base, ov)
    assert out["learningRate"] == "5e-5"
    assert out["epochs"] == 2


def test_store_crud_and_gc(tmp_path):
    store = Store(str(tmp_path))
    llm = LLM(name="m1", spec={"a": 1})
    store.create(llm)
    got = store.get(LLM, "default", "m1")
    assert got.spec == {"a": 1}
    child = Finetune(name="c1", spec=finetune_spec())
    child.set_owner(llm)
    store.create(child)
    store.delete(LLM, "default", "m1")
    store.gc_sweep()
    assert store.try_get(Finetune, "default", "c1") is None


def test_finetune_cascade_to_checkpoint(tmp_path):
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    ft = Finetune(name="ft1", spec=finetune_spec())
    mgr.store.create(ft)
    deadline = time.time() + 240
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(Finetune, "default", "ft1")
        if cur.status.get("state") in ("Successful", "Failed"):
            break
        time.sleep(0.3)
    cur = mgr.store.get(Finetune, "default", "ft1")
    assert cur.status.get("state") == "Successful", cur.status
    ck = mgr.store.get(LLMCheckpoint, "default", "ft1-checkpoint")
    path = ck.spec["checkpoint"]
    assert os.path.exists(os.path.join(path, "adapter_model.safetensors"))
    assert ck.spec["llm"]["llmRef"] == "llama-tiny"


def test_finetune_failure_propagates(tmp_path):
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    spec = finetune_spec()
    spec["llm"] = "nonexistent-model"     # trainer will exit nonzero
    ft = Finetune(name="ftbad", spec=spec)
    mgr.store.create(ft)
    deadline = time.time() + 120
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(Finetune, "default", "ftbad")
        if cur.status.get("state") in ("Successful", "Failed"):
            break
        time.sleep(0.3)
    assert mgr.store.get(Finetune, "default",
                         "ftbad").status["state"] == "Failed"


def test_job_precondition_backrefs(tmp_path):
    mgr = mk_manager(tmp_path)
    # no resources yet: job must wait (ErrRecalibrate path)
    job = FinetuneJob(name="j1", spec={
        "fineTune": {"finetuneSpec": finetune_spec()}})
    mgr.store.create(job)
    mgr.reconcile_once()
    assert mgr.store.get(FinetuneJob, "default",
                         "j1").status.get("state", "") == ""
    seed_resources(mgr.store)
    mgr._not_before.clear()     # skip the requeue backoff in tests
    mgr.reconcile_once()
    mgr.reconcile_once()
    llm = mgr.store.get(LLM, "default", "llama-tiny")
    assert "j1" in llm.status.get("referenceFinetuneName", [])


@pytest.mark.slow
def test_full_job_pipeline_with_serve_and_scoring(tmp_path):
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    job = FinetuneJob(name="job1", spec={
        "fineTune": {"finetuneSpec": finetune_spec()}})
    mgr.store.create(job)
    deadline = time.time() + 300
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(FinetuneJob, "default", "job1")
        if cur.status.get("state") in ("Successful", "Failed"):
            break
        time.sleep(0.3)
    cur = mgr.store.get(FinetuneJob, "default", "job1")
    assert cur.status.get("state") == "Successful", cur.status
    res = cur.status.get("result", {})
    assert res.get("modelExportResult") is True
    assert res.get("serve", "").startswith("http://")
    assert res.get("score") is not None
    sc = mgr.store.get(Scoring, "default", "job1-scoring")
    assert sc.status.get("score") == res["score"]
    # serve process torn down after scoring
    pid = cur.status["serveInfo"]["pid"]
    time.sleep(1.0)
    for _ in range(20):
        try:
            os.kill(pid, 0)
            time.sleep(0.5)
        except OSError:
            break
    else:
        pytest.fail("serve process still alive")


def test_experiment_fanout_best_version(tmp_path):
    """configs[3] shape: a FinetuneExperiment fans out concurrent jobs
    (lr sweep via hyperparameter overrides), aggregates their statuses
    and picks bestVersion by descending score
    (finetuneexperiment_controller.go:123-216)."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    spec_a = finetune_spec()
    spec_b = finetune_spec()
    spec_b["hyperparameter"]["overrides"] = {"learningRate": "5e-4"}
    exp = FinetuneExperiment(name="exp2", spec={
        "finetuneJobs": [
            {"name": "e2-j1", "spec": {"fineTune":
                                       {"finetuneSpec": spec_a}}},
            {"name": "e2-j2", "spec": {"fineTune":
                                       {"finetuneSpec": spec_b}}},
        ]})
    mgr.store.create(exp)
    deadline = time.time() + 300
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(FinetuneExperiment, "default", "exp2")
        if cur.status.get("state") in ("Success", "Failed"):
            break
        time.sleep(0.3)
    cur = mgr.store.get(FinetuneExperiment, "default", "exp2")
    assert cur.status.get("state") == "Success", cur.status
    assert len(cur.status["jobsStatus"]) == 2
    best = cur.status.get("bestVersion")
    assert best and best.get("llm") == "llama-tiny"
    scores = [_int_score(js["finetuneJobStatus"].get("result", {})
                         .get("score"))
              for js in cur.status["jobsStatus"]
              if js["finetuneJobStatus"].get("state") == "Successful"]
    assert _int_score(best["score"]) == max(scores)
    # jobs were gang-scheduled through the shared GPU inventory: both
    # jobs' finetunes reached Successful
    for name in ("e2-j1", "e2-j2"):
        st = mgr.store.get(FinetuneJob, "default", name).status
        assert st.get("state") in ("Successful", "Failed")


def _int_score(s):
    try:
        return int(float(s))
    except (TypeError, ValueError):
        return -1


def test_experiment_pending_pause(tmp_path):
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    exp = FinetuneExperiment(name="exp1", spec={
        "pending": True,
        "finetuneJobs": [{"name": "e1-j1",
                          "spec": {"fineTune":
                                   {"finetuneSpec": finetune_spec()}}}]})
    mgr.store.create(exp)
    mgr.reconcile_once()
    assert mgr.store.get(FinetuneExperiment, "default",
                         "exp1").status["state"] == "Pending"
    assert mgr.store.try_get(FinetuneJob, "default", "e1-j1") is None


def test_cli_apply_and_get(tmp_path, capsys):
    from datatunerx_amd.cli import main as cli
    manifest = {
        "apiVersion": "core.datatunerx.io/v1beta1", "kind": "LLM",
        "metadata": {"name": "m2", "namespace": "default"},
        "spec": {"family": "llama"}}
    f = tmp_path / "m.yaml"
    f.write_text(yaml.safe_dump(manifest))
    cli(["--state-dir", str(tmp_path / "s"), "apply", "-f", str(f)])
    cli(["--state-dir", str(tmp_path / "s"), "get", "llm"])
    out = capsys.readouterr().out
    assert "m2" in out


def test_admission_validation(tmp_path):
    """Webhook parity: invalid objects rejected at create with every
    problem listed; defaults filled (controller_manager.go:112-135)."""
    from datatunerx_amd.api.store import Store
    from datatunerx_amd.api.validation import ValidationError
    store = Store(str(tmp_path / "s"))
    with pytest.raises(ValidationError, match="llm is required"):
        store.create(FinetuneJob(name="bad", spec={
            "fineTune": {"finetuneSpec": {"dataset": "d",
                                          "hyperparameter":
                                          {"hyperparameterRef": "h"}}}}))
    with pytest.raises(ValidationError, match="DNS-1123"):
        store.create(LLM(name="Bad_Name", spec={}))
    with pytest.raises(ValidationError, match="mutually exclusive"):
        store.create(Hyperparameter(name="hpx", spec={
            "parameters": {"int4": True, "int8": True}}))
    with pytest.raises(ValidationError, match="non-empty"):
        store.create(FinetuneExperiment(name="e", spec={
            "finetuneJobs": []}))
    # defaults: node filled, scoring config defaulted
    job = FinetuneJob(name="ok", spec={
        "fineTune": {"finetuneSpec": finetune_spec()}})
    store.create(job)
    got = store.get(FinetuneJob, "default", "ok")
    assert got.spec["scoringPluginConfig"]["name"] == "builtin"
    assert got.spec["fineTune"]["finetuneSpec"]["node"] == 1


def test_manager_metrics_endpoint(tmp_path):
    """/metrics + /healthz (controller-runtime :8080 parity)."""
    import urllib.request
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    mgr.reconcile_once()
    srv = mgr.serve_metrics(port=0)      # OS-assigned (no collisions)
    try:
        url = f"http://127.0.0.1:{srv.server_address[1]}"
        assert urllib.request.urlopen(url + "/healthz",
                                      timeout=10).read() == b"ok"
        text = urllib.request.urlopen(url + "/metrics",
                                      timeout=10).read().decode()
        assert "dtx_reconcile_total" in text
    finally:
        srv.shutdown()


def test_finetune_restart_policy(tmp_path):
    """spec.restartPolicy.maxRetries relaunches a crashed trainer before
    declaring Failed (bounded elasticity; improvement over the
    reference's propagate-only failure handling)."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    spec = finetune_spec()
    spec["llm"] = "nonexistent-model"         # trainer exits nonzero
    spec["restartPolicy"] = {"maxRetries": 2}
    ft = Finetune(name="ftretry", spec=spec)
    mgr.store.create(ft)
    deadline = time.time() + 180
    while time.time() < deadline:
        mgr._not_before.clear()
        mgr.reconcile_once()
        cur = mgr.store.get(Finetune, "default", "ftretry")
        if cur.status.get("state") == "Failed":
            break
        time.sleep(0.2)
    cur = mgr.store.get(Finetune, "default", "ftretry")
    assert cur.status.get("state") == "Failed"
    assert cur.status.get("restarts") == 2


def test_cli_run_one_shot(tmp_path, capsys):
    """`dtx run -f ...` applies manifests, reconciles to completion and
    prints final states (dtx-ctl-style one-shot)."""
    from datatunerx_amd.cli import main as cli
    _PORT[0] += 50
    st = str(tmp_path / "s")
    store = Store(st)
    seed_resources(store)
    man = {
        "apiVersion": "finetune.datatunerx.io/v1beta1",
        "kind": "FinetuneJob",
        "metadata": {"name": "clijob", "namespace": "default"},
        "spec": {"fineTune": {"finetuneSpec": finetune_spec()}}}
    f = tmp_path / "job.yaml"
    f.write_text(yaml.safe_dump(man))
    import datatunerx_amd.api.controllers as C
    with pytest.raises(SystemExit) as e:
        cli(["--state-dir", st, "run", "-f", str(f),
             "--work-dir", str(tmp_path / "w"), "--timeout", "300"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "finetunejob/clijob: Successful" in out


@pytest.mark.slow
def test_tp_serve_pipeline(tmp_path):
    """serveConfig.tensorParallel=2: the controller launches a 2-rank TP
    service through the supervisor (gloo on CPU), rank 0 serves HTTP,
    scoring completes against it, and BOTH rank processes are reaped at
    teardown (configs[4]'s inference-compare shape)."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    job = FinetuneJob(name="tpjob", spec={
        "fineTune": {"finetuneSpec": finetune_spec()},
        "serveConfig": {"tensorParallel": 2}})
    mgr.store.create(job)
    deadline = time.time() + 300
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(FinetuneJob, "default", "tpjob")
        if cur.status.get("state") in ("Successful", "Failed"):
            break
        time.sleep(0.3)
    cur = mgr.store.get(FinetuneJob, "default", "tpjob")
    assert cur.status.get("state") == "Successful", cur.status
    assert cur.status.get("result", {}).get("score") is not None
    pids = cur.status["serveInfo"]["pids"]
    assert len(pids) == 2
    for pid in pids:
        for _ in range(20):
            try:
                os.kill(pid, 0)
                time.sleep(0.5)
            except OSError:
                break
        else:
            pytest.fail(f"serve rank pid {pid} still alive")


@pytest.mark.slow
def test_gang_node2_trains_both_ranks(tmp_path):
    """node=2 Finetune through the controller + supervisor: two trainer
    rank processes launch (gloo rendezvous over 127.0.0.1), both rank
    logs exist, training succeeds."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    spec = finetune_spec()
    spec["node"] = 2
    ft = Finetune(name="ft2rank", spec=spec)
    mgr.store.create(ft)
    deadline = time.time() + 240
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(Finetune, "default", "ft2rank")
        if cur.status.get("state") in ("Successful", "Failed"):
            break
        time.sleep(0.3)
    cur = mgr.store.get(Finetune, "default", "ft2rank")
    assert cur.status.get("state") == "Successful", cur.status
    info = cur.status["trainJobInfo"]
    assert len(info["pids"]) == 2
    log_dir = info["logDir"]
    assert os.path.exists(os.path.join(log_dir, "rank0.log"))
    assert os.path.exists(os.path.join(log_dir, "rank1.log"))
    # world_size=2 rendezvous really happened (rank 1 trained too)
    assert os.path.getsize(os.path.join(log_dir, "rank1.log")) > 0


def test_gang_inventory_all_or_nothing():
    """C++ GpuInventory: gang allocation is all-or-nothing; a gang that
    does not fit queues (empty result) until a release frees the GPUs."""
    from datatunerx_amd.native import _dtx_native
    inv = _dtx_native.GpuInventory(4)
    a = inv.allocate(2, "job-a")
    b = inv.allocate(2, "job-b")
    assert len(a) == 2 and len(b) == 2 and not set(a) & set(b)
    assert inv.allocate(1, "job-c") == []      # full: queued, nothing held
    inv.release_owner("job-a")
    c = inv.allocate(2, "job-c")
    assert sorted(c) == sorted(a)


@pytest.mark.slow
def test_serve_concurrent_requests(tmp_path):
    """The engine pool serves concurrent /chat/completions correctly:
    two simultaneous requests return the same (greedy) completions as
    sequential ones."""
    import json as _json
    import threading
    import urllib.request

    import torch

    from datatunerx_amd.serve.engine import InferenceEngine, build_model
    from datatunerx_amd.serve.server import (EnginePool, build_handler)
    from http.server import ThreadingHTTPServer

    model = build_model("llama-tiny", torch.device("cpu"))
    pool = EnginePool([InferenceEngine(model, template="vanilla",
                                       device=torch.device("cpu"))
                       for _ in range(2)])
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), build_handler(pool))
    port = httpd.server_address[1]
    t = threading.Thread(target=httpd.serve_forever, daemon=True)
    t.start()
    try:
        def ask(content):
            req = urllib.request.Request(
                f"http://127.0.0.1:{port}/chat/completions",
                data=_json.dumps({
                    "messages": [{"role": "user", "content": content}],
                    "max_tokens": 8, "temperature": 0.0}).encode(),
                headers={"Content-Type": "application/json"})
            with urllib.request.urlopen(req, timeout=60) as r:
                return _json.load(r)["choices"][0]["message"]["content"]

        seq = [ask("alpha"), ask("beta")]
        results = [None, None]

        def worker(i, content):
            results[i] = ask(content)

        ts = [threading.Thread(target=worker, args=(0, "alpha")),
              threading.Thread(target=worker, args=(1, "beta"))]
        for th in ts:
            th.start()
        for th in ts:
            th.join(timeout=120)
        assert results == seq
    finally:
        httpd.shutdown()


def test_generate_batch_matches_sequential():
    """Ragged batched decode == per-request greedy generation (the
    batching front's correctness contract)."""
    import torch

    from datatunerx_amd.serve.engine import InferenceEngine, build_model
    model = build_model("llama-tiny", torch.device("cpu"))
    eng = InferenceEngine(model, template="vanilla",
                          device=torch.device("cpu"))
    prompts = [eng.tok.encode("hello world", add_special_tokens=True),
               eng.tok.encode("a much longer prompt with many words",
                              add_special_tokens=True),
               eng.tok.encode("x", add_special_tokens=True)]
    batched = eng.generate_batch(prompts, max_new_tokens=12)
    seq = [eng.generate(p, max_new_tokens=12) for p in prompts]
    assert batched == seq


def test_kv_cache_modes_agree():
    """One counter-backed cache (right-padded prefill, then device-mode
    single-token updates at per-row positions) holds, row by row, exactly
    what B = 1 host-mode caches hold, and attention over it with the
    per-row lengths gives exactly the per-row result."""
    import torch

    from datatunerx_amd.ops.autograd import attention
    from datatunerx_amd.serve.engine import KVCache, _DecodeState
    B, Hq, Hkv, D, max_s, lens = 3, 4, 2, 64, 16, [1, 5, 3]
    cpu = torch.device("cpu")
    g = torch.Generator().manual_seed(0)

    def rand(*shape):
        return torch.randn(*shape, generator=g)

    st = _DecodeState(B, Hkv, max_s, D, 1, cpu, torch.float32)
    cache = st.caches[0]
    kp, vp = rand(B, max(lens), Hkv, D), rand(B, max(lens), Hkv, D)
    assert cache.update(kp, vp)[2] is None       # pads hold random k/v
    st.set_state(lens)
    hosts = [KVCache(1, Hkv, max_s, D, cpu, torch.float32)
             for _ in range(B)]
    for b, h in enumerate(hosts):
        h.update(kp[b:b + 1, :lens[b]], vp[b:b + 1, :lens[b]])
    def check_counters():
        # len == pos + 1; the cache write index is pos in row b's slots
        assert torch.equal(st.len32, st.pos32 + 1)
        assert torch.equal(st.wpos, torch.arange(B) * max_s + st.pos32)

    for step in range(1, 4):
        check_counters()
        q, k1, v1 = rand(B, 1, Hq, D), rand(B, 1, Hkv, D), \
            rand(B, 1, Hkv, D)
        k, v, len_dev = cache.update(k1, v1)
        assert len_dev is st.len32
        assert len_dev.tolist() == [n + step for n in lens]
        o = attention(q, k, v, len_dev=len_dev)
        for b, h in enumerate(hosts):
            hk, hv, none = h.update(k1[b:b + 1], v1[b:b + 1])
            assert none is None and hk.shape[1] == lens[b] + step
            assert torch.equal(k[b:b + 1, :hk.shape[1]], hk)
            assert torch.equal(v[b:b + 1, :hv.shape[1]], hv)
            assert torch.equal(o[b:b + 1], attention(q[b:b + 1], hk, hv))
        st.advance()
    check_counters()


def test_one_token_batch_and_stream_terminators():
    """A batch whose prompts are all ONE token long (its prefill is a
    single-token update of an empty cache) matches per-request
    generation; every row of a batched stream ends with exactly one
    (row, None), after that row's last delta."""
    import torch

    from datatunerx_amd.serve.engine import InferenceEngine, build_model
    model = build_model("llama-tiny", torch.device("cpu"))
    eng = InferenceEngine(model, template="vanilla",
                          device=torch.device("cpu"))
    assert eng.generate_batch([[5], [6]], max_new_tokens=4) == \
        [eng.generate([5], max_new_tokens=4),
         eng.generate([6], max_new_tokens=4)]
    reqs = [{"messages": [{"role": "user", "content": c}],
             "max_tokens": n} for c, n in (("alpha", 3), ("beta", 6))]
    events = list(eng.chat_batch_stream(reqs))
    for i in range(len(reqs)):
        row = [d for r, d in events if r == i]
        assert row.count(None) == 1 and row[-1] is None, events
        assert "".join(row[:-1]) == eng.chat_batch(reqs)[i]


@pytest.mark.slow
def test_serve_batched_requests_match_sequential(tmp_path):
    """Concurrent non-streaming requests through the BatchingFront give
    the same greedy completions as sequential single requests."""
    import json as _json
    import threading
    import urllib.request

    import torch

    from datatunerx_amd.serve.engine import InferenceEngine, build_model
    from datatunerx_amd.serve.server import (BatchingFront, EnginePool,
                                             build_handler)
    from http.server import ThreadingHTTPServer

    model = build_model("llama-tiny", torch.device("cpu"))
    pool = EnginePool([InferenceEngine(model, template="vanilla",
                                       device=torch.device("cpu"))])
    batcher = BatchingFront(
        InferenceEngine(model, template="vanilla",
                        device=torch.device("cpu")), max_batch=4,
        linger=0.05)
    httpd = ThreadingHTTPServer(("127.0.0.1", 0),
                                build_handler(pool, batcher))
    port = httpd.server_address[1]
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    try:
        def ask(content, n=8):
            req = urllib.request.Request(
                f"http://127.0.0.1:{port}/chat/completions",
                data=_json.dumps({
                    "messages": [{"role": "user", "content": content}],
                    "max_tokens": n, "temperature": 0.0}).encode(),
                headers={"Content-Type": "application/json"})
            with urllib.request.urlopen(req, timeout=120) as r:
                return _json.load(r)["choices"][0]["message"]["content"]

        seq = [ask("alpha"), ask("beta"), ask("gamma")]
        results = [None] * 3

        def worker(i, c):
            results[i] = ask(c)

        ts = [threading.Thread(target=worker, args=(i, c))
              for i, c in enumerate(["alpha", "beta", "gamma"])]
        for th in ts:
            th.start()
        for th in ts:
            th.join(timeout=180)
        assert results == seq
    finally:
        httpd.shutdown()


def test_serve_batched_stream_matches_batch(tmp_path):
    """Streamed requests join the batch: concurrent SSE streams through
    the BatchingFront concatenate to the same greedy completions."""
    import json as _json
    import threading
    import urllib.request

    import torch

    from datatunerx_amd.serve.engine import InferenceEngine, build_model
    from datatunerx_amd.serve.server import (BatchingFront, EnginePool,
                                             build_handler)
    from http.server import ThreadingHTTPServer

    model = build_model("llama-tiny", torch.device("cpu"))
    pool = EnginePool([InferenceEngine(model, template="vanilla",
                                       device=torch.device("cpu"))])
    batcher = BatchingFront(
        InferenceEngine(model, template="vanilla",
                        device=torch.device("cpu")), max_batch=4,
        linger=0.05)
    httpd = ThreadingHTTPServer(("127.0.0.1", 0),
                                build_handler(pool, batcher))
    port = httpd.server_address[1]
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    try:
        def ask(content, stream):
            data = {"messages": [{"role": "user", "content": content}],
                    "max_tokens": 8, "temperature": 0.0}
            if stream:
                data["stream"] = True
            req = urllib.request.Request(
                f"http://127.0.0.1:{port}/chat/completions",
                data=_json.dumps(data).encode(),
                headers={"Content-Type": "application/json"})
            with urllib.request.urlopen(req, timeout=120) as r:
                if not stream:
                    return _json.load(r)["choices"][0]["message"][
                        "content"]
                text = ""
                for line in r:
                    line = line.decode().strip()
                    if line.startswith("data: ") and \
                            line != "data: [DONE]":
                        text += _json.loads(line[6:])["choices"][0][
                            "delta"]["content"]
                return text

        want = [ask("alpha", False), ask("beta", False)]
        got = [None, None]

        def worker(i, c):
            got[i] = ask(c, True)

        ts = [threading.Thread(target=worker, args=(i, c))
              for i, c in enumerate(["alpha", "beta"])]
        for th in ts:
            th.start()
        for th in ts:
            th.join(timeout=120)
        assert got == want
    finally:
        httpd.shutdown()


def test_builtin_model_registry_covers_all_serve_names():
    """Every builtin model name the platform advertises resolves to a
    config through the ONE registry the engine and the TP server share
    (a llama3-8b serve request once failed only on GPU because the
    engine's name list had drifted from the server's)."""
    from datatunerx_amd.serve.engine import builtin_config
    from datatunerx_amd.serve.server import _llama_config
    names = ["llama2-7b", "llama-2-7b", "llama2-13b", "llama-2-13b",
             "llama3-8b", "llama-3-8b", "llama-tiny", "llama-mini",
             "gpt2-small", "gpt2", "gpt2-tiny"]
    for n in names:
        family, cfg = builtin_config(n)
        assert cfg.vocab_size > 0
        if family == "llama":
            assert _llama_config(n) is not None
    with pytest.raises(ValueError):
        builtin_config("no-such-model")
    with pytest.raises(ValueError):
        _llama_config("gpt2-small")
    # GQA geometry reaches the engine path for llama3
    _, c3 = builtin_config("llama3-8b", lora_r=4)
    assert c3.num_key_value_heads == 8 and c3.lora_r == 4


def test_sampler_temperature_and_top_p():
    """Sampler unit behavior: temperature=0 is argmax; top_p keeps only
    the smallest prefix of the sorted distribution; temperature>0 draws
    only from kept tokens."""
    import torch

    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import InferenceEngine
    m = LlamaForCausalLM(LlamaConfig.tiny(), lora=False,
                         dtype=torch.float32)
    eng = InferenceEngine(m, template="vanilla",
                          device=torch.device("cpu"))
    logits = torch.tensor([0.1, 3.0, 2.0, -1.0, 0.5])
    assert eng._sample(logits, 0.0, 1.0) == 1
    torch.manual_seed(0)
    # top_p=0.5: after softmax(T=0.5) token 1 dominates; only it is kept
    for _ in range(20):
        assert eng._sample(logits, 0.5, 0.5) == 1
    # temperature high, top_p=0.9: draws restricted to the top mass
    torch.manual_seed(1)
    seen = {eng._sample(logits, 1.5, 0.9) for _ in range(200)}
    assert 3 not in seen          # lowest-probability token filtered out
    assert 1 in seen and len(seen) >= 2


def test_dpo_job_pipeline(tmp_path):
    """A FinetuneJob whose Hyperparameter requests stage=dpo runs the
    DPO trainer through the full control plane (train -> checkpoint ->
    build -> serve -> score) on synthetic preference data."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store, hp_params={"stage": "dpo",
                                         "dpoBeta": "0.2",
                                         "loRA_Dropout": "0.0"})
    job = FinetuneJob(name="dpojob", spec={
        "fineTune": {"finetuneSpec": finetune_spec()}})
    mgr.store.create(job)
    deadline = time.time() + 300
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(FinetuneJob, "default", "dpojob")
        if cur.status.get("state") in ("Successful", "Failed"):
            break
        time.sleep(0.3)
    cur = mgr.store.get(FinetuneJob, "default", "dpojob")
    assert cur.status.get("state") == "Successful", cur.status
    # the trained artifact is a LoRA adapter (DPO trains adapters only)
    ft = mgr.store.get(Finetune, "default", "dpojob-finetune")
    ck = (ft.status.get("llmCheckpoint") or {}).get("checkpointPath")
    assert ck and os.path.exists(os.path.join(ck,
                                              "adapter_model.safetensors"))


def test_validation_rejects_bad_stage(tmp_path):
    from datatunerx_amd.api.validation import validate_
    from datatunerx_amd.api.types import Hyperparameter
    hp = Hyperparameter(name="h", spec={"parameters": {"stage": "ppo"}})
    with pytest.raises(Exception, match="stage"):
        validate_(hp)
    validate_(Hyperparameter(name="h2",
                             spec={"parameters": {"stage": "dpo"}}))


def test_openai_compat_endpoints(tmp_path):
    """OpenAI-SDK-shaped clients work: GET /v1/models lists the served
    model and POST /v1/chat/completions aliases /chat/completions."""
    import http.client
    import json
    import threading
    from http.server import ThreadingHTTPServer

    import torch

    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import InferenceEngine
    from datatunerx_amd.serve.server import build_handler
    m = LlamaForCausalLM(LlamaConfig.tiny(), lora=False,
                         dtype=torch.float32)
    m.init_random(seed=1)
    eng = InferenceEngine(m, template="vanilla",
                          device=torch.device("cpu"))
    httpd = ThreadingHTTPServer(("127.0.0.1", 0),
                                build_handler(eng, model_name="llama-tiny"))
    port = httpd.server_address[1]
    t = threading.Thread(target=httpd.serve_forever, daemon=True)
    t.start()
    try:
        c = http.client.HTTPConnection("127.0.0.1", port, timeout=30)
        c.request("GET", "/v1/models")
        r = json.loads(c.getresponse().read())
        assert r["data"][0]["id"] == "llama-tiny"
        body = json.dumps({"messages": [{"role": "user",
                                         "content": "hi"}],
                           "max_tokens": 4})
        c.request("POST", "/v1/chat/completions", body=body)
        r1 = json.loads(c.getresponse().read())
        c.request("POST", "/chat/completions", body=body)
        r2 = json.loads(c.getresponse().read())
        assert r1["choices"][0]["message"]["content"] == \
            r2["choices"][0]["message"]["content"]
    finally:
        httpd.shutdown()


def test_serve_rejects_malformed_requests(tmp_path):
    """Malformed /chat/completions bodies get clean 400s, valid ones
    still work, and the server survives all of them."""
    import http.client
    import json as _json
    import threading
    from http.server import ThreadingHTTPServer

    import torch

    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import InferenceEngine
    from datatunerx_amd.serve.server import build_handler
    m = LlamaForCausalLM(LlamaConfig.tiny(), lora=False,
                         dtype=torch.float32)
    m.init_random(seed=1)
    eng = InferenceEngine(m, template="vanilla",
                          device=torch.device("cpu"))
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), build_handler(eng))
    port = httpd.server_address[1]
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    try:
        def post(obj):
            c = http.client.HTTPConnection("127.0.0.1", port, timeout=30)
            c.request("POST", "/chat/completions",
                      body=_json.dumps(obj) if not isinstance(obj, bytes)
                      else obj)
            r = c.getresponse()
            return r.status, r.read()
        for bad in [{"messages": [{}]},
                    {"messages": "hi"},
                    {"messages": [{"role": 1, "content": "x"}]},
                    {"messages": [{"role": "user", "content": None}]},
                    {"messages": [{"role": "user", "content": "x"}],
                     "max_tokens": "many"},
                    []]:
            st, _ = post(bad)
            assert st == 400, (bad, st)
        st, _ = post(b"not json at all")
        assert st == 400
        st, body = post({"messages": [{"role": "user", "content": "hi"}],
                         "max_tokens": 4})
        assert st == 200 and b"choices" in body
    finally:
        httpd.shutdown()


def test_engine_rejects_empty_prompts():
    import torch

    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import InferenceEngine
    m = LlamaForCausalLM(LlamaConfig.tiny(), lora=False,
                         dtype=torch.float32)
    eng = InferenceEngine(m, template="vanilla",
                          device=torch.device("cpu"))
    with pytest.raises(ValueError, match="empty"):
        eng.generate([], max_new_tokens=2)
    with pytest.raises(ValueError, match="empty"):
        eng.generate_batch([[1, 2], []], max_new_tokens=2)


def test_multiturn_chat_history_assembly():
    """chat() folds prior (user, assistant) turns through the template's
    multiturn encoding — the prompt contains all turns in order."""
    import torch

    from datatunerx_amd.data.dataset import ByteTokenizer
    from datatunerx_amd.data.templates import get_template
    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import InferenceEngine
    m = LlamaForCausalLM(LlamaConfig.tiny(), lora=False,
                         dtype=torch.float32)
    m.init_random(seed=0)
    eng = InferenceEngine(m, template="llama2",
                          device=torch.device("cpu"))
    msgs = [{"role": "system", "content": "be brief"},
            {"role": "user", "content": "first q"},
            {"role": "assistant", "content": "first a"},
            {"role": "user", "content": "second q"}]
    seen = {}
    orig = eng.generate

    def spy(src, *a, **kw):
        seen["src"] = list(src)
        return orig(src, *a, **kw)
    eng.generate = spy
    eng.chat(msgs, max_tokens=2)
    t = get_template("llama2")
    want, _ = t.encode_oneturn(ByteTokenizer(), "second q", "",
                               [("first q", "first a")], "be brief")
    assert seen["src"] == want
    text = ByteTokenizer().decode(seen["src"])
    assert text.index("first q") < text.index("first a") < \
        text.index("second q")
    assert "be brief" in text


def test_cli_logs_command(tmp_path, capsys):
    """`dtx logs <job>` prints the trainer's jsonl step log from the
    manager's work dir (finds the job's Finetune child by suffix)."""
    import json as _json

    from datatunerx_amd.cli import main as cli
    work = tmp_path / "w" / "default" / "myjob-finetune" / "output" / \
        "watch"
    os.makedirs(work)
    with open(work / "trainer_log.jsonl", "w") as f:
        for i in range(5):
            f.write(_json.dumps({"current_steps": i + 1,
                                 "loss": 1.0 / (i + 1)}) + "\n")
    st = str(tmp_path / "s")
    cli(["--state-dir", st, "logs", "myjob",
         "--work-dir", str(tmp_path / "w"), "--tail", "2"])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 2
    assert _json.loads(out[-1])["current_steps"] == 5
    with pytest.raises(SystemExit, match="no trainer log"):
        cli(["--state-dir", st, "logs", "nosuch",
             "--work-dir", str(tmp_path / "w")])


def test_plugin_scoring_pipeline(tmp_path):
    """scoringPluginConfig with loadPlugin: the job's score comes from a
    user 'module:function' plugin called with (endpoint, parameters) —
    the reference's plugin-scoring pod, in-process."""
    import sys
    plug_dir = tmp_path / "plugins"
    os.makedirs(plug_dir)
    with open(plug_dir / "dtx_test_scorer.py", "w") as f:
        f.write(
            "import json, urllib.request\n"
            "def my_score(endpoint, params):\n"
            "    # prove the endpoint is live AND params flow through\n"
            "    r = urllib.request.urlopen(endpoint + '/health',\n"
            "                               timeout=30)\n"
            "    assert json.loads(r.read())['status'] == 'ok'\n"
            "    return int(params['base']) + 7\n")
    sys.path.insert(0, str(plug_dir))
    try:
        mgr = mk_manager(tmp_path)
        seed_resources(mgr.store)
        job = FinetuneJob(name="plugjob", spec={
            "fineTune": {"finetuneSpec": finetune_spec()},
            "scoringPluginConfig": {"name": "dtx_test_scorer:my_score",
                                    "parameters": {"base": 100}}})
        mgr.store.create(job)
        deadline = time.time() + 300
        while time.time() < deadline:
            mgr.reconcile_once()
            cur = mgr.store.get(FinetuneJob, "default", "plugjob")
            if cur.status.get("state") in ("Successful", "Failed"):
                break
            time.sleep(0.3)
        cur = mgr.store.get(FinetuneJob, "default", "plugjob")
        assert cur.status.get("state") == "Successful", cur.status
        assert cur.status["result"]["score"] == "107"
    finally:
        sys.path.remove(str(plug_dir))


def test_manager_restart_resumes_inflight_job(tmp_path):
    """Control-plane crash-restart: a NEW Manager over the same
    state/work dirs drives a job that was mid-training to Successful
    (the reference gets this from the apiserver; here the file-backed
    store + status files are the durable state)."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store, hp_params={"maxSteps": 6})
    job = FinetuneJob(name="rejob", spec={
        "fineTune": {"finetuneSpec": finetune_spec()}})
    mgr.store.create(job)
    # reconcile until the Finetune exists and training has LAUNCHED
    deadline = time.time() + 120
    launched = False
    while time.time() < deadline and not launched:
        mgr.reconcile_once()
        ft = mgr.store.try_get(Finetune, "default", "rejob-finetune")
        launched = bool(ft and ft.status.get("state") == "Running")
        time.sleep(0.2)
    assert launched
    del mgr                                     # "crash"

    mgr2 = mk_manager(tmp_path)                 # same dirs (mk_manager
    deadline = time.time() + 300                # is deterministic here)
    while time.time() < deadline:
        mgr2.reconcile_once()
        cur = mgr2.store.get(FinetuneJob, "default", "rejob")
        if cur.status.get("state") in ("Successful", "Failed"):
            break
        time.sleep(0.3)
    cur = mgr2.store.get(FinetuneJob, "default", "rejob")
    assert cur.status.get("state") == "Successful", cur.status


def test_batcher_separates_mixed_sampling_params(tmp_path):
    """A greedy request never rides in the same batched generation as a
    temperature-sampled one: concurrent mixed requests all succeed and
    the greedy ones return exactly the sequential greedy output."""
    import queue as _q
    import threading

    import torch

    from datatunerx_amd.models import LlamaConfig, LlamaForCausalLM
    from datatunerx_amd.serve.engine import InferenceEngine
    from datatunerx_amd.serve.server import BatchingFront
    m = LlamaForCausalLM(LlamaConfig.tiny(), lora=False,
                         dtype=torch.float32)
    m.init_random(seed=3)
    eng = InferenceEngine(m, template="vanilla",
                          device=torch.device("cpu"))
    # engine-level guard: mixed params in one batch are refused
    with pytest.raises(ValueError, match="share"):
        eng.chat_batch([
            {"messages": [{"role": "user", "content": "a"}],
             "max_tokens": 4, "temperature": 0.0},
            {"messages": [{"role": "user", "content": "b"}],
             "max_tokens": 4, "temperature": 0.9}])

    front = BatchingFront(eng, max_batch=8, linger=0.05)
    msgs = [{"role": "user", "content": "hello there"}]
    want = eng.chat(msgs, max_tokens=6)          # sequential greedy
    results = _q.Queue()

    def one(temp):
        try:
            results.put((temp, front.chat(msgs, 6, temp, 1.0)))
        except Exception as e:                   # pragma: no cover
            results.put((temp, e))
    threads = [threading.Thread(target=one, args=(t,))
               for t in (0.0, 0.0, 0.8, 0.0, 0.8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    outs = [results.get(timeout=10) for _ in range(5)]
    for temp, out in outs:
        assert not isinstance(out, Exception), out
        if temp == 0.0:
            assert out == want                   # greedy stayed greedy


def test_cli_apply_clean_errors(tmp_path, capsys):
    from datatunerx_amd.cli import main as cli
    st = str(tmp_path / "s")
    bad_yaml = tmp_path / "bad.yaml"
    bad_yaml.write_text("kind: [unclosed")
    with pytest.raises(SystemExit, match="invalid YAML"):
        cli(["--state-dir", st, "apply", "-f", str(bad_yaml)])
    bad_kind = tmp_path / "kind.yaml"
    bad_kind.write_text("kind: Nope\nmetadata: {name: x}\n")
    with pytest.raises(SystemExit, match="unknown kind"):
        cli(["--state-dir", st, "apply", "-f", str(bad_kind)])
    invalid = tmp_path / "invalid.yaml"
    invalid.write_text(
        "apiVersion: finetune.datatunerx.io/v1beta1\n"
        "kind: Hyperparameter\n"
        "metadata: {name: h}\n"
        "spec: {parameters: {stage: ppo}}\n")
    with pytest.raises(SystemExit, match="stage must be"):
        cli(["--state-dir", st, "apply", "-f", str(invalid)])


def test_experiment_mixed_stage_jobs(tmp_path):
    """Experiment fan-out where one job OVERRIDES the hyperparameter to
    stage=dpo: the override merge (updateHyperparameters parity) flows
    through to the trainer flags, both jobs finish, both score."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store, hp_params={"loRA_Dropout": "0.0"})
    spec_sft = finetune_spec()
    spec_dpo = finetune_spec()
    spec_dpo["hyperparameter"]["overrides"] = {"stage": "dpo",
                                               "dpoBeta": "0.3"}
    exp = FinetuneExperiment(name="expmix", spec={
        "finetuneJobs": [
            {"name": "mx-sft", "spec": {"fineTune":
                                        {"finetuneSpec": spec_sft}}},
            {"name": "mx-dpo", "spec": {"fineTune":
                                        {"finetuneSpec": spec_dpo}}},
        ]})
    mgr.store.create(exp)
    deadline = time.time() + 300
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(FinetuneExperiment, "default", "expmix")
        if cur.status.get("state") in ("Success", "Failed"):
            break
        time.sleep(0.3)
    cur = mgr.store.get(FinetuneExperiment, "default", "expmix")
    assert cur.status.get("state") == "Success", cur.status
    states = {js["name"]: js["finetuneJobStatus"].get("state")
              for js in cur.status["jobsStatus"]}
    assert states == {"mx-sft": "Successful", "mx-dpo": "Successful"}
    # the dpo job's override flowed to the trainer: its Finetune args
    # carry --stage dpo --dpo_beta 0.3; the sft job's don't
    ft_dpo = mgr.store.get(Finetune, "default", "mx-dpo-finetune")
    ft_sft = mgr.store.get(Finetune, "default", "mx-sft-finetune")
    ov = (ft_dpo.spec.get("hyperparameter") or {}).get("overrides") or {}
    assert ov.get("stage") == "dpo" and ov.get("dpoBeta") == "0.3", ov
    assert not ((ft_sft.spec.get("hyperparameter") or {})
                .get("overrides") or {})
    # both trained checkpoints exist (adapters in both stages)
    for ft in (ft_dpo, ft_sft):
        ck = (ft.status.get("llmCheckpoint") or {}).get("checkpointPath")
        assert ck and os.path.exists(
            os.path.join(ck, "adapter_model.safetensors")), ft.status


def test_delete_job_mid_training_cleans_up(tmp_path):
    """Deleting a FinetuneJob while training runs: the finalizer path
    stops the trainer process, releases the gang GPUs, strips
    back-references and removes the job + GC's its children."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store, hp_params={"maxSteps": 2000})  # long run
    job = FinetuneJob(name="deljob", spec={
        "fineTune": {"finetuneSpec": finetune_spec()}})
    mgr.store.create(job)
    deadline = time.time() + 120
    pid = None
    while time.time() < deadline and pid is None:
        mgr.reconcile_once()
        ft = mgr.store.try_get(Finetune, "default", "deljob-finetune")
        if ft and ft.status.get("state") == "Running":
            info = ft.status.get("trainJobInfo") or {}
            pids = info.get("pids") or []
            pid = pids[0] if pids else None
        time.sleep(0.2)
    assert pid is not None, "training never started"
    assert _alive(pid)

    mgr.store.delete(FinetuneJob, "default", "deljob")
    deadline = time.time() + 120
    while time.time() < deadline:
        mgr.reconcile_once()
        mgr.store.gc_sweep()
        if mgr.store.try_get(FinetuneJob, "default", "deljob") is None:
            break
        time.sleep(0.2)
    assert mgr.store.try_get(FinetuneJob, "default", "deljob") is None
    # children are GC'd over the next reconcile passes (gc_sweep marks
    # the orphan; the Finetune controller's finalizer removes it)
    deadline = time.time() + 60
    while time.time() < deadline:
        mgr.reconcile_once()
        if mgr.store.try_get(Finetune, "default",
                             "deljob-finetune") is None:
            break
        time.sleep(0.2)
    assert mgr.store.try_get(Finetune, "default", "deljob-finetune") \
        is None
    # the trainer process was actually stopped
    for _ in range(50):
        if not _alive(pid):
            break
        time.sleep(0.2)
    assert not _alive(pid), f"trainer pid {pid} still alive"
    # gang GPUs released: a fresh job can allocate immediately
    hp = mgr.store.get(Hyperparameter, "default", "hp")
    hp.spec["parameters"]["maxSteps"] = 2
    mgr.store.update(hp)
    job2 = FinetuneJob(name="afterjob", spec={
        "fineTune": {"finetuneSpec": finetune_spec()}})
    mgr.store.create(job2)
    deadline = time.time() + 300
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(FinetuneJob, "default", "afterjob")
        if cur.status.get("state") in ("Successful", "Failed"):
            break
        time.sleep(0.3)
    assert mgr.store.get(FinetuneJob, "default",
                         "afterjob").status.get("state") == "Successful"


def _alive(pid) -> bool:
    try:
        os.kill(int(pid), 0)
        return True
    except OSError:
        return False


def test_delete_experiment_mid_training_cleans_cascade(tmp_path):
    """Deleting a FinetuneExperiment mid-training cascades: jobs,
    Finetunes and trainer processes all go; nothing leaks."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store, hp_params={"maxSteps": 2000})
    exp = FinetuneExperiment(name="delexp", spec={
        "finetuneJobs": [
            {"name": "dx-j1", "spec": {"fineTune":
                                       {"finetuneSpec": finetune_spec()}}},
        ]})
    mgr.store.create(exp)
    deadline = time.time() + 120
    pid = None
    while time.time() < deadline and pid is None:
        mgr.reconcile_once()
        ft = mgr.store.try_get(Finetune, "default", "dx-j1-finetune")
        if ft and ft.status.get("state") == "Running":
            pids = (ft.status.get("trainJobInfo") or {}).get("pids") or []
            pid = pids[0] if pids else None
        time.sleep(0.2)
    assert pid is not None and _alive(pid)

    mgr.store.delete(FinetuneExperiment, "default", "delexp")
    deadline = time.time() + 120
    while time.time() < deadline:
        mgr.reconcile_once()
        gone = all(mgr.store.try_get(c, "default", n) is None
                   for c, n in [(FinetuneExperiment, "delexp"),
                                (FinetuneJob, "dx-j1"),
                                (Finetune, "dx-j1-finetune")])
        if gone:
            break
        time.sleep(0.2)
    assert mgr.store.try_get(FinetuneExperiment, "default",
                             "delexp") is None
    assert mgr.store.try_get(FinetuneJob, "default", "dx-j1") is None
    assert mgr.store.try_get(Finetune, "default",
                             "dx-j1-finetune") is None
    for _ in range(50):
        if not _alive(pid):
            break
        time.sleep(0.2)
    assert not _alive(pid), f"trainer pid {pid} leaked"


@pytest.mark.slow
def test_concurrent_jobs_with_mid_flight_deletion(tmp_path):
    """Churn: three jobs run concurrently through the gang scheduler;
    one is deleted mid-training; the other two still complete and the
    deleted one's GPUs return to the pool."""
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store, hp_params={"maxSteps": 40})
    for i in range(3):
        mgr.store.create(FinetuneJob(name=f"churn{i}", spec={
            "fineTune": {"finetuneSpec": finetune_spec()}}))
    deleted = False
    deadline = time.time() + 300
    while time.time() < deadline:
        mgr.reconcile_once()
        if not deleted:
            ft = mgr.store.try_get(Finetune, "default",
                                   "churn1-finetune")
            if ft and ft.status.get("state") == "Running":
                mgr.store.delete(FinetuneJob, "default", "churn1")
                deleted = True
        states = [(mgr.store.try_get(FinetuneJob, "default",
                                     f"churn{i}") or
                   type("o", (), {"status": {}})).status.get("state")
                  for i in (0, 2)]
        gone = mgr.store.try_get(FinetuneJob, "default",
                                 "churn1") is None
        if deleted and gone and all(s in ("Successful", "Failed")
                                    for s in states):
            break
        time.sleep(0.3)
    assert deleted
    assert mgr.store.try_get(FinetuneJob, "default", "churn1") is None
    for i in (0, 2):
        cur = mgr.store.get(FinetuneJob, "default", f"churn{i}")
        assert cur.status.get("state") == "Successful", (i, cur.status)


def test_example_manifests_validate(tmp_path):
    """Every shipped examples/*.yaml passes admission on a fresh store
    (catches doc drift against the validation rules)."""
    import glob

    from datatunerx_amd.api.store import Store
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    store = Store(str(tmp_path / "s"))
    files = sorted(glob.glob(os.path.join(root, "examples", "*.yaml")))
    assert len(files) >= 4
    applied = []
    for fn in files:
        with open(fn) as f:
            for obj in store.apply_manifest(f.read()):
                applied.append(f"{obj.kind}/{obj.name}")
    assert any(a.startswith("FinetuneJob/") for a in applied)
    assert any(a.startswith("FinetuneExperiment/") for a in applied)
    assert any(a.startswith("Hyperparameter/") for a in applied)


def test_entrypoints_help():
    """All four module entrypoints respond to --help (import-time and
    argparse wiring stay sound)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for mod in ("datatunerx_amd.cli", "datatunerx_amd.api.manager",
                "datatunerx_amd.serve.server", "datatunerx_amd.train.run"):
        r = subprocess.run([sys.executable, "-m", mod, "--help"],
                           capture_output=True, text=True, timeout=120,
                           cwd=root)
        assert r.returncode == 0, (mod, r.stderr[-300:])
        assert "usage" in (r.stdout + r.stderr).lower(), mod


def test_serve_template_from_cr(tmp_path):
    """serveConfig.template reaches the serve process args; bad values
    are rejected at admission."""
    from datatunerx_amd.api.validation import ValidationError, validate_
    job = FinetuneJob(name="tj", spec={
        "fineTune": {"finetuneSpec": finetune_spec()},
        "serveConfig": {"template": "llama3"}})
    validate_(job)
    with pytest.raises(ValidationError, match="template"):
        validate_(FinetuneJob(name="tj2", spec={
            "fineTune": {"finetuneSpec": finetune_spec()},
            "serveConfig": {"template": "nope"}}))
    # e2e: the job serves with the requested template and still scores
    mgr = mk_manager(tmp_path)
    seed_resources(mgr.store)
    mgr.store.create(FinetuneJob(name="tmpljob", spec={
        "fineTune": {"finetuneSpec": finetune_spec()},
        "serveConfig": {"template": "llama3"}}))
    deadline = time.time() + 300
    while time.time() < deadline:
        mgr.reconcile_once()
        cur = mgr.store.get(FinetuneJob, "default", "tmpljob")
        if cur.status.get("state") in ("Successful", "Failed"):
            break
        time.sleep(0.3)
    assert mgr.store.get(FinetuneJob, "default",
                         "tmpljob").status.get("state") == "Successful"


def test_cli_get_output_formats(tmp_path, capsys):
    """`dtx get -o yaml|json` emit loadable documents; the default
    table lists namespace/name/state."""
    import json as _json

    import yaml as _yaml

    from datatunerx_amd.cli import main as cli
    st = str(tmp_path / "s")
    store = Store(st)
    seed_resources(store)
    cli(["--state-dir", st, "get", "hyperparameter", "-o", "json"])
    docs = _json.loads(capsys.readouterr().out)
    assert docs[0]["kind"] == "Hyperparameter"
    assert docs[0]["spec"]["parameters"]["loRA_R"] == 4
    cli(["--state-dir", st, "get", "dataset", "-o", "yaml"])
    ydocs = list(_yaml.safe_load_all(capsys.readouterr().out))
    assert ydocs[0]["kind"] == "Dataset"
    cli(["--state-dir", st, "get", "llm"])
    table = capsys.readouterr().out
    assert "NAMESPACE" in table and "llama-tiny" in table


def test_cli_delete_missing_and_unknown_kind(tmp_path, capsys):
    from datatunerx_amd.cli import main as cli
    st = str(tmp_path / "s")
    # deleting a nonexistent object is a no-op, not a crash
    cli(["--state-dir", st, "delete", "finetunejob", "nothere"])
    assert "deleted" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="unknown kind"):
        cli(["--state-dir", st, "get", "gizmo"])
