"""ops/hip/qgemv_fp8.hip against the fp64 product of the CPU quantizer's fp8
operands under kernel_check's row bound (as test_fp8_gemm_gpu.py checks the
GEMM); then row independence, routing, refusals and the engine."""

import functools

import pytest
import torch

import kernel_check as kc
from test_fp8_gemm_gpu import rnd

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    from datatunerx_amd.ops import _dtx_hip as hip
    from datatunerx_amd.ops import reference as ref
    DEV = torch.device("cuda:0")

BF, F64, F8 = torch.bfloat16, torch.float64, torch.float8_e4m3fn
K_ROUND = 128 * (8 * 4 + 1)    # one k-step past a round of 8 waves x 4 steps


@functools.lru_cache(maxsize=None)
def weight(N, K):
    w8, sw = ref.quant_fp8_rows(rnd(N, K, seed=1))
    return w8.to(DEV), sw.to(DEV), w8.to(F64) * sw.to(F64)[:, None]


def check(x, N, name):
    w8, sw, b = weight(N, x.shape[1])
    x8, sa = ref.quant_fp8_rows(x)
    a = x8.to(F64) * sa.to(F64)[:, None]
    got = hip.qgemv_fp8(x.to(DEV), w8, sw)
    assert got.dtype == BF and got.shape == (x.shape[0], N)
    kc.assert_rows(got, a @ b.t(), a.abs() @ b.abs().t(), name=name)
    return got


# N: under a tile, a tail tile, four-tile blocks (N >= 8192) whose last has
# 8 live rows and three tiles past N; K: 1 step, 3, a round + 1
@pytest.mark.parametrize("K", [128, 384, K_ROUND])
@pytest.mark.parametrize("N", [8, 40, 8200])
@pytest.mark.parametrize("M", [1, 2, 5, 16])
def test_qgemv_fp8(M, N, K):
    check(rnd(M, K), N, f"qgemv_fp8 {M}x{N}x{K}")


def test_qgemv_fp8_quantizer_sparse_rows():
    """Three non-zeros a row: the absmax and two on e4m3 ties of x / s that
    x * (1 / s) misses (s = 7/64, 7/512); one all-zero row. On the CPU twin
    the honest quantizer is at 0.18 of the bound, any one code moved by one
    step at 1.3 to 8.0, the reciprocal (4 codes move) at 4.6."""
    x = torch.zeros(4, 128)
    x[0, [5, 64, 127]] = torch.tensor([49.0, 175 / 8, -203 / 8])
    x[1, [0, 33, 90]] = torch.tensor([-203 / 64, 175 / 64, 49 / 8])
    x[3, [17, 18, 100]] = torch.tensor([0.75, -3.0, 1.625])
    assert torch.equal(x.to(BF).float(), x)
    got = check(x.to(BF), 16, "qgemv_fp8 sparse rows")
    assert not got[2].any()
    assert hip.qgemv_fp8(x[:0].to(BF).to(DEV),
                         *weight(16, 128)[:2]).shape == (0, 16)


@pytest.mark.parametrize("r", [0, 11])
def test_qgemv_fp8_row_does_not_depend_on_batch(r):
    x = rnd(16, K_ROUND).to(DEV)
    w8, sw, _ = weight(40, K_ROUND)
    assert torch.equal(hip.qgemv_fp8(x, w8, sw)[r],
                       hip.qgemv_fp8(x[r:r + 1].contiguous(), w8, sw)[0])


def test_qlinear_e4m3_routing():
    w8, sw, _ = weight(256, 256)
    x = rnd(4, 256).to(DEV)
    assert torch.equal(ops.qlinear(x, w8, sw, 8, codebook="e4m3"),
                       hip.qgemv_fp8(x, w8, sw))
    x = rnd(64, 256).to(DEV)
    assert torch.equal(ops.qlinear(x, w8, sw, 8, codebook="e4m3"),
                       ops.gemm_fp8_nt(*ops.quant_fp8_rows(x), w8, sw))


def test_qgemv_fp8_refusals():
    def z(*shape, dt=torch.float32):
        return torch.zeros(*shape, dtype=dt).to(DEV)
    N, K, big = 8, 128, hip.quant_fp8_max_k() + 128
    x, w8, sw = z(2, K, dt=BF), z(N, K, dt=F8), z(N)
    for args, name in [
            ((z(2, 192, dt=BF), z(N, 192, dt=F8), sw), "M=2 N=8 K=192"),
            ((z(1, big, dt=BF), z(N, big, dt=F8), sw), f"M=1 N=8 K={big}"),
            ((z(17, K, dt=BF), w8, sw), "M=17 N=8 K=128"),
            ((x, z(N, 2 * K, dt=F8)[:, ::2], sw), "w8"),
            ((x, w8, torch.zeros(N).pin_memory()), "sw")]:
        with pytest.raises(RuntimeError, match=name):
            hip.qgemv_fp8(*args)
    torch.cuda.synchronize()


def test_engine_fp8_base_batched_equals_per_request():
    from datatunerx_amd.serve.engine import InferenceEngine, build_model
    torch.manual_seed(0)
    model = build_model("llama-mini", DEV, base_gemm="fp8")   # 256 / 512
    eng = InferenceEngine(model, device=DEV)
    prompts = [list(range(4, 9)), list(range(20, 29)), list(range(40, 60))]
    single = [eng.generate(p, max_new_tokens=8) for p in prompts]
    assert eng.generate_batch(prompts, max_new_tokens=8) == single
