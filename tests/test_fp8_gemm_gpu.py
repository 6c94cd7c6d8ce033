"""FP8 base GEMMs on the GPU (ops/hip/gemm_fp8.hip): the row quantizer
bit for bit against its CPU twin, the e4m3 MFMA GEMM against the fp64
product of the SAME fp8 operands under the row bound of kernel_check (so
only fp32 accumulation and the output rounding are seen; this is also the
check of the 128-deep operand lane layout), the binding's refusals, and the
four autograd nodes on the fp8 route against themselves on the CPU twins.
"""

import pytest
import torch

import kernel_check as kc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    from datatunerx_amd.ops import _dtx_hip as hip
    from datatunerx_amd.ops import autograd as ag
    from datatunerx_amd.ops import reference as ref
    DEV = torch.device("cuda:0")

BF, F32, F64, F8 = (torch.bfloat16, torch.float32, torch.float64,
                    torch.float8_e4m3fn)


def rnd(M, K, seed=0):
    """bf16 [M,K], row r scaled by 2^(r % 7): a swapped scale shows."""
    g = torch.Generator().manual_seed(seed + 7 * M + K)
    x = torch.randn(M, K, generator=g)
    return (x * torch.exp2(torch.arange(M) % 7.0)[:, None]).to(BF)


# ---------------------------------------------------------------- quantize
@pytest.mark.parametrize("M,K", [(1, 128), (5, 256), (300, 384),
                                 (3, 16384)])
def test_quant_fp8_rows_bit_exact(M, K):
    assert K <= hip.quant_fp8_max_k()
    x = rnd(M, K)
    if M > 2:
        x[0] = 0.0                                   # all-zero row
        x[1] = 0.01
        x[1, K // 3] = 0.01 * 1024                   # one element 2^10 x
        x[2] = 3.0 * (1 - 2 * (torch.arange(K) % 2)).to(BF)   # +-absmax
    q, s = ops.quant_fp8_rows(x.to(DEV))
    q_r, s_r = ref.quant_fp8_rows(x)
    assert q.dtype == F8 and q.shape == x.shape and s.shape == (M,)
    assert torch.equal(s.cpu().view(torch.int32), s_r.view(torch.int32))
    assert torch.equal(q.cpu().view(torch.uint8), q_r.view(torch.uint8))
    assert float(q_r.float().abs().max()) == 448.0


def test_quant_fp8_rows_k_limit():
    with pytest.raises(RuntimeError, match="x must"):
        hip.quant_fp8_rows(torch.zeros(1, hip.quant_fp8_max_k() + 8,
                                       dtype=BF, device=DEV))


# -------------------------------------------------------------------- GEMM
def fp8_case(M, N, K):
    a8, sa = ref.quant_fp8_rows(rnd(M, K))
    b8, sb = ref.quant_fp8_rows(rnd(N, K, seed=1))
    src = rnd(M, N, seed=2)
    a, b = a8.to(F64) * sa.to(F64)[:, None], b8.to(F64) * sb.to(F64)[:, None]
    return (a8, sa, b8, sb, src), a @ b.t(), a.abs() @ b.abs().t()


def check_gemm(M, N, K):
    args, want, bud = fp8_case(M, N, K)
    a8, sa, b8, sb, src = (t.to(DEV) for t in args)
    got = ops.gemm_fp8_nt(a8, sa, b8, sb)
    assert got.dtype == BF and got.shape == (M, N)
    kc.assert_rows(got, want, bud, name=f"gemm_fp8_nt {M}x{N}x{K}")
    got = ops.gemm_fp8_nt(a8, sa, b8, sb, src)
    kc.assert_rows(got, want + args[4].to(F64),
                   bud + args[4].to(F64).abs(),
                   name=f"gemm_fp8_nt+src {M}x{N}x{K}")


# K = 256, 384, 768: 2, 3 and 6 tiles (prologue-only drain, odd ring wrap,
# more tiles than ring slots); M: the tail and a second row of tiles.
@pytest.mark.parametrize("K", [256, 384, 768])
@pytest.mark.parametrize("N", [256, 512])
@pytest.mark.parametrize("M", [1, 255, 257, 600])
def test_gemm_fp8_nt(M, N, K):
    check_gemm(M, N, K)


def test_gemm_fp8_nt_cluster_grid():
    check_gemm(2048, 1024, 384)      # 8 x 4 blocks: the cluster grid order
    b8, sb = ref.quant_fp8_rows(rnd(256, 256))       # M == 0: no launch
    assert ops.gemm_fp8_nt(torch.zeros(0, 256).to(F8).to(DEV),
                           torch.zeros(0, device=DEV), b8.to(DEV),
                           sb.to(DEV)).shape == (0, 256)


def test_gemm_fp8_nt_refusals():
    """Every refused input is memory-safe without its check, built as
    tests/test_binding_contract_gpu.py describes."""
    def z(*shape, dt=F32):
        return torch.zeros(*shape, dtype=dt).to(DEV)
    M, N, K = 8, 256, 256
    a8, sa, b8, sb = z(M, K, dt=F8), z(M), z(N, K, dt=F8), z(N)
    for args, name in [
            ((z(M, 320, dt=F8), sa, z(N, 320, dt=F8), sb), "b8"),  # K % 128
            ((z(M, 128, dt=F8), sa, z(N, 128, dt=F8), sb), "b8"),  # K = 128
            ((a8, sa, z(128, K, dt=F8), z(128)), "b8"),            # N % 256
            ((z(M, K, dt=BF), sa, b8, sb), "a8"),
            ((a8, z(M + 8), b8, sb), "sa"),
            ((a8, sa, z(N, 2 * K, dt=F8)[:, ::2], sb), "b8"),
            ((a8, sa, b8, torch.zeros(N).pin_memory()), "sb")]:
        with pytest.raises(RuntimeError, match=name):
            hip.gemm_fp8_nt(*args, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------- nodes
M_, K_, N_ = 64, 256, 256


def run_node(kind, dev, fp8):
    """One forward and backward of a base-GEMM node on `dev`; fp8 operands
    come from that device's quantizer (bit-identical on both). Returns the
    outputs, dx and the LoRA gradients."""
    w = [rnd(N_, K_, seed=10 + i).to(dev) / 64 for i in range(3)]
    f8 = [(*ops.quant_fp8_rows(t), *ops.quant_fp8_rows(t.t().contiguous()))
          if fp8 else None for t in w]
    x = (rnd(M_, K_, seed=3) / 8).to(dev).requires_grad_(True)
    res = rnd(M_, N_, seed=4).to(dev)
    a = [(rnd(8, K_, seed=5 + i) / 16).to(dev).requires_grad_(True)
         for i in range(2)]
    b = [(rnd(N_, 8, seed=7 + i) / 16).to(dev).requires_grad_(True)
         for i in range(2)]
    if kind == "frozen":
        ys = (ag.FrozenGemm.apply(x, w[0], None, res, False, f8[0]),)
    elif kind == "lora":
        ys = (ag.LoRALinear.apply(x, w[0], a[0], b[0], 2.0, None, 0, 1.0,
                                  False, f8[0]),)
    elif kind == "paired":
        ys = ag.PairedFrozenGemm.apply(x, w[0], w[1], None, None, f8[0],
                                       f8[1])
    else:
        ys = ag.QKVProj.apply(x, w[0], a[0], b[0], w[1], w[2], a[1], b[1],
                              2.0, 0, 0, 1.0, None, None, None,
                              tuple(f8) if fp8 else None)
    dys = [(rnd(M_, N_, seed=20 + i) / 8).to(dev) for i in range(len(ys))]
    torch.autograd.backward(ys, dys)
    lora_grads = [t.grad for t in a + b if t.grad is not None]
    return list(ys) + [x.grad], lora_grads


@pytest.mark.parametrize("kind", ["frozen", "lora", "paired", "qkv"])
def test_fp8_nodes_match_cpu_twins(kind):
    got, lg = run_node(kind, DEV, True)
    want, _ = run_node(kind, torch.device("cpu"), True)
    for i, (g, w_) in enumerate(zip(got, want)):
        kc.assert_rows(g, w_.to(F64), name=f"{kind} out{i}")
    # the low-rank kernels read the bf16 x and dy: LoRA grads never see fp8
    _, lg_bf16 = run_node(kind, DEV, False)
    assert len(lg) == len(lg_bf16) == {"lora": 2, "qkv": 4}.get(kind, 0)
    for g, w_ in zip(lg, lg_bf16):
        assert torch.equal(g, w_)
