"""ops.gemm_nt_add on the GPU: d = bf16(a @ b^T + c) on hipBLASLt with
C != D (ops/hip/basegemm.cpp), against the fp32 product, with the metric
and tolerance of the gemm_nt tests (assert_close of test_ops_gpu.py).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from datatunerx_amd import ops
    DEV = torch.device("cuda:0")
    assert ops.have_ext(), "HIP extension must be built for GPU tests"

torch.manual_seed(0)


def mk(*shape, dtype=torch.bfloat16, scale=1.0):
    return (torch.randn(*shape, device=DEV, dtype=torch.float32)
            .mul(scale).to(dtype))


def assert_close(got, want, rtol=2e-2, name=""):
    got, want = got.float(), want.float()
    denom = want.abs().max().clamp(min=1e-3)
    err = (got - want).abs().max() / denom
    assert err < rtol, f"{name}: rel err {err:.4f} (max {denom:.3f})"


def want_of(a, b, c):
    return a.float() @ b.float().t() + c.float()


def check(M, N, K):
    a, b, c = mk(M, K), mk(N, K), mk(M, N)
    c0 = c.clone()
    d = ops.gemm_nt_add(a, b, c)
    assert d.shape == (M, N) and d.dtype == torch.bfloat16
    assert_close(d, want_of(a, b, c0), name=f"gemm_nt_add {M}x{N}x{K}")
    assert torch.equal(c, c0), "c was written"
    assert d.untyped_storage().data_ptr() != c.untyped_storage().data_ptr()


@pytest.mark.parametrize("M,N,K", [
    (1, 256, 64),             # one row
    (127, 256, 128),          # M below one tile
    (1023, 512, 4096),        # the lm_head's S-1 tail at small size
    (300, 1288, 192),         # N, K multiples of 8 but of no tile
    (512, 4096, 11008),       # down-proj K
])
def test_gemm_nt_add(M, N, K):
    check(M, N, K)


def test_plan_cache_hit_then_other_shape():
    check(200, 512, 256)
    check(200, 512, 256)      # descriptor cache hit
    check(136, 264, 320)      # another shape after it
    check(200, 512, 256)


def test_side_stream_ordering():
    """a is produced on a side stream and d consumed on it with no sync
    in between: the GEMM must be enqueued on that stream."""
    M, N, K = 512, 1024, 2048
    b, c = mk(N, K), mk(M, N)
    src = mk(M, K)
    a = torch.zeros_like(src)             # what a wrong-stream GEMM reads
    big = mk(8192, 8192, scale=0.01)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):                # milliseconds of work ahead of a
            big @ big
        a.copy_(src)
        d = ops.gemm_nt_add(a, b, c)
        out = d.float() * 2.0
    s.synchronize()
    assert_close(out, 2.0 * want_of(src, b, c), name="side stream")


def test_refusals():
    M, N, K = 32, 64, 48
    a, b, c = mk(M, K), mk(N, K), mk(M, N)
    with pytest.raises(RuntimeError, match="a must be bf16"):
        ops.gemm_nt_add(a.to(torch.float16), b, c)
    with pytest.raises(RuntimeError, match="b must be bf16 on the GPU"):
        ops.gemm_nt_add(a, b.cpu(), c)
    with pytest.raises(RuntimeError, match="c must be contiguous"):
        ops.gemm_nt_add(a, b, mk(N, M).t())
    with pytest.raises(RuntimeError, match=r"c must be \[32, 64\]"):
        ops.gemm_nt_add(a, b, mk(M, N + 8))
    with pytest.raises(RuntimeError, match="differ in K"):
        ops.gemm_nt_add(a, mk(N, K + 8), c)
    buf = mk(M * K + 8)
    a_off = buf[1:1 + M * K].view(M, K)   # misaligned by one element
    assert a_off.is_contiguous() and a_off.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError, match="16-byte alignment"):
        ops.gemm_nt_add(a_off, b, c)


def test_one_hipblaslt_and_it_is_torchs():
    """The extension links hipBLASLt itself (basegemm.cpp): the process
    must hold one copy, the one in torch's lib directory, and its major
    version must be that of the headers the extension was built with."""
    import os
    with open("/proc/self/maps") as f:
        libs = {line.split()[-1] for line in f if "libhipblaslt" in line}
    assert len(libs) == 1, libs
    torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    assert os.path.dirname(os.path.realpath(libs.pop())) == \
        os.path.realpath(torch_lib)
    header, loaded = ops._load_ext().gemm_nt_add_versions()
    print(f"hipBLASLt headers {header}, loaded {loaded}")
    assert header // 100000 == loaded // 100000


def test_empty_dims_launch_nothing():
    N, K = 64, 48
    d = ops.gemm_nt_add(mk(0, K), mk(N, K), mk(0, N))
    assert d.shape == (0, N)
    d = ops.gemm_nt_add(mk(16, K), mk(0, K), mk(16, 0))
    assert d.shape == (16, 0)
    c = mk(16, N)
    d = ops.gemm_nt_add(mk(16, 0), mk(N, 0), c)
    assert torch.equal(d, c)
    assert d.untyped_storage().data_ptr() != c.untyped_storage().data_ptr()
