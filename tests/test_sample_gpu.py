"""ops.sample on the GPU (sample.hip) against the fp64 oracle of
tests/sample_cases.py: exact tokens on inputs whose every decision has an
fp64 margin of at least 1e-4 of the row mass (derivation: sample_cases),
greedy == torch.argmax, the RNG bit for bit, row independence, the drawn
distribution, and the binding's refusals."""

import pytest
import torch

import sample_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from datatunerx_amd import ops
    assert ops.have_ext()
    return ops


@pytest.mark.parametrize("idx", range(len(sc.CASES)))
def test_exact_tokens(idx):
    """One row per nucleus member with u at the fp64 midpoint of the
    member's CDF interval (index order), plus u = 0 and u = 1 - 2^-24:
    the op returns exactly that member. Covers the top-p cut, the index
    rule inside the tie group, top-k before top-p and the inverse CDF."""
    d = sc.build_case(idx)
    # preconditions: a badly chosen case fails here, not as a kernel error
    assert d["half_gap"] >= sc.MARGIN, d["half_gap"]
    assert d["margin"] >= sc.MARGIN, d["margin"]
    assert d["n_rows_mid"] >= 1
    assert d["last_share"] >= 2 * sc.MARGIN
    B = len(d["us"])
    logits = d["logits"].to(DEV).unsqueeze(0).repeat(B, 1)
    u = torch.tensor(d["us"], dtype=torch.float64).to(torch.float32)
    assert float(u.max()) < 1.0
    out = _ops().sample(logits, *sc.params(B, d["T"], d["top_p"],
                                           d["top_k"], DEV), u=u.to(DEV))
    assert out.dtype == torch.int64 and out.shape == (B,)
    got = out.cpu().tolist()
    inside = set(d["members"].tolist())
    assert all(t in inside for t in got), "token outside the fp64 nucleus"
    assert got == d["expect"]


def test_greedy_equals_argmax_and_mixes_with_sampled():
    V = 4104
    g = torch.Generator().manual_seed(7)
    rows = [torch.randn(V, generator=g) * 3 for _ in range(6)]
    tie = torch.randn(V, generator=g)
    tie[[17, 900, 4000]] = 9.0                 # the first maximum wins
    flat = torch.full((V,), 1.25)              # all equal: index 0
    ninf = torch.randn(V, generator=g)
    ninf[::3] = float("-inf")
    allneg = -torch.rand(V, generator=g) - 1.0
    allneg[[5, 2000]] = -0.5
    logits = torch.stack(rows + [tie, flat, ninf, allneg]) \
        .to(torch.bfloat16).to(DEV)
    B = logits.shape[0]
    want = logits.argmax(-1)
    assert int(want[6]) == 17 and int(want[7]) == 0 and int(want[9]) == 5
    ops = _ops()
    out = ops.sample(logits, *sc.params(B, 0.0, 1.0, 0, DEV))
    assert torch.equal(out, want)
    # greedy and sampled rows in one call: the greedy ones do not move
    T = torch.tensor([0.0, 0.9] * (B // 2), dtype=torch.float32, device=DEV)
    p = sc.params(B, 0.0, 0.8, 5, DEV, seed=3)
    mixed = ops.sample(logits, T, *p[1:])
    assert torch.equal(mixed[0::2], want[0::2])
    assert bool(((mixed >= 0) & (mixed < V)).all())
    # top_k = 1 is greedy too, at any temperature
    k1 = ops.sample(logits, *sc.params(B, 1.5, 1.0, 1, DEV, seed=9))
    assert torch.equal(k1, want)


def test_rng_on_device_is_the_integer_reference():
    """All-equal logits, V = 4096, T = 1, top_p = 1: every sum is an
    exact integer and u * 4096 is exact, so the token is the top 12 bits
    of u."""
    from datatunerx_amd.ops import reference as ref
    V = B = 4096
    g = torch.Generator().manual_seed(20261021)
    seed = torch.randint(-2 ** 62, 2 ** 62, (B,), generator=g,
                         dtype=torch.int64) * 2 + 1
    offset = torch.randint(0, 2 ** 31 - 1, (B,), generator=g,
                           dtype=torch.int64).to(torch.int32)
    seed[:5] = torch.tensor([0, 5, -1, 2 ** 63 - 1, -2 ** 63])
    offset[:5] = torch.tensor([0, 7, 2 ** 31 - 1, 2 ** 31 - 1, 1],
                              dtype=torch.int32)
    assert bool((seed < 0).any())
    want = ref.sample_rng(seed, offset) >> 12
    logits = torch.full((1, V), 0.5, dtype=torch.bfloat16,
                        device=DEV).expand(B, V)
    t, p, k, _, _ = sc.params(B, 1.0, 1.0, 0, DEV)
    out = _ops().sample(logits, t, p, k, seed.to(DEV), offset.to(DEV))
    assert torch.equal(out.cpu(), want)


def _mixed_rows(B, V, gen_seed):
    g = torch.Generator().manual_seed(gen_seed)
    logits = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16)
    logits[3] = torch.round(logits[3].float())         # big tie groups
    logits[4, ::2] = float("-inf")
    T = torch.tensor([[0.0, 0.7, 1.0, 1.4][i % 4] for i in range(B)])
    p = torch.tensor([[1.0, 0.9, 0.5, 0.97, 1.0][i % 5] for i in range(B)])
    k = torch.tensor([[0, 0, 40, 3, 0, 1000][i % 6] for i in range(B)],
                     dtype=torch.int32)
    seed = torch.randint(-2 ** 62, 2 ** 62, (B,), generator=g,
                         dtype=torch.int64)
    off = torch.randint(0, 4096, (B,), generator=g,
                        dtype=torch.int64).to(torch.int32)
    return [t.to(DEV) for t in (logits, T, p, k, seed, off)]


def test_row_independence():
    """A row's token depends on that row's inputs only: not on B, the
    row's position, the other rows, or the row stride; and not on the
    call."""
    ops = _ops()
    B, V = 64, 4104
    logits, *par = _mixed_rows(B, V, 99)
    base = ops.sample(logits, *par)
    assert torch.equal(ops.sample(logits, *par), base)      # repeatable
    assert base[0::4].eq(logits[0::4].argmax(-1)).all()     # greedy rows
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)) \
        .to(DEV)
    out = ops.sample(logits[perm].contiguous(),
                     *[t[perm].contiguous() for t in par])
    assert torch.equal(out, base[perm])
    alone = torch.cat([ops.sample(logits[i:i + 1],
                                  *[t[i:i + 1] for t in par])
                       for i in range(B)])
    assert torch.equal(alone, base)
    wide = torch.randn(B, 3, V, device=DEV).to(torch.bfloat16)
    wide[:, 1] = logits
    view = wide[:, 1]
    assert view.stride(0) == 3 * V and not view.is_contiguous()
    assert torch.equal(ops.sample(view, *par), base)


@pytest.mark.parametrize("i", range(len(sc.DIST_SETTINGS)))
def test_distribution(i):
    """65536 draws of one row follow the nucleus probabilities, over
    the seeds (seed = 1234 + row, offset 0) and over the offsets of one
    seed (what a single request consumes). Seeds are fixed, so the
    outcome is deterministic."""
    logits, T, top_p, top_k, members, pm = sc.dist_case(i)
    B = sc.DIST_ROWS
    rows = logits.to(DEV).unsqueeze(0).expand(B, -1)
    t, p, k, _, _ = sc.params(B, T, top_p, top_k, DEV)
    ar = torch.arange(B, device=DEV)
    runs = {
        "seeds": (1234 + ar, torch.zeros(B, dtype=torch.int32, device=DEV)),
        "offsets": (torch.full((B,), 77, dtype=torch.int64, device=DEV),
                    ar.to(torch.int32)),
    }
    for name, (seed, off) in runs.items():
        out = _ops().sample(rows, t, p, k, seed, off)
        chi, bins = sc.chi_square(out, members, pm)
        limit = sc.chi_square_limit(bins)
        print(f"setting {i} {name}: chi2 {chi:.1f} limit {limit:.1f} "
              f"bins {bins}")
        assert chi < limit, (name, chi, limit, bins)


def test_refusals():
    ops = _ops()
    cap = ops.sample_max_vocab()
    assert cap >= 151936

    def call(logits, n=None, **kw):
        B = logits.shape[0]
        par = list(sc.params(B if n is None else n, 1.0, 1.0, 0, DEV))
        return ops.sample(logits, *par, **kw)

    ok = torch.zeros(2, 64, dtype=torch.bfloat16, device=DEV)
    assert call(ok).shape == (2,)
    with pytest.raises(Exception, match="V % 8"):
        call(torch.zeros(2, 60, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(Exception, match="kernel limit"):
        call(torch.zeros(1, cap + 8, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(Exception, match="bf16"):
        call(torch.zeros(2, 64, dtype=torch.float32, device=DEV))
    with pytest.raises(Exception, match="temperature"):
        call(ok, n=3)
    with pytest.raises(Exception, match="u must be"):
        call(ok, u=torch.zeros(3, device=DEV))
    with pytest.raises(Exception, match="top_k"):
        par = list(sc.params(2, 1.0, 1.0, 0, DEV))
        par[2] = par[2].to(torch.int64)
        ops.sample(ok, *par)
