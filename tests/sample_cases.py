"""Shared inputs and the fp64 oracle of the sampling tests (ops.sample).

Everything here is built so that every decision the sampler takes has an
fp64 margin of at least MARGIN (1e-4 of the row mass): the kernel's fp32
sums run over at most ~150 serial terms per thread plus a ~10-level tree
(about 160 * 2^-24 ~ 1e-5 relative), exp and the x / T rounding add about
1.5e-6, so a margin of 1e-4 leaves ~8x headroom and the tests can demand
EXACT tokens. Each test asserts its margin before it calls the op.
"""

import functools
import math

import torch

MARGIN = 1e-4

# V, std, T, nominal top_p, top_k, generator seed, quant
CASES = [
    (1000, 2.0, 0.8, 0.9, 0, 1, None),
    (1032, 2.0, 1.0, 0.7, 0, 5, None),
    (32000, 4.0, 0.7, 0.9, 0, 1, None),
    (128256, 4.0, 0.7, 0.9, 0, 1, None),
    (4096, 2.0, 1.0, 0.6, 0, 3, 0.5),
    (4096, 2.0, 1.0, 0.8, 0, 3, 1.0),
    (32000, 3.0, 1.0, 0.9, 50, 4, 0.5),
    (32000, 2.0, 1.0, 0.9, 40, 4, None),
    # the widest supported vocabulary (std 5 at T 1.0 leaves a half-gap
    # below MARGIN, hence the lower temperature)
    (151936, 5.0, 0.7, 0.9, 0, 1, None),
]


def make_logits(V, std, seed, quant=None):
    """randn * std, rounded to `quant` where given, as bf16 [V]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(V, generator=g) * std
    if quant:
        x = torch.round(x / quant) * quant
    return x.to(torch.bfloat16)


class Oracle:
    """fp64 sampler state of one row: stable sort on (-logit, index),
    cumulative sums, inverse CDF in index order."""

    def __init__(self, logits, T, top_k):
        x = logits.double()
        V = x.numel()
        self.V = V
        self.w = torch.exp((x - x.max()) / T)
        # stable: equal logits keep ascending index
        self.order = torch.sort(x, descending=True, stable=True).indices
        k = V if (top_k <= 0 or top_k >= V) else top_k
        self.cand = self.order[:k]
        cum = torch.cumsum(self.w[self.cand], 0)
        self.z_c = float(cum[-1])
        self.frac = cum / cum[-1]       # cumulative fractions, in order
        self.x = x

    def midpoint_top_p(self, nominal):
        """(top_p, half_gap): the midpoint of the two cumulative
        fractions that straddle `nominal`."""
        i = int((self.frac <= nominal).sum())       # frac[i-1] <= nominal
        lo, hi = float(self.frac[i - 1]), float(self.frac[i])
        return 0.5 * (lo + hi), 0.5 * (hi - lo)

    def nucleus(self, top_p):
        """Member indices in INDEX order, and the margin of the cut."""
        if top_p >= 1.0:
            n, margin = self.cand.numel(), 1.0
        else:
            n = max(1, int((self.frac <= top_p).sum()))
            margin = float((self.frac - top_p).abs().min())
        members = torch.sort(self.cand[:n]).values
        return members, margin

    def tie_group(self, members):
        """(size of the cut key's tie group among the candidates, how
        many of it are inside the nucleus)."""
        inside = set(members.tolist())
        cut = self.x[self.order[len(inside) - 1]]
        grp = [int(i) for i in self.cand if self.x[i] == cut]
        return len(grp), sum(i in inside for i in grp)

    def cdf(self, members):
        """Index-order CDF intervals of the members: (lo, hi) fp64."""
        wm = self.w[members]
        c = torch.cumsum(wm, 0) / wm.sum()
        return torch.cat([torch.zeros(1, dtype=c.dtype), c[:-1]]), c

    def draw(self, members, u):
        lo, hi = self.cdf(members)
        j = int((hi <= u).sum())
        return int(members[min(j, members.numel() - 1)])


@functools.lru_cache(maxsize=None)
def build_case(idx):
    """-> dict(logits, T, top_p, top_k, members, us, expect, half_gap)
    for CASES[idx]: one row per nucleus member whose share of the
    nucleus mass is at least 2 * MARGIN, with u = the fp64 midpoint of
    that member's CDF interval, plus u = 0 and u = 1 - 2^-24."""
    V, std, T, nominal, top_k, seed, quant = CASES[idx]
    logits = make_logits(V, std, seed, quant)
    orc = Oracle(logits, T, top_k)
    top_p, half_gap = orc.midpoint_top_p(nominal)
    members, margin = orc.nucleus(top_p)
    lo, hi = orc.cdf(members)
    share = hi - lo
    rows = [j for j in range(members.numel())
            if float(share[j]) >= 2 * MARGIN]
    us = [float(0.5 * (lo[j] + hi[j])) for j in rows]
    expect = [int(members[j]) for j in rows]
    us += [0.0, 1.0 - 2.0 ** -24]
    expect += [int(members[0]), int(members[-1])]
    return dict(logits=logits, T=T, top_p=top_p, top_k=top_k,
                members=members, us=us, expect=expect, half_gap=half_gap,
                margin=margin, oracle=orc, n_rows_mid=len(rows),
                min_share=float(share.min()), last_share=float(share[-1]))


def params(B, T, top_p, top_k, device="cpu", seed=0, offset=0):
    """ops.sample's parameter tensors for B equal rows."""
    return (torch.full((B,), T, dtype=torch.float32, device=device),
            torch.full((B,), top_p, dtype=torch.float32, device=device),
            torch.full((B,), top_k, dtype=torch.int32, device=device),
            torch.full((B,), seed, dtype=torch.int64, device=device),
            torch.full((B,), offset, dtype=torch.int32, device=device))


def chi_square_limit(bins, z=4.75):
    """Wilson-Hilferty quantile of chi-square with bins - 1 degrees of
    freedom at normal deviate z (4.75: p ~ 1e-6)."""
    k = bins - 1
    return k * (1 - 2 / (9 * k) + z * math.sqrt(2 / (9 * k))) ** 3


DIST_SETTINGS = [(1.0, 1.0, 0), (0.8, 0.9, 0), (1.0, 1.0, 12),
                 (1.3, 0.8, 20)]
DIST_V, DIST_ROWS = 64, 65536


@functools.lru_cache(maxsize=None)
def dist_case(i):
    """Distribution test input i: logits [64] bf16, the setting with its
    top_p moved to a cut midpoint (so the nucleus is unambiguous), the
    fp64 nucleus and its probabilities."""
    T, nominal, top_k = DIST_SETTINGS[i]
    logits = make_logits(DIST_V, 2.0, 11 + i)
    orc = Oracle(logits, T, top_k)
    top_p = nominal
    if nominal < 1.0:
        top_p, half_gap = orc.midpoint_top_p(nominal)
        assert half_gap >= MARGIN
    members, _ = orc.nucleus(top_p)
    pm = orc.w[members] / orc.w[members].sum()
    return logits, T, top_p, top_k, members, pm


def chi_square(tokens, members, pm):
    """(chi-square, bins) of the drawn tokens against the nucleus
    probabilities; tokens whose expected count is below 20 share a bin.
    Every token must be a nucleus member."""
    n = tokens.numel()
    counts = torch.bincount(tokens.cpu(), minlength=DIST_V).double()
    inside = torch.zeros(DIST_V, dtype=torch.bool)
    inside[members] = True
    assert float(counts[~inside].sum()) == 0, "token outside the nucleus"
    exp = pm * n
    obs = counts[members]
    small = exp < 20
    e = torch.cat([exp[~small], exp[small].sum().view(1)]) \
        if small.any() else exp
    o = torch.cat([obs[~small], obs[small].sum().view(1)]) \
        if small.any() else obs
    keep = e > 0
    return float((((o - e) ** 2) / e)[keep].sum()), int(keep.sum())
