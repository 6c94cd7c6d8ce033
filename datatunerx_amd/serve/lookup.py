"""Prompt-lookup drafting for speculative decoding: the draft tokens are
what followed the text's current ending the last time it occurred. No
draft model; pays where the output repeats its context (summaries,
extraction, rewritten code, quotations)."""

from __future__ import annotations

from typing import List, Sequence


def prompt_lookup(ids: Sequence[int], k: int, max_ngram: int = 3) -> List[int]:
    """Up to k draft tokens for the sequence `ids`: take the longest suffix
    of ids (max_ngram tokens down to 1) that also occurs earlier, and
    return what followed its LATEST earlier occurrence, cut at the end of
    ids. No earlier occurrence of even the last token: []."""
    n_ids = len(ids)
    for n in range(min(max_ngram, n_ids - 1), 0, -1):
        suffix = list(ids[n_ids - n:])
        # an earlier occurrence ends before the last token: >= 1 follower
        for start in range(n_ids - n - 1, -1, -1):
            if ids[start] == suffix[0] and \
                    list(ids[start:start + n]) == suffix:
                return list(ids[start + n:start + n + k])
    return []
