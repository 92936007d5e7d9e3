"""Draft proposers for speculative decoding (``LLMEngine(spec_tokens=T)``).

A proposer is any object with ``propose(tokens, k) -> list[int]``: given a request's prompt + output so
far, up to ``k`` tokens it expects to come next (an empty list: no proposal, the request decodes one token
this step). The engine verifies the proposal with the model itself (``ModelRunner.verify``), so a proposer
changes how many tokens a step yields, never which tokens are generated.
"""
from __future__ import annotations


class NgramProposer:
    """Prompt lookup: find the latest earlier occurrence of the sequence's last n tokens -- n from
    ``max_ngram`` down to ``min_ngram``, inside the last ``window`` tokens -- and propose the tokens that
    followed it. No model, no state; the host cost is a scan of at most ``window`` tokens per n."""

    def __init__(self, max_ngram: int = 3, min_ngram: int = 1, window: int = 1024):
        if not 1 <= min_ngram <= max_ngram:
            raise ValueError(f"NgramProposer: need 1 <= min_ngram <= max_ngram, got {min_ngram}, {max_ngram}")
        if window < 2:
            raise ValueError(f"NgramProposer: window {window} < 2")
        self.max_ngram, self.min_ngram, self.window = max_ngram, min_ngram, window

    def propose(self, tokens: list, k: int) -> list:
        if k <= 0:
            return []
        ctx = tokens[-self.window:]
        L = len(ctx)
        for n in range(min(self.max_ngram, L - 1), self.min_ngram - 1, -1):
            tail = ctx[L - n:]
            # the latest match that ends before the tail's own last token (so something follows it)
            for i in range(L - n - 1, -1, -1):
                if ctx[i:i + n] == tail:
                    return list(ctx[i + n:i + n + k])
        return []


__all__ = ["NgramProposer"]
