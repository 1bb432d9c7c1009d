"""What ``ctc_beam_search`` is held to: the definition stated directly on a dict from prefix tuples to ``(pb, pnb)`` in Python
floats, a case maker and the comparison.  Shares no code with ``_composite``.

Scores: ``|got - want| <= ulp32(want) / 2 + bound`` with ``bound = 8 * kept * 2**-52 * max(1, |want|)`` — the one rounding to
float32 plus a few float64 ulps of the running total per kept frame, accumulated linearly.  Tokens and lengths: equal.  The
reference reports its smallest gap (between the K-th and the (K + 1)-th total at any step, and between neighbouring final
hypotheses); a case is only used where that gap is at least 100 bounds, so no choice hangs on the arithmetic's last bits."""
import math

import numpy as np
import torch

NINF = float('-inf')
_memo = {}


def lae(a, b):
    m, n = max(a, b), min(a, b)
    return m if m == NINF else m + math.log1p(math.exp(n - m))


def reference(lp, length, K, nbest, blank, threshold):
    """``(hypotheses [(prefix, tot)], smallest gap, kept frames)`` of one entry; ``lp`` a (T, C) float32 tensor"""
    rows = lp.double().tolist()
    C = len(rows[0])
    beam, gap, kept = {(): (0.0, NINF)}, float('inf'), 0
    for t in range(length):
        row = rows[t]
        if math.exp(row[blank]) > threshold:
            continue
        kept += 1
        S = sorted((c for c in range(C) if c != blank), key=lambda c: (-row[c], c))[:min(K + 1, C - 1)]
        new = {}

        def add(p, dpb, dpnb):
            pb, pnb = new.get(p, (NINF, NINF))
            new[p] = (lae(pb, dpb), lae(pnb, dpnb))
        for p, (pb, pnb) in beam.items():
            tot = lae(pb, pnb)
            add(p, tot + row[blank], pnb + row[p[-1]] if p else NINF)
            for c in set(S) | {q[-1] for q in beam if q[:-1] == p and q}:
                add(p + (c,), NINF, (pb if p and c == p[-1] else tot) + row[c])
        ranked = sorted(((lae(*v), p) for p, v in new.items() if lae(*v) > NINF), reverse=True)
        if len(ranked) > K:
            gap = min(gap, ranked[K - 1][0] - ranked[K][0])
        beam = {p: new[p] for _, p in ranked[:K]}
    final = sorted(((lae(*v), p) for p, v in beam.items()), reverse=True)
    for a, b in zip(final, final[1:nbest + 1]):
        gap = min(gap, a[0] - b[0])
    return [(p, tot) for tot, p in final[:nbest]], gap, kept


def make_case(B, T, C, seed, skips=False, ragged=False):
    """``(log_probs (B, T, C) float32, lengths (B,) int32 or None)``: ``randn * 3``, 12 added to the blank logit of every third frame
    where the case uses the skip rule, ``log_softmax`` in float64 rounded to float32; ragged lengths go down to 60 %"""
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, T, C), generator=gen, dtype=torch.float64) * 3
    if skips:
        logits[:, 1::3, 0] += 12
    lengths = None
    if ragged:
        lengths = torch.tensor([T - (b * (T - (3 * T + 4) // 5)) // max(B - 1, 1) for b in range(B)], dtype=torch.int32)
    return torch.log_softmax(logits, dim=-1).float(), lengths


def expected(key, lp, lengths, K, nbest, threshold, blank=0):
    if key is not None and key in _memo:
        return _memo[key]
    T = lp.shape[1]
    out = [reference(lp[b], T if lengths is None else int(lengths[b]), K, nbest, blank, threshold) for b in range(lp.shape[0])]
    if key is not None:
        _memo[key] = out
    return out


def assert_held(got, want, nbest, what, skips=False):
    tokens, lengths, scores = (t.cpu() for t in got)
    assert tokens.dtype == torch.int32 and lengths.dtype == torch.int32 and scores.dtype == torch.float32, what
    for b, (hyps, gap, kept) in enumerate(want):
        if skips:
            assert 1 <= kept < tokens.shape[2], (what, b, kept)
        for h in range(nbest):
            if h >= len(hyps):
                assert int(lengths[b, h]) == 0 and float(scores[b, h]) == NINF and bool((tokens[b, h] == -1).all()), (what, b, h)
                continue
            p, tot = hyps[h]
            bound = 8 * max(kept, 1) * 2.0 ** -52 * max(1.0, abs(tot))
            assert gap >= 100 * bound, (what, b, 'the reference cannot decide this case', gap, bound)
            assert int(lengths[b, h]) == len(p) and tokens[b, h, :len(p)].tolist() == list(p), (what, b, h, p, tokens[b, h].tolist())
            assert bool((tokens[b, h, len(p):] == -1).all()), (what, b, h)
            err = abs(float(scores[b, h]) - tot)
            assert err <= float(np.spacing(np.float32(abs(tot)))) / 2 + bound, (what, b, h, float(scores[b, h]), tot, err)
