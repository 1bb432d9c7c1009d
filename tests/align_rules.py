"""What ``forced_align`` is held to: a scalar oracle in numpy float32, a case builder, and exact comparison.

The oracle restates the definition with plain loops, one state at a time, independently of ``_composite.forced_align``: per
entry ``S = 2 Lb + 1`` states (even: blank, ``2k + 1``: ``targets[k]``), ``alpha[0][0] = lp[0][blank]``, ``alpha[0][1] =
lp[0][targets[0]]``, and for ``t >= 1`` the predecessor among ``x0 = alpha[t-1][s]``, ``x1 = alpha[t-1][s-1]``, ``x2 = alpha[t-1][s-2]``
(odd ``s >= 3`` with a label different from the one before) by strict comparisons in the order 2, 1, 0; one float32 addition per
state; end state ``S - 1`` if its alpha is greater than ``S - 2``'s; back-pointers followed to ``t = 0``.

The recursion is comparisons and single additions, so nothing is approximate: paths must be equal element for element and
scores bit for bit — kernel, composite and oracle alike.  ``'ties'`` log-probabilities are multiples of 0.25 in ``[-8, 0]``: every
partial sum is exact in float32 and equal predecessors are common, which is what exercises the tie and end-state rules."""
import numpy as np
import torch

NINF = np.float32(-np.inf)


def entry_is_bad(T, C, targets, Tb, Lb, blank):
    """the conditions under which an entry is refused (``-1`` / NaN on the device, ``ValueError`` on the CPU)"""
    L = len(targets)
    if Tb < 1 or Tb > T or Lb < 0 or Lb > L:
        return True
    used = [int(v) for v in targets[:Lb]]
    if any(v == blank or v < 0 or v >= C for v in used):
        return True
    repeats = sum(1 for i in range(1, Lb) if used[i] == used[i - 1])
    return Tb < Lb + repeats


def to_f32(values):
    """a list of Python floats, each rounded to the nearest float32 (overflow to an infinity, NaN kept)"""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(values, dtype=np.float64).astype(np.float32).tolist()


def oracle_entry(lp, targets, Tb, Lb, blank):
    """``(path (T,) int64, score (T,) float32)`` of one entry: ``lp`` (T, C) float32 numpy, ``targets`` a sequence of ints"""
    T, C = lp.shape
    path = np.full((T,), -1, dtype=np.int64)
    score = np.full((T,), np.nan, dtype=np.float32)
    if entry_is_bad(T, C, targets, Tb, Lb, blank):
        return path, score
    S = 2 * Lb + 1
    label = [blank if s % 2 == 0 else int(targets[s // 2]) for s in range(S)]
    may_skip = [s % 2 == 1 and s >= 3 and label[s] != label[s - 2] for s in range(S)]
    ninf = float('-inf')
    # alphas are float32 values held as Python floats: the sum of two of them in double, rounded once to float32 (`to_f32`, a row
    # at a time), is the float32 sum — 53 bits hold any such sum far beyond the point where a second rounding could matter
    alpha = [ninf] * S
    alpha[0] = float(lp[0, blank])
    if S > 1:
        alpha[1] = float(lp[0, label[1]])
    back = [[0] * S]
    for t in range(1, Tb):
        emit = lp[t, label].tolist()
        new, row = [ninf] * S, [0] * S
        for s in range(S):
            x0 = alpha[s]
            x1 = alpha[s - 1] if s >= 1 else ninf
            x2 = alpha[s - 2] if may_skip[s] else ninf
            if x2 > x1 and x2 > x0:
                row[s], chosen = 2, x2
            elif x1 > x0 and x1 > x2:
                row[s], chosen = 1, x1
            else:
                row[s], chosen = 0, x0
            new[s] = chosen + emit[s]
        alpha = to_f32(new)
        back.append(row)
    s = S - 1
    if S > 1 and not alpha[S - 1] > alpha[S - 2]:
        s = S - 2
    for t in range(Tb - 1, -1, -1):
        path[t] = label[s]
        s -= back[t][s]
    path[Tb:] = blank
    score[:] = 0.0
    for t in range(Tb):
        score[t] = lp[t, path[t]]
    return path, score


_memo = {}


def oracle(key, log_probs, targets, input_lengths=None, target_lengths=None, blank=0):
    """``(paths (B, T) int64, scores (B, T) float32)`` of CPU tensors; computed once per ``key`` and shared (do not write to it)"""
    if key is not None and key in _memo:
        return _memo[key]
    lp = log_probs.detach().float().numpy()
    B, T, C = lp.shape
    L = targets.shape[1]
    rows = [oracle_entry(lp[b], targets[b].tolist(), T if input_lengths is None else int(input_lengths[b]),
                         L if target_lengths is None else int(target_lengths[b]), blank) for b in range(B)]
    out = (torch.from_numpy(np.stack([r[0] for r in rows])) if B else torch.zeros((0, T), dtype=torch.int64),
           torch.from_numpy(np.stack([r[1] for r in rows])) if B else torch.zeros((0, T)))
    if key is not None:
        _memo[key] = out
    return out


def make_log_probs(B, T, C, mode, seed):
    g = torch.Generator().manual_seed(seed)
    if mode == 'softmax':
        return torch.log_softmax(torch.randn((B, T, C), generator=g), dim=-1)
    assert mode == 'ties'
    return -0.25 * torch.randint(0, 33, (B, T, C), generator=g).float()


def make_targets(B, L, C, blank, seed, repeat_first=False, dtype=torch.int64):
    """labels other than the blank; a third of the positions repeat the label before (``repeat_first``: position 1 does)"""
    g = torch.Generator().manual_seed(seed + 1000)
    t = torch.randint(0, C - 1, (B, L), generator=g)
    t = t + (t >= blank).long()
    if L > 1:
        again = torch.rand((B, L), generator=g) < (1.0 / 3.0 if C > 2 else 1.0)
        if repeat_first:
            again[:, 1] = True
        for i in range(1, L):
            t[:, i] = torch.where(again[:, i], t[:, i - 1], t[:, i])
    return t.to(dtype)


def repeats(targets_row, Lb):
    return sum(1 for i in range(1, Lb) if int(targets_row[i]) == int(targets_row[i - 1]))


def make_case(B, T, L, C, mode, seed=0, blank=0, ragged=False, dtype=torch.int64):
    """``(log_probs, targets, input_lengths, target_lengths)`` on the CPU.  ``T == 'tight'``: exactly ``L + R`` frames.  ``ragged``:
    lengths fall to 60 % over the batch, every entry kept feasible; otherwise both lengths are None."""
    targets = make_targets(B, L, C, blank, seed, dtype=dtype)
    if T == 'tight':
        T = max(1, max(L + repeats(targets[b], L) for b in range(B)))
    log_probs = make_log_probs(B, T, C, mode, seed)
    if not ragged:
        return log_probs, targets, None, None
    share = [1.0 - 0.4 * b / max(B - 1, 1) for b in range(B)]
    tl = [int(round(L * f)) for f in share]
    il = [max(int(round(T * f)), tl[b] + repeats(targets[b], tl[b]), 1) for b, f in enumerate(share)]
    assert max(il) <= T
    return log_probs, targets, torch.tensor(il, dtype=torch.int32), torch.tensor(tl, dtype=torch.int32)


def assert_same(got, want, what):
    """paths equal element for element, scores equal bit for bit (a NaN equals only the same NaN bits' class: both NaN)"""
    gp, gs = got[0].cpu(), got[1].cpu()
    wp, ws = want
    assert tuple(gp.shape) == tuple(wp.shape) and tuple(gs.shape) == tuple(ws.shape), what
    assert torch.equal(gp.long(), wp.long()), '%s: %d of %d path elements differ' % (what, int((gp.long() != wp.long()).sum()),
                                                                                      wp.numel())
    gs, ws = gs.float(), ws.float()
    both_nan = torch.isnan(gs) & torch.isnan(ws)
    same = (gs.contiguous().view(torch.int32) == ws.contiguous().view(torch.int32)) | both_nan
    assert bool(same.all()), '%s: %d of %d scores differ in bits' % (what, int((~same).sum()), ws.numel())


def collapse(path, blank):
    out, prev = [], None
    for v in path:
        if v != prev and v != blank:
            out.append(int(v))
        prev = v
    return out
