"""not-gpu: ``forced_align`` / ``merge_tokens`` / ``TokenSpan`` on CPU tensors — the oracle of tests/align_rules.py against brute
force, the torch-operator composite against the oracle (exactly: equal paths, bit-equal scores), the argument checks, the fake
kernel and ``torch.compile``."""
import itertools
import warnings

import numpy as np
import pytest
import torch

import align_rules as A

MODES = ['softmax', 'ties']

#: (B, T, L, C, ragged) — the shape list the device tests use as well
SHAPES = [(1, 1, 1, 2, False), (1, 5, 0, 3, False), (1, 7, 3, 4, False), (1, 'tight', 5, 6, False), (3, 40, 9, 29, True),
          (2, 90, 63, 17, False), (2, 140, 64, 17, True), (2, 140, 65, 17, False)]


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


# ----------------------------------------------------------------------------- 1. the oracle against brute force
def _labellings(T, target, C, blank):
    for frames in itertools.product(range(C), repeat=T):
        if A.collapse(frames, blank) == list(target):
            yield frames


@pytest.mark.parametrize('T', [1, 2, 3, 4, 5, 6])
def test_oracle_is_the_best_labelling(T):
    """every target of up to 3 labels over C = 3 (blank 0; repeated labels included), every feasible T <= 6, 'ties' mode: the
    oracle's path collapses to the target and its total is the maximum over ALL labellings that do (sums are exact)"""
    C, blank, checked = 3, 0, 0
    for L in range(0, 4):
        for target in itertools.product([1, 2], repeat=L):
            if T < L + A.repeats(target, L):
                continue
            lp = A.make_log_probs(1, T, C, 'ties', seed=17 * T + L)[0].numpy()
            best = max(sum(float(lp[t, v]) for t, v in enumerate(frames)) for frames in _labellings(T, target, C, blank))
            path, score = A.oracle_entry(lp, list(target), T, L, blank)
            assert A.collapse(path.tolist(), blank) == list(target), (T, target, path)
            assert float(score.astype(np.float64).sum()) == best, (T, target, path, best)
            checked += 1
    assert checked >= 1


def test_oracle_marks_bad_entries():
    lp = A.make_log_probs(1, 3, 4, 'ties', 0)[0].numpy()
    for targets, Tb, Lb in [([1, 1], 2, 2), ([0, 1], 3, 2), ([1, 4], 3, 2), ([1], 4, 1), ([1], 0, 1), ([1], 3, 2)]:
        path, score = A.oracle_entry(lp, targets, Tb, Lb, 0)
        assert (path == -1).all() and np.isnan(score).all()


# ----------------------------------------------------------------------------- 2. the composite against the oracle
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '-'.join(str(v) for v in s))
def test_composite_equals_oracle(tac, shape, mode):
    B, T, L, C, ragged = shape
    for dtype in (torch.int64, torch.int32):
        lp, tg, il, tl = A.make_case(B, T, L, C, mode, seed=3, ragged=ragged, dtype=dtype)
        paths, scores = tac.forced_align(lp, tg, il, tl)
        assert paths.dtype == dtype and scores.dtype == torch.float32 and tuple(paths.shape) == tuple(lp.shape[:2])
        A.assert_same((paths, scores), A.oracle(('cpu', shape, mode), lp, tg, il, tl), '%r %s' % (shape, mode))


def test_composite_blank_elsewhere_and_float64(tac):
    lp, tg, il, tl = A.make_case(2, 12, 4, 7, 'ties', seed=5, blank=3, ragged=True)
    A.assert_same(tac.forced_align(lp, tg, il, tl, blank=3), A.oracle(None, lp, tg, il, tl, blank=3), 'blank 3')
    paths, scores = tac.forced_align(lp.double(), tg, il, tl, blank=3)
    assert scores.dtype == torch.float64
    A.assert_same((paths, scores), A.oracle(None, lp, tg, il, tl, blank=3), 'float64 (exact sums)')


def test_nan_goes_where_the_comparisons_send_it(tac):
    lp, tg, _, _ = A.make_case(1, 9, 3, 4, 'softmax', seed=8)
    lp[0, 2, 0] = float('nan')
    got, want = tac.forced_align(lp, tg), A.oracle(None, lp, tg)
    A.assert_same(got, want, 'NaN at frame 2')
    assert torch.equal(torch.isnan(got[1]), torch.isnan(want[1]))


def test_minus_infinity_columns(tac):
    lp, tg, _, _ = A.make_case(2, 11, 4, 5, 'softmax', seed=9)
    lp[:, 3:6, 0] = float('-inf')
    lp[1, :, 2] = float('-inf')
    A.assert_same(tac.forced_align(lp, tg), A.oracle(None, lp, tg), '-inf columns')


def test_empty_batch(tac):
    paths, scores = tac.forced_align(torch.zeros((0, 5, 3)), torch.zeros((0, 2), dtype=torch.int64))
    assert tuple(paths.shape) == (0, 5) and tuple(scores.shape) == (0, 5) and paths.dtype == torch.int64


# ----------------------------------------------------------------------------- 3. checks
def test_argument_checks(tac):
    lp, tg = torch.zeros((2, 5, 4)), torch.ones((2, 3), dtype=torch.int64)
    ok = torch.tensor([5, 5])
    bad_calls = [
        lambda: tac.forced_align(lp[0], tg),                                         # dimensionality
        lambda: tac.forced_align(lp, tg[0]),
        lambda: tac.forced_align(lp, tg, ok[:, None]),
        lambda: tac.forced_align(lp.long(), tg),                                     # dtypes
        lambda: tac.forced_align(lp, tg.float()),
        lambda: tac.forced_align(lp, tg.to(torch.int16)),
        lambda: tac.forced_align(lp, tg, ok.float()),
        lambda: tac.forced_align(lp, tg, blank=4),                                   # blank
        lambda: tac.forced_align(lp, tg, blank=-1),
        lambda: tac.forced_align(lp, tg[:1]),                                        # batch sizes
        lambda: tac.forced_align(lp, tg, ok[:1]),
        lambda: tac.forced_align(lp, tg, ok, torch.tensor([3, 3, 3])),
        lambda: tac.forced_align(lp[:, :0], tg),                                     # empty axes
        lambda: tac.forced_align(lp[:, :, :0], tg),
        lambda: tac.forced_align(lp, tg.to('meta')),                                 # devices
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError, match='forced_align'):
            call()
            pytest.fail('call %d was accepted' % i)


def test_cpu_values_raise_naming_the_entry(tac):
    lp = A.make_log_probs(3, 6, 5, 'softmax', 0)
    good = torch.tensor([[1, 2, 3], [1, 2, 3], [1, 2, 3]])

    def targets(row):
        t = good.clone()
        t[1] = torch.tensor(row)
        return t
    with pytest.raises(ValueError, match='entry 1.*cannot hold'):
        tac.forced_align(lp, targets([2, 2, 2]), torch.tensor([6, 4, 6]), None)      # Tb = Lb + R - 1
    with pytest.raises(ValueError, match='entry 1.*blank'):
        tac.forced_align(lp, targets([1, 0, 3]))
    with pytest.raises(ValueError, match='entry 1.*outside the 5 classes'):
        tac.forced_align(lp, targets([1, 5, 3]))
    with pytest.raises(ValueError, match='entry 1.*outside the 5 classes'):
        tac.forced_align(lp, targets([1, -2, 3]))
    with pytest.raises(ValueError, match='entry 2.*input length'):
        tac.forced_align(lp, good, torch.tensor([6, 6, 7]))
    with pytest.raises(ValueError, match='entry 0.*input length'):
        tac.forced_align(lp, good, torch.tensor([0, 6, 6]))
    with pytest.raises(ValueError, match='entry 2.*target length'):
        tac.forced_align(lp, good, None, torch.tensor([3, 3, 4]))
    # a bad value past the entry's own length is not used
    tac.forced_align(lp, targets([1, 2, 0]), None, torch.tensor([3, 2, 3]))


# ----------------------------------------------------------------------------- 4. merge_tokens / TokenSpan
def test_merge_tokens(tac):
    tokens = torch.tensor([0, 3, 3, 0, 0, 5, 3, 3, 3, 0])
    scores = torch.tensor([-1.0, -0.5, -1.5, -9.0, -9.0, -0.25, -1.0, -2.0, -3.0, -7.0])
    spans = tac.merge_tokens(tokens, scores)
    assert spans == [tac.TokenSpan(3, 1, 3, -1.0), tac.TokenSpan(5, 5, 6, -0.25), tac.TokenSpan(3, 6, 9, -2.0)]
    assert [len(s) for s in spans] == [2, 1, 3]
    assert tac.functional.merge_tokens is tac.merge_tokens and tac.functional.TokenSpan is tac.TokenSpan
    # another blank: the zeros become spans, the threes are dropped
    assert [(s.token, s.start, s.end) for s in tac.merge_tokens(tokens, scores, blank=3)] == \
        [(0, 0, 1), (0, 3, 5), (5, 5, 6), (0, 9, 10)]
    assert tac.merge_tokens(torch.zeros(4, dtype=torch.int64), torch.zeros(4)) == []
    assert tac.merge_tokens(torch.tensor([2]), torch.tensor([-0.5])) == [tac.TokenSpan(2, 0, 1, -0.5)]
    assert tac.merge_tokens(torch.tensor([0]), torch.tensor([-0.5])) == []
    with pytest.raises(ValueError, match='same length'):
        tac.merge_tokens(tokens, scores[:-1])
    with pytest.raises(ValueError, match='1D'):
        tac.merge_tokens(tokens[None], scores[None])
    with pytest.raises(ValueError, match='1D'):
        tac.merge_tokens(tokens, scores[None])


def test_merge_tokens_of_an_alignment(tac):
    lp, tg, _, _ = A.make_case(1, 30, 6, 9, 'softmax', seed=4)
    paths, scores = tac.forced_align(lp, tg)
    spans = tac.merge_tokens(paths[0], scores[0])
    assert [s.token for s in spans] == tg[0].tolist()
    for s in spans:
        assert s.score == pytest.approx(float(scores[0, s.start:s.end].double().mean()), rel=1e-12)


# ----------------------------------------------------------------------------- 5. op plumbing
def test_gradient_is_the_scatter_at_paths(tac):
    lp, tg, il, tl = A.make_case(2, 10, 3, 5, 'softmax', seed=6, ragged=True)
    x = lp.clone().requires_grad_(True)
    paths, scores = tac.forced_align(x, tg, il, tl)
    assert not paths.requires_grad and scores.requires_grad
    w = torch.linspace(0.5, 2.0, 20).reshape(2, 10)
    (scores * w).sum().backward()
    want = torch.zeros_like(lp)
    for b in range(2):
        for t in range(int(il[b])):
            want[b, t, paths[b, t]] = w[b, t]
    assert torch.equal(x.grad, want)


def test_fake_kernel_shapes_and_dtypes(tac):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        lp = torch.empty((3, 11, 7), dtype=torch.float16)
        tg = torch.empty((3, 4), dtype=torch.int32)
        paths, scores = torch.ops.tac_amd.forced_align(lp, tg, None, None, 0)
        assert tuple(paths.shape) == (3, 11) and paths.dtype == torch.int32
        assert tuple(scores.shape) == (3, 11) and scores.dtype == torch.float16


def test_torch_compile_fullgraph(tac):
    lp, tg, il, tl = A.make_case(2, 10, 3, 5, 'ties', seed=7, ragged=True)

    def fn(x, targets, a, b):
        paths, scores = tac.forced_align(x * 1.0, targets, a, b)
        return paths, scores * 1.0

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = torch.compile(fn, fullgraph=True, backend='aot_eager')(lp, tg, il, tl)
    A.assert_same(got, A.oracle(None, lp, tg, il, tl), 'torch.compile')
