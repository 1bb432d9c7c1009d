"""-m gpu: ``forced_align`` on the gfx950 kernel (csrc/align.hip) — strict mode and poisoned outputs on.

Reference: the scalar float32 oracle of tests/align_rules.py.  The recursion is comparisons and single additions, so the
comparison is exact: equal paths, bit-equal scores, in both the 'softmax' and the 'ties' mode.  Every device call is counted:
ONE launch.  Shapes are the smallest at which each mechanism of the kernel can go wrong; the thresholds come from the kernel's
own constants (a lane per pair of states, 64 pairs per wave, one wave without a barrier and several with one; 6144 back-pointer
words in the LDS, 3 per wave and step, in chunks of at most 2048 steps)."""
import warnings

import pytest
import torch

import align_rules as A

pytestmark = pytest.mark.gpu

ENTRY = 'tac_forced_align_f32'
MODES = ['softmax', 'ties']
BP_WORDS, STAGE = 6144, 2048


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    yield t
    t._hip.set_poison_outputs(False)
    t.set_strict(False)
    t.set_lazy_fusion(True)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def dev(t):
    return None if t is None else t.cuda()


def run(tac_, lp, tg, il=None, tl=None, blank=0):
    """the public functional on device tensors, the launches counted: one, and no composite route (strict mode)"""
    before = dict(tac_._hip.launches)
    paths, scores = tac_.forced_align(lp, tg, il, tl, blank)
    assert launched_since(tac_, before) == {ENTRY: 1}, launched_since(tac_, before)
    assert paths.dtype == tg.dtype and scores.dtype == torch.float32
    assert tuple(paths.shape) == tuple(lp.shape[:2]) == tuple(scores.shape)
    return paths, scores


def held(tac_, shape, mode, seed=1, ragged=False, blank=0, dtype=torch.int64):
    B, T, L, C = shape
    case = A.make_case(B, T, L, C, mode, seed=seed, blank=blank, ragged=ragged, dtype=dtype)
    want = A.oracle(('gpu', shape, mode, seed, ragged, blank), *case, blank=blank)
    got = run(tac_, *(dev(t) for t in case), blank=blank)
    A.assert_same(got, want, '(B, T, L, C) = %r, %s' % (shape, mode))
    return case, got


def chunk_rows(waves):
    return min(STAGE, BP_WORDS // (3 * waves))


# ----------------------------------------------------------------------------- 1. the shape list
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape,ragged', [((1, 1, 1, 2), False), ((1, 5, 0, 3), False), ((1, 7, 3, 4), False),
                                          ((1, 'tight', 5, 6), False), ((3, 40, 9, 29), True), ((2, 90, 63, 17), False),
                                          ((2, 140, 64, 17), True), ((2, 140, 65, 17), False)],
                         ids=lambda v: '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_shape_list(tac, shape, ragged, mode):
    """the smallest case; no targets; a repeat; exactly L + R frames (one forced path); ragged lengths down to 60 %; 64, 65 and 66
    pairs of states: the last lane of one wave, then two waves and the hand-over through the LDS"""
    held(tac, shape, mode, seed=3, ragged=ragged)


def test_repeat_at_the_front_and_tight(tac):
    """targets [a, a, b]: R = 1, T = L + R + 3; and T = L + R exactly"""
    lp = A.make_log_probs(1, 7, 4, 'ties', 11)
    tg = torch.tensor([[2, 2, 3]])
    A.assert_same(run(tac, lp.cuda(), tg.cuda()), A.oracle(None, lp, tg), '[a, a, b], T = 7')
    A.assert_same(run(tac, lp[:, :4].cuda(), tg.cuda()), A.oracle(None, lp[:, :4], tg), '[a, a, b], T = 4')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('L', [127, 128, 300])
def test_more_waves(tac, L, mode):
    """L + 1 = 128 | 129: two full waves, then a third with one pair; 301 pairs: five waves, a partial last one"""
    held(tac, (2, L + L // 2, L, 11), mode, seed=L, ragged=True)


def test_most_targets(tac):
    """L + 1 = 1024: sixteen waves"""
    L = tac._hip.align_max_targets() - 1
    assert L == 1023
    lp = A.make_log_probs(1, L + 9, 4, 'ties', 2)
    tg = (1 + torch.arange(L) % 3)[None]                            # no repeats: L + 9 frames leave room to choose
    want = A.oracle(('most',), lp, tg)
    assert int(want[0].min()) >= 0
    A.assert_same(run(tac, lp.cuda(), tg.cuda()), want, 'L + 1 = 1024')


# ----------------------------------------------------------------------------- 2. back-pointers beyond the LDS plan
@pytest.mark.parametrize('L,waves,chunks,mode', [(2, 1, 2, 'softmax'), (2, 1, 1, 'ties'), (70, 2, 1, 'ties'), (260, 5, 1, 'softmax')])
def test_workspace_and_chunked_backtrack(tac, L, waves, chunks, mode):
    """Tb - 1 one more than `chunks` chunks of rows hold — the smallest T at which the back-pointers leave the LDS (`chunks` = 1),
    with one wave and with several: they go to the workspace and come back in chunks + 1 pieces, the last of one row.  The
    second entry of the batch is shorter and stays in the LDS."""
    rows = chunk_rows(waves)
    T = chunks * rows + 2
    assert tac._native.lib().tac_forced_align_workspace(2, T, L + 1) == 2 * (T - 1) * 3 * waves * 8
    assert tac._native.lib().tac_forced_align_workspace(2, rows + 1, L + 1) == 0
    B, C = 2, 5
    lp = A.make_log_probs(B, T, C, mode, L)
    tg = A.make_targets(B, L, C, 0, L)
    need = max(L + A.repeats(tg[b], L) for b in range(B))
    assert need <= rows - 3
    il = torch.tensor([T, rows - 3], dtype=torch.int32)
    want = A.oracle(('spill', L, chunks, mode), lp, tg, il, None)
    assert int(want[0].min()) >= 0
    A.assert_same(run(tac, lp.cuda(), tg.cuda(), il.cuda(), None), want, 'L = %d, T = %d' % (L, T))


# ----------------------------------------------------------------------------- 3. layouts and dtypes
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_target_dtypes_and_blank_elsewhere(tac, dtype):
    for blank in (0, 4, 8):
        held(tac, (3, 33, 10, 9), 'ties', seed=4, ragged=True, blank=blank, dtype=dtype)


def test_length_dtypes(tac):
    lp, tg, il, tl = A.make_case(3, 33, 10, 9, 'softmax', seed=4, ragged=True)
    want = A.oracle(None, lp, tg, il, tl)
    A.assert_same(run(tac, lp.cuda(), tg.cuda(), il.long().cuda(), tl.long().cuda()), want, 'int64 lengths')
    A.assert_same(run(tac, lp.cuda(), tg.cuda(), il.cuda(), None), A.oracle(None, lp, tg, il, None), 'target_lengths None')


@pytest.mark.parametrize('mode', MODES)
def test_slice_of_a_larger_tensor(tac, mode):
    """batch, time and class strides all non-trivial, the base not 16-byte aligned: read in place, no composite route"""
    big = A.make_log_probs(5, 47, 2 * 13 + 3, mode, 12).cuda()
    view = big[1:4, 3:43, 1:27:2]
    assert view.stride() == (47 * 29, 29, 2) and view.data_ptr() % 16 != 0
    tg = A.make_targets(3, 8, 13, 0, 12)
    il = torch.tensor([40, 31, 24], dtype=torch.int32)
    tl = torch.tensor([8, 6, 5], dtype=torch.int32)
    want = A.oracle(None, view.cpu().contiguous(), tg, il, tl)
    A.assert_same(run(tac, view, tg.cuda(), il.cuda(), tl.cuda()), want, 'slice, %s' % mode)
    A.assert_same(run(tac, view.contiguous(), tg.cuda(), il.cuda(), tl.cuda()), want, 'its copy, %s' % mode)


def test_minus_infinity_columns(tac):
    lp, tg, _, _ = A.make_case(2, 21, 6, 5, 'softmax', seed=9)
    lp[:, 3:6, 0] = float('-inf')
    lp[1, :, 2] = float('-inf')
    lp[0, 10, :] = float('-inf')
    A.assert_same(run(tac, lp.cuda(), tg.cuda()), A.oracle(None, lp, tg), '-inf columns')


def test_nan_goes_where_the_comparisons_send_it(tac):
    lp, tg, _, _ = A.make_case(1, 9, 3, 4, 'softmax', seed=8)
    lp[0, 2, 0] = float('nan')
    got, want = run(tac, lp.cuda(), tg.cuda()), A.oracle(None, lp, tg)
    A.assert_same(got, want, 'NaN at frame 2')
    assert torch.equal(torch.isnan(got[1].cpu()), torch.isnan(want[1]))


# ----------------------------------------------------------------------------- 4. refused entries, determinism
@pytest.mark.parametrize('what', ['infeasible', 'blank', 'range', 'negative', 'input_length', 'target_length'])
def test_refused_middle_entry(tac, what):
    """the middle entry is all -1 / NaN; its neighbours have the bits they have when run alone"""
    B, T, L, C = 3, 30, 6, 7
    lp = A.make_log_probs(B, T, C, 'ties', 21)
    tg = A.make_targets(B, L, C, 0, 21)
    il, tl = torch.tensor([30, 20, 25], dtype=torch.int32), torch.tensor([6, 5, 4], dtype=torch.int32)
    if what == 'infeasible':
        tg[1] = torch.tensor([3, 3, 3, 2, 2, 1])
        il[1] = 5 + 3 - 1                                           # Tb = Lb + R - 1
    elif what == 'blank':
        tg[1, 2] = 0
    elif what == 'range':
        tg[1, 4] = C
    elif what == 'negative':
        tg[1, 0] = -3
    elif what == 'input_length':
        il[1] = T + 1
    else:
        tl[1] = L + 1
    paths, scores = run(tac, lp.cuda(), tg.cuda(), il.cuda(), tl.cuda())
    assert bool((paths[1] == -1).all()) and bool(torch.isnan(scores[1]).all())
    want = A.oracle(None, lp, tg, il, tl)
    A.assert_same((paths, scores), want, what)
    for b in (0, 2):
        alone = run(tac, lp[b:b + 1].cuda(), tg[b:b + 1].cuda(), il[b:b + 1].cuda(), tl[b:b + 1].cuda())
        assert torch.equal(alone[0][0], paths[b])
        assert torch.equal(alone[1][0].view(torch.int32), scores[b].view(torch.int32))


def test_bad_value_past_the_length_is_not_used(tac):
    lp, tg, il, tl = A.make_case(2, 20, 6, 7, 'softmax', seed=5, ragged=True)
    tg[1, int(tl[1]):] = 99
    A.assert_same(run(tac, lp.cuda(), tg.cuda(), il.cuda(), tl.cuda()), A.oracle(None, lp, tg, il, tl), 'unused targets')


def test_two_runs_same_bits(tac):
    lp, tg, il, tl = (dev(t) for t in A.make_case(4, 200, 70, 31, 'softmax', seed=13, ragged=True))
    a, b = run(tac, lp, tg, il, tl), run(tac, lp, tg, il, tl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_empty_batch_launches_nothing(tac):
    before = dict(tac._hip.launches)
    paths, scores = tac.forced_align(torch.zeros((0, 5, 3)).cuda(), torch.zeros((0, 2), dtype=torch.int64).cuda())
    assert launched_since(tac, before) == {} and tuple(paths.shape) == (0, 5) == tuple(scores.shape)


# ----------------------------------------------------------------------------- 5. routes
def test_routes(tac):
    """float32, contiguous or sliced, is the kernel (every `run` above, strict); float64, half precision, an expanded view and
    L + 1 over the limit raise under strict mode and give the oracle's result, announced, when it is off"""
    lp, tg, _, _ = A.make_case(2, 12, 4, 6, 'ties', seed=14)
    limit = tac._hip.align_max_targets()
    long_tg = torch.ones((1, limit), dtype=torch.int64)
    long_tg[0, 1::2] = 2
    long_lp = A.make_log_probs(1, limit + 4, 3, 'ties', 15)
    half = lp.half()                                                # (multiples of 0.25 down to -8: exact in half, sums to 2048)
    cases = [('float64', lp.double(), tg, A.oracle(None, lp, tg)),
             ('float16', half, tg, None),
             ('expanded', lp[:1].expand(2, -1, -1), tg, A.oracle(None, lp[:1].expand(2, -1, -1).contiguous(), tg)),
             ('over the limit', long_lp, long_tg, A.oracle(None, long_lp, long_tg))]
    for what, x, targets, want in cases:
        xd = x.cuda() if what != 'expanded' else lp[:1].cuda().expand(2, -1, -1)
        with pytest.raises(RuntimeError, match='strict mode'):
            tac.forced_align(xd, targets.cuda())
        tac.set_strict(False)
        try:
            before = dict(tac._hip.launches)
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter('always')
                tac._ops._warned.clear()
                got = tac.forced_align(xd, targets.cuda())
            assert launched_since(tac, before) == {}, what
            assert any(issubclass(w.category, tac.CompositeRouteWarning) for w in seen), what
        finally:
            tac.set_strict(True)
        assert got[1].dtype == x.dtype and got[0].dtype == targets.dtype
        if want is None:                                            # half: against the composite on the CPU, same arithmetic
            cpu = tac.forced_align(x, targets)
            assert torch.equal(got[0].cpu(), cpu[0]) and torch.equal(got[1].cpu().view(torch.int16), cpu[1].view(torch.int16))
        else:
            A.assert_same(got, want, what)


def test_gradient_of_scores(tac):
    lp, tg, il, tl = A.make_case(2, 15, 4, 6, 'softmax', seed=16, ragged=True)
    x = lp.cuda().requires_grad_(True)
    before = dict(tac._hip.launches)
    paths, scores = tac.forced_align(x, tg.cuda(), il.cuda(), tl.cuda())
    assert launched_since(tac, before) == {ENTRY: 1}
    assert not paths.requires_grad
    with pytest.raises(RuntimeError, match='strict mode'):         # the backward is torch operators: announced
        scores.sum().backward(retain_graph=True)
    tac.set_strict(True, backward=False)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', tac.CompositeRouteWarning)
            scores.sum().backward()
    finally:
        tac.set_strict(True)
    want = torch.zeros_like(lp)
    p = paths.cpu()
    for b in range(2):
        for t in range(int(il[b])):
            want[b, t, p[b, t]] = 1.0
    assert torch.equal(x.grad.cpu(), want)


def test_merge_tokens_on_device_tensors(tac):
    lp, tg, _, _ = A.make_case(1, 60, 9, 12, 'softmax', seed=17)
    paths, scores = run(tac, lp.cuda(), tg.cuda())
    spans = tac.merge_tokens(paths[0], scores[0])
    assert spans == tac.merge_tokens(paths[0].cpu(), scores[0].cpu())
    assert [s.token for s in spans] == tg[0].tolist()
