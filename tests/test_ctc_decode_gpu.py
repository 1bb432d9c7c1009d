"""-m gpu: ``ctc_beam_search`` on the gfx950 kernels (csrc/ctc_decode.hip) — strict mode and poisoned outputs on — against the dict
reference of tests/ctc_decode_rules.py (its bound and its condition).  Every call is counted: one ``tac_ctc_beam_search_f32``."""
import warnings

import pytest
import torch

import ctc_decode_rules as R

pytestmark = pytest.mark.gpu

ENTRY = 'tac_ctc_beam_search_f32'


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


def run(tac_, lp, lengths, K, nbest, thr, blank=0):
    before = dict(tac_._hip.launches)
    got = tac_.ctc_beam_search(lp, lengths, K, nbest, blank, thr)
    assert launched_since(tac_, before) == {ENTRY: 1}, launched_since(tac_, before)
    assert tuple(got[0].shape) == (lp.shape[0], nbest, lp.shape[1]) and tuple(got[1].shape) == tuple(got[2].shape)
    return got


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


@pytest.mark.parametrize('shape', [(1, 1, 2, 1, 1, 1.0), (1, 12, 5, 4, 4, 1.0), (2, 30, 7, 5, 3, .95), (3, 40, 29, 10, 10, .95),
                                   (2, 40, 29, 1, 1, .95), (2, 30, 34, 32, 32, 1.0), (2, 30, 33, 32, 1, .95),
                                   (1, 50, 301, 10, 2, .95), (1, 30, 2049, 10, 2, .95), (1, 6, 'wide + 1', 8, 1, 1.0),
                                   (1, 200, 32, 10, 3, .95)], ids=lambda v: '-'.join(str(x) for x in v))
def test_shape_list(tac, shape):
    B, T, C, K, nbest, thr = shape
    C = tac._hip.ctc_beam_wide_classes() + 1 if C == 'wide + 1' else C
    lp, lengths = R.make_case(B, T, C, seed=1, skips=thr < 1, ragged=B > 2)
    want = R.expected(('gpu', shape), lp, lengths, K, nbest, thr)
    got = run(tac, lp.cuda(), None if lengths is None else lengths.cuda(), K, nbest, thr)
    R.assert_held(got, want, nbest, repr(shape), skips=thr < 1)


def test_slice_of_a_larger_tensor(tac):
    big, _ = R.make_case(5, 47, 2 * 13 + 3, seed=12, skips=True)
    view = big.cuda()[1:4, 3:43, 1:27:2]
    assert view.stride() == (47 * 29, 29, 2) and view.data_ptr() % 16 != 0
    lengths = torch.tensor([40, 31, 24], dtype=torch.int64)
    flat = view.cpu().contiguous()
    want = R.expected(None, flat, lengths, 6, 3, .95)
    R.assert_held(run(tac, view, lengths.cuda(), 6, 3, .95), want, 3, 'slice')
    R.assert_held(run(tac, flat.cuda(), lengths.cuda(), 6, 3, .95), want, 3, 'its copy')


def test_fewer_hypotheses_than_nbest(tac):
    lp, _ = R.make_case(2, 9, 6, seed=5)
    lp[:, :, 0], lp[:, :, 1:] = -1e-3, -9.0                         # every frame skipped at 0.95: the empty prefix, score 0
    tokens, lengths, scores = run(tac, lp.cuda(), None, 4, 2, .95)
    assert lengths.tolist() == [[0, 0]] * 2 and scores.tolist() == [[0.0, float('-inf')]] * 2 and bool((tokens == -1).all())
    lp, _ = R.make_case(1, 1, 3, seed=6)                            # one frame, two tokens: three prefixes, the fourth absent
    R.assert_held(run(tac, lp.cuda(), None, 4, 4, 1.0), R.expected(None, lp, None, 4, 4, 1.0), 4, '(1, 1, 3)')
    lp, _ = R.make_case(2, 14, 6, seed=7)
    lp[:, 3:6, 2], lp[1, :, 4], lp[0, 9, 1:] = float('-inf'), float('-inf'), float('-inf')
    R.assert_held(run(tac, lp.cuda(), None, 5, 5, 1.0), R.expected(None, lp, None, 5, 5, 1.0), 5, '-inf columns')


@pytest.mark.parametrize('what', ['nan', 'length'])
def test_bad_middle_entry(tac, what):
    lp, _ = R.make_case(3, 25, 11, seed=8, skips=True)
    lengths = torch.tensor([25, 20, 22], dtype=torch.int32)
    if what == 'nan':
        lp[1, 7, 5] = float('nan')
    else:
        lengths[1] = 26
    got = run(tac, lp.cuda(), lengths.cuda(), 6, 3, .95)
    assert bool(torch.isnan(got[2][1]).all()) and got[1][1].tolist() == [0, 0, 0] and bool((got[0][1] == -1).all())
    for b in (0, 2):
        alone = run(tac, lp[b:b + 1].cuda(), lengths[b:b + 1].cuda(), 6, 3, .95)
        assert same_bits([t[b:b + 1] for t in got], alone), b
    keep = [0, 2]
    R.assert_held([t[keep] for t in got], R.expected(None, lp[keep], lengths[keep], 6, 3, .95), 3, what)


def test_two_runs_same_bits(tac):
    lp, lengths = R.make_case(4, 120, 31, seed=9, skips=True, ragged=True)
    lp, lengths = lp.cuda(), lengths.cuda()
    assert same_bits(run(tac, lp, lengths, 10, 10, .95), run(tac, lp, lengths, 10, 10, .95))
    flat = torch.log_softmax(torch.zeros((2, 40, 9)), dim=-1).cuda()    # every selection ties
    first = run(tac, flat, None, 10, 10, 1.0)
    assert same_bits(first, run(tac, flat, None, 10, 10, 1.0)) and first[1].min() >= 0


def test_routes(tac):
    lp, _ = R.make_case(2, 12, 40, seed=10)
    half = lp.half()
    cases = [('float64', lp.double().cuda(), lp, 5), ('float16', half.cuda(), half.float(), 5),
             ('expanded', lp[:1].cuda().expand(2, -1, -1), lp[:1].expand(2, -1, -1).contiguous(), 5), ('beam 33', lp.cuda(), lp, 33)]
    for what, xd, x, K in cases:
        with pytest.raises(RuntimeError, match='strict mode'):
            tac.ctc_beam_search(xd, None, K, 2, 0, 1.0)
        tac.set_strict(False)
        try:
            before = dict(tac._hip.launches)
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter('always')
                tac._ops._warned.clear()
                got = tac.ctc_beam_search(xd, None, K, 2, 0, 1.0)
            assert launched_since(tac, before) == {}, what
            assert any(issubclass(w.category, tac.CompositeRouteWarning) for w in seen), what
        finally:
            tac.set_strict(True)
        assert got[0].is_cuda
        R.assert_held(got, R.expected(None, x, None, K, 2, 1.0), 2, what)


def test_decoder_and_empty_batch(tac):
    names = ['-'] + [chr(97 + i) for i in range(8)]
    lp, lengths = R.make_case(2, 20, 9, seed=11, ragged=True)
    tokens, lens, scores = run(tac, lp.cuda(), lengths.cuda(), 5, 2, .95)
    out = tac.CTCBeamDecoder(names, nbest=2, beam_size=5)(lp.cuda(), lengths.cuda())
    for b in range(2):
        assert [h.tokens for h in out[b]] == [tokens[b, h, :int(lens[b, h])].tolist() for h in range(2)]
        assert [h.score for h in out[b]] == scores[b].tolist()
        assert all(h.words == [names[i] for i in h.tokens] for h in out[b])
    before = dict(tac._hip.launches)
    empty = tac.ctc_beam_search(torch.zeros((0, 5, 3)).cuda())
    assert launched_since(tac, before) == {} and tuple(empty[0].shape) == (0, 1, 5)
