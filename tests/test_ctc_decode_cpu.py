"""not-gpu: ``ctc_beam_search`` / ``CTCBeamDecoder`` on CPU tensors — the composite against the dict reference of
tests/ctc_decode_rules.py, the argument checks, the decoder class and the exports."""
import pytest
import torch

import ctc_decode_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


@pytest.mark.parametrize('shape', [(1, 12, 5, 4, 4, 1.0), (3, 40, 29, 10, 10, .95), (2, 30, 33, 32, 1, .95)],
                         ids=lambda v: '-'.join(str(x) for x in v))
def test_composite_against_the_reference(tac, shape):
    B, T, C, K, nbest, thr = shape
    lp, lengths = R.make_case(B, T, C, seed=1, skips=thr < 1, ragged=B > 2)
    got = tac.ctc_beam_search(lp, lengths, K, nbest, 0, thr)
    assert tuple(got[0].shape) == (B, nbest, T) and tuple(got[1].shape) == (B, nbest) == tuple(got[2].shape)
    R.assert_held(got, R.expected(('cpu', shape), lp, lengths, K, nbest, thr), nbest, repr(shape), skips=thr < 1)


def test_other_blank_and_float64(tac):
    lp, _ = R.make_case(2, 20, 9, seed=2)
    want = R.expected(None, lp, None, 5, 3, 1.0, blank=4)
    R.assert_held(tac.ctc_beam_search(lp, None, 5, 3, 4, 1.0), want, 3, 'blank 4')
    R.assert_held(tac.ctc_beam_search(lp.double(), None, 5, 3, 4, 1.0), want, 3, 'float64')


def test_argument_checks(tac):
    lp, _ = R.make_case(2, 6, 4, seed=3)
    ok = torch.tensor([6, 5])
    for bad in (lambda: tac.ctc_beam_search(lp[0]), lambda: tac.ctc_beam_search(lp.long()),
                lambda: tac.ctc_beam_search(lp[:, :, :1]), lambda: tac.ctc_beam_search(lp[:, :0]),
                lambda: tac.ctc_beam_search(lp, ok.float()), lambda: tac.ctc_beam_search(lp, ok[:1]),
                lambda: tac.ctc_beam_search(lp, ok.to('meta')), lambda: tac.ctc_beam_search(lp, blank=4),
                lambda: tac.ctc_beam_search(lp, beam_size=0), lambda: tac.ctc_beam_search(lp, beam_size=3, nbest=4),
                lambda: tac.ctc_beam_search(lp, blank_skip_threshold=float('nan')),
                lambda: tac.ctc_beam_search(lp, torch.tensor([6, 7])), lambda: tac.ctc_beam_search(lp, torch.tensor([-1, 6]))):
        with pytest.raises(ValueError, match='ctc_beam_search'):
            bad()
    tokens, lengths, scores = tac.ctc_beam_search(lp, torch.tensor([0, 6]), nbest=2, blank_skip_threshold=1.0)
    assert lengths[0].tolist() == [0, 0] and scores[0].tolist() == [0.0, float('-inf')] and bool((tokens[0] == -1).all())
    assert tuple(tac.ctc_beam_search(torch.zeros((0, 5, 3)))[0].shape) == (0, 1, 5)


def test_decoder_from_a_list_and_a_file(tac, tmp_path):
    names = ['<blk>', 'a', 'b', 'c', '|']
    lp, lengths = R.make_case(2, 15, 5, seed=4, ragged=True)
    path = tmp_path / 'tokens.txt'
    path.write_text('\n'.join(names) + '\n')
    tokens, lens, scores = tac.ctc_beam_search(lp, lengths, 4, 2, 0, 1.0)
    for decoder in (tac.CTCBeamDecoder(names, nbest=2, beam_size=4, blank_skip_threshold=1.0),
                    tac.ctc_decoder(str(path), nbest=2, beam_size=4, blank_skip_threshold=1.0)):
        out = decoder(lp, lengths)
        assert [len(hyps) for hyps in out] == [2, 2]
        for b in range(2):
            for h in range(2):
                ids = tokens[b, h, :int(lens[b, h])].tolist()
                assert out[b][h] == tac.CTCHypothesis(tokens=ids, words=[names[i] for i in ids], score=float(scores[b, h]))
    with pytest.raises(ValueError, match='CTCBeamDecoder'):
        tac.CTCBeamDecoder(names, nbest=3, beam_size=2)
    with pytest.raises(ValueError, match='CTCBeamDecoder'):
        tac.CTCBeamDecoder(names)(lp[:, :, :4])


def test_exports(tac):
    assert 'ctc_beam_search' in tac.functional.__all__ and tac.functional.ctc_beam_search is tac.ctc_beam_search
    assert set(tac.decoder.__all__) == {'CTCHypothesis', 'CTCBeamDecoder', 'ctc_decoder'}
    assert tac.CTCBeamDecoder is tac.decoder.CTCBeamDecoder and tac.ctc_decoder is tac.decoder.ctc_decoder
