"""``CTCBeamDecoder`` / ``ctc_decoder``: torchaudio's ``cuda_ctc_decoder`` (``CUCTCDecoder``) over ``functional.ctc_beam_search`` —
CTC prefix beam search without a language model, on the gfx950 kernels of csrc/ctc_decode.hip for float32 device tensors."""
import dataclasses
from typing import List

import torch

from . import functional

__all__ = ['CTCHypothesis', 'CTCBeamDecoder', 'ctc_decoder']


@dataclasses.dataclass
class CTCHypothesis:
    """One hypothesis (torchaudio's ``CUCTCHypothesis``): the token ids, their strings, and the log-probability"""
    tokens: List[int]
    words: List[str]
    score: float


class CTCBeamDecoder:
    """``decoder(log_prob, encoder_out_lens) -> List[List[CTCHypothesis]]``, ``nbest`` hypotheses per batch entry, best first.

    ``tokens`` is the list of token strings, or the path of a file with one token per line; index 0 is the blank, as in
    torchaudio.  ``log_prob`` is ``(batch, time, class)`` log-softmax output with ``class == len(tokens)``, ``encoder_out_lens``
    ``(batch,)`` int32 / int64 or None.  ``words`` of a hypothesis holds the strings of its tokens.  Hypotheses that do not exist
    (fewer live prefixes than ``nbest``) are left out.  One device-to-host copy per output per call."""

    def __init__(self, tokens, nbest=1, beam_size=10, blank_skip_threshold=0.95):
        if isinstance(tokens, str):
            with open(tokens) as handle:
                tokens = [line.rstrip('\n') for line in handle]
        self.tokens = list(tokens)
        if len(self.tokens) < 2:
            raise ValueError('CTCBeamDecoder: need the blank and at least one token, got %d' % len(self.tokens))
        if not 1 <= nbest <= beam_size:
            raise ValueError('CTCBeamDecoder: need 1 <= nbest <= beam_size, got nbest %d and beam_size %d' % (nbest, beam_size))
        if not 0.0 <= blank_skip_threshold <= 1.0:
            raise ValueError('CTCBeamDecoder: blank_skip_threshold must be between 0 and 1')
        self.nbest, self.beam_size, self.blank_skip_threshold = int(nbest), int(beam_size), float(blank_skip_threshold)

    def __call__(self, log_prob, encoder_out_lens=None):
        if not isinstance(log_prob, torch.Tensor) or log_prob.dim() != 3 or log_prob.shape[2] != len(self.tokens):
            raise ValueError('CTCBeamDecoder: log_prob must be (batch, time, %d)' % len(self.tokens))
        tokens, lengths, scores = functional.ctc_beam_search(log_prob, encoder_out_lens, self.beam_size, self.nbest, 0,
                                                             self.blank_skip_threshold)
        tokens, lengths, scores = tokens.cpu().tolist(), lengths.cpu().tolist(), scores.cpu().tolist()
        out = []
        for b in range(len(scores)):
            hyps = []
            for h in range(self.nbest):
                if scores[b][h] == float('-inf'):
                    continue
                ids = tokens[b][h][:lengths[b][h]]
                hyps.append(CTCHypothesis(tokens=ids, words=[self.tokens[i] for i in ids], score=scores[b][h]))
            out.append(hyps)
        return out


def ctc_decoder(tokens, nbest=1, beam_size=10, blank_skip_threshold=0.95):
    """Build a ``CTCBeamDecoder`` (torchaudio's ``cuda_ctc_decoder`` factory)."""
    return CTCBeamDecoder(tokens, nbest=nbest, beam_size=beam_size, blank_skip_threshold=blank_skip_threshold)
