"""``torchaudio.compliance.kaldi`` call sites: ``fbank`` with torchaudio's signature and defaults, on ``functional.kaldi_fbank``.

    from torchaudio_contrib_amd import kaldi
    feats = kaldi.fbank(waveform, num_mel_bins=80, sample_frequency=16000.0)        # (channels, time) -> (frames, 80)
"""
from . import functional as F

__all__ = ['fbank']


def fbank(waveform, blackman_coeff=0.42, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0,
          high_freq=0.0, htk_compat=False, low_freq=20.0, min_duration=0.0, num_mel_bins=23, preemphasis_coefficient=0.97,
          raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True, sample_frequency=16000.0, snip_edges=True,
          subtract_mean=False, use_energy=False, use_log_fbank=True, use_power=True, vtln_high=-500.0, vtln_low=100.0,
          vtln_warp=1.0, window_type='povey'):
    """``(channels, time)`` → ``(frames, num_mel_bins [+ 1])`` of channel ``max(channel, 0)``: see ``functional.kaldi_fbank``.
    A waveform shorter than ``min_duration`` seconds gives an empty ``(0, num_mel_bins [+ 1])`` result, as one shorter than a
    frame does."""
    if waveform.dim() != 2:
        raise ValueError('kaldi.fbank: expected a waveform of shape (channels, time), got %s' % (tuple(waveform.shape),))
    row = waveform[max(int(channel), 0)]
    if row.shape[-1] < min_duration * sample_frequency:
        row = row[:0]
    return F.kaldi_fbank(row, blackman_coeff=blackman_coeff, dither=dither, energy_floor=energy_floor, frame_length=frame_length,
                         frame_shift=frame_shift, high_freq=high_freq, htk_compat=htk_compat, low_freq=low_freq,
                         num_mel_bins=num_mel_bins, preemphasis_coefficient=preemphasis_coefficient, raw_energy=raw_energy,
                         remove_dc_offset=remove_dc_offset, round_to_power_of_two=round_to_power_of_two,
                         sample_frequency=sample_frequency, snip_edges=snip_edges, subtract_mean=subtract_mean,
                         use_energy=use_energy, use_log_fbank=use_log_fbank, use_power=use_power, vtln_high=vtln_high,
                         vtln_low=vtln_low, vtln_warp=vtln_warp, window_type=window_type)
