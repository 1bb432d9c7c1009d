"""``torchaudio.compliance.kaldi`` call sites: ``fbank``, ``mfcc`` and ``spectrogram`` with torchaudio's signatures and defaults,
on ``functional.kaldi_fbank`` / ``kaldi_mfcc`` / ``kaldi_spectrogram``.

    from torchaudio_contrib_amd import kaldi
    feats = kaldi.fbank(waveform, num_mel_bins=80, sample_frequency=16000.0)        # (channels, time) -> (frames, 80)
    ceps = kaldi.mfcc(waveform, num_mel_bins=30, num_ceps=24)                       # (channels, time) -> (frames, 24)
    spec = kaldi.spectrogram(waveform)                                              # (channels, time) -> (frames, 257)
"""
from . import functional as F

__all__ = ['fbank', 'mfcc', 'spectrogram']


def _channel_row(waveform, channel, min_duration, sample_frequency, name):
    """row ``max(channel, 0)`` of ``(channels, time)``; empty when the waveform is shorter than ``min_duration`` seconds"""
    if waveform.dim() != 2:
        raise ValueError('kaldi.%s: expected a waveform of shape (channels, time), got %s' % (name, tuple(waveform.shape)))
    row = waveform[max(int(channel), 0)]
    if row.shape[-1] < min_duration * sample_frequency:
        row = row[:0]
    return row


def fbank(waveform, blackman_coeff=0.42, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0,
          high_freq=0.0, htk_compat=False, low_freq=20.0, min_duration=0.0, num_mel_bins=23, preemphasis_coefficient=0.97,
          raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True, sample_frequency=16000.0, snip_edges=True,
          subtract_mean=False, use_energy=False, use_log_fbank=True, use_power=True, vtln_high=-500.0, vtln_low=100.0,
          vtln_warp=1.0, window_type='povey'):
    """``(channels, time)`` → ``(frames, num_mel_bins [+ 1])`` of channel ``max(channel, 0)``: see ``functional.kaldi_fbank``.
    A waveform shorter than ``min_duration`` seconds gives an empty ``(0, num_mel_bins [+ 1])`` result, as one shorter than a
    frame does."""
    row = _channel_row(waveform, channel, min_duration, sample_frequency, 'fbank')
    return F.kaldi_fbank(row, blackman_coeff=blackman_coeff, dither=dither, energy_floor=energy_floor, frame_length=frame_length,
                         frame_shift=frame_shift, high_freq=high_freq, htk_compat=htk_compat, low_freq=low_freq,
                         num_mel_bins=num_mel_bins, preemphasis_coefficient=preemphasis_coefficient, raw_energy=raw_energy,
                         remove_dc_offset=remove_dc_offset, round_to_power_of_two=round_to_power_of_two,
                         sample_frequency=sample_frequency, snip_edges=snip_edges, subtract_mean=subtract_mean,
                         use_energy=use_energy, use_log_fbank=use_log_fbank, use_power=use_power, vtln_high=vtln_high,
                         vtln_low=vtln_low, vtln_warp=vtln_warp, window_type=window_type)


def mfcc(waveform, blackman_coeff=0.42, cepstral_lifter=22.0, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0,
         frame_shift=10.0, high_freq=0.0, htk_compat=False, low_freq=20.0, num_ceps=13, min_duration=0.0, num_mel_bins=23,
         preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True,
         sample_frequency=16000.0, snip_edges=True, subtract_mean=False, use_energy=False, vtln_high=-500.0, vtln_low=100.0,
         vtln_warp=1.0, window_type='povey'):
    """``(channels, time)`` → ``(frames, num_ceps)`` of channel ``max(channel, 0)``: see ``functional.kaldi_mfcc``.  A waveform
    shorter than ``min_duration`` seconds gives an empty ``(0, num_ceps)`` result, as one shorter than a frame does."""
    row = _channel_row(waveform, channel, min_duration, sample_frequency, 'mfcc')
    return F.kaldi_mfcc(row, blackman_coeff=blackman_coeff, cepstral_lifter=cepstral_lifter, dither=dither,
                        energy_floor=energy_floor, frame_length=frame_length, frame_shift=frame_shift, high_freq=high_freq,
                        htk_compat=htk_compat, low_freq=low_freq, num_ceps=num_ceps, num_mel_bins=num_mel_bins,
                        preemphasis_coefficient=preemphasis_coefficient, raw_energy=raw_energy, remove_dc_offset=remove_dc_offset,
                        round_to_power_of_two=round_to_power_of_two, sample_frequency=sample_frequency, snip_edges=snip_edges,
                        subtract_mean=subtract_mean, use_energy=use_energy, vtln_high=vtln_high, vtln_low=vtln_low,
                        vtln_warp=vtln_warp, window_type=window_type)


def spectrogram(waveform, blackman_coeff=0.42, channel=-1, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0,
                min_duration=0.0, preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True,
                sample_frequency=16000.0, snip_edges=True, subtract_mean=False, window_type='povey'):
    """``(channels, time)`` → ``(frames, N / 2 + 1)`` of channel ``max(channel, 0)``: see ``functional.kaldi_spectrogram``.  A
    waveform shorter than ``min_duration`` seconds gives an empty ``(0, N / 2 + 1)`` result, as one shorter than a frame does."""
    row = _channel_row(waveform, channel, min_duration, sample_frequency, 'spectrogram')
    return F.kaldi_spectrogram(row, blackman_coeff=blackman_coeff, dither=dither, energy_floor=energy_floor,
                               frame_length=frame_length, frame_shift=frame_shift,
                               preemphasis_coefficient=preemphasis_coefficient, raw_energy=raw_energy,
                               remove_dc_offset=remove_dc_offset, round_to_power_of_two=round_to_power_of_two,
                               sample_frequency=sample_frequency, snip_edges=snip_edges, subtract_mean=subtract_mean,
                               window_type=window_type)
