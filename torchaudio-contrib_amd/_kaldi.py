"""The definition behind ``functional.kaldi_fbank`` (torchaudio's ``compliance.kaldi.fbank``): sizes, frame counts, windows and
the mel bank, in float64 on the host.  Shared by the torch-operator route (``_composite.kaldi_fbank``), which casts them to the
waveform's dtype, and by the gfx950 route (``_hip.kaldi_fbank``), which rounds them to float32 once and packs the bank's runs.

    W = int(sample_frequency * frame_length / 1000),  S = int(sample_frequency * frame_shift / 1000),
    N = the next power of two >= W (``round_to_power_of_two``) or W

The bank is triangular IN MEL (``mel(f) = 1127 ln(1 + f / 700)``), over the FFT bins ``k < N / 2``; the Nyquist bin has no weight.

``functional.kaldi_mfcc`` (``compliance.kaldi.mfcc``) and ``functional.kaldi_spectrogram`` (``compliance.kaldi.spectrogram``) share
every step up to the power spectrum.  The spectrogram is ``log max(|rfft|^2, eps)`` over all ``N / 2 + 1`` bins with the log energy
in place of the DC bin.  The cepstrum is ``C = L D`` of the log-mel row ``L`` (``M = num_mel_bins``, ``Q = cepstral_lifter``):

    D[b][0] = sqrt(1 / M),  D[b][c] = sqrt(2 / M) cos(pi (b + 1/2) c / M);   lift[c] = 1 + Q / 2 sin(pi c / Q)  (1 where Q = 0)

then ``C[0] = e`` with ``use_energy``; with ``htk_compat`` column 0 moves to the end, times sqrt 2 unless it is the energy.
"""
import collections
import math

import torch

EPS = 2.0 ** -23            # float32 machine epsilon: the floor under every logarithm
WINDOWS = ('hamming', 'hanning', 'povey', 'rectangular', 'blackman')

#: the op's arguments behind the waveform, in schema order
Params = collections.namedtuple('Params', [
    'blackman_coeff', 'dither', 'energy_floor', 'frame_length', 'frame_shift', 'high_freq', 'htk_compat', 'low_freq',
    'num_mel_bins', 'preemphasis_coefficient', 'raw_energy', 'remove_dc_offset', 'round_to_power_of_two', 'sample_frequency',
    'snip_edges', 'subtract_mean', 'use_energy', 'use_log_fbank', 'use_power', 'window_type'])

SCHEMA_ARGS = ('float blackman_coeff, float dither, float energy_floor, float frame_length, float frame_shift, float high_freq, '
               'bool htk_compat, float low_freq, int num_mel_bins, float preemphasis_coefficient, bool raw_energy, '
               'bool remove_dc_offset, bool round_to_power_of_two, float sample_frequency, bool snip_edges, bool subtract_mean, '
               'bool use_energy, bool use_log_fbank, bool use_power, str window_type')


#: ``kaldi_mfcc``: the op's arguments behind the waveform (``use_log_fbank`` and ``use_power`` are the definition, not options)
MfccParams = collections.namedtuple('MfccParams', [
    'blackman_coeff', 'cepstral_lifter', 'dither', 'energy_floor', 'frame_length', 'frame_shift', 'high_freq', 'htk_compat',
    'low_freq', 'num_ceps', 'num_mel_bins', 'preemphasis_coefficient', 'raw_energy', 'remove_dc_offset', 'round_to_power_of_two',
    'sample_frequency', 'snip_edges', 'subtract_mean', 'use_energy', 'window_type'])

MFCC_SCHEMA_ARGS = ('float blackman_coeff, float cepstral_lifter, float dither, float energy_floor, float frame_length, '
                    'float frame_shift, float high_freq, bool htk_compat, float low_freq, int num_ceps, int num_mel_bins, '
                    'float preemphasis_coefficient, bool raw_energy, bool remove_dc_offset, bool round_to_power_of_two, '
                    'float sample_frequency, bool snip_edges, bool subtract_mean, bool use_energy, str window_type')

#: ``kaldi_spectrogram``: no bank, and the energy is always column 0
SpectrogramParams = collections.namedtuple('SpectrogramParams', [
    'blackman_coeff', 'dither', 'energy_floor', 'frame_length', 'frame_shift', 'preemphasis_coefficient', 'raw_energy',
    'remove_dc_offset', 'round_to_power_of_two', 'sample_frequency', 'snip_edges', 'subtract_mean', 'window_type'])

SPECTROGRAM_SCHEMA_ARGS = ('float blackman_coeff, float dither, float energy_floor, float frame_length, float frame_shift, '
                           'float preemphasis_coefficient, bool raw_energy, bool remove_dc_offset, bool round_to_power_of_two, '
                           'float sample_frequency, bool snip_edges, bool subtract_mean, str window_type')


def sizes(sample_frequency, frame_length, frame_shift, round_to_power_of_two):
    """(W, S, N)"""
    w = int(sample_frequency * frame_length * 0.001)
    s = int(sample_frequency * frame_shift * 0.001)
    n = w
    if round_to_power_of_two and w >= 1:
        n = 1 << (w - 1).bit_length()
    return w, s, n


def num_frames(length, w, s, snip_edges):
    if snip_edges:
        return 0 if length < w else 1 + (length - w) // s
    return (length + s // 2) // s


def resolved_high(high_freq, sample_frequency):
    return high_freq + 0.5 * sample_frequency if high_freq <= 0.0 else high_freq


def check(p, name='kaldi_fbank'):
    """``ValueError`` for arguments outside the definition; returns (W, S, N).  ``p``: any of the three parameter tuples (the
    bank's and the cepstrum's arguments are checked where ``p`` has them)."""
    w, s, n = sizes(p.sample_frequency, p.frame_length, p.frame_shift, p.round_to_power_of_two)
    bins = getattr(p, 'num_mel_bins', None)
    if bins is not None and bins <= 3:
        raise ValueError('%s: num_mel_bins must be greater than 3, got %r' % (name, bins))
    if p.window_type not in WINDOWS:
        raise ValueError('%s: invalid window type %r (one of %s)' % (name, p.window_type, ', '.join(WINDOWS)))
    if w < 2:
        raise ValueError('%s: a window of %d samples (frame_length %r ms at %r Hz): choose at least 2' %
                         (name, w, p.frame_length, p.sample_frequency))
    if s < 1:
        raise ValueError('%s: a shift of %d samples (frame_shift %r ms at %r Hz): choose at least 1' %
                         (name, s, p.frame_shift, p.sample_frequency))
    if bins is not None:
        nyquist = 0.5 * p.sample_frequency
        high = resolved_high(p.high_freq, p.sample_frequency)
        if not (0.0 <= p.low_freq < high <= nyquist):
            raise ValueError('%s: bad frequency range: low_freq %r, high_freq %r (resolved %r) at a Nyquist of %r' %
                             (name, p.low_freq, p.high_freq, high, nyquist))
    ceps = getattr(p, 'num_ceps', None)
    if ceps is not None:
        if ceps < 1:
            raise ValueError('%s: num_ceps must be at least 1, got %r' % (name, ceps))
        if ceps > bins:
            raise ValueError('%s: num_ceps cannot be larger than num_mel_bins: %r vs %r' % (name, ceps, bins))
    return w, s, n


def fbank_params(p):
    """the ``Params`` of the log-mel rows under a ``kaldi_mfcc`` call: logarithm of the power bank, no energy column, no mean"""
    return Params(p.blackman_coeff, p.dither, p.energy_floor, p.frame_length, p.frame_shift, p.high_freq, False, p.low_freq,
                  p.num_mel_bins, p.preemphasis_coefficient, p.raw_energy, p.remove_dc_offset, p.round_to_power_of_two,
                  p.sample_frequency, p.snip_edges, False, False, True, True, p.window_type)


def dct64(num_mel_bins, num_ceps):
    """float64 ``(num_mel_bins, num_ceps)``: the orthonormal DCT-II, ``D[b][0] = sqrt(1 / M)``, ``D[b][c] = sqrt(2 / M)
    cos(pi (b + 1/2) c / M)``"""
    b = torch.arange(num_mel_bins, dtype=torch.float64)[:, None]
    c = torch.arange(num_ceps, dtype=torch.float64)[None, :]
    d = math.sqrt(2.0 / num_mel_bins) * torch.cos(math.pi / num_mel_bins * (b + 0.5) * c)
    d[:, 0] = math.sqrt(1.0 / num_mel_bins)
    return d


def lifter64(num_ceps, cepstral_lifter):
    """float64 ``(num_ceps,)``: ``1 + Q / 2 sin(pi c / Q)``; ones where ``Q = 0``"""
    if cepstral_lifter == 0.0:
        return torch.ones(num_ceps, dtype=torch.float64)
    c = torch.arange(num_ceps, dtype=torch.float64)
    return 1.0 + 0.5 * cepstral_lifter * torch.sin(math.pi * c / cepstral_lifter)


def mfcc_table64(p):
    """float64 ``(num_mel_bins, num_ceps)``: ``D[b][c] lift[c]``, column 0 times sqrt 2 for ``htk_compat`` without
    ``use_energy`` — what both routes multiply the log-mel rows by (rounded to their dtype once); the columns are in the
    definition's order, the HTK rotation is the routes' own"""
    table = dct64(p.num_mel_bins, p.num_ceps) * lifter64(p.num_ceps, p.cepstral_lifter)[None, :]
    if p.htk_compat and not p.use_energy:
        table[:, 0] *= math.sqrt(2.0)
    return table


def window64(window_type, w, blackman_coeff=0.42):
    """the symmetric (``periodic=False``) window of ``w`` samples, float64"""
    i = torch.arange(w, dtype=torch.float64)
    phase = 2.0 * math.pi * i / (w - 1)
    if window_type == 'hanning':
        return 0.5 - 0.5 * torch.cos(phase)
    if window_type == 'hamming':
        return 0.54 - 0.46 * torch.cos(phase)
    if window_type == 'povey':
        return (0.5 - 0.5 * torch.cos(phase)).pow(0.85)
    if window_type == 'rectangular':
        return torch.ones(w, dtype=torch.float64)
    if window_type == 'blackman':
        return blackman_coeff - 0.5 * torch.cos(phase) + (0.5 - blackman_coeff) * torch.cos(2.0 * phase)
    raise ValueError('kaldi_fbank: invalid window type %r (one of %s)' % (window_type, ', '.join(WINDOWS)))


def mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def mel_bank64(num_mel_bins, n, sample_frequency, low_freq, high_freq):
    """float64 ``(num_mel_bins, n / 2 + 1)``; the last column (the Nyquist bin, or bin ``n // 2`` of an odd transform) is zero"""
    high = resolved_high(high_freq, sample_frequency)
    lo_mel, hi_mel = mel(low_freq), mel(high)
    delta = (hi_mel - lo_mel) / (num_mel_bins + 1)
    b = torch.arange(num_mel_bins, dtype=torch.float64)[:, None]
    left, centre, right = lo_mel + b * delta, lo_mel + (b + 1.0) * delta, lo_mel + (b + 2.0) * delta
    k = torch.arange(n // 2, dtype=torch.float64)
    mu = 1127.0 * torch.log(1.0 + (k * (sample_frequency / n)) / 700.0)[None, :]
    weights = torch.minimum((mu - left) / (centre - left), (right - mu) / (right - centre)).clamp(min=0.0)
    return torch.cat([weights, torch.zeros(num_mel_bins, 1, dtype=torch.float64)], 1)


def mirror_index(length, w, s, m):
    """``(m, w)`` int64: the sample every element of every frame reads with ``snip_edges=False`` — frame ``t`` starts at
    ``t s - (w // 2 - s // 2)``, position ``j < 0`` reads ``x[-j - 1]``, ``j >= length`` reads ``x[2 length - 1 - j]``"""
    start = torch.arange(m, dtype=torch.int64) * s - (w // 2 - s // 2)
    j = start[:, None] + torch.arange(w, dtype=torch.int64)[None, :]
    j = torch.where(j < 0, -j - 1, torch.where(j >= length, 2 * length - 1 - j, j))
    if m and (int(j.min()) < 0 or int(j.max()) >= length):
        raise ValueError('kaldi_fbank: a waveform of %d samples is too short to mirror for frames of %d samples' % (length, w))
    return j


def packed_runs(bank32):
    """``(weights float32 [w_total], table int32 [3, bands])``: every band's run of non-zero weights over the bins below the
    last column, back to back, and {first bin, bins, offset} per band (what ``tac_kaldi_fbank_f32`` reads)"""
    bands = bank32.shape[0]
    body = bank32[:, :-1]
    runs, table, off = [], [[], [], []], 0
    for b in range(bands):
        nz = torch.nonzero(body[b]).reshape(-1)
        lo, cnt = (int(nz[0]), int(nz[-1]) - int(nz[0]) + 1) if nz.numel() else (0, 0)
        runs.append(body[b, lo:lo + cnt])
        for col, val in zip(table, (lo, cnt, off)):
            col.append(val)
        off += cnt
    weights = torch.cat(runs) if off else torch.zeros(1, dtype=torch.float32)
    return weights.to(torch.float32).contiguous(), torch.tensor(table, dtype=torch.int32)
