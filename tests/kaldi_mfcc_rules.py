"""Shared by tests/test_kaldi_mfcc_cpu.py and tests/test_kaldi_mfcc_gpu.py: the float64 references of ``kaldi_mfcc`` and
``kaldi_spectrogram`` and the rules their float32 results are held to.  Everything up to the power spectrum — framing, mean
removal, energy, pre-emphasis, window, the per-bin error bound of a float32 evaluation — is tests/kaldi_rules.py (imported, not
repeated): ``kaldi_rules.reference`` gives, per frame, the mel values ``value`` before the logarithm with their linear bound
``bound``, and the energy with its bound.

Spectrogram.  ``out[t][k] = log max(|rfft_N(frame_t)[k]|^2, eps)`` for ``k = 1 .. N/2`` (the Nyquist bin included), ``out[t][0]`` the
log energy floored at ``log energy_floor``.  This is the fbank definition with an IDENTITY bank over all ``N/2 + 1`` bins and
``use_energy``: ``value = P[k]``, ``bound = FRAME_POW max_k P + (2 |X[k]| D[k] + D[k]^2)``, so ``kaldi_rules.reference`` is run with
such a bank (placed in its bank cache under a key no real bank has) and ``kaldi_rules._log_check`` holds the bins 1 .. N/2;
column 0 is under the existing energy rule.  ``KEEP`` = 99 % of the bins above the floor must be held; additionally the Nyquist
column must be held in at least half of the frames (``NYQUIST_KEEP``), so that it cannot sit wholly inside the 1 %.

MFCC.  With ``M`` bins, ``Q = cepstral_lifter``, ``L[b] = log max(value[b], eps)``:

    D[b][0] = sqrt(1/M),  D[b][c] = sqrt(2/M) cos(pi (b + 1/2) c / M);   C[c] = sum_b L[b] D[b][c];   C[c] *= 1 + Q/2 sin(pi c / Q)
    use_energy: C[0] = e;   htk_compat: [C1 .. C_{n-1}, C0], that C0 times sqrt 2 unless it is the energy

A band is *held* as in ``_log_check`` (``value - B > eps``) with the allowance ``a[b] = B / value + 4 u |log value|``, or *deep*
(``value + B < eps``) with ``a[b] = 0`` and ``L[b] = log eps``.  A frame is checked when every band is held or deep; then

    |got[c] - C[c]| <= |lift[c]| (sum_b |D[b][c]| a[b] + (M + 2) u sum_b |D[b][c] L[b]|) + 2 u |C[c]|

(the float32 table entry, the M products and sums of a chain in any order: ``(M + 2) u`` on the sum of magnitudes; the last term
for the lifter folded into the table and the rounding of the result), times sqrt 2 where the definition scales.  At least
``FRAMES_KEEP`` = 90 % of the frames must be checked.  The energy column is under the existing energy rule, on every frame.
"""
import math

import numpy as np
import torch

import kaldi_rules as R

U, EPS = R.U, R.EPS
FRAMES_KEEP = 0.90
NYQUIST_KEEP = 0.5
IDENTITY = -1.0          # the ``low_freq`` under which the identity bank sits in ``kaldi_rules``' bank cache

MFCC_DEFAULTS = dict(R.DEFAULTS, cepstral_lifter=22.0, num_ceps=13)
del MFCC_DEFAULTS['use_log_fbank'], MFCC_DEFAULTS['use_power']
SPECTROGRAM_KEYS = ('blackman_coeff', 'dither', 'energy_floor', 'frame_length', 'frame_shift', 'preemphasis_coefficient',
                    'raw_energy', 'remove_dc_offset', 'round_to_power_of_two', 'sample_frequency', 'snip_edges', 'subtract_mean',
                    'window_type')
SPECTROGRAM_DEFAULTS = {k: R.DEFAULTS[k] for k in SPECTROGRAM_KEYS}

#: the MFCC options against the defaults: num_ceps 1 / 13 / M, M 4 / 23 / 40, Q 0 / 22, use_energy x htk_compat, the energy of the
#: windowed frame, mirrored ends (80 bins with 40 coefficients needs the two-row waveform: ``MFCC_TWO_ROWS``)
MFCC_OPTIONS = [dict(num_ceps=1), dict(num_ceps=23), dict(num_mel_bins=4, num_ceps=4), dict(num_mel_bins=40), dict(cepstral_lifter=0.0),
                dict(use_energy=True), dict(htk_compat=True), dict(use_energy=True, htk_compat=True),
                dict(use_energy=True, raw_energy=False), dict(snip_edges=False)]
MFCC_TWO_ROWS = dict(num_mel_bins=80, num_ceps=40)
SPECTROGRAM_OPTIONS = [dict(snip_edges=False), dict(remove_dc_offset=False), dict(preemphasis_coefficient=0.0),
                       dict(window_type='rectangular'), dict(window_type='hamming'), dict(raw_energy=False), dict(energy_floor=0.0)]


def mfcc_options(**kw):
    o = dict(MFCC_DEFAULTS)
    o.update(kw)
    return o


def spectrogram_options(**kw):
    o = dict(SPECTROGRAM_DEFAULTS)
    o.update(kw)
    return o


def waveform_kw(kw):
    """the keywords ``kaldi_rules.waveform`` looks at"""
    return {k: v for k, v in kw.items() if k in ('preemphasis_coefficient', 'remove_dc_offset')}


def dct64(bins, ceps):
    out = np.empty((bins, ceps), dtype=np.float64)
    for b in range(bins):
        out[b, 0] = math.sqrt(1.0 / bins)
        for c in range(1, ceps):
            out[b, c] = math.sqrt(2.0 / bins) * math.cos(math.pi * (b + 0.5) * c / bins)
    return out


def lifter64(ceps, q):
    return np.array([1.0 if q == 0.0 else 1.0 + 0.5 * q * math.sin(math.pi * c / q) for c in range(ceps)], dtype=np.float64)


def _fbank_options(o, **over):
    ro = R.options(**{k: v for k, v in o.items() if k in R.DEFAULTS})
    ro.update(use_log_fbank=True, use_power=True, subtract_mean=False, htk_compat=False)
    ro.update(over)
    return ro


def _floored_log_energy(r, o):
    with np.errstate(invalid='ignore'):
        e = np.log(np.maximum(r.energy, EPS))
        if o['energy_floor'] > 0.0:
            e = np.maximum(e, math.log(o['energy_floor']))
        return np.where(np.isnan(r.energy), np.nan, e)


def _energy_check(e_col, r, o, what):
    floor = max(EPS, o['energy_floor']) if o['energy_floor'] > 0.0 else EPS
    return R._log_check(e_col, r.energy, r.energy_bound, floor, np.float32(math.log(floor)), what + ' energy')[0]


class MfccReference(object):
    """``out`` (rows, m, num_ceps) float64 in the call's column order; ``unsubtracted``; ``coeffs`` / ``allow`` (rows, m, num_ceps)
    in the definition's order (C0 first); ``checked`` (rows, m): the frames whose bands are all held or deep; ``fbank``: the
    ``kaldi_rules.Reference`` underneath."""


def mfcc_reference(x, o):
    bins, ceps, q = o['num_mel_bins'], o['num_ceps'], o['cepstral_lifter']
    r = R.reference(x, _fbank_options(o, use_energy=False))
    rows, m = r.value.shape[:2]
    d, lift = dct64(bins, ceps), lifter64(ceps, q)
    scale = np.ones(ceps)
    if o['htk_compat'] and not o['use_energy']:
        scale[0] = math.sqrt(2.0)
    energy = _floored_log_energy(r, o)
    ref = MfccReference()
    ref.fbank = r
    ref.coeffs = np.zeros((rows, m, ceps))
    ref.allow = np.zeros((rows, m, ceps))
    ref.checked = np.zeros((rows, m), dtype=bool)
    for row in range(rows):
        for t in range(m):
            value, bound = r.value[row, t], r.bound[row, t]
            with np.errstate(invalid='ignore'):
                held, deep = (value - bound) > EPS, (value + bound) < EPS
                safe = np.where(held, value, 1.0)
                a = np.where(held, bound / safe + 4.0 * U * np.abs(np.log(safe)), 0.0)
                logs = np.where(np.isnan(value), np.nan, np.log(np.maximum(value, EPS)))
            ref.checked[row, t] = bool((held | deep).all())
            for c in range(ceps):
                acc, mag, slack = 0.0, 0.0, 0.0
                for b in range(bins):
                    acc += logs[b] * d[b, c]
                    mag += abs(logs[b] * d[b, c])
                    slack += abs(d[b, c]) * a[b]
                ref.coeffs[row, t, c] = acc * lift[c] * scale[c]
                ref.allow[row, t, c] = abs(lift[c]) * scale[c] * (slack + (bins + 2) * U * mag) + 2.0 * U * abs(ref.coeffs[row, t, c])
            if o['use_energy']:
                ref.coeffs[row, t, 0] = energy[row, t]
    out = ref.coeffs
    if o['htk_compat']:
        out = np.concatenate([out[..., 1:], out[..., :1]], -1)
    ref.unsubtracted = out
    ref.out = out - out.mean(1, keepdims=True) if (o['subtract_mean'] and m) else out
    return ref


def check_mfcc(got, ref, o, what=''):
    """``got``: the float32 result (…, m, num_ceps) WITHOUT ``subtract_mean`` for the waveform ``ref`` was made from.  Returns the
    worst ratios of error to allowance and the share of checked frames."""
    g = np.asarray(got, dtype=np.float64).reshape(ref.coeffs.shape)
    assert np.isfinite(g).all(), '%s: non-finite output' % what
    if o['htk_compat']:
        g = np.concatenate([g[..., -1:], g[..., :-1]], -1)
    res = {}
    first = 0
    if o['use_energy']:
        res['energy'] = _energy_check(g[..., 0], ref.fbank, o, what)
        first = 1
    ratio = np.abs(g - ref.coeffs) / np.maximum(ref.allow, 1e-300)
    ratio = np.where(ref.checked[..., None], ratio, 0.0)[..., first:]
    res['cepstrum'] = float(ratio.max()) if ratio.size else 0.0
    res['frames'] = float(ref.checked.mean()) if ref.checked.size else 1.0
    assert res['cepstrum'] <= 1.0, '%s: a coefficient is %.3f of its allowance off at %r' % (
        what, res['cepstrum'], np.unravel_index(ratio.argmax(), ratio.shape))
    assert res['frames'] >= FRAMES_KEEP, '%s: only %d of %d frames have all bands held or deep' % (
        what, int(ref.checked.sum()), ref.checked.size)
    return res


class SpectrogramReference(object):
    """``out`` / ``unsubtracted`` (rows, m, N/2 + 1) float64; ``fbank``: the ``kaldi_rules.Reference`` under the identity bank
    (``value`` = P, ``bound`` per bin, ``energy`` / ``energy_bound``)."""


def spectrogram_reference(x, o):
    w, s, n = R.sizes(R.options(**o))
    bins = n // 2 + 1
    ro = _fbank_options(o, use_energy=True, num_mel_bins=bins, low_freq=IDENTITY, high_freq=0.0)
    R._bank_cache[(bins, n, ro['sample_frequency'], IDENTITY, 0.0)] = np.eye(bins)
    r = R.reference(x, ro)
    m = r.value.shape[1]
    ref = SpectrogramReference()
    ref.fbank = r
    # r.unsubtracted = [e, log P[0], log P[1], .. log P[N/2]]: the energy takes the DC bin's place
    ref.unsubtracted = np.concatenate([r.unsubtracted[..., :1], r.unsubtracted[..., 2:]], -1)
    ref.out = ref.unsubtracted - ref.unsubtracted.mean(1, keepdims=True) if (o['subtract_mean'] and m) else ref.unsubtracted
    return ref


def nyquist_share(ref):
    """share of the frames whose Nyquist bin is held by the log rule"""
    r = ref.fbank
    held = (r.value[..., -1] - r.bound[..., -1]) > EPS
    return float(held.mean()) if held.size else 1.0


def check_spectrogram(got, ref, o, what=''):
    r = ref.fbank
    g = np.asarray(got, dtype=np.float64).reshape(ref.unsubtracted.shape)
    res = {}
    res['log'], res['kept'] = R._log_check(g[..., 1:], r.value[..., 1:], r.bound[..., 1:], EPS, R.LOG_EPS32, what + ' bins')
    res['energy'] = _energy_check(g[..., 0], r, o, what)
    res['nyquist'] = nyquist_share(ref)
    assert res['nyquist'] >= NYQUIST_KEEP, '%s: the Nyquist bin is held in only %.2f of the frames' % (what, res['nyquist'])
    return res


def row_gradient(x, o, grad_out, mode):
    """float64 gradient of ``sum(out * grad_out)`` w.r.t. the waveform ``x`` (rows, n) of ``mode`` 'mfcc' / 'spectrogram',
    through torch float64 operators applied frame by frame to the definitions above"""
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    rows, length = xt.shape
    fo = R.options(**{k: v for k, v in o.items() if k in R.DEFAULTS})
    w, s, n = R.sizes(fo)
    m = R.num_frames(length, w, s, o['snip_edges'])
    win = torch.from_numpy(R.window64(o['window_type'], w, o['blackman_coeff']))
    c = o['preemphasis_coefficient']
    if mode == 'mfcc':
        bank = torch.from_numpy(R.cached_bank(fo))
        scale = math.sqrt(2.0) if (o['htk_compat'] and not o['use_energy']) else 1.0
        table = torch.from_numpy(dct64(o['num_mel_bins'], o['num_ceps']) * lifter64(o['num_ceps'], o['cepstral_lifter'])[None, :])
    g = torch.tensor(np.asarray(grad_out, dtype=np.float64)).reshape(rows, m, -1)
    total = xt.new_zeros(())
    for row in range(rows):
        for t in range(m):
            f = xt[row, torch.tensor(R.frame_indices(length, w, s, t, o['snip_edges']))]
            if o['remove_dc_offset']:
                f = f - f.sum() / w
            e = (f * f).sum() if o['raw_energy'] else None
            if c != 0.0:
                f = f - c * torch.cat([f[:1], f[:-1]])
            f = f * win
            if e is None:
                e = (f * f).sum()
            le = torch.log(torch.clamp(e, min=EPS))
            if o['energy_floor'] > 0.0:
                le = torch.clamp(le, min=math.log(o['energy_floor']))
            z = torch.fft.rfft(torch.cat([f, f.new_zeros(n - w)]))
            power = z.real ** 2 + z.imag ** 2
            if mode == 'mfcc':
                coeffs = torch.log(torch.clamp(bank @ power, min=EPS)) @ table
                first = le[None] if o['use_energy'] else coeffs[:1] * scale
                cols = [coeffs[1:], first] if o['htk_compat'] else [first, coeffs[1:]]
            else:
                cols = [le[None], torch.log(torch.clamp(power[1:], min=EPS))]
            total = total + (torch.cat(cols) * g[row, t]).sum()
    total.backward()
    return xt.grad.numpy()
