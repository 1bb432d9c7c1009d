"""Shared by tests/test_coded_cpu.py and tests/test_coded_gpu.py: the case generator, the input layouts and the checks of the
coded frame loads — int16 PCM and 8-bit mu-law codes (uint8 / int64) read by the fused mel chain itself
(``tac_melspec_sparse_coded_f32``: csrc/melspec_stream3.hpp, stft_small3.hpp, stft_n400_s3.hpp) — and the float32 layouts of every
kernel family (a plain module: no tests in here).

A case is a pure function of ``(seed, case)`` (``draw``): the STFT arguments of tests/test_gpu_fuzz.py (fft_length 256 / 400 / 512 /
1024 / 2048, every hop from fft_length / 16 up — odd ones included —, short and odd windows, both centrings, the four pad modes,
``normalized``), power 2 or 1, linear or dB output, a mel bank, a sample format and a LAYOUT: a storage offset of 0 - 3 elements, rows
``length + pad`` apart (pad 0 - 3, sometimes 61), or a layout the host has to copy (transposed leading dims, a strided time axis).
The elements between the rows and in front of the first one hold a fill value that is no sample of the signal.

Signals.  int16: ``(signals.gained_with_silence * 25000).astype(int16)`` — zero is exact, so a silent frame must come out exactly
zero in the linear output.  mu-law: ``mu_law_encoding`` (the oracle's, 256 levels) of the same waveform; no code decodes to 0.0, so
there is no exact-zero condition for the codes.

Reference: the float64 oracle on the DECODED waveform — ``int16 / 32768``, or the reference's own 256-entry table (``lut256`` of
tests/golden/g5_mulaw.npz) — with the call's float32 window and bank cast to float64.

Checks (tests/frame_bounds.py; tolerances of tests/test_gpu_fuzz.py):

* linear, power 2: ``check_frames(..., FRAME_POW)``;
* dB: ``check_mel_db64(..., power=power)`` with its own keep conditions;
* linear, power 1: per element, ``|got - value| <= B``, derived as follows (u = 2^-24).  The kernel contracts its float32 |X| row
  with the float32 bank in float32.  (a) Every |X|[f] of a frame is within ``FRAME`` of the frame's largest magnitude (the project's
  per-frame bound for |X|); the bank carries that to ``mel_linear_bound(|X|64, fb, FRAME)[m] = FRAME max_f |X| sum_f fb[f, m]`` — the
  mask ``check_mel_db64`` already uses for power 1.  (b) The contraction of a band of K non-zero weights is K products and K - 1
  additions of non-negative terms: in any order (and with or without fused multiply-adds) every term passes through at most K
  roundings, so the float32 sum is within ``((1 + u)^K - 1) S <= (K + 2) u S`` of the exact sum S of the float32 terms for K u < 0.1,
  and S <= value + (a).  Together

      B[m] = mel_linear_bound(|X|64, fb, FRAME)[m] + (K[m] + 2) u (value[m] + mel_linear_bound(...)[m]).

  A silent frame has B = 0: it must come out exactly zero.

The route.  Every drawn case is inside what the coded entry covers, so a call is exactly one launch of it.  What it declines (then
the samples are converted first and the float32 kernels run) is never drawn:

* power 1 at fft_length 256 / 400 / 512 / 1024 — their coded kernels are instantiated for |X|^2 only (csrc/stft_small.hip
  ``launch_small_mel_entry``, csrc/stft_n400.hip ``launch_n400_mel``): power 1 is drawn at 2048 only;
* a bank that does not fit the kernels' tables (``bank_fits``): at 256 / 400 / 512 / 1024 a band wider than 48 bins from its first
  bin rounded down to a multiple of four (twelve four-tap steps: csrc/mel_lanes.hpp ``pack_lane_mel``; the wider tables of 1024 are
  float32-only), at 2048 more than 40 steps over the 64-band slots (256 floats per step beside twelve exchange areas in 160 KB of
  LDS: csrc/melspec_sparse.hip ``pack_lanes``).  A drawn band count that does not fit moves up the list of counts (and around) until
  one does;
* rows shorter than a frame (tests/test_gpu_parity.py covers that decline): length >= fft_length + 1.

Two more rules keep the dB check meaningful rather than the route (rules 4 and 5).  A silent span of the waveform is no silence once encoded:
code 128 decodes to 8.6e-5, a constant offset whose transform is one bin of 8.6e-5 N / 2 (0.088 at 2048).  A frame on the border of
such a span holds that bin and a little noise; at power 1 its noise bands pass the dB clamp (|X| > 3.2e-4) while FRAME of the
offset's bin is more than 1e-3 dB of them, and ``frame_bounds.interior_frames`` — which finds span borders by their zero samples —
counts the frame as interior, so its 99 % condition fails on the reference route already.  (At power 2 a band above the clamp is
within reach of the frame's largest bin whatever the offset.)  mu-law cases of power 1 therefore draw rows that hold no span:
length < 2 (fft_length + hop).  And a frame that is all decoded silence (a silent row, the inside of a span) has one or two bands on
that bin; where such a band is above the clamp without being held by the dB rule (``silence_at_the_clamp``: a sliver of a band's
weight on bin 0 or 1), a row of few frames loses more than 1 % of its elements to it: a dB case moves on to a band count without
such a band where there is one.
"""
import math
import os
import types

import numpy as np
import torch

import frame_bounds as fbnd
from oracle import signals, torch_ref

U = 2.0 ** -24
FRAME = 2e-6        # complex rows and |X|, per frame                      (as tests/test_gpu_fuzz.py)
FRAME_DFT = 5e-6    # ... of the windowed-DFT matrix route
FRAME_POW = 2e-5    # |X|^2 and mel power, per frame
BASE = 4106         # base of the case stream: with TAC_FUZZ_SEED=0 the default 32 cases cover ``COVERAGE`` (tests/test_coded_cpu.py)

SIZES = (256, 400, 512, 1024, 2048)
FORMATS = ('int16', 'mulaw_u8', 'mulaw_i64')
PAD_MODES = ('reflect', 'constant', 'replicate', 'circular')
MEL_COUNTS = (13, 23, 40, 64, 80, 128)
SAMPLE_RATES = (8000, 16000, 22050, 44100)
DTYPES = {'int16': torch.int16, 'mulaw_u8': torch.uint8, 'mulaw_i64': torch.int64, 'float32': torch.float32}
FILL = {'int16': 12345, 'mulaw_u8': 7, 'mulaw_i64': 7, 'float32': 0.75}     # between the rows: no silence, no sample of the signal
CODED_ENTRY = 'tac_melspec_sparse_coded_f32'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

_banks = {}
_device_banks = {}
_two_sided = {}
_lut = []


def lut256():
    """the reference's decoded values of the 256 codes (float32), as float64"""
    if not _lut:
        _lut.append(np.load(os.path.join(GOLDEN, 'g5_mulaw.npz'))['lut256'].astype(np.float64))
    return _lut[0]


def bank(n, num_mels, sample_rate, htk):
    """the (n / 2 + 1, num_mels) float32 mel bank of the package (host tensor, cached)"""
    key = (n, num_mels, sample_rate, htk)
    if key not in _banks:
        import torchaudio_contrib_amd as tac
        _banks[key] = tac.create_mel_filter(n // 2 + 1, num_mels, 0.0, sample_rate / 2.0, htk).to(torch.float32).contiguous()
    return _banks[key]


def band_steps(fb):
    """per band: four-tap steps from its first non-zero bin rounded down to a multiple of four to its last (0: empty band)"""
    nz = (fb != 0).numpy()
    out = []
    for m in range(nz.shape[1]):
        idx = np.nonzero(nz[:, m])[0]
        out.append(0 if idx.size == 0 else -(-(int(idx[-1]) + 1 - (int(idx[0]) & ~3)) // 4))
    return out


def bank_fits(fb, n):
    """Whether the coded kernels of fft_length ``n`` hold this bank (the module docstring names the two rules)."""
    steps = band_steps(fb)
    m = len(steps)
    if not 8 <= m <= 128:
        return False
    if n != 2048:
        return max(steps) <= 12
    if m % 64 and steps[-1] > steps[0]:             # laid out from the widest end (pack_lanes: ``rev``)
        steps = steps[::-1]
    slots = [max(steps[s:s + 64]) for s in range(0, m, 64)]
    if len(slots) == 2 and m % 64 == 0 and slots[0] <= 4 and slots[1] <= 16:
        slots = [4, 14 if slots[1] <= 14 else 16]   # the two unrolled shapes
    else:
        slots = [max(4, (s + 3) & ~3) for s in slots]
    return sum(slots) <= 40


def silence_at_the_clamp(c, fb, amin=1e-7, db_tol=1e-3):
    """Rule 5: whether a frame of decoded mu-law silence (all code 128) has a band that is above the dB clamp and not held by the dB
    rule — ``assert_db``'s own two conditions, evaluated in float64 on that one frame."""
    if c.fmt == 'int16':
        return False
    kw = dict(win_length=c.win_length, center=False, normalized=c.normalized)
    x = np.full((1, c.n), lut256()[128])
    p = fbnd.ref64(x, c.n, c.n, torch.hann_window(c.win_length), c.power, **kw)
    fb64 = fb.double()
    lin = fbnd.mel_linear_bound(fbnd.frames_of(p, 'spec'), fb64, fbnd.POW_TOL if c.power == 2.0 else FRAME)
    v = fbnd.frames_of(torch_ref.apply_filterbank(p, fb64), 'spec')
    safe = ((v - lin).clamp(min=0) ** 2 > amin) & (fbnd.DB_PER_REL * lin / v.clamp(min=math.sqrt(amin)) <= db_tol)
    return bool(((v * v > amin) & ~safe).any())


def draw(seed, case):
    """Case ``case`` of stream ``seed``: a namespace of the arguments, the format and the layout.  Pure."""
    rng = np.random.default_rng((BASE + seed, case))
    c = types.SimpleNamespace(seed=seed, case=case, sig=8800 + case + 7919 * seed)
    n = c.n = int(rng.choice(SIZES))
    c.hop = int(rng.integers(max(1, n // 16), n + 1)) if rng.random() < 0.5 else int(rng.choice([n // 4, n // 2, n // 8]))
    c.win_length = n if rng.random() < 0.6 else int(rng.integers(n // 4, n + 1))
    c.center = bool(rng.random() < 0.75)
    c.pad_mode = str(rng.choice(PAD_MODES))
    c.normalized = bool(rng.random() < 0.3)
    power = float(rng.choice([2.0, 2.0, 1.0]))
    c.power = power if n == 2048 else 2.0                                   # (rule 1 of the docstring)
    c.db = bool(rng.random() < 0.5)
    c.lead = tuple(int(v) for v in rng.integers(1, 6, size=int(rng.integers(1, 3))))
    c.length = int(rng.integers(n + 1, 12 * n + 1))
    c.fmt = str(rng.choice(FORMATS))
    if c.fmt != 'int16' and c.power == 1.0:                                 # (rule 4: rows without silent spans)
        c.length = int(rng.integers(n + 1, min(12 * n, 2 * (n + c.hop) - 1) + 1))
    c.sample_rate = int(rng.choice(SAMPLE_RATES))
    c.htk = bool(rng.random() < 0.5)
    first = int(rng.integers(0, len(MEL_COUNTS)))
    fitting = []
    for count in MEL_COUNTS[first:] + MEL_COUNTS[:first]:                   # (rules 2 and 5)
        mels = min(count, n // 4)
        if mels not in fitting and bank_fits(bank(n, mels, c.sample_rate, c.htk), n):
            fitting.append(mels)
    assert fitting, 'no band count fits the coded kernels: %r' % c
    held = [m for m in fitting if not (c.db and silence_at_the_clamp(c, bank(n, m, c.sample_rate, c.htk)))]
    c.num_mels = (held or fitting)[0]
    c.offset = int(rng.integers(0, 4))
    c.row_pad = 61 if rng.random() < 0.1 else int(rng.integers(0, 4))
    c.copy = None
    if rng.random() < 0.15:
        c.copy = 'transposed' if (len(c.lead) == 2 and min(c.lead) > 1 and rng.random() < 0.5) else 'strided'
    return c


def fixed(n, fmt, **kw):
    """A case by hand (the edge lists): defaults are hop = n / 4, the full window, centred, reflect, power 2, three rows, a bank of
    16 kHz that fits the size, a dense aligned layout."""
    mels = {256: 23, 400: 40, 512: 40, 1024: 80, 2048: 80}.get(n, min(40, n // 4))
    c = types.SimpleNamespace(seed=-1, case=-1, sig=8700, n=n, hop=n // 4, win_length=n, center=True, pad_mode='reflect', normalized=False,
                              power=2.0, db=False, lead=(3,), length=3 * n + n // 4 + 5, sample_rate=16000, htk=False,
                              num_mels=mels, fmt=fmt, offset=0, row_pad=0, copy=None, onesided=True)
    c.__dict__.update(kw)
    return c


def tag(c):
    d = dict(c.__dict__)
    return tuple(d[k] for k in ('case', 'fmt', 'n', 'hop', 'win_length', 'center', 'pad_mode', 'normalized', 'power', 'db', 'lead',
                                'length', 'num_mels', 'sample_rate', 'htk', 'offset', 'row_pad', 'copy'))


def stft_kw(c):
    kw = dict(win_length=c.win_length, center=c.center, pad_mode=c.pad_mode, normalized=c.normalized)
    if not getattr(c, 'onesided', True):
        kw['onesided'] = False
    return kw


def waveform(c):
    """(stored samples as a dense numpy array of the format's dtype, the decoded waveform in float64, has-silence flag)"""
    shape = c.lead + (c.length,)
    x = signals.gained_with_silence(shape, c.sig, c.n, c.hop)
    if c.fmt == 'float32':
        return x, x.astype(np.float64), signals.has_silence(shape, c.n, c.hop)
    if c.fmt == 'int16':
        pcm = (x * 25000).astype(np.int16)
        return pcm, pcm.astype(np.float64) / 32768.0, signals.has_silence(shape, c.n, c.hop)
    codes = torch_ref.mu_law_encoding(torch.from_numpy(x), 256).numpy()
    assert codes.min() >= 0 and codes.max() <= 255
    stored = codes.astype(np.uint8) if c.fmt == 'mulaw_u8' else codes.astype(np.int64)
    return stored, lut256()[codes], False


def laid_out(dense, fmt, offset, row_pad, copy, device):
    """``dense`` (numpy, (*, L)) as a tensor on ``device`` in the layout: element (r, j) at ``offset + r (L + row_pad) + j`` of one
    buffer (FILL everywhere else), or a view the host has to copy ('transposed': the two leading dims swapped in storage;
    'strided': every second element of rows 2 L long)."""
    t = torch.from_numpy(np.ascontiguousarray(dense))
    lead, length = tuple(t.shape[:-1]), int(t.shape[-1])
    if copy == 'transposed':
        return t.transpose(0, 1).contiguous().to(device).transpose(0, 1)
    if copy == 'strided':
        buf = torch.full(lead + (2 * length,), FILL[fmt], dtype=t.dtype)
        buf[..., ::2] = t
        return buf.to(device)[..., ::2]
    rows = int(np.prod(lead))
    flat = torch.full((offset + rows * (length + row_pad),), FILL[fmt], dtype=t.dtype)
    flat[offset:].view(lead + (length + row_pad,))[..., :length] = t
    return flat.to(device)[offset:].view(lead + (length + row_pad,))[..., :length]


def call(c, view, window, fb):
    """the op on the stored samples: power, dB and ``normalized`` as the case says (ref 1, amin 1e-7)"""
    args = (c.n, c.hop, c.win_length, c.center, c.pad_mode, c.normalized, getattr(c, 'onesided', True), c.power, c.db, 1.0, 1e-7)
    if c.fmt in ('int16', 'float32'):
        return torch.ops.tac_amd.melspectrogram(view, window, fb, *args)
    return torch.ops.tac_amd.melspectrogram_mulaw(view, window, fb, 256, *args)


def n_frames(c):
    return 1 + (c.length + (2 * (c.n // 2) if c.center else 0) - c.n) // c.hop


def check_power1(got, x64, c, window, fb, test, case):
    """the per-element bound of the module docstring; returns the worst |got - value| / B"""
    mag = fbnd.ref64(x64, c.n, c.hop, window, 1.0, **stft_kw(c))
    fb64 = fb.detach().cpu().double()
    value = fbnd.frames_of(torch_ref.apply_filterbank(mag, fb64), 'spec')
    lin = fbnd.mel_linear_bound(fbnd.frames_of(mag, 'spec'), fb64, FRAME)
    width = (fb64 != 0).sum(0).double()
    bound = lin + (width + 2.0) * U * (value + lin)
    err = (fbnd.as_frames(got, 'spec') - value).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    bad = ~(err <= bound)
    worst = float(torch.nan_to_num(ratio, nan=math.inf).max())
    assert not bool(bad.any()), '%s %r: %d mel value(s) beyond the power-1 bound; worst |err| / bound %.3e' % (test, case, int(bad.sum()), worst)
    fbnd.report(test, case, c.n, 'mel-power1', worst, 1.0, silent=int((value.amax(-1) == 0).sum()))
    return worst


def check(got, x64, silent, c, window, fb, test):
    """shape, dtype and the rule of the case's output kind against the float64 oracle on the decoded waveform ``x64``"""
    case = tag(c)
    assert got.dtype == torch.float32 and tuple(got.shape) == c.lead + (fb.shape[1], n_frames(c)), (case, got.dtype, tuple(got.shape))
    got = got.detach().cpu()
    kw = stft_kw(c)
    if c.db:
        return fbnd.check_mel_db64(got, x64, c.n, c.hop, fb, test, case, window, power=c.power, **kw)
    if c.power == 1.0:
        return check_power1(got, x64, c, window, fb, test, case)
    mel64 = fbnd.ref64(x64, c.n, c.hop, window, 2.0, fb, **kw)
    return fbnd.check_frames(got, mel64, 'spec', FRAME_POW, test, case, c.n, silent)


def run(c, device, test, launches=None, route=None):
    """One case end to end on ``device``.  ``launches``: the package's launch counters; ``route(ran)`` is then called with the
    entries the call launched ({entry: count}) before the values are checked.  Returns what the check returns."""
    stored, x64, silent = waveform(c)
    fb = bank(c.n, c.num_mels, c.sample_rate, c.htk) if getattr(c, 'onesided', True) else two_sided_bank(c)
    window = torch.hann_window(c.win_length)
    view = laid_out(stored, c.fmt, c.offset, c.row_pad, c.copy, device)
    assert view.dtype == DTYPES[c.fmt] and tuple(view.shape) == c.lead + (c.length,)
    wd, fd = window.to(device), on_device(fb, device)
    before = None if launches is None else dict(launches)
    got = call(c, view, wd, fd)
    if launches is not None and route is not None:
        route({k: v - before.get(k, 0) for k, v in launches.items() if v != before.get(k, 0)})
    return check(got, x64, silent, c, window, fb, test)


def on_device(fb, device):
    """``fb`` on ``device``, one copy per bank (the packed tables of the fused kernels are cached on the tensor object)"""
    key = (id(fb), str(device))
    if key not in _device_banks:
        _device_banks[key] = (fb, fb.to(device))
    return _device_banks[key][1]


def two_sided_bank(c):
    """a bank over all ``n`` bins of a two-sided transform: the mel triangles on the lower half, mirrored onto the upper"""
    key = (c.n, c.num_mels, c.sample_rate, c.htk)
    if key not in _two_sided:
        half = bank(*key)
        _two_sided[key] = torch.cat([half, half[1:-1].flip(0)], 0).contiguous()
    return _two_sided[key]


COVERAGE = ('fmt int16', 'fmt mulaw_u8', 'fmt mulaw_i64', 'odd hop', 'odd row stride int16', 'odd offset int16', 'odd offset mulaw_u8',
            'pad reflect', 'pad constant', 'pad replicate', 'pad circular', 'center False', 'power 1', 'linear', 'copy')


def covers(c):
    """the entries of ``COVERAGE`` this case provides"""
    out = {'fmt ' + c.fmt}
    if c.center:                                    # (the pad mode of an uncentred call is never read)
        out.add('pad ' + c.pad_mode)
    dense = c.copy is None
    rows = int(np.prod(c.lead))
    if c.hop % 2:
        out.add('odd hop')
    if dense and c.fmt == 'int16' and rows > 1 and (c.length + c.row_pad) % 2 and c.hop % 2 == 0 and c.offset % 2 == 0:
        out.add('odd row stride int16')         # (hop, padding and pointer on the pair: the stride term alone decides the host rule)
    if dense and c.offset % 2 and c.fmt in ('int16', 'mulaw_u8'):
        out.add('odd offset ' + c.fmt)
    if not c.center:
        out.add('center False')
    if c.power == 1.0:
        out.add('power 1')
    if not c.db:
        out.add('linear')
    if c.copy:
        out.add('copy')
    return out


# ------------------------------------------------------------------ the smallest shapes at which the loaders can go wrong
def _odd_below_half(n):
    w = n // 2 - 1
    return w if w % 2 else w - 1


#: kind -> overrides of ``fixed`` as a function of fft_length (every kind runs at the five sizes, the three formats, linear and dB)
EDGES = {
    'one-frame-at-the-clamp': lambda n: dict(center=False, length=n),                     # cs + N <= length with cs = 0 = length - N
    'length-n+1-centred': lambda n: dict(length=n + 1),
    'two-frames': lambda n: dict(center=False, length=n + n // 4),
    'one-row': lambda n: dict(lead=(1,)),
    'rows-5x3': lambda n: dict(lead=(5, 3), length=2 * n + n // 4 + 3),
    'odd-hop': lambda n: dict(hop=n // 4 - 1, length=4 * n + 5),
    'odd-row-padding': lambda n: dict(row_pad=1, length=3 * n + n // 4 + 6),              # int16: row 0 on its pair, row 1 off it
    'odd-offset': lambda n: dict(offset=1),                                               # uint8 / int16: the pointer off its pair
    'odd-short-window': lambda n: dict(win_length=_odd_below_half(n)),
    'pad-constant': lambda n: dict(pad_mode='constant'),
    'pad-replicate': lambda n: dict(pad_mode='replicate'),
    'pad-circular': lambda n: dict(pad_mode='circular'),
    'power-1': lambda n: dict(power=1.0, length=2 * n),                                   # (no silent spans: rule 4)
    'normalized': lambda n: dict(normalized=True),
}


def edge_cases(kind):
    for n in SIZES:
        for fmt in FORMATS:
            for db in (False, True):
                yield fixed(n, fmt, db=db, case=kind, sig=8700 + sorted(EDGES).index(kind), **EDGES[kind](n))


def coded_entry_covers(c):
    """whether a (fixed) case is one the coded entry takes: the rules of the module docstring"""
    return (c.n in SIZES and getattr(c, 'onesided', True) and (c.power == 2.0 or c.n == 2048) and c.length >= c.n and
            bank_fits(bank(c.n, c.num_mels, c.sample_rate, c.htk), c.n))
