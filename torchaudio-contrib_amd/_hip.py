"""Launchers of the gfx950 kernels: the bodies of the ``tac_amd::*`` ops for float32 tensors on a HIP device.

Every function takes fully resolved, already validated arguments (``functional.py`` fills in defaults;
``_ops.py`` routes by device / dtype) and goes through the C ABI of ``include/tac_amd.h`` via ctypes — raw
device pointers, sizes and the caller's current HIP stream.  PyTorch only provides the output allocation and
the stream.  There is no fallback in here: a missing ``libtac_amd.so`` or a failing launch raises.
"""
import ctypes
import itertools
import math
import os
import threading
import weakref

import torch

from . import _kaldi
from . import _native
from . import _resample
from . import _rir
from ._bounded import Bounded

_lock = threading.Lock()

#: number of kernels launched through the C ABI since import, per entry point (tests assert on it so that a
#: silently taken non-HIP route cannot pass as the HIP path)
launches = {}


def _count(name, *filled):
    launches[name] = launches.get(name, 0) + 1
    check_written(name, *filled)


#: ``accept`` of the launches whose caller takes another route when the entry point declines the call
_DECLINED = (_native.TAC_E_UNSUPPORTED,)


def _launch(name, dev, filled, *args, accept=()):
    """One launch of the entry point ``name`` on ``dev``'s current stream (the last argument of every entry point), checked and
    counted.  ``filled``: the tensors (or slices) it fills, checked for poison while that is on.  A return code in ``accept``
    (``TAC_E_UNSUPPORTED`` where the caller then takes another route) is handed back as it is, and nothing is counted."""
    with _native.on_device(dev):
        rc = getattr(_native.lib(), name)(*args, _native.stream_ptr(dev))
    if rc in accept:
        return rc
    _native.check(rc, name)
    _count(name, *filled)
    return _native.TAC_OK


# ----------------------------------------------------------------------------- constant-table caches
# Everything derived from a window / filterbank / coefficient tensor (packed weights, tile plans, transposes, adjoint tables,
# DFT matrices, the istft envelope, host read-backs) hangs ON the tensor object, and ``cached_on`` below is the only code that
# hangs it there.  A slot (one of ``_CACHE_ATTRS``, the list ``invalidate`` walks) holds ``(stamp, {key: table})``; the stamp
# is what identifies the tensor's contents cheaply: the version counter (every in-place torch op bumps it), the data pointer
# (``set_`` / ``.data = other``) and the invalidation epoch below.  A table that is ``None`` is a result like any other ("this
# bank is not band-sparse" costs a host synchronisation to find out, once).  A slot keeps 16 tables unless its site says
# otherwise: ``_tac_istft`` 64 small envelopes, ``_tac_dft`` / ``_tac_dftT`` ONE matrix each — at fft_length 8192 a matrix is
# 8192 x 8194 floats = 268 MB, so a window used at a second geometry gives up the first one's matrix.
# Writes that PyTorch itself does not record — ``t.data.mul_(2)`` (``.data`` has its own version counter), writes
# through an alias created before the cache, ``from_dlpack`` / raw-pointer writers — cannot be seen without reading the
# tensor back on every call; after such a write call ``invalidate(t)`` (or ``invalidate()`` for everything).
_epoch = 0
_CACHE_ATTRS = ('_tac_pack', '_tac_plan', '_tac_T', '_tac_adj', '_tac_dft', '_tac_dftT', '_tac_finite', '_tac_istft', '_tac_dct', '_tac_coef', '_tac_conv')


_unstamped = itertools.count()


def _stamp(t):
    """What identifies a tensor's contents cheaply.  Tensors created under ``torch.inference_mode`` carry no version counter
    (reading it raises): they get a stamp that never repeats, i.e. their derived tables are rebuilt on every call rather
    than risk serving a stale one after an in-place write nobody recorded."""
    if t.is_inference():
        return ('unversioned', next(_unstamped))
    return (t._version, t.data_ptr(), _epoch)


def cached_on(t, attr, key, build, limit=16):
    """``build()`` once per (contents of ``t``, ``key``), whatever it returns (a ``None`` is kept like any table): the table
    lives on the tensor object in the slot ``attr`` (one of ``_CACHE_ATTRS``), stamped as above, so an in-place write to ``t``
    rebuilds it.  The slot keeps at most ``limit`` tables — exactly, unlike ``Bounded``, which may exceed its limit by one: a
    ``limit`` of 1 has to mean one DFT matrix — and is emptied when one more arrives.  ``build`` runs outside
    inference mode: its tensors may be saved for a later call's backward.  A tensor object that cannot carry attributes has
    its tables rebuilt on every call."""
    cache = getattr(t, attr, None)
    stamp = _stamp(t)
    if cache is None or cache[0] != stamp:
        if attr not in _CACHE_ATTRS:            # (checked where a slot is written: a hit costs nothing for it)
            raise ValueError('cached_on: %r is not in _CACHE_ATTRS, invalidate() would miss it' % (attr,))
        cache = (stamp, {})
        try:
            setattr(t, attr, cache)
        except (AttributeError, RuntimeError):
            pass
    tables = cache[1]
    try:
        return tables[key]
    except KeyError:
        pass
    with torch.inference_mode(False):
        made = build()
    if len(tables) >= limit:
        tables.clear()
    tables[key] = made
    return made


def invalidate(tensor=None):
    """Forget the tables derived from ``tensor`` (a window or filterbank), or — without an argument — from every
    tensor: they are rebuilt from the current contents on the next call.  Needed only after a write PyTorch's version
    counter does not see (``t.data.mul_(2)``, raw-pointer writes); ordinary in-place ops are detected by themselves.
    Pass the tensor object the layers were given (``invalidate(module.filterbank)``): only its tables are dropped.  Passing an
    alias that carries no tables itself (``module.filterbank.data``, a view) is allowed and invalidates everything."""
    global _epoch
    from . import _lazy
    if tensor is None:
        with _lock:
            _epoch += 1
            _geometry_routes_clear()
            _lazy._plans.clear()
            ext = _native.ext()
            if ext is not None:
                ext.set_epoch(_epoch)           # (plans a caller still holds stop matching)
        return
    carried = False
    for name in _CACHE_ATTRS:
        if hasattr(tensor, name):
            carried = True
            try:
                delattr(tensor, name)
            except (AttributeError, RuntimeError):
                pass
    with _lock:
        carried = carried or any(k[0] == id(tensor) for g in _geometry_cache.values() for k in g.routes) \
            or any(id(tensor) in k[:2] for k in _lazy._plans)
    if not carried:
        # nothing is cached ON this object: it is an alias of the tensor the tables hang on (`module.filterbank.data`, a view,
        # a second wrapper of the same storage) — which object that is cannot be told from here, so everything goes
        invalidate()
        return
    # only this tensor's entries go: the tables of every other window / filterbank stay valid (a global epoch bump would
    # have each of them rebuilt, with a host synchronisation, on its next use)
    with _lock:
        for g in _geometry_cache.values():
            for key in [k for k in g.routes if k[0] == id(tensor)]:
                del g.routes[key]
        for key in [k for k in _lazy._plans if id(tensor) in k[:2]]:         # bound-argument launchers built from it
            del _lazy._plans[key]


def _geometry_routes_clear():
    for g in _geometry_cache.values():
        g.routes.clear()


# ----------------------------------------------------------------------------- STFT geometry
class StftGeometry(object):
    """Validated geometry of one stft call on one input layout (the checks ``torch.stft`` performs, reference
    functional.py:99-107), cached per (shape, strides, parameters) so that a repeated call costs a dict lookup."""
    __slots__ = ('lead', 'length', 'rows', 'row_stride', 'flatten', 'n_fft', 'hop', 'win_length', 'center',
                 'pad_mode', 'normalized', 'onesided', 'n_frames', 'n_bins', 'fft_kernel', 'pow2_kernel', 'mixed_radix', 'desc',
                 'stft_shape', 'spec_shape', 'routes')


_geometry_cache = Bounded(512)


def stft_frames(length, n_fft, hop, center):
    pad = n_fft // 2 if center else 0
    return 1 + (length + 2 * pad - n_fft) // hop


def check_stft_args(shape, n_fft, hop, win_length, center, pad_mode):
    """The argument checks of ``torch.stft`` + ``F.pad`` that do not depend on the backend (same exception types:
    the reference's tests expect ``RuntimeError`` for an input too short to reflect-pad,
    reference tests/test_functional.py:31)."""
    if len(shape) < 1 or any(int(s) == 0 for s in shape):
        raise RuntimeError('stft: expected a non-empty tensor of shape (*, channel, time)')
    length = int(shape[-1])
    if n_fft <= 0 or hop <= 0:
        raise RuntimeError('stft: expected 0 < n_fft and 0 < hop_length, got n_fft=%d hop_length=%d' % (n_fft, hop))
    if not 0 < win_length <= n_fft:
        raise RuntimeError('stft: expected 0 < win_length <= n_fft, got win_length=%d' % win_length)
    if pad_mode not in _native.PAD_MODES:
        raise NotImplementedError('stft: unsupported pad_mode %r' % (pad_mode,))
    pad = n_fft // 2 if center else 0
    if center and pad_mode == 'reflect' and pad >= length:
        raise RuntimeError('stft: reflect padding (%d, %d) must be smaller than the signal length %d'
                           % (pad, pad, length))
    if center and pad_mode == 'circular' and pad > length:
        raise RuntimeError('stft: circular padding (%d, %d) must not exceed the signal length %d'
                           % (pad, pad, length))
    if length + 2 * pad < n_fft:
        raise RuntimeError('stft: expected n_fft <= padded signal length %d, got n_fft=%d' % (length + 2 * pad, n_fft))


def fft_kernel_size(n_fft):
    """power-of-two sizes in [32, 4096] take the wave-level FFT kernels (``big_fft_size``: 8192 ... 32768 the four-step
    kernel; ``smooth_fft_size``: even lengths with a 7-smooth half the generic Stockham kernel); every other size up to 8192
    is evaluated as a windowed-DFT matrix product on the fp32 matrix cores (``_stft_dft``) — except ``mixed_radix_size``."""
    return (n_fft & (n_fft - 1)) == 0 and 32 <= n_fft <= 4096


def mixed_radix_size(n_fft):
    """fft_length 400 (25 ms at 16 kHz) has its own kernel (csrc/stft_n400.hip: 200 = 8 x 25) for the one-sided
    complex / |X| / |X|^2 (+dB) rows; its other forms take the DFT-matrix route."""
    return n_fft == 400


def big_fft_size(n_fft):
    """fft_length 8192 / 16384 / 32768: one frame per workgroup as a four-step transform over the wave-level 1024-point FFT
    (csrc/stft_big.hip, round 5) — forward stft / spectrogram rows of every form; gradients at 8192 take the generic
    Stockham adjoint of csrc/stft_smooth.hip, above that they are a composite route."""
    return n_fft in (8192, 16384, 32768)


def smooth_fft_size(n_fft):
    """even fft_length <= 8192 (not a power of two, not 400) whose half is 7-smooth — 480, 960, 1200, 1920, 882 ...: generic
    Stockham passes of radix 4 / 2 / 3 / 5 / 7 (csrc/stft_smooth.hip, round 5) for the forward stft / spectrogram rows AND their
    gradients (``stft_smooth_backward_kernel`` behind ``tac_stft_backward_f32``: the same passes on conjugated data; 8192 as well).  Mirrors ``stft_smooth_covers`` of the library."""
    if n_fft < 8 or n_fft % 2 or n_fft > 8192 or n_fft & (n_fft - 1) == 0 or n_fft == 400:
        return False
    m = n_fft // 2
    for r in (2, 3, 5, 7):
        while m % r == 0:
            m //= r
    return m == 1


def hip_covers_n_fft(n_fft):
    return fft_kernel_size(n_fft) or n_fft <= 8192 or big_fft_size(n_fft)


def hip_covers_backward(n_fft):
    return fft_kernel_size(n_fft) or n_fft <= 8192


def geometry(wave, n_fft, hop, win_length, center, pad_mode, normalized, onesided):
    key = (tuple(wave.shape), tuple(wave.stride()), n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    g = _geometry_cache.get(key)
    if g is not None:
        return g
    check_stft_args(wave.shape, n_fft, hop, win_length, center, pad_mode)
    g = StftGeometry()
    length = int(wave.shape[-1])
    g.lead = tuple(int(s) for s in wave.shape[:-1])
    g.length = length
    g.rows = 1
    for s in g.lead:
        g.rows *= s
    # can the rows be addressed as base + r * row_stride without a copy?
    flat = wave.reshape(-1, length) if wave.dim() != 2 else wave
    viewable = flat.data_ptr() == wave.data_ptr() and flat.stride(1) == 1 and \
        (flat.shape[0] == 1 or flat.stride(0) >= length)
    g.flatten = not viewable
    g.row_stride = length if (g.flatten or flat.shape[0] == 1) else int(flat.stride(0))
    g.n_fft, g.hop, g.win_length = n_fft, hop, win_length
    g.center, g.pad_mode, g.normalized, g.onesided = bool(center), pad_mode, bool(normalized), bool(onesided)
    g.n_frames = stft_frames(length, n_fft, hop, center)
    g.n_bins = n_fft // 2 + 1 if onesided else n_fft
    g.fft_kernel = fft_kernel_size(n_fft) or big_fft_size(n_fft) or smooth_fft_size(n_fft)   # tac_stft_f32 / tac_spectrogram_f32 take it
    g.pow2_kernel = fft_kernel_size(n_fft)                  # ... and the fused chains / gradient kernels of the power-of-two sizes
    if not g.fft_kernel and n_fft > 8192:
        raise NotImplementedError('stft: fft_length %d is outside the HIP path (power of two in [32, 32768], or any '
                                  'length <= 8192 through the DFT-matrix kernel)' % n_fft)
    g.mixed_radix = mixed_radix_size(n_fft)
    g.desc = None if not (g.fft_kernel or g.mixed_radix) else _native.StftDesc(
        rows=g.rows, length=length, row_stride=g.row_stride, n_fft=n_fft, hop=hop, win_length=win_length,
        center=1 if center else 0, pad_mode=_native.PAD_MODES[pad_mode], normalized=1 if normalized else 0,
        onesided=1 if onesided else 0, reserved=0)
    g.stft_shape = g.lead + (g.n_frames, g.n_bins, 2)
    g.spec_shape = g.lead + (g.n_frames, g.n_bins)
    g.routes = {}
    with _lock:
        _geometry_cache[key] = g
    return g


def _rows_of(wave, g):
    """The tensor whose data pointer + g.row_stride addresses the rows (a copy only for layouts that cannot be)."""
    return wave.reshape(-1, g.length).contiguous() if g.flatten else wave


def _dft_matrix(window, n_fft, win_length, onesided, normalized):
    """(N, 2F) float32 device matrix [w[n] cos(2 pi k n / N), -w[n] sin(2 pi k n / N)] for the DFT-matrix path,
    built on the device in float64 (angles reduced exactly through (n*k) mod N in int64) and rounded once — a
    constant table like the FFT twiddles, cached on the window tensor: the matrix of ONE geometry (up to 268 MB)."""
    def build():
        dev = window.device
        w = torch.zeros(n_fft, dtype=torch.float64, device=dev)
        off = (n_fft - win_length) // 2
        w[off:off + win_length] = window.detach().double()
        if normalized:
            w = w / math.sqrt(n_fft)
        n_bins = n_fft // 2 + 1 if onesided else n_fft
        n = torch.arange(n_fft, dtype=torch.int64, device=dev)[:, None]
        k = torch.arange(n_bins, dtype=torch.int64, device=dev)[None, :]
        ang = ((n * k) % n_fft).double() * (2.0 * math.pi / n_fft)
        mat = torch.stack([torch.cos(ang) * w[:, None], -torch.sin(ang) * w[:, None]], dim=-1)
        return mat.to(torch.float32).reshape(n_fft, 2 * n_bins).contiguous()
    return cached_on(window, '_tac_dft', (n_fft, win_length, bool(onesided), bool(normalized)), build, limit=1)


def _stft_dft(wave, window, g):
    """Any fft_length (non power of two, or 4096 < N <= 8192): the framed signal is never materialised — the
    filterbank GEMM kernel reads frame t, sample n at ``padded[row, t*hop + n]`` (stride_f = 1, stride_t = hop)
    and multiplies by the (N, 2F) windowed-DFT matrix on the fp32 matrix cores.  The padded copy is plain data
    movement done by torch; everything arithmetic is the HIP kernel."""
    x = wave.reshape(-1, g.length)
    if g.center:
        pad = g.n_fft // 2
        x = torch.nn.functional.pad(x.unsqueeze(1), (pad, pad), mode=g.pad_mode).squeeze(1)
    x = x.contiguous()
    mat = _dft_matrix(window, g.n_fft, g.win_length, g.onesided, g.normalized)
    out = _empty(g.stft_shape, device=x.device)
    _launch('tac_apply_filterbank_f32', x.device, (out,), _native.ptr(x), x.shape[0], g.n_fft, g.n_frames, x.stride(0), 1, g.hop,
            _native.ptr(mat), None, 2 * g.n_bins, _native.ptr(out))
    return out.transpose(-3, -2)


def stft(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided):
    g = geometry(wave, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    if not (g.fft_kernel or (g.mixed_radix and g.onesided)):
        return _stft_dft(wave, window, g)
    src = _rows_of(wave, g)
    out = _empty(g.stft_shape, device=wave.device)
    _launch('tac_stft_f32', wave.device, (out,), _native.ptr(src), _native.ptr(window), g.desc, _native.ptr(out))
    return out.transpose(-3, -2)


def spectrogram(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db, ref, amin):
    g = geometry(wave, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    if not (g.fft_kernel or (g.mixed_radix and g.onesided and power in (1.0, 2.0))):
        mag = complex_norm(_stft_dft(wave, window, g), power)
        return amplitude_to_db(mag, ref, amin) if db else mag
    src = _rows_of(wave, g)
    out = _empty(g.spec_shape, device=wave.device)
    _launch('tac_spectrogram_f32', wave.device, (out,), _native.ptr(src), _native.ptr(window), g.desc, float(power),
            1 if db else 0, float(ref), float(amin), _native.ptr(out))
    return out.transpose(-2, -1)


# ----------------------------------------------------------------------------- inverse STFT (csrc/istft.hip)
#: how the last calls of ``istft`` got their frame-major rows: used in place (what ``stft`` / ``phase_vocoder`` return) or copied
istft_layout = {'in_place': 0, 'copied': 0}


def istft_covers(n_fft):
    """the fft_lengths the frame kernels invert: every one ``tac_stft_backward_f32`` takes"""
    return bool(fft_kernel_size(n_fft) or mixed_radix_size(n_fft) or smooth_fft_size(n_fft) or n_fft == 8192)


def istft_full_length(n_frames, n_fft, hop, center):
    """samples the frames determine: ``hop (T - 1) + n_fft`` minus the two halves ``center`` padded"""
    return hop * (n_frames - 1) + n_fft - (2 * (n_fft // 2) if center else 0)


def _istft_desc(rows, out_len, row_stride, n_fft, hop, win_length, center, normalized):
    return _native.StftDesc(rows=rows, length=out_len, row_stride=row_stride, n_fft=n_fft, hop=hop, win_length=win_length,
                            center=1 if center else 0, pad_mode=0, normalized=1 if normalized else 0, onesided=1, reserved=0)


def istft_envelope(window, n_fft, hop, win_length, center, n_frames, kept):
    """``1 / env`` of ``hop (T - 1) + n_fft`` padded positions as a device tensor, env the overlap-add of the squared window —
    a constant of (window contents, geometry), cached on the window tensor like the other derived tables.  The first use of an
    entry for a kept range of ``kept`` samples reads min env once (a host synchronisation) and raises the ``RuntimeError``
    ``torch.istft`` raises when the window overlap-add vanishes there (NOLA); later calls synchronise nothing."""
    def build():
        inv_env = torch.empty(hop * (n_frames - 1) + n_fft, dtype=torch.float32, device=window.device)
        desc = _istft_desc(1, 1, 1, n_fft, hop, win_length, center, False)
        _launch('tac_istft_envelope_f32', window.device, (), _native.ptr(window), desc, n_frames, _native.ptr(inv_env), None)
        return inv_env, set()
    entry = cached_on(window, '_tac_istft', (n_fft, hop, win_length, bool(center), n_frames), build, limit=64)
    if kept not in entry[1]:
        pad = n_fft // 2 if center else 0
        peak = float(entry[0][pad:pad + kept].max().item())         # (one table serves both: min env = 1 / max (1 / env))
        lowest = 1.0 / peak if peak > 0.0 else float('inf')
        if not lowest >= 1e-11:
            raise RuntimeError('istft: window overlap add min: %g is below 1e-11 (fft_length=%d, hop_length=%d, center=%s): '
                               'the window does not satisfy the NOLA condition' % (lowest, n_fft, hop, bool(center)))
        entry[1].add(kept)
    return entry[0]


def _istft_rows(spec):
    """logical (*, F, T, 2) -> the frame-major (rows, T, F, 2) tensor the kernels read, without a copy where the input already
    is one (the strided views ``stft`` and ``phase_vocoder`` return)."""
    sp = spec.transpose(-3, -2)
    if sp.is_contiguous() and sp.data_ptr() % 16 == 0:
        istft_layout['in_place'] += 1
    else:
        istft_layout['copied'] += 1
        sp = sp.contiguous()
    return sp.reshape((-1,) + tuple(sp.shape[-3:]))


def istft(spec, window, n_fft, hop, win_length, center, normalized, length, route=None):
    """one-sided ``(*, F, T, 2)`` float32 -> ``(*, samples)`` (tac_istft_f32).  fft_length 2048 with hop 256 / 512 / 1024 and
    ``center``: one fused launch — inverse transform, window and overlap-add in LDS, no frame in memory, no workspace.  Every
    other geometry (and ``route='general'``, the measuring tools' A/B switch): the frame kernels in inverse mode into a workspace,
    then the gather that divides by the window envelope.  Either way every output element is written by the launch."""
    n_frames = int(spec.shape[-2])
    full = istft_full_length(n_frames, n_fft, hop, center)
    if full <= 0:
        raise RuntimeError('istft: %d frame(s) of fft_length %d leave no samples after removing the centre padding'
                           % (n_frames, n_fft))
    out_len = full if length is None else int(length)
    inv_env = istft_envelope(window, n_fft, hop, win_length, center, n_frames, min(full + (n_fft // 2 if center else 0), out_len))
    lead = tuple(int(s) for s in spec.shape[:-3])
    rows = _istft_rows(spec)
    n_rows = int(rows.shape[0])
    out = _empty(lead + (out_len,), device=spec.device)
    desc = _istft_desc(n_rows, out_len, out_len, n_fft, hop, win_length, center, normalized)
    need = int(_native.lib().tac_istft_workspace(desc, n_frames))
    if need < 0:
        _native.check(need, 'tac_istft_workspace')

    head = (_native.ptr(rows), rows.stride(0), rows.stride(1), n_frames, _native.ptr(window), _native.ptr(inv_env), desc)
    rc = _native.TAC_E_UNSUPPORTED
    if need == 0 and route != 'general':
        rc = _launch('tac_istft_f32', spec.device, (out,), *head, None, 0, _native.ptr(out), accept=_DECLINED)
    if rc == _native.TAC_E_UNSUPPORTED:                                 # (the general route takes any geometry and alignment)
        need = n_rows * n_frames * n_fft * 4
        work = torch.empty(need // 4, dtype=torch.float32, device=spec.device)      # scratch: every frame is written before it is read
        _launch('tac_istft_f32', spec.device, (out,), *head, _native.ptr(work), need, _native.ptr(out))
    return out


def istft_backward(grad_out, window, n_fft, hop, win_length, center, normalized, n_frames):
    """gradient of ``istft`` w.r.t. the spectrogram, ``(*, samples) -> (*, F, T, 2)``: ``stft`` (center=False framing, same
    window) of ``grad_out / env`` zero-extended to the padded length, then the bin weights of irfft's adjoint — 1 for the real
    parts of the DC and Nyquist bins, 0 for their imaginary parts, 2 elsewhere, times the inverse's 1 / N (sqrt(N) / N)."""
    out_len = int(grad_out.shape[-1])
    full = istft_full_length(n_frames, n_fft, hop, center)
    inv_env = istft_envelope(window, n_fft, hop, win_length, center, n_frames, min(full + (n_fft // 2 if center else 0), out_len))
    lead = tuple(int(s) for s in grad_out.shape[:-1])
    go = grad_out.reshape(-1, out_len)
    go = go if go.is_contiguous() else go.contiguous()
    n_rows, n_pos, n_bins = int(go.shape[0]), hop * (n_frames - 1) + n_fft, n_fft // 2 + 1
    padded = _empty((n_rows, n_pos), device=go.device)
    gspec = _empty(lead + (n_frames, n_bins, 2), device=go.device)
    dev = go.device
    with _native.on_device(dev):
        _launch('tac_istft_grad_input_f32', dev, (padded,), _native.ptr(go), out_len, _native.ptr(inv_env),
                _istft_desc(n_rows, out_len, out_len, n_fft, hop, win_length, center, normalized), n_frames, _native.ptr(padded))
        fwd = _native.StftDesc(rows=n_rows, length=n_pos, row_stride=n_pos, n_fft=n_fft, hop=hop, win_length=win_length, center=0,
                               pad_mode=0, normalized=0, onesided=1, reserved=0)
        _launch('tac_stft_f32', dev, (gspec,), _native.ptr(padded), _native.ptr(window), fwd, _native.ptr(gspec))
        _launch('tac_istft_grad_bins_f32', dev, (gspec,), _native.ptr(gspec), n_rows * n_frames, n_fft, 1 if normalized else 0)
    return gspec.transpose(-3, -2)


# ----------------------------------------------------------------------------- Griffin-Lim (csrc/griffinlim.hip)
def griffinlim_covers(specgram, angles0=None):
    """the layouts ``tac_griffinlim_prepare_f32`` reads where they lie: positive strides on every axis longer than one"""
    for t in (specgram, angles0):
        if t is not None and any(n > 1 and s <= 0 for n, s in zip(t.shape, t.stride())):
            return False
    return True


def _gl_rows(t, n_freqs, n_frames):
    """``(…, F, T)`` as ``(rows, F, T)`` with ONE row stride: a view where the leading dims fold, else a copy of plain data"""
    try:
        return t.view(-1, n_freqs, n_frames)
    except RuntimeError:
        return t.reshape(-1, n_freqs, n_frames)


def griffinlim_prepare(specgram, angles0, power):
    """``(rows, F, T)`` float32 with any positive strides (and ``angles0``, complex64 of that shape, or None) -> the frame-major
    magnitude ``M (rows, T, F)`` and first iterate ``X0 (rows, T, F, 2)``, one launch.  A dense frame-major input at power 1 IS
    ``M``: nothing is copied and only ``X0`` is written."""
    rows, n_freqs, n_frames = (int(s) for s in specgram.shape)
    dev = specgram.device
    fm = specgram.transpose(1, 2)
    keep = float(power) == 1.0 and fm.is_contiguous() and fm.data_ptr() % 16 == 0
    mag = fm if keep else _empty((rows, n_frames, n_freqs), device=dev)
    x0 = _empty((rows, n_frames, n_freqs, 2), device=dev)
    a_args = (None, 0, 0, 0) if angles0 is None else (_native.ptr(angles0),) + tuple(int(s) for s in angles0.stride())
    _launch('tac_griffinlim_prepare_f32', dev, (x0,) if keep else (mag, x0), _native.ptr(specgram), rows, n_freqs, n_frames,
            *(int(s) for s in specgram.stride()), *a_args, float(power), None if keep else _native.ptr(mag), _native.ptr(x0))
    return mag, x0


def griffinlim_update(r, rprev, mag, m):
    """``X = M (R - m Rprev) / (|R - m Rprev| + 1e-16)`` over frame-major ``(…, 2)`` pairs (``rprev`` None on the first step), one
    launch.  The operands are read where they lie and have to be dense; any element alignment."""
    x = _empty(tuple(r.shape), device=r.device)
    _launch('tac_griffinlim_update_f32', r.device, (x,), _native.ptr(r), None if rprev is None else _native.ptr(rprev),
            _native.ptr(mag), r.numel() // 2, float(m), _native.ptr(x))
    return x


def griffinlim(specgram, window, angles0, n_fft, hop, win_length, power, n_iter, m, length):
    """``(…, F, T)`` float32 magnitudes -> ``(…, samples)``: one prepare launch, then per iteration ``tac_istft_f32`` (its fused
    one-launch route at fft_length 2048), ``tac_stft_f32`` and the update kernel.  ``Rprev`` is the previous ``stft`` output kept by
    reference; every buffer of an iteration is released to the allocator before the next one asks, so nothing grows with
    ``n_iter``, and nothing inside the loop waits for the host (the NOLA check of the window's envelope is cached on the window)."""
    n_freqs, n_frames = int(specgram.shape[-2]), int(specgram.shape[-1])
    lead = tuple(int(s) for s in specgram.shape[:-2])
    full = istft_full_length(n_frames, n_fft, hop, True)
    out_len = full if length is None else int(length)
    istft_envelope(window, n_fft, hop, win_length, True, n_frames, min(full + n_fft // 2, out_len))      # NOLA, before any launch of the op
    spec3 = _gl_rows(specgram, n_freqs, n_frames)
    ang3 = None if angles0 is None else _gl_rows(angles0, n_freqs, n_frames)
    mag, x = griffinlim_prepare(spec3, ang3, power)
    y = istft(x.transpose(1, 2), window, n_fft, hop, win_length, True, False, length)
    prev = None
    for _ in range(n_iter):
        r = stft(y, window, n_fft, hop, win_length, True, 'reflect', False, True).transpose(1, 2)      # frame-major, dense
        x = griffinlim_update(r, prev, mag, m)
        y = istft(x.transpose(1, 2), window, n_fft, hop, win_length, True, False, length)
        prev = r
    return y.reshape(lead + (out_len,))


# ----------------------------------------------------------------------------- poisoned outputs (test hook)
# While ``set_poison_outputs(True)`` is on, every buffer a launcher here allocates for a kernel to fill starts as a fixed bit
# pattern (a quiet NaN with a payload no arithmetic produces; a negative sentinel for int64 codes), and after each launch the
# part of the buffer that launch fills is compared with the pattern on the launch stream.  Hits are added to a device counter
# per entry point; ``poison_report()`` reads them (one host sync, outside any call).  A position no kernel writes can then
# neither pass a comparison by holding an earlier identical result nor hide as zeros of a fresh allocation.
# Constant tables built once per filterbank or window (packed banks, tile plans, adjoint tables) and the gradient copies torch
# itself fills (``go``) are not per-call kernel outputs and are allocated plainly.
POISON_OUTPUTS = False          # read-only mirror of the switch: change it with set_poison_outputs()

#: the poison patterns, as the integers of the same width the buffer is viewed as
POISON_BITS = {torch.float32: 0x7FC0DEAD, torch.float64: 0x7FF80000DEADBEEF, torch.int64: -0x21524111DEADBEEF,
               torch.int32: -0x21524111}
_BIT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int64: torch.int64, torch.int32: torch.int32}
_poison_hits = {}                # (entry point, device index) -> int64 device counter of poisoned elements left after a launch


def set_poison_outputs(on):
    """Switch poisoning and the write check on or off — for the ctypes launchers here and the compiled binding alike."""
    global POISON_OUTPUTS
    POISON_OUTPUTS = bool(on)
    ext = _native.ext()
    if ext is not None:
        ext.set_poison(POISON_OUTPUTS)


def poison_fill(t):
    """Fill ``t`` (float32 / float64 / int32 / int64, any device) with its poison pattern; returns ``t``."""
    if t.numel():
        t.view(_BIT_VIEW[t.dtype]).fill_(POISON_BITS[t.dtype])
    return t


def poison_count(t):
    """Number of elements of ``t`` that hold the poison pattern, as a 0-d int64 tensor on ``t``'s device (no host sync)."""
    if not t.numel():
        return torch.zeros((), dtype=torch.int64, device=t.device)
    return (t.view(_BIT_VIEW[t.dtype]) == POISON_BITS[t.dtype]).sum()


def _poisoning(t):
    return POISON_OUTPUTS and not (t.is_cuda and torch.cuda.is_current_stream_capturing())


def _empty(shape, dtype=torch.float32, device=None):
    out = torch.empty(shape, dtype=dtype, device=device)
    return poison_fill(out) if _poisoning(out) else out


def _empty_strided(shape, stride, dtype=torch.float32, device=None):
    out = torch.empty_strided(shape, stride, dtype=dtype, device=device)
    return poison_fill(out) if _poisoning(out) else out


def _empty_like(x):
    out = torch.empty_like(x)
    return poison_fill(out) if _poisoning(out) else out


def check_written(name, *parts):
    """After a launch of ``name``: count the poisoned elements left in ``parts`` (the tensors, or the slices of them, that
    this launch fills) into the entry point's device counter.  Enqueued on the current stream; skipped while a graph is
    being captured and while poisoning is off."""
    if not POISON_OUTPUTS:
        return
    for t in parts:
        if t is None or not t.numel() or not _poisoning(t):
            continue
        key = (name, t.device.index)
        acc = _poison_hits.get(key)
        if acc is None:
            with torch.inference_mode(False):       # (an inference tensor could not be updated outside inference mode)
                acc = _poison_hits[key] = torch.zeros((), dtype=torch.int64, device=t.device)
        acc += poison_count(t)


def poison_report(reset=True):
    """{entry point: number of poisoned elements its launches left} for every entry point with at least one, since the last
    reset.  Reads the device counters (a host synchronisation): call it between calls, not inside one."""
    bad = {}
    for (name, _), acc in list(_poison_hits.items()):
        n = int(acc.item())
        if n:
            bad[name] = bad.get(name, 0) + n
    if reset:
        _poison_hits.clear()
    return bad

# A/B knob for the two fused Melspectrogram kernels: 'auto' (band-sparse when the bank allows it, else MFMA),
# 'sparse', 'mfma'
MEL_PATH = os.environ.get('TAC_MEL_PATH', 'auto')


def _melbank_pack(fb, n_fft):
    """(wpack, desc, info) device/host buffers of the band-sparse contraction for this filterbank and fft size, or
    None when the bank is not band-sparse enough (then the MFMA kernels are used).  Built once per filterbank
    version (one host sync) and cached on the tensor object."""
    def build():
        n_freqs, n_mels = fb.shape
        wpack = torch.empty(24576, dtype=torch.float32, device=fb.device)
        desc = torch.empty(8192, dtype=torch.int32, device=fb.device)
        info = (ctypes.c_int32 * 8)()
        with _native.on_device(fb.device):
            rc = _native.lib().tac_melbank_pack(_native.ptr(fb), n_freqs, n_mels, n_fft, _native.ptr(wpack), 24576,
                                                _native.ptr(desc), 8192, ctypes.cast(info, ctypes.c_void_p),
                                                _native.stream_ptr(fb.device))
        if rc == _native.TAC_E_UNSUPPORTED:
            return None
        _native.check(rc, 'tac_melbank_pack')
        return wpack, desc, info
    return cached_on(fb, '_tac_pack', n_fft, build)


# The fused fft_length-2048 float32 launches contract 128-band banks in the PAIR layout (csrc/melspec_sparse.hip pack_pairs: 14
# steps per frame instead of 4 + 14 for the standard bank).  False: the classic lane layout — for same-process A/B runs and the test
# that compares the two; packs are cached per selector, plans are not: call ``invalidate()`` after changing it.
PAIR_LAYOUT = True
PACK_PAIRS_2048 = -2048         # TAC_PACK_PAIRS_2048 (include/tac_amd.h): the one Python copy; tools take it from here


def _fused_pack(fb, n_fft):
    """``_melbank_pack`` for the forward float32 fused launch: the pair layout where the bank fits one of its shapes, else
    (and for every other fft size) the classic pack.  The coded-input and backward kernels take the classic pack."""
    if PAIR_LAYOUT and n_fft == 2048 and tuple(fb.shape) == (1025, 128):
        pack = _melbank_pack(fb, PACK_PAIRS_2048)
        if pack is not None:
            return pack
    return _melbank_pack(fb, n_fft)


def _filterbank_plan(fb):
    """(device int32 plan, host ctypes copy): non-zero bin range per 16-band tile, computed by a device kernel.
    The plan rides on the filterbank tensor object itself (a module's constant buffer is scanned once — the only
    host sync on the path — and rescanned when modified in place); keying a cache on ``data_ptr`` would go stale
    when the allocator reuses an address."""
    def build():
        n_freqs, n_mels = fb.shape
        n_ints = 2 * ((n_mels + 15) // 16)
        plan = torch.empty(n_ints, dtype=torch.int32, device=fb.device)
        host = (ctypes.c_int32 * n_ints)()
        with _native.on_device(fb.device):
            rc = _native.lib().tac_filterbank_plan(_native.ptr(fb), n_freqs, n_mels, _native.ptr(plan),
                                                   ctypes.cast(host, ctypes.c_void_p), _native.stream_ptr(fb.device))
        _native.check(rc, 'tac_filterbank_plan')
        return plan, host
    return cached_on(fb, '_tac_plan', fb.device, build)


def _fused_mel_route(g, fb, power):
    """'sparse' / 'mfma' when one fused kernel covers this geometry + filterbank, else None (then the caller chains
    the spectrogram, filterbank and dB kernels)."""
    if not ((g.pow2_kernel or g.mixed_radix) and g.onesided and g.n_fft <= 4096 and fb.dim() == 2 and
            fb.shape[0] == g.n_bins and 0 < fb.shape[1] <= 512 and fb.is_contiguous()):
        return None
    if g.mixed_radix:       # fft_length 400: only the band-sparse form has a fused kernel
        ok = power in (1.0, 2.0) and MEL_PATH != 'mfma' and _melbank_pack(fb, g.n_fft) is not None
        return 'sparse' if ok else None
    if power in (1.0, 2.0) and MEL_PATH != 'mfma' and _melbank_pack(fb, g.n_fft) is not None:
        return 'sparse'
    if MEL_PATH == 'sparse' or g.n_fft > 2048:      # (fft_length 4096: only the band-sparse form has a fused kernel)
        return None
    _, host = _filterbank_plan(fb)
    rc = _native.lib().tac_melspec_supported(g.desc, float(power), ctypes.cast(host, ctypes.c_void_p), fb.shape[1])
    return 'mfma' if rc == _native.TAC_OK else None


class MelPlan(object):
    """Bound-argument launcher of the fused band-sparse kernel for ONE (waveform layout, window, filterbank, parameters):
    what ``melspectrogram`` below works out on every call — geometry, route, packed bank, ctypes conversions — done once.
    ``launch(wave)`` then costs an allocation and one foreign call.  Valid while the window and the filterbank keep their
    stamps (checked by the caller, ``_lazy.DeferredSpectral.realize``) and the device is current."""
    __slots__ = ('fn', 'win_ptr', 'desc', 'power', 'wpack', 'dsc', 'info', 'wpack_ptr', 'dsc_ptr', 'info_ptr', 'n_mels',
                 'db', 'ref', 'amin', 'shape', 'device', 'dev_index', 'window', 'fb', 'win_stamp', 'fb_stamp', 'layout', 'cplan',
                 'last_rc')

    def run(self, wave):
        """``matches`` + ``launch`` in one: the result, or None when the plan does not apply (any more).  With the compiled
        binding (csrc/binding/tac_ext.cpp) the checks, the allocation, the stream lookup and the foreign call are one C++ call."""
        c = self.cplan
        if c is not None:
            v = c.launch(wave)
            if v is not None:
                launches['tac_melspec_sparse_f32'] = launches.get('tac_melspec_sparse_f32', 0) + 1
                if POISON_OUTPUTS:                  # (the binding poisons its output while the switch is on)
                    check_written('tac_melspec_sparse_f32', v)
            else:
                self.last_rc = c.last_rc
            return v
        return self.launch(wave) if self.matches(wave) else None

    def launch(self, wave):
        out = _empty(self.shape, device=self.device)
        rc = self.fn(wave.data_ptr(), self.win_ptr, self.desc, self.power, self.wpack_ptr, self.dsc_ptr, self.info_ptr,
                     self.n_mels, self.db, self.ref, self.amin, out.data_ptr(),
                     torch._C._cuda_getCurrentRawStream(self.dev_index))
        if rc != _native.TAC_OK:
            self.last_rc = rc
            return None                     # (the general path reports it)
        launches['tac_melspec_sparse_f32'] = launches.get('tac_melspec_sparse_f32', 0) + 1
        if POISON_OUTPUTS:
            check_written('tac_melspec_sparse_f32', out)
        return out.transpose(-2, -1)

    def matches(self, wave):
        """same layout, same device current, tables still those of the tensors' current contents"""
        return (wave.shape, wave.stride(), wave.dtype) == self.layout and torch._C._cuda_getDevice() == self.dev_index \
            and _stamp(self.window) == self.win_stamp and _stamp(self.fb) == self.fb_stamp


def mel_plan(wave, window, fb, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db, ref, amin):
    """A ``MelPlan`` when this call is one launch of the fused band-sparse kernel on plain float32 tensors whose rows need no
    copy, else None (the general ``melspectrogram`` handles everything)."""
    if not (type(wave) is torch.Tensor and wave.dtype == torch.float32 and window.dtype == torch.float32
            and window.is_contiguous() and fb.dtype == torch.float32 and fb.dim() == 2 and wave.is_cuda
            and window.device == wave.device and fb.device == wave.device and not window.is_inference()
            and not fb.is_inference()):
        return None
    g = geometry(wave, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    if g.flatten or g.desc is None or fb.shape[0] != g.n_bins or _fused_mel_route(g, fb, power) != 'sparse':
        return None
    wpack, dsc, info = _fused_pack(fb, g.n_fft)
    p = MelPlan()
    p.fn = _native.lib().tac_melspec_sparse_f32
    p.window, p.fb, p.win_stamp, p.fb_stamp = window, fb, _stamp(window), _stamp(fb)
    p.win_ptr, p.desc, p.power = window.data_ptr(), g.desc, float(power)
    p.wpack, p.dsc, p.info = wpack, dsc, info                          # (kept alive with the plan)
    p.wpack_ptr, p.dsc_ptr, p.info_ptr = wpack.data_ptr(), dsc.data_ptr(), ctypes.cast(info, ctypes.c_void_p)
    p.n_mels, p.db, p.ref, p.amin = int(fb.shape[1]), 1 if db else 0, float(ref), float(amin)
    p.shape = g.lead + (g.n_frames, int(fb.shape[1]))
    p.device, p.dev_index = wave.device, wave.device.index
    p.layout = (wave.shape, wave.stride(), wave.dtype)
    p.cplan = None
    p.last_rc = 0
    ext = _native.ext()
    if ext is not None:
        try:
            p.cplan = ext.MelPlan(ctypes.cast(p.fn, ctypes.c_void_p).value, wave, window, fb, wpack, dsc, bytes(g.desc),
                                  [int(v) for v in info], p.power, p.n_mels, bool(db), p.ref, p.amin, [int(n) for n in p.shape],
                                  _epoch)
        except Exception:                       # noqa: BLE001 — the ctypes launcher above covers the call
            p.cplan = None
    return p


def melspectrogram(wave, window, fb, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db, ref,
                   amin):
    g = geometry(wave, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    if fb.dim() != 2 or fb.shape[0] != g.n_bins:
        raise RuntimeError('apply_filterbank: size mismatch, spectrogram has %d bins, filterbank %s'
                           % (g.n_bins, tuple(fb.shape)))
    # the route is cached per (filterbank object, version, power); ``id`` alone could be reused by a NEW tensor once
    # the old one is collected, so the entry carries a weak reference that must still point at this very object
    rkey = (id(fb), _stamp(fb), power, MEL_PATH)
    hit = g.routes.get(rkey)
    if hit is not None and hit[0]() is fb:
        route = hit[1]
    else:
        if len(g.routes) > 16:
            g.routes.clear()
        route = _fused_mel_route(g, fb, power)
        g.routes[rkey] = (weakref.ref(fb), route)
    if route is None:       # (fft_length 4096, |X|^p with p outside {1, 2}, banks the fused kernels reject)
        spec = spectrogram(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power,
                           False, 1.0, 1e-7)
        return apply_filterbank(spec, fb, db=(ref, amin) if db else None)    # the dB epilogue rides on the filterbank kernel
    n_mels = fb.shape[1]
    src = _rows_of(wave, g)
    out = _empty(g.lead + (g.n_frames, n_mels), device=wave.device)
    if route == 'sparse':          # band-sparse contraction (the faster form for triangular banks)
        wpack, desc, info = _fused_pack(fb, g.n_fft)
        rc = _launch('tac_melspec_sparse_f32', wave.device, (out,), _native.ptr(src), _native.ptr(window), g.desc, float(power),
                     _native.ptr(wpack), _native.ptr(desc), ctypes.cast(info, ctypes.c_void_p), n_mels, 1 if db else 0,
                     float(ref), float(amin), _native.ptr(out), accept=_DECLINED)
        if rc == _native.TAC_E_UNSUPPORTED:         # a geometry the fused kernel of this size declines: the two-kernel chain
            spec = spectrogram(wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power,
                               False, 1.0, 1e-7)
            return apply_filterbank(spec, fb, db=(ref, amin) if db else None)
        return out.transpose(-2, -1)
    _, plan_host = _filterbank_plan(fb)
    _launch('tac_melspec_f32', wave.device, (out,), _native.ptr(src), _native.ptr(window), g.desc, float(power), _native.ptr(fb),
            ctypes.cast(plan_host, ctypes.c_void_p), n_mels, 1 if db else 0, float(ref), float(amin), _native.ptr(out))
    return out.transpose(-2, -1)


# ----------------------------------------------------------------------------- filterbank
def apply_filterbank(spec, fb, allow_sparse=True, db=None):
    """``db = (ref, amin)``: followed by ``amplitude_to_db`` — in the same launch when the band-sparse streaming kernel
    takes the call, as a second kernel behind the MFMA GEMM."""
    fb = fb if fb.is_contiguous() else fb.contiguous()
    n_freqs, n_frames = spec.shape[-2], spec.shape[-1]
    lead = tuple(spec.shape[:-2])
    n_mels = fb.shape[1]
    out = _empty(lead + (n_frames, n_mels), device=spec.device)
    if out.numel():
        rows = spec.reshape(-1, n_freqs, n_frames)
        # frame-major spectrogram (what the kernels here produce) + band-sparse bank: stream it through the fused
        # kernel's contraction; anything else goes through the fp32 MFMA GEMM
        pack = _melbank_pack(fb, 0) if (allow_sparse and rows.stride(1) == 1 and MEL_PATH != 'mfma') else None
        if pack is not None:
            wpack, desc, info = pack
            head = (_native.ptr(rows), rows.shape[0], n_freqs, n_frames, rows.stride(0) if rows.shape[0] > 1 else 0, rows.stride(2),
                    _native.ptr(wpack), _native.ptr(desc), ctypes.cast(info, ctypes.c_void_p), n_mels)
            if db is None:
                rc = _launch('tac_apply_filterbank_sparse_f32', spec.device, (out,), *head, _native.ptr(out),
                             accept=_DECLINED)
            else:
                rc = _launch('tac_apply_filterbank_sparse_db_f32', spec.device, (out,), *head, 1, float(db[0]), float(db[1]),
                             _native.ptr(out), accept=_DECLINED)
            if rc != _native.TAC_E_UNSUPPORTED:
                return out.transpose(-2, -1)
        plan, _ = _filterbank_plan(fb)
        _launch('tac_apply_filterbank_f32', spec.device, (out,), _native.ptr(rows), rows.shape[0], n_freqs, n_frames, rows.stride(0),
                rows.stride(1), rows.stride(2), _native.ptr(fb), _native.ptr(plan), n_mels, _native.ptr(out))
    out = out.transpose(-2, -1)
    return out if db is None else amplitude_to_db(out, db[0], db[1])


# ----------------------------------------------------------------------------- DCT (MFCC)
DCT_MAX_DIM, DCT_MAX_MATRIX = 256, 32768


def dct_covers(n_in, n_out):
    """The sizes ``tac_dct_rows_f32`` holds in the LDS (csrc/mfcc.hip) — symmetric, so that the gradient (the same kernel with
    the transposed matrix) is covered whenever the forward is."""
    return 1 <= n_in <= DCT_MAX_DIM and 1 <= n_out <= DCT_MAX_DIM and n_in * n_out <= DCT_MAX_MATRIX


def _dct_matrix(mat, transposed):
    """``mat`` (or its transpose, for the gradient) as a contiguous float32 tensor on its device; copies are cached on the tensor
    object per version, like the filterbank's packs and its transpose."""
    if not transposed and mat.dtype == torch.float32 and mat.is_contiguous():
        return mat.detach()
    def build():
        src = mat.detach().t() if transposed else mat.detach()
        return src.to(torch.float32).contiguous()
    return cached_on(mat, '_tac_dct', bool(transposed), build)


def dct_rows(x, mat, transposed=False):
    """``(…, n_in, T) x (n_in, n_out) -> (…, n_out, T)``: ``tac_dct_rows_f32`` on ``x`` where it lies — any strides; the leading
    dims are copied only when no single row stride expresses them.  ``transposed``: ``mat`` is ``(n_out, n_in)`` and applied as
    its transpose (the gradient).  The result is the logical view of frame-major storage, like every spectral output here."""
    m = _dct_matrix(mat, transposed)
    n_in, n_out = m.shape
    n_frames = x.shape[-1]
    lead = tuple(x.shape[:-2])
    out = _empty(lead + (n_frames, n_out), device=x.device)
    if out.numel():
        rows = x.reshape(-1, n_in, n_frames)            # a view wherever the leading dims collapse into one stride
        if any(st <= 0 for st, n in zip(rows.stride(), rows.shape) if n > 1):
            rows = rows.contiguous()                    # (expanded / flipped axes: the kernel takes positive strides)
        _launch('tac_dct_rows_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], n_in, n_frames, rows.stride(0), rows.stride(1),
                rows.stride(2), _native.ptr(m), n_out, _native.ptr(out))
    return out.transpose(-2, -1)


# ----------------------------------------------------------------------------- resample
#: floats of compact bank (phases * taps) ``tac_polyphase_f32`` holds in the LDS: 80 KiB, half of it.  Both banks of every pair
#: among 8000 / 11025 / 12000 / 16000 / 22050 / 24000 / 32000 / 44100 / 48000 / 88200 / 96000 Hz at the default filter fit
#: (the largest, the gradient of 32000 -> 11025 and 96000 -> 11025, is 1280 x 13 = 16640).
RESAMPLE_MAX_BANK = 20480
RESAMPLE_MAX_PHASES = 2048
#: outputs per tile of the kernel (512 / 256 where 1024 outputs' input span does not fit), and the spans' limits in floats
RESAMPLE_TILE = 1024
_RS_SPAN_WIDE, _RS_SPAN_MAX = 8192, 14336


def _rs_span_cap(b, tile, off_min, off_max):
    return (3 + ((b.phases - 1 + tile - 1) // b.phases) * b.step + (off_max - off_min) + b.K + 3) & ~3


def resample_tile(b):
    """Outputs per tile ``tac_polyphase_f32`` takes for this bank (csrc/resample.hip), or None where it does not cover it."""
    if b.phases > RESAMPLE_MAX_PHASES or b.phases * b.K > RESAMPLE_MAX_BANK:
        return None
    off_min, off_max = min(b.off), max(b.off)
    for tile in (1024, 512, 256):
        if _rs_span_cap(b, tile, off_min, off_max) <= (_RS_SPAN_MAX if tile == 256 else _RS_SPAN_WIDE):
            return tile
    return None


def resample_covers(orig, new, lpw, rolloff, method, beta):
    """True where the kernel holds BOTH banks of this (reduced) pair — the forward's and the gradient's — so that a call that
    runs on the kernel also trains on it."""
    return resample_tile(_resample.bank(orig, new, lpw, rolloff, method, beta)) is not None and \
        resample_tile(_resample.adjoint_bank(orig, new, lpw, rolloff, method, beta)) is not None


_resample_tables = Bounded(64)


def _resample_device_bank(key, adjoint, device):
    """(Bank, tap-major float32 bank, int32 [off | run], off_min, off_max, run_min) on ``device``: rounded once from the
    float64 bank, cached per argument tuple and device."""
    hit = _resample_tables.get((key, adjoint, device))
    if hit is None:
        b = (_resample.adjoint_bank if adjoint else _resample.bank)(*key)
        taps = b.taps.t().contiguous().to(torch.float32).to(device)
        table = torch.tensor([b.off, b.run], dtype=torch.int32).to(device)
        hit = _resample_tables[(key, adjoint, device)] = (b, taps, table, min(b.off), max(b.off), min(b.run))
    return hit


def polyphase(x, key, n_out, adjoint=False):
    """``(…, L) -> (…, n_out)`` through ``tac_polyphase_f32`` with the forward bank of ``key`` (the reduced argument tuple of
    ``_resample.bank``) or, ``adjoint``, with its transpose: one launch.  ``x`` is read where it lies when its leading dims
    collapse into one positive row stride over unit-stride rows; it is copied otherwise."""
    b, taps, table, off_min, off_max, run_min = _resample_device_bank(key, adjoint, x.device)
    length = x.shape[-1]
    out = _empty(tuple(x.shape[:-1]) + (n_out,), device=x.device)
    if out.numel():
        if length == 0:
            return out.zero_()
        rows = x.reshape(-1, length)
        if (length > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) <= 0):
            rows = rows.contiguous()
        _launch('tac_polyphase_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], length, rows.stride(0), _native.ptr(taps),
                _native.ptr(table), b.phases, b.K, run_min, b.step, off_min, off_max, n_out, _native.ptr(out))
    return out


#: what ``tac_polyphase_wide_f32`` takes (csrc/resample.hip: RSW_*): floats of bank it reads from global memory (4 MB: an XCD's L2
#: with the Infinity Cache behind it), taps per phase, floats of one tile's input span, rows of a unit, bytes of LDS
RESAMPLE_WIDE_MAX_BANK = 1 << 20
RESAMPLE_WIDE_MAX_TAPS = 64
RESAMPLE_WIDE_SPAN_MAX = 8192
RESAMPLE_WIDE_ROWS = 4
_RSW_LDS_BYTES = 160 * 1024

_wide_plans = Bounded(64)


def resample_wide_starts(b):
    """int64 ``(phases + 1,)``: the first input sample output ``n`` reads, ``j * step + off[p]``, for ``n = 0 .. phases``"""
    off = torch.tensor(b.off, dtype=torch.int64)
    return torch.cat((off, off[:1] + b.step))


def resample_wide_plan(b):
    """``(span, tile)`` of ``tac_polyphase_wide_f32`` for this bank, or None where the kernel does not take it.  The kernel stages,
    per tile of ``tile`` consecutive outputs, the inputs from the first one its FIRST output reads — which is the first one any
    of them reads only if the starts ``j * step + off[p]`` never decrease in ``n``, across the wrap ``p = phases - 1 -> 0`` too:
    checked here.  ``span`` is the exact maximum, over every phase a tile can start at, of the samples from there to the last
    one the tile reads (a sliding maximum of ``start + run`` over ``phases + tile - 1`` outputs).  Cached per bank."""
    hit = _wide_plans.get(id(b))
    if hit is not None and hit[0] is b:
        return hit[1]
    plan = None
    start = resample_wide_starts(b)
    if b.K <= RESAMPLE_WIDE_MAX_TAPS and b.phases * b.K <= RESAMPLE_WIDE_MAX_BANK and not bool((start[1:] < start[:-1]).any()):
        off = torch.tensor(b.off, dtype=torch.int64)
        run = torch.tensor(b.run, dtype=torch.int64).clamp(0, b.K)
        for tile in (1024, 512, 256):
            n = torch.arange(b.phases + tile - 1, dtype=torch.int64)
            j = torch.div(n, b.phases, rounding_mode='floor')
            p = n - j * b.phases
            first = j * b.step + off[p]
            last = (first + run[p]).unfold(0, tile, 1).max(dim=1).values           # (phases,): the end of the tile that starts at n
            span = max(int((last - first[:b.phases]).max()), 1)
            if span <= RESAMPLE_WIDE_SPAN_MAX and 4 * RESAMPLE_WIDE_ROWS * ((3 + span + b.K + 3) & ~3) <= _RSW_LDS_BYTES:
                plan = (span, tile)
                break
    _wide_plans[id(b)] = (b, plan)
    return plan


def resample_fit_covers(key, length, out_len):
    """True where ``resample_fit`` of ``(…, length)`` to ``out_len`` samples runs AND trains on the kernels: the LDS kernel where it
    holds both banks and nothing is cut or padded, else the wide kernel where both banks have a plan."""
    if resample_covers(*key) and out_len == _resample.out_length(length, key[0], key[1]):
        return True
    return resample_wide_plan(_resample.bank(*key)) is not None and resample_wide_plan(_resample.adjoint_bank(*key)) is not None


def polyphase_wide(x, key, n_out, out_len, adjoint=False, l_in=None, out=None):
    """``(…, L) -> (…, out_len)`` through ``tac_polyphase_wide_f32``: the sums of ``polyphase`` for ``n < min(n_out, out_len)``,
    zeros behind them; one launch.  ``l_in``: the samples of a row that are read (the rest count as zero), all of them by default;
    ``out``: a dense float32 tensor of the result's shape to fill instead of a new one."""
    b, taps, table, _, _, _ = _resample_device_bank(key, adjoint, x.device)
    plan = resample_wide_plan(b)
    if plan is None:
        raise RuntimeError('polyphase_wide: the bank of %d phases x %d taps has no plan (resample_wide_plan)' % (b.phases, b.K))
    length = x.shape[-1] if l_in is None else min(int(l_in), x.shape[-1])
    shape = tuple(x.shape[:-1]) + (out_len,)
    if out is None:
        out = _empty(shape, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError('polyphase_wide: out must be a dense float32 tensor of shape %r on %s' % (shape, x.device))
    if out.numel():
        if length <= 0 or n_out <= 0:
            return out.zero_()
        rows = x.reshape(-1, x.shape[-1])
        if (x.shape[-1] > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) <= 0):
            rows = rows.contiguous()
        _launch('tac_polyphase_wide_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], length, rows.stride(0),
                _native.ptr(taps), _native.ptr(table), b.phases, b.K, b.step, plan[0], plan[1], n_out, out_len, _native.ptr(out))
    return out


def resample_fit(x, key, out_len, adjoint=False, length=None, wide=None):
    """``resample`` by the reduced pair of ``key`` cut or zero-padded to ``out_len`` samples; with ``adjoint`` its gradient: ``x`` is
    grad_out ``(…, out_len)``, read as zero beyond ``min(n_out, out_len)``, and the result has ``length`` samples.  The LDS kernel
    where it holds the banks and ``out_len == n_out``, the wide kernel otherwise — the same bits; ``wide`` forces either."""
    n_out = _resample.out_length(length if adjoint else x.shape[-1], key[0], key[1])
    if wide is None:
        wide = not (out_len == n_out and resample_covers(*key))
    if not wide:
        return polyphase(x, key, length if adjoint else n_out, adjoint=adjoint)
    if adjoint:
        return polyphase_wide(x, key, length, length, adjoint=True, l_in=min(n_out, out_len))
    return polyphase_wide(x, key, n_out, out_len)


# ----------------------------------------------------------------------------- lfilter
#: samples per lane and per tile of ``tac_lfilter_f32`` (csrc/lfilter.hip: LF_C, LF_TILE = 1024 lanes * LF_C); checked against the
#: library's own value at the first launch
LFILTER_C = 16
LFILTER_TILE = 1024 * LFILTER_C
#: coefficients per side the kernel takes (order <= 2)
LFILTER_MAX_COEFFS = 3

_lfilter_ok = Bounded(256)
_lfilter_chunk_checked = False


def _lfilter_arrays(b, a):
    n = len(a)
    return (ctypes.c_double * n)(*b), (ctypes.c_double * n)(*a)


def lfilter_covers(b, a):
    """True where ``tac_lfilter_f32`` takes these coefficients (tuples of Python floats, ``a[0] != 0`` already checked): at most
    three per side, and a state transition over one tile that is finite in float64 (any stable filter, and the unstable ones up to
    a pole radius of about 1.09)."""
    key = (tuple(b), tuple(a))
    hit = _lfilter_ok.get(key)
    if hit is None:
        if len(key[1]) > LFILTER_MAX_COEFFS or len(key[0]) != len(key[1]):
            hit = False
        else:
            cb, ca = _lfilter_arrays(*key)
            hit = _native.lib().tac_lfilter_supported(cb, ca, len(key[1])) == _native.TAC_OK
        _lfilter_ok[key] = hit
    return hit


def host_coeffs(t):
    """The coefficients of a 1-D tensor as a tuple of Python floats (float32 converts exactly).  A device tensor is read back once
    per version of its contents (one host sync) and the tuple cached on the tensor object, like the tables of a window."""
    def build():
        return tuple(t.detach().to(torch.float64).tolist())
    return cached_on(t, '_tac_coef', (), build) if t.is_cuda else build()


def lfilter_rows(x, b, a, clamp, reverse=False):
    """``(…, L) -> (…, L)`` through ``tac_lfilter_f32``: one launch.  ``b`` / ``a`` are tuples of Python floats; ``reverse`` runs the
    filter from the end of each row (the adjoint).  ``x`` is read where it lies when its leading dims collapse into one positive
    row stride over unit-stride rows; it is copied otherwise."""
    global _lfilter_chunk_checked
    length = x.shape[-1]
    out = _empty(tuple(x.shape), device=x.device)
    if out.numel():
        h = _native.lib()
        if not _lfilter_chunk_checked:
            if h.tac_lfilter_chunk() != LFILTER_C:
                raise RuntimeError('libtac_amd.so filters %d samples per lane, _hip.LFILTER_C says %d'
                                   % (h.tac_lfilter_chunk(), LFILTER_C))
            _lfilter_chunk_checked = True
        rows = x.reshape(-1, length)
        if (length > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) <= 0):
            rows = rows.contiguous()
        cb, ca = _lfilter_arrays(b, a)
        _launch('tac_lfilter_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], length, rows.stride(0), cb, ca, len(a),
                int(bool(clamp)), int(bool(reverse)), _native.ptr(out))
    return out


# ----------------------------------------------------------------------------- sosfilt (csrc/sosfilt.hip)
#: sections per launch of ``tac_sosfilt_f32`` (SOS_MAX: order 16), its samples per tile (LF_TILE, shared with ``lfilter``) and the
#: cap of its persistent grid per CU (SOS_BLOCKS_PER_CU); checked against the library's own values at the first launch
SOSFILT_MAX_SECTIONS = 8
SOSFILT_TILE = LFILTER_TILE
SOSFILT_BLOCKS_PER_CU = 2

_sosfilt_ok = Bounded(256)
_sosfilt_checked = False


def _sosfilt_array(sos):
    flat = [v for row in sos for v in row]
    return (ctypes.c_double * len(flat))(*flat)


def host_sos(t):
    """The sections of an ``(S, 6)`` tensor as a tuple of tuples of Python floats; a device tensor is read back once per version
    of its contents, as ``host_coeffs`` reads a coefficient vector."""
    def build():
        return tuple(tuple(row) for row in t.detach().to(torch.float64).tolist())
    return cached_on(t, '_tac_coef', 'sos', build) if t.is_cuda else build()


def sosfilt_covers(sos):
    """True where ``tac_sosfilt_f32`` takes these sections (a tuple of ``(b0, b1, b2, a0, a1, a2)`` tuples, every ``a0`` finite and
    not zero already checked): at most ``SOSFILT_MAX_SECTIONS`` of them, each passing ``lfilter_covers``' rule."""
    hit = _sosfilt_ok.get(sos)
    if hit is None:
        hit = 1 <= len(sos) <= SOSFILT_MAX_SECTIONS and \
            _native.lib().tac_sosfilt_supported(_sosfilt_array(sos), len(sos)) == _native.TAC_OK
        _sosfilt_ok[sos] = hit
    return hit


def sosfilt_rows(x, sos, clamp, reverse=False):
    """``(…, L) -> (…, L)`` through ``tac_sosfilt_f32``: the whole cascade in one launch.  ``sos`` as for ``sosfilt_covers``;
    ``reverse`` runs the adjoint (the sections in reverse order, each from the end of the row).  ``x`` is read where it lies when
    its leading dims collapse into one positive row stride over unit-stride rows; it is copied otherwise."""
    global _sosfilt_checked
    length = x.shape[-1]
    out = _empty(tuple(x.shape), device=x.device)
    if out.numel():
        h = _native.lib()
        if not _sosfilt_checked:
            found = (h.tac_sosfilt_max_sections(), h.tac_sosfilt_tile(), h.tac_sosfilt_blocks_per_cu())
            if found != (SOSFILT_MAX_SECTIONS, SOSFILT_TILE, SOSFILT_BLOCKS_PER_CU):
                raise RuntimeError('libtac_amd.so reports (sections, tile, blocks per CU) = %r for sosfilt, _hip says %r'
                                   % (found, (SOSFILT_MAX_SECTIONS, SOSFILT_TILE, SOSFILT_BLOCKS_PER_CU)))
            _sosfilt_checked = True
        rows = x.reshape(-1, length)
        if (length > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) <= 0):
            rows = rows.contiguous()
        _launch('tac_sosfilt_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], length, rows.stride(0), _sosfilt_array(sos),
                len(sos), int(bool(clamp)), int(bool(reverse)), _native.ptr(out))
    return out


# ----------------------------------------------------------------------------- SoX effects (csrc/sox_effects.hip)
#: samples per tile of ``tac_overdrive_f32`` (lfilter's walk), of ``tac_phaser_f32`` and of the flanger's FIR path, the samples the
#: flanger's feedback path stages per chunk, the longest delays the kernels hold in the LDS and the caps of their persistent
#: grids per CU; checked against the library's own values at the first launch
OVERDRIVE_TILE = LFILTER_TILE
OVERDRIVE_BLOCKS_PER_CU = 2
PHASER_TILE = 4096
PHASER_MAX_DELAY = 1024
PHASER_SEQ_MAX_DELAY = 256
PHASER_BLOCKS_PER_CU = 1
FLANGER_TILE = 4096
FLANGER_CHUNK = 1024
FLANGER_MAX_BLOCK = 64
FLANGER_MAX_DELAY = 4096
FLANGER_BLOCKS_PER_CU = 4
FLANGER_FB_BLOCKS_PER_CU = 8

_sox_checked = False


def _sox_check():
    global _sox_checked
    if not _sox_checked:
        h = _native.lib()
        found = (h.tac_overdrive_tile(), h.tac_overdrive_blocks_per_cu(), h.tac_phaser_tile(), h.tac_phaser_max_delay(),
                 h.tac_phaser_seq_max_delay(), h.tac_phaser_blocks_per_cu(), h.tac_flanger_tile(), h.tac_flanger_chunk(),
                 h.tac_flanger_max_block(), h.tac_flanger_max_delay(), h.tac_flanger_blocks_per_cu(), h.tac_flanger_fb_blocks_per_cu())
        said = (OVERDRIVE_TILE, OVERDRIVE_BLOCKS_PER_CU, PHASER_TILE, PHASER_MAX_DELAY, PHASER_SEQ_MAX_DELAY, PHASER_BLOCKS_PER_CU,
                FLANGER_TILE, FLANGER_CHUNK, FLANGER_MAX_BLOCK, FLANGER_MAX_DELAY, FLANGER_BLOCKS_PER_CU, FLANGER_FB_BLOCKS_PER_CU)
        if found != said:
            raise RuntimeError('libtac_amd.so reports %r for the SoX effects\' tiles, delays and grids, _hip says %r' % (found, said))
        _sox_checked = True


def _sox_rows(x):
    """``x`` as ``(rows, length)`` read where it lies when its leading dims collapse into one positive row stride over unit-stride
    rows; copied otherwise (``lfilter_rows``' rule)"""
    length = x.shape[-1]
    rows = x.reshape(-1, length)
    if (length > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) <= 0):
        rows = rows.contiguous()
    return rows


def sox_table(host, device):
    """The device copy of a host LFO table (``_sox.phaser_plan`` / ``flanger_plan``), uploaded once per device and kept on the host
    tensor object"""
    return cached_on(host, '_tac_coef', ('sox', str(device)), lambda: host.to(device))


def overdrive_covers(g, c):
    return _native.lib().tac_overdrive_supported(float(g), float(c)) == _native.TAC_OK


def overdrive_rows(x, g, c):
    """``(…, L) -> (…, L)`` through ``tac_overdrive_f32``: one launch.  ``g``, ``c``: the linear gain and the offset."""
    out = _empty(tuple(x.shape), device=x.device)
    if out.numel():
        _sox_check()
        rows = _sox_rows(x)
        _launch('tac_overdrive_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], x.shape[-1], rows.stride(0), float(g), float(c),
                _native.ptr(out))
    return out


def phaser_covers(L, P):
    return _native.lib().tac_phaser_supported(int(L), int(P)) == _native.TAC_OK


def phaser_rows(x, table, L, gain_in, gain_out, decay, sequential=False):
    """``(…, L) -> (…, L)`` through ``tac_phaser_f32``: one launch.  ``table``: the int32 HOST tensor of the LFO period
    (``_sox.phaser_plan``).  ``sequential`` launches the one-lane-per-row ablation variant instead (``tac_phaser_seq_f32``)."""
    out = _empty(tuple(x.shape), device=x.device)
    if out.numel():
        _sox_check()
        rows = _sox_rows(x)
        mod = sox_table(table, x.device)
        _launch('tac_phaser_seq_f32' if sequential else 'tac_phaser_f32', x.device, (out,), _native.ptr(rows), rows.shape[0],
                x.shape[-1], rows.stride(0), _native.ptr(mod), int(table.numel()), int(L), float(gain_in), float(decay),
                float(gain_out), _native.ptr(out))
    return out


def flanger_covers(plan, channels):
    return _native.lib().tac_flanger_supported(int(plan.Lb), int(plan.P), int(plan.W), int(channels)) == _native.TAC_OK


def flanger_rows(x, plan):
    """``(…, C, L) -> (…, C, L)`` through ``tac_flanger_f32``: one launch, the FIR path where ``plan.fb == 0`` and the
    wave-per-row feedback path otherwise.  ``plan``: a ``_sox.FlangerPlan`` made for ``C`` channels."""
    out = _empty(tuple(x.shape), device=x.device)
    if out.numel():
        _sox_check()
        channels = x.shape[-2]
        rows = _sox_rows(x)
        lfo = sox_table(plan.lfo, x.device)
        phases = (ctypes.c_int32 * channels)(*plan.phases[:channels])
        _launch('tac_flanger_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], channels, x.shape[-1], rows.stride(0),
                _native.ptr(lfo), int(plan.P), phases, int(plan.Lb), int(plan.W), float(plan.fb), float(plan.in_gain),
                float(plan.delay_gain), int(bool(plan.quadratic)), _native.ptr(out))
    return out


# ----------------------------------------------------------------------------- loudness (csrc/loudness.hip)
#: samples of one row per tile of ``tac_loudness_f32`` (csrc/loudness.hip: LO_TILE), checked against the library's own value at the
#: first launch, and the shortest hop its bins take (LO_C: at most one bin edge in a lane's chunk)
LOUDNESS_TILE = 16384
LOUDNESS_MIN_STEP = 16
_loudness_tile_checked = False


def loudness_entries(x, stages, gate, step):
    """``(…, C, L) -> (…)`` through ``tac_loudness_f32``: one entry, two launches on the current stream.  ``stages``: the two
    ``(b, a)`` of the K-weighting as tuples of Python floats.  ``x`` is read where it lies when its leading dimensions collapse
    into one positive stride beside a positive channel stride over unit-stride rows; it is copied otherwise.  The float64 bins
    come from torch's allocator."""
    global _loudness_tile_checked
    lead, (channels, length) = tuple(x.shape[:-2]), x.shape[-2:]
    rows = x.unsqueeze(0) if x.dim() == 2 else x.reshape(-1, channels, length)
    entries = rows.shape[0]
    if (length > 1 and rows.stride(2) != 1) or (entries > 1 and rows.stride(0) <= 0) or (channels > 1 and rows.stride(1) <= 0):
        rows = rows.contiguous()
    h = _native.lib()
    if not _loudness_tile_checked:
        if h.tac_loudness_tile() != LOUDNESS_TILE:
            raise RuntimeError('libtac_amd.so walks %d samples per tile, _hip.LOUDNESS_TILE says %d' % (h.tac_loudness_tile(), LOUDNESS_TILE))
        _loudness_tile_checked = True
    need = int(h.tac_loudness_work_bytes(entries, channels, length, gate, step))
    if need <= 0:
        raise RuntimeError('tac_loudness_f32 does not take %d entries of %d channels and %d samples at gate %d, step %d'
                           % (entries, channels, length, gate, step))
    out = _empty((entries,), device=x.device)
    work = _empty((need // 8,), dtype=torch.float64, device=x.device)
    coeffs = (ctypes.c_double * 12)(*[v for b, a in stages for v in tuple(b) + tuple(a)])
    _launch('tac_loudness_f32', x.device, (out, work), _native.ptr(rows), entries, channels, length, rows.stride(0), rows.stride(1),
            gate, step, coeffs, _native.ptr(work), _native.ptr(out))
    return out.reshape(lead)


# ----------------------------------------------------------------------------- detect_pitch_frequency (csrc/pitch.hip)
#: the longest median window ``tac_pitch_smooth_i32`` takes (csrc/pitch.hip: PT_MAX_WIN), checked against the library at the first use
PITCH_MAX_WIN = 64
_pitch_win_checked = False


def pitch_plan(n_frames, frame, max_lag):
    """``(G, LDS bytes)``: the frames one workgroup of ``tac_pitch_lags_f32`` takes together and what it stages them in, or None
    where the ``frame + max_lag`` samples of a single frame are beyond its LDS plan"""
    global _pitch_win_checked
    h = _native.lib()
    if not _pitch_win_checked:
        if h.tac_pitch_max_win() != PITCH_MAX_WIN:
            raise RuntimeError('libtac_amd.so takes median windows up to %d, _hip.PITCH_MAX_WIN says %d' % (h.tac_pitch_max_win(), PITCH_MAX_WIN))
        _pitch_win_checked = True
    group, nbytes = ctypes.c_int32(0), ctypes.c_int32(0)
    if h.tac_pitch_plan(n_frames, frame, max_lag, ctypes.byref(group), ctypes.byref(nbytes)) != 0:
        return None
    return group.value, nbytes.value


def _pitch_rows(x):
    """``(…, time)`` as ``(n0, n1, time)`` read where it lies: a view when the leading dimensions collapse into two positive strides
    beside a positive time stride, a contiguous copy otherwise"""
    time = x.shape[-1]
    if x.dim() == 1:
        rows = x.reshape(1, 1, time)
    elif x.dim() == 2:
        rows = x.unsqueeze(0)
    else:
        rows = x.reshape(-1, x.shape[-2], time)          # (a view where the strides allow it, else torch copies)
    if any(st <= 0 for st, n in zip(rows.stride(), rows.shape) if n > 1):
        rows = rows.contiguous()
    return rows


def pitch_lags(x, frame, max_lag, lag_min):
    """``(…, time)`` float32 → int32 ``(…, ceil(time / frame))``: the first launch of csrc/pitch.hip alone, ``tac_pitch_lags_f32``"""
    rows = _pitch_rows(x)
    n0, n1, time = rows.shape
    n_frames = -(-time // frame)
    lags = _empty((n0 * n1, n_frames), dtype=torch.int32, device=x.device)
    _launch('tac_pitch_lags_f32', x.device, (lags,), _native.ptr(rows), n0, n1, time, rows.stride(0), rows.stride(1), rows.stride(2),
            frame, max_lag, lag_min, _native.ptr(lags))
    return lags.reshape(tuple(x.shape[:-1]) + (n_frames,))


def pitch_smooth(lags, win_length, sample_rate):
    """int32 ``(…, n_frames)`` → float32 ``(…, n_frames + (win_length - 1) // 2 - win_length + 1)``: the second launch alone,
    ``tac_pitch_smooth_i32`` — the lower median over ``win_length`` lags behind copies of the first, then ``sample_rate / lag``"""
    n_frames = lags.shape[-1]
    rows = lags.reshape(-1, n_frames).contiguous()
    n_out = n_frames + (win_length - 1) // 2 - win_length + 1
    out = _empty((rows.shape[0], max(n_out, 0)), device=lags.device)
    _launch('tac_pitch_smooth_i32', lags.device, (out,), _native.ptr(rows), rows.shape[0], n_frames, win_length, sample_rate,
            _native.ptr(out))
    return out.reshape(tuple(lags.shape[:-1]) + (n_out,))


def pitch_frequency(x, sample_rate, frame, max_lag, lag_min, win_length):
    """``(…, time)`` float32 → float32 ``(…, n_out)`` through ``tac_pitch_frequency_f32``: one entry, two launches on the current
    stream.  The int32 lags between them come from torch's allocator."""
    rows = _pitch_rows(x)
    n0, n1, time = rows.shape
    n_frames = -(-time // frame)
    n_out = n_frames + (win_length - 1) // 2 - win_length + 1
    lags = _empty((n0 * n1, n_frames), dtype=torch.int32, device=x.device)
    out = _empty((n0 * n1, n_out), device=x.device)
    _launch('tac_pitch_frequency_f32', x.device, (out, lags), _native.ptr(rows), n0, n1, time, rows.stride(0), rows.stride(1),
            rows.stride(2), sample_rate, frame, max_lag, lag_min, win_length, _native.ptr(lags), _native.ptr(out))
    return out.reshape(tuple(x.shape[:-1]) + (n_out,))


# ----------------------------------------------------------------------------- vad / vad_start (csrc/vad.hip)
_vad_tables = Bounded(16)


def vad_limits(p):
    """``(bins per lane, parts, LDS bytes, longest search, workgroups per CU)`` of the measuring launch for the ``_vad.Plan`` ``p``,
    or None where ``tac_vad_plan`` declines its bins (more than 2048 spectrum bins, 512 cepstrum bins or 144 KiB of LDS)"""
    out = [ctypes.c_int32(0) for _ in range(5)]
    rc = _native.lib().tac_vad_plan(p.dft, p.s0, p.s1, p.c0, p.c1, *[ctypes.byref(v) for v in out])
    if rc == _native.TAC_E_UNSUPPORTED:
        return None
    _native.check(rc, 'tac_vad_plan')
    return tuple(v.value for v in out)


def vad_max_search():
    """the longest backward search (measures) ``tac_vad_decide_f32`` takes"""
    out = ctypes.c_int32(0)
    _native.lib().tac_vad_plan(16, 1, 2, 0, 1, None, None, None, ctypes.byref(out), None)
    return out.value


def vad_covers_dft(dft):
    """the transform lengths ``tac_spectrogram_f32`` has an FFT kernel for, among the powers of two ``vad`` asks for"""
    return fft_kernel_size(dft) or big_fft_size(dft)


def _vad_device_tables(p, device):
    """(measurement window ``2 / sqrt(mlen) hann(mlen)``, cepstral window ``2 / sqrt(nb) hann(nb)``, ``(cos, sin)(2 pi i / (dft / 2))`` as ``(dft / 2, 2)``) on
    ``device`` as float32: the windows from torch's float32 Hann values, the table from float64 on the host, each rounded once;
    cached per geometry and device"""
    key = (p.mlen, p.dft, p.s0, p.s1, device)
    hit = _vad_tables.get(key)
    if hit is None:
        with torch.inference_mode(False):
            nb, half = p.s1 - p.s0, p.dft // 2
            win = torch.hann_window(p.mlen, dtype=torch.float32) * (2.0 / math.sqrt(p.mlen))
            win2 = torch.hann_window(nb, dtype=torch.float32) * (2.0 / math.sqrt(nb))
            angle = torch.arange(half, dtype=torch.float64) * (2.0 * math.pi / half)
            tab = torch.stack([torch.cos(angle), torch.sin(angle)], -1)
            tab[half // 4, 0] = tab[3 * half // 4, 0] = tab[half // 2, 1] = 0.0     # (the zeros of both, exactly)
            hit = (win.to(device), win2.to(device), tab.to(torch.float32).to(device))
        _vad_tables[key] = hit
    return hit


def _vad_decay(p):
    """the host array ``tac_vad_measures_f32`` takes: smooth, up and down with their complements, formed in float64"""
    return (ctypes.c_float * 6)(p.smooth, 1.0 - p.smooth, p.up, 1.0 - p.up, p.down, 1.0 - p.down)


def vad_magnitudes(x, p):
    """``(…, time)`` float32 → the frame-major ``(rows, T, dft / 2 + 1)`` rows ``|X_t|`` of the measurement windows, one
    ``tac_spectrogram_f32`` launch.  torch's framing puts a window of ``mlen`` in the middle of ``dft`` samples, the definition at
    their front: the rows are copied once behind ``(dft - mlen) // 2`` zeros (and in front of the rest), which also makes any
    layout dense — data movement by torch, like the padding of every centred STFT here."""
    time = x.shape[-1]
    left = (p.dft - p.mlen) // 2
    rows = torch.nn.functional.pad(x.reshape(-1, time), (left, p.dft - p.mlen - left))
    win = _vad_device_tables(p, x.device)[0]
    spec = spectrogram(rows, win, p.dft, p.period, p.mlen, False, 'constant', False, True, 1.0, False, 1.0, 1e-10)
    return spec.transpose(-2, -1)


def vad_measures_of(mag, p):
    """the frame-major ``(rows, T, dft / 2 + 1)`` rows of ``vad_magnitudes`` → float32 ``(rows, T)``: launch 2 alone,
    ``tac_vad_measures_f32``"""
    rows, n_frames = mag.shape[0], mag.shape[1]
    _, win2, tab = _vad_device_tables(p, mag.device)
    meas = _empty((rows, n_frames), device=mag.device)
    _launch('tac_vad_measures_f32', mag.device, (meas,), _native.ptr(mag), rows, n_frames, p.dft, p.s0, p.s1, p.c0, p.c1,
            min(p.boot_max, 2 ** 31 - 1), _vad_decay(p), p.nra, _native.ptr(win2), _native.ptr(tab), _native.ptr(meas))
    return meas


def vad_measures(x, p):
    """``(…, time)`` float32 → float32 ``(…, T)``: launches 1 and 2 of ``vad``, ``tac_spectrogram_f32`` and ``tac_vad_measures_f32``"""
    n_frames = (x.shape[-1] - p.mlen) // p.period + 1 if x.shape[-1] >= p.mlen else 0
    rows = math.prod(x.shape[:-1])
    if not (rows and n_frames):
        return _empty(tuple(x.shape[:-1]) + (n_frames,), device=x.device)
    return vad_measures_of(vad_magnitudes(x, p), p).reshape(tuple(x.shape[:-1]) + (n_frames,))


def vad_decide(meas, p, time):
    """float32 ``(groups, channels, T)`` → ``(start int64 (groups,), triggered bool (groups,))``: launch 3 alone, ``tac_vad_decide_f32``"""
    groups, channels, n_frames = meas.shape
    meas = meas.contiguous()
    start = _empty((groups,), dtype=torch.int64, device=meas.device)
    triggered = torch.empty((groups,), dtype=torch.bool, device=meas.device)
    _launch('tac_vad_decide_f32', meas.device, (start,), _native.ptr(meas), groups, channels, n_frames, time, p.n, min(p.gap, p.n), p.period,
            p.pre, p.keep, p.level, p.trig, 1.0 - p.trig, _native.ptr(start), _native.ptr(triggered))
    return start, triggered


def vad_start(x, p, groups, channels):
    """``(…, time)`` float32 of ``groups * channels`` rows → ``(start int64 (groups,), triggered bool (groups,))``: one
    ``tac_spectrogram_f32`` launch and one ``tac_vad_start_f32`` entry of two, all on the current stream; nothing waits for the host.
    The float32 measures between the launches come from torch's allocator."""
    time = x.shape[-1]
    n_frames = (time - p.mlen) // p.period + 1 if time >= p.mlen else 0
    if n_frames == 0:            # no measurement window fits: never triggered, nothing to launch
        return (torch.full((groups,), max(time - p.keep, 0), dtype=torch.int64, device=x.device),
                torch.zeros((groups,), dtype=torch.bool, device=x.device))
    mag = vad_magnitudes(x, p)
    _, win2, tab = _vad_device_tables(p, x.device)
    meas = _empty((groups * channels, n_frames), device=x.device)
    start = _empty((groups,), dtype=torch.int64, device=x.device)
    triggered = torch.empty((groups,), dtype=torch.bool, device=x.device)
    _launch('tac_vad_start_f32', x.device, (start, meas), _native.ptr(mag), groups, channels, n_frames, time, p.dft, p.s0, p.s1, p.c0, p.c1,
            min(p.boot_max, 2 ** 31 - 1), _vad_decay(p), p.nra, _native.ptr(win2), _native.ptr(tab), p.n, min(p.gap, p.n), p.period, p.pre, p.keep, p.level, p.trig,
            1.0 - p.trig, _native.ptr(meas), _native.ptr(start), _native.ptr(triggered))
    return start, triggered


# ----------------------------------------------------------------------------- simulate_rir_ism (csrc/rir.hip)
_rir_limits = None               # (constants of the library: asked for once)


def rir_limits():
    """``(shortest tile, most bands, longest delay filter, highest order)`` of ``tac_rir_ism_f32``"""
    global _rir_limits
    if _rir_limits is None:
        out = [ctypes.c_int32(0) for _ in range(4)]
        _native.check(_native.lib().tac_rir_limits(*[ctypes.byref(v) for v in out]), 'tac_rir_limits')
        _rir_limits = tuple(v.value for v in out)
    return _rir_limits


def rir_tile(rows, length, n_band):
    """``(tile, longest tile)``: the samples of a row a wave owns in a launch of ``rows`` rows of ``length`` samples and ``n_band`` bands, as
    ``tac_rir_ism_f32`` chooses it, and the longest it takes at that many bands"""
    out = [ctypes.c_int32(0) for _ in range(2)]
    _native.check(_native.lib().tac_rir_tile(rows, length, n_band, *[ctypes.byref(v) for v in out]), 'tac_rir_tile')
    return tuple(v.value for v in out)


def rir_ism(room, source, mic_array, absorption, max_order, start, length, delay_filter_length, sound_speed, sample_rate, tile=0):
    """contiguous float32 ``(B, D)``, ``(B, D)``, ``(B, M, D)``, ``(B or 1, n_band, 2 D)`` → float32 ``(B, n_band, M, length)``: samples
    ``[start, start + length)`` of the raw responses, ONE launch of ``tac_rir_ism_f32`` that writes every element.  ``tile``: the samples of
    a row a wave owns (a power of two, ``rir_tile``'s range), 0 for the launch's own choice; the bits do not depend on it."""
    B, D = room.shape
    M, nb = mic_array.shape[1], absorption.shape[1]
    img = _rir.images(max_order, D, room.device)
    tab = _rir.tap_table(delay_filter_length, room.device)
    out = _empty((B, nb, M, length), device=room.device)
    _launch('tac_rir_ism_f32', room.device, (out,), _native.ptr(room), _native.ptr(source), _native.ptr(mic_array), _native.ptr(absorption),
            nb * 2 * D if absorption.shape[0] > 1 else 0, _native.ptr(img), _native.ptr(tab), B, M, D, nb, img.shape[0], max_order, start,
            length, delay_filter_length, float(sound_speed), float(sample_rate), tile, _native.ptr(out))
    return out


def rir_ism_span(room, source, mic_array, max_order, delay_filter_length, sound_speed, sample_rate):
    """→ int64 scalar on the device, ``max(delay_i) + L - P`` over the batch: one launch of ``tac_rir_span_f32``, nothing read on the host"""
    B, D = room.shape
    img = _rir.shell(max_order, D, room.device)              # (the farthest image is in the two outermost shells)
    out = _empty((), dtype=torch.int64, device=room.device)
    _launch('tac_rir_span_f32', room.device, (out,), _native.ptr(room), _native.ptr(source), _native.ptr(mic_array), _native.ptr(img), B,
            mic_array.shape[1], D, img.shape[0], delay_filter_length, float(sound_speed), float(sample_rate), _native.ptr(out))
    return out


# ----------------------------------------------------------------------------- psd / mvdr_weights_souden / apply_beamforming (csrc/beamform.hip)
#: how the last calls got their spectrograms: read where they lay (frame-major views, channel slices, any 8-byte aligned pairs whose
#: bins run faster than their frames), or copied into the frame-major layout first
beamform_layout = {'in_place': 0, 'copied': 0}


def _bf_spec(spec):
    """``(…, C, F, T, 2)`` float32 → ``(B, C, F, T, 2)`` for the kernels: a view where the leading dimensions collapse into one
    stride, the pairs are contiguous and 8-byte aligned, every stride is even and positive and the bins run faster than the
    frames; a frame-major copy otherwise"""
    tail = tuple(spec.shape[-4:])
    x5 = None
    if spec.stride(-1) == 1:
        if spec.dim() == 4:
            x5 = spec.unsqueeze(0)
        elif spec.dim() == 5:
            x5 = spec
        else:
            try:
                x5 = spec.view((-1,) + tail)
            except RuntimeError:
                x5 = None
    if x5 is not None:
        ok = x5.data_ptr() % 8 == 0 and all(st > 0 and st % 2 == 0 for st, n in zip(x5.stride()[:4], x5.shape[:4]) if n > 1)
        if ok and tail[1] > 1 and tail[2] > 1 and x5.stride(2) > x5.stride(3):
            ok = False                                                  # time runs faster than the bins: lanes along f would not coalesce
        if not ok:
            x5 = None
    if x5 is None:
        beamform_layout['copied'] += 1                                  # (clone: ``contiguous()`` would keep a misaligned frame-major tensor)
        return spec.reshape((-1,) + tail).transpose(2, 3).clone(memory_format=torch.contiguous_format).transpose(2, 3)
    beamform_layout['in_place'] += 1
    return x5


def _bf_mask(mask, F, T):
    """``(…, F, T)`` float32 → ``(B, F, T)`` read where it lies (a copy where the leading dimensions do not collapse)"""
    m = mask.reshape(-1, F, T)
    if any(st <= 0 for st, n in zip(m.stride(), m.shape) if n > 1):
        m = m.contiguous()
    return m


def _bf_mask_args(m):
    return (None, 0, 0, 0) if m is None else (_native.ptr(m), m.stride(0), m.stride(1), m.stride(2))


def psd_chunks(frames):
    """the pieces ``tac_psd_plan`` cuts ``frames`` into: a function of the frame count alone"""
    chunks = ctypes.c_int32(0)
    _native.check(_native.lib().tac_psd_plan(frames, None, ctypes.byref(chunks)), 'tac_psd_plan')
    return chunks.value


def _bf_scratch(n_psd, chunks, C, G, device):
    """the pieces of the PSD launch: float32 sums and float64 mask sums, all of it written by the launch"""
    return _empty((n_psd, chunks, C * C, G), device=device), _empty((n_psd, chunks, G), dtype=torch.float64, device=device)


def psd(spec, mask_a=None, mask_b=None, complement=False, normalize=True, eps=1e-10):
    """``(…, C, F, T, 2)`` float32 → ``(…, F, C, C, 2)`` through ``tac_psd_f32``: one entry of two launches.  With ``mask_b`` or
    ``complement`` (the second mask is ``1 - mask_a``, formed in the kernel) BOTH PSDs come from one pass over ``spec`` and a pair
    is returned."""
    lead, (C, F, T) = tuple(spec.shape[:-4]), spec.shape[-4:-1]
    x = _bf_spec(spec)
    B = x.shape[0]
    n_psd = 2 if (mask_b is not None or complement) else 1
    ma = None if mask_a is None else _bf_mask(mask_a, F, T)
    mb = None if mask_b is None else _bf_mask(mask_b, F, T)
    chunks = psd_chunks(T)
    part, msum = _bf_scratch(n_psd, chunks, C, B * F, spec.device)
    out = [_empty((B * F, C, C, 2), device=spec.device) for _ in range(n_psd)]
    _launch('tac_psd_f32', spec.device, (part, msum, *out), _native.ptr(x), B, C, F, T, x.stride(0), x.stride(1), x.stride(2),
            x.stride(3), *_bf_mask_args(ma), *_bf_mask_args(mb), n_psd, 1 if complement else 0, 1 if normalize else 0, float(eps),
            chunks, _native.ptr(part), _native.ptr(msum), _native.ptr(out[0]), _native.ptr(out[1]) if n_psd == 2 else None)
    out = [o.reshape(lead + (F, C, C, 2)) for o in out]
    return tuple(out) if n_psd == 2 else out[0]


def _bf_ref(ref_vector, lead, C):
    """the reference vector for the kernels: ``(pointer, batch stride, tensor kept alive)``"""
    if ref_vector is None:
        return None, 0, None
    u = ref_vector.to(torch.float32)
    if u.dim() == 1:
        u = u.contiguous()
        return _native.ptr(u), 0, u
    u = u.reshape(-1, C).contiguous()
    return _native.ptr(u), C, u


def mvdr_weights_souden(psd_s, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps):
    """two ``(…, F, C, C, 2)`` float32 → ``(…, F, C, 2)`` through ``tac_mvdr_weights_souden_f32``: one launch, float64 on chip"""
    lead, F, C = tuple(psd_s.shape[:-4]), psd_s.shape[-4], psd_s.shape[-2]
    s, n = psd_s.reshape(-1, F, C, C, 2).contiguous(), psd_n.reshape(-1, F, C, C, 2).contiguous()
    B = s.shape[0]
    ref_ptr, ref_stride, keep = _bf_ref(ref_vector, lead, C)
    out = _empty((B * F, C, 2), device=psd_s.device)
    _launch('tac_mvdr_weights_souden_f32', psd_s.device, (out,), _native.ptr(s), _native.ptr(n), B, F, C, ref_ptr, ref_stride,
            ref_channel, 1 if diagonal_loading else 0, float(diag_eps), float(eps), _native.ptr(out))
    return out.reshape(lead + (F, C, 2))


def _bf_out(lead, B, F, T, device):
    """the frame-major output: ``(B, T, F, 2)`` storage, and its logical ``(…, F, T, 2)`` view"""
    store = _empty((B, T, F, 2), device=device)
    return store, store.view(lead + (T, F, 2)).transpose(-3, -2)


def apply_beamforming(weights, spec):
    """``(…, F, C, 2)`` and ``(…, C, F, T, 2)`` float32 → the frame-major view ``(…, F, T, 2)`` through ``tac_apply_beamforming_f32``"""
    lead, (C, F, T) = tuple(spec.shape[:-4]), spec.shape[-4:-1]
    x = _bf_spec(spec)
    B = x.shape[0]
    w = weights.reshape(B * F, C, 2).contiguous()
    store, out = _bf_out(lead, B, F, T, spec.device)
    _launch('tac_apply_beamforming_f32', spec.device, (store,), _native.ptr(w), _native.ptr(x), B, C, F, T, x.stride(0), x.stride(1),
            x.stride(2), x.stride(3), _native.ptr(store), T * F * 2, 2, F * 2)
    return out


def mvdr_souden(spec, mask_s, mask_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps, psd_eps):
    """``MVDR`` at ``solution='ref_channel'`` through ``tac_mvdr_souden_f32``: ONE entry of three launches on the current stream —
    both normalised PSDs from one pass over ``spec`` (``mask_n`` None: ``1 - mask_s`` formed in the kernel), the float64 solve,
    the weights applied.  Returns ``(frame-major view (…, F, T, 2), weights (…, F, C, 2))``."""
    lead, (C, F, T) = tuple(spec.shape[:-4]), spec.shape[-4:-1]
    x = _bf_spec(spec)
    B = x.shape[0]
    ms = _bf_mask(mask_s, F, T)
    mn = None if mask_n is None else _bf_mask(mask_n, F, T)
    chunks = psd_chunks(T)
    part, msum = _bf_scratch(2, chunks, C, B * F, spec.device)
    ref_ptr, ref_stride, keep = _bf_ref(ref_vector, lead, C)
    w = _empty((B * F, C, 2), device=spec.device)
    store, out = _bf_out(lead, B, F, T, spec.device)
    _launch('tac_mvdr_souden_f32', spec.device, (part, msum, w, store), _native.ptr(x), B, C, F, T, x.stride(0), x.stride(1),
            x.stride(2), x.stride(3), *_bf_mask_args(ms), *_bf_mask_args(mn), float(psd_eps), ref_ptr, ref_stride, ref_channel,
            1 if diagonal_loading else 0, float(diag_eps), float(eps), chunks, _native.ptr(part), _native.ptr(msum), _native.ptr(w),
            _native.ptr(store), T * F * 2, 2, F * 2)
    return out, w.reshape(lead + (F, C, 2))


# ----------------------------------------------------------------------------- rtf_evd / rtf_power / mvdr_weights_rtf (csrc/beamform.hip)
def rtf_power_max_iter():
    """the most ``n_iter`` ``tac_rtf_power_f32`` takes"""
    return _native.lib().tac_rtf_power_max_iter()


def rtf_evd(psd_s):
    """``(…, F, C, C, 2)`` float32 → ``(…, F, C, 2)`` through ``tac_rtf_evd_f32``: one launch, cyclic Jacobi in float64 on chip; unit
    norm, the component of largest modulus real and positive"""
    lead, F, C = tuple(psd_s.shape[:-4]), psd_s.shape[-4], psd_s.shape[-2]
    s = psd_s.reshape(-1, F, C, C, 2).contiguous()
    B = s.shape[0]
    out = _empty((B * F, C, 2), device=psd_s.device)
    _launch('tac_rtf_evd_f32', psd_s.device, (out,), _native.ptr(s), B, F, C, _native.ptr(out))
    return out.reshape(lead + (F, C, 2))


def rtf_power(psd_s, psd_n, ref_vector, ref_channel, n_iter, diagonal_loading, diag_eps):
    """two ``(…, F, C, C, 2)`` float32 → ``(…, F, C, 2)`` through ``tac_rtf_power_f32``: one launch, the solve and every product in
    float64 on chip"""
    lead, F, C = tuple(psd_s.shape[:-4]), psd_s.shape[-4], psd_s.shape[-2]
    s, n = psd_s.reshape(-1, F, C, C, 2).contiguous(), psd_n.reshape(-1, F, C, C, 2).contiguous()
    B = s.shape[0]
    ref_ptr, ref_stride, keep = _bf_ref(ref_vector, lead, C)
    out = _empty((B * F, C, 2), device=psd_s.device)
    _launch('tac_rtf_power_f32', psd_s.device, (out,), _native.ptr(s), _native.ptr(n), B, F, C, ref_ptr, ref_stride, ref_channel,
            n_iter, 1 if diagonal_loading else 0, float(diag_eps), _native.ptr(out))
    return out.reshape(lead + (F, C, 2))


def mvdr_weights_rtf(rtf, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps):
    """``(…, F, C, 2)`` and ``(…, F, C, C, 2)`` float32 → ``(…, F, C, 2)`` through ``tac_mvdr_weights_rtf_f32``: one launch.
    ``ref_channel`` -1 without a vector: no reference scaling."""
    lead, F, C = tuple(psd_n.shape[:-4]), psd_n.shape[-4], psd_n.shape[-2]
    d, n = rtf.reshape(-1, F, C, 2).contiguous(), psd_n.reshape(-1, F, C, C, 2).contiguous()
    B = n.shape[0]
    ref_ptr, ref_stride, keep = _bf_ref(ref_vector, lead, C)
    out = _empty((B * F, C, 2), device=psd_n.device)
    _launch('tac_mvdr_weights_rtf_f32', psd_n.device, (out,), _native.ptr(d), _native.ptr(n), B, F, C, ref_ptr, ref_stride,
            ref_channel, 1 if diagonal_loading else 0, float(diag_eps), float(eps), _native.ptr(out))
    return out.reshape(lead + (F, C, 2))


def rtf_mvdr(spec, rtf, psd_n, ref_vector, ref_channel, diagonal_loading, diag_eps, eps):
    """``RTFMVDR`` through ``tac_rtf_mvdr_f32``: ONE entry of two launches on the current stream — the RTF weights, the weights
    applied.  Returns ``(frame-major view (…, F, T, 2), weights (…, F, C, 2))``."""
    lead, (C, F, T) = tuple(spec.shape[:-4]), spec.shape[-4:-1]
    x = _bf_spec(spec)
    B = x.shape[0]
    d, n = rtf.reshape(B, F, C, 2).contiguous(), psd_n.reshape(B, F, C, C, 2).contiguous()
    ref_ptr, ref_stride, keep = _bf_ref(ref_vector, lead, C)
    w = _empty((B * F, C, 2), device=spec.device)
    store, out = _bf_out(lead, B, F, T, spec.device)
    _launch('tac_rtf_mvdr_f32', spec.device, (w, store), _native.ptr(x), B, C, F, T, x.stride(0), x.stride(1), x.stride(2),
            x.stride(3), _native.ptr(d), _native.ptr(n), ref_ptr, ref_stride, ref_channel, 1 if diagonal_loading else 0,
            float(diag_eps), float(eps), _native.ptr(w), _native.ptr(store), T * F * 2, 2, F * 2)
    return out, w.reshape(lead + (F, C, 2))


# ----------------------------------------------------------------------------- rnnt_loss (csrc/rnnt.hip)
def rnnt_max_targets():
    """the most ``U + 1`` the lattice launch takes: a lane per column of one workgroup"""
    return _native.lib().tac_rnnt_max_targets()


def rnnt_reason(logits):
    """why the launches of csrc/rnnt.hip do not take these float32 ``(B, T, U + 1, V)`` logits as they lie, or None"""
    B, T, U1, V = logits.shape
    if V > 1 and logits.stride(3) != 1:
        return 'a class axis without unit stride'
    if any(st <= 0 for st, n in zip(logits.stride()[:3], logits.shape[:3]) if n > 1):
        return 'expanded or non-positive strides'
    if U1 > rnnt_max_targets():
        return 'a target axis of %d (the kernel takes up to %d)' % (U1, rnnt_max_targets())
    if B * T * U1 >= 2 ** 31:
        return '%d lattice cells (the kernel takes fewer than 2^31)' % (B * T * U1)
    return None


def _rnnt_ints(t, device):
    return t if (t.dtype == torch.int32 and t.is_contiguous() and t.device == device) else \
        t.to(device=device, dtype=torch.int32).contiguous()


def _rnnt_geometry(logits):
    B, T, U1, V = logits.shape
    return (_native.ptr(logits), B, T, U1, V, logits.stride(0), logits.stride(1), logits.stride(2))


def rnnt_forward(logits, targets, logit_lengths, target_lengths, blank, fused):
    """``(costs (B,), alphas, betas, denominators (B, T, U + 1))`` of float32 logits ``rnnt_reason`` passes: two launches — the
    denominators with the two log-probabilities of every lattice cell, then alpha and beta together.  Nothing of the size of the
    logits is allocated."""
    B, T, U1, V = logits.shape
    dev = logits.device
    targets, tl, ul = _rnnt_ints(targets, dev), _rnnt_ints(logit_lengths, dev), _rnnt_ints(target_lengths, dev)
    denom, lp_blank, lp_label, alphas, betas = (_empty((B, T, U1), device=dev) for _ in range(5))
    costs = _empty((B,), device=dev)
    _launch('tac_rnnt_rows_f32', dev, (denom, lp_blank, lp_label), *_rnnt_geometry(logits), _native.ptr(targets), _native.ptr(tl),
            _native.ptr(ul), blank, 1 if fused else 0, _native.ptr(denom), _native.ptr(lp_blank), _native.ptr(lp_label),
            _native.ptr(alphas), _native.ptr(betas))
    _launch('tac_rnnt_lattice_f32', dev, (alphas, betas, costs), B, T, U1, V, _native.ptr(targets), _native.ptr(tl), _native.ptr(ul),
            _native.ptr(lp_blank), _native.ptr(lp_label), _native.ptr(alphas), _native.ptr(betas), _native.ptr(costs))
    return costs, alphas, betas, denom


def rnnt_grad(logits, targets, logit_lengths, target_lengths, alphas, betas, denom, costs, grad_costs, blank, clamp, fused):
    """the gradient with respect to the logits, contiguous ``(B, T, U + 1, V)``: one launch, one read of the logits, one write"""
    dev = logits.device
    targets, tl, ul = _rnnt_ints(targets, dev), _rnnt_ints(logit_lengths, dev), _rnnt_ints(target_lengths, dev)
    alphas, betas, denom, costs, grad_costs = (t.contiguous() for t in (alphas, betas, denom, costs, grad_costs))
    out = _empty(tuple(logits.shape), device=dev)
    _launch('tac_rnnt_grad_f32', dev, (out,), *_rnnt_geometry(logits), _native.ptr(targets), _native.ptr(tl), _native.ptr(ul),
            _native.ptr(alphas), _native.ptr(betas), _native.ptr(denom), _native.ptr(costs), _native.ptr(grad_costs), blank,
            float(clamp), 1 if fused else 0, _native.ptr(out))
    return out


# ----------------------------------------------------------------------------- forced_align (csrc/align.hip)
def align_max_targets():
    """the most ``L + 1`` the launch takes: the pairs of states of one workgroup"""
    return _native.lib().tac_forced_align_max_targets()


def align_reason(log_probs, targets):
    """why the launch of csrc/align.hip does not take these float32 ``(B, T, C)`` log-probabilities as they lie, or None"""
    if any(st <= 0 for st, n in zip(log_probs.stride(), log_probs.shape) if n > 1):
        return 'expanded or non-positive strides'
    if targets.shape[1] + 1 > align_max_targets():
        return 'a target axis of %d + 1 (the kernel takes up to %d)' % (targets.shape[1], align_max_targets())
    if max(log_probs.shape) >= 2 ** 30:
        return 'an axis of 2^30 or more'
    return None


def forced_align(log_probs, targets, input_lengths, target_lengths, blank):
    """``(paths (B, T) in the dtype of targets, scores (B, T))`` of float32 log-probabilities ``align_reason`` passes: ONE launch.
    The lengths may be None (``T`` and ``L`` in every entry)."""
    B, T, C = log_probs.shape
    L = targets.shape[1]
    dev = log_probs.device
    targets = targets if (targets.is_contiguous() and targets.device == dev) else targets.to(dev).contiguous()
    il = None if input_lengths is None else _rnnt_ints(input_lengths, dev)
    tl = None if target_lengths is None else _rnnt_ints(target_lengths, dev)
    paths = _empty((B, T), dtype=targets.dtype, device=dev)
    scores = _empty((B, T), device=dev)
    need = _native.lib().tac_forced_align_workspace(B, T, L + 1)
    work = torch.empty((need // 8,), dtype=torch.int64, device=dev) if need else None      # (not an output: plain)
    _launch('tac_forced_align_f32', dev, (paths, scores), _native.ptr(log_probs), B, T, C, log_probs.stride(0), log_probs.stride(1),
            log_probs.stride(2), _native.ptr(targets) if L else None, L, 1 if targets.dtype == torch.int64 else 0,
            None if il is None else _native.ptr(il), None if tl is None else _native.ptr(tl), blank,
            None if work is None else _native.ptr(work), _native.ptr(paths), _native.ptr(scores))
    return paths, scores


# ----------------------------------------------------------------------------- fftconvolve (csrc/fftconvolve.hip)
#: the transform lengths of the partitioned route and the most partitions ``tac_spectral_mac_f32`` takes
FFTCONV_SIZES = (2048, 4096, 8192)
FFTCONV_MAX_PARTS = 64
#: longest ONE shared kernel that takes ``tac_polyphase_f32`` (one phase, step 1) instead of the transforms.  256 is the unmeasured
#: default; ``tools/bench_fftconvolve.py`` measures the crossover
M_DIRECT = 256


def fftconvolve_n_fft(m):
    """The default transform length for a kernel of ``m`` taps: the smallest with at most 8 partitions, else 8192 (unmeasured
    rule; ``tac_fftconvolve_default_n_fft`` is the same rule in the library)."""
    for n in FFTCONV_SIZES[:-1]:
        if -(-m // (n // 2)) <= 8:
            return n
    return FFTCONV_SIZES[-1]


def fftconvolve_covers(length, m, n_fft=0):
    """True where the partitioned route takes a kernel of ``m`` taps at ``n_fft`` (0: the default rule)."""
    n = n_fft or fftconvolve_n_fft(m)
    if n not in FFTCONV_SIZES or -(-m // (n // 2)) > FFTCONV_MAX_PARTS:
        return False
    return _native.lib().tac_fftconvolve_supported(length, m, n) == _native.TAC_OK


def _conv_kernel_rows(y):
    m = int(y.shape[-1])
    rows = y.detach().reshape(-1, m)
    return rows if rows.is_contiguous() else rows.contiguous()


def _conv_spectra(y, n_fft, reverse):
    """``H``: float32 ``(h_rows, P, n_fft / 2 + 1, 2)`` of ``tac_fftconvolve_spectra_f32``, cached on ``y``."""
    def build():
        rows = _conv_kernel_rows(y)
        h_rows, m = int(rows.shape[0]), int(rows.shape[1])
        need = int(_native.lib().tac_fftconvolve_spectra_workspace(h_rows, m, n_fft))
        if need < 0:
            _native.check(need, 'tac_fftconvolve_spectra_workspace')
        work = torch.empty(need // 4, dtype=torch.float32, device=y.device)      # scratch: written before it is read
        out = _empty((h_rows, -(-m // (n_fft // 2)), n_fft // 2 + 1, 2), device=y.device)
        _launch('tac_fftconvolve_spectra_f32', y.device, (out,), _native.ptr(rows), h_rows, m, rows.stride(0), n_fft,
                int(bool(reverse)), _native.ptr(work), need, _native.ptr(out))
        return out
    return cached_on(y, '_tac_conv', ('spectra', n_fft, bool(reverse)), build)


def _conv_direct_bank(y, reverse, offset):
    """the kernel from its end (from its start for the gradient) and the {offset, run} table of ``tac_fftconvolve_direct_f32``"""
    def build():
        row = _conv_kernel_rows(y)[0]
        bank = (row.clone() if reverse else row.flip(0)).contiguous()
        table = torch.tensor([offset - (int(row.shape[0]) - 1), int(row.shape[0])], dtype=torch.int32).to(y.device)
        return bank, table
    return cached_on(y, '_tac_conv', ('direct', bool(reverse), offset), build)


def _conv_row_map(y, lead):
    """int32 map from the rows of the broadcast leading shape ``lead`` to the rows of ``y`` (None: one shared kernel)"""
    h_rows = 1
    for n in y.shape[:-1]:
        h_rows *= int(n)
    if h_rows == 1:
        return None

    def build():
        idx = torch.arange(h_rows, dtype=torch.int32).reshape(tuple(y.shape[:-1])).expand(lead)
        return idx.reshape(-1).contiguous().to(y.device)
    return cached_on(y, '_tac_conv', ('map', tuple(lead)), build)


def fftconvolve_route(m, shared, n_fft=0):
    """'direct' or the transform length the call takes"""
    if not n_fft and shared and m <= M_DIRECT:
        return 'direct'
    return n_fft or fftconvolve_n_fft(m)


def fftconvolve(x, y, n_fft=0, reverse=False, offset=0, out_len=None):
    """``(*, L)``, ``(*, M)`` float32 -> ``(*, out_len)``: samples ``offset .. offset + out_len`` of the full convolution of
    ``x`` with ``y`` (with ``y`` read from its end when ``reverse``: the gradient w.r.t. ``x``), the leading dimensions
    broadcast.  ``x`` is read where it lies when its leading dims collapse into one positive row stride over unit-stride rows;
    it is copied otherwise.  ``n_fft`` 0: the default rule, and the direct route for one shared kernel of at most ``M_DIRECT``
    taps."""
    length, m = int(x.shape[-1]), int(y.shape[-1])
    lead = tuple(torch.broadcast_shapes(tuple(x.shape[:-1]), tuple(y.shape[:-1])))
    out_len = length + m - 1 - offset if out_len is None else int(out_len)
    out = _empty(lead + (out_len,), device=x.device)
    if not out.numel():
        return out
    if tuple(x.shape[:-1]) != lead:
        x = x.expand(lead + (length,))
    rows = x.reshape(-1, length)
    if (length > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) < length):
        rows = rows.contiguous()
    n_rows = int(rows.shape[0])
    hrow = _conv_row_map(y, lead)
    route = fftconvolve_route(m, hrow is None, n_fft)
    with _native.on_device(x.device):
        if route == 'direct':
            bank, table = _conv_direct_bank(y, reverse, offset)
            _launch('tac_fftconvolve_direct_f32', x.device, (out,), _native.ptr(rows), n_rows, length, rows.stride(0),
                    _native.ptr(bank), _native.ptr(table), m, offset, out_len, _native.ptr(out))
            return out
        spectra = _conv_spectra(y, route, reverse)
        need = int(_native.lib().tac_fftconvolve_workspace(n_rows, length, m, route, offset, out_len))
        if need < 0:
            _native.check(need, 'tac_fftconvolve_workspace')
        work = torch.empty(need // 4, dtype=torch.float32, device=x.device)      # scratch: every area is written before it is read
        _launch('tac_fftconvolve_f32', x.device, (out,), _native.ptr(rows), n_rows, length, rows.stride(0), _native.ptr(spectra),
                None if hrow is None else _native.ptr(hrow), int(spectra.shape[0]), m, route, 0, offset, out_len, _native.ptr(work),
                need, _native.ptr(out), out_len)
    return out


def last_route():
    """``tac_last_route()`` of the calling thread"""
    return _native.lib().tac_last_route().decode()


# ----------------------------------------------------------------------------- kaldi fbank (csrc/kaldi_fbank.hip)
#: what ``tac_kaldi_fbank_f32`` covers: the transform lengths of ``WaveFft<N/2, 16>`` with several frames per wave, and the bands
KALDI_SIZES = (256, 512, 1024)
KALDI_MAX_BINS = 128
_KALDI_FLAGS = dict(snip_edges=1, remove_dc_offset=2, raw_energy=4, use_energy=8, htk_compat=16, use_log_fbank=32, use_power=64)

_kaldi_tables = Bounded(64)


def _kaldi_device_tables(p, w, n, device):
    """(window float32 (W,), packed weights, int32 table (3, bins)) on ``device``: built in float64 on the host, rounded once,
    cached per argument set and device.  ``SpectrogramParams`` have no bank: (window, None, None, 0)."""
    bins = getattr(p, 'num_mel_bins', None)
    band = (bins, p.sample_frequency, p.low_freq, p.high_freq) if bins is not None else None
    key = (p.window_type, p.blackman_coeff, w, n, band, device)
    hit = _kaldi_tables.get(key)
    if hit is None:
        with torch.inference_mode(False):
            window = _kaldi.window64(p.window_type, w, p.blackman_coeff).to(torch.float32)
            if bins is None:
                hit = (window.to(device), None, None, 0)
            else:
                bank = _kaldi.mel_bank64(bins, n, p.sample_frequency, p.low_freq, p.high_freq).to(torch.float32)
                weights, table = _kaldi.packed_runs(bank)
                hit = (window.to(device), weights.to(device), table.contiguous().to(device), int(weights.numel()))
        _kaldi_tables[key] = hit
    return hit


def _kaldi_rows(x):
    """``x`` (…, L) as (rows, L) for the kaldi launches: read where it lies when its leading dims collapse into one positive row
    stride over unit-stride rows, copied otherwise"""
    length = int(x.shape[-1])
    rows = x.reshape(-1, length)
    if (length > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) <= 0):
        rows = rows.contiguous()
    return rows


def _kaldi_flags(p):
    return sum(bit for name, bit in _KALDI_FLAGS.items() if getattr(p, name, False))


_kaldi_dct_tables = Bounded(64)


def _kaldi_dct_table(p, device):
    """``_kaldi.mfcc_table64`` rounded to float32 once, (num_mel_bins, num_ceps) row-major on ``device``: the lanes of a frame
    read consecutive words of one row"""
    key = (p.num_mel_bins, p.num_ceps, p.cepstral_lifter, p.htk_compat and not p.use_energy, device)
    hit = _kaldi_dct_tables.get(key)
    if hit is None:
        with torch.inference_mode(False):
            hit = _kaldi.mfcc_table64(p).to(torch.float32).contiguous().to(device)
        _kaldi_dct_tables[key] = hit
    return hit


def kaldi_mfcc_table_limit(p, w, n, device):
    """``tac_kaldi_mfcc_table_limit``: the largest ``num_mel_bins * num_ceps`` the launch has LDS for beside this call's
    window and packed bank — asked before launching, so that a larger table is routed, not refused"""
    w_total = _kaldi_device_tables(p, w, n, device)[3]
    return int(_native.lib().tac_kaldi_mfcc_table_limit(n, p.num_mel_bins, w_total))


def kaldi_mfcc(x, p, w, s, n, m):
    """``(…, L)`` float32 -> ``(…, m, num_ceps)`` through ``tac_kaldi_mfcc_f32``: one launch (``subtract_mean`` is the
    caller's); rows as ``kaldi_fbank`` takes them."""
    window, weights, table, w_total = _kaldi_device_tables(p, w, n, x.device)
    dct = _kaldi_dct_table(p, x.device)
    out = _empty(tuple(x.shape[:-1]) + (m, p.num_ceps), device=x.device)
    if not out.numel():
        return out
    rows = _kaldi_rows(x)
    _launch('tac_kaldi_mfcc_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], int(x.shape[-1]), rows.stride(0),
            _native.ptr(window), _native.ptr(weights), _native.ptr(table), _native.ptr(dct), n, w, s, p.num_mel_bins, w_total,
            p.num_ceps, _kaldi_flags(p), p.preemphasis_coefficient, p.energy_floor, _native.ptr(out))
    return out


def kaldi_spectrogram(x, p, w, s, n, m):
    """``(…, L)`` float32 -> ``(…, m, n / 2 + 1)`` through ``tac_kaldi_spectrogram_f32``: one launch (``subtract_mean`` is the
    caller's); rows as ``kaldi_fbank`` takes them."""
    window = _kaldi_device_tables(p, w, n, x.device)[0]
    out = _empty(tuple(x.shape[:-1]) + (m, n // 2 + 1), device=x.device)
    if not out.numel():
        return out
    rows = _kaldi_rows(x)
    _launch('tac_kaldi_spectrogram_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], int(x.shape[-1]), rows.stride(0),
            _native.ptr(window), n, w, s, _kaldi_flags(p), p.preemphasis_coefficient, p.energy_floor, _native.ptr(out))
    return out


def kaldi_fbank(x, p, w, s, n, m):
    """``(…, L)`` float32 -> ``(…, m, bins [+ 1])`` through ``tac_kaldi_fbank_f32``: one launch (``subtract_mean`` is the
    caller's).  ``x`` is read where it lies when its leading dims collapse into one positive row stride over unit-stride rows;
    it is copied otherwise."""
    window, weights, table, w_total = _kaldi_device_tables(p, w, n, x.device)
    length = int(x.shape[-1])
    cols = p.num_mel_bins + (1 if p.use_energy else 0)
    out = _empty(tuple(x.shape[:-1]) + (m, cols), device=x.device)
    if not out.numel():
        return out
    rows = _kaldi_rows(x)
    _launch('tac_kaldi_fbank_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], length, rows.stride(0), _native.ptr(window),
            _native.ptr(weights), _native.ptr(table), n, w, s, p.num_mel_bins, w_total, _kaldi_flags(p), p.preemphasis_coefficient,
            p.energy_floor, _native.ptr(out))
    return out


# ----------------------------------------------------------------------------- sliding CMN and deltas (csrc/cmn_deltas.hip)
#: the pad modes of ``tac_deltas_f32`` in the header's numbering
DELTAS_MODES = {'replicate': 0, 'constant': 1, 'reflect': 2, 'circular': 3}


def _positive_strides(x):
    return all(st > 0 for st, k in zip(x.stride(), x.shape) if k > 1)


def sliding_cmn_covers(x):
    """True where ``tac_sliding_cmn_f32`` reads ``x`` (…, T, F) where it lies: positive strides on every axis longer than one"""
    return x.dim() >= 2 and _positive_strides(x)


def sliding_cmn_chunk(rows, n_frames, n_feats, cmn_window, min_cmn_window):
    """frames one thread of ``tac_sliding_cmn_f32`` walks at this shape (the library's own choice)"""
    return int(_native.lib().tac_sliding_cmn_chunk(rows, n_frames, n_feats, cmn_window, min_cmn_window))


def _rows3(x):
    """``x`` (…, A, B) as (rows, A, B): a view where the leading dims collapse into one stride, a copy otherwise"""
    rows = x.reshape((-1,) + tuple(x.shape[-2:]))
    return rows if _positive_strides(rows) else rows.contiguous()


def sliding_cmn_rows(x, cmn_window, min_cmn_window, center, norm_vars, adjoint=False):
    """``(…, T, F) -> (…, T, F)``, dense, through ``tac_sliding_cmn_f32``: one launch on ``x`` where it lies (any positive
    strides; the leading dims are copied only when no single row stride expresses them).  ``adjoint``: ``x`` is the gradient of
    the output and the result the gradient of the input (``norm_vars`` off)."""
    out = _empty(tuple(x.shape), device=x.device)
    if out.numel():
        rows = _rows3(x)
        _launch('tac_sliding_cmn_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], rows.shape[1], rows.shape[2],
                rows.stride(0), rows.stride(1), rows.stride(2), cmn_window, min_cmn_window, int(bool(center)), int(bool(norm_vars)),
                int(bool(adjoint)), _native.ptr(out))
    return out


def deltas_supported(n_frames, win_length, mode, adjoint=False):
    """True where ``tac_deltas_f32`` takes these arguments: the library's own answer (``tac_deltas_supported``: the widest
    window, and for the adjoint the two modes whose gradient it has), so the cap is stated in csrc/cmn_deltas.hip alone"""
    return _native.lib().tac_deltas_supported(n_frames, win_length, DELTAS_MODES[mode], int(bool(adjoint))) == _native.TAC_OK


def deltas_covers(x, win_length, mode, adjoint=False):
    """True where ``tac_deltas_f32`` takes this call on ``x`` where it lies: ``deltas_supported`` and positive strides"""
    return deltas_supported(int(x.shape[-1]), win_length, mode, adjoint) and _positive_strides(x)


def deltas_rows(x, win_length, mode, adjoint=False):
    """``(…, F, T) -> (…, F, T)``, dense, through ``tac_deltas_f32``: one launch on ``x`` where it lies.  ``adjoint``: ``x`` is the
    gradient of the output and the result the gradient of the input."""
    out = _empty(tuple(x.shape), device=x.device)
    if out.numel():
        rows = _rows3(x)
        _launch('tac_deltas_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], rows.shape[1], rows.shape[2], rows.stride(0),
                rows.stride(1), rows.stride(2), win_length, DELTAS_MODES[mode], int(bool(adjoint)), _native.ptr(out))
    return out


# ----------------------------------------------------------------------------- SpecAugment's masks (csrc/specaug.hip)
def mask_spans_supported(k_a, k_b):
    """True where ``tac_mask_spans_f32`` takes ``k_a + k_b`` spans: the library's own answer (``tac_mask_spans_supported``), so the
    cap is stated in csrc/specaug.hip and include/tac_amd.h alone"""
    return _native.lib().tac_mask_spans_supported(k_a, k_b) == _native.TAC_OK


def mask_spans_covers(x, k_a, k_b):
    """True where ``tac_mask_spans_f32`` takes this call on ``x`` (…, A, B) where it lies: ``mask_spans_supported`` and positive
    strides on every axis longer than one"""
    return x.dim() >= 2 and mask_spans_supported(k_a, k_b) and _positive_strides(x)


def mask_spans_rows(x, spans, k_a, value_t=None, value=0.0):
    """``(…, A, B) -> (…, A, B)``, dense, through ``tac_mask_spans_f32``: every span of ``spans`` (int32 ``(R, k, 2)`` on ``x``'s
    device, ``R`` 1 or the number of rows, the first ``k_a`` along A) filled in one launch on ``x`` where it lies.  The fill is
    the 0-dim float32 device tensor ``value_t`` where given (read by the kernel: no host sync), else ``value``."""
    out = _empty(tuple(x.shape), device=x.device)
    if out.numel():
        rows = _rows3(x)
        k = int(spans.shape[-2])
        if k and (spans.dtype != torch.int32 or not spans.is_contiguous() or spans.device != x.device
                  or spans.shape[0] not in (1, rows.shape[0])):
            raise ValueError('mask_spans: spans must be a contiguous int32 (1 or %d, k, 2) tensor on %s' % (rows.shape[0], x.device))
        if value_t is not None and (value_t.dtype != torch.float32 or value_t.numel() != 1 or value_t.device != x.device):
            raise ValueError('mask_spans: the fill tensor must be one float32 element on %s' % x.device)
        _launch('tac_mask_spans_f32', x.device, (out,), _native.ptr(rows), rows.shape[0], rows.shape[1], rows.shape[2], rows.stride(0),
                rows.stride(1), rows.stride(2), _native.ptr(spans) if k else None, int(spans.shape[0]) if k else 1, k_a, k - k_a,
                None if value_t is None else _native.ptr(value_t), float(value), _native.ptr(out))
    return out


# ----------------------------------------------------------------------------- add_noise (csrc/add_noise.hip)
#: samples of one row per unit of ``tac_add_noise_f32`` (csrc/add_noise.hip: AN_TILE)
ADD_NOISE_TILE = 4096


def _add_noise_rows_of(lead):
    rows = 1
    for n in lead:
        rows *= int(n)
    return rows


def _add_noise_groups(x, lead):
    """``x`` (…, L) broadcast to ``lead + (L,)`` and read where it lies: its time stride and the ``(size, stride)`` pairs of the
    leading dimensions longer than one (a stride of 0 where ``x`` is broadcast)"""
    length = int(x.shape[-1])
    view = x.expand(tuple(lead) + (length,))
    return (view.stride(-1) if length > 1 else 1), [(int(n), int(s)) for n, s in zip(view.shape[:-1], view.stride()[:-1]) if n > 1]


def _collapse(dims):
    """the one stride that walks ``dims`` in row-major order, or None"""
    for (_, s_out), (n_in, s_in) in zip(dims[:-1], dims[1:]):
        if s_out != s_in * n_in:
            return None
    return dims[-1][1] if dims else 0


def _add_noise_plan(lead, operands):
    """How ``tac_add_noise_f32`` walks the rows of these (…, L) operands: ``(rows_inner, [(outer stride, row stride, time stride)])`` with
    row ``o * rows_inner + i`` of an operand at ``o * outer + i * row`` — the leading dimensions split at ONE place, the same for every
    operand, into two runs of one stride each (dense batches, padded rows, every second row, one noise row for all rows, one noise
    row per batch entry for its channels) — or the reason (a string) why the kernels do not read them where they lie"""
    found = [_add_noise_groups(x, lead) for x in operands]
    if any(st <= 0 for st, _ in found):
        return 'non-positive time strides'
    rows, length = _add_noise_rows_of(lead), int(operands[0].shape[-1])
    if rows and length and int(_native.lib().tac_add_noise_work_bytes(rows, length)) <= 0:
        return 'more tiles of %d samples than one launch takes' % ADD_NOISE_TILE
    count = len(found[0][1])
    for split in range(count + 1):
        strides = [(_collapse(dims[:split]), _collapse(dims[split:]), st) for st, dims in found]
        if all(so is not None and sr is not None for so, sr, _ in strides):
            inner = 1
            for n, _ in found[0][1][split:]:
                inner *= n
            return inner, strides
    return 'leading dimensions that do not collapse to two strides'


def add_noise_reason(lead, *operands):
    """None where ``tac_add_noise_f32`` / ``tac_add_noise_grad_f32`` read these (…, L) operands where they lie, else the reason"""
    plan = _add_noise_plan(lead, operands)
    return plan if isinstance(plan, str) else None


def add_noise_covers(lead, *operands):
    return add_noise_reason(lead, *operands) is None


def _add_noise_table(t, lead, dtype=None):
    """``t`` broadcast to ``lead`` as the kernel's table: ``(tensor, entries)`` with one entry where ``t`` holds one, else one per row"""
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if t.numel() == 1:
        return t.reshape(1), 1
    flat = t.expand(tuple(lead)).reshape(-1)
    return (flat if flat.is_contiguous() else flat.contiguous()), flat.shape[0]


def _add_noise_args(operands, snr, lengths, lead):
    """the arguments of either entry from the operands (``grad_out`` first where there is one) up to the scratch, and the tensors
    that have to outlive the call"""
    length = int(operands[0].shape[-1])
    rows = _add_noise_rows_of(lead)
    inner, strides = _add_noise_plan(lead, operands)
    snr_t, snr_rows = _add_noise_table(snr, lead, torch.float32)
    if lengths is None:
        len_t, len_rows, len_i64 = None, 1, 0
    else:
        if lengths.dtype not in (torch.int32, torch.int64):       # t < lengths  <=>  t < ceil(lengths)
            lengths = (lengths.ceil() if lengths.is_floating_point() else lengths).clamp(-1, length).to(torch.int64)
        len_t, len_rows = _add_noise_table(lengths, lead)
        len_i64 = int(len_t.dtype == torch.int64)
    work = torch.empty((int(_native.lib().tac_add_noise_work_bytes(rows, length)) // 8,), dtype=torch.float64, device=operands[0].device)
    args = []
    for x, (so, sr, st) in zip(operands, strides):
        args += [_native.ptr(x), so, sr, st]
    args += [rows, inner, length, _native.ptr(snr_t), snr_rows, None if len_t is None else _native.ptr(len_t), len_rows, len_i64,
             _native.ptr(work)]
    return args, (snr_t, len_t, work)


def add_noise_rows(waveform, noise, snr, lengths, lead):
    """``waveform``, ``noise`` (…, L) float32, ``snr`` and ``lengths`` (…), all broadcast to the leading shape ``lead``: ``lead + (L,)``,
    dense, through ``tac_add_noise_f32`` — one entry, three launches on the current stream, the operands read where they lie
    (``add_noise_covers``), ``snr`` and ``lengths`` read on the device.  The float64 scratch comes from torch's allocator."""
    out = _empty(tuple(lead) + (int(waveform.shape[-1]),), device=waveform.device)
    if out.numel():
        args, keep = _add_noise_args((waveform, noise), snr, lengths, lead)
        _launch('tac_add_noise_f32', waveform.device, (out,), *args, _native.ptr(out))
    return out


def add_noise_grad_rows(grad_out, waveform, noise, snr, lengths, lead, needs):
    """The gradients of ``add_noise_rows`` w.r.t. (waveform, noise, snr) where ``needs`` asks for them, each over the broadcast
    shape (``lead + (L,)``, ``lead``): one ``tac_add_noise_grad_f32`` entry — the same three launches in adjoint mode, both tensor
    gradients written in one pass."""
    shape = tuple(lead) + (int(waveform.shape[-1]),)
    dev = waveform.device
    gw = _empty(shape, device=dev) if needs[0] else None
    gn = _empty(shape, device=dev) if needs[1] else None
    gs = _empty(tuple(lead), device=dev) if needs[2] else None
    if grad_out.numel() and any(needs):
        args, keep = _add_noise_args((grad_out, waveform, noise), snr, lengths, lead)
        _launch('tac_add_noise_grad_f32', dev, (gw, gn, gs), *args, None if gw is None else _native.ptr(gw),
                None if gn is None else _native.ptr(gn), None if gs is None else _native.ptr(gs))
    return gw, gn, gs


# ----------------------------------------------------------------------------- complex pairs
def is_dense(x):
    """True when x's elements tile one gap-free block of memory (in any dim order)."""
    if x.is_contiguous():
        return True
    dims = sorted((st, n) for st, n in zip(x.stride(), x.shape) if n > 1)
    expect = 1
    for st, n in dims:
        if st != expect:
            return False
        expect *= n
    return True


def _pairs(z):
    """Dense view of a ``(*, 2)`` tensor whose storage order the elementwise kernels can walk pair by pair."""
    if z.stride(-1) != 1 or not is_dense(z) or any(s % 2 for s, n in zip(z.stride()[:-1], z.shape[:-1]) if n > 1):
        z = z.contiguous()
    return z


def _pair_output(z):
    return _empty_strided(z.shape[:-1], tuple(s // 2 for s in z.stride()[:-1]), device=z.device)


def complex_norm(z, power):
    z = _pairs(z)
    out = _pair_output(z)
    n = out.numel()
    if n:
        _launch('tac_complex_norm_f32', z.device, (out,), _native.ptr(z), n, float(power), _native.ptr(out))
    return out


def angle(z):
    z = _pairs(z)
    phase = _pair_output(z)
    if phase.numel():
        _launch('tac_magphase_f32', z.device, (phase,), _native.ptr(z), phase.numel(), 1.0, None, _native.ptr(phase))
    return phase


def magphase(z, power):
    z = _pairs(z)
    mag, phase = _pair_output(z), _pair_output(z)
    if phase.numel():
        _launch('tac_magphase_f32', z.device, (mag, phase), _native.ptr(z), phase.numel(), float(power), _native.ptr(mag),
                _native.ptr(phase))
    return mag, phase


_PV_GRID_CACHE = Bounded(64)


def _phase_vocoder_grid(n_frames, rate, device, dtype):
    """Source-frame indices and interpolation weights of every output frame, evaluated exactly as the reference's CPU
    path does (functional.py:233-247: ``torch.arange(0, T, rate)`` in the default dtype, ``% 1``, ``.long()``); which
    frames get paired depends on that rounding, so it is computed with the same host ops and cached."""
    key = (int(n_frames), float(rate), str(device), dtype, torch.get_default_dtype())
    hit = _PV_GRID_CACHE.get(key)
    if hit is None:
        steps = torch.arange(0, n_frames, rate)
        hit = (steps.long().to(torch.int32).to(device), (steps + 1).long().to(torch.int32).to(device),
               torch.remainder(steps, torch.tensor(1., dtype=steps.dtype)).to(dtype).to(device))
        _PV_GRID_CACHE[key] = hit
    return hit


def phase_vocoder_out_frames(n_frames, rate):
    return int(torch.arange(0, n_frames, rate).numel())


def phase_vocoder(spec, rate, phase_advance):
    """float32 or float64 (the reference's own test runs this op in float64, tests/test_functional.py:69-116)."""
    dtype = spec.dtype
    n_freqs, n_frames = spec.shape[-3], spec.shape[-2]
    pa = phase_advance.reshape(-1).to(dtype).contiguous()
    lead = tuple(spec.shape[:-3])
    idx0, idx1, alpha = _phase_vocoder_grid(n_frames, rate, spec.device, dtype)
    n_out = idx0.numel()
    if spec.stride(-1) != 1:
        spec = spec.contiguous()
    rows = spec.reshape((-1,) + tuple(spec.shape[-3:]))          # a view whenever the leading dims collapse
    if any(st % 2 for st in rows.stride()[:-1]) or rows.data_ptr() % (2 * rows.element_size()):
        rows = rows.contiguous()                                 # (re, im) pairs are fetched as one aligned access
    out = _empty(lead + (n_out, n_freqs, 2), dtype=dtype, device=spec.device)
    if out.numel() and n_frames:
        name = 'tac_phase_vocoder_f64' if dtype == torch.float64 else 'tac_phase_vocoder_f32'
        _launch(name, spec.device, (out,), _native.ptr(rows), rows.shape[0], n_freqs, n_frames,
                rows.stride(0) if rows.shape[0] > 1 else 0, rows.stride(1), rows.stride(2), _native.ptr(pa), _native.ptr(idx0),
                _native.ptr(idx1), _native.ptr(alpha), n_out, _native.ptr(out))
    return out.transpose(-3, -2)


def phase_vocoder_backward(spec, rate, grad_out):
    """Gradient of the float32 ``phase_vocoder`` with respect to ``spec`` (*, F, T, 2): ``grad_out`` (*, F, n_out, 2) in any layout;
    the result is frame-major like the forward's output."""
    n_freqs, n_frames = spec.shape[-3], spec.shape[-2]
    lead = tuple(spec.shape[:-3])
    idx0, idx1, alpha = _phase_vocoder_grid(n_frames, rate, spec.device, torch.float32)
    n_out = idx0.numel()
    if spec.stride(-1) != 1:
        spec = spec.contiguous()
    rows = spec.reshape((-1,) + tuple(spec.shape[-3:]))
    if any(st % 2 for st in rows.stride()[:-1]) or rows.data_ptr() % (2 * rows.element_size()):
        rows = rows.contiguous()
    go = torch.empty(lead + (n_out, n_freqs, 2), dtype=torch.float32, device=spec.device)      # frame-major, dense
    go.transpose(-3, -2).copy_(grad_out)
    gs = torch.zeros(lead + (n_frames, n_freqs, 2), dtype=torch.float32, device=spec.device)    # the kernel accumulates into it
    if go.numel() and n_frames:
        _launch('tac_phase_vocoder_backward_f32', spec.device, (), _native.ptr(rows), rows.shape[0], n_freqs, n_frames,
                rows.stride(0) if rows.shape[0] > 1 else 0, rows.stride(1), rows.stride(2), _native.ptr(idx0), _native.ptr(idx1),
                _native.ptr(alpha), n_out, _native.ptr(go), _native.ptr(gs))
    return gs.transpose(-3, -2)


# ----------------------------------------------------------------------------- stretch on magnitudes (csrc/stretch.hip)
_PV_BOUNDS_CACHE = Bounded(64)


def _stretch_bounds(n_frames, rate, device):
    """``bounds[t]`` = number of output frames whose first source frame lies below ``t`` (t = 0 .. n_frames), from the same host
    evaluation of the grid as ``_phase_vocoder_grid``: the first source frames are non-decreasing, so the outputs that read frame
    ``t`` are ``[bounds[t - 1], bounds[t + 1])`` — the ranges the gather of ``tac_stretch_norm_backward_f32`` walks."""
    key = (int(n_frames), float(rate), str(device), torch.get_default_dtype())
    hit = _PV_BOUNDS_CACHE.get(key)
    if hit is None:
        first = torch.arange(0, n_frames, rate).long()
        hit = torch.searchsorted(first, torch.arange(n_frames + 1)).to(torch.int32).to(device)
        _PV_BOUNDS_CACHE[key] = hit
    return hit


def finite_table(t):
    """Whether every element of a constant table (``TimeStretch.phase_advance``) is finite: read back once per buffer version
    (one host synchronisation) and cached on the tensor like the tables derived from windows and filterbanks."""
    return cached_on(t, '_tac_finite', (), lambda: bool(torch.isfinite(t).all()))


def _magnitude_rows(mag):
    """``mag`` (*, F, T) as frame-major rows [R][T][F] with contiguous bins — a view of what the spectrogram kernels return."""
    n_freqs, n_frames = mag.shape[-2], mag.shape[-1]
    fm = mag.transpose(-2, -1)
    if fm.stride(-1) != 1 and n_freqs > 1:
        fm = fm.contiguous()
    rows = fm.reshape(-1, n_frames, n_freqs)
    if (rows.stride(2) != 1 and n_freqs > 1) or (n_frames > 1 and rows.stride(1) < n_freqs) or (rows.shape[0] > 1 and rows.stride(0) < 0):
        rows = rows.contiguous()
    return rows


def _stretch_strides(rows):
    return (rows.stride(0) if rows.shape[0] > 1 else 0), (rows.stride(1) if rows.shape[1] > 1 else rows.shape[2])


def stretch_norm(mag, rate, power, db, ref, amin):
    """``complex_norm(phase_vocoder(X, rate), power)`` [-> dB] from ``mag = |X|`` (*, F, T): one streaming kernel plus the
    near-empty launch that restores the reference's handling of non-finite values.  Result (*, F, n_out), frame-major."""
    n_freqs, n_frames = mag.shape[-2], mag.shape[-1]
    lead = tuple(mag.shape[:-2])
    idx0, _, alpha = _phase_vocoder_grid(n_frames, rate, mag.device, torch.float32)
    n_out = idx0.numel()
    out = _empty(lead + (n_out, n_freqs), device=mag.device)
    if out.numel():
        rows = _magnitude_rows(mag)
        stride_r, stride_t = _stretch_strides(rows)
        flags = torch.empty(rows.shape[0], dtype=torch.int32, device=mag.device)       # the kernels' workspace: one word per row
        _launch('tac_stretch_norm_f32', mag.device, (out,), _native.ptr(rows), rows.shape[0], n_freqs, n_frames, stride_r, stride_t,
                _native.ptr(idx0), _native.ptr(alpha), n_out, float(power), 1 if db else 0, float(ref), float(amin), _native.ptr(out),
                _native.ptr(flags))
    return out.transpose(-2, -1)


def stretch_mel(mag, fb, rate, power, db, ref, amin):
    """``stretch_norm`` -> ``apply_filterbank`` [-> dB] in one launch when the bank packs into the one-frame-per-wave lane layout;
    any other bank (dense, custom, too few / too many bands): the rows form, then the filterbank kernels."""
    n_freqs, n_frames = mag.shape[-2], mag.shape[-1]
    if fb.dim() != 2 or fb.shape[0] != n_freqs:
        raise RuntimeError('apply_filterbank: size mismatch, spectrogram has %d bins, filterbank %s' % (n_freqs, tuple(fb.shape)))
    fb = fb if fb.is_contiguous() else fb.contiguous()
    lead = tuple(mag.shape[:-2])
    n_mels = fb.shape[1]
    idx0, _, alpha = _phase_vocoder_grid(n_frames, rate, mag.device, torch.float32)
    n_out = idx0.numel()
    pack = _melbank_pack(fb, 0) if (MEL_PATH != 'mfma' and n_out and n_mels and mag.numel()) else None
    if pack is not None:
        wpack, desc, info = pack
        rows = _magnitude_rows(mag)
        stride_r, stride_t = _stretch_strides(rows)
        out = _empty(lead + (n_out, n_mels), device=mag.device)
        flags = torch.empty(rows.shape[0], dtype=torch.int32, device=mag.device)
        rc = _launch('tac_stretch_mel_f32', mag.device, (out,), _native.ptr(rows), rows.shape[0], n_freqs, n_frames, stride_r, stride_t,
                     _native.ptr(idx0), _native.ptr(alpha), n_out, float(power), _native.ptr(wpack), _native.ptr(desc),
                     ctypes.cast(info, ctypes.c_void_p), n_mels, 1 if db else 0, float(ref), float(amin), _native.ptr(out),
                     _native.ptr(flags), accept=_DECLINED)
        if rc != _native.TAC_E_UNSUPPORTED:
            return out.transpose(-2, -1)
    spec = stretch_norm(mag, rate, power, False, 1.0, 1e-7)
    return apply_filterbank(spec, fb, db=(ref, amin) if db else None)


def stretch_norm_backward(mag, rate, power, grad_out):
    """Gradient of ``stretch_norm`` (without dB) with respect to ``mag``: a gather per source frame over the cached output ranges."""
    n_freqs, n_frames = mag.shape[-2], mag.shape[-1]
    lead = tuple(mag.shape[:-2])
    idx0, _, alpha = _phase_vocoder_grid(n_frames, rate, mag.device, torch.float32)
    n_out = idx0.numel()
    gm = _empty(lead + (n_frames, n_freqs), device=mag.device)
    if gm.numel():
        bounds = _stretch_bounds(n_frames, rate, mag.device)
        rows = _magnitude_rows(mag)
        stride_r, stride_t = _stretch_strides(rows)
        go = torch.empty(lead + (n_out, n_freqs), dtype=torch.float32, device=mag.device)          # frame-major, dense
        go.transpose(-2, -1).copy_(grad_out)
        _launch('tac_stretch_norm_backward_f32', mag.device, (gm,), _native.ptr(rows), rows.shape[0], n_freqs, n_frames, stride_r,
                stride_t, _native.ptr(idx0), _native.ptr(alpha), _native.ptr(bounds), n_out, float(power), _native.ptr(go),
                _native.ptr(gm))
    return gm.transpose(-2, -1)


# ----------------------------------------------------------------------------- elementwise
def _unary(x, name, *params):
    x = x if is_dense(x) else x.contiguous()
    out = _empty_like(x)
    if x.numel():
        _launch(name, x.device, (out,), _native.ptr(x), x.numel(), *params, _native.ptr(out))
    return out


def amplitude_to_db(x, ref, amin):
    return _unary(x, 'tac_amplitude_to_db_f32', float(ref), float(amin))


def db_to_amplitude(x, ref):
    return _unary(x, 'tac_db_to_amplitude_f32', float(ref))


_mulaw_consts = {}


def _mulaw_tables(device):
    key = str(device)
    hit = _mulaw_consts.get(key)
    if hit is None:
        from . import _mulaw_tables as tab
        thr = torch.tensor(list(tab.THR256_POS) + list(tab.THR256_NEG), dtype=torch.int32, device=device)
        lut = torch.tensor(list(tab.LUT256_BITS), dtype=torch.int64).to(torch.int32).view(torch.float32)
        hit = (thr, len(tab.THR256_POS), len(tab.THR256_NEG), tab.ZERO_CODE_256, lut.to(device))
        with _lock:
            _mulaw_consts[key] = hit
    return hit


def mu_law_encoding(x, n_quantize):
    x = x if x.is_contiguous() else x.contiguous()
    out = _empty(x.shape, dtype=torch.int64, device=x.device)
    if x.numel():
        if n_quantize == 256:
            thr, n_pos, n_neg, zero, _ = _mulaw_tables(x.device)
            thr_ptr = _native.ptr(thr)
        else:
            thr_ptr, n_pos, n_neg, zero = None, 0, 0, 0
        _launch('tac_mulaw_encode_f32_i64', x.device, (out,), _native.ptr(x), x.numel(), n_quantize, thr_ptr, n_pos, n_neg, zero,
                _native.ptr(out))
    return out


def mu_law_decoding_int(codes, n_quantize):
    """int64 codes -> float32 (reference functional.py:348-354 with the default dtype)."""
    codes = codes.to(torch.int64).contiguous()
    out = _empty(codes.shape, device=codes.device)
    if codes.numel():
        lut_ptr = _native.ptr(_mulaw_tables(codes.device)[4]) if n_quantize == 256 else None
        _launch('tac_mulaw_decode_i64_f32', codes.device, (out,), _native.ptr(codes), codes.numel(), n_quantize, lut_ptr,
                _native.ptr(out))
    return out


def mu_law_decoding_float(codes, n_quantize):
    """float32 codes -> float32: integral codes in [0, 256) with n_quantize == 256 come from the reference's own
    table (bit-exact, what reference tests/test_functional.py:182-193 bit-compares), everything else from the
    closed form."""
    lut = _mulaw_tables(codes.device)[4] if n_quantize == 256 else None
    return _unary(codes, 'tac_mulaw_decode_f32_f32', n_quantize, None if lut is None else _native.ptr(lut))


def mu_law_encoding_f64(x, n_quantize):
    """float64 waveform -> int64 codes, the formula in double (reference functional.py:329-335 on double input)."""
    x = x if x.is_contiguous() else x.contiguous()
    out = _empty(x.shape, dtype=torch.int64, device=x.device)
    if x.numel():
        _launch('tac_mulaw_encode_f64_i64', x.device, (out,), _native.ptr(x), x.numel(), n_quantize, _native.ptr(out))
    return out


def mu_law_decoding_f64(codes, n_quantize):
    """int64 or float64 codes -> float64 (reference functional.py:349-354 evaluated in double)."""
    codes = codes if codes.is_contiguous() else codes.contiguous()
    out = _empty(codes.shape, dtype=torch.float64, device=codes.device)
    if codes.numel():
        _launch('tac_mulaw_decode_f64', codes.device, (out,), _native.ptr(codes), 1 if codes.dtype == torch.int64 else 0,
                codes.numel(), n_quantize, _native.ptr(out))
    return out


# ----------------------------------------------------------------------------- gradients
def transposed_bank(fb):
    """(M, F) contiguous transpose of a filterbank, cached on the tensor per version (the adjoint of the filterbank
    stage is the same GEMM kernel with this matrix)."""
    return cached_on(fb, '_tac_T', (), lambda: fb.detach().t().contiguous())


def _adjoint_table(fb):
    """Per-bin {w0, w1, band0, band1} table of a bank with at most two non-zero weights per bin (every triangular mel
    bank), built on the device once per filterbank version (one host sync) and cached on the tensor; None otherwise."""
    def build():
        n_freqs, n_mels = fb.shape
        if n_mels > 512 or 16 * n_freqs + 4 * 4 * n_mels > 64 * 1024:
            return None
        src = fb if fb.is_contiguous() else fb.contiguous()         # (the cache stays on the caller's tensor object)
        table = torch.empty(4 * n_freqs + 4, dtype=torch.float32, device=fb.device)
        nnz = ctypes.c_int32(0)
        with _native.on_device(fb.device):
            rc = _native.lib().tac_filterbank_adjoint_pack(_native.ptr(src), n_freqs, n_mels, _native.ptr(table),
                                                           ctypes.cast(ctypes.pointer(nnz), ctypes.c_void_p),
                                                           _native.stream_ptr(fb.device))
        _native.check(rc, 'tac_filterbank_adjoint_pack')
        return table if nnz.value <= 2 else None
    return cached_on(fb, '_tac_adj', (), build)


def apply_filterbank_backward(grad_out, fb):
    """(*, M, T) gradient -> (*, F, T): two multiply-adds per output through the per-bin table of a bank with at most
    two non-zero weights per bin (tac_apply_filterbank_adjoint_f32); any other bank: the forward MFMA GEMM with the
    transposed bank."""
    table = _adjoint_table(fb) if (grad_out.dim() >= 2 and fb.dim() == 2 and MEL_PATH != 'mfma') else None
    if table is not None:
        n_freqs, n_mels = fb.shape
        gm = grad_out.transpose(-2, -1)                               # physical frame-major (*, T, M)
        gm = gm if gm.is_contiguous() else gm.contiguous()
        if gm.dtype != torch.float32:
            gm = gm.float()
        out = _empty(tuple(gm.shape[:-1]) + (n_freqs,), device=gm.device)
        rc = _launch('tac_apply_filterbank_adjoint_f32', gm.device, (out,), _native.ptr(gm), gm.numel() // n_mels, n_mels,
                     _native.ptr(table), n_freqs, _native.ptr(out), accept=_DECLINED)
        if rc != _native.TAC_E_UNSUPPORTED:
            return out.transpose(-2, -1)
    return apply_filterbank(grad_out, transposed_bank(fb), allow_sparse=False)


def melspectrogram_backward_fused(grad_mel, wave, window, fb, n_fft, hop, win_length, center, pad_mode, normalized, power):
    """Gradient of the waveform from the gradient of the (linear) mel values ``(*, M, T)`` in ONE kernel: the filterbank
    adjoint is formed per frame inside the backward kernel (tac_melspectrogram_backward_ola_f32), so the gradient of the
    power spectrogram — 4·F bytes per frame written by the adjoint kernel and read back by the backward kernel — never
    exists.  None when the form does not cover the case (fft_length other than 512 / 1024 / 2048, too many bands, a hop the
    register-ring kernels are not instantiated for at 512 / 1024, a bank with
    more than two non-zero weights per bin): the caller then runs the two kernels."""
    if n_fft not in (400, 512, 1024, 2048) or fb.dim() != 2 or fb.shape[1] > (256 if n_fft == 2048 else 128) or MEL_PATH == 'mfma':
        return None
    if n_fft == 400:        # overlap-add inside the kernel when the hop allows it, else frame gradients + the gather kernel
        out = _melspectrogram_backward_ola(grad_mel, wave, window, fb, n_fft, hop, win_length, center, pad_mode, normalized, power)
        if out is not None:
            return out
        return _melspectrogram_backward_fused_n400(grad_mel, wave, window, fb, hop, win_length, center, pad_mode, normalized, power)
    return _melspectrogram_backward_ola(grad_mel, wave, window, fb, n_fft, hop, win_length, center, pad_mode, normalized, power)


def _melspectrogram_backward_ola(grad_mel, wave, window, fb, n_fft, hop, win_length, center, pad_mode, normalized, power):
    table = _adjoint_table(fb)
    if table is None:
        return None
    g = geometry(wave, n_fft, hop, win_length, center, pad_mode, normalized, True)
    if g.desc is None:
        return None
    need = _native.lib().tac_spectrogram_backward_ola_workspace(g.desc)
    if need < 0:
        return None
    n_freqs, n_mels = fb.shape
    gm = grad_mel.transpose(-2, -1)                                   # physical frame-major (*, T, M)
    gm = gm if gm.is_contiguous() else gm.contiguous()
    if gm.dtype != torch.float32:
        gm = gm.float()
    out = _empty(tuple(wave.shape), device=wave.device)
    work = _empty(max(int(need), 4) // 4, device=wave.device)          # (scratch: poisoned, not checked)
    rc = _launch('tac_melspectrogram_backward_ola_f32', wave.device, (out,), _native.ptr(_rows_of(wave, g)), _native.ptr(window),
                 g.desc, _native.ptr(gm), n_mels, _native.ptr(table), n_freqs, float(power), _native.ptr(work), int(need),
                 _native.ptr(out), g.length, accept=_DECLINED)
    return None if rc == _native.TAC_E_UNSUPPORTED else out


def _melspectrogram_backward_fused_n400(grad_mel, wave, window, fb, hop, win_length, center, pad_mode, normalized, power):
    """fft_length 400: the mixed-radix backward kernel forms the filterbank adjoint itself (tac_melspectrogram_backward_f32),
    frame gradients cross memory once, gather overlap-add follows (tac_overlap_add_f32)."""
    table = _adjoint_table(fb)
    if table is None:
        return None
    g = geometry(wave, 400, hop, win_length, center, pad_mode, normalized, True)
    if g.desc is None:
        return None
    n_freqs, n_mels = fb.shape
    gm = grad_mel.transpose(-2, -1)                                   # physical frame-major (*, T, M)
    gm = gm if gm.is_contiguous() else gm.contiguous()
    if gm.dtype != torch.float32:
        gm = gm.float()
    frames = _empty((g.rows, g.n_frames, 400), device=wave.device)
    out = _empty(tuple(wave.shape), device=wave.device)
    desc = _native.StftDesc(rows=g.rows, length=g.length, row_stride=g.length, n_fft=400, hop=hop, win_length=win_length,
                            center=1 if center else 0, pad_mode=_native.PAD_MODES[pad_mode],
                            normalized=1 if normalized else 0, onesided=1, reserved=0)
    with _native.on_device(wave.device):
        rc = _launch('tac_melspectrogram_backward_f32', wave.device, (frames,), _native.ptr(_rows_of(wave, g)), _native.ptr(window),
                     g.desc, _native.ptr(gm), n_mels, _native.ptr(table), n_freqs, float(power), _native.ptr(frames),
                     accept=_DECLINED)
        if rc == _native.TAC_E_UNSUPPORTED:
            return None
        _launch('tac_overlap_add_f32', wave.device, (out,), _native.ptr(frames), desc, _native.ptr(out), g.length)
    return out


def stft_backward(grad_spec, wave, window, n_fft, hop, win_length, center, pad_mode, normalized, grad_norm=None,
                  power=2.0):
    """grad of the one-sided stft output ``(*, F, T, 2)`` w.r.t. the waveform: one inverse real FFT per frame
    (tac_stft_backward_f32) followed by the gather form of overlap-add (tac_overlap_add_f32).
    With ``grad_norm`` (the gradient of ``complex_norm(spec, power)``, shape ``(*, F, T)``) ``grad_spec`` is the
    spectrum itself and the norm's adjoint is folded into the load (tac_stft_norm_backward_f32) — or ``None``: the
    kernel then transforms the frames of ``wave`` again itself and no spectrum exists in memory
    (tac_spectrogram_backward_f32)."""
    g = geometry(wave, n_fft, hop, win_length, center, pad_mode, normalized, True)
    gs = None
    if grad_spec is not None:
        gs = grad_spec.transpose(-3, -2)                              # physical frame-major (*, T, F, 2)
        gs = gs if gs.is_contiguous() else gs.contiguous()
    gn = None
    if grad_norm is not None:
        gn = grad_norm.transpose(-2, -1)                              # (*, T, F)
        gn = gn if gn.is_contiguous() else gn.contiguous()
        if gn.dtype != torch.float32:
            gn = gn.float()
    out = _empty(tuple(wave.shape), device=wave.device)
    if gs is None and g.desc is not None:
        # fft_length 256 … 2048 with hop a multiple of fft_length / 16, fft_length 400 with hop a multiple of 4: overlap-add
        # inside the kernel, no frame gradients in memory
        need = _native.lib().tac_spectrogram_backward_ola_workspace(g.desc)
        if need >= 0:
            work = _empty(max(int(need), 4) // 4, device=wave.device)  # (scratch: poisoned, not checked)
            rc = _launch('tac_spectrogram_backward_ola_f32', wave.device, (out,), _native.ptr(_rows_of(wave, g)), _native.ptr(window),
                         g.desc, _native.ptr(gn), float(power), _native.ptr(work), int(need), _native.ptr(out), g.length,
                         accept=_DECLINED)
            if rc != _native.TAC_E_UNSUPPORTED:
                return out
    frames = _empty((g.rows, g.n_frames, n_fft), device=wave.device)
    desc = _native.StftDesc(rows=g.rows, length=g.length, row_stride=g.length, n_fft=n_fft, hop=hop,
                            win_length=win_length, center=1 if center else 0, pad_mode=_native.PAD_MODES[pad_mode],
                            normalized=1 if normalized else 0, onesided=1, reserved=0)
    dev = wave.device
    with _native.on_device(dev):
        if gn is None:
            _launch('tac_stft_backward_f32', dev, (frames,), _native.ptr(gs), _native.ptr(window), desc, _native.ptr(frames))
        elif gs is None:
            _launch('tac_spectrogram_backward_f32', dev, (frames,), _native.ptr(_rows_of(wave, g)), _native.ptr(window), g.desc,
                    _native.ptr(gn), float(power), _native.ptr(frames))
        else:
            _launch('tac_stft_norm_backward_f32', dev, (frames,), _native.ptr(gs), _native.ptr(gn), float(power),
                    _native.ptr(window), desc, _native.ptr(frames))
        _launch('tac_overlap_add_f32', dev, (out,), _native.ptr(frames), desc, _native.ptr(out), g.length)
    return out


# ---- the general gradient routes: every fft_length the forward kernels cover, two-sided outputs, and the gradients of
# the window and the filterbank (the reference differentiates through every argument, functional.py:99-107, 183-184).
# Built from the unfused pieces — inverse FFT per frame or the DFT-matrix GEMM with the transposed matrix, gather
# overlap-add, a frames x samples reduction for the window, the MFMA GEMM for the filterbank — so frame gradients do go
# through memory here; the fused backward kernels above remain the route of the common case (gradient of the waveform
# only, one-sided power-of-two sizes).
def fold_twosided(grad, n_fft, width):
    """physical frame-major gradient of a two-sided output (*, T, n_fft[, 2]) -> the one-sided bins (*, T, F[, 2])."""
    n_bins = n_fft // 2 + 1
    lead = tuple(grad.shape[:-2]) if width == 2 else tuple(grad.shape[:-1])
    out = _empty(lead + ((n_bins, 2) if width == 2 else (n_bins,)), device=grad.device)
    frames = out.numel() // (n_bins * width)
    _launch('tac_fold_twosided_f32', grad.device, (out,), _native.ptr(grad), frames, n_fft, width, _native.ptr(out))
    return out


def sum_slabs(x):
    """(S, ...) -> (...): the slabs added up in order (deterministic)."""
    out = _empty(tuple(x.shape[1:]), device=x.device)
    _launch('tac_sum_slabs_f32', x.device, (out,), _native.ptr(x), x.shape[0], out.numel(), _native.ptr(out))
    return out


_ones_cache = Bounded(64)


def _ones_window(device, n):
    key = (str(device), n)
    w = _ones_cache.get(key)
    if w is None:
        with torch.inference_mode(False):
            w = torch.ones(n, dtype=torch.float32, device=device)
        _ones_cache[key] = w
    return w


def _dft_matrix_t(window, n_fft, win_length, normalized):
    """(2F, N) transpose of the one-sided windowed-DFT matrix: the adjoint of ``_stft_dft`` is the same GEMM with it."""
    def build():
        return _dft_matrix(window, n_fft, win_length, True, normalized).t().contiguous()
    return cached_on(window, '_tac_dftT', (n_fft, win_length, bool(normalized)), build, limit=1)


def _desc(g, row_stride=None, onesided=None):
    return _native.StftDesc(rows=g.rows, length=g.length, row_stride=g.length if row_stride is None else row_stride,
                            n_fft=g.n_fft, hop=g.hop, win_length=g.win_length, center=1 if g.center else 0,
                            pad_mode=_native.PAD_MODES[g.pad_mode], normalized=1 if g.normalized else 0,
                            onesided=(1 if g.onesided else 0) if onesided is None else onesided, reserved=0)


def _frame_gradients(gs, window, g):
    """one-sided gradient spectrum (rows, T, F, 2) -> frame gradients (rows, T, n_fft), window and scale applied."""
    frames = _empty((g.rows, g.n_frames, g.n_fft), device=gs.device)
    with _native.on_device(gs.device):
        if fft_kernel_size(g.n_fft) or g.mixed_radix or smooth_fft_size(g.n_fft) or g.n_fft == 8192:
            _launch('tac_stft_backward_f32', gs.device, (frames,), _native.ptr(gs), _native.ptr(window), _desc(g, onesided=1),
                    _native.ptr(frames))
        else:
            n_cols = 2 * (g.n_fft // 2 + 1)
            mat_t = _dft_matrix_t(window, g.n_fft, g.win_length, g.normalized)
            _launch('tac_apply_filterbank_f32', gs.device, (frames,), _native.ptr(gs), g.rows, n_cols, g.n_frames,
                    g.n_frames * n_cols, 1, n_cols, _native.ptr(mat_t), None, g.n_fft, _native.ptr(frames))
    return frames


def stft_backward_general(grad_spec, wave, window, n_fft, hop, win_length, center, pad_mode, normalized, onesided,
                          need_wave=True, need_window=False):
    """(grad_wave, grad_window) from the gradient of the complex stft output ``(*, n_bins, T, 2)`` — any fft_length up
    to 8192, one- or two-sided."""
    g = geometry(wave, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    gs = grad_spec.transpose(-3, -2)                                   # physical frame-major (*, T, n_bins, 2)
    gs = gs if (gs.is_contiguous() and gs.dtype == torch.float32) else gs.contiguous().float()
    if not g.onesided:
        gs = fold_twosided(gs, n_fft, 2)
    window = window if window.is_contiguous() else window.contiguous()
    dev = wave.device
    grad_wave = grad_window = None
    if need_wave:
        frames = _frame_gradients(gs, window, g)
        grad_wave = _empty(tuple(wave.shape), device=dev)
        _launch('tac_overlap_add_f32', dev, (grad_wave,), _native.ptr(frames), _desc(g), _native.ptr(grad_wave), g.length)
        del frames
    if need_window:
        unwindowed = _frame_gradients(gs, _ones_window(dev, win_length), g)
        src = _rows_of(wave, g)
        desc = _desc(g, row_stride=g.row_stride)
        n_part = int(_native.lib().tac_window_grad_partials(desc))
        if n_part < 0:
            _native.check(n_part, 'tac_window_grad_partials')
        partial = _empty((n_part, n_fft), device=dev)
        _launch('tac_window_grad_f32', dev, (partial,), _native.ptr(unwindowed), _native.ptr(src), desc, _native.ptr(partial), n_part)
        off = (n_fft - win_length) // 2
        grad_window = sum_slabs(partial)[off:off + win_length]
    return grad_wave, grad_window


def filterbank_grad(spec, grad_out):
    """d/d filterbank of ``apply_filterbank(spec, fb)``: grad_fb[f][m] = sum over (*, t) of spec[.., f, t] *
    grad_out[.., m, t] — one fp32 MFMA GEMM whose contraction runs over every frame of the batch."""
    sp = spec.transpose(-2, -1)                                        # (*, T, F)
    sp = sp if (sp.is_contiguous() and sp.dtype == torch.float32) else sp.contiguous().float()
    gm = grad_out.transpose(-2, -1)                                    # (*, T, M)
    gm = gm if (gm.is_contiguous() and gm.dtype == torch.float32) else gm.contiguous().float()
    n_freqs, n_mels = sp.shape[-1], gm.shape[-1]
    total = sp.numel() // n_freqs
    if total >= 2 ** 31:
        raise NotImplementedError('filterbank gradient: more than 2^31 frames in one call')
    out = _empty((n_freqs, n_mels), device=sp.device)
    if total == 0:
        return out.zero_()
    _launch('tac_apply_filterbank_f32', sp.device, (out,), _native.ptr(sp), 1, total, n_freqs, 0, n_freqs, 1, _native.ptr(gm), None,
            n_mels, _native.ptr(out))
    return out


def stft_backward_supported(n_fft, onesided):
    """one-sided power-of-two sizes and fft_length 400: an inverse-FFT kernel per frame (csrc/backward.hip,
    csrc/stft_n400.hip); everything else takes ``stft_backward_general``"""
    return bool(onesided) and (fft_kernel_size(n_fft) or mixed_radix_size(n_fft))


def backward_recomputes_spectrum(n_fft):
    """Sizes whose spectrogram backward kernel transforms the frames again itself (16 elements per lane, and the
    mixed-radix fft_length 400; at 4096 the second transform does not fit the registers and the spectrum is recomputed
    into memory by the stft kernel)."""
    return (fft_kernel_size(n_fft) and n_fft <= 2048) or mixed_radix_size(n_fft)


def complex_norm_backward(z, grad_out, power):
    """(*, F, T, 2) pairs and (*, F, T) gradients in, (*, F, T, 2) out — all walked in z's dense storage order."""
    z = _pairs(z)
    want = tuple(s // 2 for s in z.stride()[:-1])
    if grad_out.dtype == torch.float32 and grad_out.shape == z.shape[:-1] and grad_out.stride() == want:
        go = grad_out                                                 # already in z's storage order: no copy
    else:
        go = torch.empty_strided(z.shape[:-1], want, dtype=torch.float32, device=z.device)
        go.copy_(grad_out)
    gz = _empty_strided(z.shape, z.stride(), device=z.device)
    n = go.numel()
    if n:
        _launch('tac_complex_norm_backward_f32', z.device, (gz,), _native.ptr(z), _native.ptr(go), n, float(power), _native.ptr(gz))
    return gz


def magphase_backward(z, grad_mag, grad_phase, power):
    """Gradient of ``magphase`` / ``angle``: (*, F, T, 2) pairs and one or two (*, F, T) gradients in (either may be None), (*, F, T, 2)
    out — all walked in z's dense storage order."""
    z = _pairs(z)
    want = tuple(s // 2 for s in z.stride()[:-1])

    def ordered(g):
        if g is None or (g.dtype == torch.float32 and g.shape == z.shape[:-1] and g.stride() == want):
            return g                                                  # already in z's storage order: no copy
        go = torch.empty_strided(z.shape[:-1], want, dtype=torch.float32, device=z.device)
        go.copy_(g)
        return go
    gm, gp = ordered(grad_mag), ordered(grad_phase)
    gz = _empty_strided(z.shape, z.stride(), device=z.device)
    n = z.numel() // 2
    if n:
        _launch('tac_magphase_backward_f32', z.device, (gz,), _native.ptr(z), None if gm is None else _native.ptr(gm),
                None if gp is None else _native.ptr(gp), n, float(power), _native.ptr(gz))
    return gz


def db_to_amplitude_backward(x, grad_out, ref):
    x = x if is_dense(x) else x.contiguous()
    if grad_out.dtype == torch.float32 and grad_out.shape == x.shape and grad_out.stride() == x.stride():
        go = grad_out                                                 # already in x's storage order: no copy
    else:
        go = torch.empty_like(x)
        go.copy_(grad_out)
    gx = _empty_like(x)
    if x.numel():
        _launch('tac_db_to_amplitude_backward_f32', x.device, (gx,), _native.ptr(x), _native.ptr(go), x.numel(), float(ref),
                _native.ptr(gx))
    return gx


def amplitude_to_db_backward(x, grad_out, amin):
    x = x if is_dense(x) else x.contiguous()
    if grad_out.dtype == torch.float32 and grad_out.shape == x.shape and grad_out.stride() == x.stride():
        go = grad_out                                                 # already in x's storage order: no copy
    else:
        go = torch.empty_like(x)
        go.copy_(grad_out)
    gx = _empty_like(x)
    if x.numel():
        _launch('tac_amplitude_to_db_backward_f32', x.device, (gx,), _native.ptr(x), _native.ptr(go), x.numel(), float(amin),
                _native.ptr(gx))
    return gx


# ----------------------------------------------------------------------------- hpss
def hpss_supported(kernel_f, kernel_t):
    return kernel_f % 2 == 1 and kernel_t % 2 == 1 and 1 <= kernel_f <= 63 and 1 <= kernel_t <= 63


def hpss(mag, kernel_f, kernel_t, power, hard, masks_only=False):
    """(harm, perc, mask_harm, mask_perc), float32, in the (dense) layout of ``mag``  (*, F, T); with ``masks_only`` the two
    masks alone (the kernels then skip the two masked-spectrogram stores: 40 % of the traffic)."""
    mag = mag if is_dense(mag) else mag.contiguous()
    n_freqs, n_frames = mag.shape[-2], mag.shape[-1]
    rows = mag.reshape(-1, n_freqs, n_frames)
    if rows.data_ptr() != mag.data_ptr():                          # leading dims do not collapse in this layout
        mag = mag.contiguous()
        rows = mag.reshape(-1, n_freqs, n_frames)
    outs = [_empty_like(mag) for _ in range(2 if masks_only else 4)]
    if mag.numel():
        null = ctypes.c_void_p(0)
        _launch('tac_hpss_f32', mag.device, outs, _native.ptr(rows), rows.shape[0], n_freqs, n_frames,
                rows.stride(0) if rows.shape[0] > 1 else 0, rows.stride(1), rows.stride(2), kernel_f, kernel_t, float(power),
                1 if hard else 0, null if masks_only else _native.ptr(outs[0]), null if masks_only else _native.ptr(outs[1]),
                _native.ptr(outs[-2]), _native.ptr(outs[-1]))
    return tuple(outs)


def hpss_backward(mag, kernel_f, kernel_t, power, hard, grads):
    """d hpss / d mag: ``grads`` = the gradients of (harm, perc, mask_harm, mask_perc), each a tensor of mag's shape or None; the result
    is in mag's (dense) layout.  The gradient of a median goes to the element it selected (float atomics: the last bits vary)."""
    mag = mag if is_dense(mag) else mag.contiguous()
    n_freqs, n_frames = mag.shape[-2], mag.shape[-1]
    rows = mag.reshape(-1, n_freqs, n_frames)
    if rows.data_ptr() != mag.data_ptr():
        mag = mag.contiguous()
        rows = mag.reshape(-1, n_freqs, n_frames)

    def like_mag(g):
        if g is None:
            return None
        if g.dtype == torch.float32 and g.shape == mag.shape and g.stride() == mag.stride():
            return g
        out = torch.empty_like(mag)
        out.copy_(g)
        return out
    gs = [like_mag(g) for g in grads]
    gmag = torch.zeros_like(mag)                                   # the kernel accumulates into it
    if mag.numel():
        null = ctypes.c_void_p(0)
        _launch('tac_hpss_backward_f32', mag.device, (), _native.ptr(rows), rows.shape[0], n_freqs, n_frames,
                rows.stride(0) if rows.shape[0] > 1 else 0, rows.stride(1), rows.stride(2), kernel_f, kernel_t, float(power),
                1 if hard else 0, *[null if g is None else _native.ptr(g) for g in gs], _native.ptr(gmag))
    return gmag


# ----------------------------------------------------------------------------- coded waveforms (int16 PCM, mu-law codes)
def pcm16_to_f32(x):
    """int16 PCM -> float32 in [-1, 1): x * 2^-15 (for the kernels without a coded frame load)."""
    x = x if x.is_contiguous() else x.contiguous()
    out = _empty(x.shape, device=x.device)
    if x.numel():
        _launch('tac_pcm16_to_f32', x.device, (out,), _native.ptr(x), x.numel(), _native.ptr(out))
    return out


_SAMPLE_FORMATS = {torch.int16: _native.SAMPLES_I16, torch.uint8: _native.SAMPLES_MULAW_U8,
                   torch.int64: _native.SAMPLES_MULAW_I64}


def melspectrogram_coded(samples, window, fb, n_fft, hop, win_length, center, pad_mode, normalized, onesided, power, db,
                         ref, amin):
    """The fused chain reading int16 PCM (value = sample * 2^-15) or 8-bit mu-law codes stored as uint8 / int64
    (value = the reference's 256-entry decode table) straight from the stored samples, converted in registers inside
    the frame load.  Returns None when the single-kernel route does not cover the configuration — the caller then
    converts first and takes the float32 path."""
    g = geometry(samples, n_fft, hop, win_length, center, pad_mode, normalized, onesided)
    if not ((g.pow2_kernel or g.mixed_radix) and g.onesided and g.n_fft in (256, 400, 512, 1024, 2048) and fb.dim() == 2
            and fb.shape[0] == g.n_bins
            and fb.is_contiguous() and power in (1.0, 2.0) and MEL_PATH != 'mfma'):
        return None
    pack = _melbank_pack(fb, g.n_fft)
    if pack is None:
        return None
    wpack, desc, info = pack
    fmt = _SAMPLE_FORMATS[samples.dtype]
    lut = _mulaw_tables(samples.device)[4] if fmt != _native.SAMPLES_I16 else None
    src = _rows_of(samples, g)
    out = _empty(g.lead + (g.n_frames, fb.shape[1]), device=samples.device)
    rc = _launch('tac_melspec_sparse_coded_f32', samples.device, (out,), _native.ptr(src), fmt,
                 None if lut is None else _native.ptr(lut), _native.ptr(window), g.desc, float(power), _native.ptr(wpack),
                 _native.ptr(desc), ctypes.cast(info, ctypes.c_void_p), fb.shape[1], 1 if db else 0, float(ref), float(amin),
                 _native.ptr(out), accept=_DECLINED)
    return None if rc == _native.TAC_E_UNSUPPORTED else out.transpose(-2, -1)
