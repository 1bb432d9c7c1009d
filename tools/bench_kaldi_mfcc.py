#!/usr/bin/env python
"""Time ``kaldi_mfcc`` and ``kaldi_spectrogram`` on the gfx950 kernel (csrc/kaldi_fbank.hip) against the way to the same numbers
without them, on the same device tensors, in one process, alternating the routes.

    python tools/bench_kaldi_mfcc.py [--repeats 7] [--min-seconds 0.3] [--json OUT] [--baseline-lib LIB]

Shape: 256 rows x 160 000 samples (10 s at 16 kHz), 25 ms frames every 10 ms — 998 frames per row.  Routes, for 23 bins / 13
coefficients and for 80 / 40:

    mfcc            tac_kaldi_mfcc_f32: one launch from waveform rows to cepstra
    mfcc_unfused    ``kaldi_fbank`` (one launch), ``matmul`` with the DCT matrix, multiply by the lifter: three launches and a
                    round trip of the log-mel rows through memory
    mfcc_htk, mfcc_htk_unfused   the same with ``htk_compat``: the unfused form adds the ``cat`` of the column order
    fbank           tac_kaldi_fbank_f32 alone (the launch the new modes share their body with)
    fbank_baseline  with ``--baseline-lib``: ``tac_kaldi_fbank_f32`` of that library (a build of another commit), same arguments

and for the spectrogram

    spectrogram            tac_kaldi_spectrogram_f32: one launch
    spectrogram_composite  ``_composite.kaldi_spectrogram``: unfold, mean, pre-emphasis, window, ``rfft``, ``log`` in torch operators

Four distinct HBM-resident inputs are visited in turn; a block is at least ``--min-seconds`` of calls between two device events,
after a warm-up of every route; ``--repeats`` alternating blocks give median / min / max and the run-to-run spread.  Prints ONE
JSON line.  Needs the GPU: there is no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

ROWS, LENGTH = 256, 160000
SIZES = ((23, 13), (80, 40))


def block(fn, inputs, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[i % len(inputs)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def baseline_fbank(path, bins):
    """``tac_kaldi_fbank_f32`` of the library at ``path`` with the arguments ``_hip.kaldi_fbank`` passes for ``bins`` bins"""
    P, I32, I64, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    h = ctypes.CDLL(path)
    h.tac_kaldi_fbank_f32.restype = ctypes.c_int
    h.tac_kaldi_fbank_f32.argtypes = [P, I64, I64, I64, P, P, P, I32, I32, I32, I32, I32, I32, F, F, P, P]
    p = tac._kaldi.fbank_params(tac._kaldi.MfccParams(0.42, 22.0, 0.0, 1.0, 25.0, 10.0, 0.0, False, 20.0, 13, bins, 0.97, True, True,
                                                      True, 16000.0, True, False, False, 'povey'))
    w, s, n = tac._kaldi.check(p)
    flags = tac._hip._kaldi_flags(p)

    def run(x):
        window, weights, table, w_total = tac._hip._kaldi_device_tables(p, w, n, x.device)
        m = tac._kaldi.num_frames(x.shape[-1], w, s, True)
        out = torch.empty((x.shape[0], m, bins), device=x.device)
        rc = h.tac_kaldi_fbank_f32(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), window.data_ptr(), weights.data_ptr(),
                                   table.data_ptr(), n, w, s, bins, w_total, flags, 0.97, 1.0, out.data_ptr(),
                                   tac._native.raw_stream(x.device))
        assert rc == 0, rc
        return out
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--json', default='')
    ap.add_argument('--rows', type=int, default=ROWS)
    ap.add_argument('--baseline-lib', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_kaldi_mfcc.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(80)
    waves = [torch.rand((a.rows, LENGTH), device='cuda', generator=gen) * 2 - 1 for _ in range(4)]
    tac.set_strict(True)
    routes, pairs = {}, []
    for bins, ceps in SIZES:
        tag = '%d_%d' % (bins, ceps)
        dct = tac._kaldi.dct64(bins, ceps).float().cuda()
        lift = tac._kaldi.lifter64(ceps, 22.0).float().cuda()
        lift_htk = lift.clone()
        lift_htk[0] *= 2.0 ** 0.5

        def unfused(x, bins=bins, dct=dct, lift=lift):
            return torch.matmul(tac.kaldi_fbank(x, num_mel_bins=bins), dct) * lift

        def unfused_htk(x, bins=bins, dct=dct, lift=lift_htk):
            c = torch.matmul(tac.kaldi_fbank(x, num_mel_bins=bins), dct) * lift
            return torch.cat([c[..., 1:], c[..., :1]], -1)

        routes['mfcc_' + tag] = lambda x, bins=bins, ceps=ceps: tac.kaldi_mfcc(x, num_mel_bins=bins, num_ceps=ceps)
        routes['mfcc_unfused_' + tag] = unfused
        routes['mfcc_htk_' + tag] = lambda x, bins=bins, ceps=ceps: tac.kaldi_mfcc(x, num_mel_bins=bins, num_ceps=ceps, htk_compat=True)
        routes['mfcc_htk_unfused_' + tag] = unfused_htk
        routes['fbank_' + tag] = lambda x, bins=bins: tac.kaldi_fbank(x, num_mel_bins=bins)
        pairs += [('mfcc_' + tag, 'mfcc_unfused_' + tag), ('mfcc_htk_' + tag, 'mfcc_htk_unfused_' + tag)]
        if a.baseline_lib:
            routes['fbank_baseline_' + tag] = baseline_fbank(a.baseline_lib, bins)
            pairs.append(('fbank_' + tag, 'fbank_baseline_' + tag))
    sargs = tuple(tac._kaldi.SpectrogramParams(0.42, 0.0, 1.0, 25.0, 10.0, 0.97, True, True, True, 16000.0, True, False, 'povey'))
    routes['spectrogram'] = lambda x: tac.kaldi_spectrogram(x)
    routes['spectrogram_composite'] = lambda x: tac._composite.kaldi_spectrogram(x, *sargs)
    pairs.append(('spectrogram', 'spectrogram_composite'))

    line = {'rows': a.rows, 'samples': LENGTH, 'repeats': a.repeats, 'min_seconds': a.min_seconds, 'max_abs_diff': {}}
    for fused, other in pairs:
        x, y = routes[fused](waves[0]), routes[other](waves[0])
        line['max_abs_diff'][fused] = float((x - y).abs().max())
        del x, y
    iters = {}
    for name, fn in routes.items():                                # warm-up, and the block length that fills min-seconds
        block(fn, waves, 4)
        per_call = block(fn, waves, 8)
        iters[name] = max(8, int(a.min_seconds * 1e3 / per_call) + 1)
    times = {name: [] for name in routes}
    for _ in range(a.repeats):
        for name, fn in routes.items():
            times[name].append(block(fn, waves, iters[name]))
    for name in routes:
        t = times[name]
        med = statistics.median(t)
        line[name] = {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                      'spread': round((max(t) - min(t)) / med, 4), 'iters_per_block': iters[name]}
    line['ratios'] = {}
    for fused, other in pairs:
        line['ratios'][other + '_over_' + fused] = round(line[other]['ms_median'] / line[fused]['ms_median'], 3)
        line['ratios'][fused + '_faster_beyond_spread'] = bool(line[fused]['ms_max'] < line[other]['ms_min'])
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
