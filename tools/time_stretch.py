#!/usr/bin/env python
"""Time STFT -> TimeStretch -> ComplexNorm -> ApplyFilterbank -> AmplitudeToDb at the cfg-2 shape on the magnitude-only route
(the |X| spectrogram kernel + tac_stretch_mel_f32) against the five-launch route (set_lazy_fusion(False): complex STFT rows,
phase_vocoder, complex_norm, apply_filterbank, amplitude_to_db), in one process, alternating the two.

    python tools/time_stretch.py [--rates 0.8,1.3,2.0] [--repeats 7] [--iters 40] [--json OUT] [--profile ROUTE]

Prints one JSON line per rate: median / min / max of the per-call time in ms of both routes over ``repeats`` alternating blocks of
``iters`` calls (device events around each block, after a warm-up of both), and the algorithmic bytes of the new kernel
(T F 4 read + n_out (F or n_mels) 4 written per row).  ``--profile new|old`` runs only that route a few times (for rocprofv3).
Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

SHAPE, N_FFT, HOP, N_MELS, SR = (256, 1, 160000), 2048, 512, 128, 16000


def block(model, x, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        model(x)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rates', default='0.8,1.3,2.0')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--json', default='')
    ap.add_argument('--profile', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_stretch.py measures on the GPU only'
    tac.set_strict(True)
    gen = torch.Generator(device='cuda').manual_seed(0)
    x = torch.rand(SHAPE, device='cuda', generator=gen) * 2 - 1
    n_freqs = N_FFT // 2 + 1
    fb = tac.MelFilterbank(num_freqs=n_freqs, num_mels=N_MELS, sample_rate=SR).get_filterbank().cuda()
    lines = []
    for rate in [float(r) for r in a.rates.split(',')]:
        model = torch.nn.Sequential(tac.STFT(N_FFT, HOP), tac.TimeStretch(HOP, n_freqs, fixed_rate=rate), tac.ComplexNorm(2.0),
                                    tac.ApplyFilterbank(fb), tac.AmplitudeToDb()).cuda()
        if a.profile:
            tac.set_lazy_fusion(a.profile == 'new')
            for _ in range(5):
                model(x)
            torch.cuda.synchronize()
            continue
        times = {'new': [], 'old': []}
        for route in ('new', 'old'):                     # warm-up of both
            tac.set_lazy_fusion(route == 'new')
            block(model, x, 5)
        for _ in range(a.repeats):
            for route in ('new', 'old'):
                tac.set_lazy_fusion(route == 'new')
                times[route].append(block(model, x, a.iters))
        tac.set_lazy_fusion(True)
        rows, frames = SHAPE[0] * SHAPE[1], 1 + SHAPE[2] // HOP
        n_out = tac._hip.phase_vocoder_out_frames(frames, rate)
        line = {'rate': rate, 'shape': SHAPE, 'fft_length': N_FFT, 'hop': HOP, 'n_mels': N_MELS, 'iters': a.iters, 'repeats': a.repeats,
                'stretch_mel_algorithmic_MB': round(rows * (frames * n_freqs + n_out * N_MELS) * 4 / 1e6, 1)}
        for route in ('new', 'old'):
            t = times[route]
            line[route + '_ms'] = {'median': round(statistics.median(t), 4), 'min': round(min(t), 4), 'max': round(max(t), 4)}
        line['old_over_new'] = round(line['old_ms']['median'] / line['new_ms']['median'], 3)
        print(json.dumps(line))
        lines.append(line)
    if a.json:
        with open(a.json, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
