#!/usr/bin/env python
"""Time ``kaldi_fbank`` on the gfx950 kernel (csrc/kaldi_fbank.hip) against the composite torch route on the same device tensors,
in one process, alternating the routes.

    python tools/bench_kaldi_fbank.py [--repeats 7] [--min-seconds 0.5] [--json OUT] [--profile ROUTE]

Shape: 256 rows x 160 000 samples (10 s at 16 kHz), 25 ms frames every 10 ms, 80 bins — 998 frames per row.  Routes:

    kernel      tac_kaldi_fbank_f32: one launch from waveform rows to log mel rows
    composite   ``_composite.kaldi_fbank``: unfold, mean, pre-emphasis, window, ``rfft``, ``matmul``, ``log`` in torch operators

Four distinct HBM-resident inputs are visited in turn; a block is at least ``--min-seconds`` of calls between two device events,
after a warm-up of both routes; ``--repeats`` alternating blocks give median / min / max and the run-to-run spread.  Prints ONE
JSON line, with the achieved bytes/s of the kernel against the bytes it has to move (every sample read once, every output written
once) and the largest difference between the routes' outputs.  ``--profile kernel|composite`` runs only that route a few times
(for rocprofv3 --kernel-trace --stats).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

ROWS, LENGTH, BINS = 256, 160000, 80
HBM_BYTES_PER_S = 8e12


def block(fn, inputs, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[i % len(inputs)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--json', default='')
    ap.add_argument('--profile', default='')
    ap.add_argument('--rows', type=int, default=ROWS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_kaldi_fbank.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(80)
    waves = [torch.rand((a.rows, LENGTH), device='cuda', generator=gen) * 2 - 1 for _ in range(4)]
    args = tuple(tac._kaldi.Params(**dict(
        blackman_coeff=0.42, dither=0.0, energy_floor=1.0, frame_length=25.0, frame_shift=10.0, high_freq=0.0, htk_compat=False,
        low_freq=20.0, num_mel_bins=BINS, preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True,
        round_to_power_of_two=True, sample_frequency=16000.0, snip_edges=True, subtract_mean=False, use_energy=False,
        use_log_fbank=True, use_power=True, window_type='povey')))
    tac.set_strict(True)
    routes = {'kernel': lambda w: tac.kaldi_fbank(w, num_mel_bins=BINS),
              'composite': lambda w: tac._composite.kaldi_fbank(w, *args)}
    before = dict(tac._hip.launches)
    got = routes['kernel'](waves[0])
    launches = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
    worst = float((got - routes['composite'](waves[0])).abs().max())
    if a.profile:
        for _ in range(5):
            for x in waves:
                routes[a.profile](x)
        torch.cuda.synchronize()
        return
    iters = {}
    for name, fn in routes.items():                                # warm-up, and the block length that fills min-seconds
        block(fn, waves, 4)
        per_call = block(fn, waves, 8)
        iters[name] = max(8, int(a.min_seconds * 1e3 / per_call) + 1)
    times = {name: [] for name in routes}
    for _ in range(a.repeats):
        for name, fn in routes.items():
            times[name].append(block(fn, waves, iters[name]))
    frames = got.shape[-2]
    moved = a.rows * (LENGTH + frames * BINS) * 4
    line = {'rows': a.rows, 'samples': LENGTH, 'bins': BINS, 'frames_per_row': frames, 'repeats': a.repeats,
            'min_seconds': a.min_seconds, 'moved_MB': round(moved / 1e6, 1), 'launches': launches,
            'max_abs_diff_kernel_vs_composite': worst}
    for name in routes:
        t = times[name]
        med = statistics.median(t)
        line[name] = {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                      'spread': round((max(t) - min(t)) / med, 4), 'iters_per_block': iters[name]}
    med = line['kernel']['ms_median']
    line['kernel']['TB_per_s'] = round(moved / (med * 1e-3) / 1e12, 3)
    line['kernel']['share_of_8TB_per_s'] = round(moved / (med * 1e-3) / HBM_BYTES_PER_S, 4)
    line['kernel']['frames_per_s'] = round(a.rows * frames / (med * 1e-3))
    line['composite_over_kernel'] = round(line['composite']['ms_median'] / med, 3)
    line['kernel_faster_beyond_spread'] = bool(line['kernel']['ms_max'] < line['composite']['ms_min'])
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
