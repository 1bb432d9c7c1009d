#!/usr/bin/env python
"""Time the recursive-filter kernel (csrc/lfilter.hip) against the ideal streaming launch and against ``tac_polyphase_f32`` at one
phase (48000 -> 16000 reads the same tensor once; the nearest existing streaming kernel over waveforms), in one process,
alternating the routes.

    python tools/bench_lfilter.py [--repeats 7] [--min-seconds 0.3] [--json profiles/lfilter/bench.json]

Shapes: 256 x 1 x 160000 (the waveform of benchmark config 2) and one row of 16 000 000 samples (one workgroup walks a row, so a
single row uses one CU: the under-filled case).  Routes per shape:

    highpass            highpass_biquad(20 Hz at 16 kHz) forward: the float64 recursion and scan
    highpass_backward   the same kernel run from the end of each row (the gradient w.r.t. the waveform, no clamp mask)
    preemphasis         preemphasis forward: the kernel without recursion
    preemphasis_backward
    polyphase           tac_polyphase_f32, 48000 -> 16000, on the same tensor

Two distinct HBM-resident inputs are visited in turn; a block is at least ``--min-seconds`` of calls between two device events,
after a warm-up of every route; ``--repeats`` alternating blocks give median / min / max.  Prints ONE JSON line (and writes it to
``--json``) with, for the filter routes, the achieved bytes/s against the algorithmic traffic — one float32 read and one write per
sample — and its share of 8 TB/s.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402
from torchaudio_contrib_amd import _filters, _resample  # noqa: E402

SHAPES = ((256, 1, 160000), (1, 1, 16000000))
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
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--json', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_lfilter.py measures on the GPU only'
    tac.set_strict(True)
    hb, ha = _filters.highpass(16000, 20.0)
    pb, pa = (1.0, -0.97), (1.0, 0.0)
    key = _resample.constants(48000, 16000)
    result = {'chunk': tac._hip.LFILTER_C, 'tile': tac._hip.LFILTER_TILE, 'repeats': a.repeats, 'min_seconds': a.min_seconds,
              'shapes': []}
    for shape in SHAPES:
        gen = torch.Generator(device='cuda').manual_seed(shape[0])
        waves = [torch.rand(shape, device='cuda', generator=gen) * 2 - 1 for _ in range(2)]
        n_out = _resample.out_length(shape[-1], key[0], key[1])
        routes = {
            'highpass': lambda w: tac._hip.lfilter_rows(w, hb, ha, True),
            'highpass_backward': lambda w: tac._hip.lfilter_rows(w, hb, ha, False, reverse=True),
            'preemphasis': lambda w: tac._hip.lfilter_rows(w, pb, pa, False),
            'preemphasis_backward': lambda w: tac._hip.lfilter_rows(w, pb, pa, False, reverse=True),
            'polyphase': lambda w: tac._hip.polyphase(w, key, n_out),
        }
        before = dict(tac._hip.launches)
        tac.highpass_biquad(waves[0], 16000, 20.0)
        tac.preemphasis(waves[0])
        launched = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        iters = {}
        for name, fn in routes.items():                            # warm-up, and the block length that fills min-seconds
            block(fn, waves, 2)
            iters[name] = max(4, int(a.min_seconds * 1e3 / block(fn, waves, 4)) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, waves, iters[name]))
        samples = shape[0] * shape[1] * shape[2]
        line = {'shape': list(shape), 'traffic_MB': round(samples * 8 / 1e6, 1), 'launches': launched,
                'ideal_ms_at_8TB_per_s': round(samples * 8 / HBM_BYTES_PER_S * 1e3, 4)}
        for name in routes:
            t = times[name]
            med = statistics.median(t)
            line[name] = {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                          'spread': round((max(t) - min(t)) / med, 4), 'iters_per_block': iters[name]}
            moved = samples * 8 if name != 'polyphase' else (samples + shape[0] * shape[1] * n_out) * 4
            line[name]['TB_per_s'] = round(moved / (med * 1e-3) / 1e12, 4)
            line[name]['share_of_8TB_per_s'] = round(moved / (med * 1e-3) / HBM_BYTES_PER_S, 4)
        result['shapes'].append(line)
        del waves
        torch.cuda.empty_cache()
    text = json.dumps(result)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
