#!/usr/bin/env python
"""Time the polyphase resampling kernel (csrc/resample.hip) against ``_composite.resample`` — torch's ``conv1d`` with the full
bank, torchaudio's formulation — on the same device tensors, in one process, alternating the routes.

    python tools/bench_resample.py [--repeats 7] [--min-seconds 0.5] [--json profiles/resample/bench.json] [--profile ROUTE]

Pairs: 48000 -> 16000, 44100 -> 16000, 16000 -> 44100 on 256 rows x 10 s.  Routes per pair:

    kernel      tac_polyphase_f32 (one launch)
    composite   _composite.resample: pad, conv1d at stride orig with the (new, 1, 2 width + orig) bank, interleave, cut
    backward    the gradient w.r.t. the waveform: the same kernel with the adjoint bank

Two distinct HBM-resident inputs are visited in turn; a block is at least ``--min-seconds`` of calls between two device events,
after a warm-up of every route; ``--repeats`` alternating blocks give median / min / max and the run-to-run spread.  Prints ONE
JSON line (and writes it to ``--json``); for the kernel routes also the achieved bytes/s against the algorithmic traffic — the
input read once and the output written once, (L_in + L_out) * 4 bytes per row — and its share of 8 TB/s.  ``--profile
kernel|composite|backward`` runs only that route a few times (for rocprofv3 --kernel-trace --stats).  Needs the GPU: there is no
fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402
from torchaudio_contrib_amd import _composite, _resample  # noqa: E402

ROWS, SECONDS = 256, 10
PAIRS = ((48000, 16000), (44100, 16000), (16000, 44100))
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
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_resample.py measures on the GPU only'
    tac.set_strict(True)
    result = {'rows': ROWS, 'seconds': SECONDS, 'repeats': a.repeats, 'min_seconds': a.min_seconds, 'pairs': []}
    for orig_freq, new_freq in PAIRS:
        key = _resample.constants(orig_freq, new_freq)
        orig, new = key[0], key[1]
        l_in = orig_freq * SECONDS
        l_out = _resample.out_length(l_in, orig, new)
        gen = torch.Generator(device='cuda').manual_seed(orig_freq)
        waves = [torch.rand((ROWS, l_in), device='cuda', generator=gen) * 2 - 1 for _ in range(2)]
        grads = [torch.rand((ROWS, l_out), device='cuda', generator=gen) * 2 - 1 for _ in range(2)]
        fwd, adj = _resample.bank(*key), _resample.adjoint_bank(*key)
        routes = {'kernel': (lambda w: tac._hip.polyphase(w, key, l_out), waves),
                  'composite': (lambda w: _composite.resample(w, *key), waves),
                  'backward': (lambda g: tac._hip.polyphase(g, key, l_in, adjoint=True), grads)}
        before = dict(tac._hip.launches)
        got = tac.resample(waves[0], orig_freq, new_freq)
        launched = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        worst = float((got - _composite.resample(waves[0], *key)).abs().max())
        if a.profile:
            fn, inputs = routes[a.profile]
            for _ in range(5):
                for x in inputs:
                    fn(x)
            torch.cuda.synchronize()
            continue
        iters = {}
        for name, (fn, inputs) in routes.items():                  # warm-up, and the block length that fills min-seconds
            block(fn, inputs, 4)
            per_call = block(fn, inputs, 8)
            iters[name] = max(8, int(a.min_seconds * 1e3 / per_call) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, (fn, inputs) in routes.items():
                times[name].append(block(fn, inputs, iters[name]))
        moved = ROWS * (l_in + l_out) * 4
        width = _resample.width_of(orig, new, key[2], key[3])
        line = {'orig_freq': orig_freq, 'new_freq': new_freq, 'orig': orig, 'new': new, 'samples_in': l_in, 'samples_out': l_out,
                'bank': [fwd.phases, fwd.K], 'adjoint_bank': [adj.phases, adj.K], 'full_bank': [new, 2 * width + orig],
                'tile': tac._hip.resample_tile(fwd), 'adjoint_tile': tac._hip.resample_tile(adj), 'traffic_MB': round(moved / 1e6, 1),
                'fma_per_output': fwd.K, 'launches': launched, 'max_abs_diff_kernel_vs_composite': worst}
        for name in routes:
            t = times[name]
            med = statistics.median(t)
            line[name] = {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                          'spread': round((max(t) - min(t)) / med, 4), 'iters_per_block': iters[name]}
            if name != 'composite':
                line[name]['TB_per_s'] = round(moved / (med * 1e-3) / 1e12, 3)
                line[name]['share_of_8TB_per_s'] = round(moved / (med * 1e-3) / HBM_BYTES_PER_S, 4)
        line['composite_over_kernel'] = round(line['composite']['ms_median'] / line['kernel']['ms_median'], 3)
        line['kernel_faster_beyond_spread'] = bool(line['kernel']['ms_max'] < line['composite']['ms_min'])
        line['composite_faster_beyond_spread'] = bool(line['composite']['ms_max'] < line['kernel']['ms_min'])
        result['pairs'].append(line)
        del waves, grads
        torch.cuda.empty_cache()
    if a.profile:
        return
    text = json.dumps(result)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
