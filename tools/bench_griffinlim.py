#!/usr/bin/env python
"""Time ``griffinlim`` on the gfx950 kernels (prepare, then ``tac_istft_f32`` + ``tac_stft_f32`` + ``tac_griffinlim_update_f32`` a
step) against the composite of torch operators on the same device tensors, in one process, alternating the two.

    python tools/bench_griffinlim.py [--repeats 5] [--calls 3] [--n-iter 32] [--json OUT] [--shapes all|issue]

Shapes: 256 rows of 160 000 samples' worth of frames: 2048 / 512 (313 frames x 1025 bins, cfg-2's spectrogram) and 400 / 160 (1001 x
201); with ``--shapes all`` also 2048 / 256 and 2048 / 1024, the other two hops of the fused inverse.  ``n_iter`` iterations at
momentum 0.99 from ``1 + 0j``.  A block is ``--calls`` calls between two device events after a warm-up of every route; ``--repeats``
alternating blocks give median / min / max and the run-to-run spread.  Per route: ms per call, launches per call (the package's
own counter; for the composite the device kernels one profiled call shows), and ms per iteration as (call at n_iter - call at 0) /
n_iter — beside a ``clone`` of one complex spectrogram, the traffic yardstick (8 bytes read and 8 written a bin).  Prints ONE JSON
line.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402
from torchaudio_contrib_amd import _composite  # noqa: E402

ROWS, LENGTH = 256, 160000
SHAPES = {'issue': ((2048, 512), (400, 160)), 'all': ((2048, 512), (2048, 256), (2048, 1024), (400, 160))}
MOMENTUM = 0.99


def block(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def summary(t):
    med = statistics.median(t)
    return {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4), 'spread': round((max(t) - min(t)) / med, 4)}


def device_kernels(fn):
    """device kernels of one call, by the profiler; None where it is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(e.count for e in prof.key_averages() if getattr(e, 'device_time_total', 0) > 0))
    except Exception:                                       # noqa: BLE001 — a figure of the report, not of the result
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--n-iter', type=int, default=32)
    ap.add_argument('--shapes', default='issue', choices=sorted(SHAPES))
    ap.add_argument('--json', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_griffinlim.py measures on the GPU only'
    m = MOMENTUM / (1 + MOMENTUM)
    result = {'rows': ROWS, 'samples': LENGTH, 'n_iter': a.n_iter, 'momentum': MOMENTUM, 'repeats': a.repeats, 'calls_per_block': a.calls,
              'shapes': []}
    for n_fft, hop in SHAPES[a.shapes]:
        window = torch.hann_window(n_fft, device='cuda')
        gen = torch.Generator(device='cuda').manual_seed(n_fft + hop)
        wave = torch.rand((ROWS, LENGTH), device='cuda', generator=gen) * 2 - 1
        spec = tac.complex_norm(tac.stft(wave, n_fft, hop, window=window), 2.0).contiguous()      # (rows, F, T), time-contiguous, power 2
        z = tac.stft(wave, n_fft, hop, window=window).transpose(-3, -2)
        del wave

        def hip(n_iter):
            return lambda: tac._hip.griffinlim(spec, window, None, n_fft, hop, n_fft, 2.0, n_iter, m, None)

        def composite(n_iter):
            return lambda: _composite.griffinlim(spec, window, None, n_fft, hop, n_fft, 2.0, n_iter, m, None)

        routes = {'update': hip(a.n_iter), 'update_0': hip(0), 'composite': composite(a.n_iter), 'composite_0': composite(0),
                  'clone': lambda: z.clone()}
        launches, names = {}, {}
        for name, fn in routes.items():                            # warm-up, and the launches of one call
            fn()
            if name == 'update':
                before = dict(tac._hip.launches)
                fn()
                launches[name] = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
                names[name] = tac._hip.last_route()
        launches['composite'] = device_kernels(routes['composite'])
        torch.cuda.synchronize()
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, a.calls if name != 'clone' else 20 * a.calls))
        frames = int(spec.shape[-1])
        bins = ROWS * frames * (n_fft // 2 + 1)
        line = {'fft_length': n_fft, 'hop': hop, 'frames_per_row': frames, 'bins': bins, 'complex_spectrogram_MB': round(bins * 8 / 1e6, 1),
                'launches_per_call': launches, 'last_route': names}
        for name in routes:
            line[name] = summary(times[name])
        for name, zero in (('update', 'update_0'), ('composite', 'composite_0')):
            line[name]['ms_per_iteration'] = round((line[name]['ms_median'] - line[zero]['ms_median']) / a.n_iter, 4)
        line['composite_over_update'] = round(line['composite']['ms_median'] / line['update']['ms_median'], 3)
        result['shapes'].append(line)
        del spec, z
        torch.cuda.empty_cache()
    text = json.dumps(result)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
