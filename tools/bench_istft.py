#!/usr/bin/env python
"""Time ``istft`` on the gfx950 kernels — the fused one-launch route and the general two-launch route of csrc/istft.hip — against
``torch.istft`` on the same device tensors, in one process, alternating the routes.

    python tools/bench_istft.py [--repeats 7] [--min-seconds 0.5] [--json OUT] [--profile ROUTE]

Geometries: 256 rows x 160 000 samples at fft_length / hop 2048 / 512, 400 / 160 and 1024 / 256.  Four distinct HBM-resident
spectrograms are visited in turn; a block is at least ``--min-seconds`` of launches between two device events, after a warm-up of
both routes; ``--repeats`` alternating blocks give median / min / max and the run-to-run spread.  Prints ONE JSON line: per
geometry the ms per call of the fused route (2048 / 512), the general route (forced: ``route='general'`` of the launcher) and ``torch.istft``, the compulsory bytes (the spectrum read once, the samples written once) and the
achieved bytes/s against them as a share of 8 TB/s.  ``--profile fused|general|torch`` runs only that route a few times (for rocprofv3
--kernel-trace --stats).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

ROWS, LENGTH = 256, 160000
GEOMETRIES = ((2048, 512), (400, 160), (1024, 256))
FUSED = ((2048, 512),)
HBM_BYTES_PER_S = 8e12


def block(fn, specs, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(specs[i % len(specs)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--json', default='')
    ap.add_argument('--profile', default='')
    ap.add_argument('--routes', default='fused,general,torch', help="'general,torch' leaves the fused route out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_istft.py measures on the GPU only'
    tac.set_strict(True)
    result = {'rows': ROWS, 'samples': LENGTH, 'repeats': a.repeats, 'min_seconds': a.min_seconds, 'geometries': []}
    for n_fft, hop in GEOMETRIES:
        window = torch.hann_window(n_fft, device='cuda')
        gen = torch.Generator(device='cuda').manual_seed(n_fft)
        specs = [tac.stft(torch.rand((ROWS, LENGTH), device='cuda', generator=gen) * 2 - 1, n_fft, hop, window=window)
                 for _ in range(4)]
        views = [torch.view_as_complex(s) for s in specs]          # the same storage, as torch.istft wants it
        by_ptr = {s.data_ptr(): v for s, v in zip(specs, views)}
        def hip_route(route):
            return lambda s: tac._hip.istft(s, window, n_fft, hop, n_fft, True, False, LENGTH, route=route)
        routes = {'general': hip_route('general'),
                  'torch': lambda s: torch.istft(by_ptr[s.data_ptr()], n_fft, hop, window=window, length=LENGTH)}
        if (n_fft, hop) in FUSED and 'fused' in a.routes.split(','):
            routes = dict(fused=hip_route(None), **routes)
        route_names = {}
        for name in routes:
            if name != 'torch':
                routes[name](specs[0])
                route_names[name] = tac._native.lib().tac_last_route().decode()
        if a.profile:
            for _ in range(5):
                for s in specs:
                    routes.get(a.profile, routes['general'])(s)
            torch.cuda.synchronize()
            continue
        iters = {}
        for name, fn in routes.items():                            # warm-up, and the block length that fills min-seconds
            block(fn, specs, 4)
            per_call = block(fn, specs, 8)
            iters[name] = max(8, int(a.min_seconds * 1e3 / per_call) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, specs, iters[name]))
        frames = specs[0].shape[-2]
        compulsory = ROWS * (frames * (n_fft // 2 + 1) * 8 + LENGTH * 4)
        line = {'fft_length': n_fft, 'hop': hop, 'frames_per_row': frames, 'compulsory_MB': round(compulsory / 1e6, 1),
                'general_route_extra_MB': round(2 * ROWS * frames * n_fft * 4 / 1e6, 1), 'routes': route_names}
        for name in routes:
            t = times[name]
            med = statistics.median(t)
            line[name] = {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                          'spread': round((max(t) - min(t)) / med, 4), 'iters_per_block': iters[name],
                          'compulsory_TB_per_s': round(compulsory / (med * 1e-3) / 1e12, 3),
                          'share_of_8TB_per_s': round(compulsory / (med * 1e-3) / HBM_BYTES_PER_S, 4)}
        line['torch_over_general'] = round(line['torch']['ms_median'] / line['general']['ms_median'], 3)
        if 'fused' in line:
            line['general_over_fused'] = round(line['general']['ms_median'] / line['fused']['ms_median'], 3)
            line['fused_faster_beyond_spread'] = bool(line['fused']['ms_max'] < line['general']['ms_min'])
        result['geometries'].append(line)
        del specs, views, by_ptr
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
