#!/usr/bin/env python
"""Time ``fftconvolve`` on the gfx950 kernels — the partitioned route of csrc/fftconvolve.hip at each admissible transform length
and the direct route — against the computation it replaces, ``irfft(rfft(x, n) * rfft(y, n), n)`` at ``n = L + M - 1`` in float32
on the same device tensors, in one process, alternating the routes.

    python tools/bench_fftconvolve.py [--m 64,512,4000,16000,48000] [--repeats 7] [--min-seconds 0.5] [--json OUT] [--profile ROUTE]

256 rows x 160 000 samples, one shared decaying kernel of M taps.  Four distinct HBM-resident inputs are visited in turn; a block
is at least ``--min-seconds`` of calls between two device events, after a warm-up of every route; ``--repeats`` alternating blocks
give median / min / max and the spread.  The same tensors give the accuracy comparison: the worst per-block ratio (block N / 2,
neighbourhood N, N = 2048) of every route against the float64 one-shot form on four rows.  ``--crossover`` times the direct route
against the 2048 route for M = 32 ... 2048 (the measurement behind ``_hip.M_DIRECT``).  Prints ONE JSON line per invocation and
appends it to ``--json``.  ``--profile spectral-2048|...|direct|torch`` runs only that route a few times (for rocprofv3
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
TAPS = (64, 512, 4000, 16000, 48000)
CROSSOVER = (32, 64, 128, 256, 512, 1024, 2048)
DIRECT_MAX = 4096            # (the polyphase kernel's input span per tile ends a little above this)


def block(fn, xs, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(xs[i % len(xs)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def block_ratio(got, ref, hop=1024, n_fft=2048):
    """worst per-block error over the largest reference magnitude within n_fft of the block (tests/istft_rules.py::block_ratios)"""
    n = ref.shape[1]
    fill = (-n) % hop
    err = torch.nn.functional.pad((got.double() - ref).abs(), (0, fill)).reshape(ref.shape[0], -1, hop).amax(-1)
    mag = torch.nn.functional.pad(ref.abs(), (0, fill)).reshape(ref.shape[0], -1, hop).amax(-1)
    reach = (n_fft + hop - 1) // hop
    scale = torch.nn.functional.max_pool1d(mag[:, None, :], 2 * reach + 1, stride=1, padding=reach)[:, 0, :]
    return float((err / scale).max())


def one_shot(x, y):
    n = x.shape[-1] + y.shape[-1] - 1
    return torch.fft.irfft(torch.fft.rfft(x, n=n) * torch.fft.rfft(y, n=n), n=n)


def routes_for(m, y, crossover):
    H = tac._hip
    routes = {}
    for n in H.FFTCONV_SIZES:
        if H.fftconvolve_covers(LENGTH, m, n) and (not crossover or n == 2048):
            routes['spectral-%d' % n] = (lambda n_: lambda x: H.fftconvolve(x, y, n_))(n)
    if m <= DIRECT_MAX:
        saved = H.M_DIRECT

        def direct(x):
            H.M_DIRECT = DIRECT_MAX
            try:
                return H.fftconvolve(x, y, 0)
            finally:
                H.M_DIRECT = saved
        routes['direct'] = direct
    if not crossover:
        routes['torch'] = lambda x: one_shot(x, y)
    return routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--m', default=','.join(str(m) for m in TAPS))
    ap.add_argument('--crossover', action='store_true')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--json', default='')
    ap.add_argument('--profile', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_fftconvolve.py measures on the GPU only'
    tac.set_strict(True)
    taps = CROSSOVER if a.crossover else tuple(int(v) for v in a.m.split(','))
    result = {'rows': ROWS, 'samples': LENGTH, 'repeats': a.repeats, 'min_seconds': a.min_seconds, 'crossover': a.crossover,
              'default_rule': {str(m): tac._hip.fftconvolve_route(m, True) for m in taps}, 'kernels': []}
    gen = torch.Generator(device='cuda').manual_seed(1)
    xs = [torch.rand((ROWS, LENGTH), device='cuda', generator=gen) * 2 - 1 for _ in range(4)]
    for x in xs:                                                     # a loud start and a quiet rest: what a reverb tail follows
        x[:, LENGTH // 8:] *= 2.0 ** -10
    for m in taps:
        y = (torch.randn(1, m, device='cuda', generator=gen) * torch.exp(-6.0 * torch.arange(m, device='cuda') / m)).contiguous()
        routes = routes_for(m, y, a.crossover)
        names = {}
        for name, fn in routes.items():
            fn(xs[0])
            names[name] = tac._hip.last_route() if name != 'torch' else 'torch.fft'
        if a.profile:
            for _ in range(5):
                for x in xs:
                    routes[a.profile](x)
            torch.cuda.synchronize()
            continue
        ref = one_shot(xs[0][:4].double(), y.double())
        line = {'taps': m, 'routes': names, 'samples_out': LENGTH + m - 1}
        iters = {}
        for name, fn in routes.items():
            line[name] = {'worst_block_ratio': float('%.3g' % block_ratio(fn(xs[0][:4].contiguous()), ref))}
            block(fn, xs, 2)
            iters[name] = max(4, int(a.min_seconds * 1e3 / block(fn, xs, 4)) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, xs, iters[name]))
        for name in routes:
            t = times[name]
            med = statistics.median(t)
            line[name].update({'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                               'spread': round((max(t) - min(t)) / med, 4), 'iters_per_block': iters[name],
                               'Gsamples_per_s': round(ROWS * (LENGTH + m - 1) / (med * 1e-3) / 1e9, 2)})
        if 'torch' in routes:
            for name in routes:
                if name != 'torch':
                    line[name]['torch_over_this'] = round(line['torch']['ms_median'] / line[name]['ms_median'], 3)
        result['kernels'].append(line)
        del y, routes
        torch.cuda.empty_cache()
    if a.profile:
        return
    text = json.dumps(result)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
