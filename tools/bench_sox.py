#!/usr/bin/env python
"""Time the SoX-effect kernels (csrc/sox_effects.hip) against a ``clone`` of their output — the traffic yardstick: one read and one
write of the tensor — and, at a length short enough to finish, against the device composites (the loops over time in torch
operators that were the only route before), in one process, alternating the routes.

    python tools/bench_sox.py [--repeats 5] [--min-seconds 0.3] [--composite-length 2000] [--json profiles/sox_effects/bench.json]

Shapes: 256 x 160000 at 16 kHz (the waveform of benchmark config 2; the flanger sees it as 256 entries of one channel) and
8 x 2 x 2 880 000 at 48 kHz (a minute of stereo: sixteen rows, so the row-per-workgroup kernels use sixteen CUs — the under-filled
case).  Routes per shape:

    overdrive        tac_overdrive_f32, gain 20, colour 20
    phaser           tac_phaser_f32 (pointer jumping), the defaults
    phaser_seq       tac_phaser_seq_f32 (one lane per row): the ablation variant
    flanger_fir      tac_flanger_f32 with regen 0 (the defaults): the streaming FIR
    flanger_fb64     ... with regen 50, delay 10 ms: 64 slots per step
    flanger_fb1      ... with regen 50, delay 0: ONE slot per step, latency-bound by construction
    clone            torch's copy of the output

Two distinct HBM-resident inputs are visited in turn; a block is at least ``--min-seconds`` of calls between two device events
(never fewer than two calls), after a warm-up of every route; ``--repeats`` alternating blocks give median / min / max.  The
composites are timed on ``(4, composite_length)`` (``(2, 2, composite_length)`` for the flanger) by wall clock around a
synchronised call, ``--repeats`` times, and reported with their cost per sample of a row — nothing is extrapolated.  Prints ONE
JSON line (and writes it to ``--json``).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

SHAPES = (((256, 160000), 16000), ((8, 2, 2880000), 48000))
HBM_BYTES_PER_S = 8e12


def block(fn, inputs, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[i % len(inputs)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def summary(t):
    med = statistics.median(t)
    return {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4), 'spread': round((max(t) - min(t)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--composite-length', type=int, default=2000)
    ap.add_argument('--json', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_sox.py measures on the GPU only'
    H, S = tac._hip, tac._sox
    result = {'tiles': {'overdrive': H.OVERDRIVE_TILE, 'phaser': H.PHASER_TILE, 'flanger_fir': H.FLANGER_TILE, 'flanger_chunk': H.FLANGER_CHUNK},
              'repeats': a.repeats, 'min_seconds': a.min_seconds, 'shapes': [], 'composites': {}}
    tac.set_strict(True)
    for shape, rate in SHAPES:
        gen = torch.Generator(device='cuda').manual_seed(shape[0])
        waves = [(torch.rand(shape, device='cuda', generator=gen) * 2 - 1) * 0.5 for _ in range(2)]
        samples = waves[0].numel()
        channels = shape[-2] if len(shape) == 3 else 1

        def as_channels(w):
            return w if w.dim() == 3 else w.unsqueeze(1)

        L, P, table = S.phaser_plan(rate, 3.0, 0.5, True)
        plans = {'flanger_fir': S.flanger_plan(rate, 0.0, 2.0, 0.0, 71.0, 0.5, 25.0, 'sinusoidal', 'linear', channels),
                 'flanger_fb64': S.flanger_plan(rate, 10.0, 2.0, 50.0, 71.0, 0.5, 25.0, 'sinusoidal', 'linear', channels),
                 'flanger_fb1': S.flanger_plan(rate, 0.0, 2.0, 50.0, 71.0, 0.5, 25.0, 'sinusoidal', 'linear', channels)}
        assert (plans['flanger_fb64'].W, plans['flanger_fb1'].W) == (64, 1)
        g, c = S.overdrive_constants(20.0, 20.0)
        routes = {'overdrive': lambda w: H.overdrive_rows(w, g, c),
                  'phaser': lambda w: H.phaser_rows(w, table, L, 0.4, 0.74, 0.4),
                  'phaser_seq': lambda w: H.phaser_rows(w, table, L, 0.4, 0.74, 0.4, sequential=True),
                  'clone': lambda w: w.clone()}
        for name, plan in plans.items():
            routes[name] = lambda w, plan=plan: H.flanger_rows(as_channels(w), plan)
        differ = float((routes['phaser'](waves[0]) - routes['phaser_seq'](waves[0])).abs().max())
        iters = {}
        for name, fn in routes.items():
            block(fn, waves, 2)
            iters[name] = max(2, int(a.min_seconds * 1e3 / block(fn, waves, 2)) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, waves, iters[name]))
        line = {'shape': list(shape), 'sample_rate': rate, 'traffic_MB': round(samples * 8 / 1e6, 1),
                'ideal_ms_at_8TB_per_s': round(samples * 8 / HBM_BYTES_PER_S * 1e3, 4), 'phaser_delay_samples': L,
                'flanger_delay_line': {k: p.Lb for k, p in plans.items()}, 'max_abs_difference_of_the_two_phasers': differ, 'routes': {}}
        clone = statistics.median(times['clone'])
        for name in routes:
            entry = summary(times[name])
            entry['iters_per_block'] = iters[name]
            entry['times_clone'] = round(entry['ms_median'] / clone, 2)
            entry['TB_per_s_of_one_read_one_write'] = round(samples * 8 / (entry['ms_median'] * 1e-3) / 1e12, 4)
            line['routes'][name] = entry
        line['phaser_jumping_faster_beyond_spread'] = max(times['phaser']) < min(times['phaser_seq'])
        line['phaser_seq_over_jumping'] = round(statistics.median(times['phaser_seq']) / statistics.median(times['phaser']), 3)
        result['shapes'].append(line)
        del waves
        torch.cuda.empty_cache()
    # ---- the device composites, at a length short enough to finish
    tac.set_strict(False)
    n = a.composite_length
    x2 = torch.rand(4, n, device='cuda') - 0.5
    x3 = torch.rand(2, 2, n, device='cuda') - 0.5
    composites = {'overdrive': lambda: tac._composite.overdrive(x2, 20.0, 20.0),
                  'phaser': lambda: tac._ops._phaser_cpu(x2, 16000.0, 0.4, 0.74, 3.0, 0.4, 0.5, True),
                  'flanger': lambda: tac._ops._flanger_cpu(x3, 16000.0, 0.0, 2.0, 50.0, 71.0, 0.5, 25.0, 'sinusoidal', 'linear')}
    kernels = {'overdrive': lambda: tac.overdrive(x2), 'phaser': lambda: tac.phaser(x2, 16000.0),
               'flanger': lambda: tac.flanger(x3, 16000.0, regen=50.0)}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', tac.CompositeRouteWarning)
        for name, fn in composites.items():
            entry = {}
            for what, f in (('composite', fn), ('kernel', kernels[name])):
                f()
                torch.cuda.synchronize()
                t = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    t.append((time.perf_counter() - t0) * 1e3)
                entry[what] = summary(t)
            entry['length'] = n
            entry['rows'] = 4
            entry['composite_us_per_sample_of_a_row'] = round(entry['composite']['ms_median'] * 1e3 / n, 3)
            entry['composite_over_kernel_at_this_length'] = round(entry['composite']['ms_median'] / entry['kernel']['ms_median'], 1)
            result['composites'][name] = entry
    text = json.dumps(result)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
