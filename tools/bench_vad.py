#!/usr/bin/env python
"""Time ``vad_start`` on the gfx950 kernels (csrc/vad.hip behind ``tac_spectrogram_f32``) against the composite route
(``_composite.vad_measures`` / ``_composite.vad_start``: torch operators, one loop over the frames and one over the search) on the same
device, in one process.

    python tools/bench_vad.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases speech,long] [--composite-calls 3]

Shapes (every row is silent — 0.001 noise — for its first 2 s, so that no route is flattered by an early trigger: the reference's
own loop would stop there, these routes measure the whole row either way):

    speech      (256, 160000) at 16 kHz         10 s of mono speech, 256 utterances, ``joint='none'``: 199 frames a row, dft 2048
    long        (8, 2, 2880000) at 48 kHz       one minute of stereo, 8 programmes, ``joint='channel'``: 1199 frames of 16 rows, dft 8192

Routes:

    kernel      ``tac.vad_start``: the padded copy of the rows, ``tac_spectrogram_f32``, and one ``tac_vad_start_f32`` entry of two launches
    spectrum    ``_hip.vad_magnitudes`` alone: the copy and launch 1
    measures    ``_hip.vad_measures_of`` alone on a spectrum made beforehand: launch 2 (launch 3 is what is left of ``kernel``)
    composite   ``_composite.vad_measures`` + ``_composite.vad_start`` on the device, timed over ``--composite-calls`` single calls after
                one warm-up call (0: not at all), launches counted by torch's profiler
    clone       ``x.clone()``: one read and one write of the waveform, the floor beside which the spread is reported

Batches are visited in turn, enough of them that no waveform is served from the 256 MiB last-level cache by an earlier visit; a block is
at least ``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating blocks give
median / min / max.  The routes must agree before their times mean anything: the share of equal ``start`` values is reported and held
to 90 % (they may differ where a measure is closer to a threshold than float32 tells apart: tests/vad_rules.py).  ``TAC_AMD_LIB``
selects another build of the library (the tile-length A/B of tools/ablation/README.md).  Prints ONE JSON line.  Needs the GPU."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

CASES = {'speech': ((256, 160000), 16000, 'none'), 'long': ((8, 2, 2880000), 48000, 'channel')}


def block(fn, batches, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(iters):
        fn(batches[i % len(batches)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def speech(shape, rate, gen):
    """rows of 2 s of 0.001 noise, then bursts of a 19-harmonic voice (0.6 s on, 0.4 s off, a fundamental of 100 … 220 Hz a row) in
    0.01 noise"""
    n = shape[-1]
    lead = int(math.prod(shape[:-1]))
    t = torch.arange(n, device='cuda') / rate
    f0 = 100.0 + 120.0 * torch.rand(lead, 1, device='cuda', generator=gen)
    voice = torch.zeros(lead, n, device='cuda')
    for h in range(1, 20):
        voice += torch.sin(2.0 * math.pi * h * f0 * t)
    offset = torch.rand(lead, 1, device='cuda', generator=gen)
    gate = ((t >= 2.0) & (((t - 2.0 + offset) % 1.0) < 0.6)).float()
    level = torch.where(t >= 2.0, 0.01, 0.001)
    x = 0.3 / 19 * voice * gate + level * torch.randn(lead, n, device='cuda', generator=gen)
    return x.reshape(shape)


def launches_of(fn):
    """device kernels launched by one call, counted by torch's profiler"""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    except RuntimeError:
        return None                                                 # (no tracer on this machine)
    return sum(e.count for e in prof.key_averages() if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower()
               and 'memcpy' not in e.key.lower() and 'memset' not in e.key.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--json', default='')
    ap.add_argument('--cases', default='speech,long')
    ap.add_argument('--composite-calls', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_vad.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(17)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count, 'library': os.path.basename(tac._native.LIB_PATH)}
    args = tac._vad.resolve(tac._vad.DEFAULTS)
    for case in a.cases.split(','):
        shape, rate, joint = CASES[case]
        p = tac._vad.plan(rate, *args)
        lead, channels = tac._vad.groups(shape, joint)
        nbytes = 4 * math.prod(shape)
        count = max(2, -(-600 * 1000 * 1000 // nbytes) + 1)                  # the waveforms of the batches: beyond the cache
        batches = [speech(shape, rate, gen) for _ in range(count)]
        spectra = {id(x): tac._hip.vad_magnitudes(x, p) for x in batches}
        tac.set_strict(True)
        routes = {'clone': lambda x: x.clone(), 'kernel': lambda x: tac.vad_start(x, rate, joint=joint),
                  'spectrum': lambda x: tac._hip.vad_magnitudes(x, p), 'measures': lambda x: tac._hip.vad_measures_of(spectra[id(x)], p)}
        frames = tac._vad.frames(shape[-1], p)
        rows = math.prod(shape[:-1])
        res = {'shape': list(shape), 'sample_rate': rate, 'joint': joint, 'batches': count, 'waveform_MB': round(nbytes / 1e6, 1),
               'frames_a_row': frames, 'rows': rows, 'dft': p.dft, 'spectrum_bins': p.s1 - p.s0, 'cepstrum_bins': p.c1 - p.c0,
               'spectrum_MB': round(4 * rows * frames * (p.dft // 2 + 1) / 1e6, 1),
               'plan_bins_per_lane_parts_lds_bytes': list(tac._hip.vad_limits(p)[:3])}
        before = dict(tac._hip.launches)
        got = routes['kernel'](batches[0])
        res['tac_entries_per_call'] = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        again = routes['kernel'](batches[0])
        res['kernel_twice_equal'] = bool(torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]))
        res['kernel_launches_per_call'] = launches_of(lambda: routes['kernel'](batches[0]))
        res['triggered_share'] = round(float(got[1].float().mean()), 4)
        res['start_seconds_min_max'] = [round(float(got[0].min()) / rate, 3), round(float(got[0].max()) / rate, 3)]
        assert res['kernel_twice_equal'] and res['tac_entries_per_call'] == {'tac_spectrogram_f32': 1, 'tac_vad_start_f32': 1}, res
        iters = {}
        for name, fn in routes.items():                            # warm-up, and the block length that fills min-seconds
            block(fn, batches, count)
            per_call = block(fn, batches, count)
            iters[name] = max(count, int(a.min_seconds * 1e3 / per_call) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, batches, iters[name]))
        for name in routes:
            t = times[name]
            res[name] = {'ms_median': round(statistics.median(t), 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                         'iters_per_block': iters[name]}
        cl = res['clone']
        res['clone_spread'] = round((cl['ms_max'] - cl['ms_min']) / cl['ms_median'], 4)
        cl['TB_per_s'] = round(2 * nbytes / (cl['ms_median'] * 1e-3) / 1e12, 3)
        res['measures']['TB_per_s_of_the_spectrum_read'] = round(4 * rows * frames * (p.dft // 2 + 1) / (res['measures']['ms_median'] * 1e-3) / 1e12, 3)
        res['decide_ms_by_difference'] = round(res['kernel']['ms_median'] - res['spectrum']['ms_median'] - res['measures']['ms_median'], 4)
        if a.composite_calls > 0:
            tac.set_strict(False)

            def composite(x):
                meas = tac._composite.vad_measures(x, p)
                return tac._composite.vad_start(meas.reshape(math.prod(lead), channels, meas.shape[-1]), p, x.shape[-1])

            ref = composite(batches[0])                              # warm-up: the allocator's blocks and every operator's first call
            res['starts_equal_share'] = round(float((ref[0].reshape(-1) == got[0].reshape(-1)).float().mean()), 4)
            assert res['starts_equal_share'] >= 0.9, res
            del ref
            single = []
            for i in range(a.composite_calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                composite(batches[i % count])
                torch.cuda.synchronize()
                single.append((time.perf_counter() - t0) * 1e3)
            res['composite'] = {'ms_single_calls': [round(t, 1) for t in single], 'launches_per_call': launches_of(lambda: composite(batches[0]))}
            res['composite_over_kernel'] = round(min(single) / res['kernel']['ms_median'], 1)
            tac.set_strict(True)
        else:
            res['composite'] = 'not measured'
        line[case] = res
        del batches, got, again, spectra
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
