#!/usr/bin/env python
"""Time ``detect_pitch_frequency`` on the gfx950 kernels (csrc/pitch.hip) against the composite route (``_composite.detect_pitch_frequency``:
torch operators, a Python loop over the lags) on the same device, in one process.

    python tools/bench_pitch.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases speech,long] [--composite-calls 3]

Shapes:

    speech      (256, 160000) at 16 kHz         10 s of mono speech, 256 utterances: F 160, L 189, 256 k frames
    long        (8, 2, 2880000) at 48 kHz       one minute of stereo, 8 programmes: F 480, L 565, 96 k frames of 16 rows

Routes:

    kernel      ``tac.detect_pitch_frequency``: one ``tac_pitch_frequency_f32`` entry, two launches
    lags        ``_hip.pitch_lags`` alone: the first launch (the second is the difference)
    composite   ``_composite.detect_pitch_frequency`` on the device: about eight launches a lag plus cat / max / unfold / median; timed
                over ``--composite-calls`` single calls after one warm-up call (0: not at all), launches counted by torch's profiler
    clone       ``x.clone()``: one read and one write of the waveform, the floor beside which the spread is reported

Batches are visited in turn, enough of them that no waveform is served from the 256 MiB last-level cache by an earlier visit; a block is
at least ``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating blocks give
median / min / max.  ``G_fma_per_s`` counts the frames x L x F products of the definition.  The routes must agree before their times
mean anything: they may differ only where two lags of a frame are closer than float32 tells apart (tests/pitch_rules.py), so the
share of bit-equal outputs is reported and held to 90 %.  Prints ONE JSON line.  Needs the GPU."""
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

CASES = {'speech': ((256, 160000), 16000), 'long': ((8, 2, 2880000), 48000)}


def block(fn, batches, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(iters):
        fn(batches[i % len(batches)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def voiced(shape, rate, gen):
    """speech-like rows: three harmonics of a fundamental that wanders between 90 and 300 Hz, 5 % noise"""
    n = shape[-1]
    lead = int(math.prod(shape[:-1]))
    f0 = 90.0 + 210.0 * torch.rand(lead, 1, device='cuda', generator=gen)
    drift = 1.0 + 0.3 * torch.sin(2.0 * math.pi * torch.arange(n, device='cuda') / (0.7 * rate)).unsqueeze(0)
    phase = 2.0 * math.pi * torch.cumsum(f0 * drift / rate, -1)
    x = torch.sin(phase) + 0.5 * torch.sin(2.0 * phase) + 0.25 * torch.sin(3.0 * phase)
    x = 0.2 * x + 0.05 * torch.randn(lead, n, device='cuda', generator=gen)
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
    assert torch.cuda.is_available(), 'bench_pitch.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(17)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}
    for case in a.cases.split(','):
        shape, rate = CASES[case]
        geo = tac._pitch.geometry(shape[-1], rate, 1e-2, 30, 85, 3400)
        nbytes = 4 * math.prod(shape)
        count = max(2, -(-600 * 1000 * 1000 // nbytes) + 1)                  # the waveforms of the batches: beyond the cache
        batches = [voiced(shape, rate, gen) for _ in range(count)]
        tac.set_strict(True)
        routes = {'clone': lambda x: x.clone(), 'kernel': lambda x: tac.detect_pitch_frequency(x, rate),
                  'lags': lambda x: tac._hip.pitch_lags(x, geo.frame, geo.max_lag, geo.lag_min)}
        frames = math.prod(shape[:-1]) * geo.n_frames
        res = {'shape': list(shape), 'sample_rate': rate, 'batches': count, 'waveform_MB': round(nbytes / 1e6, 1), 'frame': geo.frame,
               'max_lag': geo.max_lag, 'frames': frames, 'G_fma': round(frames * geo.max_lag * geo.frame / 1e9, 2),
               'plan_G_and_lds_bytes': list(tac._hip.pitch_plan(geo.n_frames, geo.frame, geo.max_lag))}
        before = dict(tac._hip.launches)
        got = routes['kernel'](batches[0])
        res['tac_entries_per_call'] = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        res['kernel_twice_equal'] = bool(torch.equal(got, routes['kernel'](batches[0])))
        res['kernel_launches_per_call'] = launches_of(lambda: routes['kernel'](batches[0]))
        assert res['kernel_twice_equal'] and res['tac_entries_per_call'] == {'tac_pitch_frequency_f32': 1}, res
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
        res['lags']['G_fma_per_s'] = round(frames * geo.max_lag * geo.frame / (res['lags']['ms_median'] * 1e-3) / 1e9, 1)
        res['kernel']['TB_per_s_of_one_read'] = round(nbytes / (res['kernel']['ms_median'] * 1e-3) / 1e12, 4)
        if a.composite_calls > 0:
            tac.set_strict(False)
            composite = lambda x: tac._composite.detect_pitch_frequency(x, rate)  # noqa: E731
            ref = composite(batches[0])                              # warm-up: the allocator's blocks and every operator's first call
            res['outputs_equal_share'] = round(float((ref == got).float().mean()), 4)
            assert res['outputs_equal_share'] >= 0.9, res
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
        del batches, got
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
