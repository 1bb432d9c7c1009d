#!/usr/bin/env python
"""Time the cascade kernel (csrc/sosfilt.hip) against the only cascade there was before it — S launches of ``tac_lfilter_f32``
with clamp off, float32 between the stages — and against a ``clone`` of the output, in one process, alternating the routes.

    python tools/bench_sosfilt.py [--repeats 7] [--min-seconds 0.3] [--json profiles/sosfilt/bench.json]

Shapes: 256 x 160000 (the waveform of benchmark config 2: more rows than workgroups) and 16 x 2 880 000 (a minute at 48 kHz: one
workgroup walks a row, so sixteen rows use sixteen CUs — the under-filled case).  Sections: the first S of four cookbook
biquads (a 4th-order Butterworth high-pass at 300 Hz and low-pass at 3400 Hz, 16 kHz), twice over for S = 8; every section is
recursive with three taps.  Routes per shape and S = 1, 2, 4, 8:

    sosfilt     one launch of tac_sosfilt_f32
    lfilter_xS  S launches of tac_lfilter_f32, each reading the previous one's float32 output
    clone       torch's copy of the output: one read and one write of the tensor

Two distinct HBM-resident inputs are visited in turn; a block is at least ``--min-seconds`` of calls between two device events,
after a warm-up of every route; ``--repeats`` alternating blocks give median / min / max.  Prints ONE JSON line (and writes it to
``--json``).  ``faster_beyond_spread`` per S: the one launch's slowest block is faster than the S launches' fastest.  Needs the
GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

SHAPES = ((256, 160000), (16, 2880000))
SECTIONS = (1, 2, 4, 8)
HBM_BYTES_PER_S = 8e12


def bandpass_sections():
    """Four cookbook biquads that band-limit to 300-3400 Hz at 16 kHz (two high-passes, two low-passes), as rows of ``sos``"""
    f = tac._filters
    designs = (f.highpass(16000, 300.0, 0.541), f.lowpass(16000, 3400.0, 0.541), f.highpass(16000, 300.0, 1.307),
               f.lowpass(16000, 3400.0, 1.307))
    return tuple(tuple(b) + tuple(a) for b, a in designs)


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
    assert torch.cuda.is_available(), 'bench_sosfilt.py measures on the GPU only'
    tac.set_strict(True)
    four = bandpass_sections()
    assert len(four) == 4 and tac._hip.sosfilt_covers(four)
    result = {'tile': tac._hip.SOSFILT_TILE, 'max_sections': tac._hip.SOSFILT_MAX_SECTIONS, 'repeats': a.repeats,
              'min_seconds': a.min_seconds, 'shapes': []}
    for shape in SHAPES:
        gen = torch.Generator(device='cuda').manual_seed(shape[0])
        waves = [torch.rand(shape, device='cuda', generator=gen) * 2 - 1 for _ in range(2)]
        samples = shape[0] * shape[1]
        line = {'shape': list(shape), 'traffic_MB': round(samples * 8 / 1e6, 1),
                'ideal_ms_at_8TB_per_s': round(samples * 8 / HBM_BYTES_PER_S * 1e3, 4), 'sections': {}}
        for count in SECTIONS:
            sos = (four + four)[:count]

            def stages(w, sos=sos):
                for row in sos:
                    w = tac._hip.lfilter_rows(w, row[:3], row[3:], False)
                return w

            routes = {'sosfilt': lambda w, sos=sos: tac._hip.sosfilt_rows(w, sos, False), 'lfilter_xS': stages,
                      'clone': lambda w: w.clone()}
            before = dict(tac._hip.launches)
            one, many = routes['sosfilt'](waves[0]), routes['lfilter_xS'](waves[0])
            launched = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
            assert launched == {'tac_sosfilt_f32': 1, 'tac_lfilter_f32': count}, launched
            differ = float((one - many).abs().max())            # float32 between the stages: the two cascades differ, a little
            iters = {}
            for name, fn in routes.items():                      # warm-up, and the block length that fills min-seconds
                block(fn, waves, 2)
                iters[name] = max(4, int(a.min_seconds * 1e3 / block(fn, waves, 4)) + 1)
            times = {name: [] for name in routes}
            for _ in range(a.repeats):
                for name, fn in routes.items():
                    times[name].append(block(fn, waves, iters[name]))
            entry = {'launches': launched, 'max_abs_difference_of_the_two_cascades': differ}
            for name in routes:
                t = times[name]
                med = statistics.median(t)
                entry[name] = {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                               'spread': round((max(t) - min(t)) / med, 4), 'iters_per_block': iters[name],
                               'TB_per_s_of_one_read_one_write': round(samples * 8 / (med * 1e-3) / 1e12, 4)}
            entry['speedup_over_lfilter_xS'] = round(statistics.median(times['lfilter_xS']) / statistics.median(times['sosfilt']), 3)
            entry['faster_beyond_spread'] = max(times['sosfilt']) < min(times['lfilter_xS'])
            line['sections'][str(count)] = entry
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
