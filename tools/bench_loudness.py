#!/usr/bin/env python
"""Time ``loudness`` on the gfx950 kernels (csrc/loudness.hip) against the same definition evaluated two other ways on the same device,
in one process, alternating the routes.

    python tools/bench_loudness.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases speech,long] [--composite-calls 1]

Shapes:

    speech      (256, 1, 160000) at 16 kHz      10 s of mono speech, 256 utterances
    long        (8, 2, 2880000) at 48 kHz       one minute of stereo, 8 programmes: 16 rows for 256 CUs

Routes:

    kernel      ``tac.loudness``: one ``tac_loudness_f32`` entry, two launches, the waveform read once
    pieces      the definition with this package's own kernels: ``treble_biquad`` and ``highpass_biquad`` (two ``tac_lfilter_f32``
                launches, each writing a float32 waveform) and torch's ``square`` / ``unfold`` / ``mean`` / ``log10`` / compares
    composite   ``_composite.loudness``: torch operators alone, whose recursion is a loop over time — two or three small launches a
                sample, seconds a call; timed over ``--composite-calls`` single calls, on ``speech`` only (0: not at all)
    clone       ``x.clone()``: one read and one write of the waveform, the floor beside which the spread is reported

Batches are visited in turn, enough of them that no waveform is served from the 256 MiB last-level cache by an earlier visit; a block is
at least ``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating blocks give
median / min / max.  The kernel's rate is given against the ONE read of the waveform (4 bytes a sample).  Prints ONE JSON line.  Needs
the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

CASES = {'speech': ((256, 1, 160000), 16000), 'long': ((8, 2, 2880000), 48000)}
WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)


def block(fn, batches, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(iters):
        fn(batches[i % len(batches)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def pieces(x, rate):
    """the definition with the package's own filter kernel and torch's reductions, in float32"""
    gate, step = tac._filters.loudness_blocks(rate)
    w = tac.functional.treble_biquad(x, rate, 4.0, 1500.0, 1.0 / 2.0 ** 0.5)
    w = tac.highpass_biquad(w, rate, 38.0, 0.5)
    energy = torch.square(w).unfold(-1, gate, step).mean(-1)
    g = torch.tensor(WEIGHTS[:energy.shape[-2]], device=x.device)

    def level(e):
        return -0.691 + 10.0 * torch.log10((g * e).sum(-1))

    def gated(keep):
        return (keep.unsqueeze(-2) * energy).sum(-1) / torch.count_nonzero(keep, dim=-1).unsqueeze(-1)

    l = -0.691 + 10.0 * torch.log10((g.unsqueeze(-1) * energy).sum(-2))
    keep = l > -70.0
    keep = keep & (l > (level(gated(keep)) - 10.0).unsqueeze(-1))
    return level(gated(keep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--json', default='')
    ap.add_argument('--cases', default='speech,long')
    ap.add_argument('--composite-calls', type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_loudness.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(91)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}
    for case in a.cases.split(','):
        shape, rate = CASES[case]
        nbytes = 4
        for k in shape:
            nbytes *= k
        count = max(2, -(-600 * 1000 * 1000 // nbytes) + 1)                  # the waveforms of the batches: beyond the cache
        # speech-like levels: noise at 0.05 with a quiet second half in every other entry, so both gates have work
        batches = []
        for _ in range(count):
            x = torch.randn(shape, device='cuda', generator=gen) * 0.05
            x[::2, ..., shape[-1] // 2:] *= 0.01
            batches.append(x)
        tac.set_strict(True)
        routes = {'clone': lambda x: x.clone(), 'kernel': lambda x: tac.loudness(x, rate), 'pieces': lambda x: pieces(x, rate)}
        res = {'shape': list(shape), 'sample_rate': rate, 'batches': count, 'waveform_MB': round(nbytes / 1e6, 1)}
        before = dict(tac._hip.launches)
        got = routes['kernel'](batches[0])
        res['tac_entries_per_call'] = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        res['max_abs_kernel_minus_pieces_dB'] = float((got - routes['pieces'](batches[0])).abs().max())
        res['kernel_twice_equal'] = bool(torch.equal(got, routes['kernel'](batches[0])))
        # the routes have to agree before their times mean anything: float32 filter outputs and float32 sums of `gate` terms
        # leave the pieces within (gate + 64) 2^-24 of the energy, 10 / ln 10 times that in dB, with a factor 4 of room
        gate = tac._filters.loudness_blocks(rate)[0]
        res['agreement_limit_dB'] = 4 * 4.343 * (gate + 64) * 2.0 ** -24
        assert res['kernel_twice_equal'] and res['max_abs_kernel_minus_pieces_dB'] <= res['agreement_limit_dB'], res
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
        res['kernel']['TB_per_s_of_one_read'] = round(nbytes / (res['kernel']['ms_median'] * 1e-3) / 1e12, 4)
        res['pieces_over_kernel'] = round(res['pieces']['ms_median'] / res['kernel']['ms_median'], 3)
        if case == 'speech' and a.composite_calls > 0:
            tac.set_strict(False)
            single = []
            for i in range(a.composite_calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = tac._composite.loudness(batches[i % count], rate)
                torch.cuda.synchronize()
                single.append((time.perf_counter() - t0) * 1e3)
            res['composite'] = {'ms_single_calls': [round(t, 1) for t in single]}
            res['composite_over_kernel'] = round(min(single) / res['kernel']['ms_median'], 1)
            res['max_abs_kernel_minus_composite_dB'] = float((routes['kernel'](batches[(a.composite_calls - 1) % count]) - ref).abs().max())
            assert res['max_abs_kernel_minus_composite_dB'] <= res['agreement_limit_dB'], res
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
