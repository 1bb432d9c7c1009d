#!/usr/bin/env python
"""Time the ``MVDR`` layer on the gfx950 kernels (csrc/beamform.hip) against the composite route (``_composite.mvdr_souden``: torch
operators, an einsum that materialises ``(…, freq, time, ch, ch)`` per mask) on the same device, in one process.

    python tools/bench_beamform.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases array,long] [--composite-calls 2]

Shapes (batch, channels, bins, frames), frame-major as ``stft`` returns them:

    array       (16, 8, 257, 1000)      16 utterances of 10 s from 8 microphones at fft_length 512
    long        (8, 8, 2049, 2813)      the multichannel row of BASELINE configs[3]: one minute at 48 kHz, fft_length 4096

Routes:

    kernel      ``tac.MVDR()(spec, mask_s)``: one ``tac_mvdr_souden_f32`` entry, three launches; mask_n is the complement
    two_masks   ``tac.MVDR()(spec, mask_s, mask_n)``: the same entry reading a second mask
    psd / apply the PSD launch pair (both masks, ``_hip.psd``) and the apply launch (``_hip.apply_beamforming``) by themselves
    composite   ``_composite.mvdr_souden`` on the device, timed over ``--composite-calls`` single calls after one warm-up call
                (0: not at all), launches counted by torch's profiler
    clone       ``spec.clone()``: one read and one write of the spectrogram, the floor beside which the spread is reported

The algorithmic traffic of ``kernel`` is two reads of the spectrogram, one of the mask and one write of the output; ``share_of_8TBps``
is that traffic over the median time over 8 TB/s.  The pieces of the PSD launch (written once, read once) are reported beside it as
``scratch_MB`` and are not counted.  Batches are visited in turn, enough of them that no spectrogram is served from the 256 MiB
last-level cache by an earlier visit; a block is at least ``--min-seconds`` of calls between two device events after a warm-up of every
route; ``--repeats`` alternating blocks give median / min / max.  Prints ONE JSON line.  Needs the GPU."""
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

CASES = {'array': (16, 8, 257, 1000), 'long': (8, 8, 2049, 2813)}


def block(fn, batches, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(iters):
        fn(*batches[i % len(batches)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def scene(shape, gen):
    """(frame-major pairs (B, C, F, T, 2), mask_s, mask_n (B, F, T)): one source through a steering vector plus noise at 0.3"""
    B, C, F, T = shape
    steer = torch.randn(B, C, 1, F, 2, device='cuda', generator=gen)
    source = torch.randn(B, 1, T, F, 2, device='cuda', generator=gen)
    x = torch.view_as_real(torch.view_as_complex(steer) * torch.view_as_complex(source))
    x = x + 0.3 * torch.randn(B, C, T, F, 2, device='cuda', generator=gen)
    ms = 0.02 + 0.96 * torch.rand(B, F, T, device='cuda', generator=gen)
    mn = 0.02 + 0.96 * torch.rand(B, F, T, device='cuda', generator=gen)
    return x.transpose(2, 3), ms, mn


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
    ap.add_argument('--cases', default='array,long')
    ap.add_argument('--composite-calls', type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_beamform.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(23)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}
    mvdr = tac.MVDR()
    for case in a.cases.split(','):
        shape = CASES[case]
        B, C, F, T = shape
        spec_bytes, mask_bytes, out_bytes = 8 * B * C * F * T, 4 * B * F * T, 8 * B * F * T
        count = max(2, -(-600 * 1000 * 1000 // spec_bytes) + 1)              # the spectrograms of the batches: beyond the cache
        batches = [scene(shape, gen) for _ in range(count)]
        tac.set_strict(True)
        chunks = tac._hip.psd_chunks(T)
        weights = tac._hip.mvdr_souden(batches[0][0], batches[0][1], None, None, 0, True, 1e-7, 1e-8, 1e-15)[1]
        routes = {'clone': lambda x, ms, mn: x.clone(), 'kernel': lambda x, ms, mn: mvdr(x, ms),
                  'two_masks': lambda x, ms, mn: mvdr(x, ms, mn),
                  'psd': lambda x, ms, mn: tac._hip.psd(x, ms, None, complement=True, normalize=True, eps=1e-15),
                  'apply': lambda x, ms, mn: tac._hip.apply_beamforming(weights, x)}
        traffic = 2 * spec_bytes + mask_bytes + out_bytes
        res = {'shape': list(shape), 'batches': count, 'spec_MB': round(spec_bytes / 1e6, 1), 'traffic_MB': round(traffic / 1e6, 1),
               'pieces': chunks, 'scratch_MB': round(2 * chunks * B * F * (4 * C * C + 8) / 1e6, 1)}
        before, layout = dict(tac._hip.launches), dict(tac._hip.beamform_layout)
        got = routes['kernel'](*batches[0])
        res['tac_entries_per_call'] = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        res['spec_read_in_place'] = tac._hip.beamform_layout['copied'] == layout['copied']
        res['kernel_twice_equal'] = bool(torch.equal(got, routes['kernel'](*batches[0])))
        res['kernel_launches_per_call'] = launches_of(lambda: routes['kernel'](*batches[0]))
        assert res['kernel_twice_equal'] and res['spec_read_in_place'] and res['tac_entries_per_call'] == {'tac_mvdr_souden_f32': 1}, res
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
        cl['TB_per_s'] = round(2 * spec_bytes / (cl['ms_median'] * 1e-3) / 1e12, 3)
        for name, nbytes in (('kernel', traffic), ('two_masks', traffic + mask_bytes), ('psd', spec_bytes + mask_bytes),
                             ('apply', spec_bytes + out_bytes)):
            rate = nbytes / (res[name]['ms_median'] * 1e-3) / 1e12
            res[name]['TB_per_s'] = round(rate, 3)
            res[name]['share_of_8TBps'] = round(rate / 8.0, 3)
        res['kernel_over_clone'] = round(res['kernel']['ms_median'] / cl['ms_median'], 2)
        if a.composite_calls > 0:
            tac.set_strict(False)
            none = tac._beamform.none(batches[0][0])
            composite = lambda x, ms, mn: tac._composite.mvdr_souden(x, ms, none, none, 0, True, 1e-7, 1e-8, 1e-15)  # noqa: E731
            ref = composite(*batches[0])                             # warm-up: the allocator's blocks and every operator's first call
            res['max_abs_difference_over_max'] = float((ref - got).abs().max() / ref.abs().max())
            del ref
            single = []
            for i in range(a.composite_calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                composite(*batches[i % count])
                torch.cuda.synchronize()
                single.append((time.perf_counter() - t0) * 1e3)
            res['composite'] = {'ms_single_calls': [round(t, 1) for t in single],
                                'launches_per_call': launches_of(lambda: composite(*batches[0]))}
            res['composite_over_kernel'] = round(min(single) / res['kernel']['ms_median'], 1)
            tac.set_strict(True)
        else:
            res['composite'] = 'not measured'
        line[case] = res
        del batches, got, weights
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
