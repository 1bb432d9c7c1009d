#!/usr/bin/env python
"""Time ``simulate_rir_ism_batch`` on the gfx950 kernel (csrc/rir.hip) against the composite route (``_composite.rir_ism``: the definition
in float64 torch operators, a ``(rooms, bands, images, channels, taps)`` tensor summed with ``index_add``) on the same device, in one
process, and the reverberation chain ``simulate_rir_ism_batch → fftconvolve`` against ``fftconvolve`` alone.

    python tools/bench_rir.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases train,array,chain] [--composite-calls 3]

Shapes (rooms of 4 … 9 m by 3 … 7 m by 2.5 … 4 m drawn per entry, the source and the microphones inside, absorption 0.2 … 0.5 per room):

    train       256 rooms, 4 channels, order 10 (1561 images), 8000 samples at 16 kHz       a training batch, one room an utterance
    array       8 rooms, 8 channels, order 17 (7175 images), 16000 samples at 16 kHz        long responses of a microphone array
    chain       256 rooms, 1 channel, order 10, 8000 samples, into ``fftconvolve`` with a (256, 1, 160000) batch of 10 s utterances

Routes:

    kernel      ``tac.simulate_rir_ism_batch(…, output_length=n)``: one ``tac_rir_ism_f32`` launch
    tile_N      ``_hip.rir_ism`` with the tile (the samples of a row a wave owns) given by hand, N = 128 … 2048: the A/B behind the launch's
                own choice (``res['tile']``); all give the kernel's bits
    span        ``tac_amd::rir_ism_span`` alone: the launch ``output_length=None`` adds (its host read is not in the time)
    composite   ``_composite.rir_ism`` on the device, timed over ``--composite-calls`` single calls after one warm-up call (0: not at all),
                launches counted by torch's profiler
    chain       the simulation and ``fftconvolve``; ``convolve`` is ``fftconvolve`` alone on responses made beforehand

A block is at least ``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating
blocks give median / min / max.  The routes must agree before their times mean anything: the largest difference between kernel and
composite is reported relative to the largest sample and held to 1e-6.  ``TAC_AMD_LIB`` selects another build of the library.
Prints ONE JSON line.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

CASES = {'train': (256, 4, 10, 8000), 'array': (8, 8, 17, 16000), 'chain': (256, 1, 10, 8000)}
CHAIN_SAMPLES = 160000


def block(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def rooms(count, channels, gen):
    lo, hi = torch.tensor([4.0, 3.0, 2.5], device='cuda'), torch.tensor([9.0, 7.0, 4.0], device='cuda')
    room = lo + (hi - lo) * torch.rand(count, 3, device='cuda', generator=gen)
    source = room * (0.1 + 0.8 * torch.rand(count, 3, device='cuda', generator=gen))
    mics = room[:, None, :] * (0.1 + 0.8 * torch.rand(count, channels, 3, device='cuda', generator=gen))
    absorption = 0.2 + 0.3 * torch.rand(count, 1, 6, device='cuda', generator=gen)
    return room, source, mics, absorption


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


def timed(routes, repeats, min_seconds):
    iters = {}
    for name, fn in routes.items():                                # warm-up, and the block length that fills min-seconds
        block(fn, 2)
        per_call = block(fn, 3)
        iters[name] = max(3, int(min_seconds * 1e3 / per_call) + 1)
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            times[name].append(block(fn, iters[name]))
    return {name: {'ms_median': round(statistics.median(t), 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                   'iters_per_block': iters[name]} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--json', default='')
    ap.add_argument('--cases', default='train,array,chain')
    ap.add_argument('--composite-calls', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_rir.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(23)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count, 'library': os.path.basename(tac._native.LIB_PATH),
            'min_tile_bands_taps_order': list(tac._hip.rir_limits())}
    for case in a.cases.split(','):
        count, channels, order, n = CASES[case]
        room, source, mics, absorption = rooms(count, channels, gen)
        images = tac._rir.n_images(order, 3)
        res = {'rooms': count, 'channels': channels, 'max_order': order, 'images': images, 'output_length': n,
               'taps_M': round(count * channels * images * 81 / 1e6, 1), 'output_MB': round(4 * count * channels * n / 1e6, 2)}
        tac.set_strict(True)

        def kernel():
            return tac.simulate_rir_ism_batch(room, source, mics, order, absorption, n)

        before = dict(tac._hip.launches)
        got = kernel()
        res['tac_entries_per_call'] = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        res['kernel_twice_equal'] = bool(torch.equal(got.view(torch.int32), kernel().view(torch.int32)))
        res['kernel_launches_per_call'] = launches_of(kernel)
        res['natural_length'] = int(tac._ops.call('rir_ism_span', room, source, mics, order, 81, 343.0, 16000.0))
        assert res['kernel_twice_equal'] and res['tac_entries_per_call'] == {'tac_rir_ism_f32': 1}, res
        if case == 'chain':
            x = torch.randn(count, 1, CHAIN_SAMPLES, device='cuda', generator=gen)
            routes = {'kernel': kernel, 'convolve': lambda: tac.fftconvolve(x, got), 'chain': lambda: tac.fftconvolve(x, kernel())}
            res['waveform_MB'] = round(4 * count * CHAIN_SAMPLES / 1e6, 1)
        else:
            routes = {'kernel': kernel, 'span': lambda: tac._ops.call('rir_ism_span', room, source, mics, order, 81, 343.0, 16000.0)}
        res['tile'] = tac._hip.rir_tile(count * channels, n, 1)[0]
        if case != 'chain':                                          # the tile A/B: the launch with every tile given by hand, same process
            for tile in (128, 256, 512, 1024, 2048):
                routes['tile_%d' % tile] = lambda tile=tile: tac._hip.rir_ism(room, source, mics, absorption, order, 40, n, 81, 343.0, 16000.0, tile)
                assert torch.equal(routes['tile_%d' % tile]()[:, 0].view(torch.int32), got.view(torch.int32)), tile
        res.update(timed(routes, a.repeats, a.min_seconds))
        res['kernel']['G_taps_per_s'] = round(count * channels * images * 81 / (res['kernel']['ms_median'] * 1e-3) / 1e9, 1)
        if case == 'chain':
            res['chain_over_convolve'] = round(res['chain']['ms_median'] / res['convolve']['ms_median'], 3)
        elif a.composite_calls > 0:
            tac.set_strict(False)

            def composite():
                return tac._composite.rir_ism(room, source, mics, absorption, order, 40, n, 81, 343.0, 16000.0)[:, 0]

            ref = composite()                                        # warm-up: the allocator's blocks and every operator's first call
            res['kernel_composite_max_diff_over_peak'] = float((ref - got).abs().max() / ref.abs().max())
            assert res['kernel_composite_max_diff_over_peak'] <= 1e-6, res
            del ref
            single = []
            for _ in range(a.composite_calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                composite()
                torch.cuda.synchronize()
                single.append((time.perf_counter() - t0) * 1e3)
            res['composite'] = {'ms_single_calls': [round(t, 1) for t in single], 'launches_per_call': launches_of(composite),
                                'peak_GB': round(torch.cuda.max_memory_allocated() / 1e9, 1)}
            res['composite_over_kernel'] = round(min(single) / res['kernel']['ms_median'], 1)
            tac.set_strict(True)
        else:
            res['composite'] = 'not measured'
        line[case] = res
        del got
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
