#!/usr/bin/env python
"""Time SpecAugment on the gfx950 kernel (csrc/specaug.hip) against the package's composite route of the same call and against
``x.clone()`` of the same tensor, in one process, alternating the routes.

    python tools/bench_specaug.py [--repeats 7] [--min-seconds 0.2] [--json OUT] [--profile CASE:ROUTE]

Shapes (freq, time last two unless said otherwise):

    fbank       (256, 80, 1000)        80 mel bins x 1000 frames, contiguous: 16-byte loads
    kaldi       (256, 1000, 80)        the Kaldi layout (time, freq) masked where it lies: time spans on axis 1, frequency spans on axis 2
    kaldi_T     (256, 1000, 80).mT     the same storage through ``SpecAugment`` as the (…, freq, time) view: the turned load
    ast         (256, 1, 128, 3000)    128 bins x 3000 frames with a channel axis

Mask sets: ``2x100+2x27`` = SpecAugment(2, 100, 2, 27) and ``10x50+2x27`` = SpecAugment(10, 50, 2, 27, p=0.2), iid masks, zero masking
off (the fill is the input's mean, read by the kernel on the device).

Routes: ``kernel`` (one ``tac_mask_spans_f32`` launch), ``composite`` (``_composite.mask_spans``: one ``masked_fill`` pass per mask,
in torch operators) and ``clone`` (``x.clone()`` into the dense layout the kernel writes: one read and one write of the same bytes by
code that is not this project's — the floor of any copy).  Two timings per route: ``pass`` — the data pass alone on a span table
made beforehand — and ``call`` — the whole call with its draws, the mean and the table, between device events, with the host's
wall time per call beside it.  Launch counts per call come from ``torch.profiler`` (every device kernel, torch's included).

Inputs are visited in turn, enough of them to exceed the 256 MiB last-level cache several times over; a block is at least
``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating blocks give median / min /
max.  The spread of ``clone`` is reported first: the differences between routes mean nothing below it.  Prints ONE JSON line.
``--profile fbank:2x100+2x27:kernel`` runs only that route a few times (for ``rocprofv3 --kernel-trace --stats``).  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

S, C = tac._specaug, tac._composite
MASK_SETS = {'2x100+2x27': (2, 100, 2, 27, 1.0), '10x50+2x27': (10, 50, 2, 27, 0.2)}


def block(fn, inputs, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for i in range(iters):
        fn(inputs[i % len(inputs)])
    stop.record()
    host = (time.perf_counter() - t0) / iters
    stop.synchronize()
    return start.elapsed_time(stop) / iters, host * 1e3


def spans_of(x, masks, time_on_a):
    """the span table of one call, drawn as SpecAugment draws it: ``(table, k_a)``"""
    n_t, t_param, n_f, f_param, p = masks
    n_a, n_b = int(x.shape[-2]), int(x.shape[-1])
    n_time, n_freq = (n_a, n_b) if time_on_a else (n_b, n_a)
    t_pair = S.draws_iid(x, n_t, S.clamp_param(t_param, n_time, p), n_time)
    f_pair = S.draws_iid(x, n_f, f_param, n_freq)
    return S.table(t_pair, f_pair, x) if time_on_a else S.table(f_pair, t_pair, x)


def device_kernels(fn, x):
    """device kernels of one call, or None where the profiler is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(x)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(x)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
    except Exception:                                   # noqa: BLE001 — a count that cannot be taken is reported as such
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--json', default='')
    ap.add_argument('--profile', default='')
    ap.add_argument('--rows', type=int, default=256)
    ap.add_argument('--no-launch-counts', action='store_true')
    ap.add_argument('--passes-only', action='store_true', help='clone and the kernel data pass alone')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_specaug.py measures on the GPU only'
    tac.set_strict(True)
    gen = torch.Generator(device='cuda').manual_seed(80)
    shapes = {'fbank': ((a.rows, 80, 1000), False, False), 'kaldi': ((a.rows, 1000, 80), True, False),
              'kaldi_T': ((a.rows, 1000, 80), False, True), 'ast': ((a.rows, 1, 128, 3000), False, False)}
    line = {'rows': a.rows, 'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0)}
    only = a.profile.split(':') if a.profile else None
    for case, (shape, time_on_a, turned) in shapes.items():
        if only and only[0] != case:
            continue
        nbytes = 4
        for n in shape:
            nbytes *= n
        count = max(2, -(-800 * 1000 * 1000 // nbytes))
        inputs = [torch.randn(shape, device='cuda', generator=gen) + 5.0 for _ in range(count)]
        if turned:
            inputs = [x.transpose(-1, -2) for x in inputs]
        res = {'shape': list(inputs[0].shape), 'strides': list(inputs[0].stride()), 'inputs': count, 'moved_MB': round(2 * nbytes / 1e6, 1)}
        clone = lambda x: x.clone(memory_format=torch.contiguous_format)          # noqa: E731
        for set_name, masks in MASK_SETS.items():
            if only and only[1] != set_name:
                continue
            torch.manual_seed(1)
            tables = [spans_of(x, masks, time_on_a) for x in inputs]
            means = [x.mean() for x in inputs]
            by_ptr = {x.data_ptr(): i for i, x in enumerate(inputs)}

            def pass_kernel(x):
                i = by_ptr[x.data_ptr()]
                return tac._ops.call('mask_spans', x, tables[i][0], tables[i][1], means[i], 0.0)

            def pass_composite(x):
                i = by_ptr[x.data_ptr()]
                return C.mask_spans(x, tables[i][0], tables[i][1], means[i])

            def call_kernel(x):
                spans, k_a = spans_of(x, masks, time_on_a)
                return tac._ops.call('mask_spans', x, spans, k_a, x.mean(), 0.0)

            def call_composite(x):
                spans, k_a = spans_of(x, masks, time_on_a)
                return C.mask_spans(x, spans, k_a, x.mean())

            layer = tac.SpecAugment(*masks[:4], p=masks[4])
            if not time_on_a:
                call_kernel = layer                                                # the layer itself: (…, freq, time)
            routes = {'clone': clone, 'pass_kernel': pass_kernel, 'pass_composite': pass_composite, 'call_kernel': call_kernel,
                      'call_composite': call_composite}
            if a.passes_only:
                routes = {'clone': clone, 'pass_kernel': pass_kernel}
                for name, fn in routes.items():
                    block(fn, inputs, count)
                    t = sorted(block(fn, inputs, 40 * count)[0] for _ in range(5))
                    res[set_name + ' ' + name] = [round(v, 4) for v in t]
                continue
            if only:
                fn = routes[{'kernel': 'call_kernel', 'composite': 'call_composite', 'clone': 'clone'}[only[2]]]
                for _ in range(3):
                    for x in inputs:
                        fn(x)
                torch.cuda.synchronize()
                return
            before = dict(tac._hip.launches)
            got = pass_kernel(inputs[0])
            launches = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
            same = bool(torch.equal(got, pass_composite(inputs[0])))
            masked_share = float((got != inputs[0]).float().mean())
            del got
            iters = {}
            for name, fn in routes.items():                        # warm-up, and the block length that fills min-seconds
                block(fn, inputs, count)
                per_call = block(fn, inputs, count)[0]
                iters[name] = max(count, int(a.min_seconds * 1e3 / per_call) + 1)
            times = {name: [] for name in routes}
            hosts = {name: [] for name in routes}
            for _ in range(a.repeats):
                for name, fn in routes.items():
                    dev_ms, host_ms = block(fn, inputs, iters[name])
                    times[name].append(dev_ms)
                    hosts[name].append(host_ms)
            out = {'k_spans': int(tables[0][0].shape[-2]), 'tac_launches_per_pass': launches, 'kernel_equals_composite': same,
                   'masked_share': round(masked_share, 4)}
            for name in routes:
                t = times[name]
                out[name] = {'ms_median': round(statistics.median(t), 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                             'host_ms_median': round(statistics.median(hosts[name]), 4), 'iters_per_block': iters[name]}
                if not a.no_launch_counts:
                    out[name]['device_kernels_per_call'] = device_kernels(routes[name], inputs[0])
            cl = out['clone']
            out['clone_spread'] = round((cl['ms_max'] - cl['ms_min']) / cl['ms_median'], 4)
            out['pass_kernel']['TB_per_s'] = round(2 * nbytes / (out['pass_kernel']['ms_median'] * 1e-3) / 1e12, 3)
            out['clone']['TB_per_s'] = round(2 * nbytes / (cl['ms_median'] * 1e-3) / 1e12, 3)
            out['pass_kernel_over_clone'] = round(out['pass_kernel']['ms_median'] / cl['ms_median'], 3)
            out['pass_composite_over_kernel'] = round(out['pass_composite']['ms_median'] / out['pass_kernel']['ms_median'], 3)
            out['call_composite_over_kernel'] = round(out['call_composite']['ms_median'] / out['call_kernel']['ms_median'], 3)
            res[set_name] = out
        line[case] = res
        del inputs
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
