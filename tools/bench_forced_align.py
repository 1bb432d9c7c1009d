#!/usr/bin/env python
"""Time ``forced_align`` on the gfx950 kernel (csrc/align.hip) — one launch — against the package's own torch-operator composite
on the device (several launches per frame: the baseline to beat) and the composite on the host CPU with the transfers included
(what people do today), in one process.

    python tools/bench_forced_align.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases long,vocab,batch] [--composite-calls 2]

Shapes (batch, time, target, class):

    long        (1, 3000, 200, 32)      a 60 s utterance at 20 ms frames, characters
    vocab       (1, 1500, 60, 5000)     word pieces: the emissions are a gather from rows of 5000
    batch       (32, 3000, 200, 32)     lengths ragged down to 60 % of the maximum
    wide        (1, 2100, 1023, 32)     the most targets the kernel takes: sixteen waves (not in the default list)
    mid         (1, 1000, 100, 32)      101 pairs of states: two waves (likewise)

A block is at least ``--min-seconds`` of calls between two device events after a warm-up; ``--repeats`` blocks give median / min /
max in ms per call, and microseconds per dependent step of the recursion (``max_b Tb - 1`` steps; the backtrack and the outputs
are inside that figure).  The launches of one functional call are counted.  The composites are timed over ``--composite-calls`` single calls after one warm-up call (0: not at all) and compared
with the kernel's result, which must be identical.  Prints ONE JSON line.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

CASES = {'long': (1, 3000, 200, 32), 'vocab': (1, 1500, 60, 5000), 'batch': (32, 3000, 200, 32), 'wide': (1, 2100, 1023, 32),
         'mid': (1, 1000, 100, 32)}


def block(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def same(a, b):
    return bool(torch.equal(a[0].cpu(), b[0].cpu())) and bool(torch.equal(a[1].cpu().view(torch.int32), b[1].cpu().view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--json', default='')
    ap.add_argument('--cases', default='long,vocab,batch')
    ap.add_argument('--composite-calls', type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_forced_align.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(31)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}
    H, Cp = tac._hip, tac._composite
    for case in a.cases.split(','):
        B, T, L, C = CASES[case]
        tac.set_strict(True)
        lp = torch.log_softmax(torch.randn((B, T, C), device='cuda', generator=gen), dim=-1)
        targets = torch.randint(1, C, (B, L), device='cuda', generator=gen)
        share = [1.0 - 0.4 * i / max(B - 1, 1) for i in range(B)]
        il_host, tl_host = [max(1, round(T * s)) for s in share], [int(L * s) for s in share]
        il = torch.tensor(il_host, dtype=torch.int32, device='cuda')
        tl = torch.tensor(tl_host, dtype=torch.int32, device='cuda')
        steps = max(il_host) - 1
        res = {'shape': [B, T, L, C], 'steps': steps}

        before = dict(H.launches)
        want = tac.forced_align(lp, targets, il, tl)
        res['launches_per_call'] = {k: v - before.get(k, 0) for k, v in H.launches.items() if v != before.get(k, 0)}
        assert res['launches_per_call'] == {'tac_forced_align_f32': 1}, res['launches_per_call']
        assert same(want, tac.forced_align(lp, targets, il, tl)), 'two calls differ'
        assert int(want[0].min()) >= 0, 'an entry of the benchmark is infeasible'

        routes = {'kernel': lambda: tac.forced_align(lp, targets, il, tl)}
        iters = {}
        for name, fn in routes.items():                            # warm-up, and the block length that fills min-seconds
            block(fn, 1)
            per_call = block(fn, 2)
            iters[name] = max(2, int(a.min_seconds * 1e3 / per_call) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, iters[name]))
        for name in routes:
            t = times[name]
            res[name] = {'ms_median': round(statistics.median(t), 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                         'us_per_step': round(statistics.median(t) * 1e3 / steps, 4), 'iters_per_block': iters[name]}
        kernel_ms = res['kernel']['ms_median']
        if a.composite_calls > 0:
            tac.set_strict(False)

            def composite_device():
                return Cp.forced_align(lp, targets, il, tl, 0)

            def composite_host():                                   # log-probabilities to the host, the alignment back
                out = Cp.forced_align(lp.cpu(), targets.cpu(), il.cpu(), tl.cpu(), 0)
                return out[0].cuda(), out[1].cuda()

            res['composite'] = {}
            with torch.no_grad():
                for name, fn in (('device', composite_device), ('host_with_transfer', composite_host)):
                    identical = same(fn(), want)                    # warm-up: the allocator's blocks, every operator's first call
                    single = []
                    for _ in range(a.composite_calls):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        single.append((time.perf_counter() - t0) * 1e3)
                    res['composite'][name] = {'ms_single_calls': [round(t, 2) for t in single], 'identical_to_kernel': identical,
                                              'us_per_step': round(min(single) * 1e3 / steps, 2),
                                              'composite_over_kernel': round(min(single) / kernel_ms, 1)}
                    torch.cuda.empty_cache()
            tac.set_strict(True)
        else:
            res['composite'] = 'not measured'
        line[case] = res
        del lp, want
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
