#!/usr/bin/env python
"""Time ``sliding_window_cmn`` and ``compute_deltas`` on the gfx950 kernels (csrc/cmn_deltas.hip) against the composite torch route
and against ``x.clone()`` of the same tensor, in one process, alternating the routes.

    python tools/bench_cmn_deltas.py [--repeats 7] [--min-seconds 0.3] [--json OUT] [--profile CASE:ROUTE]

Shapes: 256 rows x 1000 frames x 80 features (what ``kaldi_fbank`` returns for 256 utterances of 10 s).  Cases:

    cmn             sliding_window_cmn at the defaults (cmn_window 600, min_cmn_window 100)
    cmn_vars        the same with norm_vars=True
    deltas_T        compute_deltas (win_length 5, 'replicate') on the transposed views (256, 80, 1000) of the (1000, 80) matrices:
                    lanes load along the features, the tile is turned in the LDS
    deltas          compute_deltas on contiguous (256, 80, 1000)

Routes per case: ``kernel`` (one launch), ``composite`` (``_composite``: float64 cumsum differences / an index gather, in torch
operators) and ``clone`` (``x.clone()``: one read and one write of the same bytes by code that is not this project's — the
yardstick; for ``deltas_T`` the clone writes the dense (256, 80, 1000) layout the kernel writes, so it transposes too).

Eight distinct inputs of 81.9 MB are visited in turn (655 MB, well beyond the 256 MiB last-level cache, so that no route is
served from it); a block is at least ``--min-seconds`` of calls between two device events, after a warm-up of every route;
``--repeats`` alternating blocks give median / min / max.  Prints ONE JSON line.  ``--profile
cmn:kernel`` (any case:route) runs only that route a few times.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

ROWS, FRAMES, FEATS = 256, 1000, 80
INPUTS = 8


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
    ap.add_argument('--profile', default='')
    ap.add_argument('--rows', type=int, default=ROWS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_cmn_deltas.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(80)
    feats = [torch.randn((a.rows, FRAMES, FEATS), device='cuda', generator=gen) + 5.0 for _ in range(INPUTS)]
    turned = [x.transpose(-1, -2) for x in feats]                                   # (rows, 80, 1000) views, stride_f == 1
    dense = [x.contiguous() for x in turned]
    C = tac._composite
    tac.set_strict(True)
    cases = {
        'cmn': (feats, {'kernel': lambda x: tac.sliding_window_cmn(x),
                        'composite': lambda x: C.sliding_window_cmn(x, 600, 100, False, False),
                        'clone': lambda x: x.clone()}),
        'cmn_vars': (feats, {'kernel': lambda x: tac.sliding_window_cmn(x, norm_vars=True),
                             'composite': lambda x: C.sliding_window_cmn(x, 600, 100, False, True),
                             'clone': lambda x: x.clone()}),
        'deltas_T': (turned, {'kernel': lambda x: tac.compute_deltas(x),
                              'composite': lambda x: C.compute_deltas(x, 5, 'replicate'),
                              'clone': lambda x: x.clone(memory_format=torch.contiguous_format)}),
        'deltas': (dense, {'kernel': lambda x: tac.compute_deltas(x),
                           'composite': lambda x: C.compute_deltas(x, 5, 'replicate'),
                           'clone': lambda x: x.clone()}),
    }
    if a.profile:
        case, route = a.profile.split(':')
        inputs, routes = cases[case]
        for _ in range(5):
            for x in inputs:
                routes[route](x)
        torch.cuda.synchronize()
        return
    moved = a.rows * FRAMES * FEATS * 4 * 2
    line = {'inputs': INPUTS, 'rows': a.rows, 'frames': FRAMES, 'feats': FEATS, 'repeats': a.repeats, 'min_seconds': a.min_seconds,
            'moved_MB': round(moved / 1e6, 1)}
    for case, (inputs, routes) in cases.items():
        before = dict(tac._hip.launches)
        got = routes['kernel'](inputs[0])
        launches = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        worst = float((got - routes['composite'](inputs[0])).abs().max())
        iters = {}
        for name, fn in routes.items():                            # warm-up, and the block length that fills min-seconds
            block(fn, inputs, INPUTS)
            per_call = block(fn, inputs, INPUTS)
            iters[name] = max(8, int(a.min_seconds * 1e3 / per_call) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, inputs, iters[name]))
        res = {'launches': launches, 'max_abs_diff_kernel_vs_composite': worst}
        for name in routes:
            t = times[name]
            med = statistics.median(t)
            res[name] = {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                         'iters_per_block': iters[name]}
        med = res['kernel']['ms_median']
        res['kernel']['TB_per_s'] = round(moved / (med * 1e-3) / 1e12, 3)
        res['kernel_over_clone'] = round(med / res['clone']['ms_median'], 3)
        res['composite_over_kernel'] = round(res['composite']['ms_median'] / med, 3)
        line[case] = res
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
