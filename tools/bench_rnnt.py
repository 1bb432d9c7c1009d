#!/usr/bin/env python
"""Time ``rnnt_loss`` on the gfx950 kernels (csrc/rnnt.hip) — each of its three launches, the forward call and forward + backward —
against the torch-operator composite, ``torch.log_softmax`` (the floor any unfused implementation pays before its recursion starts)
and a ``clone`` of the logits, on the same device in one process.

    python tools/bench_rnnt.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases recipe,chars] [--composite-calls 2]

Shapes (batch, time, target + 1, class), lengths ragged down to 60 % of the maximum:

    recipe      (32, 400, 101, 1024)    the Emformer / Conformer transducer recipes: 5.3 GB of logits
    chars       (8, 150, 31, 29)        characters: the dynamic program dominates

A block is at least ``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating
blocks give median / min / max in ms per call.  The composite is timed over ``--composite-calls`` single calls after one warm-up
call (0: not at all).  Derived figures: the share of 8 TB/s the rows launch reaches on the bytes of the VALID part of the logits, the
share the gradient launch reaches on that read plus the write of the whole gradient, and the time per dependent step of the lattice
launch (``max_b Tb + Ub`` steps).  Prints ONE JSON line.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

CASES = {'recipe': (32, 400, 101, 1024), 'chars': (8, 150, 31, 29)}
PEAK = 8e12


def block(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--json', default='')
    ap.add_argument('--cases', default='recipe,chars')
    ap.add_argument('--composite-calls', type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_rnnt.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(31)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}
    H, Cp, N = tac._hip, tac._composite, tac._native
    for case in a.cases.split(','):
        B, T, U1, V = CASES[case]
        U = U1 - 1
        tac.set_strict(True)
        logits = torch.randn((B, T, U1, V), device='cuda', generator=gen)
        targets = torch.randint(0, V - 1, (B, U), device='cuda', generator=gen).to(torch.int32)
        share = [1.0 - 0.4 * i / max(B - 1, 1) for i in range(B)]
        tl_host, ul_host = [max(1, round(T * s)) for s in share], [int(U * s) for s in share]
        tl = torch.tensor(tl_host, dtype=torch.int32, device='cuda')
        ul = torch.tensor(ul_host, dtype=torch.int32, device='cuda')
        blank = V - 1
        valid_bytes = 4 * V * sum(t * (u + 1) for t, u in zip(tl_host, ul_host))
        all_bytes = 4 * logits.numel()
        steps = max(t + u for t, u in zip(tl_host, ul_host))
        res = {'shape': [B, T, U1, V], 'logits_MB': round(all_bytes / 1e6, 1), 'valid_MB': round(valid_bytes / 1e6, 1), 'steps': steps}

        denom, lpb, lpl, alphas, betas = (torch.empty((B, T, U1), device='cuda') for _ in range(5))
        costs, ones = torch.empty(B, device='cuda'), torch.ones(B, device='cuda')
        grad = torch.empty_like(logits)
        geo = (N.ptr(logits), B, T, U1, V, logits.stride(0), logits.stride(1), logits.stride(2))
        dev = logits.device

        def rows():
            H._launch('tac_rnnt_rows_f32', dev, (), *geo, N.ptr(targets), N.ptr(tl), N.ptr(ul), blank, 1, N.ptr(denom), N.ptr(lpb),
                      N.ptr(lpl), N.ptr(alphas), N.ptr(betas))

        def lattice():
            H._launch('tac_rnnt_lattice_f32', dev, (), B, T, U1, V, N.ptr(targets), N.ptr(tl), N.ptr(ul), N.ptr(lpb), N.ptr(lpl),
                      N.ptr(alphas), N.ptr(betas), N.ptr(costs))

        def gradient():
            H._launch('tac_rnnt_grad_f32', dev, (), *geo, N.ptr(targets), N.ptr(tl), N.ptr(ul), N.ptr(alphas), N.ptr(betas),
                      N.ptr(denom), N.ptr(costs), N.ptr(ones), blank, -1.0, 1, N.ptr(grad))

        x = logits.detach().requires_grad_(True)
        go = torch.ones_like(logits)

        def forward():
            return tac.rnnt_loss(logits, targets, tl, ul, reduction='none')

        def forward_backward():
            return torch.autograd.grad(tac.rnnt_loss(x, targets, tl, ul, reduction='sum'), x)[0]

        def log_softmax_backward():
            return torch.autograd.grad(torch.log_softmax(x, -1), x, go)[0]

        routes = {'rows_launch': rows, 'lattice_launch': lattice, 'grad_launch': gradient, 'forward': forward,
                  'forward_backward': forward_backward, 'log_softmax': lambda: torch.log_softmax(logits, -1),
                  'log_softmax_backward': log_softmax_backward, 'clone': lambda: logits.clone()}
        want = forward()
        got_grad = forward_backward()
        assert torch.equal(want, forward()) and torch.equal(got_grad, forward_backward()), 'two calls differ'
        assert bool(torch.isfinite(want).all())
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
                         'iters_per_block': iters[name]}
        ms = {name: res[name]['ms_median'] for name in routes}
        res['rows_launch']['share_of_8TBps_on_valid_bytes'] = round(valid_bytes / (ms['rows_launch'] * 1e-3) / PEAK, 3)
        res['grad_launch']['share_of_8TBps_on_valid_read_plus_write'] = round((valid_bytes + all_bytes) / (ms['grad_launch'] * 1e-3) / PEAK, 3)
        res['lattice_launch']['us_per_step'] = round(ms['lattice_launch'] * 1e3 / steps, 4)
        res['forward_over_clone'] = round(ms['forward'] / ms['clone'], 2)
        res['forward_backward_over_clone'] = round(ms['forward_backward'] / ms['clone'], 2)
        res['forward_over_log_softmax'] = round(ms['forward'] / ms['log_softmax'], 2)
        res['forward_backward_over_log_softmax_backward'] = round(ms['forward_backward'] / ms['log_softmax_backward'], 2)
        del go, grad
        torch.cuda.empty_cache()
        if a.composite_calls > 0:
            def composite_forward():
                return Cp.rnnt_loss(logits, targets, tl, ul, blank, -1.0, True)

            def composite_forward_backward():
                c, al, be, de = Cp.rnnt_loss(logits, targets, tl, ul, blank, -1.0, True)
                return Cp.rnnt_loss_grad(logits, targets, tl, ul, al, be, de, c, ones, blank, -1.0, True)

            res['composite'] = {}
            with torch.no_grad():
                for name, fn, mine, kernel in (('forward', composite_forward, want, 'forward'),
                                               ('forward_backward', composite_forward_backward, got_grad, 'forward_backward')):
                    ref = fn()                                      # warm-up: the allocator's blocks and every operator's first call
                    ref = ref[0] if isinstance(ref, tuple) else ref
                    diff = float((ref - mine).abs().max() / ref.abs().max())
                    del ref
                    single = []
                    for _ in range(a.composite_calls):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        single.append((time.perf_counter() - t0) * 1e3)
                    res['composite'][name] = {'ms_single_calls': [round(t, 2) for t in single], 'max_abs_difference_over_max': diff,
                                              'composite_over_kernel': round(min(single) / ms[kernel], 1)}
                    torch.cuda.empty_cache()
        else:
            res['composite'] = 'not measured'
        line[case] = res
        del logits, x, want, got_grad
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
