#!/usr/bin/env python
"""Time ``ctc_loss`` on the gfx950 kernels (csrc/ctc_loss.hip) — its two launches, the forward call and forward + backward — against
``torch.nn.functional.ctc_loss`` on the same device and a ``clone`` of the log-probabilities, in one process.

    python tools/bench_ctc_loss.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases words,subwords,chars]

Shapes (N, T, C) with S targets; the model's ``(N, T, C)`` output is passed as ``.transpose(0, 1)``, as a recipe would:

    words       (32, 1500, 5000)  S = 150   lengths ragged down to 60 %
    subwords    (32, 750, 500)    S = 100
    chars       (8, 3000, 32)     S = 400

A block is at least ``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating
blocks give median / min / max in ms per call.  Derived figures: the time per dependent step of the lattice launch (``max_b Tb``
steps), and the gradient launch's bytes (the read of the valid frames plus the write of the whole gradient) over its time as a
share of 8 TB/s.  Prints ONE JSON line.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

CASES = {'words': (32, 1500, 5000, 150, True), 'subwords': (32, 750, 500, 100, False), 'chars': (8, 3000, 32, 400, False)}
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
    ap.add_argument('--cases', default='words,subwords,chars')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ctc_loss.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(38)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}
    H, F = tac._hip, torch.nn.functional
    tac.set_strict(True)
    for case in a.cases.split(','):
        N, T, C, S, ragged = CASES[case]
        lp = torch.log_softmax(torch.randn((N, T, C), device='cuda', generator=gen), -1).transpose(0, 1)
        targets = torch.randint(1, C, (N, S), device='cuda', generator=gen)
        share = [1.0 - (0.4 * i / max(N - 1, 1) if ragged else 0.0) for i in range(N)]
        il_host, tl_host = [max(1, round(T * s)) for s in share], [int(S * s) for s in share]
        il, tl = torch.tensor(il_host, device='cuda'), torch.tensor(tl_host, device='cuda')
        valid_bytes, all_bytes = 4 * C * sum(il_host), 4 * lp.numel()
        res = {'shape': [N, T, C], 'S': S, 'log_probs_MB': round(all_bytes / 1e6, 1), 'valid_MB': round(valid_bytes / 1e6, 1),
               'steps': max(il_host)}
        x = lp.detach().requires_grad_(True)
        costs, alphas, betas = H.ctc_loss_forward(lp, targets, il, tl, 0, S, True)
        ones = torch.ones_like(costs)

        def forward_backward():
            return torch.autograd.grad(tac.ctc_loss(x, targets, il, tl, reduction='sum'), x)[0]

        def torch_forward_backward():
            return torch.autograd.grad(F.ctc_loss(x, targets, il, tl, reduction='sum'), x)[0]

        routes = {'lattice_launch': lambda: H.ctc_loss_forward(lp, targets, il, tl, 0, S, True),
                  'alpha_only_launch': lambda: H.ctc_loss_forward(lp, targets, il, tl, 0, S, False),
                  'grad_launch': lambda: H.ctc_loss_grad(lp, targets, il, tl, alphas, betas, costs, ones, 0, S, False),
                  'forward': lambda: tac.ctc_loss(lp, targets, il, tl, reduction='none'),
                  'forward_backward': forward_backward,
                  'torch_forward': lambda: F.ctc_loss(lp, targets, il, tl, reduction='none'),
                  'torch_forward_backward': torch_forward_backward, 'clone': lambda: lp.clone()}
        want, theirs = routes['forward'](), routes['torch_forward']()
        grad, their_grad = forward_backward(), torch_forward_backward()
        assert torch.equal(want, routes['forward']()) and torch.equal(grad, forward_backward()), 'two calls differ'
        res['max_cost_difference_over_cost'] = float(((want - theirs).abs() / theirs.abs()).max())
        res['max_grad_difference'] = float((grad - their_grad).abs().max())
        del grad, their_grad
        iters = {}
        for name, fn in routes.items():                            # warm-up, and the block length that fills min-seconds
            block(fn, 1)
            iters[name] = max(2, int(a.min_seconds * 1e3 / block(fn, 2)) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, iters[name]))
        for name in routes:
            t = times[name]
            res[name] = {'ms_median': round(statistics.median(t), 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                         'iters_per_block': iters[name]}
        ms = {name: res[name]['ms_median'] for name in routes}
        res['lattice_launch']['us_per_step'] = round(ms['lattice_launch'] * 1e3 / res['steps'], 4)
        res['grad_launch']['share_of_8TBps_on_valid_read_plus_write'] = round((valid_bytes + all_bytes) / (ms['grad_launch'] * 1e-3) / PEAK, 3)
        res['torch_forward_over_forward'] = round(ms['torch_forward'] / ms['forward'], 2)
        res['torch_forward_backward_over_forward_backward'] = round(ms['torch_forward_backward'] / ms['forward_backward'], 2)
        res['forward_backward_over_clone'] = round(ms['forward_backward'] / ms['clone'], 2)
        line[case] = res
        del lp, x, alphas, betas
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
