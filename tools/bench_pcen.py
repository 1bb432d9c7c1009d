"""Times ``pcen`` on the device: the kernels of csrc/pcen.hip against ``_composite.pcen`` on the same device and against a ``clone`` of
the input (the traffic floor: one read, one write), forward and forward + backward with all five gradients.  Device events around
windows of ``--seconds`` of calls, ``--repeats`` windows a route with the routes alternating (median, min, max): call times, host
enqueue included, not kernel times.  Prints one JSON line.  Needs a HIP device: there is no fall-back."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac                                    # noqa: E402
from torchaudio_contrib_amd import _composite                           # noqa: E402

SHAPES = {'frame-major (256, 128, 313)': (256, 128, 313), 'frame-major (64, 80, 3000)': (64, 80, 3000)}


def window(fn, calls):
    """ms per call of ``calls`` calls between two device events: a CALL time, host enqueue included"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=0.3, help='length of one timed window of a route')
    ap.add_argument('--repeats', type=int, default=5, help='windows per route, the routes alternating')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pcen needs the GPU'
    tac.set_strict(True)
    result = {}
    for name, (rows, F, T) in SHAPES.items():
        g = torch.Generator(device='cuda').manual_seed(1)
        x = (torch.rand((rows, T, F), device='cuda', generator=g) * 10).transpose(-1, -2)
        params = [torch.full((F,), v, device='cuda') for v in (0.98, 2.0, 0.5, 0.06)]
        table = torch.stack(params)
        grad = torch.rand_like(x)

        def train(fn):
            leaves = [x.detach().requires_grad_(True)] + [p.detach().requires_grad_(True) for p in params]
            torch.autograd.grad(fn(*leaves), leaves, grad)

        def plain(fn):
            with torch.no_grad():
                return fn()

        kernel = lambda e, ga, bi, po, b: tac.pcen(e, gain=ga, bias=bi, power=po, b=b)
        composite = lambda e, ga, bi, po, b: _composite.pcen(e, torch.stack((ga, bi, po, b)), 1e-6, 0)
        routes = {'clone': lambda: x.clone(), 'forward': lambda: plain(lambda: tac.pcen(x, b=0.06)),
                  'forward composite': lambda: plain(lambda: _composite.pcen(x, table, 1e-6, 0)),
                  'forward + backward': lambda: train(kernel), 'forward + backward composite': lambda: train(composite)}
        err = float((routes['forward']() - routes['forward composite']()).abs().max())
        for fn in routes.values():
            window(fn, 2)                                                   # (warm-up: code objects, allocator, tables)
        calls = {k: max(2, int(args.seconds * 1e3 / window(fn, 3))) for k, fn in routes.items()}
        seen = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, fn in routes.items():
                seen[k].append(window(fn, calls[k]))
        ms = {k: sorted(v)[len(v) // 2] for k, v in seen.items()}
        gb = rows * F * T * 4 / 1e9
        result[name] = dict(ms_median={k: round(v, 4) for k, v in ms.items()}, ms_min={k: round(min(v), 4) for k, v in seen.items()},
                            ms_max={k: round(max(v), 4) for k, v in seen.items()}, calls_per_window=calls, max_abs_diff_to_composite=err,
                            forward_GBps=round(2 * gb / ms['forward'] * 1e3, 1), clone_GBps=round(2 * gb / ms['clone'] * 1e3, 1),
                            training_GBps=round(7 * gb / ms['forward + backward'] * 1e3, 1))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
