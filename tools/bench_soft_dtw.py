"""Times ``soft_dtw`` on the device: the kernels of csrc/soft_dtw.hip against the package's composite route (``_composite``: an
anti-diagonal of torch operators at a time) on the same device, forward and forward + backward.  Device events around windows of
``--seconds`` of calls, ``--repeats`` windows a route with the routes alternating (median, min, max): call times, host enqueue
included, not kernel times.  The time of a lattice step is the forward call time over its ``N + M - 1`` dependent steps (the cost
launch included: an upper estimate).  Prints one JSON line.  Needs a HIP device: there is no fall-back."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac                                    # noqa: E402
from torchaudio_contrib_amd import _composite                           # noqa: E402

SHAPES = [(32, 512, 512, 80), (8, 2048, 2048, 80), (64, 128, 400, 80)]
GAMMA = 1.0


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
    ap.add_argument('--composite-calls', type=int, default=1, help='calls in a window of the composite route (thousands of launches each)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_soft_dtw needs the GPU'
    tac.set_strict(True)
    result = {}
    for B, N, M, D in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(1)
        x, y = torch.randn((B, N, D), device='cuda', generator=g), torch.randn((B, M, D), device='cuda', generator=g)
        xl, yl = torch.full((B,), N, dtype=torch.int32, device='cuda'), torch.full((B,), M, dtype=torch.int32, device='cuda')
        w = torch.rand((B,), device='cuda', generator=g)

        def forward():
            with torch.no_grad():
                return tac.soft_dtw(x, y, GAMMA)

        def train():
            xg, yg = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
            return torch.autograd.grad(tac.soft_dtw(xg, yg, GAMMA), (xg, yg), w)

        def forward_composite():
            return _composite.soft_dtw_lattice(x, y, xl, yl, GAMMA, both=False)[0]

        def train_composite():
            value, delta, R, Q = _composite.soft_dtw_lattice(x, y, xl, yl, GAMMA)
            return _composite.soft_dtw_grad(x, y, xl, yl, delta, R, Q, value, w, GAMMA)

        routes = {'forward': forward, 'forward + backward': train, 'forward composite': forward_composite,
                  'forward + backward composite': train_composite}
        rel = float(((forward() - forward_composite()).abs() / forward_composite().abs()).max())
        grad_diff = float((train()[0] - train_composite()[0]).abs().max())
        calls = {}
        for k, fn in routes.items():
            window(fn, 1)                                                   # (warm-up: code objects, allocator)
            calls[k] = args.composite_calls if 'composite' in k else max(2, int(args.seconds * 1e3 / window(fn, 3)))
        seen = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, fn in routes.items():
                seen[k].append(window(fn, calls[k]))
        ms = {k: sorted(v)[len(v) // 2] for k, v in seen.items()}
        result['(%d, %d, %d, %d)' % (B, N, M, D)] = dict(
            ms_median={k: round(v, 4) for k, v in ms.items()}, ms_min={k: round(min(v), 4) for k, v in seen.items()},
            ms_max={k: round(max(v), 4) for k, v in seen.items()}, calls_per_window=calls, max_rel_value_diff_to_composite=rel,
            max_abs_grad_x_diff_to_composite=grad_diff, us_per_lattice_step=round(1e3 * ms['forward'] / (N + M - 1), 4),
            kept_MB=round(3 * B * (N + M - 1) * N * 4 / 1e6, 1))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
