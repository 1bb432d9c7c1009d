"""Times ``cqt`` on the gfx950 kernel (csrc/cqt.hip) against the ``_composite`` route (the padded ``conv1d``) on the same device,
in one process.

    python tools/bench_cqt.py [--out profiles/cqt/bench.json] [--repeats 5]

Every timing is device events around ``iters`` calls after a warm-up of the same shape, the median of ``repeats`` windows, the two
routes alternating.  The arithmetic a shape needs is counted from the wavelets' own lengths: 4 FLOP per tap, bin and frame (a
real sample times a complex tap, accumulated), and what the kernel executes is counted from its bank (16 columns per block, zero
fill included).  Needs the MI355X: without a device it fails."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac                                    # noqa: E402
from torchaudio_contrib_amd import _cqt, _ops                            # noqa: E402

SR = 22050.0
SHAPES = [(64, 30.0), (1, 10.0)]
F32_MATRIX_PEAK = 157.3e12          # MI355X, float32 on the matrix pipe, FLOP/s


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def timed(fns, repeats):
    """{name: median ms per call}, the candidates alternating"""
    plans = {}
    for name, fn in fns.items():
        once = window(fn, 1)
        window(fn, 2)
        plans[name] = (fn, max(1, min(50, int(200.0 / max(once, 1e-3)))))
    samples = {name: [] for name in plans}
    for _ in range(repeats):
        for name, (fn, iters) in plans.items():
            samples[name].append(window(fn, iters))
    return {name: sorted(s)[len(s) // 2] for name, s in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_cqt needs the MI355X'
    plan = _cqt.plan(SR, 32.70, 84, 12, 1.0, 0.0, 1, True)
    results = []
    for rows, seconds in SHAPES:
        x = torch.randn(rows, int(seconds * SR), device='cuda')
        frames = 1 + x.shape[-1] // 512
        tac.set_strict(True)
        before = dict(tac._hip.launches)
        got = tac.cqt(x[:2, :44100], SR)
        tac.set_strict(False)
        want = _ops._cqt_composite(x[:2, :44100].double(), plan, 512, True, 'reflect', 0)
        entry = {'rows': rows, 'seconds': seconds, 'frames': frames,
                 'max_abs_diff_vs_float64_composite_2_rows_2_s': float((got - want).abs().max()),
                 'flop_needed': 4.0 * sum(plan.lengths) * frames * rows,
                 'flop_executed': 2.0 * 16 * 16 * int(plan.bank.shape[0]) * 32 * -(-frames // 32) * rows}
        entry.update({k + '_ms': v for k, v in timed({
            'kernel': lambda: tac.cqt(x, SR),
            'kernel_power2': lambda: tac.cqt(x, SR, power=2.0),
            'composite': lambda: _ops._cqt_composite(x, plan, 512, True, 'reflect', 0),
        }, args.repeats).items()})
        entry['kernel_share_of_f32_matrix_peak_needed_flop'] = entry['flop_needed'] / (entry['kernel_ms'] * 1e-3) / F32_MATRIX_PEAK
        entry['kernel_share_of_f32_matrix_peak_executed_flop'] = entry['flop_executed'] / (entry['kernel_ms'] * 1e-3) / F32_MATRIX_PEAK
        entry['composite_over_kernel'] = entry['composite_ms'] / entry['kernel_ms']
        entry['entries_called'] = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        results.append(entry)
        print(json.dumps(entry), flush=True)
        del x
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump({'device': torch.cuda.get_device_name(0), 'sample_rate': SR, 'repeats': args.repeats,
                       'f32_matrix_peak_flops': F32_MATRIX_PEAK, 'results': results}, fh)


if __name__ == '__main__':
    main()
