"""Times ``oscillator_bank`` / ``filter_waveform`` on the gfx950 kernels (csrc/ddsp.hip) against the ``_composite`` route on the
device and against a ``clone`` of the inputs, in one process, forward and forward + backward.

    python tools/bench_ddsp.py [--out profiles/ddsp/bench.json] [--repeats 5]

Every timing is device events around ``iters`` calls after a warm-up of the same shape, the median of ``repeats`` windows, the two
routes alternating.  A route that does not fit the device's memory at a shape is reported as ``null`` with the error's first line.
Needs the MI355X: without a device it fails."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac                                    # noqa: E402
from torchaudio_contrib_amd import _composite as C                      # noqa: E402

SR = 16000.0
OSC_SHAPES = [(16, 64000, 64), (256, 16000, 8), (2, 960000, 100)]
FW_SHAPES = [((256, 160000), 1000, 65, False), ((256, 160000), 250, 513, True), ((16, 2880000), 1, 513, False)]


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def timed(fns, repeats):
    """{name: median ms per call}, the candidates alternating; a candidate that raises is None with its reason"""
    out, alive = {}, {}
    for name, fn in fns.items():
        try:
            once = window(fn, 1)
            window(fn, 2)
            alive[name] = (fn, max(1, min(50, int(200.0 / max(once, 1e-3)))))
        except (RuntimeError, torch.OutOfMemoryError) as err:
            out[name] = None
            out[name + '_error'] = str(err).split('\n')[0][:160]
            torch.cuda.empty_cache()
    samples = {name: [] for name in alive}
    for _ in range(repeats):
        for name, (fn, iters) in alive.items():
            samples[name].append(window(fn, iters))
    for name, s in samples.items():
        out[name] = sorted(s)[len(s) // 2]
    return out


def with_backward(fn, leaves):
    def run():
        for leaf in leaves:
            leaf.grad = None
        fn().sum().backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ddsp needs the MI355X'
    tac.set_strict(True)
    results = []
    for rows, time, n in OSC_SHAPES:
        f = (torch.rand(rows, time, n, device='cuda') * 0.4 * SR).requires_grad_(True)
        a = torch.rand(rows, time, n, device='cuda').requires_grad_(True)
        fd, ad = f.detach(), a.detach()
        before = dict(tac._hip.launches)
        err = float((tac.oscillator_bank(fd[:, :2000], ad[:, :2000], SR) - C.oscillator_bank(fd[:, :2000].double(), ad[:, :2000].double(),
                                                                                          SR, 'sum')).abs().max())
        entry = {'op': 'oscillator_bank', 'shape': [rows, time, n], 'cells': rows * time * n,
                 'spans_per_row': int(tac._native.lib().tac_oscbank_spans(rows, time)),
                 'max_abs_diff_vs_float64_composite_first_2000_steps': err,
                 'bytes_per_cell_forward': 8 + 4.0 / n + (4 if time > tac._hip.OSCBANK_SPAN and rows < 512 else 0)}
        entry.update({k + '_ms': v for k, v in timed({
            'kernel_forward': lambda: tac.oscillator_bank(fd, ad, SR),
            'composite_forward': lambda: C.oscillator_bank(fd, ad, SR, 'sum'),
            'clone_inputs': lambda: (fd.clone(), ad.clone()),
            'kernel_forward_backward': with_backward(lambda: tac.oscillator_bank(f, a, SR), (f, a)),
            'composite_forward_backward': with_backward(lambda: C.oscillator_bank(f, a, SR, 'sum'), (f, a)),
        }, args.repeats).items()})
        entry['entries_called'] = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        results.append(entry)
        print(json.dumps(entry), flush=True)
        del f, a, fd, ad
        torch.cuda.empty_cache()
    for shape, F, K, shared in FW_SHAPES:
        x = torch.randn(shape, device='cuda', requires_grad=True)
        h = (torch.randn((F, K) if shared else (shape[0], F, K), device='cuda') / K).requires_grad_(True)
        xd, hd = x.detach(), h.detach()
        err = float((tac.filter_waveform(xd[:2, :8000], hd if shared else hd[:2]) -
                     C.filter_waveform(xd[:2, :8000].double(), (hd if shared else hd[:2]).double(), -1)).abs().max())
        entry = {'op': 'filter_waveform', 'shape': list(shape), 'filters': F, 'taps': K, 'shared': shared,
                 'max_abs_diff_vs_float64_composite_2_rows_8000_samples': err}
        entry.update({k + '_ms': v for k, v in timed({
            'kernel_forward': lambda: tac.filter_waveform(xd, hd),
            'composite_forward': lambda: C.filter_waveform(xd, hd, -1),
            'clone_inputs': lambda: xd.clone(),
            'kernel_forward_backward': with_backward(lambda: tac.filter_waveform(x, h), (x, h)),
            'composite_forward_backward': with_backward(lambda: C.filter_waveform(x, h, -1), (x, h)),
        }, args.repeats).items()})
        results.append(entry)
        print(json.dumps(entry), flush=True)
        del x, h, xd, hd
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump({'device': torch.cuda.get_device_name(0), 'sample_rate': SR, 'repeats': args.repeats, 'results': results}, fh)


if __name__ == '__main__':
    main()
