#!/usr/bin/env python
"""Time the wide polyphase kernel (``tac_polyphase_wide_f32``, csrc/resample.hip) and ``pitch_shift`` / ``PitchShift`` on it — in one
process, on the same device tensors, alternating the routes.

    python tools/bench_pitch_shift.py [--repeats 7] [--min-seconds 0.3] [--json profiles/pitch_shift/bench.json]

Launches (``launches`` of the result), each beside a ``clone`` of its output (the floor of writing it) and beside
``tac_polyphase_f32`` at the small pair of the same K (5 : 4 for K = 16, 4 : 5 for K = 13: what taking the taps from L2 instead of
the LDS costs):

    10079 : 8000   forward and adjoint, (256, 160000)         16 kHz, n_steps = 4
    12699 : 16000  forward and adjoint, (256, 160000)         16 kHz, n_steps = -4
    42763 : 48000  forward, (16, 2880000)                     48 kHz, n_steps = -2: the largest bank, 48000 x 13 floats
    composite      ``_composite.resample_compact`` on the device (K gathers and multiply-adds) for 10079 : 8000; the ``conv1d``
                   composite cannot be timed: its bank is 323 MB there and 8.2 GB at 42763 : 48000

Chains (``chains``): ``pitch_shift`` and ``PitchShift`` forward + backward at (32, 160000), 16 kHz, n_steps = 4, against the same
chain in torch operators on the device (``_composite``: torch.stft, the vocoder in torch ops, torch.istft, the compact composite).

A block is at least ``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating
blocks give median / min / max.  ``faster_beyond_spread``: the slowest block of the kernels beats the fastest of the other route.
Prints ONE JSON line (and writes it to ``--json``).  Needs the GPU: there is no fallback."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402
from torchaudio_contrib_amd import _augment, _composite, _resample  # noqa: E402

H = tac._hip


def block(fn, inputs, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[i % len(inputs)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def measure(routes, repeats, min_seconds):
    """{name: stats} of ``routes`` = {name: (fn, inputs)}: warmed, then ``repeats`` alternating blocks"""
    iters = {}
    for name, (fn, inputs) in routes.items():
        block(fn, inputs, 3)
        per_call = block(fn, inputs, 4)
        iters[name] = max(4, int(min_seconds * 1e3 / per_call) + 1)
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, (fn, inputs) in routes.items():
            times[name].append(block(fn, inputs, iters[name]))
    out = {}
    for name, t in times.items():
        med = statistics.median(t)
        out[name] = {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                     'spread': round((max(t) - min(t)) / med, 4), 'iters_per_block': iters[name]}
    return out


def launch_case(orig_freq, new_freq, rows, l_in, small, adjoint, with_composite, a):
    key = _resample.constants(orig_freq, new_freq)
    skey = _resample.constants(*small)
    n_out = _resample.out_length(l_in, key[0], key[1])
    gen = torch.Generator(device='cuda').manual_seed(orig_freq + int(adjoint))
    b = (_resample.adjoint_bank if adjoint else _resample.bank)(*key)
    sb = (_resample.adjoint_bank if adjoint else _resample.bank)(*skey)
    assert sb.K == b.K, (sb.K, b.K)
    if adjoint:         # grad_out (rows, n_out) -> (rows, l_in)
        inputs = [torch.rand((rows, n_out), device='cuda', generator=gen) * 2 - 1 for _ in range(2)]
        s_out = _resample.out_length(l_in, skey[0], skey[1])
        s_inputs = [torch.rand((rows, s_out), device='cuda', generator=gen) * 2 - 1 for _ in range(2)]
        wide = lambda g: H.resample_fit(g, key, n_out, adjoint=True, length=l_in, wide=True)      # noqa: E731
        lds = lambda g: H.polyphase(g, skey, l_in, adjoint=True)                                   # noqa: E731
        moved = rows * (n_out + l_in) * 4
    else:
        inputs = [torch.rand((rows, l_in), device='cuda', generator=gen) * 2 - 1 for _ in range(2)]
        s_in = n_out * skey[0] // skey[1]                                                          # the same number of outputs
        s_inputs = [torch.rand((rows, s_in), device='cuda', generator=gen) * 2 - 1 for _ in range(2)]
        wide = lambda w: H.resample_fit(w, key, n_out, wide=True)                                  # noqa: E731
        lds = lambda w: H.polyphase(w, skey, _resample.out_length(s_in, skey[0], skey[1]))         # noqa: E731
        moved = rows * (n_out + l_in) * 4
    outs = [wide(inputs[0]), wide(inputs[1])]
    routes = {'wide': (wide, inputs), 'clone': (torch.clone, outs), 'lds_small_pair': (lds, s_inputs)}
    if with_composite:
        routes['composite_compact'] = (lambda w: _composite.resample_compact(w, *key, n_out), inputs)
    stats = measure(routes, a.repeats, a.min_seconds)
    line = {'pair': [key[0], key[1]], 'adjoint': adjoint, 'rows': rows, 'samples_in': inputs[0].shape[-1], 'samples_out': outs[0].shape[-1],
            'bank': [b.phases, b.K], 'plan': list(H.resample_wide_plan(b)), 'small_pair': list(small), 'traffic_MB': round(moved / 1e6, 1)}
    line.update(stats)
    line['wide']['TB_per_s'] = round(moved / (stats['wide']['ms_median'] * 1e-3) / 1e12, 3)
    line['wide_over_clone'] = round(stats['wide']['ms_median'] / stats['clone']['ms_median'], 3)
    line['wide_over_lds'] = round(stats['wide']['ms_median'] / stats['lds_small_pair']['ms_median'], 3)
    if with_composite:
        line['composite_over_wide'] = round(stats['composite_compact']['ms_median'] / stats['wide']['ms_median'], 2)
    return line


def torch_chain(window, sample_rate, n_steps, n_fft=512):
    """``pitch_shift`` in torch operators on the device: what the package would run without its kernels"""
    hop = n_fft // 4
    rate, source = _augment.pitch_rates(sample_rate, n_steps)
    key = _resample.constants(source, sample_rate)
    advance = torch.linspace(0, math.pi * hop, n_fft // 2 + 1, device=window.device)[:, None]

    def run(x):
        length = x.shape[-1]
        spec = _composite.stft(x, window, n_fft, hop, n_fft, True, 'reflect', False, True)
        y = _composite.istft(_composite.phase_vocoder(spec, rate, advance), window, n_fft, hop, n_fft, True, False, True,
                             int(round(length / rate)))
        return _composite.resample_compact(y, *key, length)
    return run


def chain_case(rows, length, sample_rate, n_steps, a):
    gen = torch.Generator(device='cuda').manual_seed(7)
    waves = [(torch.rand((rows, length), device='cuda', generator=gen) * 2 - 1).requires_grad_(True) for _ in range(2)]
    layer = tac.PitchShift(sample_rate, n_steps).cuda()
    stock = torch_chain(layer.window, sample_rate, n_steps)

    def train(fn):
        def step(x):
            x.grad = None
            fn(x).square().mean().backward()
        return step

    def infer(fn):
        def step(x):
            with torch.no_grad():
                fn(x)
        return step

    functional = lambda x: tac.pitch_shift(x, sample_rate, n_steps)        # noqa: E731
    with torch.no_grad():
        diff = float((functional(waves[0]) - stock(waves[0])).abs().max())
    routes = {'pitch_shift_fwd_bwd': (train(functional), waves), 'PitchShift_fwd_bwd': (train(layer), waves),
              'torch_ops_fwd_bwd': (train(stock), waves), 'pitch_shift_fwd': (infer(functional), waves),
              'torch_ops_fwd': (infer(stock), waves)}
    stats = measure(routes, a.repeats, a.min_seconds)
    line = {'rows': rows, 'samples': length, 'sample_rate': sample_rate, 'n_steps': n_steps, 'max_abs_diff_kernels_vs_torch_ops': diff}
    line.update(stats)
    for ours, theirs in (('pitch_shift_fwd_bwd', 'torch_ops_fwd_bwd'), ('PitchShift_fwd_bwd', 'torch_ops_fwd_bwd'),
                         ('pitch_shift_fwd', 'torch_ops_fwd')):
        line[ours]['torch_ops_over_kernels'] = round(stats[theirs]['ms_median'] / stats[ours]['ms_median'], 2)
        line[ours]['faster_beyond_spread'] = bool(stats[ours]['ms_max'] < stats[theirs]['ms_min'])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--json', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_pitch_shift.py measures on the GPU only'
    tac.set_strict(True)
    result = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'launches': [], 'chains': []}
    for orig, new, rows, l_in, small, adjoint, comp in (
            (10079, 8000, 256, 160000, (5, 4), False, True), (10079, 8000, 256, 160000, (5, 4), True, False),
            (12699, 16000, 256, 160000, (4, 5), False, False), (12699, 16000, 256, 160000, (4, 5), True, False),
            (42763, 48000, 16, 2880000, (4, 5), False, False)):
        result['launches'].append(launch_case(orig, new, rows, l_in, small, adjoint, comp, a))
        torch.cuda.empty_cache()
    tac.set_strict(True, backward=True)
    result['chains'].append(chain_case(32, 160000, 16000, 4, a))
    text = json.dumps(result)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
