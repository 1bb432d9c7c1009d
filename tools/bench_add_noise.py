#!/usr/bin/env python
"""Time ``add_noise`` on the gfx950 kernels (csrc/add_noise.hip) against the definition in torch operators on the device
(``_composite.add_noise``: what a user had before the kernels), forward and forward + backward, in one process, alternating the routes.

    python tools/bench_add_noise.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--variant NAME=LIB ...] [--cases speech,long]

Shapes:

    speech      (256, 160000)          10 s at 16 kHz, a length per row drawn in [8 s, 10 s], a ratio per row
    long        (8, 8, 2880000)        3 min at 16 kHz, 64 rows, lengths likewise in [0.8 L, L]

Routes: ``kernel`` (``tac.add_noise``: one ``tac_add_noise_f32`` entry, three launches), ``composite`` (torch operators), each as
``fwd`` and as ``fwd_bwd`` (all three gradients through ``torch.autograd.grad``, ``grad_out`` a tensor of its own per batch), and
``clone`` (``x.clone()`` of one operand: the floor of one read and one write).  The kernel route's rate is given against the algorithmic 5 N 4 bytes (two reads by the sums,
two by the mix, one write).

``--variant NAME=LIB`` times the forward entry of another build of the library (``tools/build_variant.sh NAME "-DTAC_AN_MIX_REVERSE=0"
add_noise.hip`` builds the mix kernel that walks its units in the reduce kernel's order instead of the reverse) against the
default build's, both called through ctypes on the same buffers, alternating: the mix-order A/B of DESIGN 3.18.

Batches are visited in turn, enough of them that no operand is served from the 256 MiB last-level cache by an earlier visit; a block
is at least ``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating blocks give
median / min / max.  The spread of ``clone`` is reported: differences between routes mean nothing below it.  Prints ONE JSON line.
Needs the GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

C, N = tac._composite, tac._native
SHAPES = {'speech': (256, 160000), 'long': (8, 8, 2880000)}


def block(fn, batches, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for i in range(iters):
        fn(batches[i % len(batches)])
    stop.record()
    host = (time.perf_counter() - t0) / iters
    stop.synchronize()
    return start.elapsed_time(stop) / iters, host * 1e3


def raw_entry(handle):
    """the forward entry of a library handle on dense (rows, L) operands, through ctypes: ``fn(batch)``"""
    P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    handle.tac_add_noise_f32.argtypes = [P, I64, I64, I64, P, I64, I64, I64, I64, I64, I64, P, I64, P, I64, I32, P, P, P]
    handle.tac_add_noise_f32.restype = ctypes.c_int
    handle.tac_add_noise_work_bytes.argtypes = [I64, I64]
    handle.tac_add_noise_work_bytes.restype = I64

    def fn(batch):
        w, n, snr, lengths = batch['w2'], batch['n2'], batch['snr1'], batch['len1']
        rows, length = w.shape
        rc = handle.tac_add_noise_f32(N.ptr(w), 0, length, 1, N.ptr(n), 0, length, 1, rows, rows, length, N.ptr(snr), rows, N.ptr(lengths), rows, 1,
                                      N.ptr(batch['work']), N.ptr(batch['out']), N.stream_ptr(w.device))
        assert rc == 0, rc
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--json', default='')
    ap.add_argument('--cases', default='speech,long')
    ap.add_argument('--variant', action='append', default=[], help='NAME=path of another build of libtac_amd.so')
    ap.add_argument('--no-backward', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_add_noise.py measures on the GPU only'
    tac.set_strict(True)
    gen = torch.Generator(device='cuda').manual_seed(90)
    handles = {'default': N.lib()}
    for spec in a.variant:
        name, path = spec.split('=', 1)
        handles[name] = ctypes.CDLL(os.path.abspath(path))
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}
    for case in a.cases.split(','):
        shape = SHAPES[case]
        lead, length = shape[:-1], shape[-1]
        rows = 1
        for k in lead:
            rows *= k
        nbytes = 4 * rows * length
        count = max(2, -(-600 * 1000 * 1000 // (3 * nbytes)) + 1)           # operands and outputs of the batches: beyond the cache
        batches = []
        for _ in range(count):
            b = {'w': torch.randn(shape, device='cuda', generator=gen), 'n': torch.randn(shape, device='cuda', generator=gen),
                 'snr': torch.rand(lead, device='cuda', generator=gen) * 30 - 5,
                 'lengths': (length * (0.8 + 0.2 * torch.rand(lead, device='cuda', generator=gen))).long()}
            b['g'] = torch.randn(shape, device='cuda', generator=gen)        # grad_out: memory of its own, as in a training step
            b['w2'], b['n2'], b['snr1'], b['len1'] = b['w'].view(rows, length), b['n'].view(rows, length), b['snr'].reshape(rows), b['lengths'].reshape(rows)
            b['work'] = torch.empty((int(N.lib().tac_add_noise_work_bytes(rows, length)) // 8,), dtype=torch.float64, device='cuda')
            b['out'] = torch.empty((rows, length), device='cuda')
            batches.append(b)

        def fwd_kernel(b):
            return tac.add_noise(b['w'], b['n'], b['snr'], b['lengths'])

        def fwd_composite(b):
            return C.add_noise(b['w'], b['n'], b['snr'], b['lengths'])

        def with_grad(fn):
            def run(b):
                ins = [b[k].detach().requires_grad_(True) for k in ('w', 'n', 'snr')]
                out = fn(dict(b, w=ins[0], n=ins[1], snr=ins[2]))
                return torch.autograd.grad(out, ins, b['g'])
            return run

        routes = {'clone': lambda b: b['w'].clone(), 'fwd_kernel': fwd_kernel, 'fwd_composite': fwd_composite}
        if not a.no_backward:
            routes['fwd_bwd_kernel'] = with_grad(fwd_kernel)
            routes['fwd_bwd_composite'] = with_grad(fwd_composite)
        for name, handle in handles.items():
            routes['entry_' + name] = raw_entry(handle)
        res = {'shape': list(shape), 'batches': count, 'operand_MB': round(nbytes / 1e6, 1)}
        before = dict(tac._hip.launches)
        got = fwd_kernel(batches[0])
        res['tac_entries_per_call'] = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        ref = fwd_composite(batches[0])
        res['max_abs_kernel_minus_composite'] = float((got - ref).abs().max())
        for name in handles:
            routes['entry_' + name](batches[0])
            res['entry_%s_equals_kernel' % name] = bool(torch.equal(batches[0]['out'].view(shape), got))
        del got, ref
        iters = {}
        for name, fn in routes.items():                            # warm-up, and the block length that fills min-seconds
            block(fn, batches, count)
            per_call = block(fn, batches, count)[0]
            iters[name] = max(count, int(a.min_seconds * 1e3 / per_call) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, batches, iters[name])[0])
        for name in routes:
            t = times[name]
            res[name] = {'ms_median': round(statistics.median(t), 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                         'iters_per_block': iters[name]}
        cl = res['clone']
        res['clone_spread'] = round((cl['ms_max'] - cl['ms_min']) / cl['ms_median'], 4)
        cl['TB_per_s'] = round(2 * nbytes / (cl['ms_median'] * 1e-3) / 1e12, 3)
        for name in ['fwd_kernel'] + ['entry_' + h for h in handles]:
            res[name]['TB_per_s_of_5N'] = round(5 * nbytes / (res[name]['ms_median'] * 1e-3) / 1e12, 3)
        res['fwd_composite_over_kernel'] = round(res['fwd_composite']['ms_median'] / res['fwd_kernel']['ms_median'], 3)
        if not a.no_backward:
            res['fwd_bwd_composite_over_kernel'] = round(res['fwd_bwd_composite']['ms_median'] / res['fwd_bwd_kernel']['ms_median'], 3)
        for name in handles:
            if name != 'default':
                res['entry_%s_over_default' % name] = round(res['entry_' + name]['ms_median'] / res['entry_default']['ms_median'], 4)
        line[case] = res
        del batches
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
