#!/usr/bin/env python
"""Time ``rtf_evd`` / ``rtf_power`` / ``mvdr_weights_rtf`` / ``RTFMVDR`` and the chains ``psd → rtf_evd | rtf_power → RTFMVDR`` on the
gfx950 kernels (csrc/beamform.hip) against the same calls through ``_composite`` (torch operators: ``linalg.eigh`` / ``solve`` /
``matmul`` / ``einsum``) on the same device, in one process, with the Souden ``MVDR`` entry as the neighbour.

    python tools/bench_rtf.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases array,long] [--composite-calls 2]

Shapes (batch, channels, bins, frames), frame-major as ``stft`` returns them — those of tools/bench_beamform.py:

    array       (16, 8, 257, 1000)      16 utterances of 10 s from 8 microphones at fft_length 512
    long        (8, 8, 2049, 2813)      one minute at 48 kHz, fft_length 4096

Routes (kernel; each has a ``composite`` twin timed over ``--composite-calls`` single calls after one warm-up call, 0: not at all,
with the device kernels of one call counted by torch's profiler):

    rtf_evd / rtf_power / mvdr_weights_rtf      one launch each, on PSDs (and an RTF) made beforehand
    rtfmvdr                                     ``tac.RTFMVDR()``: one ``tac_rtf_mvdr_f32`` entry, two launches
    chain_evd / chain_power                     ``_hip.psd`` (both masks, one pass) → the RTF → ``RTFMVDR``
    souden_weights / psd / souden               the Souden weights launch, the PSD launch pair and the whole ``MVDR`` entry

Batches are visited in turn, enough of them that no spectrogram is served from the 256 MiB last-level cache by an earlier visit (the
PSD-only routes read 2 to 17 MB a batch and are served from it, as they are behind the PSD launch of a real chain); a block is at
least ``--min-seconds`` of calls between two device events after a warm-up of every route; ``--repeats`` alternating blocks give
median / min / max.  Prints ONE JSON line.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402
from bench_beamform import CASES, block, scene, launches_of  # noqa: E402


def entries(fn):
    before = dict(tac._hip.launches)
    out = fn()
    return out, {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--json', default='')
    ap.add_argument('--cases', default='array,long')
    ap.add_argument('--composite-calls', type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_rtf.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(29)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}
    H, Cp = tac._hip, tac._composite
    mvdr, rtfmvdr = tac.MVDR(), tac.RTFMVDR()
    for case in a.cases.split(','):
        shape = CASES[case]
        B, C, F, T = shape
        spec_bytes = 8 * B * C * F * T
        count = max(2, -(-600 * 1000 * 1000 // spec_bytes) + 1)
        tac.set_strict(True)
        batches = []
        for _ in range(count):                                     # (x, ms, mn, psd_s, psd_n, rtf), all pairs
            x, ms, mn = scene(shape, gen)
            ps, pn = H.psd(x, ms, mn, normalize=True, eps=1e-15)
            batches.append((x, ms, mn, ps, pn, H.rtf_evd(ps)))
        none = tac._beamform.none(batches[0][0])

        def chain(rtf_of):
            def run(x, ms, mn, ps, pn, d):
                ps, pn = H.psd(x, ms, mn, normalize=True, eps=1e-15)
                return H.rtf_mvdr(x, rtf_of(ps, pn), pn, None, 0, True, 1e-7, 1e-8)[0]
            return run

        def composite_chain(rtf_of):
            def run(x, ms, mn, ps, pn, d):
                ps, pn = Cp.psd(x, ms, True, 1e-15), Cp.psd(x, mn, True, 1e-15)
                return Cp.rtf_mvdr(x, rtf_of(ps, pn), pn, none, 0)
            return run

        routes = {
            'rtf_evd': lambda x, ms, mn, ps, pn, d: H.rtf_evd(ps),
            'rtf_power': lambda x, ms, mn, ps, pn, d: H.rtf_power(ps, pn, None, 0, 3, True, 1e-7),
            'mvdr_weights_rtf': lambda x, ms, mn, ps, pn, d: H.mvdr_weights_rtf(d, pn, None, 0, True, 1e-7, 1e-8),
            'rtfmvdr': lambda x, ms, mn, ps, pn, d: rtfmvdr(x, d, pn, 0),
            'chain_evd': chain(lambda ps, pn: H.rtf_evd(ps)),
            'chain_power': chain(lambda ps, pn: H.rtf_power(ps, pn, None, 0, 3, True, 1e-7)),
            'souden_weights': lambda x, ms, mn, ps, pn, d: H.mvdr_weights_souden(ps, pn, None, 0, True, 1e-7, 1e-8),
            'psd': lambda x, ms, mn, ps, pn, d: H.psd(x, ms, mn, normalize=True, eps=1e-15),
            'souden': lambda x, ms, mn, ps, pn, d: mvdr(x, ms, mn),
        }
        composites = {
            'rtf_evd': lambda x, ms, mn, ps, pn, d: Cp.rtf_evd(ps),
            'rtf_power': lambda x, ms, mn, ps, pn, d: Cp.rtf_power(ps, pn, none, 0, 3),
            'mvdr_weights_rtf': lambda x, ms, mn, ps, pn, d: Cp.mvdr_weights_rtf(d, pn, none, 0),
            'rtfmvdr': lambda x, ms, mn, ps, pn, d: Cp.rtf_mvdr(x, d, pn, none, 0),
            'chain_evd': composite_chain(lambda ps, pn: Cp.rtf_evd(ps)),
            'chain_power': composite_chain(lambda ps, pn: Cp.rtf_power(ps, pn, none, 0, 3)),
        }
        res = {'shape': list(shape), 'systems': B * F, 'batches': count, 'spec_MB': round(spec_bytes / 1e6, 1),
               'psd_MB': round(8 * B * F * C * C / 1e6, 1)}
        layout = dict(H.beamform_layout)
        got, res['tac_entries_per_call'] = {}, {}
        for name, fn in routes.items():
            got[name], res['tac_entries_per_call'][name] = entries(lambda: fn(*batches[0]))
            again = fn(*batches[0])
            same = all(torch.equal(g, w) for g, w in zip(got[name], again)) if isinstance(again, tuple) else torch.equal(got[name], again)
            assert same, name + ': two calls differ'
        res['spec_read_in_place'] = H.beamform_layout['copied'] == layout['copied']
        res['kernel_launches_per_call'] = {name: launches_of(lambda: fn(*batches[0])) for name, fn in routes.items()}
        assert res['spec_read_in_place'] and res['tac_entries_per_call']['rtfmvdr'] == {'tac_rtf_mvdr_f32': 1}, res
        iters = {}
        for name, fn in routes.items():                            # warm-up, and the block length that fills min-seconds
            block(fn, batches, count)
            per_call = block(fn, batches, count)
            iters[name] = max(count, int(a.min_seconds * 1e3 / per_call) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, fn in routes.items():
                times[name].append(block(fn, batches, iters[name]))
        for name in routes:
            t = times[name]
            res[name] = {'ms_median': round(statistics.median(t), 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                         'iters_per_block': iters[name]}
        for name in ('rtf_evd', 'rtf_power', 'mvdr_weights_rtf'):
            res[name]['over_souden_weights'] = round(res[name]['ms_median'] / res['souden_weights']['ms_median'], 2)
            res[name]['over_psd'] = round(res[name]['ms_median'] / res['psd']['ms_median'], 2)
        if a.composite_calls > 0:
            tac.set_strict(False)
            res['composite'] = {}
            for name, fn in composites.items():
                ref = fn(*batches[0])                               # warm-up: the allocator's blocks and every operator's first call
                mine = got[name]
                diff = float((ref - mine).abs().max() / ref.abs().max())
                del ref
                single = []
                for i in range(a.composite_calls):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(*batches[i % count])
                    torch.cuda.synchronize()
                    single.append((time.perf_counter() - t0) * 1e3)
                res['composite'][name] = {'ms_single_calls': [round(t, 2) for t in single],
                                          'launches_per_call': launches_of(lambda: fn(*batches[0])),
                                          'max_abs_difference_over_max': diff,
                                          'composite_over_kernel': round(min(single) / res[name]['ms_median'], 1)}
                torch.cuda.empty_cache()
            tac.set_strict(True)
        else:
            res['composite'] = 'not measured'
        line[case] = res
        del batches, got
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
