#!/usr/bin/env python
"""Time ``ctc_beam_search`` on the gfx950 kernels (csrc/ctc_decode.hip) — one entry of two launches — against what stands next to
it: a ``clone`` of the logits and ``torch.topk(k=11)`` for the first launch (the frame tables), and the package's own composite
(class lists by torch operators, the beam in Python on the host) with the logits on the device and on the host, in one process.

    python tools/bench_ctc_decode.py [--repeats 5] [--min-seconds 0.2] [--json OUT] [--cases bpe,small,chars] [--composite-calls 1]

Shapes (batch, time, class), beam:

    bpe         (32, 1500, 5000), 10    a BPE vocabulary
    small       (32, 750, 500), 10      a smaller vocabulary
    chars       (1, 3000, 32), 32       characters, latency only

Lengths go down to 60 % of the maximum; every case runs at the thresholds 0.95 and 1.0.  A block is at least ``--min-seconds`` of
calls between two device events after a warm-up; ``--repeats`` blocks give median / min / max in ms per call.  ``tables`` is the
entry with a threshold of -1: every frame is skipped, so the first launch does all its work and the second reads one flag per
frame; ``us_per_kept_frame`` is (entry - tables) over the most kept frames of an entry.  The composites are timed over single calls
after none (they are seconds long) and compared with the kernel's tokens.  Prints ONE JSON line.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

CASES = {'bpe': ((32, 1500, 5000), 10), 'small': ((32, 750, 500), 10), 'chars': ((1, 3000, 32), 32)}


def block(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def measure(routes, repeats, min_seconds):
    iters, times = {}, {name: [] for name in routes}
    for name, fn in routes.items():                                # warm-up, and the block length that fills min-seconds
        block(fn, 1)
        iters[name] = max(2, int(min_seconds * 1e3 / block(fn, 2)) + 1)
    for _ in range(repeats):
        for name, fn in routes.items():
            times[name].append(block(fn, iters[name]))
    return {name: {'ms_median': round(statistics.median(t), 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                   'iters_per_block': iters[name]} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--json', default='')
    ap.add_argument('--cases', default='bpe,small,chars')
    ap.add_argument('--composite-calls', type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ctc_decode.py measures on the GPU only'
    gen = torch.Generator(device='cuda').manual_seed(37)
    line = {'repeats': a.repeats, 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0),
            'cus': torch.cuda.get_device_properties(0).multi_processor_count}
    H, Cp = tac._hip, tac._composite
    for case in a.cases.split(','):
        (B, T, C), K = CASES[case]
        tac.set_strict(True)
        logits = torch.randn((B, T, C), device='cuda', generator=gen) * 3
        logits[:, 1::3, 0] += 12                                    # every third frame is nearly certain of the blank
        lp = torch.log_softmax(logits, dim=-1)
        del logits
        lens_host = [max(1, round(T * (1.0 - 0.4 * i / max(B - 1, 1)))) for i in range(B)]
        lens = torch.tensor(lens_host, dtype=torch.int32, device='cuda')
        res = {'shape': [B, T, C], 'beam': K, 'logits_MB': round(B * T * C * 4 / 1e6, 1)}
        res['stock'] = measure({'clone': lambda: lp.clone(), 'topk11': lambda: torch.topk(lp, 11, dim=-1)}, a.repeats, a.min_seconds)
        res['tables'] = measure({'tables': lambda: tac.ctc_beam_search(lp, lens, K, 1, 0, -1.0)}, a.repeats, a.min_seconds)['tables']
        for thr in (0.95, 1.0):
            before = dict(H.launches)
            want = tac.ctc_beam_search(lp, lens, K, 1, 0, thr)
            launched = {k: v - before.get(k, 0) for k, v in H.launches.items() if v != before.get(k, 0)}
            assert launched == {'tac_ctc_beam_search_f32': 1}, launched
            kept = int(((lp[:, :, 0].exp() <= thr) & (torch.arange(T, device='cuda')[None] < lens[:, None])).sum(dim=1).max())
            r = measure({'entry': lambda: tac.ctc_beam_search(lp, lens, K, 1, 0, thr)}, a.repeats, a.min_seconds)['entry']
            r['launches_per_call'], r['kept_frames'] = launched, kept
            r['us_per_kept_frame'] = round((r['ms_median'] - res['tables']['ms_median']) * 1e3 / max(kept, 1), 3)
            if a.composite_calls > 0:
                tac.set_strict(False)
                lp_host, lens_cpu = lp.cpu(), lens.cpu()
                for name, args in (('composite_device_logits', (lp, lens)), ('composite_host_logits', (lp_host, lens_cpu))):
                    single = []
                    for _ in range(a.composite_calls):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        got = Cp.ctc_beam_search(args[0], args[1], K, 1, 0, thr)
                        torch.cuda.synchronize()
                        single.append((time.perf_counter() - t0) * 1e3)
                        print('%s %s %s: %.0f ms' % (case, thr, name, single[-1]), file=sys.stderr, flush=True)
                    r[name] = {'ms_single_calls': [round(t, 1) for t in single],
                               'same_tokens_as_kernel': bool(torch.equal(got[0].cpu(), want[0].cpu())),
                               'max_score_difference': float((got[2].cpu() - want[2].cpu()).abs().max()),
                               'composite_over_kernel': round(min(single) / r['ms_median'], 1)}
                del lp_host
                tac.set_strict(True)
            res['threshold_%s' % thr] = r
        line[case] = res
        del lp, want
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
