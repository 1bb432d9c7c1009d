#!/usr/bin/env python
"""Time the DCT behind the mel dB rows (csrc/mfcc.hip) and the whole ``MFCC`` chain against ``torch.matmul`` on the same device
tensors, in one process, alternating the routes.

    python tools/bench_mfcc.py [--repeats 7] [--min-seconds 0.5] [--json OUT] [--profile ROUTE]

Shapes: 256 rows x 160 000 samples at fft_length / hop / bands 2048 / 512 / 128 (cfg-2) and 400 / 160 / 80 (the speech front
end), 40 coefficients each.  Routes per shape:

    dct         tac_dct_rows_f32 alone on the mel dB tensor (the frame-major view the fused launch returns)
    matmul      torch.matmul on the same tensor: transpose, matmul, transpose
    mfcc        the whole MFCC chain from the waveform: the fused Melspectrogram + dB launch, then the DCT kernel
    mel_matmul  the chain without the kernel: Melspectrogram -> AmplitudeToDb, then ``matmul``

Four distinct HBM-resident inputs are visited in turn; a block is at least ``--min-seconds`` of calls between two device events,
after a warm-up of every route; ``--repeats`` alternating blocks give median / min / max and the run-to-run spread.  Prints ONE
JSON line; for ``dct`` and ``matmul`` also the achieved bytes/s against the (n_in + n_out) * 4 bytes per frame the product has
to move.  ``--profile dct|matmul|mfcc|mel_matmul`` runs only that route a few times (for rocprofv3 --kernel-trace --stats).
Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchaudio_contrib_amd as tac  # noqa: E402

ROWS, LENGTH, COEFFS = 256, 160000, 40
SHAPES = ((2048, 512, 128), (400, 160, 80))
HBM_BYTES_PER_S = 8e12


def block(fn, inputs, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(inputs[i % len(inputs)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--json', default='')
    ap.add_argument('--profile', default='')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mfcc.py measures on the GPU only'
    result = {'rows': ROWS, 'samples': LENGTH, 'coeffs': COEFFS, 'repeats': a.repeats, 'min_seconds': a.min_seconds,
              'shapes': []}
    for n_fft, hop, mels in SHAPES:
        kw = dict(num_mels=mels, sample_rate=16000, fft_length=n_fft, hop_length=hop)
        gen = torch.Generator(device='cuda').manual_seed(n_fft)
        waves = [torch.rand((ROWS, 1, LENGTH), device='cuda', generator=gen) * 2 - 1 for _ in range(4)]
        mfcc = tac.MFCC(num_coeffs=COEFFS, **kw).cuda()
        mel_db = torch.nn.Sequential(*tac.Melspectrogram(**kw), tac.AmplitudeToDb()).cuda()
        mat = mfcc[4].dct_matrix
        tac.set_strict(True)
        dbs = [mel_db(w) for w in waves]
        by_ptr = {w.data_ptr(): d for w, d in zip(waves, dbs)}

        def matmul(db):
            return torch.matmul(db.transpose(-1, -2), mat).transpose(-1, -2)

        # per route: (callable, inputs it walks over)
        routes = {'dct': (lambda db: tac._hip.dct_rows(db, mat), dbs), 'matmul': (matmul, dbs),
                  'mfcc': (mfcc, waves), 'mel_matmul': (lambda w: matmul(mel_db(w)), waves)}
        before = dict(tac._hip.launches)
        got = mfcc(waves[0])
        chain = {k: v - before.get(k, 0) for k, v in tac._hip.launches.items() if v != before.get(k, 0)}
        worst = float((got - matmul(by_ptr[waves[0].data_ptr()])).abs().max())
        if a.profile:
            fn, inputs = routes[a.profile]
            for _ in range(5):
                for x in inputs:
                    fn(x)
            torch.cuda.synchronize()
            continue
        iters = {}
        for name, (fn, inputs) in routes.items():                  # warm-up, and the block length that fills min-seconds
            block(fn, inputs, 4)
            per_call = block(fn, inputs, 8)
            iters[name] = max(8, int(a.min_seconds * 1e3 / per_call) + 1)
        times = {name: [] for name in routes}
        for _ in range(a.repeats):
            for name, (fn, inputs) in routes.items():
                times[name].append(block(fn, inputs, iters[name]))
        frames = dbs[0].shape[-1]
        moved = ROWS * frames * (mels + COEFFS) * 4
        line = {'fft_length': n_fft, 'hop': hop, 'num_mels': mels, 'frames_per_row': frames, 'frames': ROWS * frames,
                'dct_MB': round(moved / 1e6, 1), 'mfcc_launches': chain, 'max_abs_diff_kernel_vs_matmul': worst}
        for name in routes:
            t = times[name]
            med = statistics.median(t)
            line[name] = {'ms_median': round(med, 4), 'ms_min': round(min(t), 4), 'ms_max': round(max(t), 4),
                          'spread': round((max(t) - min(t)) / med, 4), 'iters_per_block': iters[name]}
            if name in ('dct', 'matmul'):
                line[name]['TB_per_s'] = round(moved / (med * 1e-3) / 1e12, 3)
                line[name]['share_of_8TB_per_s'] = round(moved / (med * 1e-3) / HBM_BYTES_PER_S, 4)
        line['matmul_over_dct'] = round(line['matmul']['ms_median'] / line['dct']['ms_median'], 3)
        line['dct_faster_beyond_spread'] = bool(line['dct']['ms_max'] < line['matmul']['ms_min'])
        line['matmul_faster_beyond_spread'] = bool(line['matmul']['ms_max'] < line['dct']['ms_min'])
        line['mel_matmul_over_mfcc'] = round(line['mel_matmul']['ms_median'] / line['mfcc']['ms_median'], 3)
        result['shapes'].append(line)
        del waves, dbs, by_ptr, mfcc, mel_db
        torch.cuda.empty_cache()
    if a.profile:
        return
    text = json.dumps(result)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
