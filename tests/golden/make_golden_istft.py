#!/usr/bin/env python
"""Generate tests/golden/g12_stft_backward_pin.npz: the frame gradients ``tac_stft_backward_f32`` writes for a seeded gradient
spectrum at fft_length 2048, 400 and 960, as raw float32 bits.  The frame kernels behind that entry point gained an inverse
(istft) operand mode; the file pins what the gradient mode returned on the commit BEFORE that change, and
tests/test_istft_gpu.py::test_stft_backward_bits_unchanged compares the present build with it bit for bit.

    python tests/golden/make_golden_istft.py --commit <hash of the commit the library was built from> [--out FILE]

Needs a gfx950 device and the built library.  Inputs are regenerated from the seeds below, so only outputs are stored.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

#: (fft_length, hop, win_length, normalized, rows, frames)
CASES = ((2048, 512, 2048, False, 2, 5), (2048, 256, 1200, True, 1, 3), (400, 160, 400, False, 3, 11),
         (400, 100, 256, True, 1, 9), (960, 240, 960, False, 2, 5), (960, 480, 600, True, 1, 4))


def case_inputs(n_fft, hop, win_length, normalized, rows, frames):
    """(gradient spectrum (rows, T, F, 2) float32, window (win_length,) float32), both from fixed seeds."""
    gen = torch.Generator().manual_seed(1200 + n_fft + hop)
    spec = torch.randn(rows, frames, n_fft // 2 + 1, 2, generator=gen, dtype=torch.float32)
    window = torch.hann_window(win_length, periodic=True, dtype=torch.float32) + 0.0625
    return spec, window


def frame_gradients(spec, window, n_fft, hop, win_length, normalized):
    """tac_stft_backward_f32 on cuda:0 through the C ABI: (rows, T, n_fft) float32 on the host."""
    import torchaudio_contrib_amd as tac
    nat = tac._native
    rows, frames = spec.shape[0], spec.shape[1]
    length = hop * (frames - 1)                      # center=True: exactly `frames` frames
    desc = nat.StftDesc(rows=rows, length=length, row_stride=length, n_fft=n_fft, hop=hop, win_length=win_length, center=1,
                        pad_mode=nat.PAD_MODES['constant'], normalized=1 if normalized else 0, onesided=1, reserved=0)
    dev = torch.device('cuda:0')
    gs, w = spec.to(dev).contiguous(), window.to(dev)
    out = torch.full((rows, frames, n_fft), float('nan'), dtype=torch.float32, device=dev)
    with nat.on_device(dev):
        rc = nat.lib().tac_stft_backward_f32(nat.ptr(gs), nat.ptr(w), desc, nat.ptr(out), nat.stream_ptr(dev))
    nat.check(rc, 'tac_stft_backward_f32')
    torch.cuda.synchronize()
    return out.cpu()


def key(n_fft, hop, win_length, normalized, rows, frames):
    return 'n%d_h%d_w%d_%s' % (n_fft, hop, win_length, 'norm' if normalized else 'plain')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit the library under test was built from')
    ap.add_argument('--out', default=os.path.join(HERE, 'g12_stft_backward_pin.npz'))
    args = ap.parse_args()
    out = {'commit': np.array(args.commit), 'torch': np.array(torch.__version__)}
    for case in CASES:
        spec, window = case_inputs(*case)
        fr = frame_gradients(spec, window, *case[:4])
        assert bool(torch.isfinite(fr).all()), case
        out[key(*case)] = fr.numpy().view(np.uint32)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print('g12 done on', args.commit, {k: v.shape for k, v in out.items() if k.startswith('n')})


if __name__ == '__main__':
    main()
