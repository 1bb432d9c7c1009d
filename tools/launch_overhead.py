#!/usr/bin/env python
"""Host-side cost of one launch on the general ctypes path: issue time of one small call (the kernel is then a few microseconds,
so the loop is bound by Python + ctypes), as tools/host_overhead.py takes it for the fused pipeline.
``python tools/launch_overhead.py [ROOT] [OP]`` measures the package under ROOT (default: this checkout) — for A/B runs of two
trees.  OP: ``complex_norm`` (the default: an 8-pair tensor, no table), ``apply_filterbank`` (a (1, 33, 16) spectrogram with a
(33, 8) bank: one pack look-up per call) or ``istft`` (fft_length 64, hop 16, 9 frames: one envelope look-up per call)."""
import os, sys, time
import torch
root = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
op = sys.argv[2] if len(sys.argv) > 2 else 'complex_norm'
sys.path.insert(0, os.path.abspath(root))
import torchaudio_contrib_amd as tac
if op == 'complex_norm':
    z = torch.rand(8, 2, device='cuda') * 2 - 1
    call = lambda: tac.complex_norm(z)
elif op == 'apply_filterbank':
    spec = torch.rand(1, 16, 33, device='cuda').transpose(-2, -1)       # frame-major, as the spectrogram kernels return it
    fb = tac.create_mel_filter(33, 8, 0.0, 8000.0, False).cuda()
    call = lambda: tac.apply_filterbank(spec, fb)
elif op == 'istft':
    spec = torch.rand(1, 1, 33, 9, 2, device='cuda') * 2 - 1
    window = torch.hann_window(64, device='cuda')
    call = lambda: tac.istft(spec, 64, 16, window=window)
else:
    sys.exit('launch_overhead.py: unknown op %r (complex_norm, apply_filterbank, istft)' % op)
for _ in range(200):
    y = call()
torch.cuda.synchronize()
n = 2000
for repeat in range(3):
    t0 = time.perf_counter()
    for _ in range(n):
        y = call()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print('%s %s repeat %d: issue %.2f us/call   issue+drain %.2f us/call'
          % (os.path.basename(os.path.abspath(root)), op, repeat, (t1 - t0) / n * 1e6, (t2 - t0) / n * 1e6), flush=True)
