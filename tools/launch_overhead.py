#!/usr/bin/env python
"""Host-side cost of one launch on the general ctypes path: issue time of ``tac.complex_norm`` on an 8-pair tensor (the kernel is
then a few microseconds, so the loop is bound by Python + ctypes), as tools/host_overhead.py takes it for the fused pipeline.
``python tools/launch_overhead.py [ROOT]`` measures the package under ROOT (default: this checkout) — for A/B runs of two trees."""
import os, sys, time
import torch
root = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(root))
import torchaudio_contrib_amd as tac
z = torch.rand(8, 2, device='cuda') * 2 - 1
for _ in range(200):
    y = tac.complex_norm(z)
torch.cuda.synchronize()
n = 2000
for repeat in range(3):
    t0 = time.perf_counter()
    for _ in range(n):
        y = tac.complex_norm(z)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print('%s repeat %d: issue %.2f us/call   issue+drain %.2f us/call'
          % (os.path.basename(os.path.abspath(root)), repeat, (t1 - t0) / n * 1e6, (t2 - t0) / n * 1e6), flush=True)
