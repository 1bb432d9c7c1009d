#!/usr/bin/env python
"""Host-only cost of a table look-up that hits: no device, no library.  A CPU tensor gets the slot a first call would have left
(``(stamp, {key: table})``, the layout ``_tac_pack`` and ``_tac_istft`` had before ``cached_on`` carried them, and have now),
then ``_melbank_pack`` and ``istft_envelope`` are called 200 000 times each; the best of five rounds is printed, with ``_stamp``
alone beside them.  ``python tools/table_hit_cost.py [ROOT]`` measures the package under ROOT (default: this checkout) — for A/B
runs of two trees; pin it to one core (``taskset -c N``) on a shared host."""
import os, sys, time
import torch
root = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(root))
import torchaudio_contrib_amd as tac
H = tac._hip
fb = torch.rand(33, 8)
window = torch.hann_window(64)
fb._tac_pack = (H._stamp(fb), {0: ('wpack', 'desc', 'info')})
window._tac_istft = (H._stamp(window), {(64, 16, 64, True, 9): (torch.ones(192), {128})})


def best(call, n=200000):
    low = float('inf')
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        low = min(low, (time.perf_counter() - t0) / n)
    return low * 1e6


print('%s: pack hit %.3f us   envelope hit %.3f us   stamp %.3f us'
      % (os.path.basename(os.path.abspath(root)), best(lambda: H._melbank_pack(fb, 0)),
         best(lambda: H.istft_envelope(window, 64, 16, 64, True, 9, 128)), best(lambda: H._stamp(fb))), flush=True)
