#!/usr/bin/env python
"""Generate tests/golden/g11_stretch_chain.npz from the UNMODIFIED reference: its own layer chain
``STFT -> TimeStretch -> ComplexNorm [-> ApplyFilterbank]`` (reference tests/test_layers.py:86-106) at two rates and two powers.

    python tests/golden/make_golden_stretch.py

The reference is imported exactly the way ``make_golden.py`` imports it (same legacy ``torch.stft`` shim, same path); inputs come
from ``oracle.signals``, so only outputs are stored (about 150 KB).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shim and imports the reference)

ref, signals = mg.ref, mg.signals

SHAPE, N_FFT, HOP, N_MELS, SAMPLE_RATE = (2, 1, 4000), 512, 128, 40, 16000
RATES, POWERS = (0.7, 1.3), (1.0, 2.0)
SPEC_KEPT = ((0.7, 1.0), (1.3, 2.0))          # the 257-bin rows are stored for these; the 40-band mel rows for every combination


def main():
    x = torch.from_numpy(signals.audio_like(SHAPE, seed=111))
    n_freqs = N_FFT // 2 + 1
    bank = ref.MelFilterbank(num_freqs=n_freqs, num_mels=N_MELS, sample_rate=SAMPLE_RATE).get_filterbank()
    out = {'bank': mg.np32(bank)}
    for rate in RATES:
        for power in POWERS:
            rows = torch.nn.Sequential(ref.STFT(N_FFT, HOP), ref.TimeStretch(HOP, n_freqs, fixed_rate=rate),
                                       ref.ComplexNorm(power=power))(x)
            if (rate, power) in SPEC_KEPT:
                out['spec_r%g_p%g' % (rate, power)] = mg.np32(rows)
            out['mel_r%g_p%g' % (rate, power)] = mg.np32(ref.ApplyFilterbank(bank)(rows))
    np.savez_compressed(os.path.join(mg.GOLD, 'g11_stretch_chain.npz'), **out)
    print('g11 done, torch', torch.__version__)


if __name__ == '__main__':
    main()
