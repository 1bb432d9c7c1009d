#!/usr/bin/env python
"""Generate tests/golden/g13_dct.npz with ``scipy.fft.dct`` — an implementation independent of the closed form in
tests/dct_rules.py and of ``functional.create_dct`` (needs scipy; no test imports it).

    python tests/golden/make_golden_dct.py

For every (num_mels, num_coeffs) of ``dct_rules.GOLDEN_SIZES``: ``x_<M>`` — 16 seeded standard-normal float64 frames (16, M) — and,
for norm None ('none') and 'ortho', ``y_<M>_<C>_<norm>`` = ``scipy.fft.dct(x, type=2, norm=norm, axis=-1)[:, :C]`` in float64."""
import os
import sys

import numpy as np
from scipy.fft import dct

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dct_rules as R  # noqa: E402

FRAMES = 16


def main():
    out = {}
    for num_mels, num_coeffs in R.GOLDEN_SIZES:
        x = np.random.default_rng(1300 + num_mels).standard_normal((FRAMES, num_mels))
        out['x_%d' % num_mels] = x
        for norm in (None, 'ortho'):
            out['y_%d_%d_%s' % (num_mels, num_coeffs, R.norm_tag(norm))] = dct(x, type=2, norm=norm, axis=-1)[:, :num_coeffs]
    np.savez(R.GOLDEN, **out)
    print('wrote %s: %d bytes' % (R.GOLDEN, os.path.getsize(R.GOLDEN)))


if __name__ == '__main__':
    main()
