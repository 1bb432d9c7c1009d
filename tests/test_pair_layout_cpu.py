"""The pair layout of the fused fft_length-2048 kernel (csrc/melspec_sparse.hip pack_pairs, TAC_PACK_PAIRS_2048), checked without a
device through tac_melbank_pack_host: every lane runs three segments of A, B, C four-tap steps — band l; band 64 + l (lanes >= 32:
its first B quads); lanes >= 32 the next C quads of band 64 + l, lanes < 32 the quads of band 96 + l behind those — and lane l + 32
adds the C sum of lane l to its own.  Replaces the contraction of reference functional.py:183-184 for 128-band banks."""
import ctypes
import os

import numpy as np
import pytest

PAIRS = -2048
ROW = 1025 + 7                                  # bins + the zeroed slack floats of a row buffer
# (sample rate, htk) -> total steps: the table of the issue for the three instantiated shapes (4, 6, 4), (4, 7, 3), (3, 7, 5); a bank
# whose minimal shape is not instantiated takes the smallest instantiated one that holds it (15 steps; classic 18 or 20)
BANKS = {(8000, False): 14, (16000, False): 14, (16000, True): 14, (22050, True): 14, (32000, True): 14,
         (22050, False): 15, (32000, False): 15, (44100, False): 15, (48000, False): 15, (44100, True): 15, (48000, True): 15}
SHAPES = ((4, 6, 4), (4, 7, 3), (3, 7, 5))
CLASSIC_STEPS = {(8000, False): 18, (16000, False): 18, (16000, True): 18, (22050, True): 18, (32000, True): 18, (22050, False): 18,
                 (32000, False): 20, (44100, False): 20, (48000, False): 20, (44100, True): 18, (48000, True): 20}


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    if not os.path.exists(t._native.LIB_PATH):
        t.build_native()
    return t


def pack_host(tac, fb, n_fft):
    h = tac._native.lib()
    n_freqs, n_mels = fb.shape
    wpack, desc, info = np.zeros(24576, dtype=np.float32), np.zeros(8192, dtype=np.int32), (ctypes.c_int32 * 8)()
    h.tac_melbank_pack_host.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    rc = h.tac_melbank_pack_host(fb.ctypes.data, n_freqs, n_mels, n_fft, wpack.ctypes.data, wpack.size, desc.ctypes.data, desc.size,
                                 ctypes.cast(info, ctypes.c_void_p))
    return rc, wpack, desc, [int(v) for v in info]


def band_of_cell(seg, lane):
    """the band a cell's sum ends up in (the combine: lane l < 32 hands its segment-C sum to lane l + 32)"""
    if seg == 0:
        return lane
    if seg == 1 or lane >= 32:
        return 64 + lane
    return 96 + lane


@pytest.mark.parametrize('sr,htk', sorted(BANKS))
def test_pair_tables_hold_every_weight_once_and_match_the_dense_product(tac, sr, htk):
    fb = np.ascontiguousarray(tac.create_mel_filter(1025, 128, 0.0, sr / 2.0, htk).numpy().astype(np.float32))
    rc, wpack, desc, info = pack_host(tac, fb, PAIRS)
    assert rc == tac._native.TAC_OK, rc
    total, (A, B, C) = info[3], info[4:7]
    assert info[0] == 256 * total and info[1] == 3 and info[2] == 64 + 512 and total == A + B + C
    assert (A, B, C) in SHAPES and total == BANKS[(sr, htk)] and total < CLASSIC_STEPS[(sr, htk)]
    steps, first = (A, B, C), desc[:192].reshape(3, 64)
    assert (first % 4 == 0).all() and first.min() >= 0
    w = wpack[:256 * total].reshape(total, 64, 4)
    seen = np.zeros(fb.shape, dtype=np.int32)
    base = 0
    for seg in range(3):
        for lane in range(64):
            f0, m = int(first[seg, lane]), band_of_cell(seg, lane)
            assert f0 + 4 * steps[seg] <= ROW, (seg, lane, f0)
            taps = w[base:base + steps[seg], lane].reshape(-1)
            for k in np.nonzero(taps)[0]:
                assert f0 + k < 1025 and taps[k] == fb[f0 + k, m], (seg, lane, int(k))      # an exact copy, in a cell of its band
                seen[f0 + k, m] += 1
        base += steps[seg]
    assert np.array_equal(seen, (fb != 0).astype(np.int32))                 # each non-zero weight exactly once, nothing else
    # the kernel's contraction in float64: three segment sums per lane, then the lane <-> lane + 32 combine
    rng = np.random.default_rng(11)
    rows = np.concatenate([rng.random((3, 1025)), np.zeros((3, 7))], axis=1)
    want = rows[:, :1025] @ fb.astype(np.float64)
    got = np.zeros_like(want)
    for r, row in enumerate(rows):
        seg_sum, base = np.zeros((3, 64)), 0
        for seg in range(3):
            for lane in range(64):
                f0 = int(first[seg, lane])
                seg_sum[seg, lane] = float(w[base:base + steps[seg], lane].reshape(-1).astype(np.float64) @ row[f0:f0 + 4 * steps[seg]])
            base += steps[seg]
        got[r, :64] = seg_sum[0]
        got[r, 64:96] = seg_sum[1, :32]
        got[r, 96:] = seg_sum[1, 32:] + seg_sum[2, 32:] + seg_sum[2, :32]
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # behind the pair table: the classic table of the same bank, bit for bit what n_fft = 2048 packs
    rc2, wpack2, desc2, info2 = pack_host(tac, fb, 2048)
    assert rc2 == tac._native.TAC_OK and info2[1] == 2 and info2[2] == 64 and info2[4] == 4 and info2[5] == info[7]
    assert info2[3] == CLASSIC_STEPS[(sr, htk)]
    assert np.array_equal(wpack[info[0]:info[0] + info2[0]], wpack2[:info2[0]]) and np.array_equal(desc[192:320], desc2[:128])


def test_classic_pack_is_unchanged_by_the_pair_selector(tac):
    """n_fft = 2048 keeps the two-slot (4, 14) table of the benchmark bank: what the gradient path and the coded formats consume"""
    fb = np.ascontiguousarray(tac.create_mel_filter(1025, 128, 0.0, 8000.0, False).numpy().astype(np.float32))
    rc, wpack, desc, info = pack_host(tac, fb, 2048)
    assert rc == tac._native.TAC_OK and info == [256 * 18, 2, 64, 18, 4, 14, 0, 0]


def wide_bank(bins=80):
    """128 bands, the last one `bins` wide: 80 bins are 20 quads, more than B + 2 C of every shape"""
    fb = np.zeros((1025, 128), dtype=np.float32)
    for m in range(127):
        fb[4 * m:4 * m + 6, m] = 0.5
    fb[900:900 + bins, 127] = 0.25
    return fb


GROUPS = ((0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27), (4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31))


def row_read_cycles(first, steps):
    """LDS cycles of a frame's 16-byte row reads: the hardware serves a wave's read in four groups of sixteen lanes, one cycle per
    group plus one for every further DIFFERENT quad on the same bank group ((byte / 16) mod 16); csrc/lane_placement.hpp"""
    total = 0
    for s, n in enumerate(steps):
        for gi in range(4):
            quads = {}
            for i in GROUPS[gi & 1]:
                q = int(first[64 * s + i + 32 * (gi >> 1)]) // 4
                quads.setdefault(q & 15, set()).add(q)
            total += n * max(len(v) for v in quads.values())
    return total


def test_row_reads_of_the_benchmark_pair_table_cost_no_more_lds_cycles_than_the_classic_table(tac):
    """16 kHz Slaney: 14 steps are 56 cycles without conflicts (classic: 18 steps, 72).  Counted on the tables: the classic table takes
    84 cycles (12 of conflicts, all in slot 0), the pair table 80 (24 of conflicts: the same 12 of segment A, and 12 in segment B where
    bands 64 ... 95 fill all six steps and leave no slack; the split bands' pieces are conflict-free).  The other banks are printed."""
    for (sr, htk) in sorted(BANKS):
        fb = np.ascontiguousarray(tac.create_mel_filter(1025, 128, 0.0, sr / 2.0, htk).numpy().astype(np.float32))
        _, _, desc, info = pack_host(tac, fb, PAIRS)
        _, _, desc2, info2 = pack_host(tac, fb, 2048)
        pair, classic = row_read_cycles(desc, info[4:7]), row_read_cycles(desc2, info2[4:6])
        print('row-read LDS cycles per frame, %d Hz %s: pair %s %d (conflict-free %d), classic %s %d (%d)'
              % (sr, 'htk' if htk else 'slaney', info[4:7], pair, 4 * info[3], info2[4:6], classic, 4 * info2[3]))
        if (sr, htk) == (16000, False):
            assert pair <= classic and pair - 4 * info[3] <= 24


@pytest.mark.parametrize('name', ['a widest band of 17 quads', 'htk at 88.2 kHz'])
def test_pair_pack_leaves_banks_whose_classic_table_the_fast_kernels_do_not_run(tac, name):
    """17 quads fit (3, 7, 5) — 7 + 2 x 5 — but the classic table of such a bank is (4, 20): the general kernel's, which the launcher
    could not hand to the kernel forms that contract the classic table behind a pair table.  The bank stays on the classic pack."""
    if name == 'htk at 88.2 kHz':
        fb = np.ascontiguousarray(tac.create_mel_filter(1025, 128, 0.0, 44100.0, True).numpy().astype(np.float32))
    else:
        fb = wide_bank(68)
    rc, _, _, _ = pack_host(tac, fb, PAIRS)
    assert rc == tac._native.TAC_E_UNSUPPORTED
    rc, _, _, info = pack_host(tac, fb, 2048)
    assert rc == tac._native.TAC_OK and info[1:3] == [2, 64] and info[4:6] == [4, 20]


@pytest.mark.parametrize('name', ['40 bands', '160 bands', 'a band wider than every shape'])
def test_pair_pack_refuses_what_no_shape_holds_and_the_classic_pack_takes_it(tac, name):
    if name == 'a band wider than every shape':
        fb = wide_bank()
    else:
        fb = np.ascontiguousarray(tac.create_mel_filter(1025, int(name.split()[0]), 0.0, 8000.0, False).numpy().astype(np.float32))
    rc, _, _, _ = pack_host(tac, fb, PAIRS)
    assert rc == tac._native.TAC_E_UNSUPPORTED
    rc, wpack, desc, info = pack_host(tac, fb, 2048)
    assert rc == tac._native.TAC_OK and info[1] == (fb.shape[1] + 63) // 64 and not info[2] & 512
    assert info[0] == 256 * info[3] == 256 * sum(info[4:4 + info[1]])
