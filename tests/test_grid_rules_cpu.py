"""Not gpu: tests/grid_rules.py itself.  The shapes it hands tests/test_grid_wrap_gpu.py make every persistent side kernel walk its
loop more than once on a 256- and on a 304-CU part, against the grid restated from the launchers; every launcher expression quoted
there stands verbatim in the source file it names; and the construction the GPU tests rest on — a big batch that repeats a few base
rows or frames gives the base result again, bit for bit — holds for the package's CPU route of ``lfilter``, ``resample`` and
``dct``."""
import os

import numpy as np
import pytest
import torch

import dct_rules
import grid_rules as G
import lfilter_rules
import resample_rules


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


@pytest.mark.parametrize('cus', G.CU_COUNTS)
def test_every_shape_wraps_its_grid(cus):
    cases = G.shapes(cus)
    chain = G.chain_shapes(cus)                      # (the STFT chain's part: tests/test_chain_wrap_rules_cpu.py holds it to more)
    assert len(cases) == 23 + len(chain) and all(cases[name] == c for name, c in chain.items())
    for name, c in cases.items():
        ratio = G.assert_wraps(cus, name, c)
        print('%d CUs, %s: work / grid %.3f, largest tensor %.0f MB' % (cus, name, ratio, 4e-6 * c['floats']))
    # the rule has teeth: every case cut to three rows (one row of 257 frames, a 150 x 150 plane: the most the files of the ops
    # themselves take) fails it
    for name, c in cases.items():
        if name in chain:
            continue
        cut = dict(c, rows=min(3, c['rows']))
        if c['entry'] == 'tac_dct_rows_f32':
            cut['n_frames'] = 257
        if c['entry'] == 'tac_hpss_backward_f32':
            cut['n_freqs'] = cut['n_frames'] = 150
        with pytest.raises(AssertionError, match='rounds|round'):
            G.assert_wraps(cus, name + ', cut', cut)


def test_the_sizes_on_a_256_cu_part():
    """the figures the rules were written down with"""
    s = G.shapes(256)
    assert s['lfilter, float loads']['rows'] == 2 * 512 + 5 and s['lfilter, float loads']['length'] == 16384 + 37
    assert s['resample 160:441']['n_out'] > 3 * 1024 and s['resample 160:441']['rows'] * 4 == 2 * 5 * 256 + 4    # 5 per CU: 31 KB of LDS
    assert s['resample 2:1']['rows'] * 4 == 2 * 2048 + 4 and (s['resample 2:1']['tile'], s['resample 2:1']['per_cu']) == (1024, 8)
    assert (s['resample 12:1']['tile'], s['resample 12:1']['per_cu'], s['resample 12:1']['rows'] * 4) == (512, 6, 2 * 6 * 256 + 4)
    assert (s['resample 16:1']['tile'], s['resample 16:1']['per_cu']) == (256, 8) and 3 * 256 < s['resample 16:1']['n_out'] < 4 * 256
    g = s['resample 1:12 gradient']
    assert (g['tile'], g['per_cu']) == (512, 6) and 3 * 512 < g['length'] < 4 * 512 and G.polyphase_form(1, 12) == (1024, 8)
    assert G.dct_tile(40, 13) == (64, 16384) and G.dct_tile(256, 128)[0] == 16 and G.DCT_LDS_BYTES // G.dct_tile(256, 128)[1] == 1
    assert s['dct 256 x 128, 1 row']['n_frames'] == (2 * 256 + 4) * 16 + 1
    assert [G.mac_tile(p) for p in (4, 8, 16, 17)] == [16, 32, 64, 80]
    assert s['hpss gradient']['n_frames'] == 1200 and s['istft gradient']['rows'] == 8
    assert G.persistent_blocks(0, 4, 7) == 1 and G.persistent_blocks(9, 4, 7) == 3 and G.persistent_blocks(99, 4, 7) == 7


def test_quoted_launcher_expressions_are_in_the_sources(tac):
    csrc = os.path.join(os.path.dirname(os.path.abspath(tac.__file__)), 'csrc')
    for name, quotes in G.QUOTED:
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        for q in quotes:
            assert q in text, '%s no longer holds %r: tests/grid_rules.py restates a launcher that has changed' % (name, q)
    # the constants the Python side mirrors
    assert tac._hip.LFILTER_TILE == G.LFILTER_TILE and tac._hip.RESAMPLE_TILE == G.POLYPHASE_TILE
    for orig, new in ((2, 1), (3, 2), (160, 441)):
        key = tac._resample.constants(orig, new)
        assert tac._hip.resample_tile(tac._resample.bank(*key)) == G.POLYPHASE_TILE
    assert tac._hip.resample_tile(tac._resample.adjoint_bank(*tac._resample.constants(3, 2))) == G.POLYPHASE_TILE
    for orig, new in ((12, 1), (16, 1), (1, 12), (160, 441)):
        key = tac._resample.constants(orig, new)
        for adjoint, bank in ((False, tac._resample.bank(*key)), (True, tac._resample.adjoint_bank(*key))):
            assert tac._hip.resample_tile(bank) == G.polyphase_form(orig, new, adjoint)[0]


# ----------------------------------------------------------------------------- big batch = repeated base rows, on the CPU route
def repeat_rows(base, rows):
    """row r = base[r % len(base)]"""
    return base[torch.arange(rows) % base.shape[0]].contiguous()


def test_repeated_rows_repeat_the_result_lfilter(tac):
    base = lfilter_rules.waveform((G.BASE_ROWS, 301), seed=1)
    for name, b, a in lfilter_rules.filters(tac):
        if name not in ('high-pass 100 Hz at 16 kHz', 'preemphasis 0.97'):
            continue
        bt, at = torch.tensor(b, dtype=torch.float64), torch.tensor(a, dtype=torch.float64)
        small = tac.lfilter(torch.from_numpy(base), at, bt, clamp=False)
        ref, bound = lfilter_rules.reference(base, b, a)
        lfilter_rules.assert_close(small, ref, bound, name)
        big = tac.lfilter(repeat_rows(torch.from_numpy(base), 23), at, bt, clamp=False)
        assert big.shape == (23, 301) and torch.equal(big.view(torch.int32), repeat_rows(small, 23).view(torch.int32)), name


def test_repeated_rows_repeat_the_result_resample(tac):
    for orig, new in ((2, 1), (3, 2), (160, 441), (12, 1), (16, 1), (1, 12)):
        base = resample_rules.waveform((G.BASE_ROWS, 311), seed=orig)
        small = tac.resample(torch.from_numpy(base), orig, new)
        resample_rules.assert_within(small, base, orig, new, 'resample %d:%d' % (orig, new))
        big = tac.resample(repeat_rows(torch.from_numpy(base), 23), orig, new)
        assert big.shape[0] == 23 and torch.equal(big.view(torch.int32), repeat_rows(small, 23).view(torch.int32)), (orig, new)


def test_repeated_frames_repeat_the_result_dct(tac):
    for n_in, n_out in ((40, 13), (256, 128)):
        d32, d64 = tac.create_dct(n_out, n_in, 'ortho'), dct_rules.dct_matrix64(n_out, n_in, 'ortho')
        base = dct_rules.db_like((1, n_in, G.BASE_FRAMES), seed=n_in)
        small = tac.dct(torch.from_numpy(base), d32)
        dct_rules.assert_within(small, base, d64, 'dct %d x %d' % (n_in, n_out))
        frames = torch.arange(331) % G.BASE_FRAMES
        one_row = torch.from_numpy(base)[..., frames].contiguous()
        big = tac.dct(one_row, d32)
        assert big.shape == (1, n_out, 331) and torch.equal(big.view(torch.int32), small[..., frames].view(torch.int32)), (n_in, n_out)
        three = tac.dct(torch.from_numpy(np.ascontiguousarray(np.broadcast_to(one_row.numpy(), (3, n_in, 331)))), d32)
        assert torch.equal(three.view(torch.int32), big.expand(3, n_out, 331).view(torch.int32)), (n_in, n_out)
