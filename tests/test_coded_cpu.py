"""The coded-input cases of tests/coded_rules.py without a device: the same generator and the same checks through the CPU route
of ``melspectrogram`` (int16 PCM) and ``melspectrogram_mulaw`` (uint8 / int64 codes), the fixed edge cases of
tests/test_coded_gpu.py included.  The keep conditions of the dB rule and the silent-frame conditions are properties of the inputs
and the bounds, not of a kernel: they are established here, on the reference route, before a kernel is held to them.  Also: what the
default run of the generator covers, and its narrowing rules against the host-side packer of the fused kernels' bank tables."""
import numpy as np
import pytest
import torch

import coded_rules as R

CASES = 32          # the default run of tests/test_coded_gpu.py (TAC_FUZZ_CASES), seed 0


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


@pytest.mark.parametrize('block', range(4))
def test_cpu_route_meets_every_rule_on_the_drawn_cases(tac, block):
    for case in range(block * CASES // 4, (block + 1) * CASES // 4):
        c = R.draw(0, case)
        R.run(c, 'cpu', 'coded_cpu_' + c.fmt)


@pytest.mark.parametrize('kind', sorted(R.EDGES))
def test_cpu_route_meets_every_rule_on_the_edge_cases(tac, kind):
    for c in R.edge_cases(kind):
        R.run(c, 'cpu', 'coded_cpu_edges_' + c.fmt)


def test_default_run_covers_what_it_claims():
    seen = set()
    for case in range(CASES):
        seen |= R.covers(R.draw(0, case))
    assert not set(R.COVERAGE) - seen, sorted(set(R.COVERAGE) - seen)


def test_generator_is_a_pure_function_inside_its_space():
    for seed in (0, 3):
        for case in range(256):
            c, again = R.draw(seed, case), R.draw(seed, case)
            assert c == again
            assert c.n in R.SIZES and max(1, c.n // 16) <= c.hop <= c.n and c.n // 4 <= c.win_length <= c.n
            assert c.n + 1 <= c.length <= 12 * c.n and 1 <= len(c.lead) <= 2 and all(1 <= v <= 5 for v in c.lead)
            assert c.power == 2.0 or (c.power == 1.0 and c.n == 2048)
            assert c.num_mels <= c.n // 4 and 0 <= c.offset <= 3 and c.row_pad in (0, 1, 2, 3, 61)
            assert R.coded_entry_covers(c)


def test_layouts_place_the_samples_where_they_say():
    dense = np.arange(2 * 3 * 11, dtype=np.int16).reshape(2, 3, 11) + 1
    for offset in range(4):
        for pad in (0, 1, 3, 61):
            v = R.laid_out(dense, 'int16', offset, pad, None, 'cpu')
            assert v.storage_offset() == offset and v.stride() == (3 * (11 + pad), 11 + pad, 1)
            assert np.array_equal(v.numpy(), dense)
            whole = torch.empty(0, dtype=torch.int16).set_(v.untyped_storage())
            assert int((whole == R.FILL['int16']).sum()) == whole.numel() - dense.size == offset + 6 * pad
    for copy in ('transposed', 'strided'):
        v = R.laid_out(dense, 'int16', 0, 0, copy, 'cpu')
        assert np.array_equal(v.numpy(), dense) and not v.is_contiguous()
        flat = v.reshape(-1, 11)
        assert flat.data_ptr() != v.data_ptr() or flat.stride(1) != 1          # what makes the host copy (``_hip.geometry``)


def test_narrowing_rules_are_the_packers(tac):
    """``coded_rules.bank_fits`` against ``tac_melbank_pack_host`` (the tables of the fused kernels, built without a device) over every
    bank the generator can draw: the rule says yes exactly where the packer accepts the bank in the layout the coded kernels read
    (at 1024 the packer also builds wider tables, of up to 20 steps, which only the float32 kernels are instantiated for)."""
    h = tac._native.lib()
    yes = no = 0
    for n in R.SIZES:
        for rate in R.SAMPLE_RATES:
            for htk in (False, True):
                for count in R.MEL_COUNTS:
                    mels = min(count, n // 4)
                    fb = R.bank(n, mels, rate, htk).numpy()
                    wpack, desc, info = np.zeros(24576, np.float32), np.zeros(8192, np.int32), np.zeros(8, np.int32)
                    rc = h.tac_melbank_pack_host(fb.ctypes.data, fb.shape[0], mels, n, wpack.ctypes.data, wpack.size, desc.ctypes.data,
                                                 desc.size, info.ctypes.data)
                    assert rc in (tac._native.TAC_OK, tac._native.TAC_E_UNSUPPORTED), (n, rate, htk, mels, rc)
                    packs = rc == tac._native.TAC_OK and (n == 2048 or int(info[4]) <= 12)
                    assert R.bank_fits(torch.from_numpy(fb), n) == packs, (n, rate, htk, mels, rc, info.tolist())
                    yes, no = yes + packs, no + (not packs)
    assert yes > 100 and no > 40          # both answers occur: the rule is not vacuous
