"""-m gpu: every persistent kernel of the STFT chain with more units than its grid has workgroups — strict mode and poisoned outputs
on, as in the files of the ops themselves.

tests/test_gpu_fullsize.py walks the chain past its grid at three geometries (2048 / 512, 4096 / 1024, 400 / 160, one-sided, Hann);
every other instantiation saw `(2, 2, 9000)`-sized inputs, whose workgroups take one unit and leave.  Here the sizes come from
``grid_rules.chain_shapes`` for the CU count of the device (two rounds of the grid and a remainder), every case holds them to the
restated launcher (``grid_rules.assert_wraps``) before it launches, asserts its entry point by the launch counters and its
instantiation by the route the launcher records, and runs the body of tests/chain_wrap_rules.py — the same body
tests/test_chain_wrap_rules_cpu.py runs on the CPU route.  No tolerance is new."""
import pytest
import torch

import chain_wrap_rules as CW
import grid_rules as G

pytestmark = pytest.mark.gpu

CASES = G.chain_shapes(G.CU_COUNTS[0])           # (the names; the sizes are taken for the device's CU count)


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    yield t
    t._hip.set_poison_outputs(False)
    t.set_strict(False)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


@pytest.fixture(scope='module')
def cus(tac):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def wrapping(cus_, name):
    """the sizes of case ``name`` on this device, held to the restated grid before anything is launched"""
    c = G.chain_shapes(cus_)[name]
    ratio = G.assert_wraps(cus_, name, c)
    print('%s on %d CUs: %.3f rounds of the grid' % (name, cus_, ratio))
    return c


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'long' and not c['gradient'] and not c['inverse']])
def test_long_rows_beyond_the_grid(tac, cus, name):
    c = wrapping(cus, name)
    worst, bound = CW.long_rows_body(tac, 'cuda', name, c)
    print('%s, 3 rows of %d frames on %s: worst %s %.3g of %.1g'
          % (name, c['n_frames'], c['route'], 'share the dB mask leaves out' if c['db'] else 'frame', worst, bound))


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'short' and not c['gradient'] and not c['inverse']])
def test_short_rows_beyond_the_grid(tac, cus, name):
    c = wrapping(cus, name)
    worst, bound, bits = CW.short_rows_body(tac, 'cuda', name, c)
    print('%s, %d rows of %d frames on %s: worst %s %.3g of %.1g, the base rows\' bits repeated: %s'
          % (name, c['rows'], c['n_frames'], c['route'], 'share the dB mask leaves out' if c['db'] else 'frame', worst, bound, bits))


def test_float64_magphase_elements_beyond_the_grid(tac, cus):
    c = wrapping(cus, 'f64 magphase')
    worst, bound = CW.magphase_body(tac, 'cuda', 'f64 magphase', c, wrapping(cus, c['of']))
    print('f64 magphase, %d elements: worst %.3g of %.1g' % (c['elements'], worst, bound))


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'long' and c['gradient']])
def test_gradient_long_rows_beyond_the_grid(tac, cus, name):
    c = wrapping(cus, name)
    worst, bound = CW.gradient_long_rows_body(tac, 'cuda', name, c)
    print('%s, 3 rows of %d frames on %s: worst row %.3g of %.1g' % (name, c['n_frames'], c['route'], worst, bound))


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'short' and c['gradient']])
def test_gradient_short_rows_beyond_the_grid(tac, cus, name):
    c = wrapping(cus, name)
    worst, bound, bits = CW.gradient_short_rows_body(tac, 'cuda', name, c)
    print('%s, %d rows of %d frames: worst row %.3g of %.1g, the base rows\' bits repeated: %s (required: %s)'
          % (name, c['rows'], c['n_frames'], worst, bound, bits, c['same_kernel']))


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'long' and c['inverse']])
def test_istft_long_rows_beyond_the_grid(tac, cus, name):
    c = wrapping(cus, name)
    worst, bound = CW.istft_long_rows_body(tac, 'cuda', name, c)
    print('%s, 3 rows of %d frames on %s: worst block %.3g of %.3g' % (name, c['n_frames'], c['route'], worst, bound))


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'short' and c['inverse']])
def test_istft_short_rows_beyond_the_grid(tac, cus, name):
    c = wrapping(cus, name)
    worst, bound, bits = CW.istft_short_rows_body(tac, 'cuda', name, c)
    print('%s, %d rows of %d frames on %s: worst block %.3g of %.3g, the base rows\' bits repeated: %s'
          % (name, c['rows'], c['n_frames'], c['route'], worst, bound, bits))
