"""-m gpu: seeded sweeps of ``tac_polyphase_f32`` (through ``resample``) and ``tac_polyphase_wide_f32`` (through
``tac_amd::resample_fit``) over their argument space — strict mode and poisoned outputs on — beside the hand-picked tables of
tests/test_resample_gpu.py and tests/test_pitch_shift_gpu.py.

The generator is ``polyphase_rules.sweep`` (tests/test_polyphase_rules_cpu.py checks it alone): the reduced pair, the filter width,
the rolloff in [0.5, 0.99] (1.0 for the two wide variants nothing else reaches), the method, the Kaiser beta, 1 .. 6 rows, a length a random offset around 0 .. 3 tiles of the variant's
own tile, a layout, forward or gradient — stratified so that every instantiation public arguments reach is drawn at the default
count, by the forward or by the adjoint bank (each one by both: the tables of the two files above).  No tolerance is new: every element against the float64 sum of tests/resample_rules.py under
``(K_n + 2) * 2^-24 * sum |h64| |x|``.

``TAC_FUZZ_CASES=N`` draws N cases per kernel (default 24: a few seconds), ``TAC_FUZZ_SEED`` moves the stream, and
``TAC_FUZZ_REPORT=path`` appends one JSON line per check with the variant and the worst |err| / bound."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import pitch_shift_rules as PS
import polyphase_rules as PR
import resample_rules as R

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get('TAC_FUZZ_CASES', '24'))
SEED = int(os.environ.get('TAC_FUZZ_SEED', '0'))
NAMES = dict(lpw='lowpass_filter_width', rolloff='rolloff', method='resampling_method', beta='beta')


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
    t.set_lazy_fusion(True)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def laid_out(x, layout):
    """the rows of ``x`` on the device: ``polyphase_rules.layout_pad`` floats apart in a NaN-filled store, or dense one float into
    an allocation"""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to('cuda')
    if layout == 'misaligned':
        store = torch.full((x.size + 1,), float('nan'), device='cuda')
        store[1:] = xt.reshape(-1)
        return store[1:].view(x.shape)
    pad = PR.layout_pad(layout, x.shape[1])
    store = torch.full((x.shape[0], x.shape[1] + pad), float('nan'), device='cuda')
    store[:, :x.shape[1]] = xt
    return store[:, :x.shape[1]]


def sixteen_byte_rows(x):
    return x.data_ptr() % 16 == 0 and (x.shape[0] == 1 or x.stride(0) % 4 == 0)


def report(c, worst):
    print('%s %d:%d %r, %d rows of %d to %d, %s, %s: variant %r, worst |err| / bound %.3f' % (
        c.kernel, c.orig, c.new, c.kw, c.rows, c.length, c.out_len, c.layout, 'gradient' if c.gradient else 'forward', c.variant, worst))
    path = os.environ.get('TAC_FUZZ_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(test='polyphase_sweep', kernel=c.kernel, case=list(c[1:9]), gradient=c.gradient,
                                    variant=list(c.variant), worst=worst)) + '\n')


@pytest.mark.parametrize('kernel', [PR.LDS_ENTRY, PR.WIDE_ENTRY])
def test_sweep(tac, kernel):
    cases, drawn, rejected = PR.sweep(kernel, CASES, SEED)
    assert 4 * rejected <= drawn, '%d of %d draws rejected' % (rejected, drawn)
    lds = kernel == PR.LDS_ENTRY
    seen = set()
    for c in cases:
        kw = {NAMES[k]: v for k, v in c.kw.items()}
        key = tac._resample.constants(c.orig, c.new, **kw)
        bank = (tac._resample.adjoint_bank if c.gradient else tac._resample.bank)(*key)
        n_out = R.out_length(c.length, c.orig, c.new)
        x = R.waveform((c.rows, c.length), seed=c.seed)

        def forward(xt):
            before = dict(tac._hip.launches)
            y = tac.resample(xt, c.orig, c.new, **kw) if lds else tac._ops.call('resample_fit', xt, *key, c.out_len)
            assert launched_since(tac, before) == {kernel: 1}, c
            assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == (c.rows, c.out_len), c
            return y

        if not c.gradient:
            xt = laid_out(x, c.layout)
            assert (PR.lds_variant if lds else PR.wide_variant)(bank, sixteen_byte_rows(xt)) == c.variant, c
            got = forward(xt)
            ref, bound = PS.fit_reference(x, c.orig, c.new, c.out_len, **c.kw)
            assert not bool(got[:, n_out:].any()), c
        else:
            g = R.waveform((c.rows, c.out_len), seed=c.seed + 1)
            gt = laid_out(g, c.layout)
            assert (PR.lds_variant if lds else PR.wide_variant)(bank, sixteen_byte_rows(gt)) == c.variant, c
            xt = torch.from_numpy(x).to('cuda').requires_grad_(True)
            y = forward(xt)
            before = dict(tac._hip.launches)
            with warnings.catch_warnings():
                warnings.simplefilter('error', tac.CompositeRouteWarning)
                (got,) = torch.autograd.grad(y, xt, grad_outputs=gt)
            assert launched_since(tac, before) == {kernel: 1}, c
            assert tuple(got.shape) == (c.rows, c.length) and got.is_contiguous(), c
            ref, bound = PS.fit_adjoint_reference(g, c.length, c.orig, c.new, **c.kw)
        report(c, R.assert_close(got, ref, bound, repr(c)))
        seen.add(c.variant[:-1])
    print('%s: %d cases, %d draws, %d rejected; variants launched: %r' % (kernel, len(cases), drawn, rejected, sorted(seen, key=repr)))
