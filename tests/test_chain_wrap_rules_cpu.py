"""Not gpu: the STFT-chain part of tests/grid_rules.py and the bodies of tests/chain_wrap_rules.py on the package's CPU route.  Every
chain shape wraps its restated grid on a 256- and on a 304-CU part within the byte cap; the 4-wave form of the generic kernel has
no shape that wraps it; and every body tests/test_chain_grid_wrap_gpu.py runs passes here first — inputs, float64 references and
bounds are sound, and the float32 CPU evaluation stays inside every bound asserted (the dB mask shares included)."""
import pytest
import torch

import chain_wrap_rules as CW
import grid_rules as G

CASES = G.chain_shapes(G.CU_COUNTS[0])


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


@pytest.mark.parametrize('cus', G.CU_COUNTS)
def test_every_chain_shape_wraps_its_grid(cus):
    cases = G.chain_shapes(cus)
    assert set(cases) == set(CASES)
    for name, c in cases.items():
        ratio = G.assert_wraps(cus, name, c)
        print('%d CUs, %s: work / grid %.3f, largest tensor %.0f MB' % (cus, name, ratio, 4e-6 * c['floats']))
        if c['entry'] == 'tac_magphase_f64':
            continue
        # the frames of a row end in a partial group, and the rule has teeth: the (2, 2, 9000)-sized inputs of the other files fail it
        assert c['group'] == 1 or c['n_frames'] % c['group'] != 0, name
        assert c['inverse'] or G.frames_of_length(c['length'], c['n'], c['hop'], c['center']) == c['n_frames'], name
        # (four rows of 9000 samples: 18 frames each at 2048 / 512)
        with pytest.raises(AssertionError, match='rounds'):
            G.assert_wraps(cus, name + ', cut', dict(c, rows=4, n_frames=min(c['n_frames'], 18)))
    # every instantiation the table of the chain names has a case
    routes = {c['route'] for c in cases.values() if 'route' in c}
    for route in ('stft_kernel<32, 16, 0, 1, 1, 8>', 'stft_kernel<2048, 32, 0, 1, 0, 8>', 'stft_pipe_kernel<1024, 16, 0, 8>',
                  'stft_ring3_kernel<1024, 16, 0, 12, 8>', 'stft_stream3_kernel<1024, 16, 0, 12>', 'stft_stream3_kernel<1024, 16, 2, 16>',
                  'stft_small3_kernel<128, 0, 0, 1, 12>', 'stft_small3_kernel<256, 1, 0, 1, 16>', 'stft_smooth_kernel<0, 64>',
                  'stft_smooth_kernel<1, 256>', 'stft_smooth_kernel<0, 256, false>', 'stft_smooth_kernel<1, 256, false>', 'stft_big_kernel<4, 0, 4>', 'stft_big_kernel<8, 1, 8>', 'stft_big_kernel<16, 1, 8>',
                  'stft_n4096_kernel<0>', 'stft_f64_kernel<true>, group 16', 'stft_f64_kernel<true>, group 1',
                  'stft_f64_kernel<false>, group 1', 'stft_f64_direct_kernel',
                  'stft_smooth_backward_kernel<64, true, false>', 'stft_smooth_backward_kernel<256, true, false>',
                  'stft_smooth_backward_kernel<256, false, false>', 'stft_backward_kernel<2048, 32, SRC_GRAD, false>',
                  'melspec_backward_ring3_kernel<true, 2, false>', 'melspec_backward_ring3_kernel<false, 8, false>',
                  'melspec_backward_ring3_kernel<true, 2, true>', 'melspec_backward_ring3_kernel<true, 8, true>',
                  'melspec_backward_ring3_kernel<false, 8, true>',
                  'melspec_backward_ring3_multi_kernel<512, true, 2, false>', 'melspec_backward_ring3_multi_kernel<512, true, 4, false>',
                  'melspec_backward_ring3_multi_kernel<512, true, 8, true>', 'melspec_backward_ring3_multi_kernel<256, false, 2, false>',
                  'melspec_backward_ring3_multi_kernel<256, false, 4, true>', 'melspec_backward_ring3_multi_kernel<256, true, 8, false>',
                  'spectrogram_backward_ola_kernel<true, false, 4>', 'spectrogram_backward_ola_kernel<true, true, 8>',
                  'spectrogram_backward_ola_multi_kernel<512, true>', 'spectrogram_backward_ola_multi_kernel<256, false>',
                  'spectrogram_backward_ola_multi_kernel<128, true>', 'stft_n400_backward_kernel<SRC_WAVE, true, false, false>',
                  'istft_general<960>: frame kernel (inverse mode) + istft_ola_kernel<vec4=1>',
                  'istft_general<400>: frame kernel (inverse mode) + istft_ola_kernel<vec4=1>',
                  'istft_fused_kernel<256>', 'istft_fused_kernel<1024>'):
        assert route in routes, route
    assert [G.smooth_form(n) for n in (300, 4500, 6000)] == [(4, 8, '64'), (1, 2, '256'), (1, 2, '256 half')]
    assert any(c['trim'] for c in cases.values() if c.get('inverse')), 'an istft case with length= trimming'
    assert 'tac_apply_filterbank_adjoint_f32' in cases['gradient ola multi 256 / 64, mel, short rows']['launches']
    assert G.f64_form(6000) == (1, 'stft_f64_kernel<false>, group 1') and G.f64_form(134)[1] == 'stft_f64_direct_kernel'


@pytest.mark.parametrize('cus', G.CU_COUNTS)
def test_the_four_wave_generic_kernel_has_no_shape_that_wraps(cus):
    for nc, e in G.GENERIC_CORES:
        assert G.narrow_generic_never_wraps(cus, nc, e), (cus, nc, e)


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'long' and not c['gradient'] and not c['inverse']])
def test_long_rows_body_on_the_cpu_route(tac, name):
    worst, bound = CW.long_rows_body(tac, 'cpu', name, CASES[name])
    print('%s: worst %s %.3g of %.1g' % (name, 'share the dB mask leaves out' if CASES[name]['db'] else 'frame', worst, bound))


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'short' and not c['gradient'] and not c['inverse']])
def test_short_rows_body_on_the_cpu_route(tac, name):
    worst, bound, bits = CW.short_rows_body(tac, 'cpu', name, CASES[name])
    print('%s: worst %s %.3g of %.1g, the base rows\' bits repeated: %s'
          % (name, 'share the dB mask leaves out' if CASES[name]['db'] else 'frame', worst, bound, bits))


def test_float64_magphase_body_on_the_cpu_route(tac):
    c = CASES['f64 magphase']
    CW.magphase_body(tac, 'cpu', 'f64 magphase', c, CASES[c['of']])


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'long' and c['gradient']])
def test_gradient_long_rows_body_on_the_cpu_route(tac, name):
    worst, bound = CW.gradient_long_rows_body(tac, 'cpu', name, CASES[name])
    print('%s: worst row %.3g of %.1g' % (name, worst, bound))


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'short' and c['gradient']])
def test_gradient_short_rows_body_on_the_cpu_route(tac, name):
    worst, bound, bits = CW.gradient_short_rows_body(tac, 'cpu', name, CASES[name])
    print('%s: worst row %.3g of %.1g, the base rows\' bits repeated: %s' % (name, worst, bound, bits))


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'long' and c['inverse']])
def test_istft_long_rows_body_on_the_cpu_route(tac, name):
    worst, bound = CW.istft_long_rows_body(tac, 'cpu', name, CASES[name])
    print('%s: worst block %.3g of %.3g' % (name, worst, bound))


@pytest.mark.parametrize('name', [n for n, c in CASES.items() if c.get('form') == 'short' and c['inverse']])
def test_istft_short_rows_body_on_the_cpu_route(tac, name):
    worst, bound, bits = CW.istft_short_rows_body(tac, 'cpu', name, CASES[name])
    print('%s: worst block %.3g of %.3g, the base rows\' bits repeated: %s' % (name, worst, bound, bits))
