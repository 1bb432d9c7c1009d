"""-m gpu: the pair layout of the fused fft_length-2048 kernel (melspec_stream3_kernel<..., PA, PC>, csrc/melspec_stream3.hpp; tables:
pack_pairs, csrc/melspec_sparse.hip) on the device — reference layers.py:307-381 for 128-band banks.  Lanes 0 .. 31 contract the tail
of the band that lane + 32 owns and hand the sum over with one v_permlane32_swap; the result is the classic layout's sum in another
order.  Held to the float64 per-frame bounds of tests/frame_bounds.py and, in the same process, to the classic layout."""
import numpy as np
import pytest
import torch

import frame_bounds as fbnd
from oracle import signals

pytestmark = pytest.mark.gpu

# two summation orders of at most 64 non-negative float32 terms (a band's taps) differ by at most 2 . 64 . 2^-24 of the value
ORDER_REL = 2.0 * 64.0 * 2.0 ** -24

# (3, 1, 30000): 177 frames — edge frames, silent spans and a silent row, workgroups with one frame or none.
# (12, 1, 150000): 3 516 frames, more than 12 waves x 256 workgroups: every wave draws a second frame from the workgroup's counter.
SHAPES = [(3, 1, 30000), (12, 1, 150000)]
# (sample rate, htk) -> the instantiation's trailing template arguments <..., B + C, waves, A, C>
BANKS = {(16000, False): '10, 12, 4, 4>', (16000, True): '10, 12, 4, 3>', (22050, False): '12, 12, 3, 5>', (44100, False): '12, 12, 3, 5>'}


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    was = t._hip.PAIR_LAYOUT
    t._hip.PAIR_LAYOUT = True                 # (whatever the shipped default: these tests are about the pair layout)
    t.invalidate()
    yield t
    t._hip.PAIR_LAYOUT = was
    t.invalidate()
    t._hip.set_poison_outputs(False)
    t.set_strict(False)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


@pytest.fixture(scope='module')
def inputs():
    return {shape: signals.gained_with_silence(shape, 620, 2048, 512) for shape in SHAPES}


def launched_since(tac_, before):
    now = tac_._hip.launches
    return {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def one_launch(tac, chain, x):
    before = dict(tac._hip.launches)
    out = tac.realize(chain(x))
    assert launched_since(tac, before) == {'tac_melspec_sparse_f32': 1}
    return out.detach().cpu().numpy(), tac._native.lib().tac_last_route().decode()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('sr,htk', sorted(BANKS))
def test_pair_layout_matches_the_oracle_and_the_classic_layout(tac, inputs, shape, sr, htk):
    x = inputs[shape]
    xd = torch.from_numpy(x).cuda()
    for power in (2.0, 1.0):
        layers = list(tac.Melspectrogram(num_mels=128, sample_rate=sr, fft_length=2048, hop_length=512, htk=htk))
        layers[1] = tac.ComplexNorm(power)
        lin_chain = torch.nn.Sequential(*layers).cuda()
        db_chain = torch.nn.Sequential(*layers, tac.AmplitudeToDb()).cuda()
        fb, window = lin_chain[2].filterbank, lin_chain[0].window
        case = (shape, sr, htk, power)
        assert tac._hip.PAIR_LAYOUT
        lin, route = one_launch(tac, lin_chain, xd)
        assert route.startswith('melspec_stream3_kernel<1024, 16, %s, 0, ' % ('true' if power == 2.0 else 'false')) and route.endswith(BANKS[(sr, htk)]), route
        db, route_db = one_launch(tac, db_chain, xd)
        assert route_db == route
        assert not tac._hip.poison_report()
        fbnd.check_frames(lin, fbnd.ref64(x, 2048, 512, window, power, fb), 'spec', 1e-5, 'pair_layout', case, 2048, True)
        fbnd.check_mel_db64(db, x, 2048, 512, fb, 'pair_layout', case, window, power=power)
        # the classic layout in the same process
        tac._hip.PAIR_LAYOUT = False
        tac.invalidate()
        try:
            classic, croute = one_launch(tac, lin_chain, xd)
        finally:
            tac._hip.PAIR_LAYOUT = True
            tac.invalidate()
        assert croute.startswith('melspec_stream3_kernel<1024, 16, ') and croute.endswith(', 12>'), croute
        diff, bound = np.abs(lin.astype(np.float64) - classic), ORDER_REL * np.abs(classic.astype(np.float64))
        worst = float((diff[diff > 0] / np.maximum(bound[diff > 0], 1e-300)).max()) if diff.max() > 0 else 0.0
        print('pair_layout %r: max |pair - classic| / (2 . 64 . 2^-24 |classic|) = %.3g' % (case, worst))
        assert (diff <= bound).all(), (case, worst)


def test_bank_at_the_edge_of_a_shape_takes_the_classic_layout(tac):
    """HTK bank for 88.2 kHz audio: its widest band (17 quads) fits the (3, 7, 5) pair shape but its classic table is (4, 20), which only
    the general kernel runs — the pair packer declines it and the fused call runs the classic layout, as before the pair layout existed."""
    x = torch.from_numpy(signals.gained_with_silence((3, 1, 30000), 620, 2048, 512)).cuda()
    chain = torch.nn.Sequential(*tac.Melspectrogram(num_mels=128, sample_rate=88200, fft_length=2048, hop_length=512, htk=True)).cuda()
    assert tac._hip._melbank_pack(chain[2].filterbank, tac._hip.PACK_PAIRS_2048) is None
    got, route = one_launch(tac, chain, x)
    assert route == 'melspec_stream3_kernel<1024, 16, true, 0, 0, 12>', route
    fbnd.check_frames(got, fbnd.ref64(x.cpu().numpy(), 2048, 512, chain[0].window, 2.0, chain[2].filterbank), 'spec', 1e-5, 'pair_layout',
                      'htk 88.2 kHz', 2048, True)
