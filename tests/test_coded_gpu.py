"""-m gpu: the frame loads the fuzz of tests/test_gpu_fuzz.py does not reach.

Coded inputs (tests/coded_rules.py: generator, layouts, float64 reference on the decoded waveform, rules): int16 PCM and mu-law codes
(uint8 / int64) read by the fused mel chain itself, over hops of either parity, short and odd windows, every pad mode and centring,
power 1 and 2, linear and dB output, storage offsets and padded rows — every case ONE launch of ``tac_melspec_sparse_coded_f32`` —
and a fixed list of the smallest shapes at which its fast and gather paths and the host rule between them
(``coded_pairs_aligned``) can go wrong.  ``TAC_FUZZ_CASES`` / ``TAC_FUZZ_SEED`` / ``TAC_FUZZ_REPORT`` as in tests/test_gpu_fuzz.py.
tests/test_coded_cpu.py runs the same cases through the CPU route.

Float32 layouts: rows that start 0 / 4 / 8 / 12 bytes off a 16-byte boundary and rows 0 - 3 floats apart from dense, through every
STFT kernel family and every fused mel kernel (``vec2_ok`` / ``vec4_ok`` of ``make_geometry`` reached through the pointer and the
row stride, not through hop and length)."""
import os

import pytest
import torch

import coded_rules as R
import frame_bounds as fbnd
from oracle import signals, torch_ref

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get('TAC_FUZZ_CASES', '32'))
SEED = int(os.environ.get('TAC_FUZZ_SEED', '0'))
LAYOUTS = [(offset, pad) for offset in range(4) for pad in range(4)]          # floats in front of row 0, floats between rows


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)       # every kernel output starts as a NaN pattern: a sample no kernel writes cannot pass by luck
    yield t
    t._hip.set_poison_outputs(False)
    t.set_strict(False)


@pytest.fixture(autouse=True)
def every_output_written(tac):
    """After each test: no launch left a position of what it fills holding the poison pattern (named per entry point)."""
    tac._hip.poison_report()
    yield
    left = tac._hip.poison_report()
    assert not left, 'kernel outputs left unwritten (poisoned elements per entry point): %r' % left


def coded_only(c):
    def route(ran):
        assert ran == {R.CODED_ENTRY: 1}, (R.tag(c), ran)
    return route


def converted_first(c):
    def route(ran):
        assert R.CODED_ENTRY not in ran and sum(ran.values()) > 1, (R.tag(c), ran)
    return route


def one_launch(c):
    def route(ran):
        assert R.CODED_ENTRY not in ran and sum(ran.values()) == 1, (R.tag(c), ran)
    return route


def two_launch_chain(c):
    def route(ran):
        banks = [k for k in ran if k.startswith('tac_apply_filterbank')]              # (dense or band-sparse; dB in it or behind it)
        assert ran.get('tac_spectrogram_f32') == 1 and len(banks) == 1 and ran[banks[0]] == 1, (R.tag(c), ran)
        assert set(ran) <= {'tac_spectrogram_f32', banks[0], 'tac_amplitude_to_db_f32'} and sum(ran.values()) <= 3, (R.tag(c), ran)
    return route


# ----------------------------------------------------------------------------- coded frame loads
def test_fuzz_coded_melspectrogram(tac):
    for case in range(CASES):
        c = R.draw(SEED, case)
        R.run(c, 'cuda', 'fuzz_coded_' + c.fmt, tac._hip.launches, coded_only(c))


@pytest.mark.parametrize('kind', sorted(R.EDGES))
def test_coded_edges(tac, kind):
    """``coded_rules.EDGES`` at the five sizes, the three formats, linear and dB.  Power 1 at 256 / 400 / 512 / 1024 is outside the
    coded kernels (|X|^2 only): converted first, same rules."""
    for c in R.edge_cases(kind):
        R.run(c, 'cuda', 'coded_edges_' + c.fmt, tac._hip.launches, coded_only(c) if R.coded_entry_covers(c) else converted_first(c))


@pytest.mark.parametrize('n,onesided', [(128, True), (4096, True), (512, False)])
def test_coded_sizes_without_a_coded_load(tac, n, onesided):
    """fft_length 128 and 4096 and two-sided rows have no coded frame load: the samples are converted by a kernel of their own, then
    the float32 chain runs — more than one launch, none of them the coded entry, the same float64 rules."""
    for fmt in R.FORMATS:
        for db in (False, True):
            for mels in (40, 80, 128):                             # (coded_rules' rule 5: decoded silence off the dB clamp)
                c = R.fixed(n, fmt, db=db, onesided=onesided, num_mels=min(mels, n // 4), case='no-coded-load')
                if not (db and R.silence_at_the_clamp(c, R.bank(n, c.num_mels, c.sample_rate, c.htk))):
                    break
            assert not R.coded_entry_covers(c)
            R.run(c, 'cuda', 'coded_converted_' + fmt, tac._hip.launches, converted_first(c))


# ----------------------------------------------------------------------------- float32 layouts
FAMILIES = [(256, 64), (400, 160), (512, 128), (1024, 256), (2048, 512), (2048, 256), (2048, 500), (4096, 1024), (8192, 2048),
            (960, 240), (1018, 300)]


def layout_rows(n, hop, seed):
    """three rows whose length is a multiple of four floats (so that offset and padding alone decide the alignment classes)"""
    length = 4 * ((3 * n + hop) // 4) + 8
    return signals.gained_with_silence((3, length), seed, n, hop)


def named(tac, n, call):
    """(result, the kernel ``tac_last_route()`` names for this call or None).  Not every launcher writes the name, and an unwritten
    name is the previous call's: a launch that does write one — of another family than ``n`` — goes first, and a call after which
    that name still stands named nothing."""
    other = (2048, 500) if n != 2048 else (960, 240)
    tac.stft(named.x[:, :3 * other[0]], other[0], hop_length=other[1])
    planted = tac._hip.last_route()
    assert planted.startswith('stft_stream3' if n != 2048 else 'stft_smooth'), planted
    out = call()
    route = tac._hip.last_route()
    return out, (None if route == planted else route)


@pytest.mark.parametrize('n,hop', FAMILIES)
def test_float32_layouts_every_kernel_family(tac, n, hop):
    """Complex rows (``stft``) and |X|^2 rows (``Spectrogram``) of 16 layouts per family against the float64 oracle, and bit for bit
    against the dense copy where ``tac_last_route()`` names the same kernel for both.  (2048, 512): the aligned dense layout takes
    the hop ring, every other one does not — the routing switch, both ways."""
    x = layout_rows(n, hop, 4400 + n)
    named.x = torch.from_numpy(layout_rows(2048, 500, 4399)).cuda()
    layer = tac.Spectrogram(n, hop, power=2.).cuda()
    z64 = fbnd.ref64(x, n, hop)                                    # (the window ``stft`` builds itself, on the device)
    p64 = torch_ref.complex_norm(fbnd.ref64(x, n, hop, layer[0].window), 2.0)
    tol = R.FRAME_DFT if n == 1018 else R.FRAME
    for offset, pad in LAYOUTS:
        view = R.laid_out(x, 'float32', offset, pad, None, 'cuda')
        assert view.data_ptr() % 16 == 4 * offset and view.stride() == (x.shape[1] + pad, 1)
        dense = view.contiguous()
        what = (n, hop, offset, pad)
        for kind, op, ref, bound in (('complex', lambda t: tac.stft(t, n, hop_length=hop), z64, tol), ('spec', layer, p64, R.FRAME_POW)):
            got, route = named(tac, n, lambda: op(view))
            got_dense, route_dense = named(tac, n, lambda: op(dense))
            fbnd.check_frames(got.cpu(), ref, kind, bound, 'layouts_' + kind, what, n, True)
            if route is not None and route == route_dense:
                assert torch.equal(got, got_dense), (what, kind, route)
            if (n, hop) == (2048, 512):
                assert route is not None and route.startswith('stft_ring3') == ((offset, pad) == (0, 0)), (what, kind, route)


@pytest.mark.parametrize('n', [256, 400, 512, 1024, 2048, 4096])
def test_float32_layouts_fused_mel(tac, n):
    """The fused mel kernels of every size on the same 16 layouts: banks of 40 / 80 / 128 bands (at most fft_length / 4), linear
    (per frame, FRAME_POW) and dB (``check_mel_db64``), one launch per call.  The one-launch chain of 4096 reads its frames sixteen
    bytes at a time and declines every other alignment (csrc/stft_n4096.hip ``launch_n4096_mel``;
    tests/test_gpu_parity.py::test_melspectrogram_4096_one_launch_geometries): there the dense aligned layout is one launch and every
    other one the spectrogram and the filterbank kernel (and the dB kernel where it does not ride along) — that switch, both ways."""
    hop = 160 if n == 400 else n // 4
    length = 4 * ((3 * n + hop) // 4) + 8
    for mels in sorted({min(m, n // 4) for m in (40, 80, 128)}):
        for offset, pad in LAYOUTS:
            for db in (False, True):
                c = R.fixed(n, 'float32', hop=hop, length=length, num_mels=mels, db=db, offset=offset, row_pad=pad,
                            case='layout', sig=4500 + n)
                R.run(c, 'cuda', 'layouts_fused_mel', tac._hip.launches,
                      one_launch(c) if n != 4096 or (offset, pad) == (0, 0) else two_launch_chain(c))
