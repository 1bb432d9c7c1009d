"""-m gpu: ``resample`` / ``Resample`` on the gfx950 kernel (csrc/resample.hip) — strict mode and poisoned outputs on, as in
tests/test_mfcc_gpu.py.

Reference and bound: tests/resample_rules.py — the float64 sum per output sample and, per element,
``(K_n + 2) * 2^-24 * sum |h64| |x|``; every element is checked.  The lengths are the smallest that reach each path of the
kernel: 1, 2, ``width``, ``orig - 1 / orig / orig + 1`` (less than one block of phases, exactly one, one and a sample), the input
span of one tile of the case's 1024, 512 or 256 outputs minus one / exactly / plus one (the last output of a tile, the first of the
next), and three tiles plus a remainder (every tile position of a row, the span's start at every alignment; at most 3 rows x 4 tiles = 12 units
on a grid of 12 workgroups, so no workgroup takes a second unit here: tests/test_grid_wrap_gpu.py does that).  Rows 1 and 3; dense
rows (16-byte loads), a padded row stride and a start one float into the allocation (float loads), a padded stride of four floats
(16-byte loads across rows), and a (2, 3, L) batch.  A reference is computed once per (filter, length) and shared by the layouts.

The cases come from tests/polyphase_rules.py, whose census (tests/test_polyphase_rules_cpu.py) holds them to every instantiation
``polyphase_kernel<P1, SKEW, VEC>`` at every tile that public arguments reach, for the forward and for the adjoint bank; each test
asserts the instantiation the restated launcher rule predicts before it launches, and prints it."""
import warnings

import numpy as np
import pytest
import torch

import polyphase_rules as PR
import resample_rules as R

pytestmark = pytest.mark.gpu

ENTRY = 'tac_polyphase_f32'
TILE = 1024                         # outputs per tile of the kernel for the short banks (_hip.RESAMPLE_TILE)
HANN, WIDE, KAISER = PR.HANN, PR.WIDE_FILTER, PR.KAISER
CASES = PR.LDS_CASES                # the first twelve take TILE outputs per tile (asserted below), the rest 512 and 256


def case_id(c):
    return '%d:%d%s' % (c[0], c[1], ''.join('-%s' % v for v in c[2].values()))


def product_kw(kw):
    names = dict(lpw='lowpass_filter_width', rolloff='rolloff', method='resampling_method', beta='beta')
    return {names[k]: v for k, v in kw.items()}


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    assert t._hip.RESAMPLE_TILE == TILE
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


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to('cuda')


def padded(x, pad):
    """rows ``pad`` floats apart: with pad = 3 the row stride is no multiple of four (float loads), with 4 it is"""
    store = torch.full(tuple(x.shape[:-1]) + (x.shape[-1] + pad,), float('nan'), device='cuda')
    store[..., :x.shape[-1]] = dev(x)
    return store[..., :x.shape[-1]]


def misaligned(x):
    """dense, but starting one float into its allocation: 4-byte aligned only"""
    store = torch.full((x.size + 1,), float('nan'), device='cuda')
    store[1:] = dev(x).reshape(-1)
    return store[1:].view(x.shape)


def variant_of(tac_, case, adjoint=False):
    """(tile, P1, SKEW, per_cu) the restated launcher rule gives the case's bank, which ``_hip.resample_tile`` must agree with"""
    key = tac_._resample.constants(case[0], case[1], **product_kw(case[2]))
    bank = (tac_._resample.adjoint_bank if adjoint else tac_._resample.bank)(*key)
    v = PR.lds_variant(bank, True)
    assert v is not None and tac_._hip.resample_tile(bank) == v[0] and tac_._hip.resample_covers(*key), case_id(case)
    return v[0], v[1], v[2], v[4]


def sixteen_byte_rows(x):
    """the launcher's VEC: a 16-byte aligned start and, with more than one row, a row stride that is a multiple of four"""
    rows = x.reshape(-1, x.shape[-1])
    return rows.data_ptr() % 16 == 0 and (rows.shape[0] == 1 or rows.stride(0) % 4 == 0)


LAYOUTS = (('dense', dev), ('padded by 3', lambda x: padded(x, 3)), ('padded by 4', lambda x: padded(x, 4)),
           ('misaligned', misaligned))


def lengths_of(orig, new, kw, tile):
    _, width, _ = R.filter_constants(orig, new, kw.get('lpw', 6), kw.get('rolloff', 0.99))
    span = tile * orig // new                   # the longest input whose output is one tile
    want = [1, 2, width, orig - 1, orig, orig + 1, span - 1, span, span + 1, 3 * tile * orig // new + orig // 2 + 5]
    return sorted(set(n for n in want if n >= 1))


def run_one(tac_, xt, orig, new, kw, what):
    before = dict(tac_._hip.launches)
    got = tac_.resample(xt, orig, new, **product_kw(kw))
    assert launched_since(tac_, before) == {ENTRY: 1}, what
    assert type(got) is torch.Tensor and got.dtype == torch.float32 and got.is_contiguous(), what
    assert tuple(got.shape) == tuple(xt.shape[:-1]) + (R.out_length(xt.shape[-1], orig, new),), what
    return got


# ----------------------------------------------------------------------------- the kernel, element by element
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_kernel_within_the_bound(tac, case):
    orig, new, kw = case
    tile, p1, skew, per_cu = variant_of(tac, case)
    assert (tile == TILE) == (case in CASES[:12]) and (tile, p1, skew) == PR.lds_variant(PR.case_geometry(case), True)[:3]
    worst, loads = 0.0, set()
    lengths = lengths_of(orig, new, kw, tile)
    for length in lengths:
        x = R.waveform((3, length), seed=1000 * orig + 10 * new + length)
        ref, bound = R.reference(x, orig, new, **kw)
        for tag, build in LAYOUTS:
            for rows in (1, 3):
                what = '%s, %d rows of %d, %s' % (case_id(case), rows, length, tag)
                xt = build(x[:rows])
                assert tuple(xt.shape) == (rows, length) and np.array_equal(xt.cpu().numpy(), x[:rows]), what
                loads.add(sixteen_byte_rows(xt))
                got = run_one(tac, xt, orig, new, kw, what)
                worst = max(worst, R.assert_close(got, ref[:rows], bound[:rows], what))
    for length in (lengths[-4], lengths[-1] // 3):
        x4 = R.waveform((2, 3, length), seed=77 * orig + new + length)
        what = '%s, (2, 3, %d)' % (case_id(case), length)
        ref, bound = R.reference(x4, orig, new, **kw)
        worst = max(worst, R.assert_close(run_one(tac, dev(x4), orig, new, kw, what), ref, bound, what))
        # leading dims no single row stride expresses (copied by the launcher), and a 1-D input
        swapped = dev(np.ascontiguousarray(np.swapaxes(x4, 0, 1))).transpose(0, 1)
        worst = max(worst, R.assert_close(run_one(tac, swapped, orig, new, kw, what + ' swapped'), ref, bound, what))
        worst = max(worst, R.assert_close(run_one(tac, dev(x4[1, 2]), orig, new, kw, what + ' 1-D'), ref[1, 2], bound[1, 2], what))
    assert loads == {False, True}, 'both load forms'
    print('resample %s: tile %d, P1 %d, SKEW %d, VEC 0 and 1, %d per CU, K %d: worst |err| / bound %.3f' % (
        case_id(case), tile, p1, skew, per_cu, PR.case_geometry(case).K, worst))


def test_exact_zeros_stay_exact(tac):
    x = R.waveform((3, 4000), seed=9)
    got = tac.resample(dev(x), 3, 2)
    # inputs 1000 .. 1499 are zero: outputs whose whole window lies inside are exactly zero (width = 10 at 3:2)
    assert not bool(got[:, 680:990].any())


def test_two_calls_agree_bit_for_bit(tac):
    for orig, new in ((3, 1), (441, 160), (160, 441), (2, 3), (12, 1), (25, 2), (16, 1), (50, 3)):
        tile = variant_of(tac, (orig, new, HANN))[0]
        assert tile == PR.pinned_tile(orig, new)
        xt = dev(R.waveform((3, 3 * tile * orig // new + 77), seed=orig))
        assert torch.equal(tac.resample(xt, orig, new), tac.resample(xt, orig, new))


@pytest.mark.parametrize('case', [(3, 1, HANN), (2, 3, HANN), (441, 160, HANN), (160, 441, HANN), (3, 2, KAISER),
                                  (12, 1, HANN), (25, 2, HANN), (17, 1, HANN), (50, 3, HANN)], ids=case_id)
def test_nan_reaches_the_outputs_the_rules_say(tac, case):
    orig, new, kw = case
    tile = variant_of(tac, case)[0]
    assert tile == PR.pinned_tile(orig, new)
    length = tile * orig // new + 2 * orig + 3
    for index in (0, length // 2, tile * orig // new - 1, length - 1):
        x = R.waveform((3, length), seed=5 + index)
        clean = x.copy()
        x[1, index] = np.nan
        clean[1, index] = 0.0
        got = tac.resample(dev(x), orig, new, **product_kw(kw))
        hit = torch.isnan(got).cpu().numpy()
        want = np.zeros_like(hit)
        want[1] = R.reached_by(index, length, orig, new, **kw)
        assert want[1].any()
        assert np.array_equal(hit, want), '%s, NaN at %d: %d NaN outputs, expected %d' % (
            case_id(case), index, int(hit.sum()), int(want.sum()))
        ref, bound = R.reference(clean, orig, new, **kw)
        got = torch.where(torch.from_numpy(want).to('cuda'), torch.from_numpy(ref.astype(np.float32)).to('cuda'), got)
        R.assert_close(got, ref, bound + 2.0 ** -24 * np.abs(ref) * want, 'the outputs next to a NaN, %s' % case_id(case))


# ----------------------------------------------------------------------------- gradient
@pytest.mark.parametrize('case', PR.LDS_GRADIENT_CASES, ids=case_id)
def test_gradient_is_the_kernel_with_the_adjoint_bank(tac, case):
    """the launch of the gradient makes ``length`` outputs with the adjoint bank: lengths on both sides of one of ITS tiles too.
    grad_out goes to the launcher where it lies: dense, rows 3 floats apart, rows a multiple of four floats apart (16-byte
    loads whatever ``n_out`` is) and dense one float into its allocation (float loads whatever it is) — both forms at each length"""
    orig, new, kw = case
    assert tac._ops.strict()
    tile, p1, skew, per_cu = variant_of(tac, case, adjoint=True)
    forward_tile = variant_of(tac, case)[0]
    assert (tile, p1, skew) == PR.lds_variant(PR.case_geometry(case, True), True)[:3]
    assert tile == PR.pinned_tile(orig, new, adjoint=True) and forward_tile == PR.pinned_tile(orig, new)
    for length in sorted({orig + 1, forward_tile * orig // new + orig + 3, tile - 3, tile + orig + 3}):
        n_out = R.out_length(length, orig, new)
        x = dev(R.waveform((3, length), seed=length)).requires_grad_(True)
        g = R.waveform((3, n_out), seed=length + 1)
        aref, abound = R.adjoint_reference(g, length, orig, new, **kw)
        loads = set()
        for tag, gt in (('dense', dev(g)), ('padded', padded(g, 3)), ('stride a multiple of four', padded(g, (-n_out) % 4 or 4)),
                        ('misaligned', misaligned(g))):
            assert gt.stride(-1) == 1 and tuple(gt.shape) == (3, n_out)
            loads.add(sixteen_byte_rows(gt))
            y = tac.resample(x, orig, new, **product_kw(kw))
            before = dict(tac._hip.launches)
            with warnings.catch_warnings():
                warnings.simplefilter('error', tac.CompositeRouteWarning)
                (gx,) = torch.autograd.grad(y, x, grad_outputs=gt)
            what = 'grad %s, length %d, grad_out %s' % (case_id(case), length, tag)
            assert launched_since(tac, before) == {ENTRY: 1}, what
            assert tuple(gx.shape) == (3, length) and gx.is_contiguous()
            ratio = R.assert_close(gx, aref, abound, what)
            (again,) = torch.autograd.grad(tac.resample(x, orig, new, **product_kw(kw)), x, grad_outputs=gt)
            assert torch.equal(gx, again)
        assert loads == {False, True}, 'both load forms, length %d' % length
        print('%s, VEC 0 and 1, adjoint tile %d, P1 %d, SKEW %d, %d per CU: worst |err| / bound %.3f' % (what, tile, p1, skew, per_cu, ratio))
    # double backward has no kernel: refused under strict
    y = tac.resample(x, orig, new)
    with pytest.raises(RuntimeError, match='strict mode'):
        torch.autograd.grad(y, x, grad_outputs=dev(g), create_graph=True)


# ----------------------------------------------------------------------------- the layers on a narrow tile
@pytest.mark.parametrize('orig_freq,new_freq', [(96000, 8000), (8000, 96000)])
def test_layers_on_the_narrow_tile(tac, orig_freq, new_freq):
    """12:1 runs the forward on 512 outputs per tile, 1:12 the gradient: a (2, 2, L) batch of three such tiles and a remainder,
    one launch each way, nothing announced, both results held to their references"""
    orig, new = R.reduced(orig_freq, new_freq)
    case = (orig, new, HANN)
    tiles = variant_of(tac, case)[0], variant_of(tac, case, adjoint=True)[0]
    assert tiles == (PR.pinned_tile(orig, new), PR.pinned_tile(orig, new, adjoint=True)) and set(tiles) == {512, TILE}
    length = 3 * 512 * orig + 17
    layer = tac.Resample(orig_freq, new_freq).cuda()
    x = R.waveform((2, 2, length), seed=orig_freq // 1000)
    xt = dev(x).requires_grad_(True)
    before = dict(tac._hip.launches)
    y = layer(xt)
    assert launched_since(tac, before) == {ENTRY: 1} and tuple(y.shape) == (2, 2, R.out_length(length, orig, new))
    y.retain_grad()
    before = dict(tac._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        y.square().mean().backward()
    assert launched_since(tac, before) == {ENTRY: 1}
    worst = R.assert_close(y, *R.reference(x, orig, new), 'Resample(%d, %d)' % (orig_freq, new_freq))
    # the gradient against the adjoint of the grad_out the kernel was handed (2 y / N, as the device rounded it)
    aref, abound = R.adjoint_reference(y.grad.cpu().numpy(), length, orig, new)
    assert bool(y.grad.any()) and tuple(xt.grad.shape) == (2, 2, length)
    worst_adj = R.assert_close(xt.grad, aref, abound, 'gradient of Resample(%d, %d)' % (orig_freq, new_freq))
    print('Resample(%d, %d), tiles %r: worst |err| / bound %.3f forward, %.3f gradient' % (orig_freq, new_freq, tiles, worst, worst_adj))


# ----------------------------------------------------------------------------- refusals
def test_routes_outside_the_kernel(tac):
    orig, new = 2000, 2001                      # 2001 phases of 14 taps: beyond RESAMPLE_MAX_BANK
    assert not tac._hip.resample_covers(*tac._resample.constants(orig, new))
    x = R.waveform((2, 300), seed=3)
    xt = dev(x)
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.resample(xt, orig, new)
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.resample(xt.double(), 3, 2)                                     # float64 on the device
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.resample(xt[:1].expand(3, 300), 3, 2)                           # a stride of zero
    # 60:1 is the integer decimation just beyond the last the kernel holds (48:1; 59:1 is refused for its span like 60:1)
    assert tac._hip.resample_covers(*tac._resample.constants(48, 1)) and not tac._hip.resample_covers(*tac._resample.constants(59, 1))
    assert not tac._hip.resample_covers(*tac._resample.constants(60, 1))
    with pytest.raises(RuntimeError, match='strict mode'):
        tac.resample(xt, 60, 1)
    assert launched_since(tac, before) == {}
    # equal rates and empty inputs launch nothing and are no route at all
    assert tac.resample(xt, 48000, 48000) is xt
    assert tuple(tac.resample(xt[:, :0], 3, 2).shape) == (2, 0)
    assert launched_since(tac, before) == {}
    tac.set_strict(False)
    try:
        # the composite is torch's conv1d over all 2 width + orig taps of a phase, zeros included: its own float32 bound counts
        # every one of them where the kernel's counts the K_n non-zero ones
        _, width, _ = R.filter_constants(orig, new, 6, 0.99)
        k_min = min(len(R.phase_taps(orig, new, p)[0]) for p in range(new))
        ref, bound = R.reference(x, orig, new)
        for xin, scale in ((xt, (2 * width + orig + 2) / (k_min + 2)), (xt.double(), 1e-8)):
            for key in [k for k in tac._ops._warned if k[0] == 'resample']:
                tac._ops._warned.discard(key)
            with pytest.warns(tac.CompositeRouteWarning):
                got = tac.resample(xin, orig, new)
            assert got.dtype == xin.dtype and launched_since(tac, before) == {}
            r64, b64 = R.reference(xin.cpu().numpy(), orig, new)
            R.assert_close(got, r64, b64 * scale + 1e-300, 'stock-torch route, %s' % xin.dtype)
    finally:
        tac.set_strict(True)


# ----------------------------------------------------------------------------- the chain
def test_resample_in_front_of_the_fused_mel_chain(tac):
    kw = dict(num_mels=80, sample_rate=16000, fft_length=400, hop_length=160)
    x = dev(R.waveform((2, 2, 48000), seed=13))
    rs = tac.Resample(48000, 16000).cuda()
    parent = torch.nn.Sequential(*tac.Melspectrogram(**kw), tac.AmplitudeToDb()).cuda()
    before = dict(tac._hip.launches)
    y = rs(x)
    assert launched_since(tac, before) == {ENTRY: 1} and tuple(y.shape) == (2, 2, 16000)
    before = dict(tac._hip.launches)
    db = parent(y)
    mel_launch = launched_since(tac, before)
    assert len(mel_launch) == 1 and list(mel_launch.values()) == [1], mel_launch
    chain = torch.nn.Sequential(rs, *parent)
    before = dict(tac._hip.launches)
    got = chain(x)
    assert launched_since(tac, before) == dict(mel_launch, **{ENTRY: 1})
    assert type(got) is torch.Tensor and tuple(got.shape) == (2, 2, 80, 101) and torch.equal(got, db)
    assert torch.equal(rs.bank.cpu(), tac._resample.bank(3, 1, 6, 0.99, 'sinc_interp_hann', None).taps.float())
    # and it trains: both gradients on kernels, nothing announced
    xg = x.clone().requires_grad_(True)
    before = dict(tac._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        chain(xg).square().mean().backward()
    assert launched_since(tac, before).get(ENTRY) == 2 and bool(torch.isfinite(xg.grad).all()) and bool(xg.grad.any())
