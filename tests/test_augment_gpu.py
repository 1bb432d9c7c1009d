"""-m gpu: ``add_noise`` / ``AddNoise`` on the gfx950 kernels (csrc/add_noise.hip) and ``speed`` / ``Speed`` / ``SpeedPerturbation`` on the
resample kernel — strict mode and poisoned outputs on, as in tests/test_specaug_gpu.py.

Reference and bound: tests/augment_rules.py — the float64 definition and, for every finite element,
``|got - want| <= u |want| + 2 u |scale64 noise_t| + 2^-149`` with ``u = 2^-24``: one rounding of ``scale`` to float32 and one of the
result, the factor 2 letting a multiply-then-add form pass as well as the fused one (derived, not measured; the float64 sums add
terms of order ``L 2^-53``).  The gradients are held to the same form of bound around the float64 formulas.  Every test prints its
worst ratio to the bound.  Shapes: the smallest that reach each path — L = 1 .. 5 (less than one 16-byte chunk, exactly one, one and a
sample), ``T - 1 / T / T + 1`` around one tile of ``T = ADD_NOISE_TILE`` samples and ``2 T + 5`` (three tiles); rows 1 and 3; lengths 0,
1, T, T + 1 (the mask edge inside the second tile), L, L + 7 and -1 mixed within a batch; ratios -5, 0, 10, 40 dB, shared and per row.
A reference is computed once per (length, lengths, ratios) and shared by the layouts.

Launch counts: a forward call is ONE ``tac_add_noise_f32`` entry (three launches on the stream behind it), a backward pass ONE
``tac_add_noise_grad_f32`` entry, whichever of the three gradients are asked for."""
import warnings

import numpy as np
import pytest
import torch

import augment_rules as R

pytestmark = pytest.mark.gpu

ENTRY, GRAD_ENTRY, RESAMPLE_ENTRY = 'tac_add_noise_f32', 'tac_add_noise_grad_f32', 'tac_polyphase_f32'
T = R.TILE


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    t._native.lib()
    t.set_strict(True)
    t._hip.set_poison_outputs(True)
    assert t._hip.ADD_NOISE_TILE == T == int(t._native.lib().tac_add_noise_tile())
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
    """rows ``pad`` floats apart, NaN between them: with pad = 3 the row stride is no multiple of four (dwords), with 4 it is"""
    store = torch.full(tuple(x.shape[:-1]) + (x.shape[-1] + pad,), float('nan'), device='cuda')
    store[..., :x.shape[-1]] = dev(x)
    return store[..., :x.shape[-1]]


def misaligned(x):
    """dense, but starting one float into its allocation: 4-byte aligned only"""
    store = torch.full((x.numel() + 1,), float('nan'), device='cuda')
    store[1:] = dev(x).reshape(-1)
    return store[1:].view(x.shape)


def every_second_sample(x):
    store = torch.full(tuple(x.shape[:-1]) + (2 * x.shape[-1],), float('nan'), device='cuda')
    store[..., ::2] = dev(x)
    return store[..., ::2]


LAYOUTS = (('dense', dev), ('padded by 3', lambda x: padded(x, 3)), ('padded by 4', lambda x: padded(x, 4)),
           ('misaligned', misaligned), ('time stride 2', every_second_sample))
LENGTHS = (1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T + 5)


def run(tac_, w, n, snr, lengths, what):
    """one call: exactly one entry, a fresh dense float32 tensor, the same bits when called again"""
    before = dict(tac_._hip.launches)
    got = tac_.add_noise(w, n, snr, lengths)
    assert launched_since(tac_, before) == {ENTRY: 1}, what
    lead = torch.broadcast_shapes(w.shape[:-1], n.shape[:-1], snr.shape)
    assert type(got) is torch.Tensor and got.dtype == torch.float32 and got.is_contiguous(), what
    assert tuple(got.shape) == tuple(lead) + (w.shape[-1],) and got.data_ptr() not in (w.data_ptr(), n.data_ptr()), what
    again = tac_.AddNoise()(w, n, snr, lengths)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), what + ': two calls differ'
    return got


def length_tables(rows, length):
    """[(name, lengths or None)]: none, three mixed tables (int64, int32, int64) and one length shared by every row"""
    return [('no lengths', None)] + \
           [('lengths %r' % (t.tolist(),), t) for t in (R.lengths_for(rows, length, 0), R.lengths_for(rows, length, 3, torch.int32),
                                                        R.lengths_for(rows, length, 6))] + \
           [('one shared length', torch.tensor([max(length - 2, 1)], dtype=torch.int32))]


def ratios(rows, which):
    return torch.tensor([R.SNRS[(which + i) % 4] for i in range(rows)]) if which < 4 else torch.tensor([R.SNRS[which % 4]])


# ----------------------------------------------------------------------------- 1. the kernels, element by element
@pytest.mark.parametrize('length', LENGTHS)
def test_kernel_within_the_bound(tac, length):
    w_all, n_all = R.normal((3, length), seed=length), R.normal((3, length), seed=length + 1)
    worst, which = 0.0, 0
    for rows in (1, 3):
        w, n = w_all[:rows], n_all[:rows]
        for name, lengths in length_tables(rows, length):
            snr = ratios(rows, which % 8)                   # per row (0 .. 3) and shared (4 .. 7) in turn
            which += 1
            t = R.terms(w, n, snr, lengths)
            bound = R.forward_bound(t)
            lengths_d = None if lengths is None else dev(lengths)
            for tag, build in LAYOUTS:
                what = '%d rows of %d, %s, snr %r, %s' % (rows, length, name, snr.tolist(), tag)
                wt, nt = build(w), build(n)
                assert torch.equal(wt.cpu(), w) and torch.equal(nt.cpu(), n), what
                got = run(tac, wt, nt, dev(snr), lengths_d, what)
                worst = max(worst, R.worst_ratio(got, t['out'], bound))
                assert worst <= 1.0, (what, worst)
            # one noise row for every row (row stride 0), against dense and padded waveforms
            shared = n[:1].expand(rows, length)
            ts = R.terms(w, shared, snr, lengths)
            for tag, build in LAYOUTS[:2]:
                got = run(tac, build(w), build(n[:1]).expand(rows, length), dev(snr), lengths_d, 'expanded noise, ' + tag)
                worst = max(worst, R.worst_ratio(got, ts['out'], R.forward_bound(ts)))
                assert worst <= 1.0, (name, tag, worst)
    print('L = %d: worst |got - want| / bound = %.3f' % (length, worst))


@pytest.mark.parametrize('length', (5, T + 1))
def test_batches_and_broadcast_tables(tac, length):
    """a (2, 3, L) batch: dense, with a ratio and a length per row, per batch entry (``(2, 1)``) and shared (``(1, 1)``); one noise
    row for all six and one per batch entry (``(2, 1, L)``: the outer stride walks the batch, the row stride is 0)"""
    w, n = R.normal((2, 3, length), seed=40), R.normal((2, 3, length), seed=41)
    worst = 0.0
    for snr, lengths in ((torch.tensor([[-5.0, 0.0, 10.0], [40.0, 10.0, 0.0]]), R.lengths_for(6, length, 1).view(2, 3)),
                         (torch.tensor([[10.0], [-5.0]]), torch.tensor([[length], [3]], dtype=torch.int32)),
                         (torch.tensor([[40.0]]), None), (torch.tensor([[0.0]]), torch.tensor([[T]]))):
        for noise in (n, n[:1, :1], n[:, :1]):              # a row each, one for all six, one per batch entry for its channels
            t = R.terms(w, noise, snr, lengths)
            what = 'snr %r lengths %r noise %r' % (tuple(snr.shape), None if lengths is None else tuple(lengths.shape), tuple(noise.shape))
            got = run(tac, dev(w), dev(noise), dev(snr), None if lengths is None else dev(lengths), what)
            worst = max(worst, R.worst_ratio(got, t['out'], R.forward_bound(t)))
            assert worst <= 1.0, (what, worst)
    print('(2, 3, %d): worst ratio %.3f' % (length, worst))


@pytest.mark.parametrize('dtype', (torch.float16, torch.bfloat16))
def test_half_inputs_are_widened(tac, dtype):
    w, n = dev(R.normal((3, 70), seed=50)).to(dtype), dev(R.normal((3, 70), seed=51)).to(dtype)
    snr, lengths = dev(torch.tensor([10.0, 0.0, -5.0])).to(dtype), dev(torch.tensor([70, 9, 33]))
    before = dict(tac._hip.launches)
    got = tac.add_noise(w, n, snr, lengths)
    assert launched_since(tac, before) == {ENTRY: 1} and got.dtype == dtype
    t = R.terms(w.float(), n.float(), snr.float(), lengths)
    step = 2.0 ** (-11 if dtype == torch.float16 else -8)              # the result is rounded to the narrow format once more
    err = (got.double().cpu() - t['out']).abs()
    assert bool((err <= R.forward_bound(t) + step * t['out'].abs()).all())


# ----------------------------------------------------------------------------- 2. NaNs and special rows
@pytest.mark.parametrize('name,build', LAYOUTS[:2])
def test_a_nan_behind_the_length_stays_where_it_is(tac, name, build):
    length = 2 * T + 5
    w, n = R.normal((3, length), seed=60), R.normal((3, length), seed=61)
    lengths, snr = torch.tensor([T + 1, length - 1, 5]), torch.tensor([10.0, 0.0, -5.0])
    clean = run(tac, build(w), build(n), dev(snr), dev(lengths), name)
    w2, n2 = w.clone(), n.clone()
    w2[0, T + 1], n2[0, T + 2], w2[0, length - 1] = float('nan'), float('nan'), float('inf')       # right behind the edge, and the end
    n2[1, length - 1], w2[2, 5], n2[2, T] = float('nan'), float('nan'), float('nan')
    got = run(tac, build(w2), build(n2), dev(snr), dev(lengths), name + ', NaNs behind the lengths')
    hit = torch.zeros((3, length), dtype=torch.bool)
    for r, i in ((0, T + 1), (0, T + 2), (0, length - 1), (1, length - 1), (2, 5), (2, T)):
        hit[r, i] = True
    got, clean = got.cpu(), clean.cpu()
    assert bool((~torch.isfinite(got[hit])).all())
    assert torch.equal(got[~hit].view(torch.int32), clean[~hit].view(torch.int32))                  # every other sample: the same bits
    # a NaN inside the mask makes exactly that row NaN
    for operand in (0, 1):
        w3, n3 = w.clone(), n.clone()
        (w3, n3)[operand][1, T - 1] = float('nan')
        got = run(tac, build(w3), build(n3), dev(snr), dev(lengths), name + ', a NaN inside the mask').cpu()
        assert bool(torch.isnan(got[1]).all())
        assert torch.equal(got[[0, 2]].view(torch.int32), clean[[0, 2]].view(torch.int32))


def test_special_rows(tac):
    """``E_s = 0``: scale 0; ``E_n = 0``: inf (NaN where the noise is 0, an infinity behind the length where it is not); both: NaN"""
    for length in (5, T + 6):
        w, n = R.normal((4, length), seed=70), R.normal((4, length), seed=71)
        lengths = torch.tensor([length, length - 2, length, 0])
        w[0] = 0.0
        n[1, :length - 2] = 0.0
        w[2], n[2] = 0.0, 0.0
        snr = torch.tensor([0.0, 10.0, -5.0, 40.0])
        t = R.terms(w, n, snr, lengths)
        assert float(t['scale'][0]) == 0.0 and bool(torch.isinf(t['scale'][1])) and bool(torch.isnan(t['scale'][2:]).all())
        for tag, build in LAYOUTS[:2]:
            got = run(tac, build(w), build(n), dev(snr), dev(lengths), 'special rows, ' + tag)
            assert R.worst_ratio(got, t['out'], R.forward_bound(t)) <= 1.0
            got = got.cpu()
            assert torch.equal(got[0], w[0]) and bool(torch.isnan(got[1, :length - 2]).all()) and bool(torch.isinf(got[1, length - 2:]).all())
            assert bool(torch.isnan(got[2:]).all())


# ----------------------------------------------------------------------------- 3. gradients
@pytest.mark.parametrize('length', (5, T + 1, 2 * T + 5))
def test_gradients_are_the_same_kernels(tac, length):
    w0, n0, g0 = R.normal((3, length), seed=80), R.normal((3, length), seed=81), R.normal((3, length), seed=82)
    worst = dict(g_wave=0.0, g_noise=0.0, g_snr=0.0)
    composite_before = dict(tac._ops.composite_calls)
    cases = [(tag, build, lengths, noise_rows, snr) for tag, build in LAYOUTS[:2]
             for lengths in (None, torch.tensor([min(T + 1, length), 1, length + 7]), torch.tensor([max(length - 1, 1)], dtype=torch.int32))
             for noise_rows, snr in ((3, torch.tensor([10.0, -5.0, 40.0])), (1, torch.tensor([0.0])))]
    for tag, build, lengths, noise_rows, snr in cases:
        what = 'L %d, %s, lengths %r, %d noise row(s)' % (length, tag, None if lengths is None else lengths.tolist(), noise_rows)
        w = build(w0).requires_grad_(True)
        n = build(n0[:noise_rows]).requires_grad_(True)             # one row: broadcast over the three, its gradient summed
        s = dev(snr).requires_grad_(True)
        g = build(g0)                                               # grad_out in the same layout
        before = dict(tac._hip.launches)
        out = tac.add_noise(w, n, s, None if lengths is None else dev(lengths))
        got = torch.autograd.grad(out, (w, n, s), g)
        assert launched_since(tac, before) == {ENTRY: 1, GRAD_ENTRY: 1}, what
        r = R.gradients(g0, w0, n0[:noise_rows], snr, lengths)
        want, bound = R.gradient_bounds(r, (w0.shape, n0[:noise_rows].shape, snr.shape))
        for key, have in zip(('g_wave', 'g_noise', 'g_snr'), got):
            assert have.dtype == torch.float32 and tuple(have.shape) == tuple(want[key].shape), (what, key)
            worst[key] = max(worst[key], R.worst_ratio(have, want[key], bound[key]))
            assert worst[key] <= 1.0, (what, key, worst[key])
        # one gradient alone: the same entry, once
        before = dict(tac._hip.launches)
        (only,) = torch.autograd.grad(tac.add_noise(w, n.detach(), s.detach(), None if lengths is None else dev(lengths)), (w,), g)
        assert launched_since(tac, before) == {ENTRY: 1, GRAD_ENTRY: 1}
        assert torch.equal(only.view(torch.int32), got[0].view(torch.int32)), what
    assert tac._ops.composite_calls == composite_before             # no stock-torch route, forward or backward
    print('L = %d: worst gradient ratios %s' % (length, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('length', (5, T + 1))
def test_a_noise_row_per_batch_entry(tac, length):
    """noise ``(B, 1, L)`` against a waveform ``(B, C, L)`` — dense and with padded channels — on the kernels where it lies, forward and
    backward; the noise gradient is folded over the channels"""
    w0, n0, g0 = R.normal((2, 3, length), seed=130), R.normal((2, 1, length), seed=131), R.normal((2, 3, length), seed=132)
    snr0, lengths = torch.tensor([[10.0], [-5.0]]), torch.tensor([[length], [max(length - 2, 1)]])
    r = R.gradients(g0, w0, n0, snr0, lengths)
    want, bound = R.gradient_bounds(r, (w0.shape, n0.shape, snr0.shape))
    t = R.terms(w0, n0, snr0, lengths)
    worst = 0.0
    for tag, build in (('dense', dev), ('padded channels', lambda x: dev(torch.cat([x, x[:, :1]], 1))[:, :x.shape[1]])):
        w, n, s = build(w0).requires_grad_(True), dev(n0).requires_grad_(True), dev(snr0).requires_grad_(True)
        before = dict(tac._hip.launches)
        out = tac.add_noise(w, n, s, dev(lengths))
        got = torch.autograd.grad(out, (w, n, s), dev(g0))
        assert launched_since(tac, before) == {ENTRY: 1, GRAD_ENTRY: 1}, tag
        worst = max(worst, R.worst_ratio(out, t['out'], R.forward_bound(t)))
        for key, have in zip(('g_wave', 'g_noise', 'g_snr'), got):
            assert tuple(have.shape) == tuple(want[key].shape), (tag, key)
            worst = max(worst, R.worst_ratio(have, want[key], bound[key]))
        assert worst <= 1.0, (tag, worst)
    print('(2, 3, %d) with noise (2, 1, %d): worst ratio %.3f' % (length, length, worst))


def test_reverb_noise_fbank_chain(tac):
    """``FFTConvolve -> AddNoise -> KaldiFbank`` on (4, 16000): one entry each forward, under strict.  ``kaldi_fbank`` has no gradient
    kernel (its backward is an announced route, as tests/test_specaug_gpu.py has it), so the gradient at its input is taken with
    backward strictness off; from there on AddNoise and FFTConvolve train under strict, and AddNoise's gradients are held to the bound."""
    rng = np.random.default_rng(90)
    wave = dev(rng.standard_normal((4, 16000)).astype(np.float32)).requires_grad_(True)
    rir = dev((rng.standard_normal((1, 800)) * np.exp(-np.arange(800) / 100.0)).astype(np.float32))
    noise = dev(rng.standard_normal((4, 16799)).astype(np.float32)).requires_grad_(True)
    snr = dev(torch.tensor([10.0, 0.0, 20.0, 5.0])).requires_grad_(True)
    lengths = dev(torch.tensor([16799, 12000, 16000, 8000]))
    conv, add, fbank = tac.FFTConvolve('full'), tac.AddNoise(), tac.KaldiFbank(num_mel_bins=80)
    before = dict(tac._hip.launches)
    reverbed = conv(wave, rir)
    mixed = add(reverbed, noise, snr, lengths)
    leaf = mixed.detach().requires_grad_(True)
    feats = fbank(leaf)
    since = launched_since(tac, before)
    # (the room response's spectra are a table made on its first use: an entry of their own beside the convolution's)
    assert since == {'tac_fftconvolve_spectra_f32': 1, 'tac_fftconvolve_f32': 1, ENTRY: 1, 'tac_kaldi_fbank_f32': 1}, since
    assert tuple(feats.shape) == (4, 103, 80) and bool(torch.isfinite(feats).all())
    tac.set_strict(True, backward=False)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', tac.CompositeRouteWarning)
            (g_mixed,) = torch.autograd.grad(feats.square().mean(), leaf)
    finally:
        tac.set_strict(True)
    before = dict(tac._hip.launches)
    g_wave, g_noise, g_snr = torch.autograd.grad(mixed, (wave, noise, snr), g_mixed)
    since = launched_since(tac, before)
    assert since.pop(GRAD_ENTRY) == 1 and since and all(k.startswith('tac_fftconvolve') for k in since), since
    assert bool(torch.isfinite(g_wave).all()) and bool(g_wave.any())
    r = R.gradients(g_mixed, reverbed, noise, snr, lengths)
    want, bound = R.gradient_bounds(r)
    ratios_ = [R.worst_ratio(have, want[key], bound[key]) for key, have in (('g_noise', g_noise), ('g_snr', g_snr))]
    print('chain: worst gradient ratios %.3f (noise), %.3f (snr)' % tuple(ratios_))
    assert max(ratios_) <= 1.0


def test_nothing_waits_for_the_host(tac):
    """``snr`` and ``lengths`` are read on the device: a warmed-up forward and backward pass makes no synchronising call"""
    w, n = dev(R.normal((3, T + 1), seed=95)).requires_grad_(True), dev(R.normal((3, T + 1), seed=96)).requires_grad_(True)
    snr, lengths, g = dev(torch.tensor([10.0, 0.0, -5.0])).requires_grad_(True), dev(torch.tensor([T + 1, 7, T])), dev(R.normal((3, T + 1), seed=97))
    x, speed_lengths = dev(R.normal((2, 1601), seed=98)), dev(torch.tensor([1601, 901], dtype=torch.int32))
    layer = tac.Speed(16000, 0.9)
    torch.autograd.grad(tac.add_noise(w, n, snr, lengths), (w, n, snr), g)
    layer(x, speed_lengths)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        torch.autograd.grad(tac.add_noise(w, n, snr, lengths), (w, n, snr), g)
        out, out_lengths = layer(x, speed_lengths)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert out_lengths.is_cuda and out_lengths.dtype == torch.int32 and out_lengths.tolist() == [1779, 1002]


# ----------------------------------------------------------------------------- 4. speed
FACTORS = ((0.9, 9, 10), (1.1, 11, 10), (0.95, 19, 20), (1.05, 21, 20))


def test_speed_is_one_resample_launch(tac):
    x = dev(R.normal((2, 3, 1601), seed=100))
    for dtype in (torch.int32, torch.int64, torch.float32):
        lengths = dev(torch.tensor([[1601, 800, 1], [7, 1600, 34]]).to(dtype))
        for factor, source, target in FACTORS:
            want = tac.resample(x, source, target)
            want_lengths = torch.ceil(lengths.cpu() * target / source).to(dtype)
            for fn in (lambda: tac.speed(x, 16000, factor, lengths), lambda: tac.Speed(16000, factor)(x, lengths)):
                before = dict(tac._hip.launches)
                out, out_lengths = fn()
                assert launched_since(tac, before) == {RESAMPLE_ENTRY: 1}, factor
                assert torch.equal(out.view(torch.int32), want.view(torch.int32)), factor
                assert out_lengths.is_cuda and out_lengths.dtype == dtype and torch.equal(out_lengths.cpu(), want_lengths), factor
    before = dict(tac._hip.launches)
    out, out_lengths = tac.speed(x, 16000, 1.0, lengths)
    assert out is x and torch.equal(out_lengths, lengths) and tac.Speed(16000, 1.0)(x)[0] is x
    assert launched_since(tac, before) == {}                            # factor 1.0: the input itself, nothing launched


def test_speed_perturbation_draws_and_launches(tac):
    x = dev(R.normal((2, 1600), seed=101))
    factors = [0.9, 1.0, 1.1]
    layer = tac.SpeedPerturbation(16000, factors).cuda()
    lengths = dev(torch.tensor([1600, 805]))
    picked = set()
    for seed in range(8):
        torch.manual_seed(seed)
        index = int(torch.randint(3, ()))
        picked.add(index)
        torch.manual_seed(seed)
        before = dict(tac._hip.launches)
        out, out_lengths = layer(x, lengths)
        assert launched_since(tac, before) == ({} if index == 1 else {RESAMPLE_ENTRY: 1}), seed
        want, want_lengths = tac.speed(x, 16000, factors[index], lengths)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(out_lengths, want_lengths), seed
    assert picked == {0, 1, 2}


# ----------------------------------------------------------------------------- 5. announced routes
def test_other_routes_are_announced(tac):
    length = 70
    w, n, snr, lengths = R.normal((2, 3, length), seed=110), R.normal((2, 3, length), seed=111), torch.tensor([[10.0], [-5.0]]), torch.tensor([[70], [31]])
    wt, nt, st, lt = dev(w), dev(n), dev(snr), dev(lengths)
    w4, n4 = dev(R.normal((2, 4, 4, length), seed=112))[:, :3, :3], dev(R.normal((2, 3, 3, length), seed=113))
    cases = (('dtype float64', wt.double(), nt.double(), st.double(), lt),
             ('non-positive time strides', wt, nt[..., :1].expand(2, 3, length), st, lt),
             ('leading dimensions that do not collapse', w4, n4, st[..., None], lt[..., None]))          # three strides: two is what the kernels walk
    for reason, a, b, c, l in cases:
        with pytest.raises(RuntimeError, match='strict'):
            tac.add_noise(a, b, c, l)
    tac.set_strict(False)
    try:
        for reason, a, b, c, l in cases:
            (key,) = [k for k in tac._ops.composite_calls if k[0] == 'add_noise' and reason in k[1]]
            counted = tac._ops.composite_calls[key]
            tac._ops._warned.discard(key)
            before = dict(tac._hip.launches)
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter('always')
                got = tac.add_noise(a, b, c, l)
            assert launched_since(tac, before) == {}, reason
            assert any(issubclass(x.category, tac.CompositeRouteWarning) for x in seen), reason
            assert tac._ops.composite_calls[key] == counted + 1
            assert got.is_contiguous() and got.dtype == a.dtype and tuple(got.shape) == tuple(a.shape)
            t = R.terms(a, b, c, l.cpu())
            if a.dtype == torch.float64:
                assert float((got.cpu() - t['out']).abs().max()) <= 1e-12 * float(t['out'].abs().max()), reason
            else:
                # the definition in float32 operators: each sum of L squares is within L u of its value, so is their ratio's root;
                # the two logarithms, the power and the products add a handful of roundings (16 u covers them at these magnitudes)
                bound = R.U * t['out'].abs() + (length + 16) * R.U * (t['scale'].unsqueeze(-1) * t['n']).abs()
                assert R.worst_ratio(got, t['out'], bound) <= 1.0, reason
    finally:
        tac.set_strict(True)


# ----------------------------------------------------------------------------- 6. past the grid
@pytest.mark.parametrize('name,length,tiles', R.WRAP_FORMS)
def test_grid_wrap(tac, name, length, tiles):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus in R.CU_COUNTS:
        R.assert_wraps(cus)
    rows = R.wrap_rows(cus, tiles)
    units, grid = R.launch(cus, rows, length)
    assert units == rows * tiles > 2 * grid and ((units - 2 * grid) // tiles) % 2 == 1 and rows > grid
    base_w, base_n, base_g = (dev(R.normal((R.BASE_ROWS, length), seed=120 + i)) for i in range(3))
    base_snr = dev(torch.tensor([10.0, -5.0, 0.0, 40.0, 3.0]))
    base_len = dev(torch.tensor([length, 1, max(length - 1, 1), length + 7, 3]))

    def both(w, n, snr, lengths, g):
        w, n, snr = (t.clone().requires_grad_(True) for t in (w, n, snr))
        before = dict(tac._hip.launches)
        out = tac.add_noise(w, n, snr, lengths)
        grads = torch.autograd.grad(out, (w, n, snr), g)
        assert launched_since(tac, before) == {ENTRY: 1, GRAD_ENTRY: 1}, name
        return (out.detach(),) + grads

    small = both(base_w, base_n, base_snr, base_len, base_g)
    pick = torch.arange(rows, device='cuda') % R.BASE_ROWS
    big = both(base_w[pick], base_n[pick], base_snr[pick], base_len[pick], base_g[pick])
    for what, b, s in zip(('out', 'grad_wave', 'grad_noise', 'grad_snr'), big, small):
        assert bool(torch.isfinite(s).all()), what
        assert torch.equal(b.view(torch.int32), s[pick].view(torch.int32)), '%s: %s' % (name, what)
