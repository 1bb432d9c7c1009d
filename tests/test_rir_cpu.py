"""not-gpu: ``simulate_rir_ism`` / ``simulate_rir_ism_batch`` / ``SimulateRirIsm`` on the CPU route (``_composite.rir_ism``: the definition in float64
torch operators, rounded once) against tests/rir_rules.py — the float64 restatement in numpy, the per-element ``BOUND`` and the case
table — and the host pieces the kernel route shares: the image table, the band filters, the checks and the fake kernels."""
import numpy as np
import pytest
import torch

import rir_rules as R


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def tensors(c):
    """room, source, mic_array of the case's batch, and its absorption as the functionals take it"""
    a = c.absorption if isinstance(c.absorption, float) else torch.from_numpy(c.absorption)
    return torch.from_numpy(c.rooms), torch.from_numpy(c.sources), torch.from_numpy(c.mics), a


def op_absorption(c):
    a = torch.from_numpy(c.bands())
    return a[None] if a.dim() == 2 else a


def per_room(c, fn, *args):
    return np.stack([fn(c.rooms[i], c.sources[i], c.mics[i], c.bands() if c.bands().ndim == 2 else c.bands()[i], c.max_order, c.L,
                        c.sample_rate, c.sound_speed, *args) for i in range(len(c.rooms))])


# ----------------------------------------------------------------------------- the rules themselves
def test_image_table(tac):
    assert [R.n_images(n, 3) for n in (1, 3, 6, 10)] == [7, 63, 377, 1561]
    for dims in (2, 3):
        for order in (0, 1, 2, 5, 10):
            table = tac._rir.images(order, dims)
            r = torch.arange(-order, order + 1)
            X = torch.cartesian_prod(*([r] * dims)).reshape(-1, dims)
            want = X[X.abs().sum(-1) <= order]
            assert table.dtype == torch.int8 and torch.equal(table.long(), want)
            assert np.array_equal(table.numpy(), R.images(order, dims)) and tac._rir.n_images(order, dims) == len(want)
    assert tac._rir.n_images(32, 3) == len(tac._rir.images(32, 3)) and tac._rir.images(3, 2) is tac._rir.images(3, 2)


def test_the_farthest_image_is_in_the_outer_shells(tac):
    """what the span launch relies on: it walks ``_rir.shell`` only, the images with ``sum |X_d| >= max_order - 1``"""
    for c in R.CASES:
        X = R.images(c.max_order, c.dims)
        outer = np.abs(X).sum(-1) >= c.max_order - 1
        assert np.array_equal(tac._rir.shell(c.max_order, c.dims).numpy(), X[outer])
        for i in range(len(c.rooms)):
            _, _, di = R.geometry(c.rooms[i], c.sources[i], c.mics[i], np.zeros((1, 2 * c.dims)), c.max_order, c.sample_rate, c.sound_speed)
            assert np.array_equal(di[outer].max(0), di.max(0))


@pytest.mark.parametrize('c', R.CASES, ids=lambda c: c.name)
def test_the_bound_is_achievable_and_refuses_the_direct_form(c):
    """the float32 model of the kernel's arithmetic stays inside the INNER bracket (half of BOUND); the direct float32 form is outside
    BOUND.  Measured over the table: the model reaches 0.17 – 0.46 of the bracket, the direct form 15 – 400 times BOUND."""
    P, n = c.L // 2, c.natural()
    want, bound = c.reference(P, n)
    model, _ = R.excess(per_room(c, R.model32, P, n), want, bound)
    direct, _ = R.excess(per_room(c, R.direct32, P, n), want, bound)
    print('%s: model32 %.3f of BOUND, direct32 %.1f' % (c.name, model, direct))
    assert model <= 0.5
    assert direct > 3.0


def test_dropped_edge_taps_are_detected_at_81_and_marginal_at_255():
    """what the bound sees: the two outermost taps dropped at L = 81 is far outside (42 times BOUND here); at L = 255 they are about as
    large as the bound itself (1.2 times here, 0.85 – 1.05 when the bound was set): below reliable detection, as rir_rules.py says"""
    for c, outside in ((R.CASES[3], True), (R.CASES[6], False)):
        P, n = c.L // 2, c.natural()
        want, bound = c.reference(P, n)
        room = 0
        amp, delay, di = R.geometry(c.rooms[room], c.sources[room], c.mics[room], c.bands(), c.max_order, c.sample_rate, c.sound_speed)
        cut = want[room].copy()
        for m in (-P, P - 1):                                        # (the tap at m = P is 0 whenever f > 0)
            w, _ = R.taps(m + (di - delay), P)
            pos = di + m + P - P
            for ch in range(amp.shape[2]):
                ok = (pos[:, ch] >= 0) & (pos[:, ch] < n)
                np.subtract.at(cut[0, ch], pos[ok, ch], (amp[0, :, ch] * w[:, ch])[ok])
        ratio, _ = R.excess(cut, want[room], bound[room])
        print('%s: outermost taps dropped: %.2f of BOUND' % (c.name, ratio))
        assert ratio > 10.0 if outside else ratio < 3.0


# ----------------------------------------------------------------------------- the composite route
@pytest.mark.parametrize('c', R.CASES, ids=lambda c: c.name)
def test_composite_within_the_bound(tac, c):
    P, n = c.L // 2, c.natural()
    room, source, mics, _ = tensors(c)
    span = torch.ops.tac_amd.rir_ism_span(room, source, mics, c.max_order, c.L, c.sound_speed, c.sample_rate)
    assert span.dtype == torch.int64 and span.dim() == 0 and int(span) == n
    for start, length in ((P, n), (0, n + P + 7)):
        want, bound = c.reference(start, length)
        got = torch.ops.tac_amd.rir_ism(room, source, mics, op_absorption(c), c.max_order, start, length, c.L, c.sound_speed, c.sample_rate)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        ratio, at = R.excess(got.numpy(), want, bound)
        assert ratio <= 1.0, (c.name, start, ratio, at)
        assert bool((got.numpy()[bound == 0] == 0).all())


def test_single_equals_batch_of_one_and_entries_are_independent(tac):
    for c in (R.CASES[2], R.CASES[3], R.CASES[5]):
        room, source, mics, a = tensors(c)
        kw = dict(center_frequency=torch.tensor(R.CENTRES)) if c is R.CASES[2] else {}
        one = tac.simulate_rir_ism(room[0], source[0], mics[0], c.max_order, a, sample_rate=c.sample_rate, delay_filter_length=c.L, **kw)
        batch = tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, sample_rate=c.sample_rate, delay_filter_length=c.L, **kw)
        assert tuple(batch.shape) == (1,) + tuple(one.shape) and torch.equal(batch[0].view(torch.int32), one.view(torch.int32))
    c = R.CASES[4]                                                       # two rooms, per-room absorption
    room, source, mics, a = tensors(c)
    n = 1500
    both = tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, n, c.L, sample_rate=c.sample_rate)
    assert tuple(both.shape) == (2, 4, n)
    for i in range(2):
        alone = tac.simulate_rir_ism(room[i], source[i], mics[i], c.max_order, a[i], n, c.L, sample_rate=c.sample_rate)
        assert torch.equal(both[i].view(torch.int32), alone.view(torch.int32))
    assert not torch.equal(both[0], both[1])


def test_output_length(tac):
    c = R.CASES[3]
    room, source, mics, a = tensors(c)
    n = c.natural()
    args = (room[0], source[0], mics[0], c.max_order, a)
    natural = tac.simulate_rir_ism(*args)
    assert tuple(natural.shape) == (4, n)
    assert torch.equal(tac.simulate_rir_ism(*args, output_length=n), natural)
    short = tac.simulate_rir_ism(*args, output_length=n - 613)
    assert torch.equal(short, natural[:, :n - 613])
    longer = tac.simulate_rir_ism(*args, output_length=n + 300)
    assert torch.equal(longer[:, :n], natural) and bool((longer[:, n:] == 0).all())
    assert float(natural.abs().max()) > 1.0
    # the batch form: None is the longest natural length of the batch
    c = R.CASES[4]
    room, source, mics, a = tensors(c)
    assert tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, None, c.L, sample_rate=c.sample_rate).shape[-1] == c.natural()


def test_order_zero_is_the_taps_in_place(tac):
    """one image, one microphone: the L - P samples from raw index P on are exactly the float64 taps amp w(m + f) rounded once"""
    room, source = torch.tensor([5.3, 4.1, 3.2]), torch.tensor([2.1, 1.7, 1.4])
    mic = torch.tensor([[3.9, 2.2, 1.0]])
    for L in (5, 81):
        P = L // 2
        out = tac.simulate_rir_ism(room, source, mic, 0, 0.3, delay_filter_length=L)
        dist = float(np.sqrt(((source.double().numpy() - mic[0].double().numpy()) ** 2).sum()))
        delay = dist * 16000.0 / 343.0
        di = int(np.ceil(delay))
        assert di > P and tuple(out.shape) == (1, di + L - P)
        w, _ = R.taps(np.arange(-P, P + 1) + (di - delay), P)
        want = np.zeros(di + L)
        want[di:di + L] = w / dist
        assert np.array_equal(out[0].numpy(), want[P:].astype(np.float32))
        assert bool((out[0, :di - P] == 0).all())


# ----------------------------------------------------------------------------- several bands
def test_band_filters_against_the_definition(tac):
    for centres, rate in ((R.CENTRES, 16000.0), ((125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0), 16000.0), ((1000.0, 3000.0), 8000.0)):
        want = R.band_filters(centres, rate)
        got64 = tac._rir.band_filters(centres, rate, 'cpu', torch.float64)
        assert tuple(got64.shape) == (len(centres), 511) and float(np.abs(got64.numpy() - want).max()) <= 1e-15
        got = tac._rir.band_filters(centres, rate)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), got64.numpy().astype(np.float32))
        assert np.allclose(want, want[:, ::-1], atol=1e-17)                     # linear phase
    edges = tac._rir.band_edges(R.CENTRES, 16000.0)
    assert edges == [(250.0, 500.0, 1000.0), (500.0, 1000.0, 2000.0), (1000.0, 2000.0, 8000.0)]


def test_multiband_is_the_hand_composition(tac):
    c = R.CASES[2]
    room, source, mics, a = tensors(c)
    centres = torch.tensor(R.CENTRES)
    P, n = c.L // 2, 700
    got = tac.simulate_rir_ism(room[0], source[0], mics[0], c.max_order, a, n, c.L, centres, c.sound_speed, c.sample_rate)
    raw = torch.ops.tac_amd.rir_ism(room, source, mics, a[None], c.max_order, 0, P + n + 255, c.L, c.sound_speed, c.sample_rate)
    filters = tac._rir.band_filters(R.CENTRES, c.sample_rate)[:, None, :]
    hand = torch.sum(tac.fftconvolve(raw[0], filters, mode='same'), dim=0)[..., P:P + n]
    assert tuple(got.shape) == (4, n) and torch.equal(got.view(torch.int32), hand.view(torch.int32))
    want = R.multiband(c.rooms[0], c.sources[0], c.mics[0], c.bands(), R.CENTRES, c.max_order, c.L, c.sample_rate, c.sound_speed, n)
    reach = float(np.abs(got.double().numpy() - want).max())
    print('multi-band CPU route: %.3g off the float64 restatement at a peak of %.3g' % (reach, np.abs(want).max()))
    # A float32 FFT convolution is off by at most about (a few log2 N + 2) u of sum_k |raw[t - k]| |h[k]|, taken at its largest over the
    # row since a transform spreads its error over the block: 64 u with N = 4096.  The raw rows themselves are within BOUND, which
    # the filters (gain at most 1 a band) pass on.  Reached here: 1.9e-7 at a peak of 2.78; tests/test_rir_gpu.py takes 4 times that.
    bands, bound = R.raw(c.rooms[0], c.sources[0], c.mics[0], c.bands(), c.max_order, c.L, c.sample_rate, c.sound_speed, 0, P + n + 255)
    filt = np.abs(R.band_filters(R.CENTRES, c.sample_rate))
    mass = sum(np.stack([np.convolve(np.abs(bands[b, ch]), filt[b]) for ch in range(4)]) for b in range(3))
    passed = sum(np.stack([np.convolve(bound[b, ch], filt[b]) for ch in range(4)]) for b in range(3))
    assert reach <= 64 * R.U * float(mass.max()) + float(passed.max())
    # the natural length
    full = tac.simulate_rir_ism(room[0], source[0], mics[0], c.max_order, a, None, c.L, centres, c.sound_speed, c.sample_rate)
    assert full.shape[-1] == c.natural()
    assert float(np.abs(full[:, :n].double().numpy() - want).max()) <= 64 * R.U * float(mass.max()) + float(passed.max())


# ----------------------------------------------------------------------------- arguments
def test_value_errors(tac):
    room, source, mics = torch.tensor([5.0, 4.0, 3.0]), torch.tensor([1.0, 2.0, 1.5]), torch.tensor([[2.0, 2.0, 1.0], [2.1, 2.0, 1.0]])
    f = tac.simulate_rir_ism
    assert tuple(f(room, source, mics, 1, 0.2, 100).shape) == (2, 100)
    for bad_room in (torch.ones(4), torch.ones(1), torch.ones(1, 3), torch.tensor(3.0)):
        with pytest.raises(ValueError, match='room'):
            f(bad_room, source, mics, 1, 0.2, 100)
    for bad_source in (torch.ones(2), torch.ones(1, 3)):
        with pytest.raises(ValueError, match='source'):
            f(room, bad_source, mics, 1, 0.2, 100)
    for bad_mics in (torch.ones(3), torch.ones(2, 2), torch.ones(1, 2, 3)):
        with pytest.raises(ValueError, match='mic_array'):
            f(room, source, bad_mics, 1, 0.2, 100)
    with pytest.raises(ValueError, match='delay_filter_length'):
        f(room, source, mics, 1, 0.2, 100, delay_filter_length=80)
    bands = torch.full((3, 6), 0.2)
    with pytest.raises(ValueError, match='center_frequency'):
        f(room, source, mics, 1, bands, 100)
    with pytest.raises(ValueError, match='center_frequency'):
        f(room, source, mics, 1, bands, 100, center_frequency=torch.tensor([500.0, 1000.0]))
    with pytest.raises(ValueError, match='absorption'):
        f(room, source, mics, 1, torch.full((4,), 0.2), 100)
    with pytest.raises(ValueError, match='absorption'):
        f(room, source, mics, 1, torch.full((1, 1, 6), 0.2), 100)            # (three dimensions: the batch form only)
    with pytest.raises(ValueError, match='output_length'):
        f(room, source, mics, 1, 0.2, 0)
    g = tac.simulate_rir_ism_batch
    assert tuple(g(room[None], source[None], mics[None], 1, torch.full((1, 1, 6), 0.2), 100).shape) == (1, 2, 100)
    with pytest.raises(ValueError, match='room'):
        g(room, source, mics, 1, 0.2, 100)
    with pytest.raises(ValueError, match='mic_array'):
        g(room[None], source[None], mics[None].expand(2, -1, -1), 1, 0.2, 100)
    with pytest.raises(ValueError, match='absorption'):
        g(room[None], source[None], mics[None], 1, torch.full((2, 1, 6), 0.2), 100)
    # 2-D rooms, and a wall order that matters: x_lo and x_hi are not interchangeable
    r2, s2, m2 = torch.tensor([6.0, 4.0]), torch.tensor([1.0, 2.0]), torch.tensor([[4.5, 1.0]])
    a = f(r2, s2, m2, 2, torch.tensor([0.1, 0.6, 0.3, 0.3]), 600)
    b = f(r2, s2, m2, 2, torch.tensor([0.6, 0.1, 0.3, 0.3]), 600)
    assert tuple(a.shape) == (1, 600) and not torch.equal(a, b)


def test_a_microphone_on_an_image_spoils_its_row_only(tac):
    c = R.CASES[5]
    room, source, mics, a = tensors(c)
    mics = mics.clone()
    clean = tac.simulate_rir_ism(room[0], source[0], mics[0], 2, a, 900)
    mics[0, 1] = source[0]
    got = tac.simulate_rir_ism(room[0], source[0], mics[0], 2, a, 900)
    assert not bool(torch.isfinite(got[1]).all()) and bool(torch.isinf(got[1]).any())
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


def test_gradient_reaches_the_geometry(tac):
    room = torch.tensor([5.3, 4.1, 3.2], dtype=torch.float64)
    source = torch.tensor([2.1, 1.7, 1.4], dtype=torch.float64, requires_grad=True)
    mics = torch.tensor([[3.3, 2.9, 1.1]], dtype=torch.float64)
    absorption = torch.full((6,), 0.3, dtype=torch.float64, requires_grad=True)
    out = tac.simulate_rir_ism(room, source, mics, 1, absorption, 400, 9)
    assert out.dtype == torch.float64
    out.square().sum().backward()
    assert source.grad is not None and bool(torch.isfinite(source.grad).all()) and float(source.grad.abs().max()) > 0
    assert absorption.grad is not None and float(absorption.grad.abs().max()) > 0


def test_fake_kernels_and_one_graph(tac):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        room, source, mics = torch.empty(5, 3), torch.empty(5, 3), torch.empty(5, 4, 3)
        out = torch.ops.tac_amd.rir_ism(room, source, mics, torch.empty(1, 3, 6), 6, 40, 4000, 81, 343.0, 16000.0)
        assert tuple(out.shape) == (5, 3, 4, 4000) and out.dtype == torch.float32
        assert torch.ops.tac_amd.rir_ism(room.double(), source.double(), mics.double(), torch.empty(5, 1, 6).double(), 6, 0, 100, 81, 343.0,
                                         16000.0).dtype == torch.float64
        span = torch.ops.tac_amd.rir_ism_span(room, source, mics, 6, 81, 343.0, 16000.0)
        assert tuple(span.shape) == () and span.dtype == torch.int64
    seen = []

    def capture(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    torch._dynamo.reset()
    c = R.CASES[1]
    room, source, mics, a = tensors(c)
    fn = torch.compile(lambda r, s, m, w: tac.simulate_rir_ism_batch(r, s, m, c.max_order, w, 150, c.L, sample_rate=c.sample_rate),
                       backend=capture, fullgraph=True)
    out = fn(room, source, mics, a)
    assert sum('tac_amd.rir_ism' in n for n in seen) == 1 and not any('rir_ism_span' in n for n in seen), seen
    assert torch.equal(out, tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, 150, c.L, sample_rate=c.sample_rate))


def test_layer_and_names(tac):
    c = R.CASES[1]
    room, source, mics, a = tensors(c)
    layer = tac.SimulateRirIsm(c.max_order, a, 300, c.L, sample_rate=c.sample_rate)
    assert len(layer.state_dict()) == 0 and not list(layer.parameters()) and not list(layer.buffers())
    want = tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, 300, c.L, sample_rate=c.sample_rate)
    assert torch.equal(layer(room, source, mics), want) and torch.equal(layer(room[0], source[0], mics[0]), want[0])
    assert repr(layer) == 'SimulateRirIsm(max_order=1, output_length=300, delay_filter_length=5, sound_speed=343.0, sample_rate=8000.0)'
    with pytest.raises(ValueError, match='delay_filter_length'):
        tac.SimulateRirIsm(3, 0.2, delay_filter_length=80)
    for name in ('simulate_rir_ism', 'simulate_rir_ism_batch'):
        assert name in tac.functional.__all__ and getattr(tac, name) is getattr(tac.functional, name)
    assert tac.SimulateRirIsm is tac.layers.SimulateRirIsm
    for name in ('tac_rir_limits', 'tac_rir_ism_f32', 'tac_rir_span_f32'):
        assert name in tac._native.PROTOTYPES
