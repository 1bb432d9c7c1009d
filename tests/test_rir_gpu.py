"""-m gpu: ``simulate_rir_ism`` / ``simulate_rir_ism_batch`` / ``SimulateRirIsm`` on the gfx950 kernel (csrc/rir.hip) — strict mode and poisoned
outputs on, as in tests/test_vad_gpu.py.

Reference and rules: tests/rir_rules.py — the float64 restatement of the definition in numpy, the per-element ``BOUND`` and the case
table (one restatement per case and window, computed once and shared).  A call is ONE ``tac_rir_ism_f32`` launch that writes every
element of the raw responses, plus ONE ``tac_rir_span_f32`` launch only when ``output_length is None``.  The launch is not persistent — a
wave takes one tile and leaves — so there is no unit beyond the grid to test; every case has more tiles than one workgroup's four."""
import warnings

import numpy as np
import pytest
import torch

import rir_rules as R

pytestmark = pytest.mark.gpu

ISM_ENTRY, SPAN_ENTRY = 'tac_rir_ism_f32', 'tac_rir_span_f32'


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


def tensors(c):
    a = c.absorption if isinstance(c.absorption, float) else torch.from_numpy(c.absorption).cuda()
    return torch.from_numpy(c.rooms).cuda(), torch.from_numpy(c.sources).cuda(), torch.from_numpy(c.mics).cuda(), a


def op_absorption(c):
    a = torch.from_numpy(c.bands()).cuda()
    return a[None] if a.dim() == 2 else a


def raw_op(tac_, c, start, length):
    """the op alone: exactly one launch, no warning"""
    room, source, mics, _ = tensors(c)
    before = dict(tac_._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac_.CompositeRouteWarning)
        got = tac_._ops.call('rir_ism', room, source, mics, op_absorption(c), c.max_order, start, length, c.L, c.sound_speed, c.sample_rate)
    assert launched_since(tac_, before) == {ISM_ENTRY: 1}
    assert got.is_cuda and got.dtype == torch.float32
    return got


def held(got, want, bound, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, what
    ratio, at = R.excess(got, want, bound)
    print('%s: %.3f of BOUND' % (what, ratio))
    assert ratio <= 1.0, (what, ratio, at)
    assert bool((got[bound == 0] == 0).all()), what              # where no image reaches: zeros, written


# ----------------------------------------------------------------------------- 1. the kernel against the float64 restatement
@pytest.mark.parametrize('c', R.CASES, ids=lambda c: c.name)
def test_kernel_within_the_bound(tac, c):
    P, n = c.L // 2, c.natural()
    for start, length in ((P, n), (0, n + P + 7)):
        want, bound = c.reference(start, length)
        got = raw_op(tac, c, start, length)
        held(got, want, bound, '%s, start %d' % (c.name, start))
        again = raw_op(tac, c, start, length)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), 'two calls differ'


@pytest.mark.parametrize('c', [R.CASES[0], R.CASES[3], R.CASES[4], R.CASES[5]], ids=lambda c: c.name)
def test_launches_of_the_functionals(tac, c):
    room, source, mics, a = tensors(c)
    P, n = c.L // 2, c.natural()
    want, bound = c.reference(P, n)
    kw = dict(delay_filter_length=c.L, sample_rate=c.sample_rate)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        before = dict(tac._hip.launches)
        natural = tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, **kw)
        assert launched_since(tac, before) == {ISM_ENTRY: 1, SPAN_ENTRY: 1}
        before = dict(tac._hip.launches)
        given = tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, n, **kw)
        assert launched_since(tac, before) == {ISM_ENTRY: 1}
        before = dict(tac._hip.launches)
        single = tac.SimulateRirIsm(c.max_order, a if isinstance(a, float) or a.dim() < 3 else a[0], n, **kw)(room[0], source[0], mics[0])
        assert launched_since(tac, before) == {ISM_ENTRY: 1}
    assert natural.is_cuda and tuple(natural.shape) == (len(c.rooms), c.mics.shape[1], n)
    assert want.shape[1] == 1
    held(natural, want[:, 0], bound[:, 0], c.name + ', natural length')
    assert torch.equal(natural.view(torch.int32), given.view(torch.int32))
    assert torch.equal(single.view(torch.int32), given[0].view(torch.int32))


def test_an_entry_alone_and_inside_a_batch(tac):
    """five different rooms, per-room absorption: every entry has the bits it has alone"""
    g = torch.Generator().manual_seed(11)
    room = torch.tensor([5.3, 4.1, 3.2]) + torch.rand(5, 3, generator=g)
    source = room * (0.2 + 0.6 * torch.rand(5, 3, generator=g))
    mics = room[:, None, :] * (0.1 + 0.8 * torch.rand(5, 3, 3, generator=g))
    a = 0.1 + 0.6 * torch.rand(5, 1, 6, generator=g)
    room, source, mics, a = room.cuda(), source.cuda(), mics.cuda(), a.cuda()
    n = 1100
    both = tac.simulate_rir_ism_batch(room, source, mics, 4, a, n)
    assert tuple(both.shape) == (5, 3, n)
    for i in range(5):
        alone = tac.simulate_rir_ism(room[i], source[i], mics[i], 4, a[i], n)
        assert torch.equal(both[i].view(torch.int32), alone.view(torch.int32)), i
        want, bound = R.raw(room[i].cpu().numpy(), source[i].cpu().numpy(), mics[i].cpu().numpy(), a[i].cpu().numpy(), 4, 81, 16000.0, 343.0, 40, n)
        held(alone, want[0], bound[0], 'room %d of 5' % i)
    assert len({tuple(both[i, 0, :400].tolist()) for i in range(5)}) == 5


# ----------------------------------------------------------------------------- 2. tile edges
#: dense enough for 10 or more images of every channel to straddle the boundary behind the third tile
TILE_CASE = R.Case('3-D order 8, float, L 81, 16 kHz', [R.ROOM_A], [R.SOURCE_A], [R.MICS_A], 8, 0.3, 81, 16000.0)


def tiled(tac_, c, start, length, tile):
    """the launcher with the tile given: one launch"""
    room, source, mics, _ = tensors(c)
    before = dict(tac_._hip.launches)
    got = tac_._hip.rir_ism(room, source, mics, op_absorption(c), c.max_order, start, length, c.L, c.sound_speed, c.sample_rate, tile)
    assert launched_since(tac_, before) == {ISM_ENTRY: 1}
    return got


@pytest.mark.parametrize('tile', [128, 256, 512, 1024, 2048])
def test_tile_edges(tac, tile):
    """every tile length the launch may choose, given by hand: lengths around one tile, three tiles plus 37, one sample, and far past the
    last image; the bits are those of the launch's own choice"""
    c = TILE_CASE                                                          # order 8: 833 images over 2087 samples
    P, n = c.L // 2, c.natural()
    assert tac._hip.rir_limits()[0] == 128 and tac._hip.rir_tile(4, 2087, 1) == (128, 2048) and n == 2087
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def rule(rows, length, top):                          # the longest tile that leaves 16 waves a CU, 128 at the least
        return next((s for s in (2048, 1024, 512, 256) if s <= top and rows * -(-length // s) >= 16 * cus), 128)

    for rows, length in ((1024, 8000), (64, 16000), (256, 8000), (100, 777)):
        assert tac._hip.rir_tile(rows, length, 1) == (rule(rows, length, 2048), 2048), (rows, length)
    assert tac._hip.rir_tile(1 << 20, 8000, 1)[0] == 2048 and tac._hip.rir_tile(1 << 20, 8000, 3) == (1024, 1024)
    assert tac._hip.rir_tile(1 << 20, 8000, 8) == (512, 512)
    far = 3 * tile + 700 if 3 * tile + 37 > n else n + 700
    want, bound = c.reference(P, 3 * 2048 + 700)
    # images straddle the tile boundaries that lie inside the response, of every channel: supports [di, di + L), boundaries at P + k tile
    _, _, di = R.geometry(c.rooms[0], c.sources[0], c.mics[0], c.bands(), c.max_order, c.sample_rate, c.sound_speed)
    inside = [k for k in (1, 2, 3) if P + k * tile < 1600]
    assert inside or tile == 2048
    for k in inside:
        assert bool(((di < P + k * tile) & (di + c.L > P + k * tile)).any(0).all()), k
    for length in (1, tile - 1, tile, tile + 1, 3 * tile + 37, far):
        got = tiled(tac, c, P, length, tile)
        held(got, want[..., :length], bound[..., :length], 'tile %d, output_length %d' % (tile, length))
        auto = raw_op(tac, c, P, length)
        assert torch.equal(got.view(torch.int32), auto.view(torch.int32)), (tile, length)
    assert bool((got[..., n:] == 0).all()) and bool((bound[..., n:] == 0).all())       # past the last image: zeros, written
    # the head cut by ``start``: the microphone 0.24 m from the source has its direct path before sample P
    assert int(di[:, 2].min()) < P and float(np.abs(want[0, 0, 2, :8]).max()) > 0.1


def test_tiles_of_several_bands(tac):
    """three bands take tiles up to 1024; a longer one is refused by the entry, not run"""
    c = R.CASES[2]
    n = c.natural()
    want, bound = c.reference(0, n + 47)
    for tile in (128, 512, 1024):
        held(tiled(tac, c, 0, n + 47, tile), want, bound, 'three bands, tile %d' % tile)
    with pytest.raises(RuntimeError):
        tiled(tac, c, 0, n + 47, 2048)


# ----------------------------------------------------------------------------- 3. several bands
def test_multiband_is_the_hand_composition(tac):
    c = R.CASES[2]
    room, source, mics, a = tensors(c)
    centres = torch.tensor(R.CENTRES)
    P, n = c.L // 2, 700
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        before = dict(tac._hip.launches)
        got = tac.simulate_rir_ism(room[0], source[0], mics[0], c.max_order, a, n, c.L, centres, c.sound_speed, c.sample_rate)
        since = launched_since(tac, before)
        assert since.pop(ISM_ENTRY) == 1 and SPAN_ENTRY not in since and since and all(k.startswith('tac_') for k in since), since
        raw = tac._ops.call('rir_ism', room, source, mics, a[None], c.max_order, 0, P + n + 255, c.L, c.sound_speed, c.sample_rate)
        filters = tac._rir.band_filters(R.CENTRES, c.sample_rate, raw.device)[:, None, :]
        hand = torch.sum(tac.fftconvolve(raw[0], filters, mode='same'), dim=0)[..., P:P + n]
        batch = tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, n, c.L, centres, c.sound_speed, c.sample_rate)
    assert tuple(got.shape) == (4, n) and torch.equal(got.view(torch.int32), hand.view(torch.int32))
    assert torch.equal(batch[0].view(torch.int32), got.view(torch.int32))
    want = R.multiband(c.rooms[0], c.sources[0], c.mics[0], c.bands(), R.CENTRES, c.max_order, c.L, c.sample_rate, c.sound_speed, n)
    reach = float(np.abs(got.cpu().double().numpy() - want).max())
    print('multi-band on the device: %.3g off the float64 restatement at a peak of %.3g' % (reach, np.abs(want).max()))
    # the margin: 4 times the 1.9e-7 the CPU composite route reaches on this case (tests/test_rir_cpu.py prints it), at a peak of 2.78
    assert reach <= 4 * 1.9e-7


# ----------------------------------------------------------------------------- 4. the chain
def test_chain_into_fftconvolve_without_the_host(tac):
    g = torch.Generator().manual_seed(5)
    room = torch.tensor([6.0, 5.0, 3.0]) + torch.rand(4, 3, generator=g)
    source = room * (0.2 + 0.6 * torch.rand(4, 3, generator=g))
    mics = room[:, None, :] * (0.2 + 0.6 * torch.rand(4, 1, 3, generator=g))
    room, source, mics = room.cuda(), source.cuda(), mics.cuda()
    x = torch.randn(4, 1, 16000, generator=g).cuda()

    def simulate():
        return tac.simulate_rir_ism_batch(room, source, mics, 6, 0.35, output_length=4000)

    tac.fftconvolve(x, simulate())                                          # (the tables reach the device once)
    torch.cuda.synchronize()
    before = dict(tac._hip.launches)
    with warnings.catch_warnings():
        warnings.simplefilter('error', tac.CompositeRouteWarning)
        torch.cuda.set_sync_debug_mode('error')                             # nothing in the simulation waits for the host, so nothing reads its result
        try:
            rir = simulate()
        finally:
            torch.cuda.set_sync_debug_mode('default')
        # (fftconvolve uploads a row map for every new kernel tensor: a copy TO the device, its own and no read of ``rir``)
        wet = tac.fftconvolve(x, rir)
    since = launched_since(tac, before)
    assert since.pop(ISM_ENTRY) == 1 and SPAN_ENTRY not in since and since and all(k.startswith('tac_') for k in since), since
    assert tuple(rir.shape) == (4, 1, 4000) and tuple(wet.shape) == (4, 1, 19999)
    want = np.stack([np.convolve(x[i, 0].cpu().double().numpy(), rir[i, 0].cpu().double().numpy()) for i in range(4)])
    scale = float(np.abs(want).max())
    assert float(np.abs(wet[:, 0].cpu().double().numpy() - want).max()) <= 1e-5 * scale        # (fftconvolve's own tests hold its bound)


# ----------------------------------------------------------------------------- 5. the refused calls
def test_refused_calls_take_the_composite(tac):
    c = R.CASES[1]
    room, source, mics, a = tensors(c)
    P, n = c.L // 2, c.natural()
    nine = torch.from_numpy(np.tile(c.bands(), (9, 1))).cuda()[None]
    before = dict(tac._hip.launches)
    with pytest.raises(RuntimeError, match='dtype float64'):
        tac.simulate_rir_ism_batch(room.double(), source.double(), mics.double(), c.max_order, a.double(), n, c.L, sample_rate=c.sample_rate)
    with pytest.raises(RuntimeError, match='9 absorption bands'):
        tac._ops.call('rir_ism', room, source, mics, nine, c.max_order, P, n, c.L, c.sound_speed, c.sample_rate)
    with pytest.raises(RuntimeError, match='a delay filter of 257 taps'):
        tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, n, 257, sample_rate=c.sample_rate)
    with pytest.raises(RuntimeError, match='expanded or non-positive strides'):
        tac.simulate_rir_ism_batch(room.expand(3, -1), source.expand(3, -1), mics.expand(3, -1, -1), c.max_order, a, n, c.L,
                                   sample_rate=c.sample_rate)
    with pytest.raises(ValueError):
        tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, n, 80, sample_rate=c.sample_rate)
    assert launched_since(tac, before) == {}
    tac.set_strict(False)
    try:
        for key in [k for k in tac._ops._warned if k[0] in ('rir_ism', 'rir_ism_span')]:
            tac._ops._warned.discard(key)
        want, bound = c.reference(P, n)
        with pytest.warns(tac.CompositeRouteWarning):
            got = tac.simulate_rir_ism_batch(room.double(), source.double(), mics.double(), c.max_order, a.double(), n, c.L,
                                             sample_rate=c.sample_rate)
        assert got.is_cuda and got.dtype == torch.float64
        held(got, want[:, 0], bound[:, 0], 'float64 on the device')
        with pytest.warns(tac.CompositeRouteWarning):
            got = tac._ops.call('rir_ism', room, source, mics, nine, c.max_order, P, n, c.L, c.sound_speed, c.sample_rate)
        assert tuple(got.shape) == (1, 9, 4, n)
        for b in range(9):
            held(got[:, b], want[:, 0], bound[:, 0], 'band %d of 9' % b)
        with pytest.warns(tac.CompositeRouteWarning):
            got = tac.simulate_rir_ism_batch(room, source, mics, c.max_order, a, n, 257, sample_rate=c.sample_rate)
        w257, b257 = R.raw_batch(c.rooms, c.sources, c.mics, c.bands(), c.max_order, 257, c.sample_rate, c.sound_speed, 128, n)
        held(got, w257[:, 0], b257[:, 0], '257 taps')
        assert launched_since(tac, before) == {}
    finally:
        tac.set_strict(True)
