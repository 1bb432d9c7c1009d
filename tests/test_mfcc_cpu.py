"""``create_dct`` / ``dct`` / ``DCT`` / ``MFCC`` without a device: the matrix against ``scipy.fft.dct`` (tests/golden/g13_dct.npz,
written by tests/golden/make_golden_dct.py), the CPU route against the float64 reference under the bound of tests/dct_rules.py,
argument errors, shapes, gradcheck, tracing as one node, the factory's children and buffers, and the C ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dct_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS = (None, 'ortho')


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


@pytest.fixture(scope='module')
def gold():
    return np.load(R.GOLDEN)


# ----------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('num_mels,num_coeffs', R.GOLDEN_SIZES)
def test_closed_form_is_scipys_dct(gold, num_mels, num_coeffs, norm):
    """x @ D64 against scipy's outputs: within 1e-13 of the sum of absolute products, per element"""
    x = gold['x_%d' % num_mels]
    want = gold['y_%d_%d_%s' % (num_mels, num_coeffs, R.norm_tag(norm))]
    d64 = R.dct_matrix64(num_coeffs, num_mels, norm)
    assert d64.shape == (num_mels, num_coeffs) and want.shape == (x.shape[0], num_coeffs)
    assert (np.abs(x @ d64 - want) <= 1e-13 * (np.abs(x) @ np.abs(d64))).all()


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('num_mels,num_coeffs', R.GOLDEN_SIZES)
def test_create_dct(tac, gold, num_mels, num_coeffs, norm):
    d = tac.create_dct(num_coeffs, num_mels, norm)
    assert d.dtype == torch.float32 and tuple(d.shape) == (num_mels, num_coeffs) and d.is_contiguous()
    d64 = R.dct_matrix64(num_coeffs, num_mels, norm)
    # one rounding of the float64 value (the 1e-15: torch's and numpy's float64 cosines may differ in their last bit)
    assert (np.abs(d.numpy().astype(np.float64) - d64) <= R.EPS * np.abs(d64) + 1e-15).all()
    # and, through the golden frames, scipy's matrix: one rounding of each of the num_mels products
    x = gold['x_%d' % num_mels]
    want = gold['y_%d_%d_%s' % (num_mels, num_coeffs, R.norm_tag(norm))]
    assert (np.abs(x @ d.numpy().astype(np.float64) - want) <= (R.EPS + 1e-13) * (np.abs(x) @ np.abs(d64))).all()
    if norm == 'ortho' and num_coeffs == num_mels:
        assert np.abs(d64.T @ d64 - np.eye(num_mels)).max() < 1e-13


def test_create_dct_defaults_and_errors(tac):
    assert torch.equal(tac.create_dct(13, 40), tac.create_dct(13, 40, norm='ortho'))
    assert torch.equal(tac.create_dct(5, 40), tac.create_dct(13, 40)[:, :5])
    for bad in ('backward', 'forward', 'orthogonal', 1):
        with pytest.raises(ValueError):
            tac.create_dct(13, 40, norm=bad)
    for bad in (0, -1, 41):
        with pytest.raises(ValueError):
            tac.create_dct(bad, 40)


# ----------------------------------------------------------------------------- dct on CPU tensors
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('n_in,n_out', [(8, 8), (23, 13), (40, 13), (80, 40), (128, 40), (128, 128), (256, 64)])
def test_dct_cpu_float32_within_the_bound(tac, n_in, n_out, norm):
    x = torch.from_numpy(R.db_like((3, n_in, 37), seed=n_in + n_out))
    x[1, :, 5] = 0.0
    x[2, :, 7] *= 1e-30
    got = tac.dct(x, tac.create_dct(n_out, n_in, norm))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, n_out, 37)
    ratio = R.assert_within(got, x, R.dct_matrix64(n_out, n_in, norm), 'cpu float32 %dx%d %s' % (n_in, n_out, norm))
    assert ratio < 1.0
    assert not bool(got[1, :, 5].any())


@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('num_mels,num_coeffs', R.GOLDEN_SIZES)
def test_dct_cpu_float64_is_the_golden(tac, gold, num_mels, num_coeffs, norm):
    x = torch.from_numpy(gold['x_%d' % num_mels].T.copy())                      # (M, 16): frames along the last axis
    want = gold['y_%d_%d_%s' % (num_mels, num_coeffs, R.norm_tag(norm))].T
    got = tac.dct(x, torch.from_numpy(R.dct_matrix64(num_coeffs, num_mels, norm)))
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_shapes_and_layout(tac):
    d = tac.create_dct(5, 12)
    for lead in ((), (3,), (2, 3)):
        x = torch.randn(lead + (12, 9))
        got = tac.dct(x, d)
        assert tuple(got.shape) == lead + (5, 9)
        assert torch.equal(got, (x.transpose(-1, -2) @ d).transpose(-1, -2))
        assert torch.equal(tac.DCT(d)(x), got)
    got = tac.dct(torch.randn(2, 3, 12, 9).transpose(0, 1), d)
    assert tuple(got.shape) == (3, 2, 5, 9)


def test_argument_errors(tac):
    d = tac.create_dct(5, 12)
    with pytest.raises(RuntimeError, match='size mismatch'):
        tac.dct(torch.randn(2, 13, 9), d)                   # 13 bands are not the matrix's 12
    with pytest.raises(RuntimeError, match='size mismatch'):
        tac.dct(torch.randn(2, 9, 12), d)                   # the band axis is dim -2
    with pytest.raises(RuntimeError, match='size mismatch'):
        tac.dct(torch.randn(12), d)
    with pytest.raises(RuntimeError, match='size mismatch'):
        tac.dct(torch.randn(2, 12, 9), d[:, 0])
    with pytest.raises(TypeError):
        tac.dct(np.zeros((12, 9), dtype=np.float32), d)
    with pytest.raises(TypeError):
        tac.dct(torch.randn(12, 9), d.numpy())


def test_gradcheck_cpu(tac):
    x = torch.randn(2, 8, 5, dtype=torch.float64, requires_grad=True)
    d = torch.from_numpy(R.dct_matrix64(6, 8)).requires_grad_(True)
    assert torch.autograd.gradcheck(tac.dct, (x, d.detach()))
    assert torch.autograd.gradcheck(tac.dct, (x, d))
    assert torch.autograd.gradgradcheck(tac.dct, (x, d.detach()))


def test_traces_as_one_node(tac):
    seen = []

    def capture(gm, example_inputs):
        seen.extend(n.target for n in gm.graph.nodes if n.op == 'call_function')
        return gm.forward

    torch._dynamo.reset()
    layer = tac.DCT(tac.create_dct(13, 40))
    x = torch.randn(2, 3, 40, 11)
    out = torch.compile(layer, backend=capture, fullgraph=True)(x)
    names = [str(t) for t in seen]
    assert sum('tac_amd.dct' in n for n in names) == 1 and len(names) == 1, names
    eager = layer(x)
    assert torch.equal(out, eager)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode() as mode:
        fake = torch.ops.tac_amd.dct(mode.from_tensor(x), mode.from_tensor(layer.dct_matrix))
    # the fake kernel describes what the device kernels write: (…, n_out, T) as a view of frame-major storage
    assert tuple(fake.shape) == tuple(eager.shape) == (2, 3, 13, 11) and fake.dtype == eager.dtype
    assert fake.stride() == (3 * 11 * 13, 11 * 13, 1, 13)


# ----------------------------------------------------------------------------- layers
def test_mfcc_factory(tac):
    kw = dict(num_mels=40, sample_rate=16000, fft_length=400, hop_length=160)
    m = tac.MFCC(num_coeffs=13, **kw)
    assert type(m) is torch.nn.Sequential
    assert [type(c).__name__ for c in m] == ['STFT', 'ComplexNorm', 'ApplyFilterbank', 'AmplitudeToDb', 'DCT']
    assert m.state_dict() == {} and [n for n, _ in m.named_buffers()] == ['0.window', '2.filterbank', '4.dct_matrix']
    assert torch.equal(m[4].dct_matrix, tac.create_dct(13, 40, 'ortho'))
    x = torch.randn(2, 1, 4000)
    want = tac.dct(tac.AmplitudeToDb()(tac.Melspectrogram(**kw)(x)), tac.create_dct(13, 40))
    got = m(x)
    assert type(got) is torch.Tensor and tuple(got.shape) == (2, 1, 13, 26) and torch.equal(got, want)
    assert torch.equal(m[4](m[3](m[2](m[1](m[0](x))))), want)                    # the children, one by one
    # the arguments reach the stages they belong to
    m2 = tac.MFCC(20, None, 2.0, 1e-5, **kw)
    assert (m2[3].ref, m2[3].amin) == (2.0, 1e-5) and torch.equal(m2[4].dct_matrix, tac.create_dct(20, 40, None))
    assert tuple(tac.MFCC(fft_length=512)[4].dct_matrix.shape) == (128, 40)     # the defaults: 40 of Melspectrogram's 128 bands
    with pytest.raises(ValueError):
        tac.MFCC(num_coeffs=41, **kw)
    assert repr(m[4]) == 'DCT(num_mels=40, num_coeffs=13)'
    m.load_state_dict({})
    assert m.double()[4].dct_matrix.dtype == torch.float64


def test_mulaw_front_end_keeps_its_chain(tac):
    """codes -> MuLawDecoding -> MFCC equals decoding first (CPU: the same operators either way)"""
    kw = dict(num_mels=40, sample_rate=16000, fft_length=400, hop_length=160)
    codes = torch.randint(0, 256, (2, 1, 4000))
    m = tac.MFCC(num_coeffs=13, **kw)
    full = torch.nn.Sequential(tac.MuLawDecoding(256), *m)
    assert torch.equal(full(codes), m(tac.mu_law_decoding(codes, 256)))


def test_names_are_exported(tac):
    for name in ('create_dct', 'dct'):
        assert name in tac.functional.__all__ and getattr(tac, name) is getattr(tac.functional, name)
    for name in ('DCT', 'MFCC'):
        assert getattr(tac, name) is getattr(tac.layers, name)
    assert 'dct' in tac._ops.cuda_kernels and hasattr(torch.ops.tac_amd, 'dct')


# ----------------------------------------------------------------------------- C ABI
def test_entry_point_is_declared_and_exported(tac):
    header = open(os.path.join(ROOT, 'include', 'tac_amd.h')).read()
    assert re.search(r'\bint\s+tac_dct_rows_f32\s*\(', header) and '(14)' in header
    assert 'tac_dct_rows_f32' in tac._native.EXPORTS
    if not os.path.exists(tac._native.LIB_PATH):
        tac.build_native()
    h = tac._native.lib()
    assert h.tac_abi_version() == 5
    fn = h.tac_dct_rows_f32
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 11
    # refusals come before anything touches a device: null pointers, empty axes, sizes beyond the cap
    p = ctypes.c_void_p(4096)
    assert fn(None, 1, 8, 4, 32, 1, 8, p, 8, p, None) == tac._native.TAC_E_INVALID
    assert fn(p, 0, 8, 4, 32, 1, 8, p, 8, p, None) == tac._native.TAC_E_INVALID
    assert fn(p, 2, 8, 4, 32, 0, 8, p, 8, p, None) == tac._native.TAC_E_INVALID
    for n_in, n_out in ((256, 256), (257, 1), (1, 257), (129, 255)):
        assert fn(p, 1, n_in, 4, 4 * n_in, 1, n_in, p, n_out, p, None) == tac._native.TAC_E_UNSUPPORTED
    assert tac._hip.dct_covers(129, 254) and tac._hip.dct_covers(256, 128) and not tac._hip.dct_covers(256, 129)
