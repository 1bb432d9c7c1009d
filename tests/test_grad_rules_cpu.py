"""not-gpu: the sweep bodies of tests/grad_rules.py on CPU tensors through the package's CPU route, at the shapes and bounds
tests/test_gradient_sweeps_gpu.py uses on the kernels — the inputs, float64 references and bounds are sound before a GPU sees
them, and torch's float32 CPU evaluation alone stays inside every bound asserted — plus the premises of the generators: total
frame counts on either side of the partial-row count, no ties in an hpss row, silent rows."""
import numpy as np
import pytest
import torch

import grad_rules as gr
from oracle import signals

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


# ----------------------------------------------------------------------------- generators
@pytest.mark.parametrize('p', (1024, 416, 1216, 97))
def test_window_cases_sit_on_either_side_of_the_partial_row_count(p):
    cases = gr.window_cases(p)
    totals = [c['total'] for c in cases]
    for want in (p - 1, p, p + 1, 2 * p + 3):
        assert want in totals
    assert any(abs(t - 3.5 * p) <= 7 for t in totals)
    assert {c['rows'] for c in cases} >= {3, 7} or p != 1024
    for c in cases:
        assert c['rows'] * c['n_frames'] == c['total']
        assert gr.frames_of_length(c['length'], c['n_fft'], c['hop'], c['kw']['center']) == c['n_frames'], c
        parts, per = gr.window_chunk(c['total'], p)
        frames = gr.window_probe_frames(c, p)
        assert 0 in frames and c['total'] - 1 in frames
        if c['total'] > p:                   # several frames per workgroup: a chunk border is probed from both sides
            assert per >= 2 and any(f % per == 0 and f - 1 in frames for f in frames if f)
        if c['rows'] >= 2:                   # ... and a row border
            assert any(f % c['n_frames'] == 0 and f - 1 in frames for f in frames if f)
    by = {c['name']: c for c in cases}
    # p + 1 frames: per = 2, so only ceil((p + 1) / 2) of the p workgroups own frames — the rest write an all-zero partial row
    parts, per = gr.window_chunk(by['p+1']['total'], p)
    assert parts == p and per == 2 and -(-(p + 1) // per) < parts
    # chunks straddle rows: some chunk border lies strictly inside a row and some row border strictly inside a chunk
    for name in ('2p+3', '3.5p/7rows', '3.5p/3rows'):
        c = by[name]
        _, per = gr.window_chunk(c['total'], p)
        assert c['rows'] == 1 or any((r * c['n_frames']) % per for r in range(1, c['rows'])), name     # (one row: a prime total)
    assert {(c['n_fft'], c['hop']) for c in cases} >= {(64, 16), (400, 160), (300, 75), (77, 20), (2048, 512)}
    assert {c['kw']['pad_mode'] for c in cases} == {'reflect', 'constant', 'replicate', 'circular'}
    assert any(not c['kw']['center'] for c in cases) and any(c['kw']['win_length'] < c['n_fft'] for c in cases)
    assert any(c['kw']['normalized'] for c in cases) and any(not c['kw']['onesided'] for c in cases) and any(c['strided'] for c in cases)


def test_window_inputs_hold_a_silent_row_and_the_probe_waveform_none():
    for c in gr.window_cases(gr.P_DEFAULT):
        x, plain = gr.window_waves(c)
        assert x.shape == plain.shape == (c['rows'], c['length'])
        if c['rows'] >= 3:
            assert not x[1].any() and x[0].any() and x[2].any()
        assert (plain != 0).mean() > 0.99
    assert sum(c['rows'] >= 3 for c in gr.window_cases(gr.P_DEFAULT)) >= 8


def test_filterbank_cases_cover_every_k_as_one_row_and_as_several():
    for k in gr.FB_K:
        modes = gr.fb_row_modes(k)
        assert modes[0] == (1, k) and all(r * t == k for r, t in modes)
        assert k == 1 or (len(modes) == 2 and modes[1][0] > 1)
        probes = gr.fb_probe_indices(k, np.random.default_rng(0))
        assert probes[0] == 0 and probes[-1] == k - 1 and all(0 <= i < k for i in probes)
        if k > 64:
            assert {0, 31, 32, k - 33, k - 1} <= set(probes)
    spec, g = gr.fb_inputs(33, 3, 11, 201, 5)
    assert spec.shape == (3, 201, 11) and g.shape == (3, 130, 11) and spec.min() >= 0
    assert not spec[0, :, 1].any() and spec[0, :, 0].any()                     # a silent frame, a live first frame


def test_hpss_rows_hold_no_two_equal_values():
    cases = gr.hpss_cases()
    assert len(cases) >= 8
    for c in cases:
        s = gr.hpss_plane(np.random.default_rng(c['seed']), c['rows'], c['n_freqs'], c['n_frames'], c['first_gain'])
        assert s.dtype == np.float32 and s.min() > 0
        for r in range(c['rows']):
            assert np.unique(s[r]).size == s[r].size, c
        assert c['kf'] // 2 < c['n_freqs'] and c['kt'] // 2 < c['n_frames']
    assert any(c['kf'] // 2 == c['n_freqs'] - 1 for c in cases) and any(c['kt'] // 2 == c['n_frames'] - 1 for c in cases)
    assert any(max(c['kf'], c['kt']) > 31 for c in cases) and any(c['kf'] != c['kt'] for c in cases)
    assert any(c['frame_major'] for c in cases) and any(not c['frame_major'] for c in cases)
    assert any(c['hard'] for c in cases) and any(c['mask_only'] for c in cases) and any(c['silent_grad'] for c in cases)


def test_vocoder_and_stretch_cases_cover_the_edges():
    cases = gr.pv_cases()
    assert cases[0]['lead'] == (3, 2) and cases[0]['n_freqs'] == 101 and (6 * 101) % 256 and 256 % 101
    assert {2, 3} <= {c['n_frames'] for c in cases}
    assert any(c['rate'] == 1.0 for c in cases) and any(c['rate'] in (2.0, 3.0) for c in cases)
    assert any(c['rate'] > c['n_frames'] and len(gr.grid(c['n_frames'], c['rate'])[0]) == 1 for c in cases)
    z, _ = gr.pv_input(cases[0])
    mag = np.hypot(z[..., 0], z[..., 1])
    assert mag.min() >= 0.5 - 1e-6 and mag.max() <= 2.0 + 1e-6
    st = gr.stretch_cases()
    assert {c['rate'] for c in st} >= set(gr.STRETCH_RATES) and {c['power'] for c in st} == {1.0, 2.0, 0.7}
    assert any(c['db'] for c in st) and any(c['mel'] and c['bank_grad'] for c in st) and any(c['mel'] and not c['bank_grad'] for c in st)


def test_accumulation_measure():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    a = torch.tensor([4.0, 2.0, 0.0], dtype=torch.float64)
    assert gr.acc_measure(torch.tensor([1.0, -2.0, 0.0]), ref, a) == 0.0
    assert abs(gr.acc_measure(torch.tensor([1.5, -2.0, 0.0]), ref, a) - 0.125) < 1e-15
    assert gr.acc_measure(torch.tensor([1.0, -2.0, 1e-30]), ref, a) == float('inf')
    assert np.isnan(gr.acc_measure(torch.tensor([1.0, float('nan'), 0.0]), ref, a))
    assert gr.acc_tight(1) == gr.acc_hard(1) == 2.0 ** -24 and gr.acc_tight(70001) < gr.acc_hard(70001) / 60
    with pytest.raises(AssertionError):
        gr.check_acc(torch.tensor([1.0 + 64 * 4.0 * 2.0 ** -24, -2.0, 0.0]), ref, a, 4, 't', 'c')


def test_sequential_float32_sum_is_the_kernels_class():
    """One fused multiply-add per frame, in frame order, in float32 — the order the GEMM's single accumulator and the partial-row sum
    keep — stays inside 4 sqrt(K) 2^-24 on the sweep's operands, and is further from the float64 sum than torch's blocked float32
    matmul (8.78 against 4.22 x 2^-24 at K = 4097, 257 bins; the kernel measures 8.78 on the MI355X)."""
    k, n_freqs = 4097, 257
    spec, g = gr.fb_inputs(k, 1, k, n_freqs, 4300 + k + n_freqs)
    s64, g64 = torch.from_numpy(spec).double(), torch.from_numpy(g).double()
    ref, abs_sum = torch.einsum('rft,rmt->fm', s64, g64), torch.einsum('rft,rmt->fm', s64.abs(), g64.abs())
    acc = np.zeros((n_freqs, g.shape[1]), dtype=np.float32)
    for t in range(k):
        acc = (acc.astype(np.float64) + np.outer(spec[0, :, t].astype(np.float64), g[0, :, t].astype(np.float64))).astype(np.float32)
    seq = gr.acc_measure(torch.from_numpy(acc), ref, abs_sum)
    blocked = gr.acc_measure(torch.einsum('rft,rmt->fm', torch.from_numpy(spec), torch.from_numpy(g)), ref, abs_sum)
    print('sequential %.3f, blocked %.3f (x 2^-24)' % (seq / gr.U, blocked / gr.U))
    assert blocked <= seq <= gr.acc_tight(k)


# ----------------------------------------------------------------------------- the sweep bodies on the CPU route
@pytest.mark.parametrize('case', gr.window_cases(gr.P_DEFAULT), ids=lambda c: c['name'])
def test_window_gradient_on_cpu(tac, case):
    gr.window_case_body(tac, CPU, case, gr.P_DEFAULT, 'cpu_window_grad')


@pytest.mark.parametrize('k,n_freqs', gr.FB_SWEEP, ids=lambda v: str(v))
def test_filterbank_gradient_on_cpu(tac, k, n_freqs):
    gr.fb_body(tac, CPU, k, n_freqs, 'cpu_filterbank_grad')


def test_filterbank_gradient_behind_recomputed_rows_on_cpu(tac):
    gr.fb_fused_mel_body(tac, CPU)
    gr.fb_stretch_mel_body(tac, CPU)


def test_hpss_gradient_on_cpu(tac):
    for c in gr.hpss_cases():
        gr.hpss_case_body(tac, CPU, c, 'cpu_hpss_grad')


def test_hpss_restatement_is_the_oracle_at_equal_widths():
    from oracle import torch_ref
    mag = torch.from_numpy(gr.hpss_plane(np.random.default_rng(3), 2, 19, 23, 0)).double()
    for k, power, hard in ((5, 2.0, False), (11, 0.7, False), (3, 1.0, True)):
        for a, b in zip(torch_ref.hpss(mag[:, None], k, power, hard), gr.hpss_unequal(mag, k, k, power, hard)):
            assert torch.equal(a[:, 0], b)


def test_phase_vocoder_gradient_on_cpu(tac):
    for c in gr.pv_cases():
        worst, class_err = gr.pv_case_body(tac, CPU, c, 'cpu_phase_vocoder_grad')
        print('case %d: advance %.0f rad, CPU route %.3e, float32 oracle %.3e per frame' % (c['case'], c['advance'], worst, class_err))
    gr.pv_gaussian_body(tac, CPU)


def test_stretch_gradients_on_cpu(tac):
    for c in gr.stretch_cases():
        gr.stretch_case_body(tac, CPU, c, 'cpu_stretch_grad')
