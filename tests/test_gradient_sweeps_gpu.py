"""-m gpu: the gradient kernels beside the main chain, swept past the one shape each was added with (tests/grad_rules.py holds
the generators, float64 references and bounds; tests/test_grad_rules_cpu.py runs the same bodies on the CPU route).

  * window gradient (``tac_window_grad_f32`` + ``tac_sum_slabs_f32``): total frame counts on either side of the partial-row
    count the device reports, so that workgroups own several frames, chunks cross from one row into the next and trailing
    workgroups own none; one-hot, silent-row and dense probes per case;
  * filterbank gradient (``_hip.filterbank_grad``): contractions over 1 .. 70 001 frames, one-hot frames held to one rounding of a
    product, dense sums to the accumulation bounds of grad_rules.py;
  * ``hpss``, ``phase_vocoder``, ``stretch_norm`` / ``stretch_mel`` gradients over their argument space, per row / per frame.

Strict mode and output poisoning are on.  ``TAC_FUZZ_CASES`` scales the drawn sweeps, ``TAC_FUZZ_SEED`` moves their stream,
``TAC_FUZZ_REPORT=path`` appends one JSON line per check (the measured numbers in DESIGN.md come from it)."""
import pytest
import torch

import grad_rules as gr

pytestmark = pytest.mark.gpu

GPU = torch.device('cuda')


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


@pytest.fixture(scope='module')
def partials(tac):
    return gr.window_partials(tac)


@pytest.mark.parametrize('index', range(len(gr.window_cases(gr.P_DEFAULT))), ids=[c['name'] for c in gr.window_cases(gr.P_DEFAULT)])
def test_window_gradient_across_the_partial_row_boundary(tac, partials, index):
    case = gr.window_cases(partials)[index]                # generated for the partial-row count of THIS device
    parts, per = gr.window_chunk(case['total'], partials)
    kernel, cpu32 = gr.window_case_body(tac, GPU, case, partials)
    print('window gradient %s: %d frames in %d rows, %d partial rows of %d frames: measure %.3g, float32 CPU %.3g (x 2^-24)'
          % (case['name'], case['total'], case['rows'], parts, per, kernel / gr.U, cpu32 / gr.U))


@pytest.mark.parametrize('k,n_freqs', gr.FB_SWEEP, ids=lambda v: str(v))
def test_filterbank_gradient_at_long_contractions(tac, k, n_freqs):
    worst = gr.fb_body(tac, GPU, k, n_freqs)
    print('filterbank gradient K %d, %d bins: (kernel, float32 CPU) measure x 2^-24 per n_mels: %r'
          % (k, n_freqs, {m: (round(a / gr.U, 2), round(b / gr.U, 2)) for m, (a, b) in worst.items()}))


def test_filterbank_gradient_behind_recomputed_rows(tac):
    gr.fb_fused_mel_body(tac, GPU)
    gr.fb_stretch_mel_body(tac, GPU)


def test_hpss_gradient_sweep(tac):
    worst = max(gr.hpss_case_body(tac, GPU, c) for c in gr.hpss_cases())
    print('hpss gradient: worst per-row ratio %.3g (bound 1e-4)' % worst)


def test_phase_vocoder_gradient_sweep(tac):
    for c in gr.pv_cases():
        worst, class_err = gr.pv_case_body(tac, GPU, c)
        print('phase_vocoder gradient case %d (advance %.0f rad, rate %.3g, %d frames): kernel %.3e, float32 oracle %.3e per frame'
              % (c['case'], c['advance'], c['rate'], c['n_frames'], worst, class_err))
    gr.pv_gaussian_body(tac, GPU)


def test_stretch_gradient_sweep(tac):
    worst = max(gr.stretch_case_body(tac, GPU, c) for c in gr.stretch_cases())
    print('stretch gradients: worst per-row ratio %.3g (bound 2e-5)' % worst)
