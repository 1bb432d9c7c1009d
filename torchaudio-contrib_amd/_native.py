"""ctypes binding of libtac_amd.so — the C ABI declared in include/tac_amd.h.

PyTorch is plumbing here (device memory, the current HIP stream); every compute call goes to
a hand-written gfx950 kernel through plain pointers.  There is deliberately NO fallback: if
the library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os
import subprocess
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TAC_AMD_LIB', os.path.join(_HERE, 'libtac_amd.so'))   # override: A/B builds
CSRC = os.path.join(_HERE, 'csrc')

TAC_OK = 0
TAC_E_INVALID = -1
TAC_E_UNSUPPORTED = -2
TAC_E_SHORT_INPUT = -3
TAC_E_LAUNCH = -4

PAD_MODES = {'constant': 0, 'reflect': 1, 'replicate': 2, 'circular': 3}
SAMPLES_F32, SAMPLES_I16, SAMPLES_MULAW_U8, SAMPLES_MULAW_I64 = 0, 1, 2, 3

ABI_VERSION = 5          # tac_abi_version() of the library this binding was written against (csrc/host_common.hip)


class StftDesc(ctypes.Structure):
    """mirror of ``tac_stft_desc`` (include/tac_amd.h)."""
    _fields_ = [('rows', ctypes.c_int64), ('length', ctypes.c_int64), ('row_stride', ctypes.c_int64),
                ('n_fft', ctypes.c_int32), ('hop', ctypes.c_int32), ('win_length', ctypes.c_int32),
                ('center', ctypes.c_int32), ('pad_mode', ctypes.c_int32), ('normalized', ctypes.c_int32),
                ('onesided', ctypes.c_int32), ('reserved', ctypes.c_int32)]


_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
_F = ctypes.c_float
_D = ctypes.c_double
_DESC = ctypes.POINTER(StftDesc)
_INT = ctypes.c_int
_STR = ctypes.c_char_p

_SPEC = [_P, _I64, _I32, _I64, _I64, _I64, _I64, _I64, _I64]          # spec, batch, channels, bins, frames, four strides
_MASK = [_P, _I64, _I64, _I64]

#: the C ABI of include/tac_amd.h, once: entry point -> (restype, argtypes).  ``lib()`` applies it to the loaded library;
#: tests/test_abi_table_cpu.py holds every entry to the header's declaration.
PROTOTYPES = {
    'tac_strerror': (_STR, [_INT]),
    'tac_last_hip_error': (_INT, []),
    'tac_abi_version': (_INT, []),
    'tac_num_frames': (_I64, [_I64, _INT, _INT, _INT]),
    'tac_num_bins': (_INT, [_INT, _INT]),
    'tac_stft_f32': (_INT, [_P, _P, _DESC, _P, _P]),
    'tac_spectrogram_f32': (_INT, [_P, _P, _DESC, _F, _INT, _F, _F, _P, _P]),
    'tac_melspec_f32': (_INT, [_P, _P, _DESC, _F, _P, _P, _I32, _INT, _F, _F, _P, _P]),
    'tac_melspec_supported': (_INT, [_DESC, _F, _P, _I32]),
    'tac_filterbank_plan': (_INT, [_P, _I32, _I32, _P, _P, _P]),
    'tac_melbank_pack': (_INT, [_P, _I32, _I32, _I32, _P, _I32, _P, _I32, _P, _P]),
    'tac_melbank_pack_host': (_INT, [_P, _I32, _I32, _I32, _P, _I32, _P, _I32, _P]),
    'tac_melspec_sparse_f32': (_INT, [_P, _P, _DESC, _F, _P, _P, _P, _I32, _INT, _F, _F, _P, _P]),
    'tac_apply_filterbank_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _I64, _P, _P, _I32, _P, _P]),
    'tac_apply_filterbank_sparse_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _P, _P, _P, _I32, _P, _P]),
    'tac_apply_filterbank_sparse_db_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _P, _P, _P, _I32, _INT, _F, _F, _P, _P]),
    'tac_complex_norm_f32': (_INT, [_P, _I64, _F, _P, _P]),
    'tac_magphase_f32': (_INT, [_P, _I64, _F, _P, _P, _P]),
    'tac_phase_vocoder_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _P, _P]),
    'tac_phase_vocoder_f64': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _I64, _P, _P]),
    'tac_phase_vocoder_backward_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _I64, _P, _P, _P, _I64, _P, _P, _P]),
    'tac_amplitude_to_db_f32': (_INT, [_P, _I64, _F, _F, _P, _P]),
    'tac_stretch_norm_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _P, _P, _I64, _F, _INT, _F, _F, _P, _P, _P]),
    'tac_stretch_mel_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _P, _P, _I64, _F, _P, _P, _P, _I32, _INT, _F, _F, _P, _P, _P]),
    'tac_stretch_norm_backward_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _P, _P, _P, _I64, _F, _P, _P, _P]),
    'tac_db_to_amplitude_f32': (_INT, [_P, _I64, _F, _P, _P]),
    'tac_mulaw_encode_f32_i64': (_INT, [_P, _I64, _I32, _P, _I32, _I32, _I32, _P, _P]),
    'tac_mulaw_decode_i64_f32': (_INT, [_P, _I64, _I32, _P, _P, _P]),
    'tac_mulaw_decode_f32_f32': (_INT, [_P, _I64, _I32, _P, _P, _P]),
    'tac_mulaw_encode_f64_i64': (_INT, [_P, _I64, _I32, _P, _P]),
    'tac_mulaw_decode_f64': (_INT, [_P, _I32, _I64, _I32, _P, _P]),
    'tac_stft_backward_f32': (_INT, [_P, _P, _DESC, _P, _P]),
    'tac_stft_norm_backward_f32': (_INT, [_P, _P, _F, _P, _DESC, _P, _P]),
    'tac_spectrogram_backward_f32': (_INT, [_P, _P, _DESC, _P, _F, _P, _P]),
    'tac_spectrogram_backward_ola_workspace': (_I64, [_DESC]),
    'tac_spectrogram_backward_ola_f32': (_INT, [_P, _P, _DESC, _P, _F, _P, _I64, _P, _I64, _P]),
    'tac_melspectrogram_backward_ola_f32': (_INT, [_P, _P, _DESC, _P, _I32, _P, _I32, _F, _P, _I64, _P, _I64, _P]),
    'tac_melspectrogram_backward_f32': (_INT, [_P, _P, _DESC, _P, _I32, _P, _I32, _F, _P, _P]),
    'tac_filterbank_adjoint_pack': (_INT, [_P, _I32, _I32, _P, _P, _P]),
    'tac_apply_filterbank_adjoint_f32': (_INT, [_P, _I64, _I32, _P, _I32, _P, _P]),
    'tac_overlap_add_f32': (_INT, [_P, _DESC, _P, _I64, _P]),
    'tac_complex_norm_backward_f32': (_INT, [_P, _P, _I64, _F, _P, _P]),
    'tac_amplitude_to_db_backward_f32': (_INT, [_P, _P, _I64, _F, _P, _P]),
    'tac_magphase_backward_f32': (_INT, [_P, _P, _P, _I64, _F, _P, _P]),
    'tac_db_to_amplitude_backward_f32': (_INT, [_P, _P, _I64, _F, _P, _P]),
    'tac_hpss_f32': (_INT, [_P, _I64, _I32, _I32, _I64, _I64, _I64, _I32, _I32, _F, _INT, _P, _P, _P, _P, _P]),
    'tac_hpss_backward_f32': (_INT, [_P, _I64, _I32, _I32, _I64, _I64, _I64, _I32, _I32, _F, _INT, _P, _P, _P, _P, _P, _P]),
    'tac_melspec_sparse_coded_f32': (_INT, [_P, _I32, _P, _P, _DESC, _F, _P, _P, _P, _I32, _INT, _F, _F, _P, _P]),
    'tac_pcm16_to_f32': (_INT, [_P, _I64, _P, _P]),
    'tac_fold_twosided_f32': (_INT, [_P, _I64, _I32, _I32, _P, _P]),
    'tac_window_grad_partials': (_I64, [_DESC]),
    'tac_window_grad_f32': (_INT, [_P, _P, _DESC, _P, _I64, _P]),
    'tac_sum_slabs_f32': (_INT, [_P, _I64, _I64, _P, _P]),
    'tac_stft_f64': (_INT, [_P, _P, _DESC, _P, _P]),
    'tac_spectrogram_f64': (_INT, [_P, _P, _DESC, _D, _INT, _D, _D, _P, _P]),
    'tac_apply_filterbank_f64': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _I64, _P, _I32, _INT, _D, _D, _P, _P]),
    'tac_magphase_f64': (_INT, [_P, _I64, _D, _P, _P, _P]),
    'tac_amplitude_to_db_f64': (_INT, [_P, _I64, _D, _D, _P, _P]),
    'tac_db_to_amplitude_f64': (_INT, [_P, _I64, _D, _P, _P]),
    'tac_last_route': (_STR, []),
    'tac_debug_clock_probe': (_INT, [_P, _I32]),
    'tac_melbank_plan_pieces_host': (_INT, [_P, _I32, _I32, _P, _P, _P, _P, _P, _I32]),
    'tac_set_fft_pipe': (_INT, [_INT]),
    'tac_istft_workspace': (_I64, [_DESC, _I64]),
    'tac_istft_envelope_f32': (_INT, [_P, _DESC, _I64, _P, _P, _P]),
    'tac_istft_f32': (_INT, [_P, _I64, _I64, _I64, _P, _P, _DESC, _P, _I64, _P, _P]),
    'tac_istft_grad_input_f32': (_INT, [_P, _I64, _P, _DESC, _I64, _P, _P]),
    'tac_istft_grad_bins_f32': (_INT, [_P, _I64, _INT, _INT, _P]),
    'tac_dct_rows_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _I64, _P, _I32, _P, _P]),
    'tac_polyphase_f32': (_INT, [_P, _I64, _I64, _I64, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I64, _P, _P]),
    'tac_lfilter_chunk': (_I32, []),
    'tac_lfilter_supported': (_INT, [_P, _P, _I32]),
    'tac_lfilter_f32': (_INT, [_P, _I64, _I64, _I64, _P, _P, _I32, _INT, _INT, _P, _P]),
    'tac_spectral_mac_tile': (_I32, [_I32]),
    'tac_spectral_mac_f32': (_INT, [_P, _P, _P, _I64, _I64, _I32, _I32, _I32, _INT, _P, _P]),
    'tac_fftconvolve_default_n_fft': (_I32, [_I64]),
    'tac_fftconvolve_supported': (_INT, [_I64, _I64, _I32]),
    'tac_fftconvolve_spectra_workspace': (_I64, [_I64, _I64, _I32]),
    'tac_fftconvolve_spectra_f32': (_INT, [_P, _I64, _I64, _I64, _I32, _INT, _P, _I64, _P, _P]),
    'tac_fftconvolve_workspace': (_I64, [_I64, _I64, _I64, _I32, _I64, _I64]),
    'tac_fftconvolve_f32': (_INT, [_P, _I64, _I64, _I64, _P, _P, _I32, _I64, _I32, _INT, _I64, _I64, _P, _I64, _P, _I64, _P]),
    'tac_fftconvolve_direct_f32': (_INT, [_P, _I64, _I64, _I64, _P, _P, _I64, _I64, _I64, _P, _P]),
    'tac_kaldi_num_frames': (_I64, [_I64, _I32, _I32, _INT]),
    'tac_kaldi_fbank_f32': (_INT, [_P, _I64, _I64, _I64, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _F, _P, _P]),
    'tac_kaldi_mfcc_table_limit': (_I64, [_I32, _I32, _I32]),
    'tac_kaldi_mfcc_f32': (_INT, [_P, _I64, _I64, _I64, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _F, _P, _P]),
    'tac_kaldi_spectrogram_f32': (_INT, [_P, _I64, _I64, _I64, _P, _I32, _I32, _I32, _I32, _F, _F, _P, _P]),
    'tac_sliding_cmn_chunk': (_I64, [_I64, _I64, _I64, _I64, _I64]),
    'tac_sliding_cmn_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _INT, _INT, _INT, _P, _P]),
    'tac_deltas_supported': (_INT, [_I64, _I32, _I32, _INT]),
    'tac_deltas_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _I32, _I32, _INT, _P, _P]),
    'tac_mask_spans_supported': (_INT, [_I32, _I32]),
    'tac_mask_spans_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I32, _I32, _P, _F, _P, _P]),
    'tac_add_noise_tile': (_I64, []),
    'tac_add_noise_work_bytes': (_I64, [_I64, _I64]),
    'tac_add_noise_f32': (_INT, [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _P, _I64, _I32, _P, _P, _P]),
    'tac_add_noise_grad_f32': (_INT, [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _P,
                                      _I64, _I32, _P, _P, _P, _P, _P]),
    'tac_loudness_tile': (_I64, []),
    'tac_loudness_work_bytes': (_I64, [_I64, _I32, _I64, _I64, _I64]),
    'tac_loudness_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, _P]),
    'tac_pitch_max_win': (_I32, []),
    'tac_pitch_plan': (_INT, [_I64, _I32, _I32, _P, _P]),
    'tac_pitch_lags_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _I32, _I32, _I32, _P, _P]),
    'tac_pitch_smooth_i32': (_INT, [_P, _I64, _I64, _I32, _I32, _P, _P]),
    'tac_pitch_frequency_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    'tac_psd_plan': (_INT, [_I64, _P, _P]),
    'tac_beamform_grid': (_I32, [_I32, _I32]),
    'tac_psd_f32': (_INT, _SPEC + _MASK + _MASK + [_I32, _I32, _I32, _D, _I32, _P, _P, _P, _P, _P]),
    'tac_mvdr_weights_souden_f32': (_INT, [_P, _P, _I64, _I64, _I32, _P, _I64, _I32, _I32, _D, _D, _P, _P]),
    'tac_apply_beamforming_f32': (_INT, [_P, _P, _I64, _I32, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _P]),
    'tac_mvdr_souden_f32': (_INT, _SPEC + _MASK + _MASK + [_D, _P, _I64, _I32, _I32, _D, _D, _I32, _P, _P, _P, _P,
                                                           _I64, _I64, _I64, _P]),
    'tac_rtf_power_max_iter': (_I32, []),
    'tac_rtf_evd_f32': (_INT, [_P, _I64, _I64, _I32, _P, _P]),
    'tac_rtf_power_f32': (_INT, [_P, _P, _I64, _I64, _I32, _P, _I64, _I32, _I32, _I32, _D, _P, _P]),
    'tac_mvdr_weights_rtf_f32': (_INT, [_P, _P, _I64, _I64, _I32, _P, _I64, _I32, _I32, _D, _D, _P, _P]),
    'tac_rtf_mvdr_f32': (_INT, _SPEC + [_P, _P, _P, _I64, _I32, _I32, _D, _D, _P, _P, _I64, _I64, _I64, _P]),
    'tac_rnnt_max_targets': (_I32, []),
    'tac_rnnt_rows_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    'tac_rnnt_lattice_f32': (_INT, [_I64, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    'tac_rnnt_grad_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _F, _I32, _P, _P]),
    'tac_forced_align_max_targets': (_I32, []),
    'tac_forced_align_workspace': (_I64, [_I64, _I64, _I64]),
    'tac_forced_align_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I32, _P, _P, _I32, _P, _P, _P, _P]),
    'tac_griffinlim_prepare_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I64, _I64, _P, _I64, _I64, _I64, _F, _P, _P, _P]),
    'tac_griffinlim_update_f32': (_INT, [_P, _P, _P, _I64, _F, _P, _P]),
    'tac_polyphase_wide_f32': (_INT, [_P, _I64, _I64, _I64, _P, _P, _I32, _I32, _I32, _I32, _I32, _I64, _I64, _P, _P]),
    'tac_vad_plan': (_INT, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    'tac_vad_measures_f32': (_INT, [_P, _I64, _I64, _I32, _I32, _I32, _I32, _I32, _I32, _P, _F, _P, _P, _P, _P]),
    'tac_vad_decide_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I32, _I32, _I64, _I64, _I64, _F, _F, _F, _P, _P, _P]),
    'tac_vad_start_f32': (_INT, [_P, _I64, _I64, _I64, _I64, _I32, _I32, _I32, _I32, _I32, _I32, _P, _F, _P, _P, _I32, _I32, _I64, _I64,
                                 _I64, _F, _F, _F, _P, _P, _P, _P]),
    'tac_rir_limits': (_INT, [_P, _P, _P, _P]),
    'tac_rir_tile': (_INT, [_I64, _I64, _I32, _P, _P]),
    'tac_rir_ism_f32': (_INT, [_P, _P, _P, _P, _I64, _P, _P, _I64, _I64, _I32, _I32, _I64, _I32, _I64, _I64, _I32, _D, _D, _I32, _P, _P]),
    'tac_rir_span_f32': (_INT, [_P, _P, _P, _P, _I64, _I64, _I32, _I64, _I32, _D, _D, _P, _P]),
    'tac_sosfilt_max_sections': (_I32, []),
    'tac_sosfilt_tile': (_I32, []),
    'tac_sosfilt_blocks_per_cu': (_I32, []),
    'tac_sosfilt_supported': (_INT, [_P, _I32]),
    'tac_sosfilt_f32': (_INT, [_P, _I64, _I64, _I64, _P, _I32, _INT, _INT, _P, _P]),
    'tac_overdrive_tile': (_I32, []),
    'tac_overdrive_blocks_per_cu': (_I32, []),
    'tac_overdrive_supported': (_INT, [_D, _D]),
    'tac_overdrive_f32': (_INT, [_P, _I64, _I64, _I64, _D, _D, _P, _P]),
    'tac_phaser_tile': (_I32, []),
    'tac_phaser_max_delay': (_I32, []),
    'tac_phaser_seq_max_delay': (_I32, []),
    'tac_phaser_blocks_per_cu': (_I32, []),
    'tac_phaser_supported': (_INT, [_I32, _I32]),
    'tac_phaser_f32': (_INT, [_P, _I64, _I64, _I64, _P, _I32, _I32, _D, _D, _D, _P, _P]),
    'tac_phaser_seq_f32': (_INT, [_P, _I64, _I64, _I64, _P, _I32, _I32, _D, _D, _D, _P, _P]),
    'tac_flanger_tile': (_I32, []),
    'tac_flanger_chunk': (_I32, []),
    'tac_flanger_max_block': (_I32, []),
    'tac_flanger_max_delay': (_I32, []),
    'tac_flanger_blocks_per_cu': (_I32, []),
    'tac_flanger_fb_blocks_per_cu': (_I32, []),
    'tac_flanger_supported': (_INT, [_I32, _I32, _I32, _I32]),
    'tac_flanger_f32': (_INT, [_P, _I64, _I32, _I64, _I64, _P, _I32, _P, _I32, _I32, _D, _D, _D, _INT, _P, _P]),
}
EXPORTS = tuple(PROTOTYPES)


class NativeLibraryError(RuntimeError):
    pass


def build(verbose=False):
    """Compile every HIP source for gfx950 into libtac_amd.so (hipcc cross-compiles without a GPU)."""
    cmd = ['make', '-C', CSRC, '-j', str(min(8, os.cpu_count() or 1))]
    proc = subprocess.run(cmd + ['../libtac_amd.so'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or proc.returncode != 0:
        print(proc.stdout)
    if proc.returncode != 0:
        raise NativeLibraryError('building libtac_amd.so failed:\n' + proc.stdout[-4000:])
    # the compiled PyTorch binding of the hot call (host C++ against the torch headers): an accelerator of the call, ctypes
    # remains the general binding — a failure here is reported, not fatal
    proc = subprocess.run(cmd + ['ext'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or proc.returncode != 0:
        print(proc.stdout[-4000:])
    global _lib, _ext, _ext_tried
    _lib = None
    _ext, _ext_tried = None, False
    return LIB_PATH


_lib = None
_lock = threading.Lock()


def lib():
    """Load (once) and return the ctypes handle; fail loudly when the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                'libtac_amd.so not found at %s — build it with `make -C %s` (or '
                '`python -c "import __graft_entry__ as g; g.build()"`).  There is no CPU fallback.'
                % (LIB_PATH, CSRC))
        h = ctypes.CDLL(LIB_PATH)
        h.tac_abi_version.restype = ctypes.c_int
        found = h.tac_abi_version()
        if found != ABI_VERSION:
            raise NativeLibraryError(
                '%s reports ABI version %d, this binding needs %d — rebuild it with `make -C %s`'
                % (LIB_PATH, found, ABI_VERSION, CSRC))
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = h
    return _lib


EXT_PATH = os.path.join(_HERE, '_tac_ext.so')
_ext = None
_ext_tried = False


def ext():
    """The compiled PyTorch binding of the hot call (csrc/binding/tac_ext.cpp -> _tac_ext.so), or None when it is not built /
    disabled with TAC_AMD_EXT=0 / built against a different torch — ctypes then carries every call (the general binding)."""
    global _ext, _ext_tried
    if _ext_tried:
        return _ext
    with _lock:
        if _ext_tried:
            return _ext
        mod = None
        if os.environ.get('TAC_AMD_EXT', '1') != '0' and os.path.exists(EXT_PATH):
            try:
                import importlib.util
                spec = importlib.util.spec_from_file_location(__package__ + '._tac_ext', EXT_PATH)
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                if getattr(mod, 'ABI', None) != 1:
                    mod = None
            except Exception as exc:            # noqa: BLE001 — the extension is an accelerator of the call, not the product
                import warnings
                warnings.warn('torchaudio_contrib_amd: compiled binding %s not usable (%s: %s); using ctypes' %
                              (EXT_PATH, type(exc).__name__, exc))
                mod = None
        _ext = mod
        _ext_tried = True
    return _ext


def binding():
    """'compiled' when the fused chain launches through _tac_ext.so, else 'ctypes'."""
    return 'compiled' if ext() is not None else 'ctypes'


def check(rc, what):
    """Turn a TAC_E_* code into the Python exception the reference's torch ops would raise."""
    if rc == TAC_OK:
        return
    h = lib()
    msg = '%s: %s' % (what, h.tac_strerror(rc).decode())
    if rc == TAC_E_LAUNCH:
        msg += ' (hipError %d)' % h.tac_last_hip_error()
    if rc == TAC_E_UNSUPPORTED:
        raise NotImplementedError(msg)          # a RuntimeError subclass
    raise RuntimeError(msg)


def raw_stream(device):
    """hipStream_t of torch's current stream on `device` as an int (no Stream object is built)."""
    return torch._C._cuda_getCurrentRawStream(device.index)


def stream_ptr(device):
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(device.index))


class _NoGuard(object):
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def on_device(device):
    """Context manager making `device` the current HIP device for a launch — free when it already is."""
    return _NO_GUARD if torch._C._cuda_getDevice() == device.index else torch.cuda.device(device)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())
