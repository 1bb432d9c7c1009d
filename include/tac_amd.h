/* tac_amd.h — C ABI of libtac_amd.so: the MI355X (gfx950) engine behind the
 * torchaudio-contrib Melspectrogram hot path.
 *
 * The reference (keunwoochoi/torchaudio-contrib) is pure Python over stock torch ops and has
 * no FFI of its own; the boundary it exposes is its functional API
 * (torchaudio_contrib/functional.py).  Each entry point below replaces the torch-op body of
 * one (or a fused chain) of those functions; the citation names the reference lines.
 *
 * Conventions
 *   - plain C types only: raw DEVICE pointers, sizes, scalars.  No torch types.
 *   - every call is asynchronous on the caller-supplied HIP stream (`stream` is a
 *     hipStream_t passed as void*; NULL = the default stream).
 *   - outputs are caller-allocated; inputs are never written.
 *   - return value: TAC_OK (0) or a negative TAC_E_* code; tac_strerror() gives text.
 *     The only global state is an immutable, mutex-guarded twiddle-table cache keyed by
 *     (n_fft, device); the first call for a new n_fft allocates + uploads it (do that
 *     warm-up before capturing a hipGraph).
 *   - "rows" = product of all leading dims (batch x channel), functional.py:89-91.
 *   - frame-major physical layouts: complex STFT out[rows][T][F][2], spectrogram
 *     out[rows][T][F], mel out[rows][T][M].  The Python layer returns them as the logical
 *     (rows, F|M, T[,2]) strided views the reference itself produces (torch.stft /
 *     transpose-matmul-transpose give exactly these strides).
 */
#ifndef TAC_AMD_H
#define TAC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAC_OK 0
#define TAC_E_INVALID (-1)      /* bad argument (null pointer, non-positive size, ...)        */
#define TAC_E_UNSUPPORTED (-2)  /* n_fft neither a power of two in [32, 32768] nor even with a 7-smooth half, n_mels too large…  */
#define TAC_E_SHORT_INPUT (-3)  /* signal too short for the requested padding / n_fft          */
#define TAC_E_LAUNCH (-4)       /* HIP runtime error; see tac_last_hip_error()                 */

/* pad_mode values (torch.nn.functional.pad modes accepted by torch.stft, functional.py:57-58) */
#define TAC_PAD_CONSTANT 0
#define TAC_PAD_REFLECT 1
#define TAC_PAD_REPLICATE 2
#define TAC_PAD_CIRCULAR 3

const char* tac_strerror(int code);
int tac_last_hip_error(void);
int tac_abi_version(void);

/* Number of STFT frames and bins for the given geometry (0 on invalid geometry).
 * T = 1 + (L + 2*(center ? n_fft/2 : 0) - n_fft) / hop   (tests/test_functional.py:14-15). */
int64_t tac_num_frames(int64_t L, int n_fft, int hop, int center);
int tac_num_bins(int n_fft, int onesided);

/* Geometry shared by the three STFT-family entry points. */
typedef struct tac_stft_desc {
    int64_t rows;        /* batch*channel                                              */
    int64_t length;      /* samples per row (L)                                        */
    int64_t row_stride;  /* elements between consecutive rows of `wave`                */
    int32_t n_fft;       /* power of two, 32..4096; or 400 (STFT / spectrogram, one-sided); any even length <= 8192 whose half is
                            7-smooth (480, 882, 960, 1200, 1920 ...) and 8192: the STFT / spectrogram rows AND their gradient
                            (tac_stft_f32, tac_spectrogram_f32, tac_stft_backward_f32: stft_smooth.hip); 16384 / 32768: the forward
                            rows only (stft_big.hip) */
    int32_t hop;         /* > 0                                                        */
    int32_t win_length;  /* 1..n_fft; window is zero-padded centred to n_fft           */
    int32_t center;      /* 1: pad n_fft/2 both sides with pad_mode                    */
    int32_t pad_mode;    /* TAC_PAD_*                                                  */
    int32_t normalized;  /* 1: multiply by n_fft^-0.5                                  */
    int32_t onesided;    /* 1: F = n_fft/2+1, 0: F = n_fft                             */
    int32_t reserved;
} tac_stft_desc;

/* (1) functional.stft, functional.py:48-113 (the torch.stft call at :99-107).
 *     out: float[rows][T][F][2]. */
int tac_stft_f32(const float* wave, const float* window, const tac_stft_desc* d,
                 float* out, void* stream);

/* (2) Spectrogram = stft + complex_norm(power) (functional.py:116-128, layers.py:267-304),
 *     magnitude/power taken in the FFT epilogue; optionally followed by amplitude_to_db
 *     (functional.py:277-296) when db != 0.   out: float[rows][T][F]. */
int tac_spectrogram_f32(const float* wave, const float* window, const tac_stft_desc* d,
                        float power, int db, float db_ref, float db_amin,
                        float* out, void* stream);

/* (3) Melspectrogram chain fused in one kernel: stft -> complex_norm(power) ->
 *     apply_filterbank (functional.py:172-184) [-> amplitude_to_db], layers.py:307-381.
 *     fb: DEVICE float[F][n_mels] row-major dense filterbank exactly as create_mel_filter returns it
 *     (functional.py:131-169); fb_plan_host: HOST int32[2*ceil(n_mels/16)] from tac_filterbank_plan
 *     (passed to the kernel by value).  Requires onesided geometry with n_fft <= 2048 and a filterbank
 *     sparse enough for the register-resident weights (sum over 16-band tiles of ceil(range/4) <= 384
 *     at n_fft = 2048) and power in {1, 2}; returns TAC_E_UNSUPPORTED otherwise — callers then chain (2) and (4).
 *     out: float[rows][T][n_mels]. */
int tac_melspec_f32(const float* wave, const float* window, const tac_stft_desc* d, float power,
                    const float* fb, const int32_t* fb_plan_host, int32_t n_mels,
                    int db, float db_ref, float db_amin, float* out, void* stream);

/* (3b) The same fused chain with a band-sparse VALU contraction instead of the MFMA tile: every (frame, band)
 *      output is one thread's dot product over the band's contiguous bin run, weights packed in LDS.  For
 *      triangular mel banks (1.5 % non-zero) this is the faster form; tac_melbank_pack returns
 *      TAC_E_UNSUPPORTED for banks that are not band-sparse enough (sum over bands of the padded support
 *      lengths > 3072), in which case callers use (3).
 *      tac_melbank_pack: one-off per (filterbank, n_fft); copies fb to the host (synchronises `stream`), deals the
 *      bands to lane groups longest-first and uploads wpack (DEVICE float[wpack_cap >= 3072]) and desc (DEVICE
 *      int32[desc_cap >= 4096]); info_host: HOST int32[8] = {weight floats, desc stride, lane groups, max group load, 0, 0, 0, 0};
 *      for n_fft = 2048 the pack is the lane layout of the streaming kernel (lane l owns bands l, 64 + l, ...; at most
 *      256 bands): wpack = float[steps][64][2] zero-padded pair weights, desc = int32[slots][64] first bins,
 *      info_host = {weight floats, slots, 64 (+ 256 since round 6 when cell 64 s + l holds band n_mels - 1 - (64 s + l): banks whose band
 *      count is not a multiple of 64, so that their widest bands share slot 0), total steps, steps of slot 0..3}; wpack_cap >= 8192.
 *      For n_fft = 4096 (round 6: the chain in ONE launch, csrc/stft_n4096_s3.hpp; at most 256 bands, power in {1, 2}, frames 16-byte
 *      aligned, rows of at least one frame — TAC_E_UNSUPPORTED otherwise and callers chain (2) and (4b)) cells (slot, lane) of up to six
 *      slots, every slot storing the step pairs of ITS longest run: uncut, cell c is band c (or n_mels - 1 - c); where that table does
 *      not fit the LDS, bands are cut into pieces that a mix table gathers.  wpack = float[steps][64][4] (wpack_cap >= 256 * steps),
 *      desc = int32[6][64] first bins, int32[6] step pairs per slot, 10 ints of padding, int32[rounds][pieces][64] mix (desc_cap >=
 *      400 + 64 * rounds * pieces), info_host = {weight floats, slots, 1000 + 4096, total steps, waves per workgroup the table leaves
 *      room for (12 / 11 / 8), pieces per band in the mix table (0: uncut), rounds of 64 bands, uncut cells in reversed band order};
 *      TAC_E_UNSUPPORTED when no layout fits the LDS beside eight waves (dense banks).
 *      tac_melbank_plan_pieces_host (a host tool, no device access): the PIECE layout of round 4 for a host copy of the bank —
 *      a lane runs three segments of L0 / L1 / L2 four-tap steps, each holding a piece of a band; a band takes up to three
 *      pieces in adjacent lanes; 12 steps instead of 18 for the standard 128-band bank.  seg_steps int32[3]; first / band /
 *      index int32[192]; weights float[weights_cap >= 256 * (L0 + L1 + L2)]; TAC_E_UNSUPPORTED when no segment triple fits.
 *      The kernel form that contracted this layout measured 3 - 5 % slower than the lane layout and is not shipped
 *      (tools/ablation/README.md); tests emulate its contraction on the plan.
 *      n_fft = TAC_PACK_PAIRS_2048 (both pack functions; n_freqs = 1025, exactly 128 bands): the PAIR layout of the fft_length-2048
 *      kernel, float32 samples only (tac_melspec_sparse_f32; the coded entry point answers TAC_E_INVALID).  Every lane runs three segments
 *      of A, B, C four-tap steps: band l; band 64 + l (lanes >= 32: its first B quads); lanes >= 32 the next C quads of band 64 + l,
 *      lanes < 32 the quads of band 96 + l behind those, whose sum the kernel hands to lane l + 32.  14 steps instead of 4 + 14 for
 *      the standard 16 kHz bank.  wpack = float[A + B + C][64][4], desc = int32[3][64] first bins (multiples of four), followed by
 *      the classic table of the same bank (weights at wpack + info[0], first bins at desc + 192) for the kernel forms that do not
 *      contract pairs; wpack_cap >= 256 * (A + B + C + 20), desc_cap >= 320.  info_host = {256 (A + B + C), 3, 64 + 512, A + B + C,
 *      A, B, C, steps of the classic slot 1}.  TAC_E_UNSUPPORTED for banks outside the instantiated shapes (4, 6, 4), (4, 7, 3),
 *      (3, 7, 5), and for banks whose classic table is not the (4, 14) / (4, 16) one of the unrolled kernels: callers then pack with
 *      n_fft = 2048.  The code means the pair layout since the revision that introduced melspec_stream3_kernel<..., PA, PC> (ABI version 5,
 *      no symbol added); -2048 selected round 4's piece layout until round 5, and libraries between the two answer it with
 *      TAC_E_UNSUPPORTED, which callers treat like any refused bank. */
#define TAC_PACK_PAIRS_2048 (-2048)
int tac_melbank_pack(const float* fb, int32_t n_freqs, int32_t n_mels, int32_t n_fft, float* wpack,
                     int32_t wpack_cap, int32_t* desc, int32_t desc_cap, int32_t* info_host, void* stream);
/* ... the same tables without a device (round 6; n_fft = 256, 400, 512, 1024, 2048 or 4096): fb_host, wpack_host, desc_host are HOST buffers, nothing is launched
 *      or copied — what tests/test_host_api.py emulates the kernels' contraction on. */
int tac_melbank_pack_host(const float* fb_host, int32_t n_freqs, int32_t n_mels, int32_t n_fft, float* wpack_host,
                          int32_t wpack_cap, int32_t* desc_host, int32_t desc_cap, int32_t* info_host);
int tac_melbank_plan_pieces_host(const float* fb_host, int32_t n_freqs, int32_t n_mels, int32_t* seg_steps, int32_t* first,
                                 int32_t* band, int32_t* index, float* weights, int32_t weights_cap);
int tac_melspec_sparse_f32(const float* wave, const float* window, const tac_stft_desc* d, float power,
                           const float* wpack, const int32_t* desc, const int32_t* info_host, int32_t n_mels,
                           int db, float db_ref, float db_amin, float* out, void* stream);

/* (3c) The fused chain reading the waveform in its stored sample format (the step before the path —
 *      PCM / mu-law decode, functional.py:338-354 — folded into the frame load, the samples are converted in registers):
 *      TAC_SAMPLES_I16 = int16 PCM, value = sample * 2^-15; TAC_SAMPLES_MULAW_U8 / _I64 = 8-bit mu-law codes stored as
 *      uint8 / int64 (what mu_law_encoding returns), value = decode_lut[code & 255] with decode_lut the DEVICE float[256]
 *      table of (8).  d->row_stride and d->length count samples.  Served by the fft_length 2048 streaming kernel and, for
 *      power 2, by the fft_length 256 / 400 / 512 / 1024 kernels; TAC_E_UNSUPPORTED otherwise (callers then convert with (8) /
 *      tac_pcm16_to_f32 and use (3b)). */
#define TAC_SAMPLES_F32 0
#define TAC_SAMPLES_I16 1
#define TAC_SAMPLES_MULAW_U8 2
#define TAC_SAMPLES_MULAW_I64 3
int tac_melspec_sparse_coded_f32(const void* samples, int32_t sample_format, const float* decode_lut,
                                 const float* window, const tac_stft_desc* d, float power, const float* wpack,
                                 const int32_t* desc, const int32_t* info_host, int32_t n_mels, int db,
                                 float db_ref, float db_amin, float* out, void* stream);
/* int16 PCM -> float32 (x * 2^-15), for the kernels without a coded frame load */
int tac_pcm16_to_f32(const int16_t* x, int64_t n, float* out, void* stream);

/* TAC_OK when (3) can run this geometry + filterbank plan, TAC_E_UNSUPPORTED when it cannot
 * (no launch, no device access). */
int tac_melspec_supported(const tac_stft_desc* d, float power, const int32_t* fb_plan_host,
                          int32_t n_mels);

/* Per 16-band tile [first, last+1) non-zero bin range of a dense filterbank, computed by a device
 * kernel into plan (DEVICE int32[2*ceil(n_mels/16)]).  When plan_host is non-NULL the stream is
 * synchronised and the plan is also copied there (one-off per filterbank). */
int tac_filterbank_plan(const float* fb, int32_t n_freqs, int32_t n_mels, int32_t* plan,
                        int32_t* plan_host, void* stream);

/* (4) functional.apply_filterbank, functional.py:172-184: out[r][t][m] = sum_f spec[r][f][t]*fb[f][m]
 *     as an fp32 MFMA (v_mfma_f32_32x32x2_f32) tile with zero-block skipping driven by fb_plan
 *     (NULL = dense).  spec element (r, f, t) lives at spec[r*stride_r + f*stride_f + t*stride_t].
 *     out: float[rows][T][n_mels]. */
int tac_apply_filterbank_f32(const float* spec, int64_t rows, int32_t n_freqs, int64_t n_frames,
                             int64_t stride_r, int64_t stride_f, int64_t stride_t,
                             const float* fb, const int32_t* fb_plan, int32_t n_mels,
                             float* out, void* stream);

/* (4b) functional.apply_filterbank for a frame-major spectrogram (the bins of a frame contiguous, frames stride_t
 *      floats apart — the layout the kernels of this library write) and a band-sparse bank packed with
 *      tac_melbank_pack(fb, n_freqs, n_mels, n_fft = 0, ...): streams the spectrogram once and runs the fused
 *      kernel's contraction.  out: frame-major [rows][n_frames][n_mels]. */
int tac_apply_filterbank_sparse_f32(const float* spec, int64_t rows, int32_t n_freqs, int64_t n_frames,
                                    int64_t stride_r, int64_t stride_t, const float* wpack,
                                    const int32_t* desc, const int32_t* info_host, int32_t n_mels,
                                    float* out, void* stream);
/* ... followed by functional.amplitude_to_db (db != 0: 10 (log10(max(x^2, db_amin)) - log10 db_ref)) in the same pass: the
 *      filterbank + dB tail of Melspectrogram -> AmplitudeToDb for a spectrogram that already exists (the chain from the waveform
 *      is one launch of (3b) up to fft_length 4096). */
int tac_apply_filterbank_sparse_db_f32(const float* spec, int64_t rows, int32_t n_freqs, int64_t n_frames,
                                       int64_t stride_r, int64_t stride_t, const float* wpack, const int32_t* desc,
                                       const int32_t* info_host, int32_t n_mels, int db, float db_ref, float db_amin,
                                       float* out, void* stream);

/* (5) functional.complex_norm, functional.py:116-128: out[i] = |(x[2i], x[2i+1])|^power. */
int tac_complex_norm_f32(const float* x, int64_t n, float power, float* out, void* stream);

/* (5b) functional.angle / functional.magphase, functional.py:187-201: phase[i] =
 *      atan2(x[2i+1], x[2i]); when mag != NULL also mag[i] = |(x[2i], x[2i+1])|^power, in the same pass. */
int tac_magphase_f32(const float* x, int64_t n, float power, float* mag, float* phase, void* stream);

/* (5c) functional.phase_vocoder, functional.py:204-274.  spec: rows x n_freqs x n_frames complex
 *      pairs with arbitrary element strides (in floats; the pair itself contiguous); phase_advance: n_freqs floats;
 *      idx0/idx1/alpha (device, n_out each): for output frame i the two source frames floor(t_i), floor(t_i + 1)
 *      (indices >= n_frames are the reference's zero padding) and the weight t_i mod 1, with t = arange(0, n_frames,
 *      rate) evaluated the way the reference evaluates it (functional.py:233-237).  out: frame-major
 *      [rows][n_out][n_freqs][2]. */
int tac_phase_vocoder_f32(const float* spec, int64_t rows, int32_t n_freqs, int64_t n_frames,
                          int64_t stride_r, int64_t stride_f, int64_t stride_t,
                          const float* phase_advance, const int32_t* idx0, const int32_t* idx1,
                          const float* alpha, int64_t n_out, float* out, void* stream);
/*      The float32 recurrence as written is ill-conditioned (which is why the reference's own test runs in float64,
 *      tests/test_functional.py:69-116); the _f32 kernel carries exp(i phase) as a unit phasor instead of the running sum (only
 *      the sum modulo one turn reaches the output) and agrees with the float64 evaluation to ~1e-6 rad; the _f64 entry point
 *      is that float64 call site itself: same arguments with double data (strides in doubles), the formula as written. */
int tac_phase_vocoder_f64(const double* spec, int64_t rows, int32_t n_freqs, int64_t n_frames,
                          int64_t stride_r, int64_t stride_f, int64_t stride_t,
                          const double* phase_advance, const int32_t* idx0, const int32_t* idx1,
                          const double* alpha, int64_t n_out, double* out, void* stream);
/* ... and its gradient with respect to the spectrogram (round 6; float32): grad_out [rows][n_out][n_freqs][2] and grad_spec
 *      [rows][n_frames][n_freqs][2] frame-major and dense, grad_spec ZERO-INITIALISED by the caller (the kernel accumulates: a source frame
 *      is read by several output frames when rate < 1, by none when rate > 2); spec, strides and the grid (idx0, idx1, alpha) as in the
 *      forward call.  The gradient with respect to phase_advance is zero (the wrap and the advance cancel). */
int tac_phase_vocoder_backward_f32(const float* spec, int64_t rows, int32_t n_freqs, int64_t n_frames, int64_t stride_r,
                                   int64_t stride_f, int64_t stride_t, const int32_t* idx0, const int32_t* idx1, const float* alpha,
                                   int64_t n_out, const float* grad_out, float* grad_spec, void* stream);

/* (5d) STFT -> TimeStretch -> ComplexNorm on magnitudes alone (stretch.hip).  complex_norm(phase_vocoder(X), power) is
 *      (alpha |X[t1]| + (1 - alpha) |X[t0]|)^power whatever the phases are — the running phase, phase_advance, the wrap and the
 *      cumulative sum cancel — so the chain is tac_spectrogram_f32(power = 1) followed by one of these.
 *      mag: float[rows][n_frames][n_freqs] magnitudes, frame-major (bins contiguous; stride_t floats between frames, stride_r
 *      between rows) — what tac_spectrogram_f32 writes with power = 1.  idx0 / alpha (device, n_out each): the first source frame
 *      and the weight of the second (idx0 + 1) per output frame, the grid of tac_phase_vocoder_f32; source frames >= n_frames are
 *      the reference's zero padding.  out[r][j][f] = (alpha[j] mag[r][idx0[j]+1][f] + (1 - alpha[j]) mag[r][idx0[j]][f])^power,
 *      followed by amplitude_to_db when db != 0 (db_ref / db_amin as in tac_spectrogram_f32).   out: float[rows][n_out][n_freqs].
 *      Non-finite input looks like the reference: a NaN source value makes every LATER output frame of its bin NaN (the reference's
 *      cumulative phase), an infinite one only the frames interpolated from it.  flags: a caller-provided WORKSPACE of `rows`
 *      int32 (device; contents on entry ignored, undefined afterwards) in which the kernel notes the first affected frame per row;
 *      a second, near-empty launch rewrites what lies behind it. */
int tac_stretch_norm_f32(const float* mag, int64_t rows, int32_t n_freqs, int64_t n_frames, int64_t stride_r, int64_t stride_t,
                         const int32_t* idx0, const float* alpha, int64_t n_out, float power, int db, float db_ref, float db_amin,
                         float* out, int32_t* flags, void* stream);
/* ... with apply_filterbank (and amplitude_to_db when db != 0) in the same launch: the interpolated, powered row is built in LDS
 *      and contracted with the band-sparse bank packed by tac_melbank_pack(..., n_fft = 0, ...).   out: float[rows][n_out][n_mels].
 *      A non-finite bin makes its whole frame NaN, as the reference's dense matmul does.  TAC_E_UNSUPPORTED for a pack in the tile
 *      layout or a bank outside 8..128 bands: callers then chain tac_stretch_norm_f32 and tac_apply_filterbank_*_f32. */
int tac_stretch_mel_f32(const float* mag, int64_t rows, int32_t n_freqs, int64_t n_frames, int64_t stride_r, int64_t stride_t,
                        const int32_t* idx0, const float* alpha, int64_t n_out, float power, const float* wpack, const int32_t* desc,
                        const int32_t* info_host, int32_t n_mels, int db, float db_ref, float db_amin, float* out, int32_t* flags,
                        void* stream);
/* ... and the gradient of tac_stretch_norm_f32 (db = 0) with respect to mag, as a gather per source frame: bounds (device,
 *      n_frames + 1 int32) holds bounds[t] = number of output frames with idx0 < t, so the outputs that read frame t are
 *      [bounds[t - 1], bounds[t + 1]).  grad_out: float[rows][n_out][n_freqs], grad_mag: float[rows][n_frames][n_freqs], both dense;
 *      every element of grad_mag is written (no zero-initialisation, no atomics: bit-reproducible). */
int tac_stretch_norm_backward_f32(const float* mag, int64_t rows, int32_t n_freqs, int64_t n_frames, int64_t stride_r,
                                  int64_t stride_t, const int32_t* idx0, const float* alpha, const int32_t* bounds, int64_t n_out,
                                  float power, const float* grad_out, float* grad_mag, void* stream);

/* (1d)-(6d) The path in float64 (the reference keeps f64 -> f64: functional.py:48-113, :116-128, :172-184, :187-201,
 *      :277-314).  Same argument meaning as the _f32 entry points with double data; d->n_fft: any even length <= 8192 whose
 *      half is 5-smooth (N/2-point mixed-radix complex Stockham transform per workgroup in LDS), or any other length
 *      <= 4096 (direct O(N^2) transform per frame: meant for short odd sizes, see _hip64.py for the sizes Python routes there);
 *      tac_apply_filterbank_f64 takes the dense bank (no plan) and optionally applies amplitude_to_db to its result;
 *      tac_magphase_f64: mag and / or phase may be NULL (complex_norm / angle alone). */
int tac_stft_f64(const double* wave, const double* window, const tac_stft_desc* d, double* out, void* stream);
int tac_spectrogram_f64(const double* wave, const double* window, const tac_stft_desc* d, double power, int db,
                        double db_ref, double db_amin, double* out, void* stream);
int tac_apply_filterbank_f64(const double* spec, int64_t rows, int32_t n_freqs, int64_t n_frames, int64_t stride_r,
                             int64_t stride_f, int64_t stride_t, const double* fb, int32_t n_mels, int db,
                             double db_ref, double db_amin, double* out, void* stream);
int tac_magphase_f64(const double* z, int64_t n, double power, double* mag, double* phase, void* stream);
int tac_amplitude_to_db_f64(const double* x, int64_t n, double ref, double amin, double* out, void* stream);
int tac_db_to_amplitude_f64(const double* x, int64_t n, double ref, double* out, void* stream);

/* (6) functional.amplitude_to_db, functional.py:277-296: 10*(log10(max(x^2, amin)) - log10(ref)). */
int tac_amplitude_to_db_f32(const float* x, int64_t n, float ref, float amin, float* out,
                            void* stream);

/* (6b) functional.db_to_amplitude, functional.py:299-314: (10^(x/10 + log10 ref))^0.5. */
int tac_db_to_amplitude_f32(const float* x, int64_t n, float ref, float* out, void* stream);

/* (7) functional.mu_law_encoding, functional.py:317-335.  out: int64 codes.
 *     thresholds (optional, device): int32[n_pos + n_neg] magnitude bit patterns at which the
 *     reference's code changes for x >= 0 (ascending, first n_pos) and x <= 0 (next n_neg);
 *     they are a fast path for |x| <= 1 (a table search instead of the logarithm).  Without them,
 *     and for |x| > 1 / NaN, the closed form is evaluated with the reference CPU path's exact
 *     float32 roundings; either way the codes are bit-identical to the reference's.
 *     zero_code = code of x == 0. */
int tac_mulaw_encode_f32_i64(const float* x, int64_t n, int32_t n_quantize,
                             const int32_t* thresholds, int32_t n_pos, int32_t n_neg,
                             int32_t zero_code, int64_t* out, void* stream);

/* (8) functional.mu_law_decoding, functional.py:338-354, for int64 codes.  lut (optional,
 *     device): float[n_quantize] table used for codes in [0, n_quantize); codes outside it
 *     (or lut == NULL) go through the closed form. */
int tac_mulaw_decode_i64_f32(const int64_t* codes, int64_t n, int32_t n_quantize,
                             const float* lut, float* out, void* stream);

/* (8b) same for float-valued codes (the reference accepts float input, functional.py:349, and its own test
 *      bit-compares that form, tests/test_functional.py:182-193): a code that is an exact integer in
 *      [0, n_quantize) is decoded through lut (optional, device, float[n_quantize]) like (8); everything else
 *      through the closed form. */
int tac_mulaw_decode_f32_f32(const float* codes, int64_t n, int32_t n_quantize, const float* lut,
                             float* out, void* stream);
/*      float64 (round 5): the same formulas evaluated in double, as the reference's CPU path does for double input
 *      (functional.py:329-335, 349-354); codes as int64 (codes_are_i64 != 0) or double. */
int tac_mulaw_encode_f64_i64(const double* x, int64_t n, int32_t n_quantize, int64_t* out, void* stream);
int tac_mulaw_decode_f64(const void* codes, int32_t codes_are_i64, int64_t n, int32_t n_quantize, double* out, void* stream);

/* (9) Gradients (the reference differentiates through stock torch ops).  All asynchronous on `stream`,
 *     caller-allocated outputs, float32, the frame-major layouts of the forward entry points.
 *     tac_stft_backward_f32: adjoint of (1) up to the overlap-add: grad_spec[rows][T][F][2] (one-sided) ->
 *       grad_frames[rows][T][n_fft] = window[n] * scale * Re sum_k grad_spec[k] e^{+2 pi i k n / n_fft}  (one inverse
 *       real FFT per frame on the same wave-level FFT as the forward pass; the even lengths with a 7-smooth half of (1): the
 *       generic Stockham passes of stft_smooth.hip, which also serve fft_length 8192; not 16384 / 32768).
 *     tac_stft_norm_backward_f32: the same with the gradient spectrum formed on load from the spectrum itself,
 *       spec[rows][T][F][2], and the gradient of |spec|^power, grad_norm[rows][T][F] (the adjoint of
 *       functional.py:116-128 folded in: Spectrogram's backward in one pass, no gradient spectrum in memory).
 *     tac_spectrogram_backward_f32: the same with NO spectrum in memory: the frame is re-read from the waveform
 *       (wave / d exactly as given to (2)), transformed again in the kernel, and the spectrum values the norm's adjoint
 *       needs are formed from the FFT's exchange area while the inverse's operands are gathered.
 *     tac_spectrogram_backward_ola_f32: the whole adjoint of (2) — tac_spectrogram_backward_f32 + tac_overlap_add_f32 —
 *       for fft_length 256 / 512 / 1024 / 2048 with a hop that is a multiple of fft_length / 16, and fft_length 400 with
 *       50 <= hop <= 400 and hop, centre padding multiples of 4 (TAC_E_UNSUPPORTED otherwise): every wave walks runs of consecutive frames and keeps their overlap-add in LDS, so no frame gradients
 *       exist in memory.  `workspace`
 *       (device) must hold tac_spectrogram_backward_ola_workspace(d) bytes (that call returns a negative TAC_E_* code
 *       for geometries the form does not cover); grad_wave[r][j] at grad_wave + r * grad_row_stride + j.
 *     tac_melspectrogram_backward_ola_f32: the same for the mel chain (layers.py:333-339, functional.py:183-184): `grad_mel`
 *       is the gradient of the (linear) mel values, (rows, n_frames, n_mels) frame-major, and the filterbank stage's adjoint
 *       — two multiply-adds per bin through the table of tac_filterbank_adjoint_pack — is formed inside the kernel, per
 *       frame: the gradient of the power spectrogram never exists in memory.  fft_length 2048 (n_mels <= 256), 512 / 1024 (hop = N/8, N/4, N/2) and 400
 *       (n_mels <= 128), banks with at most two non-zero weights per bin; TAC_E_UNSUPPORTED otherwise (callers then run tac_apply_filterbank_adjoint_f32 +
 *       tac_spectrogram_backward_ola_f32).  Same workspace as tac_spectrogram_backward_ola_f32.
 *     tac_overlap_add_f32: adjoint of framing + padding: grad_wave[r][j] = sum of grad_frames over every (frame, tap)
 *       that read sample j, reflect / replicate / circular images included (a gather: deterministic, no atomics).
 *     tac_complex_norm_backward_f32: grad_z[i] = grad_out[i] * power * |z_i|^(power-2) * z_i (0 where z_i == 0),
 *       functional.py:126-128.
 *     tac_amplitude_to_db_backward_f32: grad_x = grad_out * 20 / (ln 10 * x) where x^2 >= amin, else 0
 *       (NaN where x is NaN), functional.py:291-296.
 *     tac_magphase_backward_f32 (round 6): gradient of magphase / angle (functional.py:187-201): grad_z[i] = grad_mag[i] * power *
 *       |z_i|^(power-2) * z_i + grad_phase[i] * (-im_i, re_i) / |z_i|^2, 0 where z_i == 0; grad_mag or grad_phase may be NULL.
 *     tac_db_to_amplitude_backward_f32 (round 6): grad_x = grad_out * ln(10) / 20 * (10^(x/10 + log10 ref))^0.5, functional.py:299-314.
 *     The filterbank stage's adjoint is (4) with the transposed matrix — or, for banks with at most two non-zero
 *     weights per bin (every triangular mel bank), tac_apply_filterbank_adjoint_f32: grad_spec[i][f] = w0[f] *
 *     grad_mel[i][band0[f]] + w1[f] * grad_mel[i][band1[f]] over i < rows*T frame-major rows, with the per-bin table
 *     built on the device by tac_filterbank_adjoint_pack (table: 16 * n_freqs + 16 bytes, device; *max_nonzeros_host
 *     receives the non-zero count of the fullest bin — the table is only valid when that is <= 2; synchronous). */
int tac_stft_backward_f32(const float* grad_spec, const float* window, const tac_stft_desc* d,
                          float* grad_frames, void* stream);
int tac_stft_norm_backward_f32(const float* spec, const float* grad_norm, float power, const float* window,
                               const tac_stft_desc* d, float* grad_frames, void* stream);
int tac_spectrogram_backward_f32(const float* wave, const float* window, const tac_stft_desc* d,
                                 const float* grad_norm, float power, float* grad_frames, void* stream);
int64_t tac_spectrogram_backward_ola_workspace(const tac_stft_desc* d);
int tac_spectrogram_backward_ola_f32(const float* wave, const float* window, const tac_stft_desc* d,
                                     const float* grad_norm, float power, void* workspace, int64_t workspace_bytes,
                                     float* grad_wave, int64_t grad_row_stride, void* stream);
int tac_melspectrogram_backward_ola_f32(const float* wave, const float* window, const tac_stft_desc* d,
                                        const float* grad_mel, int32_t n_mels, const void* adjoint_table,
                                        int32_t n_freqs, float power, void* workspace, int64_t workspace_bytes,
                                        float* grad_wave, int64_t grad_row_stride, void* stream);
/* fft_length 400 (frame gradients through memory, then tac_overlap_add_f32): tac_spectrogram_backward_f32 with the filterbank
 * adjoint of the mel chain formed inside the kernel from grad_mel (rows, n_frames, n_mels <= 128) and the
 * tac_filterbank_adjoint_pack table; TAC_E_UNSUPPORTED for other sizes. */
int tac_melspectrogram_backward_f32(const float* wave, const float* window, const tac_stft_desc* d,
                                    const float* grad_mel, int32_t n_mels, const void* adjoint_table, int32_t n_freqs,
                                    float power, float* grad_frames, void* stream);
int tac_filterbank_adjoint_pack(const float* fb, int32_t n_freqs, int32_t n_mels, void* table,
                                int32_t* max_nonzeros_host, void* stream);
int tac_apply_filterbank_adjoint_f32(const float* grad_mel, int64_t rows_times_frames, int32_t n_mels,
                                     const void* table, int32_t n_freqs, float* grad_spec, void* stream);
int tac_overlap_add_f32(const float* grad_frames, const tac_stft_desc* d, float* grad_wave,
                        int64_t grad_row_stride, void* stream);
int tac_complex_norm_backward_f32(const float* z, const float* grad_out, int64_t n, float power,
                                  float* grad_z, void* stream);
/* (9b) The general gradient routes (every fft_length, two-sided outputs, gradients of the window and the filterbank —
 *     functional.py:99-107, 183-184 differentiate through every argument):
 *     tac_overlap_add_f32 above takes ANY fft_length (framing only).
 *     tac_fold_twosided_f32: gradient of a two-sided output grad[frames][n_fft][width] (width 2: complex pairs, 1: |X|^p)
 *       folded onto the n_fft/2+1 one-sided bins: out[k] = grad[k] + grad[n_fft-k] (imaginary parts: minus).
 *     tac_window_grad_partials / tac_window_grad_f32: with grad_frames_unwindowed[rows][T][n_fft] the gradient w.r.t.
 *       the windowed frames (tac_stft_backward_f32 run with a window of ones), partial[p][n] = the sum over the p-th
 *       chunk of (row, frame) of grad_frames * padded signal; tac_sum_slabs_f32 adds the n_partials rows up.
 *     tac_sum_slabs_f32: out[i] = sum_s x[s][i] in slab order. */
int tac_fold_twosided_f32(const float* grad, int64_t n_frames_total, int32_t n_fft, int32_t width, float* out,
                          void* stream);
int64_t tac_window_grad_partials(const tac_stft_desc* d);
int tac_window_grad_f32(const float* grad_frames_unwindowed, const float* wave, const tac_stft_desc* d,
                        float* partial, int64_t n_partials, void* stream);
int tac_sum_slabs_f32(const float* x, int64_t n_slabs, int64_t slab_elems, float* out, void* stream);
int tac_amplitude_to_db_backward_f32(const float* x, const float* grad_out, int64_t n, float amin,
                                     float* grad_x, void* stream);
int tac_magphase_backward_f32(const float* z, const float* grad_mag, const float* grad_phase, int64_t n, float power,
                              float* grad_z, void* stream);
int tac_db_to_amplitude_backward_f32(const float* x, const float* grad_out, int64_t n, float ref, float* grad_x, void* stream);

/* (10) hpss, beta_hpss.py:35-127: median-filter harmonic / percussive separation of a magnitude
 *      spectrogram.  mag element (r, f, t) at mag[r*stride_r + f*stride_f + t*stride_t]; the four outputs use the same
 *      strides.  kernel_f (percussive filter, along frequency) and kernel_t (harmonic filter, along time) odd, <= 63
 *      (TAC_E_UNSUPPORTED above; equal widths 9 ... 31 are one launch, every other combination two);
 *      reflect padding (needs kernel/2 < size: TAC_E_SHORT_INPUT otherwise); masks soft ((h+eps)/(h+p+eps), eps 1e-6) or
 *      hard (1.0 / 0.0); harm / perc may both be NULL (masks only).  The outputs must not overlap mag or one another
 *      (the two-launch route parks the first launch's medians in mask_perc): overlapping address ranges are
 *      refused with TAC_E_INVALID.  The test is conservative: it compares the whole address SPANS of the five tensors (first to last
 *      element touched), so interleaved outputs that never share an element — channel slices of one stacked buffer — are refused
 *      as well, and it is skipped when a stride is negative. */
int tac_hpss_f32(const float* mag, int64_t rows, int32_t n_freqs, int32_t n_frames, int64_t stride_r,
                 int64_t stride_f, int64_t stride_t, int32_t kernel_f, int32_t kernel_t, float power,
                 int hard, float* harm, float* perc, float* mask_harm, float* mask_perc, void* stream);
/* ... and its gradient with respect to mag (round 6): the four incoming gradients (each may be NULL) and grad_mag use mag's strides;
 *      grad_mag ZERO-INITIALISED by the caller (the kernel scatters with float atomics: the gradient of a median goes to the element it
 *      selected; the sum order, hence the last bits, are not reproducible from run to run).  hard != 0: the masks are not differentiable,
 *      only harm = mag * mask / perc = mag * mask are. */
int tac_hpss_backward_f32(const float* mag, int64_t rows, int32_t n_freqs, int32_t n_frames, int64_t stride_r, int64_t stride_f,
                          int64_t stride_t, int32_t kernel_f, int32_t kernel_t, float power, int hard, const float* grad_harm,
                          const float* grad_perc, const float* grad_mask_harm, const float* grad_mask_perc, float* grad_mag,
                          void* stream);

/* (11) Diagnostics (bench.py's roofline object; no effect on results).
 *      tac_last_route: name of the kernel instantiation the calling thread's last fused-chain launch (3b / 3c at fft_length
 *        2048) or last fft_length-2048 STFT / spectrogram launch (1, 2: "stft_ring3_kernel<...>" / "stft_stream3_kernel<...>"; fft_length >= 8192: "stft_big_kernel<...>") took, as rocprofv3 prints it, e.g. "melspec_stream3_kernel<1024, 16, true, 0, 14, 12>" ("" before any).
 *      tac_debug_clock_probe: while `buf` (DEVICE uint64[2 * capacity_pairs]) is set for the calling thread, every workgroup
 *        b < capacity_pairs of those launches records buf[2b] = shader cycles (s_memtime) and buf[2b + 1] = ticks of the
 *        100 MHz constant clock (s_memrealtime) its wave 0 spent in the frame loop: cycles / ticks x 100 MHz is the shader
 *        clock the kernel actually ran at.  NULL clears it.  Four scalar instructions and one 16-byte store per workgroup. */
const char* tac_last_route(void);
int tac_debug_clock_probe(uint64_t* buf, int32_t capacity_pairs);

/* (12) Route selection of the fft_length-2048 kernels (process-wide; results agree to float32 rounding, ~2e-7 of a frame's
 *      largest bin): where the 1024-point transform of a frame runs.  mode 0 = VALU (radix 16 . 16 . 4 through the LDS,
 *      melspec_stream3_kernel / stft_ring3_kernel: rounds 3 - 5), 1 = matrix pipe (two chained 32 x 32 complex DFT products on
 *      v_mfma_f32_32x32x16_f16 with fp16 hi / lo operand pairs, melspec_mfma_kernel: round 6), -1 = the default (environment
 *      TAC_FFT_PIPE=valu|mfma, else the build's default).  Returns the previous mode. */
int tac_set_fft_pipe(int mode);

/* (13) Inverse STFT (what torch.istft computes for the one-sided layout (1) writes): out[r][i] = num[i + pad] / env[i + pad],
 *      num the overlap-add of window * irfft(X_t) (times sqrt(n_fft) when d->normalized), env the overlap-add of window^2,
 *      pad = n_fft / 2 when d->center.  In `d`, `length` is the number of samples to WRITE per row (positions pad .. pad + length of the
 *      hop (T - 1) + n_fft padded ones, as torch.istft slices them; zeros past the last) and `row_stride` the row stride of `out`; pad_mode is ignored.
 *      Geometries: every n_fft tac_stft_backward_f32 takes (powers of two 32 .. 4096, 400, even lengths with a 7-smooth half,
 *      8192), one-sided; TAC_E_UNSUPPORTED otherwise.
 *      tac_istft_workspace: bytes of scratch tac_istft_f32 needs (the windowed frames, float[rows][T][n_fft]); 0 where the fused
 *      one-launch route takes the geometry (n_fft 2048, hop 256 / 512 / 1024, center, row_stride a multiple of 4: call
 *      tac_istft_f32 with workspace = NULL; a workspace of rows * T * n_fft floats selects the two-launch route instead);
 *      negative = TAC_E_*.
 *      tac_istft_envelope_f32: inv_env[p] = 1 / env[p] (and env[p] itself when `env` is not NULL) for the hop (T - 1) + n_fft
 *      padded positions; a function of the window and the geometry only — callers cache it and check min env (the NOLA
 *      condition of torch.istft) once.
 *      tac_istft_f32: spec is frame-major, the F pairs of a frame contiguous, stride_t floats between frames and stride_r
 *      between rows — dense rows only (stride_t == 2 F, stride_r == T stride_t: what (1) and the phase vocoder write),
 *      TAC_E_UNSUPPORTED for any other layout.  Two launches: the frame kernels of tac_stft_backward_f32 in their inverse operand
 *      mode, then a gather that writes every output element once.  tac_last_route() names the route.
 *      tac_istft_grad_input_f32 / tac_istft_grad_bins_f32: the two elementwise halves of the gradient w.r.t. spec around
 *      tac_stft_f32 (center = 0 on `padded`): padded[r][p] = grad_out[r][p - pad] * inv_env[p] inside the kept range, else 0
 *      (float[rows][hop (T - 1) + n_fft]; d as for tac_istft_f32, grad_stride the row stride of grad_out); then in place
 *      spec[frame][k] *= 2 s (0 < k < n_fft / 2), (s, 0) for the DC and Nyquist bins, s = (normalized ? sqrt(n_fft) : 1) / n_fft. */
int64_t tac_istft_workspace(const tac_stft_desc* d, int64_t n_frames);
int tac_istft_envelope_f32(const float* window, const tac_stft_desc* d, int64_t n_frames, float* inv_env, float* env,
                           void* stream);
int tac_istft_f32(const float* spec, int64_t stride_r, int64_t stride_t, int64_t n_frames, const float* window,
                  const float* inv_env, const tac_stft_desc* d, void* workspace, int64_t workspace_bytes, float* out,
                  void* stream);
int tac_istft_grad_input_f32(const float* grad_out, int64_t grad_stride, const float* inv_env, const tac_stft_desc* d,
                             int64_t n_frames, float* padded, void* stream);
int tac_istft_grad_bins_f32(float* spec, int64_t n_frames_total, int n_fft, int normalized, void* stream);

/* (14) functional.dct (the DCT-II of MFCC behind Melspectrogram -> AmplitudeToDb, and its adjoint with the transposed matrix):
 *      out[r][t][c] = sum_m x[r][m][t]*mat[m][c], every sum one fused multiply-add chain in ascending m — one launch, each
 *      output written once, no atomics, bit-identical from run to run; non-finite values propagate as in a dense matmul.
 *      x element (r, m, t) lives at x[r*stride_r + m*stride_m + t*stride_t], any positive strides: frame-major rows
 *      (stride_m == 1: what the mel kernels write; 16-byte loads where x and the strides are 16-byte multiples and n_in a
 *      multiple of 4) and time-contiguous rows (stride_t == 1) are read coalesced.  mat: DEVICE float[n_in][n_out], held in
 *      the LDS: 1 <= n_in, n_out <= 256 and n_in * n_out <= 32768, TAC_E_UNSUPPORTED (nothing launched) otherwise.
 *      out: float[rows][T][n_out]. */
int tac_dct_rows_f32(const float* x, int64_t rows, int32_t n_in, int64_t n_frames,
                     int64_t stride_r, int64_t stride_m, int64_t stride_t,
                     const float* mat, int32_t n_out, float* out, void* stream);

/* (15) functional.resample (polyphase windowed-sinc resampling, and its adjoint with the transposed bank):
 *      y[r][j*phases + p] = sum_{k < run[p]} bank[k][p] * x[r][j*step + off[p] + k]   for 0 <= j*phases + p < l_out,
 *      x[r][i] = x[r*stride_r + i], taken as zero outside 0 <= i < l_in; out: float[rows][l_out], dense.  One launch, each output
 *      one fused multiply-add chain over k ascending, written once: no atomics, bit-identical from run to run.  Taps behind a
 *      phase's run are never multiplied: a non-finite input sample reaches exactly the outputs whose run covers it.
 *      bank: DEVICE float[taps][phases] (tap-major), zero behind each run; table: DEVICE int32[2][phases] = off[], run[] with
 *      off_min <= off[p] <= off_max (may be negative) and taps_min <= run[p] <= taps — values outside are clamped, so a wrong
 *      table gives wrong sums, never an access outside the tile.  Forward: phases = new, step = orig; gradient: phases = orig,
 *      step = new.  The bank and one tile's input span live in the LDS: phases <= 2048, phases * taps <= 20480
 *      (RESAMPLE_MAX_BANK) and 256 outputs' span <= 14336 floats, TAC_E_UNSUPPORTED (nothing launched) otherwise.
 *      16-byte loads where x and stride_r are 16-byte multiples, float loads otherwise. */
int tac_polyphase_f32(const float* x, int64_t rows, int64_t l_in, int64_t stride_r, const float* bank, const int32_t* table,
                      int32_t phases, int32_t taps, int32_t taps_min, int32_t step, int32_t off_min, int32_t off_max,
                      int64_t l_out, float* out, void* stream);

/* (16) functional.lfilter (and biquad, the cookbook biquads, preemphasis, deemphasis): a recursive filter of order <= 2 along a row,
 *      a0 y[n] = sum_{k < n_coeffs} b[k] x[n-k] - sum_{1 <= k < n_coeffs} a[k] y[n-k],   zero initial state,
 *      x[r][i] = x[r*stride_r + i], 0 <= i < length; out: float[rows][length], dense.  b, a: HOST double[n_coeffs], n_coeffs 1..3,
 *      a[0] != 0 (TAC_E_INVALID otherwise; n_coeffs > 3 is TAC_E_UNSUPPORTED).  reverse != 0 runs the same filter from the END of
 *      each row towards its start — the adjoint, i.e. the gradient w.r.t. x.  clamp != 0 limits the result to [-1, 1].
 *      One launch, no workspace, no atomics, one writer per element, bit-identical from run to run; a row is walked by one workgroup
 *      in tiles of 1024 * tac_lfilter_chunk() samples and no workgroup waits on another.  Loads and stores are float32; the
 *      recursion, its state and the scan that joins the lanes' chunks are float64 (coefficients are divided by a[0] in float64).
 *      A non-finite sample reaches the samples after it (before it, with reverse) in its own row, and nothing else.
 *      16-byte loads where x and stride_r are 16-byte multiples, float loads otherwise.
 *      tac_lfilter_supported: TAC_OK where tac_lfilter_f32 takes these coefficients; TAC_E_UNSUPPORTED also for a filter so
 *      unstable that the largest matrix of the scan, M^(512 chunk), overflows float64 (nothing is launched for those). */
int32_t tac_lfilter_chunk(void);
int tac_lfilter_supported(const double* b, const double* a, int32_t n_coeffs);
int tac_lfilter_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const double* b, const double* a,
                    int32_t n_coeffs, int clamp, int reverse, float* out, void* stream);

/* (17) functional.fftconvolve / convolve: uniformly partitioned overlap-save on (1) and the frame kernels of (13), and the kernel
 *      between them.  B = n_fft / 2, F = B + 1, P = ceil(m / B) partitions, n_fft one of 2048 / 4096 / 8192.
 *      tac_spectral_mac_f32 (the frequency-domain delay line):
 *        Y[r][t][f] = sum_{p = 0 .. min(P-1, t)} X[r][t-p][f] * H[hrow(r)][p][f]     (complex, f < n_bins)
 *      X, Y: float[rows][T][n_bins][2] frame-major (what (1) writes and (13) reads), H: float[h_rows][P][n_bins][2]; hrow: DEVICE
 *      int32[rows] (values are clamped to 0 .. h_rows - 1), NULL = every row uses kernel 0; conj != 0 multiplies by conj(H).
 *      One launch; a lane owns one bin of one row over tac_spectral_mac_tile(P) consecutive frames.  The real and the imaginary part
 *      of an output are each ONE fused multiply-add chain in ascending p (x_r h_r, then -x_i h_i; x_r h_i, then x_i h_r); frames
 *      with t - p < 0 are neither read nor multiplied; one writer per output, no atomics, no workspace, no LDS: bit-identical from
 *      run to run.  P <= 16: H_p of the bin and a ring of the last frames of X in registers (instantiations for P <= 4 / 8 / 16);
 *      16 < P <= 64: H streamed.  P > 64: TAC_E_UNSUPPORTED, nothing launched.  X, H, Y 8-byte aligned.
 *      tac_fftconvolve_spectra_f32: H[hr][p] = the n_fft-point one-sided transform of [y[hr][p B .. (p+1) B) | B zeros] (y read from
 *        its END when reverse != 0: the kernel of the gradient w.r.t. x); y[hr][i] = y[hr*stride_r + i], i < m.  A function of y and
 *        n_fft only: callers cache it.  workspace: tac_fftconvolve_spectra_workspace(h_rows, m, n_fft) bytes, 16-byte aligned.
 *      tac_fftconvolve_f32: out[r][j] = full[r][j + offset], j < l_out, full = x[r] * y[hrow(r)] of l_in + m - 1 samples
 *        (offset + l_out <= l_in + m - 1); x[r][i] = x[r*stride_r + i] (any alignment), out[r][j] = out[r*out_stride + j].
 *        Five steps per chunk of rows: padded copy, (1) at hop B with a window of ones, tac_spectral_mac_f32, the frame kernels of
 *        (13) in inverse mode, and a gather of the kept second halves (never the discarded halves: a non-finite sample of input
 *        block b reaches output blocks b .. b + P of its row and nothing else).  workspace: tac_fftconvolve_workspace(...) bytes
 *        (16-byte aligned) — the padded copy, X and Y (the inverse's frames reuse X) for as many rows as fit under 1 GiB; the entry
 *        point walks the rows in chunks of what the workspace it is given holds (any size from one row's need up).
 *        tac_fftconvolve_supported: TAC_OK, or TAC_E_UNSUPPORTED for P > 64, another n_fft, 32-bit overflow or a row beyond 1 GiB.
 *        tac_fftconvolve_default_n_fft: the smallest n_fft with P <= 8, else 8192.
 *      tac_fftconvolve_direct_f32: the same result for ONE short shared kernel through (15) with one phase at step 1: bank = DEVICE
 *        float[m], the kernel from its end; table = DEVICE int32[2] = {offset - (m - 1), m}.
 *      tac_last_route() names the route: "spectral-2048" / "spectral-4096" / "spectral-8192" / "direct". */
int32_t tac_spectral_mac_tile(int32_t n_parts);
int tac_spectral_mac_f32(const float* X, const float* H, const int32_t* hrow, int64_t rows, int64_t n_frames, int32_t n_bins,
                         int32_t n_parts, int32_t h_rows, int conj, float* Y, void* stream);
int32_t tac_fftconvolve_default_n_fft(int64_t m);
int tac_fftconvolve_supported(int64_t l_in, int64_t m, int32_t n_fft);
int64_t tac_fftconvolve_spectra_workspace(int64_t h_rows, int64_t m, int32_t n_fft);
int tac_fftconvolve_spectra_f32(const float* y, int64_t h_rows, int64_t m, int64_t stride_r, int32_t n_fft, int reverse,
                                void* workspace, int64_t workspace_bytes, float* H, void* stream);
int64_t tac_fftconvolve_workspace(int64_t rows, int64_t l_in, int64_t m, int32_t n_fft, int64_t offset, int64_t l_out);
int tac_fftconvolve_f32(const float* x, int64_t rows, int64_t l_in, int64_t stride_r, const float* H, const int32_t* hrow,
                        int32_t h_rows, int64_t m, int32_t n_fft, int conj, int64_t offset, int64_t l_out, void* workspace,
                        int64_t workspace_bytes, float* out, int64_t out_stride, void* stream);
int tac_fftconvolve_direct_f32(const float* x, int64_t rows, int64_t l_in, int64_t stride_r, const float* bank, const int32_t* table,
                               int64_t m, int64_t offset, int64_t l_out, float* out, void* stream);

/* (18) functional.kaldi_fbank (torchaudio.compliance.kaldi.fbank): waveform rows to log mel rows in ONE launch (csrc/kaldi_fbank.hip).
 *      W = win_length, S = shift, N = n_fft (256 / 512 / 1024, W <= N), eps = 2^-23.
 *      tac_kaldi_num_frames: T = (length < W ? 0 : 1 + (length - W) / S) with snip_edges, else (length + S / 2) / S.
 *      Frame t of row r is x[r*stride_r + j], j = t S - pad .. t S - pad + W: pad = 0 with snip_edges; otherwise pad = W/2 - S/2 and
 *      the row is mirrored at both ends (j < 0 reads x[-j - 1], j >= length reads x[2 length - 1 - j]; length >= W, else
 *      TAC_E_UNSUPPORTED).  Per frame, in this order: the mean is subtracted (TAC_KALDI_REMOVE_DC); e = log max(sum f^2, eps)
 *      (TAC_KALDI_RAW_ENERGY); f[i] -= preemph * f[i-1] with f[-1] := f[0] (preemph != 0); f *= window (DEVICE float[W]); e as above
 *      on the windowed frame (no TAC_KALDI_RAW_ENERGY); zero-padding on the right to N; P = |rfft f|^2 (TAC_KALDI_POWER) or |rfft f|;
 *      out[b] = sum_k bank[b][k] P[k], then log max(., eps) (TAC_KALDI_LOG).  e = max(e, log energy_floor) where energy_floor > 0.
 *      The bank is band-sparse: table = DEVICE int32[3][n_mels] = {first bin, bins, offset into weights} per band, weights = DEVICE
 *      float[w_total] (w_total <= 4096), each band's run of consecutive bins; a run is clamped to bins 0 .. N/2 - 1 (the Nyquist
 *      bin is never read) and to the weights.  4 <= n_mels <= 128.
 *      out: float[rows][T][n_mels + 1 or 0], dense; with TAC_KALDI_USE_ENERGY e is column 0, or the last column with TAC_KALDI_HTK.
 *      A wave owns 8 / 4 / 2 consecutive frames: their one contiguous span of samples is staged in the LDS with coalesced loads (any
 *      row alignment, any shift), mean and energy are reductions over the frame's N / 32 lanes, every output element is ONE fused
 *      multiply-add chain over its band's bins in ascending order.  One writer per element, no atomics, no workspace: bit-identical
 *      from run to run.  A non-finite sample makes exactly the frames whose W samples contain it non-finite.  Another n_fft, W > N,
 *      n_mels outside 4 .. 128: TAC_E_UNSUPPORTED, nothing launched. */
#define TAC_KALDI_SNIP_EDGES 1
#define TAC_KALDI_REMOVE_DC 2
#define TAC_KALDI_RAW_ENERGY 4
#define TAC_KALDI_USE_ENERGY 8
#define TAC_KALDI_HTK 16
#define TAC_KALDI_LOG 32
#define TAC_KALDI_POWER 64
int64_t tac_kaldi_num_frames(int64_t length, int32_t win_length, int32_t shift, int snip_edges);
int tac_kaldi_fbank_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const float* window, const float* weights,
                        const int32_t* table, int32_t n_fft, int32_t win_length, int32_t shift, int32_t n_mels, int32_t w_total,
                        int32_t flags, float preemph, float energy_floor, float* out, void* stream);

/* (18b) functional.kaldi_mfcc / kaldi_spectrogram (torchaudio.compliance.kaldi.mfcc / .spectrogram): epilogues of the launch of (18),
 *      everything up to the power row P[k] = |rfft f|^2, k <= N/2, as there (same arguments, same flags, same eps).
 *      tac_kaldi_spectrogram_f32: out: float[rows][T][N/2 + 1]; out[k] = log max(P[k], eps) for k = 1 .. N/2, the Nyquist bin
 *      included; out[0] = e, the log energy of (18).  No bank.  TAC_KALDI_POWER, _LOG and _USE_ENERGY are implied, _HTK is ignored.
 *      tac_kaldi_mfcc_f32: out: float[rows][T][n_ceps], 1 <= n_ceps <= n_mels.  L[b] = log max(sum_k bank[b][k] P[k], eps) (the row of
 *      (18) with TAC_KALDI_LOG | TAC_KALDI_POWER, which are implied) stays in the LDS; C[c] = sum_b L[b] dct[b][c] is ONE fused
 *      multiply-add chain over b ascending.  dct = DEVICE float[n_mels][n_ceps]: the caller's DCT-II matrix with the lifter (and
 *      the sqrt 2 of HTK's C0) folded in.  With TAC_KALDI_USE_ENERGY C[0] := e; with TAC_KALDI_HTK the columns are stored as
 *      [C1 .. C_{n_ceps - 1}, C0].  A NaN in L reaches every coefficient of its frame and no other frame.
 *      The matrix shares the launch's 64 KB of LDS with the waves' areas, the window and the packed bank:
 *      tac_kaldi_mfcc_table_limit(n_fft, n_mels, w_total) is the largest n_mels * n_ceps a launch takes (0: arguments outside (18));
 *      beyond it TAC_E_UNSUPPORTED, nothing launched.  One writer per element, no atomics: bit-identical from run to run. */
int64_t tac_kaldi_mfcc_table_limit(int32_t n_fft, int32_t n_mels, int32_t w_total);
int tac_kaldi_mfcc_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const float* window, const float* weights,
                       const int32_t* table, const float* dct, int32_t n_fft, int32_t win_length, int32_t shift, int32_t n_mels,
                       int32_t w_total, int32_t n_ceps, int32_t flags, float preemph, float energy_floor, float* out, void* stream);
int tac_kaldi_spectrogram_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const float* window, int32_t n_fft,
                              int32_t win_length, int32_t shift, int32_t flags, float preemph, float energy_floor, float* out,
                              void* stream);

/* (19) functional.sliding_window_cmn (Kaldi's apply-cmvn-sliding): ONE launch over x[r*stride_r + t*stride_t + f*stride_f], r < rows,
 *      t < n_frames = T, f < n_feats = F (strides in elements, positive for every axis longer than one), out: float[rows][T][F], dense
 *      (csrc/cmn_deltas.hip).  W = cmn_window >= 1, M = min_cmn_window >= 1.  The window of frame t is [ws, we), n = we - ws:
 *        center:      ws = min(max(t - W/2, 0), max(T - W, 0)), we = min(ws + W, T)
 *        otherwise:   ws = max(t - W, 0), we = max(t + 1, M); where we > T: ws = max(ws - (we - T), 0), we = T   (W + 1 frames away
 *                     from the ends, as in Kaldi)
 *      out[t][f] = x[t][f] - mean(x[ws:we][f]); with norm_vars times (sum(x^2)/n - mean^2)^-1/2, and 0 where n == 1.
 *      Lanes run along f; a thread owns one feature over tac_sliding_cmn_chunk(rows, T, F, W, M) consecutive frames: it sums the
 *      window of its first frame directly and then moves both ends frame by frame.  The sums are float64 over the FINITE samples of
 *      the window, beside an integer count of the non-finite ones: a NaN or an infinity makes exactly the frames whose window holds it
 *      NaN.  The subtraction and the variance are float64, rounded to float32 once.  One writer per element, no atomics, no
 *      workspace: bit-identical from run to run.
 *      adjoint != 0 (norm_vars == 0 only, else TAC_E_UNSUPPORTED): x is grad_out and out[s] = x[s] - sum over {t : ws(t) <= s < we(t)}
 *      of x[t] / n(t), the gradient w.r.t. the input: the same sliding sum over the interval of frames whose window holds s.
 *      W and M may be any positive int64 (a window beyond the row is the row: they are capped before any sum is formed).
 *      More than 2^31 - 1 workgroups, T > 2^40: TAC_E_UNSUPPORTED, nothing launched. */
int64_t tac_sliding_cmn_chunk(int64_t rows, int64_t n_frames, int64_t n_feats, int64_t cmn_window, int64_t min_cmn_window);
int tac_sliding_cmn_f32(const float* x, int64_t rows, int64_t n_frames, int64_t n_feats, int64_t stride_r, int64_t stride_t,
                        int64_t stride_f, int64_t cmn_window, int64_t min_cmn_window, int center, int norm_vars, int adjoint,
                        float* out, void* stream);

/* (20) functional.compute_deltas: ONE launch over x[r*stride_r + f*stride_f + t*stride_t] (strides in elements, positive for every axis
 *      longer than one), out: float[rows][F][T], dense (csrc/cmn_deltas.hip).  n = (win_length - 1) / 2, denom = n (n + 1)(2n + 1) / 3:
 *        out[t] = (sum_{k = -n .. n} k x[idx(t + k)]) / denom
 *      idx is the index map of torch.nn.functional.pad: TAC_DELTAS_REPLICATE (clamp), _CONSTANT (zero outside), _REFLECT (no edge
 *      repeat, n < T) or _CIRCULAR (n <= T).  Each output is ONE fused multiply-add chain in ascending k and one division.  A
 *      workgroup stages its tile and the 2n frames around it in the LDS: with stride_t == 1 lanes load along t; with stride_f == 1
 *      (the transposed view of a (T, F) matrix) lanes load along f and the tile is turned in the LDS; the stores are along t either
 *      way.  Every other layout takes the first form.  Bit-identical from run to run.
 *      adjoint != 0 (_REPLICATE and _CONSTANT): x is grad_out and out the gradient w.r.t. the input: the taps negated over a
 *      zero-padded row, and for _REPLICATE what the clamped reads sent to s = 0 and s = T - 1 (those two in float64).
 *      tac_deltas_supported: TAC_OK; TAC_E_INVALID for win_length < 3, an unknown mode or a row too short for the mode;
 *      TAC_E_UNSUPPORTED for n > 32 (win_length > 66) and for the adjoint of the other two modes.  Nothing is launched for those. */
#define TAC_DELTAS_REPLICATE 0
#define TAC_DELTAS_CONSTANT 1
#define TAC_DELTAS_REFLECT 2
#define TAC_DELTAS_CIRCULAR 3
int tac_deltas_supported(int64_t n_frames, int32_t win_length, int32_t mode, int adjoint);
int tac_deltas_f32(const float* x, int64_t rows, int64_t n_feats, int64_t n_frames, int64_t stride_r, int64_t stride_f,
                   int64_t stride_t, int32_t win_length, int32_t mode, int adjoint, float* out, void* stream);

/* (21) SpecAugment's masks (functional.mask_along_axis / mask_along_axis_iid, TimeMasking, FrequencyMasking, SpecAugment): EVERY
 *      mask of a call in ONE launch over x[r*stride_r + a*stride_a + b*stride_b], r < rows, a < n_a = A, b < n_b = B (strides in
 *      elements, positive for every axis longer than one), out: float[rows][A][B], dense (csrc/specaug.hip).
 *      spans = DEVICE int32[span_rows][k_a + k_b][2]; span_rows is rows, or 1 for one table shared by every row.  The first k_a
 *      spans run along A, the other k_b along B; a span is [start, end), clamped to its axis by the kernel whatever the table
 *      holds, and empty where end <= start.  spans may be NULL where k_a + k_b == 0 (a dense copy).
 *        out[a][b] = fill      if an A-span of the row holds a or a B-span of the row holds b
 *                  = x[a][b]   otherwise
 *      fill = *value_ptr where value_ptr (DEVICE float) is given, else the immediate value.  The fill is selected, not multiplied
 *      in, and a masked element is not loaded: a NaN under a mask does not reach the output.
 *      Lanes run along b in 16-byte chunks where x has unit stride there, B % 4 == 0 and base and strides keep the chunks
 *      aligned; in dwords otherwise.  Where x has its unit stride along a (the transposed view of a (T, F) matrix) a 64 x 64 tile
 *      is loaded along a, turned in the LDS and stored along b.  A persistent grid of at most 32 workgroups per CU walks the units
 *      (row, A-block, B-chunk); a unit's spans become bit masks in the LDS once per unit.  One writer per element, no atomics:
 *      bit-identical from run to run.
 *      tac_mask_spans_supported: TAC_OK; TAC_E_INVALID for a negative count; TAC_E_UNSUPPORTED for k_a + k_b > TAC_MASK_MAX_SPANS.
 *      Nothing is launched for those. */
#define TAC_MASK_MAX_SPANS 64
int tac_mask_spans_supported(int32_t k_a, int32_t k_b);
int tac_mask_spans_f32(const float* x, int64_t rows, int64_t n_a, int64_t n_b, int64_t stride_r, int64_t stride_a, int64_t stride_b,
                       const int32_t* spans, int64_t span_rows, int32_t k_a, int32_t k_b, const float* value_ptr, float value,
                       float* out, void* stream);

/* (22) functional.add_noise / AddNoise: noise mixed into a waveform at a signal-to-noise ratio, and its gradient
 *      (csrc/add_noise.hip).  Row r = o * rows_inner + i (r < rows, rows_inner divides rows) of waveform starts at
 *      o * w_stride_o + i * w_stride_r and sample t lies t * w_stride_t behind it; noise likewise (strides in floats: the time
 *      strides positive, the others >= 0 — one noise row may serve every row, or one per batch entry its rows_inner channels);
 *      out: float[rows][length], dense.
 *      snr = DEVICE float[snr_rows], lengths = DEVICE int32 / int64 (lengths_i64) [length_rows] or NULL (every row whole); snr_rows
 *      and length_rows are rows or 1.  With m_t = t < lengths[r] (clamped to [0, length]):
 *        E_s = sum_t (waveform_t m_t)^2,  E_n = sum_t (noise_t m_t)^2,  scale = sqrt(E_s / E_n) 10^(-snr / 20)     in float64
 *        out_t = fma((float)scale, noise_t, waveform_t)   for every t < length
 *      Samples at or behind lengths[r] are not loaded by the sums; E_s = 0 gives scale 0, E_n = 0 inf, both NaN.  Three launches on
 *      the stream, no host wait: per-tile float64 partial sums (a tile = tac_add_noise_tile() samples of a row, a persistent grid
 *      of at most 32 workgroups per CU), a wave per row that sums them in a fixed order, and the mix over the same tiles.  No
 *      atomics: bit-identical from run to run.  16-byte accesses where unit time strides, bases, the other strides and length % 4
 *      allow.
 *      work: DEVICE scratch of tac_add_noise_work_bytes(rows, length) bytes, 8-byte aligned (0 for sizes the kernels do not take:
 *      rows * tiles beyond 2^31 - 1, for which the launchers return TAC_E_UNSUPPORTED); nothing in it has to be initialised.
 *      tac_add_noise_grad_f32: with d = sum_t grad_out_t noise_t over all t,
 *        grad_waveform_t = grad_out_t + (scale / E_s) d waveform_t m_t
 *        grad_noise_t    = scale grad_out_t - (scale / E_n) d noise_t m_t
 *        grad_snr        = -(ln 10 / 20) scale d                 float[rows]
 *      by the same three launches in adjoint mode (both tensor gradients in one pass, dense over rows); each of the three may be
 *      NULL. */
int64_t tac_add_noise_tile(void);
int64_t tac_add_noise_work_bytes(int64_t rows, int64_t length);
int tac_add_noise_f32(const float* waveform, int64_t w_stride_o, int64_t w_stride_r, int64_t w_stride_t, const float* noise,
                      int64_t n_stride_o, int64_t n_stride_r, int64_t n_stride_t, int64_t rows, int64_t rows_inner, int64_t length,
                      const float* snr, int64_t snr_rows, const void* lengths, int64_t length_rows, int32_t lengths_i64, void* work,
                      float* out, void* stream);
int tac_add_noise_grad_f32(const float* grad_out, int64_t g_stride_o, int64_t g_stride_r, int64_t g_stride_t, const float* waveform,
                           int64_t w_stride_o, int64_t w_stride_r, int64_t w_stride_t, const float* noise, int64_t n_stride_o,
                           int64_t n_stride_r, int64_t n_stride_t, int64_t rows, int64_t rows_inner, int64_t length, const float* snr,
                           int64_t snr_rows, const void* lengths, int64_t length_rows, int32_t lengths_i64, void* work,
                           float* grad_waveform, float* grad_noise, float* grad_snr, void* stream);

/* (23) functional.loudness / Loudness: ITU-R BS.1770-4 gated loudness in LKFS (csrc/loudness.hip).  waveform: `entries` batch entries
 *      of `channels` (1 .. 5) rows of `length` samples, unit time stride; channel c of entry e starts at e * stride_b + c * stride_c
 *      (strides in floats, positive where the count exceeds 1).  coeffs = HOST double[12]: b[3], a[3] of the K-weighting's shelf,
 *      then b[3], a[3] of its high-pass (a[0] != 0; normalised here).  gate and step are the block length and hop in samples; the
 *      kernels take gate == 4 * step with step >= 16 (TAC_E_UNSUPPORTED otherwise) and length >= gate (TAC_E_SHORT_INPUT).  With nb =
 *      (length - gate) / step + 1 blocks:
 *        w = clip(highpass(clip(shelf(x))))           float64 recursions, each clipped to [-1, 1] in float64, never stored
 *        E[c][k] = sum of w^2 over [k step, k step + gate) / gate,   l_k = -0.691 + 10 log10 sum_c g_c E[c][k],  g = (1, 1, 1, 1.41, 1.41)
 *        out[e] = the level of the mean E over the blocks with l_k > -70 and l_k > (the level of the mean over l_k > -70) - 10
 *      all in float64, rounded to float32 once; NaN where no block is left.  Two launches on the stream, no host wait: a workgroup
 *      per row walks it in tiles of tac_loudness_tile() samples (state, and the sum of a bin of `step` samples that a tile boundary
 *      cuts, carried from tile to tile; a persistent grid of one workgroup per CU) and writes the row's nb + 3 bin sums; a wave per
 *      entry gates and reduces.  No atomics, one writer per element: bit-identical from run to run.  Samples behind the last block are
 *      not read.
 *      work: DEVICE scratch of tac_loudness_work_bytes(entries, channels, length, gate, step) bytes, 8-byte aligned (0 for what the
 *      kernels do not take); nothing in it has to be initialised, every double of it is written.  out: float[entries]. */
int64_t tac_loudness_tile(void);
int64_t tac_loudness_work_bytes(int64_t entries, int32_t channels, int64_t length, int64_t gate, int64_t step);
int tac_loudness_f32(const float* waveform, int64_t entries, int32_t channels, int64_t length, int64_t stride_b, int64_t stride_c,
                     int64_t gate, int64_t step, const double* coeffs, void* work, float* out, void* stream);

/* (24) functional.detect_pitch_frequency / PitchFrequency: torchaudio's NCCF pitch (csrc/pitch.hip).  waveform: n0 * n1 rows of `time`
 *      samples; row r starts at (r / n1) * stride_0 + (r % n1) * stride_1 and its samples are stride_t apart (strides in floats,
 *      positive where the count exceeds 1; any alignment).  With F = frame, L = max_lag, N = ceil(time / F) frames and the row
 *      continued by zeros:
 *        nccf[t][l] = (s1 . s2) / (1e-9 + |s1|)^2 / (1e-9 + |s2|)^2,  s1 = x[tF : tF + F], s2 = x[tF + l : tF + l + F],  l = 1 .. L
 *        lag[t] = ch if nccf[t][ch] > 0.99 nccf[t][cb] else cb,  cb / ch the first arg-max over l in [lag_min + 1, L] / [lag_min + 1, L / 2]
 *        out[k] = sample_rate / lower median of padded[k : k + win_length],  padded = (win_length - 1) / 2 copies of lag[0], then lag
 *      with N + (win_length - 1) / 2 - win_length + 1 outputs a row (TAC_E_SHORT_INPUT if that is below 1).  lag_min >= 1 and
 *      lag_min < L / 2 (TAC_E_INVALID otherwise).  Products and their sums are float32 in a fixed order, the energies of s2 come from
 *      a float64 prefix of squares; the (frames, lags) matrix stays in registers and the LDS.  A frame whose F + L samples hold a NaN
 *      or Inf gets some lag in [lag_min + 1, L]; no other frame is touched by it.  An all-zero frame gets lag_min + 1.
 *      tac_pitch_lags_f32 is the first launch alone (lags: int32[n0 * n1][N]), tac_pitch_smooth_i32 the second (win_length 1 ..
 *      tac_pitch_max_win(), TAC_E_UNSUPPORTED beyond), tac_pitch_frequency_f32 both on the stream: no host wait, no atomics, one
 *      writer per element, bit-identical from run to run.  `lags` is DEVICE scratch of n0 * n1 * N int32 there, all of it written.
 *      tac_pitch_plan: the frames a workgroup of the first launch takes together (*group) and its LDS bytes, or TAC_E_UNSUPPORTED
 *      where the F + L samples of a single frame do not fit the LDS plan (64 KB); the launchers return the same. */
int32_t tac_pitch_max_win(void);
int tac_pitch_plan(int64_t n_frames, int32_t frame, int32_t max_lag, int32_t* group, int32_t* lds_bytes);
int tac_pitch_lags_f32(const float* waveform, int64_t n0, int64_t n1, int64_t time, int64_t stride_0, int64_t stride_1, int64_t stride_t,
                       int32_t frame, int32_t max_lag, int32_t lag_min, int32_t* lags, void* stream);
int tac_pitch_smooth_i32(const int32_t* lags, int64_t rows, int64_t n_frames, int32_t win_length, int32_t sample_rate, float* out,
                         void* stream);
int tac_pitch_frequency_f32(const float* waveform, int64_t n0, int64_t n1, int64_t time, int64_t stride_0, int64_t stride_1,
                            int64_t stride_t, int32_t sample_rate, int32_t frame, int32_t max_lag, int32_t lag_min, int32_t win_length,
                            int32_t* lags, float* out, void* stream);

/* (25) functional.psd / mvdr_weights_souden / apply_beamforming and the MVDR layer: torchaudio's mask-based Souden MVDR beamformer
 *      (csrc/beamform.hip).  spec: complex pairs X[b][c][f][t][2] of `batch` entries, `channels` (2 .. 8), `bins` and `frames`, read
 *      where they lie: the four strides are in floats, positive and even, the pair itself contiguous and the base 8-byte aligned
 *      (TAC_E_INVALID otherwise).  A lane owns one system g = b * bins + f; frame-major spectrograms (stride_f = 2) load coalesced.
 *      Masks are real [b][f][t] with three positive strides in floats: a unit time stride is staged through the LDS, any other is
 *      read directly.
 *
 *      tac_psd_f32: psd[g][c][e] = sum_t m'[t] X[c][t] conj(X[e][t]), m' = 1 (mask_a NULL), m (normalize 0) or m / (sum_t m + eps).
 *      n_psd 2 forms a second PSD in the same pass over spec, from mask_b, or from 1 - mask_a where `complement` is set (mask_b
 *      ignored).  Time is cut into `chunks` pieces of 64 frames (tac_psd_plan: the cut depends on `frames` alone, so a system's
 *      result does not depend on the rest of the batch); launch 1 leaves per piece
 *      float32 sums part[n_psd][chunks][channels^2][batch * bins] and float64 mask sums msum[n_psd][chunks][batch * bins] — both
 *      DEVICE scratch, all of it written — and launch 2 adds the pieces in ascending order in float64, normalises in float64,
 *      rounds once and stores both triangles from one value (Hermitian to the bit; imaginary diagonal +0).  No atomics; bit-identical
 *      from run to run.  psd_a / psd_b: float32 [batch * bins][channels][channels][2].
 *
 *      tac_mvdr_weights_souden_f32: per system, in float64 from the float32 PSDs: psd_n += (diag_eps * Re tr psd_n + 1e-8) I where
 *      diagonal_loading; N = psd_n^-1 psd_s by elimination with partial pivoting; W = N / (tr N + eps); w = W[:, ref_channel], or
 *      w = sum_c W[:, c] u[c] with u = ref_vector[b * ref_stride_b + c] (float32 on the DEVICE) where ref_vector is not NULL.
 *      Rounded to float32 once: weights[batch * bins][channels][2].
 *
 *      tac_apply_beamforming_f32: out[b][f][t] = sum_c conj(w[g][c]) X[b][c][f][t], one fused multiply-add chain over c; out is
 *      pairs with strides out_b / out_f / out_t in floats (frame-major: out_f = 2, out_t = 2 * bins).
 *
 *      tac_mvdr_souden_f32: launch 1 of tac_psd_f32 with two masks (normalize on, eps = psd_eps), the weights launch reading the
 *      pieces (it sums them exactly as launch 2 would), then the apply launch: three launches on the stream, no host wait, the
 *      same bits as the three entries called one after the other.  `weights` is an output too. */
int tac_psd_plan(int64_t frames, int32_t* chunk_frames, int32_t* chunks);
int32_t tac_beamform_grid(int32_t which, int32_t cus);   /* most workgroups of launch `which` (0 psd, 1 apply) on `cus` CUs (<= 0: this device's) */
int tac_psd_f32(const float* spec, int64_t batch, int32_t channels, int64_t bins, int64_t frames, int64_t stride_b, int64_t stride_c,
                int64_t stride_f, int64_t stride_t, const float* mask_a, int64_t a_stride_b, int64_t a_stride_f, int64_t a_stride_t,
                const float* mask_b, int64_t b_stride_b, int64_t b_stride_f, int64_t b_stride_t, int32_t n_psd, int32_t complement,
                int32_t normalize, double eps, int32_t chunks, float* part, double* msum, float* psd_a, float* psd_b, void* stream);
int tac_mvdr_weights_souden_f32(const float* psd_s, const float* psd_n, int64_t batch, int64_t bins, int32_t channels,
                                const float* ref_vector, int64_t ref_stride_b, int32_t ref_channel, int32_t diagonal_loading,
                                double diag_eps, double eps, float* weights, void* stream);
int tac_apply_beamforming_f32(const float* weights, const float* spec, int64_t batch, int32_t channels, int64_t bins, int64_t frames,
                              int64_t stride_b, int64_t stride_c, int64_t stride_f, int64_t stride_t, float* out, int64_t out_b,
                              int64_t out_f, int64_t out_t, void* stream);
int tac_mvdr_souden_f32(const float* spec, int64_t batch, int32_t channels, int64_t bins, int64_t frames, int64_t stride_b,
                        int64_t stride_c, int64_t stride_f, int64_t stride_t, const float* mask_s, int64_t s_stride_b,
                        int64_t s_stride_f, int64_t s_stride_t, const float* mask_n, int64_t n_stride_b, int64_t n_stride_f,
                        int64_t n_stride_t, double psd_eps, const float* ref_vector, int64_t ref_stride_b, int32_t ref_channel,
                        int32_t diagonal_loading, double diag_eps, double eps, int32_t chunks, float* part, double* msum,
                        float* weights, float* out, int64_t out_b, int64_t out_f, int64_t out_t, void* stream);

/* (26) functional.rtf_evd / rtf_power / mvdr_weights_rtf and the RTFMVDR layer: the relative-transfer-function (steering vector)
 *      half of torchaudio's beamforming (csrc/beamform.hip).  Systems, PSDs, weights, ref_vector / ref_stride_b / ref_channel,
 *      diagonal loading and the channel counts (2 .. 8) are those of (25); an RTF is float32 [batch * bins][channels][2].  Every
 *      entry below is ONE launch: float32 in, float64 on chip, one rounding per output.  A system's result depends on that system
 *      alone (the same bits whatever else is in the batch, and from run to run); non-finite input ends in NaNs for its system only.
 *      tac_rtf_power_f32 and tac_mvdr_weights_rtf_f32 take 16 systems a workgroup with a lane per system, as the Souden weights do.
 *
 *      tac_rtf_evd_f32: the eigenvector of the largest eigenvalue of the Hermitian psd_s (its lower triangle is read, the imaginary
 *      diagonal ignored), by Jacobi rotations in round-robin order, a group of 2, 4 or 8 lanes per system with a row of the matrix
 *      and of the eigenvectors per lane — at most 16 sweeps, left once the off-diagonal Frobenius norm is below 1e-16 of the
 *      diagonal's — at unit 2-norm, with the phase that makes the component of largest modulus (lowest index on a tie) real and
 *      positive (its imaginary part is +0).  Needs no spectral gap: psd_s = 0 or I gives the first unit vector.
 *
 *      tac_rtf_power_f32: psd_n loaded where diagonal_loading; phi = psd_n^-1 psd_s by elimination with partial pivoting;
 *      r = phi[:, ref_channel] or phi u; n_iter >= 2: n_iter - 2 times r <- phi r, then r <- psd_s r; n_iter == 1: r <- psd_n r with
 *      the loaded psd_n.  Not normalised.  n_iter < 1: TAC_E_INVALID; above tac_rtf_power_max_iter() (64): TAC_E_UNSUPPORTED.
 *
 *      tac_mvdr_weights_rtf_f32: a = psd_n^-1 rtf with the loaded psd_n; w = a / (Re rtf^H a + eps); then w *= conj(rtf[ref_channel]),
 *      or w *= sum_c conj(rtf[c]) u[c] where ref_vector is not NULL; ref_channel < 0 without a vector: no scaling.
 *
 *      tac_rtf_mvdr_f32: the launch of tac_mvdr_weights_rtf_f32, then the apply launch of (25) on spec: two launches on the stream,
 *      the bits of the two entries called one after the other.  `weights` is an output too. */
int32_t tac_rtf_power_max_iter(void);
int tac_rtf_evd_f32(const float* psd_s, int64_t batch, int64_t bins, int32_t channels, float* rtf, void* stream);
int tac_rtf_power_f32(const float* psd_s, const float* psd_n, int64_t batch, int64_t bins, int32_t channels, const float* ref_vector,
                      int64_t ref_stride_b, int32_t ref_channel, int32_t n_iter, int32_t diagonal_loading, double diag_eps, float* rtf,
                      void* stream);
int tac_mvdr_weights_rtf_f32(const float* rtf, const float* psd_n, int64_t batch, int64_t bins, int32_t channels,
                             const float* ref_vector, int64_t ref_stride_b, int32_t ref_channel, int32_t diagonal_loading,
                             double diag_eps, double eps, float* weights, void* stream);
int tac_rtf_mvdr_f32(const float* spec, int64_t batch, int32_t channels, int64_t bins, int64_t frames, int64_t stride_b,
                     int64_t stride_c, int64_t stride_f, int64_t stride_t, const float* rtf, const float* psd_n,
                     const float* ref_vector, int64_t ref_stride_b, int32_t ref_channel, int32_t diagonal_loading, double diag_eps,
                     double eps, float* weights, float* out, int64_t out_b, int64_t out_f, int64_t out_t, void* stream);

/* (27) functional.rnnt_loss and the RNNTLoss layer: the transducer loss of Graves (2012) with torchaudio's semantics, and its
 *      gradient (csrc/rnnt.hip).  logits: float32 [batch][frames][targets1][classes] with targets1 = U + 1, unit stride along the
 *      classes and positive element strides stride_b / stride_t / stride_u (a slice of a padded joint output is taken as it is);
 *      element offsets are 64-bit.  targets: DEVICE int32 [batch][U], contiguous; logit_lengths (Tb), target_lengths (Ub): DEVICE
 *      int32 [batch].  denominators, lp_blank, lp_label, alphas, betas: float32 [batch][frames][targets1]; costs, grad_costs:
 *      float32 [batch]; grad_logits: float32 [batch][frames][targets1][classes], contiguous.  blank in [0, classes).  targets1 above
 *      tac_rnnt_max_targets() (1024) and batch * frames * targets1 >= 2^31: TAC_E_UNSUPPORTED.  Every entry below is ONE launch;
 *      the forward pass is tac_rnnt_rows_f32 then tac_rnnt_lattice_f32, the backward pass tac_rnnt_grad_f32.  The order of every
 *      sum is fixed and nothing is atomic: the same bits from run to run, for the 16-byte and the dword form of the row loads (the
 *      form follows from the alignment of base and strides and classes % 4), and for an entry whatever else is in the batch.
 *
 *      An entry with Tb outside [1, frames], Ub outside [0, U] or a used target (u < Ub) outside [0, classes) gets cost NaN, alphas
 *      and betas NaN and a NaN gradient over its whole block; none of these values is used to form an address.
 *
 *      tac_rnnt_rows_f32: per row (b, t, u) with t < Tb and u <= Ub: denominators = logsumexp over the classes (fused != 0; else 0,
 *      and the launch is only the gather), lp_blank = logits[blank] - denominator, lp_label = logits[targets[b][u]] - denominator
 *      for u < Ub (else 0).  The other rows are not read: their denominators, lp_blank, lp_label, alphas and betas are written as 0.
 *
 *      tac_rnnt_lattice_f32: alphas and betas over t < Tb, u <= Ub from lp_blank / lp_label (one workgroup per entry and
 *      direction, T_b + U_b dependent steps), costs[b] = -(alphas[Tb-1][Ub] + lp_blank[Tb-1][Ub]).  logaddexp(-inf, -inf) = -inf.
 *      After both launches every element of the five arrays and of costs is written.
 *
 *      tac_rnnt_grad_f32: with g = logits[t][u][v] - denominators[t][u] + alphas[t][u] + costs[b],
 *        grad = exp(g + betas[t][u])                                               (fused != 0; else 0)
 *             - [v == blank and t == Tb-1 and u == Ub] exp(g) - [v == blank and t < Tb-1] exp(g + betas[t+1][u])
 *             - [u < Ub and v == targets[b][u]] exp(g + betas[t][u+1]),
 *      clipped to [-clamp, clamp] where clamp > 0, then times grad_costs[b]; zero for t >= Tb or u > Ub, without a read.  Every
 *      element of grad_logits is written. */
int32_t tac_rnnt_max_targets(void);
int tac_rnnt_rows_f32(const float* logits, int64_t batch, int64_t frames, int64_t targets1, int64_t classes, int64_t stride_b,
                      int64_t stride_t, int64_t stride_u, const int32_t* targets, const int32_t* logit_lengths,
                      const int32_t* target_lengths, int32_t blank, int32_t fused, float* denominators, float* lp_blank,
                      float* lp_label, float* alphas, float* betas, void* stream);
int tac_rnnt_lattice_f32(int64_t batch, int64_t frames, int64_t targets1, int64_t classes, const int32_t* targets,
                         const int32_t* logit_lengths, const int32_t* target_lengths, const float* lp_blank, const float* lp_label,
                         float* alphas, float* betas, float* costs, void* stream);
int tac_rnnt_grad_f32(const float* logits, int64_t batch, int64_t frames, int64_t targets1, int64_t classes, int64_t stride_b,
                      int64_t stride_t, int64_t stride_u, const int32_t* targets, const int32_t* logit_lengths,
                      const int32_t* target_lengths, const float* alphas, const float* betas, const float* denominators,
                      const float* costs, const float* grad_costs, int32_t blank, float clamp, int32_t fused, float* grad_logits,
                      void* stream);

/* (28) functional.forced_align: CTC Viterbi alignment (csrc/align.hip) — the recursion, the backtrack, paths and scores in ONE
 *      launch, a workgroup per batch entry.  log_probs: float32 [batch][frames][classes] with positive element strides stride_b /
 *      stride_t / stride_c (a slice of a padded model output is read where it lies; offsets are 64-bit).  targets: DEVICE
 *      [batch][max_targets], contiguous, int64 where index64 != 0, else int32; paths: DEVICE [batch][frames] of the same integer
 *      type; scores: float32 [batch][frames].  input_lengths (Tb), target_lengths (Lb): DEVICE int32 [batch], or NULL for frames /
 *      max_targets in every entry.  blank in [0, classes).
 *
 *      Per entry: states s = 0 .. 2 Lb, even ones the blank, s = 2k + 1 targets[k]; alpha[0][0] = lp[0][blank], alpha[0][1] =
 *      lp[0][targets[0]], -inf elsewhere; for t >= 1, with x0 = alpha[t-1][s], x1 = alpha[t-1][s-1] and x2 = alpha[t-1][s-2] (only
 *      for odd s >= 3 with targets[s/2] != targets[s/2 - 1]; -inf otherwise and out of range): back-pointer 2 if x2 > x1 and
 *      x2 > x0, else 1 if x1 > x0 and x1 > x2, else 0, and alpha[t][s] = chosen + lp[t][label(s)], one float32 addition.  The end
 *      state is 2 Lb if alpha[Tb-1][2 Lb] > alpha[Tb-1][2 Lb - 1], else 2 Lb - 1 (0 for Lb = 0); the back-pointers are followed to
 *      t = 0.  paths[t] = label of the state at t, scores[t] = log_probs[t][paths[t]] (the same bits); for t >= Tb: blank and 0.
 *      Selection is by ordered compares: ties go to the lower back-pointer, a NaN where the compares send it.
 *
 *      An entry with Tb outside [1, frames], Lb outside [0, max_targets], a used target equal to blank or outside [0, classes),
 *      or Tb < Lb + (number of i in [1, Lb) with targets[i] == targets[i-1]) gets paths -1 and scores NaN on all frames; none of
 *      these values forms an address, and the other entries are unaffected.  The same bits from run to run and whatever else is
 *      in the batch.
 *
 *      max_targets + 1 above tac_forced_align_max_targets() (1024): TAC_E_UNSUPPORTED.  workspace: DEVICE,
 *      tac_forced_align_workspace(batch, frames, max_targets + 1) bytes (8-byte aligned; not initialised, not an output): the
 *      back-pointers (24 bytes per step and 64 targets) of entries whose Tb - 1 steps exceed what the kernel keeps in the LDS
 *      (6144 / (3 waves) steps, 2048 at most); may be NULL where that size is 0.  tac_forced_align_workspace returns -1 for
 *      sizes tac_forced_align_f32 refuses. */
int32_t tac_forced_align_max_targets(void);
int64_t tac_forced_align_workspace(int64_t batch, int64_t frames, int64_t targets1);
int tac_forced_align_f32(const float* log_probs, int64_t batch, int64_t frames, int64_t classes, int64_t stride_b,
                         int64_t stride_t, int64_t stride_c, const void* targets, int64_t max_targets, int32_t index64,
                         const int32_t* input_lengths, const int32_t* target_lengths, int32_t blank, void* workspace, void* paths,
                         float* scores, void* stream);

/* (29) functional.griffinlim / GriffinLim (torchaudio's Griffin-Lim phase recovery; csrc/griffinlim.hip) around (1) and (13):
 *      S = specgram^(1 / power), X_0 = S angles0 (or S), then n_iter times y = istft(X), R = stft(y),
 *      X = S (R - m Rprev) / (|R - m Rprev| + 1e-16), Rprev = R, and a last istft.  M, X and R are frame-major float32,
 *      [rows][T][F] and [rows][T][F][2], dense: what (1) writes and (13) reads in place.
 *
 *      tac_griffinlim_prepare_f32: once per call.  spec[r*stride_r + f*stride_f + t*stride_t] (element strides, positive on every
 *      axis longer than one: a time-contiguous (…, F, T) tensor is turned in the LDS, a frame-major view is read along its rows),
 *      angles: NULL or complex pairs at angles[2 (r*astride_r + f*astride_f + t*astride_t)] (strides in pairs).  The root is sqrtf at
 *      power 2, none at power 1, powf(s, (float)(1 / power)) otherwise.  Writes mag[r][t][f] (skipped when mag is NULL: the caller's
 *      input already is that tensor) and x0[r][t][f] = (mag, 0), or mag * angles.
 *      tac_griffinlim_update_f32: x[i] = mag[i] A / (|A| + 1e-16), A = r[i] - m rprev[i] (A = r[i] when rprev is NULL or m is 0) over
 *      n_bins complex bins.  |A| is formed on operands scaled by a power of two: right for every finite A, no overflow or underflow; a
 *      zero bin gives exactly 0.  16-byte accesses where r, rprev, x are 16-byte and mag 8-byte aligned, dword accesses otherwise. */
int tac_griffinlim_prepare_f32(const float* spec, int64_t rows, int64_t n_freqs, int64_t n_frames, int64_t stride_r, int64_t stride_f,
                               int64_t stride_t, const float* angles, int64_t astride_r, int64_t astride_f, int64_t astride_t,
                               float power, float* mag, float* x0, void* stream);
int tac_griffinlim_update_f32(const float* r, const float* rprev, const float* mag, int64_t n_bins, float m, float* x, void* stream);

/* (30) functional.pitch_shift's resampling tail, tac_amd::resample_fit: the sums of (15) for banks the LDS cannot hold, cut or
 *      zero-padded to out_len samples a row in the store:
 *      y[r][j*phases + p] = sum_{k < run[p]} bank[k][p] * x[r][j*step + off[p] + k]   for 0 <= j*phases + p < min(n_out, out_len),
 *      y[r][n] = 0 for min(n_out, out_len) <= n < out_len;  x[r][i] = x[r*stride_r + i], zero outside 0 <= i < l_in; out:
 *      float[rows][out_len], dense.  bank and table as in (15), read from global memory (consecutive lanes, consecutive
 *      addresses); the arithmetic is (15)'s — one fused multiply-add chain over k ascending from 0, only k < run[p] — so the
 *      bits are (15)'s wherever both take a bank.  No atomics, one writer per element, bit-identical from run to run.
 *      The starts j*step + off[p] must not decrease in n = j*phases + p, and span is the most consecutive input samples that
 *      `tile` (1024, 512 or 256) consecutive outputs read, from the first sample the tile's first output reads, over every tile
 *      start (_hip.resample_wide_plan computes both on the host).  off and run are clamped to that span: a wrong table or plan
 *      gives wrong sums, never an access outside a tile's LDS slot or a row.  taps <= 64, phases * taps <= 1 << 20,
 *      span <= 8192 and four rows' spans within 160 KiB, TAC_E_UNSUPPORTED (nothing launched) otherwise.
 *      16-byte loads where x and stride_r are 16-byte multiples, float loads otherwise. */
int tac_polyphase_wide_f32(const float* x, int64_t rows, int64_t l_in, int64_t stride_r, const float* bank, const int32_t* table,
                           int32_t phases, int32_t taps, int32_t step, int32_t span, int32_t tile, int64_t n_out, int64_t out_len,
                           float* out, void* stream);

/* (31) functional.vad / vad_start / Vad: torchaudio's SoX voice-activity detector behind the |X| rows of (2) (csrc/vad.hip).
 *      mag: float[rows][n_frames][dft / 2 + 1], the frame-major rows tac_spectrogram_f32 writes at n_fft = dft, power 1, for the
 *      measurement windows scaled by 2 / sqrt(mlen).  Per row, with S = N = 0 and t = 0, 1, … over the bins [s0, s1):
 *        m = t / (1 + t) while t <= boot_max (every frame if boot_max < 0), else decay[0];   S = S m + |X_t| (1 - m);   d = S^2
 *        m2 = 0 in those boot frames, else decay[2] where d > N and decay[4] elsewhere;      N = N m2 + d (1 - m2)
 *        e = sqrt(max(0, d - nra N));  c = the dft / 2-point transform of e win at [s0, s1), zeros elsewhere
 *        r = sum over q in [c0, c1) of |c_q|^2;   meas[row][t] = r > 0 ? max(0, 21 + log(r / (c1 - c0))) : 0
 *      decay: HOST array of six floats, (smooth, 1 - smooth, up, 1 - up, down, 1 - down), the complements formed in float64 and
 *      rounded once; win: DEVICE float[s1 - s0], the scaled cepstral window; tab: DEVICE float[dft / 2][2], the cosine and sine of 2 pi i / (dft / 2).
 *      float32 throughout, every sum in a fixed order, no atomics: bit-identical from run to run and whatever the batch holds.  A
 *      non-finite sample makes its row's measures 0 from that frame on.
 *      tac_vad_decide_f32: groups of `channels` consecutive rows of meas.  Every row's mean = mean trig + meas[k] otrig over k; the
 *      trigger frame k is the first at which a row's mean reaches level, i* the lowest such row; every row i >= i* searches
 *      back from k (jT = jZ = n; for j < n with v = meas[i][k - j], 0 before frame 0: v >= level and j <= jT + gap sets jZ = jT =
 *      j, else v == 0 and jT >= jZ sets jZ = j), flush = the largest min(n - 1, jZ), start[g] = max(0, (k - flush) period - pre),
 *      triggered[g] = 1; a group that never triggers gets max(0, time - keep) and 0.  triggered: DEVICE bytes.
 *      tac_vad_start_f32: both launches on the stream (meas: DEVICE scratch float[groups * channels][n_frames], all written); no
 *      host wait.  tac_vad_plan: the bins a lane keeps, the parts of the partial transform and the LDS bytes of the measuring
 *      launch, the longest search the deciding launch takes (n_search beyond it: TAC_E_UNSUPPORTED) and the workgroups per CU its
 *      persistent grid is capped at; TAC_E_UNSUPPORTED where s1 - s0 exceeds 2048, c1 - c0 512 or the LDS 144 KiB.  dft a power of
 *      two >= 16, 1 <= s0 < s1 <= dft / 2, 0 <= c0 < c1 <= dft / 4, TAC_E_INVALID otherwise. */
int tac_vad_plan(int32_t dft, int32_t s0, int32_t s1, int32_t c0, int32_t c1, int32_t* bins_per_lane, int32_t* parts, int32_t* lds_bytes,
                 int32_t* max_search, int32_t* blocks_per_cu);
int tac_vad_measures_f32(const float* mag, int64_t rows, int64_t n_frames, int32_t dft, int32_t s0, int32_t s1, int32_t c0, int32_t c1,
                         int32_t boot_max, const float* decay, float nra, const float* win, const float* tab, float* meas, void* stream);
int tac_vad_decide_f32(const float* meas, int64_t groups, int64_t channels, int64_t n_frames, int64_t time, int32_t n_search, int32_t gap,
                       int64_t period, int64_t pre, int64_t keep, float level, float trig, float otrig, int64_t* start, void* triggered,
                       void* stream);
int tac_vad_start_f32(const float* mag, int64_t groups, int64_t channels, int64_t n_frames, int64_t time, int32_t dft, int32_t s0, int32_t s1,
                      int32_t c0, int32_t c1, int32_t boot_max, const float* decay, float nra, const float* win, const float* tab,
                      int32_t n_search, int32_t gap, int64_t period, int64_t pre, int64_t keep, float level, float trig, float otrig,
                      float* meas, int64_t* start, void* triggered, void* stream);

/* (32) functional.simulate_rir_ism / simulate_rir_ism_batch / SimulateRirIsm: image-source room impulse responses (csrc/rir.hip).
 *      room, source: float[rooms][dims]; mic: float[rooms][mics][dims]; dims 2 or 3.  absorption: float[rooms or 1][n_band][2 dims], the
 *      walls as x_lo, x_hi, y_lo, y_hi, z_lo, z_hi; absorption_stride: floats between two rooms' coefficients, 0 where all share one
 *      set.  images: DEVICE int8[n_img][dims], the integer vectors X with sum |X_d| <= max_order in cartesian_prod order (last axis
 *      fastest).  tap_table: DEVICE float[filter_length][2], cos and sin of pi m / 2P for m = -P … P, P = filter_length / 2.
 *      Per (room, image, band b, microphone c), in float64: loc_d = room_d (X_d + 1) - source_d where X_d is odd, else room_d X_d +
 *      source_d; att_b = prod_d tr_lo^|floor(X_d / 2)| tr_hi^|floor((X_d + 1) / 2)| with tr = sqrt(1 - absorption); dist = |loc - mic_c|;
 *      delay = dist sample_rate / sound_speed; di = ceil(delay); f = di - delay.  (att_b / dist) w(m + f), w(x) = sinc(x) cos^2(pi x /
 *      2P) for |x| <= P and 0 beyond, is added to sample di + m + P of the raw response of (room, b, c) in image order.
 *      out: float[rooms][n_band][mics][length], samples [start, start + length) of the raw responses: ONE launch, every element
 *      written once, zeros included; float32 taps from f, att / dist, sinpi(f) and (cos, sin)(pi f / 2P) rounded once; no atomics,
 *      the same bits every run and whatever else the batch holds.  dist = 0 gives its (room, channel) rows the inf and NaN of the
 *      formulas and no other row any.  TAC_E_UNSUPPORTED for n_band above 8, filter_length below 3 or above 255, max_order above 32
 *      (tac_rir_limits reports the three and the shortest tile); an even filter_length is TAC_E_INVALID.
 *      tile: the samples of a row a wave owns, a power of two from 128 to 2048 (1024 above 2 bands, 512 above 4), or 0 for the
 *      launch's own choice, which tac_rir_tile reports for rooms * mics rows of `length` samples: the longest tile that leaves 16
 *      waves a CU.  The result's bits do not depend on it.
 *      tac_rir_span_f32: out[0] (DEVICE int64) = max di + filter_length - P over every (room, image, microphone), one launch of one
 *      workgroup; any odd filter_length. */
int tac_rir_limits(int32_t* min_tile, int32_t* max_bands, int32_t* max_filter_length, int32_t* max_order);
int tac_rir_tile(int64_t rows, int64_t length, int32_t n_band, int32_t* tile, int32_t* max_tile);
int tac_rir_ism_f32(const float* room, const float* source, const float* mic, const float* absorption, int64_t absorption_stride,
                    const void* images, const float* tap_table, int64_t rooms, int64_t mics, int32_t dims, int32_t n_band, int64_t n_img,
                    int32_t max_order, int64_t start, int64_t length, int32_t filter_length, double sound_speed, double sample_rate,
                    int32_t tile, float* out, void* stream);
int tac_rir_span_f32(const float* room, const float* source, const float* mic, const void* images, int64_t rooms, int64_t mics, int32_t dims,
                     int64_t n_img, int32_t filter_length, double sound_speed, double sample_rate, int64_t* out, void* stream);

/* (33) functional.sosfilt / SosFilt (and filtfilt above order 2): a cascade of second-order sections along a row in ONE launch
 *      (csrc/sosfilt.hip).  sos: HOST double[n_sections][6], rows (b0, b1, b2, a0, a1, a2) as scipy lays them out; section s + 1
 *      filters the output of section s, each as (16) with zero initial state; x, out, stride_r, clamp as in (16) (clamp limits the
 *      cascade's result only).  reverse != 0 runs the sections in reverse order, each from the END of the row: the adjoint.
 *      The waveform is read once and written once as float32; everything between the sections is float64 and stays on chip, so
 *      the result is the float64 cascade rounded once.  No workspace, no atomics, one writer per element, bit-identical from run to
 *      run and whatever else the batch holds; a non-finite sample reaches the samples after it (before it, with reverse) in its
 *      own row, and nothing else.  16-byte loads where x and stride_r are 16-byte multiples, float loads otherwise.
 *      n_sections 1 .. tac_sosfilt_max_sections() (8), TAC_E_UNSUPPORTED above, TAC_E_INVALID below; a section with a zero or
 *      non-finite a0 is TAC_E_INVALID, one whose scan matrices overflow float64 (tac_lfilter_supported's rule) TAC_E_UNSUPPORTED;
 *      tac_sosfilt_supported reports the same without launching.  A row is walked by one workgroup in tiles of tac_sosfilt_tile()
 *      samples; the persistent grid holds at most tac_sosfilt_blocks_per_cu() workgroups per CU, each taking every grid-th row. */
int32_t tac_sosfilt_max_sections(void);
int32_t tac_sosfilt_tile(void);
int32_t tac_sosfilt_blocks_per_cu(void);
int tac_sosfilt_supported(const double* sos, int32_t n_sections);
int tac_sosfilt_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const double* sos, int32_t n_sections,
                    int clamp, int reverse, float* out, void* stream);

/* (34) functional.overdrive / phaser / flanger: the SoX effects defined by a loop over time, each in ONE launch
 *      (csrc/sox_effects.hip).  x, out, rows, length, stride_r as in (16): float32 rows of unit stride, out dense.  The waveform is
 *      read once and written once as float32 and every state between is float64 on chip.  No workspace, no atomics, one writer per
 *      element, bit-identical from run to run and whatever else the batch holds; a non-finite sample reaches only later samples
 *      of its own row.  16-byte loads where x and stride_r are 16-byte multiples (not the flanger's feedback path).
 *      overdrive: t = shape(g x + c) (-2/3 below -1, 2/3 above 1, t - t^3 / 3 between), v[n] = t[n] - t[n-1] + 0.995 v[n-1],
 *        out = clamp(0.5 x + 0.75 v).  g, c finite (TAC_E_INVALID otherwise; tac_overdrive_supported reports it).  lfilter's tile
 *        walk: tiles of tac_overdrive_tile() samples, at most tac_overdrive_blocks_per_cu() workgroups per CU, one row each.
 *      phaser: y[n] = gain_in x[n] + decay y[n - d(n)], d(n) = L - mod[n % P] + 1 clipped to [1, L], out = clamp(gain_out y).
 *        mod: DEVICE int32[P].  L, P >= 1 (TAC_E_INVALID), L <= tac_phaser_max_delay() (TAC_E_UNSUPPORTED);
 *        tac_phaser_supported reports both.  Pointer jumping over tiles of tac_phaser_tile() samples in the LDS.
 *        tac_phaser_seq_f32 computes the same with one lane per row (L <= tac_phaser_seq_max_delay()): the ablation variant.
 *      flanger: rows = entries * channels, row r is channel r % channels; lfo: DEVICE float32[P]; phases: HOST int32[channels],
 *        each >= 0.  D = lfo[(i + phases[c]) % P], k = floor(D) clipped to [0, Lb - 2], w[i] = x[i] + fb delayed[i-1], delayed[i]
 *        the linear (quadratic != 0: SoX's quadratic) interpolation of w[i-k], w[i-k-1] (, w[i-k-2]), out = clamp(in_gain x +
 *        delay_gain delayed).  fb == 0: a streaming FIR over tiles of tac_flanger_tile() samples.  fb != 0: a wave per row, W slots
 *        per step (the caller passes W <= 1 + min k; W <= tac_flanger_max_block()), x staged in chunks of tac_flanger_chunk().
 *        2 <= Lb <= tac_flanger_max_delay(), W <= Lb - 1, channels <= 4: TAC_E_UNSUPPORTED otherwise, tac_flanger_supported. */
int32_t tac_overdrive_tile(void);
int32_t tac_overdrive_blocks_per_cu(void);
int tac_overdrive_supported(double g, double c);
int tac_overdrive_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, double g, double c, float* out, void* stream);
int32_t tac_phaser_tile(void);
int32_t tac_phaser_max_delay(void);
int32_t tac_phaser_seq_max_delay(void);
int32_t tac_phaser_blocks_per_cu(void);
int tac_phaser_supported(int32_t L, int32_t P);
int tac_phaser_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const int32_t* mod, int32_t P, int32_t L,
                   double gain_in, double decay, double gain_out, float* out, void* stream);
int tac_phaser_seq_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const int32_t* mod, int32_t P, int32_t L,
                       double gain_in, double decay, double gain_out, float* out, void* stream);
int32_t tac_flanger_tile(void);
int32_t tac_flanger_chunk(void);
int32_t tac_flanger_max_block(void);
int32_t tac_flanger_max_delay(void);
int32_t tac_flanger_blocks_per_cu(void);
int32_t tac_flanger_fb_blocks_per_cu(void);
int tac_flanger_supported(int32_t Lb, int32_t P, int32_t W, int32_t channels);
int tac_flanger_f32(const float* x, int64_t rows, int32_t channels, int64_t length, int64_t stride_r, const float* lfo, int32_t P,
                    const int32_t* phases, int32_t Lb, int32_t W, double fb, double in_gain, double delay_gain, int quadratic,
                    float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAC_AMD_H */
