// kaldi_fbank.hip — functional.kaldi_fbank (torchaudio.compliance.kaldi.fbank): waveform rows -> log mel rows in ONE launch.
//
//   frame t of a row = x[t S - pad .. + W)  (snip_edges: pad = 0; else pad = W/2 - S/2 and the row mirrored at both ends)
//   f -= mean(f);  e = log max(sum f^2, eps);  f[i] -= c f[i-1] (f[-1] := f[0]);  f *= window;  zero-pad to N
//   P = |rfft f|^2 or |rfft f|;  out[b] = log max(sum_k bank[b][k] P[k], eps);  [e as the first or the last column]
//
// The frames are 400 samples at the START of a 512-point transform, 160 samples apart, each with its own mean and its own
// pre-emphasis: neither a window nor torch.stft's centred framing expresses that, so the STFT kernels' frame loads do not
// apply.  Here a wave owns G = 8 / 4 / 2 consecutive frames of one row (N = 256 / 512 / 1024, WaveFft<N/2, 16>, as
// stft_small3.hpp) and walks a persistent grid of such units:
//   global -> area      the ONE contiguous span of the unit's frames, (G-1) S + W samples, with coalesced float loads — any row
//                       alignment, any (odd) shift; every sample is fetched once, not W / S times; the mirrored ends are
//                       resolved here.  Where the span does not fit the wave's area (S > ~N) the frames are staged one by one.
//   area -> registers   lane t of a frame takes the sample pairs (2m, 2m+1), m = t + q N/32, and the predecessor of each pair;
//                       samples at i >= W are zeros and are not read.  Mean and energy are sums over the N/32 lanes of the
//                       frame (__shfl_xor inside the lane group): no barrier.  The energy is summed on the mean-removed values.
//   FFT, R2C            WaveFft::run in the frame's part of the same area (the staged samples are in registers by then), then
//                       |X[k]|^2 for k < N/2 + 1 back into that part as a float row.
//   bank                band b = lane t, t + N/32, ...: ONE fused multiply-add chain over the band's bin interval, ascending;
//                       intervals end below the Nyquist bin, which is never read.  log is logf (as the dB epilogue's log10f).
// One writer per output element, no atomics: bit-identical from run to run.  A non-finite sample reaches exactly the frames
// whose W samples contain it (the span is shared, the reads are per frame).
//
// kaldi.mfcc and kaldi.spectrogram are epilogues of the same launch (MODE below): everything up to the |X|^2 row is shared.
//   spectrogram         the frame's lanes write log max(|X[k]|^2, eps) for k = 1 .. N/2 (the Nyquist bin included) and the log
//                       energy as column 0: no bank, no bank tables.
//   mfcc                the bands' logarithms go to the free half of the frame's own part of the area (the row takes N/2 + 1 of
//                       its N + N/16 + 2 floats) instead of memory; after a fence lane t computes the coefficients c = t,
//                       t + N/32, ..: each ONE fused multiply-add chain over b ascending against a table in the LDS,
//                       table[b][c] = D[b][c] lift[c] (and sqrt 2 on c = 0 for HTK without energy), float64 on the host,
//                       rounded once; the lanes of a frame read consecutive words of row b.  Energy substitution and the HTK
//                       rotation are decided at the store.  A NaN band reaches every chain of its frame (NaN * 0 = NaN).
#include <cmath>

#include "host_common.hpp"

namespace tac {

constexpr int KF_WAVES = 4;
constexpr int KF_MAX_MELS = 128;
constexpr int KF_MAX_WEIGHTS = 4096;             // floats of packed bank (a triangular bank has at most N of them)
constexpr float KF_EPS = 1.1920928955078125e-07f;   // 2^-23
constexpr float KF_LOG_EPS = -15.942385f;           // float32(log 2^-23): the floor's own value, not what logf makes of it

enum { KF_FBANK = 0, KF_MFCC = 1, KF_SPECTROGRAM = 2 };      // the epilogue of the launch

enum { KF_SNIP = TAC_KALDI_SNIP_EDGES, KF_DC = TAC_KALDI_REMOVE_DC, KF_RAW_ENERGY = TAC_KALDI_RAW_ENERGY, KF_USE_ENERGY = TAC_KALDI_USE_ENERGY,
       KF_HTK = TAC_KALDI_HTK, KF_LOG = TAC_KALDI_LOG, KF_POWER = TAC_KALDI_POWER };

struct KfArgs {
    const float* x;
    long long stride_r, length, rows, n_frames;
    const float* window;      // W floats
    const float* weights;     // w_total floats: the bands' non-zero runs back to back
    const int* table;         // [3][n_mels]: first bin, bins, offset into weights
    int win_length, shift, n_mels, w_total, flags, first;     // first: start of frame 0 (0 or -(W/2 - S/2))
    float preemph, log_energy_floor;
    float* out;
};

// KF_MFCC only, and a kernel argument of its own behind the others: KfArgs and with it the fbank kernel's code stay as they were
struct KfDct {
    const float* table;       // [n_mels][n_ceps], lifter (and HTK's sqrt 2) folded in
    int n_ceps;
};

template <int LPF>
__device__ __forceinline__ float kf_group_sum(float s) {
#pragma unroll
    for (int m = LPF / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    return s;
}

// log max(v, eps); NaN stays NaN (fmaxf alone would return eps).  The device's logf(2^-23) is one ulp under the correctly
// rounded value, so a floored element is given the constant, and nothing above the floor comes out below it
__device__ __forceinline__ float kf_log_floor(float v) {
    if (v != v) return v;
    return v > KF_EPS ? fmaxf(logf(v), KF_LOG_EPS) : KF_LOG_EPS;
}

// source index of position j of the mirrored row: j < 0 reads x[-j - 1], j >= n reads x[2n - 1 - j]; never out of bounds
__device__ __forceinline__ long long kf_mirror(long long j, long long n) {
    j = j < 0 ? -j - 1 : (j >= n ? 2 * n - 1 - j : j);
    return j < 0 ? 0 : (j >= n ? n - 1 : j);
}

// CH coefficients of a frame's DCT at once: c0, c0 + LPF, ..; every chain runs over b ascending
template <int CH, int LPF>
__device__ __forceinline__ void kf_dct_chunk(const float* lrow, const float* dtab, int M, int nc, int c0, float (&acc)[4]) {
    int col[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        col[j] = c0 + j * LPF < nc ? c0 + j * LPF : nc - 1;   // a lane past the last coefficient reads the last one
        acc[j] = 0.0f;
    }
    for (int b = 0; b < M; ++b) {
        const float l = lrow[b];
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[j] = __builtin_fmaf(l, dtab[b * nc + col[j]], acc[j]);
    }
}

template <int NC, int MODE>
__global__ void __launch_bounds__(KF_WAVES * 64)
kaldi_fbank_kernel(KfArgs a, Tables tb, KfDct dct) {
    constexpr int E = 16;
    using F = WaveFft<NC, E>;
    constexpr int LPF = F::LPF, G = F::G, N = F::N;
    constexpr int WAVE_SLOTS = ((G * F::PADDED + 1) / 2) * 2;
    constexpr int AREA = 2 * WAVE_SLOTS;                       // floats of a wave's area (>= G N)
    extern __shared__ __attribute__((aligned(16))) unsigned char kf_smem[];
    cf* const smem = reinterpret_cast<cf*>(kf_smem);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane / LPF, t = lane % LPF;
    cf* const wbase = smem + w * WAVE_SLOTS;
    cf* const lds = wbase + sub * F::PADDED;
    float* const area = reinterpret_cast<float*>(wbase);
    float* const srow = reinterpret_cast<float*>(lds);         // the frame's |X|^2 row: N/2 + 1 floats of its own part
    float* const wins = reinterpret_cast<float*>(smem + KF_WAVES * WAVE_SLOTS);     // N floats, zeros from W on
    float* const wts = wins + N;
    const int W = a.win_length, S = a.shift, M = a.n_mels;
    int* const blo = reinterpret_cast<int*>(wts + a.w_total);
    int* const bnum = blo + M;
    int* const boff = bnum + M;

    for (int i = threadIdx.x; i < N; i += KF_WAVES * 64) wins[i] = i < W ? a.window[i] : 0.0f;
    for (int i = threadIdx.x; i < a.w_total; i += KF_WAVES * 64) wts[i] = a.weights[i];     // (KF_SPECTROGRAM: no bank, 0 and 0)
    for (int b = threadIdx.x; b < M; b += KF_WAVES * 64) {
        // clamped to what the row and the packed bank hold, whatever the table says: never the Nyquist bin, never past the weights
        int lo = a.table[b], n = a.table[M + b], off = a.table[2 * M + b];
        lo = lo < 0 ? 0 : (lo > NC - 1 ? NC - 1 : lo);
        n = n < 0 ? 0 : (n > NC - lo ? NC - lo : n);
        n = n > a.w_total ? a.w_total : n;
        off = off < 0 ? 0 : (off > a.w_total - n ? a.w_total - n : off);
        blo[b] = lo;
        bnum[b] = n;
        boff[b] = off;
    }
    float* const dtab = reinterpret_cast<float*>(boff + M);    // KF_MFCC: n_mels x n_ceps
    if constexpr (MODE == KF_MFCC)
        for (int i = threadIdx.x; i < M * dct.n_ceps; i += KF_WAVES * 64) dtab[i] = dct.table[i];

    cf tw[F::NTW];
    cf ptw[F::NPAIR];
    F::load_twiddles(tw, tb.w_nc, t);
#pragma unroll
    for (int i = 0; i < F::NPAIR; ++i) ptw[i] = tb.w_n[t + i * LPF];
    __syncthreads();                                           // the tables are in the LDS; no barrier after this one

    const int T = (int)a.n_frames;
    const int upr = (T + G - 1) / G;                           // units per row
    const long long total = a.rows * upr;
    const bool one_span = (long long)(G - 1) * S + W <= AREA;
    const int pitch = one_span ? S : N;                        // floats between the staged frames of a unit
    const int C = M + ((a.flags & KF_USE_ENERGY) ? 1 : 0);
    const int col0 = ((a.flags & KF_USE_ENERGY) && !(a.flags & KF_HTK)) ? 1 : 0;
    const int ecol = (a.flags & KF_HTK) ? M : 0;
    const float c = a.preemph;

    for (long long unit = (long long)blockIdx.x * KF_WAVES + w; unit < total; unit += (long long)gridDim.x * KF_WAVES) {
        const long long row = unit / upr;
        const int frame0 = (int)(unit - row * upr) * G;
        const int nlive = T - frame0 < G ? T - frame0 : G;
        const float* const src = a.x + row * a.stride_r;
        const long long s0 = (long long)frame0 * S + a.first;
        wave_lds_fence();                                      // the previous unit's bank reads precede these writes
        if (one_span) {
            const int len = (nlive - 1) * S + W;
#pragma unroll 4
            for (int i = lane; i < len; i += 64) area[i] = src[kf_mirror(s0 + i, a.length)];
        } else {
            for (int f = 0; f < nlive; ++f)
#pragma unroll 4
                for (int i = lane; i < W; i += 64) area[f * N + i] = src[kf_mirror(s0 + (long long)f * S + i, a.length)];
        }
        wave_lds_fence();

        // ---- the frame's samples: pairs (xa, xb) = (f[2m], f[2m+1]) and xp = f[2m-1], the pre-emphasis predecessor of xa
        const bool live = sub < nlive;
        const int fbase = sub * pitch;
        float xa[E], xb[E], xp[E];
#pragma unroll
        for (int q = 0; q < E; ++q) {
            const int i0 = 2 * (t + q * LPF);
            const bool ok0 = live && i0 < W, ok1 = live && i0 + 1 < W;
            const float va = area[ok0 ? fbase + i0 : 0];
            const float vb = area[ok1 ? fbase + i0 + 1 : 0];
            const float vp = area[(ok0 && i0 > 0) ? fbase + i0 - 1 : 0];
            xa[q] = ok0 ? va : 0.0f;
            xb[q] = ok1 ? vb : 0.0f;
            xp[q] = ok0 ? (i0 > 0 ? vp : va) : 0.0f;           // f[-1] := f[0]
        }
        if (a.flags & KF_DC) {
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < E; ++q) s += xa[q] + xb[q];
            const float mean = kf_group_sum<LPF>(s) / (float)W;
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int i0 = 2 * (t + q * LPF);
                const bool ok0 = live && i0 < W, ok1 = live && i0 + 1 < W;
                xa[q] = ok0 ? xa[q] - mean : 0.0f;
                xb[q] = ok1 ? xb[q] - mean : 0.0f;
                xp[q] = ok0 ? xp[q] - mean : 0.0f;
            }
        }
        float energy = 0.0f;
        if (a.flags & KF_RAW_ENERGY) {
#pragma unroll
            for (int q = 0; q < E; ++q) energy = __builtin_fmaf(xb[q], xb[q], __builtin_fmaf(xa[q], xa[q], energy));
        }
        cf v[1][E];
        {
            const cf* const wp = reinterpret_cast<const cf*>(wins);
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int i0 = 2 * (t + q * LPF);
                const bool ok1 = live && i0 + 1 < W;
                float ya = xa[q], yb = xb[q];
                if (c != 0.0f) {
                    yb = ok1 ? __builtin_fmaf(-c, xa[q], xb[q]) : 0.0f;
                    ya = __builtin_fmaf(-c, xp[q], xa[q]);
                }
                const cf wv = wp[t + q * LPF];
                v[0][q] = mkc(ya * wv.x, ok1 ? yb * wv.y : 0.0f);
            }
        }
        if (!(a.flags & KF_RAW_ENERGY)) {
#pragma unroll
            for (int q = 0; q < E; ++q) energy = __builtin_fmaf(v[0][q].y, v[0][q].y, __builtin_fmaf(v[0][q].x, v[0][q].x, energy));
        }
        if (a.flags & KF_USE_ENERGY) {
            energy = kf_log_floor(kf_group_sum<LPF>(energy));
            energy = (energy == energy) ? fmaxf(energy, a.log_energy_floor) : energy;
        }
        wave_lds_fence();                                      // every lane's sample reads precede the first pass's writes

        // ---- transform and R2C split: (|2 X[k]|^2, |2 X[N/2 - k]|^2) per pair, then the row in place of the spectrum
        {
            cf* const ldsv[1] = {lds};
            F::template run<1>(v, ldsv, tw, t);
        }
        {
            cf pw[F::NPAIR];
#pragma unroll
            for (int i = 0; i < F::NPAIR; ++i) {
                const int k = t + i * LPF;
                pw[i] = F::r2c_power_x2(lds[lds_pad(k)], lds[lds_pad((NC - k) & (NC - 1))], ptw[i]);
            }
            cf xm, unused;
            F::r2c_pair(lds, NC / 2, mkc(0.0f, -1.0f), xm, unused);
            wave_lds_fence();                                  // every Z of this unit is in registers
            const bool power = (a.flags & KF_POWER) != 0;
            auto value = [&](float p4) { return power ? 0.25f * p4 : 0.5f * sqrtf(p4); };
#pragma unroll
            for (int i = 0; i < F::NPAIR; ++i) {
                const int k = t + i * LPF;
                srow[k] = value(pw[i].x);
                srow[NC - k] = value(pw[i].y);                 // (k = 0: the Nyquist bin, which no band reads)
            }
            if (t == 0) srow[NC / 2] = value(cnorm2(xm));
            wave_lds_fence();
        }

        if constexpr (MODE == KF_SPECTROGRAM) {
            // ---- every bin's logarithm, the Nyquist bin srow[NC] included; the energy in place of the DC bin
            if (live) {
                float* const orow = a.out + (row * T + frame0 + sub) * (NC + 1);
                for (int k = t; k <= NC; k += LPF) orow[k] = k == 0 ? energy : kf_log_floor(srow[k]);
            }
        } else if constexpr (MODE == KF_MFCC) {
            // ---- the bank as below, its logarithms kept in the LDS: the half of the frame's part behind the row is free
            static_assert(NC + 2 + KF_MAX_MELS <= 2 * F::PADDED, "the log-mel row does not fit behind the spectrum row");
            float* const lrow = srow + NC + 2;
            if (live) {
                for (int b = t; b < M; b += LPF) {
                    const int lo = blo[b], n = bnum[b];
                    const float* const wb = wts + boff[b];
                    float acc = 0.0f;
                    for (int j = 0; j < n; ++j) acc = __builtin_fmaf(wb[j], srow[lo + j], acc);
                    lrow[b] = kf_log_floor(acc);
                }
            }
            wave_lds_fence();                                  // the frame's whole log-mel row is written
            // ---- DCT: coefficient c = t, t + LPF, ..; the energy in place of C0; HTK: [C1 .. C_{n-1}, C0]
            if (live) {
                const int nc = dct.n_ceps;
                float* const orow = a.out + (row * T + frame0 + sub) * nc;
                const bool sub_e = (a.flags & KF_USE_ENERGY) != 0, htk = (a.flags & KF_HTK) != 0;
                auto store = [&](int cc, float val) {
                    if (cc < nc) orow[htk ? (cc == 0 ? nc - 1 : cc - 1) : cc] = (cc == 0 && sub_e) ? energy : val;
                };
                float acc[4];
                int c0 = t;
                for (; c0 - t + 3 * LPF < nc; c0 += 4 * LPF) {          // (uniform over the wave: t is taken out)
                    kf_dct_chunk<4, LPF>(lrow, dtab, M, nc, c0, acc);
#pragma unroll
                    for (int j = 0; j < 4; ++j) store(c0 + j * LPF, acc[j]);
                }
                if (c0 - t + LPF < nc) {
                    kf_dct_chunk<2, LPF>(lrow, dtab, M, nc, c0, acc);
                    store(c0, acc[0]);
                    store(c0 + LPF, acc[1]);
                    c0 += 2 * LPF;
                }
                if (c0 - t < nc) {
                    kf_dct_chunk<1, LPF>(lrow, dtab, M, nc, c0, acc);
                    store(c0, acc[0]);
                }
            }
        } else
        // ---- the bank: one chain per output element over its band's bins, ascending
        if (live) {
            float* const orow = a.out + (row * T + frame0 + sub) * C;
            for (int b = t; b < M; b += LPF) {
                const int lo = blo[b], n = bnum[b];
                const float* const wb = wts + boff[b];
                float acc = 0.0f;
                for (int j = 0; j < n; ++j) acc = __builtin_fmaf(wb[j], srow[lo + j], acc);
                orow[col0 + b] = (a.flags & KF_LOG) ? kf_log_floor(acc) : acc;
            }
            if (t == 0 && (a.flags & KF_USE_ENERGY)) orow[ecol] = energy;
        }
    }
}

// bytes of LDS of a launch without the DCT table: the waves' areas, the window, the packed bank and its table
template <int NC>
constexpr size_t kf_lds_bytes(int w_total, int n_mels) {
    using F = WaveFft<NC, 16>;
    constexpr int WAVE_SLOTS = ((F::G * F::PADDED + 1) / 2) * 2;
    return (size_t)KF_WAVES * WAVE_SLOTS * sizeof(cf) + 4 * ((size_t)F::N + (size_t)w_total + 3 * (size_t)n_mels);
}

template <int NC, int MODE = KF_FBANK>
int kf_launch(const KfArgs& a, hipStream_t stream, KfDct dct = KfDct()) {
    using F = WaveFft<NC, 16>;
    Tables tb;
    const int rc = get_tables(2 * NC, &tb);
    if (rc != TAC_OK) return rc;
    const size_t bytes = kf_lds_bytes<NC>(a.w_total, a.n_mels) + (MODE == KF_MFCC ? 4 * (size_t)a.n_mels * (size_t)dct.n_ceps : 0);
    if (bytes > 64 * 1024) return TAC_E_UNSUPPORTED;
    const long long units = a.rows * ((a.n_frames + F::G - 1) / F::G);
    long long per_cu = (long long)(160 * 1024 / bytes);
    per_cu = per_cu > 2 ? 2 : per_cu;                          // the kernel's ~220 registers leave room for two waves per SIMD
    const long long blocks = persistent_blocks(units, KF_WAVES, (long long)device_cu_count() * per_cu);
    return launch_kernel(kaldi_fbank_kernel<NC, MODE>, blocks, KF_WAVES * 64, bytes, stream, a, tb, dct);
}

}  // namespace tac

extern "C" {

int64_t tac_kaldi_num_frames(int64_t length, int32_t win_length, int32_t shift, int snip_edges) {
    if (length < 0 || win_length < 1 || shift < 1) return 0;
    if (snip_edges) return length < win_length ? 0 : 1 + (length - win_length) / shift;
    return (length + shift / 2) / shift;
}

int tac_kaldi_fbank_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const float* window, const float* weights,
                        const int32_t* table, int32_t n_fft, int32_t win_length, int32_t shift, int32_t n_mels, int32_t w_total,
                        int32_t flags, float preemph, float energy_floor, float* out, void* stream) {
    using namespace tac;
    if (!x || !window || !weights || !table || !out) return TAC_E_INVALID;
    if (rows <= 0 || length <= 0 || win_length < 2 || shift < 1 || w_total < 1) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    if (n_fft != 256 && n_fft != 512 && n_fft != 1024) return TAC_E_UNSUPPORTED;
    if (win_length > n_fft || n_mels < 4 || n_mels > KF_MAX_MELS || w_total > KF_MAX_WEIGHTS) return TAC_E_UNSUPPORTED;
    const bool snip = (flags & KF_SNIP) != 0;
    if (!snip && length < win_length) return TAC_E_UNSUPPORTED;                 // (the mirror would leave the row)
    if (length >= 0x7fffffffLL) return TAC_E_UNSUPPORTED;
    const int64_t frames = tac_kaldi_num_frames(length, win_length, shift, snip ? 1 : 0);
    if (frames <= 0) return TAC_E_INVALID;
    if (frames >= 0x7fffffffLL || rows >= (1LL << 40)) return TAC_E_UNSUPPORTED;
    KfArgs a;
    a.x = x;
    a.stride_r = stride_r;
    a.length = length;
    a.rows = rows;
    a.n_frames = frames;
    a.window = window;
    a.weights = weights;
    a.table = table;
    a.win_length = win_length;
    a.shift = shift;
    a.n_mels = n_mels;
    a.w_total = w_total;
    a.flags = flags;
    a.first = snip ? 0 : -(win_length / 2 - shift / 2);
    a.preemph = preemph;
    a.log_energy_floor = energy_floor > 0.0f ? std::log(energy_floor) : -INFINITY;
    a.out = out;
    hipStream_t s = (hipStream_t)stream;
    return n_fft == 256 ? kf_launch<128>(a, s) : (n_fft == 512 ? kf_launch<256>(a, s) : kf_launch<512>(a, s));
}

int64_t tac_kaldi_mfcc_table_limit(int32_t n_fft, int32_t n_mels, int32_t w_total) {
    using namespace tac;
    if ((n_fft != 256 && n_fft != 512 && n_fft != 1024) || n_mels < 4 || n_mels > KF_MAX_MELS || w_total < 1 || w_total > KF_MAX_WEIGHTS)
        return 0;
    const size_t fixed = n_fft == 256 ? kf_lds_bytes<128>(w_total, n_mels)
                                      : (n_fft == 512 ? kf_lds_bytes<256>(w_total, n_mels) : kf_lds_bytes<512>(w_total, n_mels));
    return fixed >= 64 * 1024 ? 0 : (int64_t)((64 * 1024 - fixed) / 4);
}

// what the three entry points share: the checks on the rows and the framing, and the arguments derived from them
static int kf_common_args(const float* x, int64_t rows, int64_t length, int64_t stride_r, const float* window, int32_t n_fft,
                          int32_t win_length, int32_t shift, int32_t flags, float preemph, float energy_floor, float* out,
                          tac::KfArgs* a) {
    using namespace tac;
    if (!x || !window || !out) return TAC_E_INVALID;
    if (rows <= 0 || length <= 0 || win_length < 2 || shift < 1) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    if (n_fft != 256 && n_fft != 512 && n_fft != 1024) return TAC_E_UNSUPPORTED;
    if (win_length > n_fft) return TAC_E_UNSUPPORTED;
    const bool snip = (flags & KF_SNIP) != 0;
    if (!snip && length < win_length) return TAC_E_UNSUPPORTED;                 // (the mirror would leave the row)
    if (length >= 0x7fffffffLL) return TAC_E_UNSUPPORTED;
    const int64_t frames = tac_kaldi_num_frames(length, win_length, shift, snip ? 1 : 0);
    if (frames <= 0) return TAC_E_INVALID;
    if (frames >= 0x7fffffffLL || rows >= (1LL << 40)) return TAC_E_UNSUPPORTED;
    *a = KfArgs();
    a->x = x;
    a->stride_r = stride_r;
    a->length = length;
    a->rows = rows;
    a->n_frames = frames;
    a->window = window;
    a->win_length = win_length;
    a->shift = shift;
    a->flags = flags;
    a->first = snip ? 0 : -(win_length / 2 - shift / 2);
    a->preemph = preemph;
    a->log_energy_floor = energy_floor > 0.0f ? std::log(energy_floor) : -INFINITY;
    a->out = out;
    return TAC_OK;
}

int tac_kaldi_mfcc_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const float* window, const float* weights,
                       const int32_t* table, const float* dct, int32_t n_fft, int32_t win_length, int32_t shift, int32_t n_mels,
                       int32_t w_total, int32_t n_ceps, int32_t flags, float preemph, float energy_floor, float* out, void* stream) {
    using namespace tac;
    if (!weights || !table || !dct || w_total < 1 || n_ceps < 1) return TAC_E_INVALID;
    if (n_mels < 4 || n_mels > KF_MAX_MELS || w_total > KF_MAX_WEIGHTS) return TAC_E_UNSUPPORTED;
    if (n_ceps > n_mels) return TAC_E_INVALID;
    KfArgs a;
    // the log-mel row of the definition: logarithm of the power bank, whatever the caller's bits say
    const int rc = kf_common_args(x, rows, length, stride_r, window, n_fft, win_length, shift, flags | KF_LOG | KF_POWER, preemph,
                                  energy_floor, out, &a);
    if (rc != TAC_OK) return rc;
    if ((int64_t)n_mels * n_ceps > tac_kaldi_mfcc_table_limit(n_fft, n_mels, w_total)) return TAC_E_UNSUPPORTED;
    a.weights = weights;
    a.table = table;
    a.n_mels = n_mels;
    a.w_total = w_total;
    KfDct d;
    d.table = dct;
    d.n_ceps = n_ceps;
    hipStream_t s = (hipStream_t)stream;
    return n_fft == 256 ? kf_launch<128, KF_MFCC>(a, s, d)
                        : (n_fft == 512 ? kf_launch<256, KF_MFCC>(a, s, d) : kf_launch<512, KF_MFCC>(a, s, d));
}

int tac_kaldi_spectrogram_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const float* window, int32_t n_fft,
                              int32_t win_length, int32_t shift, int32_t flags, float preemph, float energy_floor, float* out,
                              void* stream) {
    using namespace tac;
    KfArgs a;
    // log |X|^2 with the log energy as column 0: power, logarithm and energy are the definition, not options
    const int rc = kf_common_args(x, rows, length, stride_r, window, n_fft, win_length, shift,
                                  (flags | KF_LOG | KF_POWER | KF_USE_ENERGY) & ~KF_HTK, preemph, energy_floor, out, &a);
    if (rc != TAC_OK) return rc;
    a.weights = nullptr;                                        // no bank: nothing of it is read (w_total = n_mels = 0)
    a.table = nullptr;
    a.n_mels = 0;
    a.w_total = 0;
    hipStream_t s = (hipStream_t)stream;
    return n_fft == 256 ? kf_launch<128, KF_SPECTROGRAM>(a, s)
                        : (n_fft == 512 ? kf_launch<256, KF_SPECTROGRAM>(a, s) : kf_launch<512, KF_SPECTROGRAM>(a, s));
}

}  // extern "C"
