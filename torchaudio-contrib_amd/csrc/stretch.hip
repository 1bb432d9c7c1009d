// stretch.hip — STFT -> TimeStretch -> ComplexNorm [-> ApplyFilterbank] [-> AmplitudeToDb] on magnitudes alone
// (layers.py:215-264 behind functional.py:116-128; reference tests/test_layers.py:86-106 composes exactly this chain).
//
// phase_vocoder returns (mag cos phi, mag sin phi) with mag = alpha |X[t1]| + (1 - alpha) |X[t0]| (functional.py:233-274), and
// complex_norm of that is mag^power whatever phi is: the running phase, phase_advance, the wrap and the cumulative sum all cancel.
// So the chain is the |X| spectrogram kernel (real rows) followed by ONE streaming pass that interpolates neighbouring frames and
// raises to `power` — and, in the mel form, contracts the band-sparse bank (mel_lanes.hpp) and takes dB in the same launch.
//
//   stretch_rows_kernel   a workgroup owns a span of consecutive output frames of one row; a thread owns 16-byte columns of the
//                         row and walks the span keeping its two source chunks in registers, so a source frame shared by
//                         neighbouring output frames (all of them below rate 1) is fetched once.  Rows of 1025 floats start on
//                         any dword: the accesses are 16 bytes wide with dword alignment, like fb_lanes_kernel's.
//   stretch_mel_kernel    fb_lanes_kernel (melspec_sparse.hip) with another loader: one wave per OUTPUT frame, the two source rows
//                         of the next frame in flight during the contraction, the blended row parked in the wave's LDS buffer,
//                         lane_mel_contract / lane_mel_store of mel_lanes.hpp behind it.
//   stretch_bwd_kernel    the adjoint of the rows form as a gather per source frame: idx0 is non-decreasing, so the outputs that
//                         read frame t are the index range [bounds[t - 1], bounds[t + 1]) — no atomics, no zero-initialised output,
//                         bit-reproducible.
//
// Non-finite input.  In the reference a NaN component has a NaN angle, and the cumulative sum carries it into EVERY later output
// frame of the bin; an infinite magnitude with a finite angle stays in the frames interpolated from it.  Frame-parallel kernels do
// not see that history: each notes the first output frame at which it met a non-finite value in one word per row (atomicMin into
// `flags`, which the entry point fills with 0x7f bytes first), and a second launch with one workgroup per row — returning at once
// for a clean row — walks the outputs from that frame on with a sticky flag per bin and overwrites what the reference would have
// lost.  In the mel form the reference's dense matmul turns one non-finite bin into a non-finite frame, so there the flag is per frame.
#include "host_common.hpp"
#include "fb_lanes.hpp"

#include <math.h>

namespace tac {

constexpr int SN_THREADS = 256;
constexpr unsigned SN_CLEAN = 0x7f7f7f7fu;           // a row's flag word after hipMemsetAsync(flags, 0x7f, ...): nothing met
typedef float sn_f4 __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at dword alignment (global memory only)

struct StretchArgs {
    const float* mag;           // [rows][n_frames][n_freqs], frame stride stride_t, row stride stride_r
    long long rows;
    int n_freqs, n_frames;
    long long stride_r, stride_t;
    const int* idx0;            // n_out source frames (the second one is idx0 + 1; >= n_frames: the reference's zero padding)
    const float* alpha;         // n_out weights of the second frame
    int n_out;
    float power;
    int db;
    float amin, log10_ref;
};

// PMODE 1: power == 1, 2: power == 2, 0: powf
template <int PMODE>
__device__ __forceinline__ float sn_pow(float v, float power) {
    if constexpr (PMODE == 1) return v;
    if constexpr (PMODE == 2) return v * v;
    return powf(v, power);
}
// d v^power / d v
template <int PMODE>
__device__ __forceinline__ float sn_dpow(float v, float power) {
    if constexpr (PMODE == 1) return 1.0f;
    if constexpr (PMODE == 2) return 2.0f * v;
    return power * powf(v, power - 1.0f);          // (0^(power - 1) = inf below power 1, as torch's pow backward has it)
}
__device__ __forceinline__ bool sn_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }
// the reference's order: frac * n1 + (1 - frac) * n0 (functional.py:266)
__device__ __forceinline__ float sn_blend(float n0, float n1, float a) { return a * n1 + (1.0f - a) * n0; }

template <class V> struct sn_lanes;
template <> struct sn_lanes<float> {
    static constexpr int N = 1;
    static __device__ __forceinline__ float get(const float& v, int) { return v; }
    static __device__ __forceinline__ void set(float& v, int, float x) { v = x; }
    static __device__ __forceinline__ float zero() { return 0.0f; }
};
template <> struct sn_lanes<sn_f4> {
    static constexpr int N = 4;
    static __device__ __forceinline__ float get(const sn_f4& v, int i) { return v[i]; }
    static __device__ __forceinline__ void set(sn_f4& v, int i, float x) { v[i] = x; }
    static __device__ __forceinline__ sn_f4 zero() { sn_f4 z = {0.0f, 0.0f, 0.0f, 0.0f}; return z; }
};

// one column (V = 16 bytes or one float at bin `f`) of output frames [j0, j1) of a row; returns the first frame at which a
// non-finite value appeared (or keeps `bad`)
template <int PMODE, class V>
__device__ __forceinline__ int sn_column(const StretchArgs& a, const float* base, float* obase, int f, int j0, int j1, int bad) {
    using L = sn_lanes<V>;
    auto frame = [&](int t) -> V {
        return t < a.n_frames ? *reinterpret_cast<const V*>(base + (long long)t * a.stride_t + f) : L::zero();
    };
    int held = -2;
    V n0 = L::zero(), n1 = L::zero();
    for (int j = j0; j < j1; ++j) {
        const int t = a.idx0[j];
        const float al = a.alpha[j];
        if (t == held + 1) {
            n0 = n1;
            n1 = frame(t + 1);
        } else if (t != held) {
            n0 = frame(t);
            n1 = frame(t + 1);
        }
        held = t;
        V o;
        bool ok = true;
#pragma unroll
        for (int i = 0; i < L::N; ++i) {
            const float v = sn_blend(L::get(n0, i), L::get(n1, i), al);
            ok = ok && sn_finite(v);
            const float p = sn_pow<PMODE>(v, a.power);
            L::set(o, i, a.db ? amp_to_db(p, a.amin, a.log10_ref) : p);
        }
        if (!ok && j < bad) bad = j;
        __builtin_nontemporal_store(o, reinterpret_cast<V*>(obase + (long long)j * a.n_freqs + f));
    }
    return bad;
}

template <int PMODE>
__global__ void __launch_bounds__(SN_THREADS)
stretch_rows_kernel(StretchArgs a, float* __restrict__ out, unsigned* __restrict__ flags, int span, int spans_per_row) {
    const long long r = blockIdx.x / spans_per_row;
    const int j0 = (int)(blockIdx.x - r * spans_per_row) * span;
    const int j1 = j0 + span < a.n_out ? j0 + span : a.n_out;
    const float* base = a.mag + r * a.stride_r;
    float* obase = out + r * (long long)a.n_out * a.n_freqs;
    const int nfull = a.n_freqs >> 2;
    int bad = 0x7fffffff;
    for (int c = threadIdx.x; c < nfull; c += SN_THREADS) bad = sn_column<PMODE, sn_f4>(a, base, obase, 4 * c, j0, j1, bad);
    if ((int)threadIdx.x < (a.n_freqs & 3)) bad = sn_column<PMODE, float>(a, base, obase, 4 * nfull + threadIdx.x, j0, j1, bad);
    if (bad != 0x7fffffff) atomicMin(flags + r, (unsigned)bad);
}

// rows form, second launch: one workgroup per row; sticky NaN per bin from the flagged frame on
__global__ void __launch_bounds__(SN_THREADS)
stretch_rows_fixup_kernel(StretchArgs a, float* __restrict__ out, const unsigned* __restrict__ flags) {
    const long long r = blockIdx.x;
    const unsigned first = flags[r];
    if (first >= (unsigned)a.n_out) return;
    const float* base = a.mag + r * a.stride_r;
    float* obase = out + r * (long long)a.n_out * a.n_freqs;
    for (int f = threadIdx.x; f < a.n_freqs; f += SN_THREADS) {
        bool sticky = false;
        for (int j = (int)first; j < a.n_out; ++j) {
            const int t = a.idx0[j];
            const float x0 = t < a.n_frames ? base[(long long)t * a.stride_t + f] : 0.0f;
            const float x1 = t + 1 < a.n_frames ? base[(long long)(t + 1) * a.stride_t + f] : 0.0f;
            if (sticky) obase[(long long)j * a.n_freqs + f] = __builtin_nanf("");
            sticky = sticky || x0 != x0 || x1 != x1;
        }
    }
}

// mel form, second launch: a frame with a non-finite interpolated bin, and every frame behind a NaN source value, is NaN throughout
__global__ void __launch_bounds__(SN_THREADS)
stretch_mel_fixup_kernel(StretchArgs a, float* __restrict__ out, int n_mels, const unsigned* __restrict__ flags) {
    const long long r = blockIdx.x;
    const unsigned first = flags[r];
    if (first >= (unsigned)a.n_out) return;
    const float* base = a.mag + r * a.stride_r;
    float* obase = out + r * (long long)a.n_out * n_mels;
    bool sticky = false;
    for (int j = (int)first; j < a.n_out; ++j) {
        const int t = a.idx0[j];
        const float al = a.alpha[j];
        bool local = false;
        for (int f = threadIdx.x; f < a.n_freqs; f += SN_THREADS) {
            const float x0 = t < a.n_frames ? base[(long long)t * a.stride_t + f] : 0.0f;
            const float x1 = t + 1 < a.n_frames ? base[(long long)(t + 1) * a.stride_t + f] : 0.0f;
            local = local || !sn_finite(sn_blend(x0, x1, al));
            sticky = sticky || x0 != x0 || x1 != x1;
        }
        if (__syncthreads_or(local || sticky))
            for (int m = threadIdx.x; m < n_mels; m += SN_THREADS) obase[(long long)j * n_mels + m] = __builtin_nanf("");
    }
}

// ---------------------------------------------------------------- mel form: fb_lanes_kernel's frame loop behind a blending loader
template <int PMODE, int S, int CHUNKS, int WAVES, int FLY>
__global__ void __launch_bounds__(WAVES * 64)
stretch_mel_kernel(StretchArgs a, LaneMel mel, unsigned* __restrict__ flags) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_freqs = a.n_freqs;
    const int pitch = fbl_pitch(n_freqs);
    float* const srow = reinterpret_cast<float*>(smem_raw) + (size_t)w * (pitch + LM_MAX_MELS + 4);
    float* const mbuf = srow + pitch;                                        // the band row, staged at its 16-byte phase
    unsigned* const next_frame = reinterpret_cast<unsigned*>(reinterpret_cast<float*>(smem_raw) +
                                                             (size_t)WAVES * (pitch + LM_MAX_MELS + 4));
    int* const mlo = reinterpret_cast<int*>(next_frame + 4);
    float* const mwl = reinterpret_cast<float*>(mlo + lm_desc_ints(64));
    lane_mel_load_tables<S, 64, FLY>(mlo, mwl, mel, threadIdx.x, WAVES * 64);

    const long long total = a.rows * a.n_out;
    const long long chunk = (total + gridDim.x - 1) / gridDim.x;
    const long long begin = (long long)blockIdx.x * chunk;
    const long long endl = begin + chunk < total ? begin + chunk : total;
    const int nloc = endl > begin ? (int)(endl - begin) : 0;
    if (threadIdx.x == 0) *next_frame = WAVES;
    __syncthreads();
    auto grab = [&]() -> int {
        unsigned v = 0;
        if (lane == 0) v = __hip_atomic_fetch_add(next_frame, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return (int)__builtin_amdgcn_readfirstlane(v);
    };
    // the two source rows of an output frame as 16-byte chunks (dword alignment); chunks past the row are clamped to its last full
    // one, a source frame past the end (the reference's zero padding) to the last frame and multiplied by zero when it is blended
    const int lastc = (n_freqs >> 2) - 1;
    f4 nx0[CHUNKS], nx1[CHUNKS];
    float tl0[3], tl1[3];
    float r_al = 0.0f, r_k0 = 0.0f, r_k1 = 0.0f;
    long long r_row = 0;
    int r_j = 0;
    auto request = [&](int i) {
        const long long gf = begin + i;
        r_row = gf / a.n_out;
        r_j = (int)(gf - r_row * a.n_out);
        const int t = a.idx0[r_j];
        r_al = a.alpha[r_j];
        r_k0 = t < a.n_frames ? 1.0f : 0.0f;
        r_k1 = t + 1 < a.n_frames ? 1.0f : 0.0f;
        const int last_t = a.n_frames - 1;
        const float* s0 = a.mag + r_row * a.stride_r + (long long)(t < last_t ? t : last_t) * a.stride_t;
        const float* s1 = a.mag + r_row * a.stride_r + (long long)(t + 1 < last_t ? t + 1 : last_t) * a.stride_t;
#pragma unroll
        for (int u = 0; u < CHUNKS; ++u) {
            const int c = lane + 64 * u;
            const int off = 4 * (c < lastc ? c : lastc);
            nx0[u] = *reinterpret_cast<const sn_f4*>(s0 + off);
            nx1[u] = *reinterpret_cast<const sn_f4*>(s1 + off);
        }
#pragma unroll
        for (int u = 0; u < 3; ++u) {                                         // the (n_freqs mod 4) bins behind the last full chunk
            tl0[u] = s0[n_freqs - 1 - u];
            tl1[u] = s1[n_freqs - 1 - u];
        }
    };
    // blend, note a non-finite value, raise to the power, park the row in LDS
    auto deposit = [&]() {
        bool ok = true;
        auto value = [&](float x0, float x1) -> float {
            const float v = sn_blend(r_k0 != 0.0f ? x0 : 0.0f, r_k1 != 0.0f ? x1 : 0.0f, r_al);
            ok = ok && sn_finite(v);
            return sn_pow<PMODE>(v, a.power);
        };
#pragma unroll
        for (int u = 0; u < CHUNKS; ++u) {
            const int c = lane + 64 * u;
            if (c <= lastc) {
                f4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = value(nx0[u][q], nx1[u][q]);
                *reinterpret_cast<f4*>(srow + 4 * c) = o;
            }
        }
        if (lane < 3 && n_freqs - 1 - lane > 4 * lastc + 3) {
            const int q = lane == 0 ? 0 : (lane == 1 ? 1 : 2);
            srow[n_freqs - 1 - lane] = value(tl0[q], tl1[q]);
        }
        if (!ok) atomicMin(flags + r_row, (unsigned)r_j);
    };
    int i = w;
    if (i < nloc) request(i);
    while (i < nloc) {
        const int nx = grab();
        wave_lds_fence();
        deposit();
        wave_lds_fence();
        if (nx < nloc) request(nx);                                           // in flight during the contraction
        const long long g0 = (begin + i) * (long long)mel.n_mels;
        const int am = (int)(g0 & 3);
        lane_mel_contract<S, 64, FLY>(srow, n_freqs, mlo, mwl, lane, mel, mbuf + am);
        wave_lds_fence();
        lane_mel_store<1>(mbuf + am, am, mel.n_mels, mel.out + g0, lane);
        i = nx;
    }
}

template <int PMODE, int S, int CHUNKS>
static int launch_stretch_mel(const StretchArgs& a, const LaneMel& mel, unsigned* flags, hipStream_t stream) {
    // twelve waves per workgroup (eight for the wide rows), one workgroup per CU: the second source row's chunks in flight take the
    // registers that let fb_lanes_kernel run sixteen (~150 VGPRs here: three waves per SIMD); the packed layout depends on the steps
    // in flight only, which stay fbl_fly()
    constexpr int WAVES = CHUNKS == FBL_CHUNKS_WIDE ? 8 : 12, FLY = CHUNKS == FBL_CHUNKS_WIDE ? 16 : 8;
    const size_t bytes = (size_t)WAVES * (fbl_pitch(a.n_freqs) + LM_MAX_MELS + 4) * sizeof(float) + 16 + lm_lds_bytes(64, mel.wtot);
    if (bytes > 160 * 1024) return TAC_E_UNSUPPORTED;
    const long long total = a.rows * a.n_out;
    if (total >= 0x7fffffffLL) return TAC_E_UNSUPPORTED;
    return launch_kernel(stretch_mel_kernel<PMODE, S, CHUNKS, WAVES, FLY>, persistent_blocks(total, WAVES, device_cu_count()), WAVES * 64,
                         bytes, stream, a, mel, flags);
}

template <int S, int CHUNKS>
static int launch_stretch_mel_pow(const StretchArgs& a, const LaneMel& mel, unsigned* flags, hipStream_t stream) {
    // wide rows (fft_length 4096) under banks of very short bands: 72 registers of source chunks next to eight slots in flight do not
    // fit the register file — the rows form and the standalone filterbank kernel take those
    if constexpr (CHUNKS == FBL_CHUNKS_WIDE && S < 10) return TAC_E_UNSUPPORTED;
    else {
    if (a.power == 1.0f) return launch_stretch_mel<1, S, CHUNKS>(a, mel, flags, stream);
    if (a.power == 2.0f) return launch_stretch_mel<2, S, CHUNKS>(a, mel, flags, stream);
    return launch_stretch_mel<0, S, CHUNKS>(a, mel, flags, stream);
    }
}

// ---------------------------------------------------------------- adjoint of the rows form: a gather per source frame
// grad_mag[r][t][f] = sum_j w_j(t) * power * mag_j[f]^(power - 1) * grad_out[r][j][f] over the outputs j that read frame t:
// idx0[j] == t (weight 1 - alpha_j, partner frame t + 1) or idx0[j] == t - 1 (weight alpha_j, partner frame t - 1)
template <int PMODE, class V>
__device__ __forceinline__ void sn_bwd_column(const StretchArgs& a, const float* base, const float* gobase, float* gmbase, int t,
                                              int f, int jlo, int jhi) {
    using L = sn_lanes<V>;
    auto frame = [&](int s) -> V {
        return (s >= 0 && s < a.n_frames) ? *reinterpret_cast<const V*>(base + (long long)s * a.stride_t + f) : L::zero();
    };
    const V mp = frame(t - 1), mc = frame(t), mn = frame(t + 1);
    V acc = L::zero();
    for (int j = jlo; j < jhi; ++j) {
        const int s = a.idx0[j];
        if (s != t && s != t - 1) continue;
        const float al = a.alpha[j];
        const bool first = s == t;                                            // frame t is the output's FIRST source frame
        const V go = *reinterpret_cast<const V*>(gobase + (long long)j * a.n_freqs + f);
#pragma unroll
        for (int i = 0; i < L::N; ++i) {
            const float v = first ? sn_blend(L::get(mc, i), L::get(mn, i), al) : sn_blend(L::get(mp, i), L::get(mc, i), al);
            const float g = sn_dpow<PMODE>(v, a.power) * L::get(go, i);
            L::set(acc, i, L::get(acc, i) + (first ? 1.0f - al : al) * g);
        }
    }
    *reinterpret_cast<V*>(gmbase + (long long)t * a.n_freqs + f) = acc;
}

template <int PMODE>
__global__ void __launch_bounds__(SN_THREADS)
stretch_bwd_kernel(StretchArgs a, const int* __restrict__ bounds, const float* __restrict__ grad_out, float* __restrict__ grad_mag) {
    const long long r = blockIdx.x / a.n_frames;
    const int t = (int)(blockIdx.x - r * a.n_frames);
    int jlo = t > 0 ? bounds[t - 1] : bounds[0];
    int jhi = bounds[t + 1];
    jlo = jlo < 0 ? 0 : jlo;
    jhi = jhi > a.n_out ? a.n_out : jhi;
    const float* base = a.mag + r * a.stride_r;
    const float* gobase = grad_out + r * (long long)a.n_out * a.n_freqs;
    float* gmbase = grad_mag + r * (long long)a.n_frames * a.n_freqs;
    const int nfull = a.n_freqs >> 2;
    for (int c = threadIdx.x; c < nfull; c += SN_THREADS) sn_bwd_column<PMODE, sn_f4>(a, base, gobase, gmbase, t, 4 * c, jlo, jhi);
    if ((int)threadIdx.x < (a.n_freqs & 3)) sn_bwd_column<PMODE, float>(a, base, gobase, gmbase, t, 4 * nfull + threadIdx.x, jlo, jhi);
}

static int stretch_args(StretchArgs* a, const float* mag, int64_t rows, int32_t n_freqs, int64_t n_frames, int64_t stride_r,
                        int64_t stride_t, const int32_t* idx0, const float* alpha, int64_t n_out, float power, int db, float db_ref,
                        float db_amin) {
    if (!mag || !idx0 || !alpha) return TAC_E_INVALID;
    if (rows <= 0 || n_freqs <= 0 || n_frames <= 0 || n_out <= 0) return TAC_E_INVALID;
    if (n_frames >= 0x7fffffffLL || n_out >= 0x7f7f7f7fLL || rows * n_out >= 0x7fffffffLL || rows * n_frames >= 0x7fffffffLL)
        return TAC_E_UNSUPPORTED;
    if (stride_t < n_freqs || (rows > 1 && stride_r < 0)) return TAC_E_INVALID;
    if (db && !(db_ref > 0.0f)) return TAC_E_INVALID;
    *a = StretchArgs{mag, (long long)rows, (int)n_freqs, (int)n_frames, rows > 1 ? (long long)stride_r : 0, (long long)stride_t, idx0,
                     alpha, (int)n_out, power, db ? 1 : 0, db_amin, db ? log10f(db_ref) : 0.0f};
    return TAC_OK;
}

}  // namespace tac

extern "C" {

int tac_stretch_norm_f32(const float* mag, int64_t rows, int32_t n_freqs, int64_t n_frames, int64_t stride_r, int64_t stride_t,
                         const int32_t* idx0, const float* alpha, int64_t n_out, float power, int db, float db_ref, float db_amin,
                         float* out, int32_t* flags, void* stream) {
    using namespace tac;
    if (rows == 0 || n_out == 0) return TAC_OK;
    if (!out || !flags) return TAC_E_INVALID;
    StretchArgs a;
    const int rc = stretch_args(&a, mag, rows, n_freqs, n_frames, stride_r, stride_t, idx0, alpha, n_out, power, db, db_ref, db_amin);
    if (rc != TAC_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    unsigned* fl = reinterpret_cast<unsigned*>(flags);
    TAC_HIP(hipMemsetAsync(fl, 0x7f, (size_t)rows * sizeof(unsigned), s));
    // spans of up to 32 output frames (a span re-reads at most two source frames its neighbour read too), shorter while that leaves
    // CUs without a workgroup
    int span = 32;
    while (span > 4 && rows * ((n_out + span - 1) / span) < 2LL * device_cu_count()) span >>= 1;
    const long long spans = (n_out + span - 1) / span;
    if (rows * spans >= 0x7fffffffLL) return TAC_E_UNSUPPORTED;
    const int lrc = launch_kernel(power == 1.0f ? stretch_rows_kernel<1> : (power == 2.0f ? stretch_rows_kernel<2> : stretch_rows_kernel<0>),
                                  rows * spans, SN_THREADS, 0, s, a, out, fl, span, (int)spans);
    if (lrc != TAC_OK) return lrc;
    return launch_kernel(stretch_rows_fixup_kernel, rows, SN_THREADS, 0, s, a, out, fl);
}

int tac_stretch_mel_f32(const float* mag, int64_t rows, int32_t n_freqs, int64_t n_frames, int64_t stride_r, int64_t stride_t,
                        const int32_t* idx0, const float* alpha, int64_t n_out, float power, const float* wpack, const int32_t* desc,
                        const int32_t* info_host, int32_t n_mels, int db, float db_ref, float db_amin, float* out, int32_t* flags,
                        void* stream) {
    using namespace tac;
    if (rows == 0 || n_out == 0) return TAC_OK;
    if (!out || !flags || !wpack || !desc || !info_host || n_mels <= 0) return TAC_E_INVALID;
    StretchArgs a;
    const int rc = stretch_args(&a, mag, rows, n_freqs, n_frames, stride_r, stride_t, idx0, alpha, n_out, power, db, db_ref, db_amin);
    if (rc != TAC_OK) return rc;
    if (info_host[2] != LM_MARK + 64) return TAC_E_UNSUPPORTED;                    // the tile kernel's layout: rows form + filterbank
    if (!lane_mel_info_ok(info_host, 64, fbl_fly(n_freqs), LM_MAX_STEPS_WAVE)) return TAC_E_INVALID;
    const int chunks = (n_freqs + 3) / 4;
    if (n_mels < LM_MIN_MELS || n_mels > LM_MAX_MELS || n_freqs < 8 || chunks > FBL_CHUNKS_WIDE * 64) return TAC_E_UNSUPPORTED;
    const LaneMel lm{wpack, desc, info_host[1], info_host[0], n_mels, a.db, a.amin, a.log10_ref, out, info_host[5] ? 1 : 0};
    hipStream_t s = (hipStream_t)stream;
    unsigned* fl = reinterpret_cast<unsigned*>(flags);
    TAC_HIP(hipMemsetAsync(fl, 0x7f, (size_t)rows * sizeof(unsigned), s));
    const bool wide = chunks > FBL_CHUNKS * 64;
    int lrc = TAC_E_INVALID;
    switch (info_host[4]) {
#define TAC_SM_CASE(SS)                                                                                      \
    case SS:                                                                                                 \
        lrc = wide ? launch_stretch_mel_pow<SS, FBL_CHUNKS_WIDE>(a, lm, fl, s) : launch_stretch_mel_pow<SS, FBL_CHUNKS>(a, lm, fl, s); \
        break;
        TAC_SM_CASE(2) TAC_SM_CASE(4) TAC_SM_CASE(6) TAC_SM_CASE(8) TAC_SM_CASE(10) TAC_SM_CASE(12) TAC_SM_CASE(14)
        TAC_SM_CASE(16) TAC_SM_CASE(18) TAC_SM_CASE(20) TAC_SM_CASE(22) TAC_SM_CASE(24) TAC_SM_CASE(26) TAC_SM_CASE(28)
        TAC_SM_CASE(30) TAC_SM_CASE(32) TAC_SM_CASE(34) TAC_SM_CASE(36)
#undef TAC_SM_CASE
        default: return TAC_E_INVALID;
    }
    if (lrc != TAC_OK) return lrc;
    return launch_kernel(stretch_mel_fixup_kernel, rows, SN_THREADS, 0, s, a, out, (int)n_mels, fl);
}

int tac_stretch_norm_backward_f32(const float* mag, int64_t rows, int32_t n_freqs, int64_t n_frames, int64_t stride_r,
                                  int64_t stride_t, const int32_t* idx0, const float* alpha, const int32_t* bounds, int64_t n_out,
                                  float power, const float* grad_out, float* grad_mag, void* stream) {
    using namespace tac;
    if (rows == 0 || n_frames == 0) return TAC_OK;
    if (!bounds || !grad_out || !grad_mag) return TAC_E_INVALID;
    StretchArgs a;
    const int rc = stretch_args(&a, mag, rows, n_freqs, n_frames, stride_r, stride_t, idx0, alpha, n_out, power, 0, 1.0f, 1e-7f);
    if (rc != TAC_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    return launch_kernel(power == 1.0f ? stretch_bwd_kernel<1> : (power == 2.0f ? stretch_bwd_kernel<2> : stretch_bwd_kernel<0>),
                         rows * n_frames, SN_THREADS, 0, s, a, bounds, grad_out, grad_mag);
}

}  // extern "C"
