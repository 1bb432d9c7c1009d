// pitch.hip — functional.detect_pitch_frequency: the normalised cross-correlation (NCCF) pitch of torchaudio in two launches.
//
// Per row of `time` samples, with F = frame, L = max_lag, N = ceil(time / F) frames and the row continued by zeros:
//     num[t, l]  = sum_{i < F} x[tF + i] x[tF + l + i]                                  l = 1 .. L
//     nccf[t, l] = num / (1e-9 + |s1|)^2 / (1e-9 + |s2(l)|)^2
//     cb = first arg-max over l in [lag_min + 1, L], ch = first arg-max over l in [lag_min + 1, L / 2],
//     lag[t] = ch if nccf[ch] > 0.99 nccf[cb] else cb
// The factor 1 / (1e-9 + |s1|)^2 is positive and the same for every lag of a frame, so neither arg-max nor the 0.99 rule sees it:
// the kernel compares u[l] = num / (1e-9 + |s2(l)|)^2 and never forms it (nor can it overflow for a quiet s1).
//
// Launch 1, pitch_lags_kernel.  A unit is a group of G consecutive frames of one row; a workgroup of 256 lanes stages the unit's span
// of G F + L samples in the LDS (zeros past the row's end by index; any strides and alignment: one 4-byte load a sample), then
//   * builds P[m] = sum of the squares of the span's first m samples, in float64 by a workgroup scan in a fixed order (a non-finite
//     sample counts as 0 there, so that it cannot reach the frames behind it): |s2(l)|^2 = P[a + l + F] - P[a + l] costs two LDS
//     reads a lag instead of F products, and in float64 a quiet frame behind a loud one loses nothing;
//   * deals the tasks (frame g, lag-block pair j) to the lanes, j fastest.  A lag block is four consecutive lags 4 b .. 4 b + 3
//     (lag 0 rides along unused); task j holds blocks j and j + NH, eight accumulators.  The products run in chunks of four
//     samples at 16-byte aligned LDS positions p: one ds_read_b128 of s1 (the same address for every lane of a frame: a
//     broadcast), and per block one new ds_read_b128 — the window x[p + 4 b .. p + 4 b + 7] keeps its upper half for the next
//     chunk — for 32 FMAs: three 16-byte reads (12 LDS cycles a wave) beside 32 VALU instructions, so the VALU, not the LDS,
//     bounds the loop.  Lanes of consecutive j read addresses 16 bytes apart: conflict-free in each group of 16 lanes.  The first
//     and last chunk of a frame are cut to [a, a + F) by predicated FMAs (not by zeroed factors: 0 x NaN would let a sample
//     outside the frame's span in);
//   * divides, keeps the two running arg-maxima (first maximum: strict `>` in ascending lag order) per task, leaves them in an LDS
//     table, and one lane per frame merges the NH entries with the lowest-lag tie rule, applies the 0.99 rule and stores the lag.
//     A NaN never wins a comparison: the lag of a frame with non-finite samples stays in [lag_min + 1, L].
// G comes from pitch_plan(): the largest lane use (G NH tasks on 256 lanes) whose span, prefix and table fit 64 KB.
//
// Launch 2, pitch_smooth_kernel.  A lane per output over an LDS tile of 256 + win_length - 1 lags (the first lag replicated in
// front by index): the lower median by rank counting — the value v with #(< v) <= m < #(<= v), m = (win_length - 1) / 2 — then
// one IEEE division sample_rate / lag.  win_length 1 .. PT_MAX_WIN.
//
// No atomics, one writer per element, fixed summation order: bit-identical from run to run.
#include <math.h>

#include "host_common.hpp"

namespace tac {

constexpr int PT_THREADS = 256;
constexpr int PT_WAVES = PT_THREADS / 64;
constexpr int PT_MAX_G = 32;                  // frames per unit, at most
constexpr int PT_MAX_TASKS = 1024;            // G * NH, at most: the table's entries
constexpr int PT_LDS_BYTES = 64 * 1024;       // what a workgroup may take: two of them per CU and more
constexpr int PT_MAX_WIN = 64;                // launch 2: the longest median window
constexpr int PT_SM_TILE = 256;               // launch 2: outputs per tile

struct PitchPlan {
    int G;            // frames per unit
    int NH;           // tasks per frame: lane j holds lag blocks j and j + NH
    int span_x;       // floats staged (zero-filled past G F + L)
    int span_p;       // doubles of the prefix: G F + L + 1
    int tasks;        // G NH
    int lds_bytes;
};

struct PtBest { float va; int la; float vh; int lh; };      // best over [lag_min + 1, L] and over [lag_min + 1, half]

inline int pt_lds_bytes(int G, int NH, int frame, int max_lag) {
    const long long span_x = (long long)G * frame + 8LL * NH + 8, span_p = (long long)G * frame + max_lag + 1;
    const long long bytes = 8 * span_p + 4 * ((span_x + 3) & ~3LL) + 16LL * G * NH + 8 * PT_WAVES;
    return bytes > (1LL << 30) ? (1 << 30) : (int)bytes;
}

// TAC_OK and the plan, or TAC_E_UNSUPPORTED where one frame's span does not fit
inline int pitch_plan(long long n_frames, int frame, int max_lag, PitchPlan* pl) {
    if (frame < 1 || max_lag < 2 || n_frames < 1 || frame > (1 << 20) || max_lag > (1 << 20)) return TAC_E_UNSUPPORTED;
    const int nb4 = max_lag / 4 + 1;                     // blocks of four lags that cover 0 .. max_lag
    const int NH = (nb4 + 1) / 2;
    int best = 0;
    double best_use = 0.0;
    for (int G = 1; G <= PT_MAX_G && G <= n_frames; ++G) {
        const int tasks = G * NH;
        if (tasks > PT_MAX_TASKS || pt_lds_bytes(G, NH, frame, max_lag) > PT_LDS_BYTES) break;
        const double use = (double)tasks / (double)(((tasks + PT_THREADS - 1) / PT_THREADS) * PT_THREADS);
        if (use > best_use + 1e-9) best = G, best_use = use;
    }
    if (!best) return TAC_E_UNSUPPORTED;
    pl->G = best;
    pl->NH = NH;
    pl->span_x = best * frame + 8 * NH + 8;
    pl->span_p = best * frame + max_lag + 1;
    pl->tasks = best * NH;
    pl->lds_bytes = pt_lds_bytes(best, NH, frame, max_lag);
    return TAC_OK;
}

struct PitchArgs {
    const float* x;
    long long n0, n1, time, stride_0, stride_1, stride_t;      // rows = n0 * n1: row r starts at (r / n1) stride_0 + (r % n1) stride_1
    long long n_frames, groups, units;                          // groups of G frames per row; units = rows * groups
    int frame, max_lag, lag_min, half;
    int G, NH, span_x, span_p;
    int* lags;                                                  // [rows][n_frames]
};

__device__ __forceinline__ double pt_wave_scan(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const double o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// one chunk of four samples at the aligned span position p: acc[b][r] += x[p + c] x[p + c + 4 b + r] for the c of [lo, hi)
template <bool CUT>
__device__ __forceinline__ void pt_chunk(const float* __restrict__ X, int p, int o0, int o1, int lo, int hi, float4& w0, float4& w1,
                                         float (&acc)[8]) {
    const float4 s = *reinterpret_cast<const float4*>(X + p);
    const float4 h0 = *reinterpret_cast<const float4*>(X + p + o0 + 4);
    const float4 h1 = *reinterpret_cast<const float4*>(X + p + o1 + 4);
    const float sv[4] = {s.x, s.y, s.z, s.w};
    const float a0[8] = {w0.x, w0.y, w0.z, w0.w, h0.x, h0.y, h0.z, h0.w};
    const float a1[8] = {w1.x, w1.y, w1.z, w1.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool on = !CUT || (p + c >= lo && p + c < hi);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float n0 = fmaf(sv[c], a0[c + r], acc[r]), n1 = fmaf(sv[c], a1[c + r], acc[4 + r]);
            acc[r] = on ? n0 : acc[r];
            acc[4 + r] = on ? n1 : acc[4 + r];
        }
    }
    w0 = h0;
    w1 = h1;
}

__global__ void __launch_bounds__(PT_THREADS)
pitch_lags_kernel(const PitchArgs A) {
    extern __shared__ __align__(16) unsigned char pt_lds[];
    float* X = reinterpret_cast<float*>(pt_lds);                                     // [span_x rounded up to 4]: 16-byte aligned
    PtBest* table = reinterpret_cast<PtBest*>(X + ((A.span_x + 3) & ~3));            // [G][NH], 16 bytes each
    double* P = reinterpret_cast<double*>(table + A.G * A.NH);                       // [span_p]
    double* wave_sum = P + A.span_p;                                                 // [PT_WAVES]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = A.frame, L = A.max_lag, G = A.G, NH = A.NH;
    const int tasks = G * NH;
    const int n_sq = A.span_p - 1;                                                   // samples under the prefix: G F + L
    const int per = (n_sq + PT_THREADS - 1) / PT_THREADS;

    for (long long u = blockIdx.x; u < A.units; u += gridDim.x) {
        const long long row = u / A.groups, grp = u - row * A.groups;
        const float* xr = A.x + (row / A.n1) * A.stride_0 + (row % A.n1) * A.stride_1;
        const long long s0 = grp * G * (long long)F;                                 // the span's first sample
        // 1. the span, zeros past the row's end and past G F + L
        for (int m = tid; m < A.span_x; m += PT_THREADS) {
            const long long s = s0 + m;
            X[m] = (m < n_sq && s < A.time) ? xr[s * A.stride_t] : 0.0f;
        }
        __syncthreads();
        // 2. P[m] = sum of the first m squares: a lane's run of `per` samples, a scan over the lanes, the run again
        {
            const int b = tid * per;
            double run = 0.0;
            for (int k = 0; k < per; ++k) {
                const int m = b + k;
                if (m < n_sq) {
                    const float v = X[m];
                    run += isfinite(v) ? (double)v * (double)v : 0.0;
                }
            }
            const double inc = pt_wave_scan(run, lane);
            if (lane == 63) wave_sum[wave] = inc;
            __syncthreads();
            double base = inc - run;
            for (int w = 0; w < wave; ++w) base += wave_sum[w];
            if (tid == 0) P[0] = 0.0;
            for (int k = 0; k < per; ++k) {
                const int m = b + k;
                if (m < n_sq) {
                    const float v = X[m];
                    base += isfinite(v) ? (double)v * (double)v : 0.0;
                    P[m + 1] = base;
                }
            }
        }
        __syncthreads();
        // 3. the correlations of (frame g, blocks j and j + NH)
        for (int task = tid; task < tasks; task += PT_THREADS) {
            const int g = task / NH, j = task - g * NH;
            const int a = g * F, end = a + F;
            const int o0 = 4 * j, o1 = 4 * (j + NH);
            float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            int p = a & ~3;
            float4 w0 = *reinterpret_cast<const float4*>(X + p + o0), w1 = *reinterpret_cast<const float4*>(X + p + o1);
            pt_chunk<true>(X, p, o0, o1, a, end, w0, w1, acc);
            p += 4;
#pragma unroll 2
            for (; p + 4 <= end; p += 4) pt_chunk<false>(X, p, o0, o1, a, end, w0, w1, acc);
            if (p < end) pt_chunk<true>(X, p, o0, o1, a, end, w0, w1, acc);
            PtBest best{-INFINITY, 0x7fffffff, -INFINITY, 0x7fffffff};
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int lag = (q < 4 ? o0 : o1) + (q & 3);
                if (lag > A.lag_min && lag <= L) {
                    const float e2 = (float)(P[a + lag + F] - P[a + lag]);
                    const float n2 = 1e-9f + sqrtf(e2);
                    const float v = acc[q] / (n2 * n2);
                    if (v > best.va) best.va = v, best.la = lag;
                    if (lag <= A.half && v > best.vh) best.vh = v, best.lh = lag;
                }
            }
            table[task] = best;
        }
        __syncthreads();
        // 4. a lane per frame: the lowest lag among equal maxima, the 0.99 rule
        if (tid < G) {
            const long long t = grp * G + tid;
            if (t < A.n_frames) {
                float va = -INFINITY, vh = -INFINITY;
                int la = A.lag_min + 1, lh = A.lag_min + 1;
                for (int j = 0; j < NH; ++j) {
                    const PtBest b = table[tid * NH + j];
                    if (b.va > va || (b.va == va && b.la < la)) va = b.va, la = b.la;
                    if (b.vh > vh || (b.vh == vh && b.lh < lh)) vh = b.vh, lh = b.lh;
                }
                A.lags[row * A.n_frames + t] = (vh > 0.99f * va) ? lh : la;
            }
        }
        __syncthreads();
    }
}

struct SmoothArgs {
    const int* lags;           // [rows][n_frames]
    float* out;                // [rows][n_out]
    long long rows, n_frames, n_out, tiles, units;
    int win, pad;
    float sample_rate;
};

__global__ void __launch_bounds__(PT_SM_TILE)
pitch_smooth_kernel(const SmoothArgs A) {
    __shared__ int S[PT_SM_TILE + PT_MAX_WIN];
    const int tid = threadIdx.x;
    const int W = A.win, mid = (W - 1) / 2;
    for (long long u = blockIdx.x; u < A.units; u += gridDim.x) {
        const long long row = u / A.tiles, t0 = (u - row * A.tiles) * PT_SM_TILE;
        const int* in = A.lags + row * A.n_frames;
        long long left = A.n_out - t0;
        const int n = left < PT_SM_TILE ? (int)left : PT_SM_TILE;
        for (int k = tid; k < n + W - 1; k += PT_SM_TILE) {
            const long long src = t0 + k - A.pad;                      // padded[t0 + k]; at most n_frames - 1
            S[k] = in[src < 0 ? 0 : src];
        }
        __syncthreads();
        if (tid < n) {
            int med = S[tid];
            for (int i = 0; i < W; ++i) {
                const int v = S[tid + i];
                int lt = 0, le = 0;
                for (int k = 0; k < W; ++k) {
                    const int w = S[tid + k];
                    lt += w < v;
                    le += w <= v;
                }
                if (lt <= mid && mid < le) med = v;
            }
            A.out[row * A.n_out + t0 + tid] = A.sample_rate / (float)med;
        }
        __syncthreads();
    }
}

inline int pitch_launch_lags(const float* waveform, int64_t n0, int64_t n1, int64_t time, int64_t stride_0, int64_t stride_1,
                             int64_t stride_t, int32_t frame, int32_t max_lag, int32_t lag_min, int32_t* lags, hipStream_t stream) {
    if (!waveform || !lags || n0 <= 0 || n1 <= 0 || time <= 0 || frame <= 0 || max_lag <= 0 || lag_min <= 0) return TAC_E_INVALID;
    if (lag_min >= max_lag / 2) return TAC_E_INVALID;                              // the range [lag_min, half) of columns is empty
    if (n0 == 1) stride_0 = 0;
    if (n1 == 1) stride_1 = 0;
    if (time == 1) stride_t = 1;
    if ((n0 > 1 && stride_0 <= 0) || (n1 > 1 && stride_1 <= 0) || stride_t <= 0) return TAC_E_INVALID;
    const long long n_frames = (time + frame - 1) / frame;
    PitchPlan pl;
    const int rc = pitch_plan(n_frames, frame, max_lag, &pl);
    if (rc != TAC_OK) return rc;
    PitchArgs A;
    A.x = waveform;
    A.n0 = n0, A.n1 = n1, A.time = time, A.stride_0 = stride_0, A.stride_1 = stride_1, A.stride_t = stride_t;
    A.n_frames = n_frames;
    A.groups = (n_frames + pl.G - 1) / pl.G;
    A.units = (long long)n0 * n1 * A.groups;
    A.frame = frame, A.max_lag = max_lag, A.lag_min = lag_min, A.half = max_lag / 2;
    A.G = pl.G, A.NH = pl.NH, A.span_x = pl.span_x, A.span_p = pl.span_p;
    A.lags = lags;
    long long per_cu = 160 * 1024 / pl.lds_bytes;                                  // workgroups a CU's LDS holds, 8 at the most
    per_cu = per_cu > 8 ? 8 : per_cu;
    const long long blocks = persistent_blocks(A.units, 1, (long long)device_cu_count() * per_cu);
    return launch_kernel(pitch_lags_kernel, blocks, PT_THREADS, (size_t)pl.lds_bytes, stream, A);
}

inline long long pitch_out_frames(long long n_frames, int win) { return n_frames + (win - 1) / 2 - win + 1; }

inline int pitch_launch_smooth(const int32_t* lags, int64_t rows, int64_t n_frames, int32_t win_length, int32_t sample_rate, float* out,
                               hipStream_t stream) {
    if (!lags || !out || rows <= 0 || n_frames <= 0 || win_length < 1 || sample_rate <= 0) return TAC_E_INVALID;
    if (win_length > PT_MAX_WIN) return TAC_E_UNSUPPORTED;
    const long long n_out = pitch_out_frames(n_frames, win_length);
    if (n_out < 1) return TAC_E_SHORT_INPUT;
    SmoothArgs A;
    A.lags = lags, A.out = out, A.rows = rows, A.n_frames = n_frames, A.n_out = n_out;
    A.tiles = (n_out + PT_SM_TILE - 1) / PT_SM_TILE;
    A.units = rows * A.tiles;
    A.win = win_length, A.pad = (win_length - 1) / 2;
    A.sample_rate = (float)sample_rate;
    const long long blocks = persistent_blocks(A.units, 1, (long long)device_cu_count() * 8);
    return launch_kernel(pitch_smooth_kernel, blocks, PT_SM_TILE, 0, stream, A);
}

}  // namespace tac

extern "C" {

int32_t tac_pitch_max_win(void) { return tac::PT_MAX_WIN; }

int tac_pitch_plan(int64_t n_frames, int32_t frame, int32_t max_lag, int32_t* group, int32_t* lds_bytes) {
    tac::PitchPlan pl;
    const int rc = tac::pitch_plan(n_frames, frame, max_lag, &pl);
    if (rc != TAC_OK) return rc;
    if (group) *group = pl.G;
    if (lds_bytes) *lds_bytes = pl.lds_bytes;
    return TAC_OK;
}

int tac_pitch_lags_f32(const float* waveform, int64_t n0, int64_t n1, int64_t time, int64_t stride_0, int64_t stride_1, int64_t stride_t,
                       int32_t frame, int32_t max_lag, int32_t lag_min, int32_t* lags, void* stream) {
    return tac::pitch_launch_lags(waveform, n0, n1, time, stride_0, stride_1, stride_t, frame, max_lag, lag_min, lags, (hipStream_t)stream);
}

int tac_pitch_smooth_i32(const int32_t* lags, int64_t rows, int64_t n_frames, int32_t win_length, int32_t sample_rate, float* out,
                         void* stream) {
    return tac::pitch_launch_smooth(lags, rows, n_frames, win_length, sample_rate, out, (hipStream_t)stream);
}

int tac_pitch_frequency_f32(const float* waveform, int64_t n0, int64_t n1, int64_t time, int64_t stride_0, int64_t stride_1,
                            int64_t stride_t, int32_t sample_rate, int32_t frame, int32_t max_lag, int32_t lag_min, int32_t win_length,
                            int32_t* lags, float* out, void* stream) {
    using namespace tac;
    if (!waveform || !lags || !out || win_length < 1 || sample_rate <= 0 || time <= 0 || frame <= 0) return TAC_E_INVALID;
    if (win_length > PT_MAX_WIN) return TAC_E_UNSUPPORTED;
    const long long n_frames = (time + frame - 1) / frame;
    if (pitch_out_frames(n_frames, win_length) < 1) return TAC_E_SHORT_INPUT;
    const int rc = pitch_launch_lags(waveform, n0, n1, time, stride_0, stride_1, stride_t, frame, max_lag, lag_min, lags, (hipStream_t)stream);
    if (rc != TAC_OK) return rc;
    return pitch_launch_smooth(lags, n0 * n1, n_frames, win_length, sample_rate, out, (hipStream_t)stream);
}

}  // extern "C"
