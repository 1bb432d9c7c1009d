// cmn_deltas.hip — functional.sliding_window_cmn (Kaldi's apply-cmvn-sliding) and functional.compute_deltas, each ONE streaming launch,
// and their adjoints (the gradients) as a mode of the same kernels.
//
// sliding_cmn_kernel, (rows, T, F) with any positive element strides.  The window of frame t is [ws(t), we(t)) (cmn_bounds below, the
// closed form of Kaldi's step-by-step procedure); both bounds are non-decreasing in t.
//   lanes run along f (the unit stride of what kaldi_fbank returns): a wave holds 64 / FL time chunks of FL features each, FL the
//   one of 64 / 32 / 16 that wastes the fewest lanes on F (80 features: FL = 16, four neighbouring feature blocks of one chunk in a
//   wave, 256 contiguous bytes per load)
//   a thread owns ONE feature over ONE chunk of `chunk` consecutive frames (the host's choice, tac_sliding_cmn_chunk): it sums the
//   window of its first frame directly, then moves the two window ends frame by frame: add the frames that enter, take out the
//   frames that leave
//   state: float64 sum and sum of squares over the FINITE samples of the window and an integer count of its non-finite ones, so a
//   NaN or an infinity makes exactly the frames whose window holds it NaN and leaves no trace in the sums once it has left
//   out[t] = x[t] - sum / n (times (sumsq / n - mean^2)^-1/2 with norm_vars, 0 where n == 1), in float64, rounded to float32 once
//   (1 / n is a float64 reciprocal, recomputed when n changes: two more float64 roundings of the mean)
// Every load of a sample is followed by at most two float64 additions to a sum of at most n terms, so a chunk of L frames puts at
// most 2 L float64 roundings of n-frame-sized sums into a mean: 2 L 2^-53 max|x| (L <= 2^14 here: under 2^-38 max|x|).
// The adjoint (norm_vars off): g_x[s] = g[s] - sum over {t : ws(t) <= s < we(t)} of g[t] / n(t).  Those t are the interval
// [lo(s), hi(s)), lo(s) the first t with we(t) > s and hi(s) the first with ws(t) > s — found by bisection for the chunk's first
// frame and moved forward from there: the same sliding sum over g[t] / n(t).
//
// deltas_kernel, (rows, F, T) with any positive element strides, out dense (rows, F, T):
//   out[t] = (sum_{k = -n .. n} k x[idx(t + k)]) / denom,   denom = n (n + 1)(2n + 1) / 3,   n <= 32
// idx is the index map of torch's pad for 'replicate' / 'constant' / 'reflect' / 'circular'.  A workgroup stages a tile of FT
// features x (TT + 2n) frames in the LDS through idx (so every sample is read from memory once per tile), then each thread runs the
// chain fmaf(k, x, acc) in ascending k over its outputs, lanes along t, and divides once: coalesced dense stores.  Two load forms:
//   lanes along t  (stride_t == 1, and every layout that has no unit stride)     tile 16 x 256
//   lanes along f  (stride_f == 1: the transposed view of a (T, F) Kaldi matrix)  tile 64 x 64, turned through the LDS (rows of odd
//                  pitch: the column writes of the load and the row reads of the chain are both free of bank conflicts)
// The adjoint ('replicate' and 'constant'): the 'constant' form with the taps negated, and for 'replicate' the two edge outputs
// s = 0 and s = T - 1 also collect what the clamped reads sent them, sum_{t < n} g[t] (S(n) - S(t)) with S(m) = m (m + 1) / 2 and
// its mirror image; those two outputs are accumulated in float64.
// One writer per element, no atomics, no workspace: bit-identical from run to run.
#include <math.h>

#include "host_common.hpp"

namespace tac {

constexpr int CMN_THREADS = 256;
constexpr long long CMN_MAX_CHUNK = 1 << 14;
constexpr long long CMN_MAX_WINDOW = 1LL << 40;             // rows and windows beyond it are refused / capped: int64 sums stay exact
constexpr long long CMN_FILL_THREADS = 256LL * 512;      // two workgroups of 256 threads on each of the 256 CUs

struct CmnGeom {
    long long T, F, W, minw;
    int center;
};

// the window [ws, we) of frame t: 0 <= ws < we <= T for 0 <= t < T
__host__ __device__ __forceinline__ void cmn_bounds(const CmnGeom& g, long long t, long long& ws, long long& we) {
    if (g.center) {
        long long a = t - g.W / 2;
        a = a < 0 ? 0 : a;
        const long long cap = g.T - g.W > 0 ? g.T - g.W : 0;
        ws = a < cap ? a : cap;
        we = ws + g.W < g.T ? ws + g.W : g.T;
    } else {
        ws = t - g.W > 0 ? t - g.W : 0;
        we = t + 1 > g.minw ? t + 1 : g.minw;
        if (we > g.T) {
            ws -= we - g.T;
            ws = ws < 0 ? 0 : ws;
            we = g.T;
        }
    }
}

__device__ __forceinline__ bool cmn_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct CmnState {
    double sum, sq;
    int bad;
};

// one sample enters (SIGN = 1) or leaves (SIGN = -1) the sums where `on`; no branch, so that an unrolled loop issues its loads together
template <bool VARS, int SIGN>
__device__ __forceinline__ void cmn_take(CmnState& s, float v, bool on) {
    const bool fin = cmn_finite(v);
    const double d = on && fin ? (double)v : 0.0;
    s.bad += on && !fin ? SIGN : 0;
    s.sum += SIGN > 0 ? d : -d;
    if constexpr (VARS) s.sq += SIGN > 0 ? d * d : -(d * d);
}

// the adjoint's term of frame j, g[j] / n(j)
__device__ __forceinline__ void cmn_take_adjoint(CmnState& s, const float* p, long long stride_t, const CmnGeom& g, long long j, int sign) {
    const float v = p[j * stride_t];
    if (!cmn_finite(v)) {
        s.bad += sign;
        return;
    }
    long long ws, we;
    cmn_bounds(g, j, ws, we);
    const double d = (double)v / (double)(we - ws);
    s.sum += sign > 0 ? d : -d;
}

template <bool ADJ, bool VARS>
__global__ void __launch_bounds__(CMN_THREADS)
sliding_cmn_kernel(const float* __restrict__ x, long long rows, CmnGeom g, long long stride_r, long long stride_t, long long stride_f,
                   long long chunk, long long n_chunks, int fl_log, long long n_fb, float* __restrict__ out) {
    const long long id = (long long)blockIdx.x * CMN_THREADS + threadIdx.x;
    long long slot = id >> fl_log;
    const long long f = (slot % n_fb << fl_log) + (id & ((1 << fl_log) - 1));
    slot /= n_fb;
    const long long ch = slot % n_chunks, row = slot / n_chunks;
    if (row >= rows || f >= g.F) return;
    const float* p = x + row * stride_r + f * stride_f;
    float* o = out + row * g.T * g.F + f;
    const long long c0 = ch * chunk;
    const long long c1 = c0 + chunk < g.T ? c0 + chunk : g.T;

    // the interval [lo, hi) whose terms the first frame of the chunk sums
    long long lo, hi;
    if constexpr (ADJ) {
        long long a = 0, b = g.T;                   // lo: the first t with we(t) > c0 (t = c0 is one: the answer is in [0, c0])
        while (a < b) {
            const long long m = (a + b) >> 1;
            long long ws, we;
            cmn_bounds(g, m, ws, we);
            if (we > c0) b = m; else a = m + 1;
        }
        lo = a;
        a = c0;                                     // hi: the first t with ws(t) > c0, or T
        b = g.T;
        while (a < b) {
            const long long m = (a + b) >> 1;
            long long ws, we;
            cmn_bounds(g, m, ws, we);
            if (ws > c0) b = m; else a = m + 1;
        }
        hi = a;
    } else {
        cmn_bounds(g, c0, lo, hi);
    }
    CmnState s{0.0, 0.0, 0};
    if constexpr (ADJ) {
        for (long long j = lo; j < hi; ++j) cmn_take_adjoint(s, p, stride_t, g, j, 1);
        for (long long t = c0; t < c1; ++t) {
            long long ws, we;
            while (hi < g.T) {
                cmn_bounds(g, hi, ws, we);
                if (ws > t) break;
                cmn_take_adjoint(s, p, stride_t, g, hi++, 1);
            }
            while (lo < hi) {
                cmn_bounds(g, lo, ws, we);
                if (we > t) break;
                cmn_take_adjoint(s, p, stride_t, g, lo++, -1);
            }
            const double r = (double)p[t * stride_t] - s.sum;
            o[t * g.F] = s.bad > 0 ? __uint_as_float(0x7fc00000u) : (float)r;
        }
    } else {
#pragma unroll 8
        for (long long j = lo; j < hi; ++j) cmn_take<VARS, 1>(s, p[j * stride_t], true);
        // Both bounds are clamped shifts of t, so from one frame to the next each moves by at most one frame: one predicated
        // sample enters, one leaves (neither at t = c0, whose window is summed already).  The three loads of a frame depend on
        // t alone, not on loaded data: the unrolled loop has those of four frames in flight.
        long long n_prev = 0;
        double rn = 0.0;
#pragma unroll 4
        for (long long t = c0; t < c1; ++t) {
            long long ws, we;
            cmn_bounds(g, t, ws, we);
            const bool enter = hi < we, leave = lo < ws;
            const float v_in = p[(enter ? hi : t) * stride_t];
            const float v_out = p[lo * stride_t];
            const float v = p[t * stride_t];
            cmn_take<VARS, 1>(s, v_in, enter);
            cmn_take<VARS, -1>(s, v_out, leave);
            hi += enter ? 1 : 0;
            lo += leave ? 1 : 0;
            const long long n = hi - lo;
            if (n != n_prev) {
                n_prev = n;
                rn = 1.0 / (double)n;
            }
            const double mean = s.sum * rn;
            double r = (double)v - mean;
            if constexpr (VARS) r = n == 1 ? 0.0 : r * rsqrt(s.sq * rn - mean * mean);
            o[t * g.F] = s.bad > 0 ? __uint_as_float(0x7fc00000u) : (float)r;
        }
    }
}

// lanes per feature block: the one of 64 / 32 / 16 that pads F the least (the widest among equals)
inline int cmn_fl_log(long long F) {
    int best = 6;
    long long waste = ((F + 63) / 64) * 64 - F;
    for (int l = 5; l >= 4; --l) {
        const long long w = ((F + (1LL << l) - 1) >> l << l) - F;
        if (w < waste) {
            waste = w;
            best = l;
        }
    }
    return best;
}

// Frames per thread.  A thread reads its first window (n0 frames) and then three samples per frame (the frame, the one entering,
// the one leaving): `fill` is the chunk that spreads the launch over CMN_FILL_THREADS threads, and a chunk is never under a
// quarter of the first window, so that reading the first windows costs at most 4/3 of the sliding itself; rows long enough to
// fill the device with chunks of a window or more read at most 4/3 of the minimum.  At most CMN_MAX_CHUNK frames (the rounding
// budget of the header), unless the window itself asks for more.
inline long long cmn_chunk(long long rows, long long T, long long F, long long W, long long minw) {
    if (rows < 1 || T < 1 || F < 1) return 1;
    W = W < CMN_MAX_WINDOW ? W : CMN_MAX_WINDOW;            // (a window that long is the whole row: no sum below can overflow)
    minw = minw < CMN_MAX_WINDOW ? minw : CMN_MAX_WINDOW;
    const int l = cmn_fl_log(F);
    const long long lanes = rows * (((F + (1LL << l) - 1) >> l) << l);
    long long want = (CMN_FILL_THREADS + lanes - 1) / lanes;
    want = want < 1 ? 1 : want;
    long long fill = (T + want - 1) / want;
    fill = fill > CMN_MAX_CHUNK ? CMN_MAX_CHUNK : fill;
    const long long n0 = W + 1 > minw ? W + 1 : minw;      // (not clamped to T: the floor is the same for every row length)
    const long long floor_ = (n0 + 3) / 4;
    long long c = fill > floor_ ? fill : floor_;
    return c < 1 ? 1 : c;
}

// ------------------------------------------------------------------------------------------------------------------ deltas
constexpr int DL_THREADS = 256;
constexpr int DL_MAX_N = 32;
enum { DL_REPLICATE = 0, DL_CONSTANT = 1, DL_REFLECT = 2, DL_CIRCULAR = 3 };

// source frame of padded position t (any integer), or -1 for a zero
__device__ __forceinline__ long long dl_index(long long t, long long T, int mode) {
    if (t >= 0 && t < T) return t;
    long long s;
    if (mode == DL_REPLICATE) s = t < 0 ? 0 : T - 1;
    else if (mode == DL_REFLECT) s = t < 0 ? -t : 2 * (T - 1) - t;
    else if (mode == DL_CIRCULAR) s = t < 0 ? t + T : t - T;
    else return -1;
    return s >= 0 && s < T ? s : -1;                // (beyond one fold: only columns no output of the row reads)
}

template <bool ALONG_F>
__global__ void __launch_bounds__(DL_THREADS)
deltas_kernel(const float* __restrict__ x, long long rows, long long F, long long T, long long stride_r, long long stride_f,
              long long stride_t, int n, int mode, int adjoint, long long n_ft, long long n_tt, float* __restrict__ out) {
    constexpr int FT = ALONG_F ? 64 : 16, TT = ALONG_F ? 64 : 256;
    extern __shared__ __attribute__((aligned(16))) float dl_tile[];
    const int cols = TT + 2 * n;
    const int pitch = cols | 1;
    long long b = blockIdx.x;
    const long long t0 = (b % n_tt) * TT;
    b /= n_tt;
    const long long f0 = (b % n_ft) * FT, row = b / n_ft;
    if (row >= rows) return;
    const float* src = x + row * stride_r;
    const int load_mode = adjoint ? DL_CONSTANT : mode;
    const long long t_need = (t0 + TT < T ? t0 + TT : T) + n;          // padded positions at and beyond it are read by no output
    for (int i = threadIdx.x; i < FT * cols; i += DL_THREADS) {
        const int ff = ALONG_F ? i % FT : i / cols;
        const int c = ALONG_F ? i / FT : i % cols;
        const long long tp = t0 - n + c;
        float v = 0.0f;
        if (f0 + ff < F && tp < t_need) {
            const long long s = dl_index(tp, T, load_mode);
            if (s >= 0) v = src[(f0 + ff) * stride_f + s * stride_t];
        }
        dl_tile[ff * pitch + c] = v;
    }
    __syncthreads();
    const float denom = (float)(n * (n + 1) * (2 * n + 1) / 3);
    const float sign = adjoint ? -1.0f : 1.0f;
    for (int i = threadIdx.x; i < FT * TT; i += DL_THREADS) {
        const int ff = i / TT, tt = i % TT;
        const long long f = f0 + ff, t = t0 + tt;
        if (f >= F || t >= T) continue;
        const float* w = dl_tile + ff * pitch + tt;          // w[j] is padded position t - n + j
        float r;
        if (adjoint && mode == DL_REPLICATE && (t == 0 || t == T - 1)) {
            // an edge of the adjoint: the interior taps and what the clamped reads of the forward pass sent here, in float64
            double acc = 0.0;
            for (int k = -n; k <= n; ++k)
                if (k != 0) acc = fma(-(double)k, (double)w[n + k], acc);
            const float* gp = src + f * stride_f;
            const long long m = n < T ? n : T;
            const double sn = 0.5 * n * (n + 1);
            if (t == 0)
                for (long long u = 0; u < m; ++u) acc = fma(-(sn - 0.5 * u * (u + 1)), (double)gp[u * stride_t], acc);
            if (t == T - 1)
                for (long long u = 0; u < m; ++u) acc = fma(sn - 0.5 * u * (u + 1), (double)gp[(T - 1 - u) * stride_t], acc);
            r = (float)(acc / (double)denom);
        } else {
            float acc = 0.0f;
            for (int k = -n; k <= n; ++k)
                if (k != 0) acc = fmaf(sign * (float)k, w[n + k], acc);
            r = acc / denom;
        }
        out[(row * F + f) * T + t] = r;
    }
}

}  // namespace tac

extern "C" {

int64_t tac_sliding_cmn_chunk(int64_t rows, int64_t n_frames, int64_t n_feats, int64_t cmn_window, int64_t min_cmn_window) {
    return tac::cmn_chunk(rows, n_frames, n_feats, cmn_window, min_cmn_window);
}

int tac_sliding_cmn_f32(const float* x, int64_t rows, int64_t n_frames, int64_t n_feats, int64_t stride_r, int64_t stride_t,
                        int64_t stride_f, int64_t cmn_window, int64_t min_cmn_window, int center, int norm_vars, int adjoint,
                        float* out, void* stream) {
    using namespace tac;
    if (!x || !out || rows <= 0 || n_frames <= 0 || n_feats <= 0 || cmn_window < 1 || min_cmn_window < 1) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (n_frames == 1) stride_t = 0;
    if (n_feats == 1) stride_f = 0;
    if ((rows > 1 && stride_r <= 0) || (n_frames > 1 && stride_t <= 0) || (n_feats > 1 && stride_f <= 0)) return TAC_E_INVALID;
    if (adjoint && norm_vars) return TAC_E_UNSUPPORTED;
    if (n_frames > CMN_MAX_WINDOW) return TAC_E_UNSUPPORTED;
    const long long chunk = cmn_chunk(rows, n_frames, n_feats, cmn_window, min_cmn_window);
    // A window of T frames or more and a minimum of 2 T or more give the bounds of those caps (the start is max(. - (M - T), 0) = 0
    // from M = 2 T on), so cmn_bounds never sees a value whose sums could overflow int64
    cmn_window = cmn_window < n_frames ? cmn_window : n_frames;
    min_cmn_window = min_cmn_window < 2 * n_frames ? min_cmn_window : 2 * n_frames;
    const CmnGeom g{(long long)n_frames, (long long)n_feats, (long long)cmn_window, (long long)min_cmn_window, center ? 1 : 0};
    const long long n_chunks = (n_frames + chunk - 1) / chunk;
    const int fl_log = cmn_fl_log(n_feats);
    const long long n_fb = (n_feats + (1LL << fl_log) - 1) >> fl_log;
    const double threads = (double)rows * (double)n_chunks * (double)(n_fb << fl_log);
    if (threads > 2147483647.0 * CMN_THREADS) return TAC_E_UNSUPPORTED;
    const long long blocks = ((long long)threads + CMN_THREADS - 1) / CMN_THREADS;
    auto kern = adjoint ? sliding_cmn_kernel<true, false> : (norm_vars ? sliding_cmn_kernel<false, true> : sliding_cmn_kernel<false, false>);
    return launch_kernel(kern, blocks, CMN_THREADS, 0, (hipStream_t)stream, x, (long long)rows, g, (long long)stride_r,
                         (long long)stride_t, (long long)stride_f, chunk, n_chunks, fl_log, n_fb, out);
}

int tac_deltas_supported(int64_t n_frames, int32_t win_length, int32_t mode, int adjoint) {
    if (win_length < 3 || mode < 0 || mode > 3 || n_frames < 1) return TAC_E_INVALID;
    const int n = (win_length - 1) / 2;
    if (mode == tac::DL_REFLECT && n >= n_frames) return TAC_E_INVALID;
    if (mode == tac::DL_CIRCULAR && n > n_frames) return TAC_E_INVALID;
    if (n > tac::DL_MAX_N) return TAC_E_UNSUPPORTED;
    if (adjoint && mode != tac::DL_REPLICATE && mode != tac::DL_CONSTANT) return TAC_E_UNSUPPORTED;
    return TAC_OK;
}

int tac_deltas_f32(const float* x, int64_t rows, int64_t n_feats, int64_t n_frames, int64_t stride_r, int64_t stride_f,
                   int64_t stride_t, int32_t win_length, int32_t mode, int adjoint, float* out, void* stream) {
    using namespace tac;
    if (!x || !out || rows <= 0 || n_feats <= 0 || n_frames <= 0) return TAC_E_INVALID;
    const int rc = tac_deltas_supported(n_frames, win_length, mode, adjoint);
    if (rc != TAC_OK) return rc;
    if (rows == 1) stride_r = 0;
    if (n_feats == 1) stride_f = 0;
    if (n_frames == 1) stride_t = 0;
    if ((rows > 1 && stride_r <= 0) || (n_feats > 1 && stride_f <= 0) || (n_frames > 1 && stride_t <= 0)) return TAC_E_INVALID;
    const int n = (win_length - 1) / 2;
    const bool along_f = stride_t != 1 && stride_f == 1 && n_feats > 1;
    const int ft = along_f ? 64 : 16, tt = along_f ? 64 : 256;
    const long long n_ft = (n_feats + ft - 1) / ft, n_tt = (n_frames + tt - 1) / tt;
    const double blocks = (double)rows * (double)n_ft * (double)n_tt;
    if (blocks > 2147483647.0) return TAC_E_UNSUPPORTED;
    const size_t bytes = (size_t)ft * ((tt + 2 * n) | 1) * sizeof(float);
    auto kern = along_f ? deltas_kernel<true> : deltas_kernel<false>;
    return launch_kernel(kern, (long long)blocks, DL_THREADS, bytes, (hipStream_t)stream, x, (long long)rows, (long long)n_feats,
                         (long long)n_frames, (long long)stride_r, (long long)stride_f, (long long)stride_t, n, (int)mode,
                         adjoint ? 1 : 0, n_ft, n_tt, out);
}

}  // extern "C"
