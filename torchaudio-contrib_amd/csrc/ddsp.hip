// ddsp.hip — the differentiable-DSP pair of torchaudio.prototype.functional: oscillator_bank and filter_waveform, with their gradients.
//
// ---------------------------------------------------------------- oscillator_bank
//   y[t, n] = a'[t, n] sin phi[t, n],   phi[t] = sum_{u <= t} (2 pi f[u] / sr mod 2 pi),   a' = 0 where |f| >= sr / 2
//
// The phase is a 64-bit PHASE ACCUMULATOR in turns (the NCO of a direct digital synthesiser): the increment frac(f / sr) is formed in
// float64 and stored as an unsigned integer in units of 2^-64 turns.  Integer addition wraps at one period by itself, is exact and is
// associative: however the time axis is cut into chunks, tiles and spans, every cell sees the same 64 bits, so the forward result does
// not depend on the partition, on the grid or on what else the batch holds.  The error of phi[t] is the (t + 1) roundings of the
// increments (2^-63 turns each: the division's rounding is recovered from its exact remainder) and nothing from the sum.  sin and cos come from the accumulator's top two bits
// (the quadrant, exact) and a float64 polynomial on the rest (|theta| <= pi / 4): the result is rounded to float32 once.
//
// ONE kernel template in four modes.  A workgroup owns a (row, span) unit: a span is the whole row where rows are plentiful, OB_SPAN
// steps otherwise (so that 2 rows of 960000 steps are 938 units, not 2).  It walks the span in tiles of OB_TILE = 256 steps, and a
// tile in groups of OB_NG = 16 oscillators:
//   global -> LDS    the (256 x 16) sub-tile of f and a (and g), in the order of the contiguous axis of the tensor (N-contiguous or
//                    time-contiguous, any positive strides), stored time-major per oscillator, skewed by one float per chunk
//   lane             a half-wave of 32 lanes owns one oscillator; a lane owns OB_C = 8 consecutive steps: increments, their total
//   scan             five cross-lane steps over the 32 chunk totals (integer adds), the tile's incoming phase from the LDS carry
//   forward          sin, product; 'none' goes back through the LDS for N-contiguous stores; 'sum' / 'mean' put float64 products in the
//                    LDS and one lane per step adds the 16 oscillators in index order into a float64 register kept across the groups
//   backward         the tiles are walked from the END of the span: the phase at a tile's start is (phase at its end) - (tile total),
//                    exact in integers; w = g a' cos phi is suffix-summed in float64 (in the chunk, across the lanes, plus the carry of
//                    everything later in the row), d a = g sin phi; both go back through the LDS
//   MODE 0           the spans' increment totals           -> ws_inc[row][span][n]     (forward with more than one span; backward always)
//   MODE 1           forward; the span's incoming phase is the integer sum of the earlier spans' totals, split over the half-wave
//   MODE 2           the spans' totals of w (backward with more than one span)         -> ws_w[row][span][n]
//   MODE 3           backward; incoming: phase at the span's end (sum of totals up to it) and the float64 sum of the later spans' w
// No atomics; one writer per element; every float64 sum has a fixed order that depends on the shape alone.
//
// ---------------------------------------------------------------- filter_waveform
//   y[t] = full[t + s],  full[n] = sum_k h_{(n - k) / C}[k] x[n - k]       (C = ceil(T / F) samples per filter, x zero-extended)
//
// forward: a workgroup owns FW_TILE = 1024 outputs of a row; a lane FW_PER = 4 consecutive ones.  The input span [t0 + s - K + 1,
//   t0 + 1024 + s) is staged once (zeros outside [0, T) by index).  The chunks j that intersect the span are walked in order; h_j is
//   staged once per chunk into one of two LDS buffers while the arithmetic reads the other.  Inside a chunk every lane runs the SAME
//   tap index k (h[k] is one broadcast LDS read) over the taps that can reach the wave's 256 outputs from that chunk, with a sliding
//   window of four x values in registers: per tap one new x read (zeroed by comparison where the sample belongs to another chunk),
//   one h read and four fused multiply-adds.  Samples of other chunks contribute exact zeros, so the chain's roundings are K at most.
//   Correct for every C >= 1; fast where C is not far below the wave's 256 outputs (the cost factor is about 1 + 256 / C).
// d x:  d x[m] = sum_k h_{m / C}[k] g[m - s + k]: the same scheme as a correlation — the g span staged, a window sliding the other way,
//   a lane keeps a chunk's sum only for its own chunk's samples.
// d h:  d h_j[k] = sum_{m in chunk j, m < T} x[m] g[m - s + k]: a workgroup per (row, chunk, piece of FW_PIECE samples); x piece and g
//   span in the LDS, a lane per tap (three taps per lane: FW_MAX_TAPS = 768), x[m] broadcast, g conflict-free.  Per-piece, per-row
//   partial sums are written; the caller adds pieces and sharing rows with one torch.sum (fixed order, no atomics).
#include <math.h>

#include "host_common.hpp"

namespace tac {

// ============================================================================= oscillator_bank
constexpr int OB_C = 8;                         // steps per lane
constexpr int OB_TL = 32;                       // lanes along time: a half-wave per oscillator
constexpr int OB_TILE = OB_C * OB_TL;           // 256 steps
constexpr int OB_NG = 16;                       // oscillators per group
constexpr int OB_THREADS = OB_TL * OB_NG;       // 512
constexpr int OB_ROW = OB_TILE + OB_TILE / OB_C;   // a skewed oscillator row of the LDS tile
constexpr int OB_SPAN = 2048;                   // steps per span where rows are few
constexpr int OB_MAX_N = 1024;                  // oscillators whose carries the LDS holds
typedef unsigned long long ob_u64;

struct ObArgs {
    const float *f, *a, *g;
    long long fr, ft, fn, ar, at, an, gr, gt, gn;       // strides in elements: row, time, oscillator
    long long rows, T, N, span, spans;
    double sr, half_sr, dscale;                         // dscale = 2 pi / sr
    int reduction;                                      // 0 sum, 1 mean, 2 none
    ob_u64* ws_inc;
    double* ws_w;
    float *out, *ga, *gf;
};

__device__ __forceinline__ int ob_at(int t) { return t + (t >> 3); }

// frac(f / sr) in units of 2^-64 turns (a non-finite f gives 0: the conversion saturates a NaN to zero)
__device__ __forceinline__ ob_u64 ob_inc(float f, double sr) {
    const double x = (double)f;
    const double q0 = x / sr;
    double q = q0 - floor(q0);                          // [0, 1]; 1.0 where a tiny negative quotient rounds up
    const ob_u64 u = q >= 1.0 ? 0ull : (ob_u64)(q * 18446744073709551616.0);
    // the quotient's own rounding (up to 2^-54 turns) is recovered from the exact remainder: the increment is good to 2^-63 turns
    const double rest = fma(-q0, sr, x) / sr;
    return fabs(q0) < 1099511627776.0 ? u + (ob_u64)(long long)(rest * 18446744073709551616.0) : u;
}

// sin and cos of 2 pi u / 2^64: the nearest quarter turn is exact integer arithmetic, the rest a float64 polynomial on [-pi/4, pi/4]
__device__ __forceinline__ void ob_sincos(ob_u64 u, double& s, double& c) {
    const ob_u64 k = (u + (1ull << 61)) >> 62;          // 0 .. 4
    const long long r = (long long)(u - (k << 62));     // (k == 4: the shift wraps to 0 and u is a small negative angle)
    const double th = (double)r * (6.283185307179586476925286766559 / 18446744073709551616.0);
    const double z = th * th;
    const double ps = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                                                   2.75573137070700676789e-06), -1.98412698298579493134e-04),
                                 8.33333333332248946124e-03), -1.66666666666666324348e-01);
    const double pc = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                                   -2.75573143513906633035e-07), 2.48015872894767294178e-05),
                                 -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double ss = fma(th * z, ps, th);
    const double cc = fma(z * z, pc, fma(-0.5, z, 1.0));
    const int q = (int)(k & 3);
    s = q == 0 ? ss : (q == 1 ? cc : (q == 2 ? -ss : -cc));
    c = q == 0 ? cc : (q == 1 ? -ss : (q == 2 ? -cc : ss));
}

// a (tile x group) block of a strided (rows, T, N) tensor into a skewed LDS tile, walking the tensor's contiguous axis fastest
__device__ __forceinline__ void ob_stage(float* dst, const float* src, long long st, long long sn, int nt, int ngc) {
    const int cells = nt * ngc;
    if (sn <= st) {
        for (int e = threadIdx.x; e < cells; e += OB_THREADS) {
            const int t = e / ngc, n = e - t * ngc;
            dst[n * OB_ROW + ob_at(t)] = src[t * st + n * sn];
        }
    } else {
        for (int e = threadIdx.x; e < cells; e += OB_THREADS) {
            const int n = e / nt, t = e - n * nt;
            dst[n * OB_ROW + ob_at(t)] = src[t * st + n * sn];
        }
    }
}

// a skewed LDS tile into a dense (T, N) block, oscillator index fastest
__device__ __forceinline__ void ob_unstage(float* dst, const float* src, long long N, int nt, int ngc) {
    const int cells = nt * ngc;
    for (int e = threadIdx.x; e < cells; e += OB_THREADS) {
        const int t = e / ngc, n = e - t * ngc;
        dst[t * N + n] = src[n * OB_ROW + ob_at(t)];
    }
}

template <int MODE>
__global__ void __launch_bounds__(OB_THREADS) oscbank_kernel(ObArgs A) {
    // Dynamic LDS: fs | as | gs (MODE >= 2), OB_NG skewed rows of floats each (fs | as doubles as the float64 product tile of the
    // 'sum' / 'mean' reduction) | gl[OB_TILE] | carry_p[N] | carry_s[N]
    extern __shared__ __attribute__((aligned(16))) unsigned char ob_lds[];
    float* fs = reinterpret_cast<float*>(ob_lds);
    float* as = fs + OB_NG * OB_ROW;
    float* gs = as + OB_NG * OB_ROW;
    float* gl = gs + (MODE >= 2 ? OB_NG * OB_ROW : 0);
    ob_u64* carry_p = reinterpret_cast<ob_u64*>(gl + OB_TILE);
    double* carry_s = reinterpret_cast<double*>(carry_p + A.N);
    double* yd = reinterpret_cast<double*>(ob_lds);

    const int tid = threadIdx.x;
    const int tl = tid & (OB_TL - 1), ng = tid >> 5;
    const long long row = blockIdx.x / A.spans, sp = blockIdx.x - row * A.spans;
    const long long t_begin = sp * A.span;
    const long long t_end = t_begin + A.span < A.T ? t_begin + A.span : A.T;
    const int N = (int)A.N;
    const bool full = A.reduction == 2;

    // ---- the unit's incoming carries: integer sums of span totals (any order gives the same bits), float64 sums in a fixed order
    // (forward: the spans before this one; backward: up to and including it, the phase at the span's END; mode 0: none)
    const long long count = MODE == 1 ? sp : (MODE >= 2 ? sp + 1 : 0);
    for (int nb = 0; nb < N; nb += OB_NG) {
        const int n = nb + ng;
        ob_u64 p = 0;
        double s = 0.0;
        if (n < N) {
            for (long long q = tl; q < count; q += OB_TL) p += A.ws_inc[(row * A.spans + q) * N + n];
            if (MODE == 3)
                for (long long q = sp + 1 + tl; q < A.spans; q += OB_TL) s += A.ws_w[(row * A.spans + q) * N + n];
        }
#pragma unroll
        for (int d = 1; d < OB_TL; d <<= 1) {
            p += __shfl_xor(p, d, OB_TL);
            if (MODE == 3) s += __shfl_xor(s, d, OB_TL);
        }
        if (tl == 0 && n < N) {
            carry_p[n] = p;
            if (MODE >= 2) carry_s[n] = s;
        }
    }
    __syncthreads();

    const long long tiles = (t_end - t_begin + OB_TILE - 1) / OB_TILE;
    for (long long ti = 0; ti < tiles; ++ti) {
        const long long t0 = t_begin + (MODE >= 2 ? tiles - 1 - ti : ti) * OB_TILE;
        const int nt = (int)(t_end - t0 < OB_TILE ? t_end - t0 : OB_TILE);
        double acc = 0.0;                                   // 'sum' / 'mean': lane tid < nt owns step t0 + tid
        if (MODE >= 2 && !full) {
            if (tid < nt) gl[tid] = A.g[row * A.gr + (t0 + tid) * A.gt];
        }
        for (int nb = 0; nb < N; nb += OB_NG) {
            const int ngc = N - nb < OB_NG ? N - nb : OB_NG;
            ob_stage(fs, A.f + row * A.fr + t0 * A.ft + nb * A.fn, A.ft, A.fn, nt, ngc);
            if (MODE != 0) ob_stage(as, A.a + row * A.ar + t0 * A.at + nb * A.an, A.at, A.an, nt, ngc);
            if (MODE >= 2 && full) ob_stage(gs, A.g + row * A.gr + t0 * A.gt + nb * A.gn, A.gt, A.gn, nt, ngc);
            __syncthreads();

            const int n = nb + ng;
            const bool active = ng < ngc;
            const int c0 = tl * OB_C;
            ob_u64 inc[OB_C];
            float av[OB_C], gv[OB_C];
            bool ok[OB_C];
            ob_u64 total = 0;
#pragma unroll
            for (int k = 0; k < OB_C; ++k) {
                const bool in = active && c0 + k < nt;
                const float fv = in ? fs[ng * OB_ROW + ob_at(c0 + k)] : 0.0f;
                inc[k] = in ? ob_inc(fv, A.sr) : 0ull;
                ok[k] = in && fabs((double)fv) < A.half_sr;
                if (MODE != 0) av[k] = in ? as[ng * OB_ROW + ob_at(c0 + k)] : 0.0f;
                if (MODE >= 2) gv[k] = !in ? 0.0f : (full ? gs[ng * OB_ROW + ob_at(c0 + k)] : gl[c0 + k]);
                total += inc[k];
            }
            ob_u64 incl = total;
#pragma unroll
            for (int d = 1; d < OB_TL; d <<= 1) {
                const ob_u64 up = __shfl_up(incl, d, OB_TL);
                if (tl >= d) incl += up;
            }
            const ob_u64 tile_total = __shfl(incl, OB_TL - 1, OB_TL);
            const ob_u64 carry = active ? carry_p[n] : 0ull;

            if constexpr (MODE == 0) {
                if (tl == 0 && active) carry_p[n] = carry + tile_total;
                __syncthreads();
            } else if constexpr (MODE == 1) {
                if (tl == 0 && active) carry_p[n] = carry + tile_total;
                ob_u64 ph = carry + (incl - total);
                double y[OB_C];
#pragma unroll
                for (int k = 0; k < OB_C; ++k) {
                    ph += inc[k];
                    double s, c;
                    ob_sincos(ph, s, c);
                    y[k] = ok[k] ? (double)av[k] * s : 0.0;
                }
                __syncthreads();                            // every lane has read its chunk: the tiles may be overwritten
                if (full) {
#pragma unroll
                    for (int k = 0; k < OB_C; ++k) fs[ng * OB_ROW + ob_at(c0 + k)] = (float)y[k];
                    __syncthreads();
                    ob_unstage(A.out + (row * A.T + t0) * A.N + nb, fs, A.N, nt, ngc);
                } else {
#pragma unroll
                    for (int k = 0; k < OB_C; ++k) yd[ng * OB_TILE + c0 + k] = y[k];
                    __syncthreads();
                    if (tid < nt) {
#pragma unroll
                        for (int j = 0; j < OB_NG; ++j) acc += yd[j * OB_TILE + tid];
                    }
                }
                __syncthreads();
            } else {
                // ---- backward: the phase at the tile's start from the phase at its end; suffix sums of w
                if (tl == 0 && active) carry_p[n] = carry - tile_total;
                ob_u64 ph = carry - tile_total + (incl - total);
                const double gscale = A.reduction == 1 ? 1.0 / (double)A.N : 1.0;
                double da[OB_C], w[OB_C];
#pragma unroll
                for (int k = 0; k < OB_C; ++k) {
                    ph += inc[k];
                    double s, c;
                    ob_sincos(ph, s, c);
                    const double g = (double)gv[k] * gscale;
                    da[k] = ok[k] ? g * s : 0.0;
                    w[k] = ok[k] ? g * (double)av[k] * c : 0.0;
                }
#pragma unroll
                for (int k = OB_C - 2; k >= 0; --k) w[k] += w[k + 1];          // the chunk's own suffix sums
                double sincl = w[0];
#pragma unroll
                for (int d = 1; d < OB_TL; d <<= 1) {
                    const double dn = __shfl_down(sincl, d, OB_TL);
                    if (tl + d < OB_TL) sincl += dn;
                }
                double later = __shfl_down(sincl, 1, OB_TL);                    // everything behind the lane's chunk in the tile
                if (tl == OB_TL - 1) later = 0.0;
                const double tile_w = __shfl(sincl, 0, OB_TL);
                const double behind = active ? carry_s[n] : 0.0;                // ... and behind the tile in the row
                if (tl == 0 && active) carry_s[n] = behind + tile_w;
                __syncthreads();
                if constexpr (MODE == 3) {
                    const double rest = later + behind;
#pragma unroll
                    for (int k = 0; k < OB_C; ++k) {
                        fs[ng * OB_ROW + ob_at(c0 + k)] = (float)da[k];
                        as[ng * OB_ROW + ob_at(c0 + k)] = (float)(A.dscale * (w[k] + rest));
                    }
                    __syncthreads();
                    ob_unstage(A.ga + (row * A.T + t0) * A.N + nb, fs, A.N, nt, ngc);
                    ob_unstage(A.gf + (row * A.T + t0) * A.N + nb, as, A.N, nt, ngc);
                    __syncthreads();
                }
            }
        }
        if (MODE == 1 && !full) {
            if (tid < nt) A.out[row * A.T + t0 + tid] = (float)(A.reduction == 1 ? acc / (double)A.N : acc);
        }
    }
    __syncthreads();
    if (MODE == 0)
        for (int n = tid; n < N; n += OB_THREADS) A.ws_inc[(row * A.spans + sp) * N + n] = carry_p[n];
    if (MODE == 2)
        for (int n = tid; n < N; n += OB_THREADS) A.ws_w[(row * A.spans + sp) * N + n] = carry_s[n];
}

// steps per span: the whole row where rows alone fill the device twice over (or the row is short), OB_SPAN otherwise
inline long long ob_span(long long rows, long long T) {
    if (T <= OB_SPAN || rows >= 2LL * device_cu_count()) return T;
    return OB_SPAN;
}

inline size_t ob_lds_bytes(int mode, long long N) {
    return (size_t)((mode >= 2 ? 3 : 2) * OB_NG * OB_ROW + OB_TILE) * sizeof(float) + (size_t)N * 16;
}

inline int ob_check(const void* f, const void* a, long long rows, long long T, long long N, const long long* st, int n_st,
                    double sr, int reduction) {
    if (!f || !a || rows <= 0 || T <= 0 || N <= 0 || reduction < 0 || reduction > 2) return TAC_E_INVALID;
    if (!(sr > 0.0) || !isfinite(sr)) return TAC_E_INVALID;
    for (int i = 0; i < n_st; ++i)
        if (st[i] < 0) return TAC_E_INVALID;
    if (N > OB_MAX_N || rows * ((T + OB_TILE - 1) / OB_TILE) > 0x7fffffffLL) return TAC_E_UNSUPPORTED;
    return TAC_OK;
}

// ============================================================================= filter_waveform
constexpr int FW_THREADS = 256;
constexpr int FW_PER = 4;                       // consecutive outputs per lane
constexpr int FW_WAVE = 64 * FW_PER;            // outputs per wave
constexpr int FW_TILE = FW_THREADS * FW_PER;    // 1024 outputs per workgroup
constexpr int FW_MAX_TAPS = 768;
constexpr int FW_TAPS_PER_LANE = FW_MAX_TAPS / FW_THREADS;
constexpr int FW_PIECE = 2048;                  // samples of a chunk per workgroup of the d h kernel

struct FwArgs {
    const float* x;                             // the rows convolved (forward: the waveform; d x: the upstream gradient)
    long long x_r;                              // row stride (unit stride along time)
    const float* h;
    long long h_div, h_outer, h_inner, h_f, h_k;        // row r reads h + (r / h_div) h_outer + (r % h_div) h_inner + j h_f + k h_k
    long long rows, T, F, K, C, s, tiles;
    float* out;
};

__device__ __forceinline__ const float* fw_filter(const FwArgs& A, long long row, long long j) {
    return A.h + (row / A.h_div) * A.h_outer + (row % A.h_div) * A.h_inner + j * A.h_f;
}

// ADJ == false: out[t] = sum_k h_{(t + s - k) / C}[k] x[t + s - k]; ADJ == true: out[m] = sum_k h_{m / C}[k] x[m - s + k]
template <bool ADJ>
__global__ void __launch_bounds__(FW_THREADS) filter_waveform_kernel(FwArgs A) {
    __shared__ float xs[FW_TILE + FW_MAX_TAPS + 8];         // the staged span, one zero in front of it and one behind
    __shared__ float hs[2][FW_MAX_TAPS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row = blockIdx.x / A.tiles;
    const long long t0 = (blockIdx.x - row * A.tiles) * FW_TILE;
    const int K = (int)A.K;
    const long long C = A.C;
    // index i of xs (behind the leading zero) is sample span0 + i
    const long long span0 = ADJ ? t0 - A.s : t0 + A.s - K + 1;
    const int len = FW_TILE + K - 1;
    const float* src = A.x + row * A.x_r;
    for (int i = tid; i < len + 2; i += FW_THREADS) {
        const long long m = span0 + i - 1;
        xs[i] = (i >= 1 && i <= len && m >= 0 && m < A.T) ? src[m] : 0.0f;
    }
    // the chunks whose samples this tile touches
    long long mlo, mhi;                                     // [mlo, mhi): forward the input samples, adjoint the outputs
    if (ADJ) {
        mlo = t0;
        mhi = t0 + FW_TILE < A.T ? t0 + FW_TILE : A.T;
    } else {
        mlo = span0 > 0 ? span0 : 0;
        mhi = span0 + len < A.T ? span0 + len : A.T;
    }
    float acc[FW_PER] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (mlo < mhi) {
        const long long jlo = mlo / C, jhi = (mhi - 1) / C;
        const float* hp = fw_filter(A, row, jlo);
        for (int k = tid; k < K; k += FW_THREADS) hs[0][k] = hp[k * A.h_k];
        __syncthreads();
        const long long nw0 = (ADJ ? t0 : t0 + A.s) + wave * FW_WAVE;      // the wave's first output (forward: as n = t + s)
        const long long n0 = nw0 + lane * FW_PER;
        for (long long j = jlo; j <= jhi; ++j) {
            const int b = (int)((j - jlo) & 1);
            float next[FW_TAPS_PER_LANE];
            if (j < jhi) {                                  // the next filter is on its way while this one is used
                const float* hn = fw_filter(A, row, j + 1);
#pragma unroll
                for (int i = 0; i < FW_TAPS_PER_LANE; ++i) {
                    const int k = tid + i * FW_THREADS;
                    next[i] = k < K ? hn[k * A.h_k] : 0.0f;
                }
            }
            const long long lo = j * C, hi = lo + C;        // the chunk's samples
            const float* hb = hs[b];
            if constexpr (!ADJ) {
                const long long kl = nw0 - hi + 1, kh = nw0 + FW_WAVE - 1 - lo;
                const int klo = (int)(kl > 0 ? kl : 0), khi = (int)(kh < K - 1 ? kh : K - 1);
                if (klo <= khi) {
                    float w[FW_PER];
#pragma unroll
                    for (int i = 0; i < FW_PER; ++i) {
                        const long long m = n0 + i - klo;
                        w[i] = (m >= lo && m < hi) ? xs[m - span0 + 1] : 0.0f;
                    }
                    for (int k = klo; k <= khi; ++k) {
                        const float hv = hb[k];
#pragma unroll
                        for (int i = 0; i < FW_PER; ++i) acc[i] = fmaf(hv, w[i], acc[i]);
#pragma unroll
                        for (int i = FW_PER - 1; i > 0; --i) w[i] = w[i - 1];
                        const long long m = n0 - k - 1;     // (k == K - 1 of the first lane: the zero in front of the span)
                        w[0] = (m >= lo && m < hi) ? xs[m - span0 + 1] : 0.0f;
                    }
                }
            } else {
                if (nw0 < hi && nw0 + FW_WAVE > lo) {       // the wave holds samples of this chunk
                    const int base = (int)(n0 - t0) + 1;    // xs index of g[m - s] for the lane's first sample
                    float w[FW_PER], sum[FW_PER] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int i = 0; i < FW_PER; ++i) w[i] = xs[base + i];
                    for (int k = 0; k < K; ++k) {
                        const float hv = hb[k];
#pragma unroll
                        for (int i = 0; i < FW_PER; ++i) sum[i] = fmaf(hv, w[i], sum[i]);
#pragma unroll
                        for (int i = 0; i < FW_PER - 1; ++i) w[i] = w[i + 1];
                        w[FW_PER - 1] = xs[base + FW_PER + k];      // (k == K - 1 of the last lane: the zero behind the span)
                    }
#pragma unroll
                    for (int i = 0; i < FW_PER; ++i)
                        if (n0 + i >= lo && n0 + i < hi) acc[i] = sum[i];
                }
            }
            if (j < jhi) {
#pragma unroll
                for (int i = 0; i < FW_TAPS_PER_LANE; ++i) {
                    const int k = tid + i * FW_THREADS;
                    if (k < K) hs[b ^ 1][k] = next[i];
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < FW_PER; ++i) {
        const long long t = t0 + tid * FW_PER + i;
        if (t < A.T) A.out[row * A.T + t] = acc[i];
    }
}

// part[row][j][p][k] = sum over the piece's samples m of x[m] g[m - s + k]
__global__ void __launch_bounds__(FW_THREADS)
filter_waveform_grad_kernels_kernel(const float* __restrict__ x, long long x_r, const float* __restrict__ g, long long g_r, long long T,
                                    long long F, long long K, long long C, long long s, long long P, float* __restrict__ part) {
    __shared__ float xs[FW_PIECE];
    __shared__ float gs[FW_PIECE + FW_MAX_TAPS];
    const int tid = threadIdx.x;
    const long long unit = blockIdx.x;
    const long long p = unit % P, j = (unit / P) % F, row = unit / (P * F);
    const long long ms = j * C + p * FW_PIECE;
    long long me = ms + FW_PIECE;
    if (me > (j + 1) * C) me = (j + 1) * C;
    if (me > T) me = T;
    const int cnt = me > ms ? (int)(me - ms) : 0;
    const int Ki = (int)K;
    float acc[FW_TAPS_PER_LANE] = {0.0f, 0.0f, 0.0f};
    if (cnt > 0) {
        for (int i = tid; i < cnt; i += FW_THREADS) xs[i] = x[row * x_r + ms + i];
        for (int i = tid; i < cnt + Ki - 1; i += FW_THREADS) {
            const long long q = ms - s + i;
            gs[i] = (q >= 0 && q < T) ? g[row * g_r + q] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < FW_TAPS_PER_LANE; ++i) {
            const int k = tid + i * FW_THREADS;
            if (k < Ki) {
                float a = 0.0f;
                for (int m = 0; m < cnt; ++m) a = fmaf(xs[m], gs[m + k], a);
                acc[i] = a;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < FW_TAPS_PER_LANE; ++i) {
        const int k = tid + i * FW_THREADS;
        if (k < Ki) part[unit * K + k] = acc[i];
    }
}

inline long long fw_chunk(long long T, long long F) { return (T + F - 1) / F; }

}  // namespace tac

extern "C" {

int32_t tac_oscbank_tile(void) { return tac::OB_TILE; }
int32_t tac_oscbank_chunk(void) { return tac::OB_C; }
int32_t tac_oscbank_span(void) { return tac::OB_SPAN; }
int32_t tac_oscbank_max_oscillators(void) { return tac::OB_MAX_N; }

int64_t tac_oscbank_spans(int64_t rows, int64_t time) {
    if (rows <= 0 || time <= 0) return 0;
    const long long span = tac::ob_span(rows, time);
    return (time + span - 1) / span;
}

int tac_oscbank_f32(const float* f, const float* a, int64_t rows, int64_t time, int64_t n, int64_t f_stride_r, int64_t f_stride_t,
                    int64_t f_stride_n, int64_t a_stride_r, int64_t a_stride_t, int64_t a_stride_n, double sample_rate,
                    int reduction, void* workspace, float* out, void* stream) {
    using namespace tac;
    const long long st[6] = {f_stride_r, f_stride_t, f_stride_n, a_stride_r, a_stride_t, a_stride_n};
    const int rc = ob_check(f, a, rows, time, n, st, 6, sample_rate, reduction);
    if (rc != TAC_OK) return rc;
    if (!out) return TAC_E_INVALID;
    ObArgs A = {};
    A.f = f, A.a = a;
    A.fr = f_stride_r, A.ft = f_stride_t, A.fn = f_stride_n, A.ar = a_stride_r, A.at = a_stride_t, A.an = a_stride_n;
    A.rows = rows, A.T = time, A.N = n;
    A.span = ob_span(rows, time);
    A.spans = (time + A.span - 1) / A.span;
    A.sr = sample_rate, A.half_sr = 0.5 * sample_rate, A.dscale = 6.283185307179586476925286766559 / sample_rate;
    A.reduction = reduction;
    A.ws_inc = static_cast<ob_u64*>(workspace);
    A.out = out;
    if (A.spans > 1) {
        if (!workspace) return TAC_E_INVALID;
        const int r0 = launch_kernel(oscbank_kernel<0>, rows * A.spans, OB_THREADS, ob_lds_bytes(0, n), (hipStream_t)stream, A);
        if (r0 != TAC_OK) return r0;
    }
    return launch_kernel(oscbank_kernel<1>, rows * A.spans, OB_THREADS, ob_lds_bytes(1, n), (hipStream_t)stream, A);
}

int tac_oscbank_grad_f32(const float* f, const float* a, const float* g, int64_t rows, int64_t time, int64_t n, int64_t f_stride_r,
                         int64_t f_stride_t, int64_t f_stride_n, int64_t a_stride_r, int64_t a_stride_t, int64_t a_stride_n,
                         int64_t g_stride_r, int64_t g_stride_t, int64_t g_stride_n, double sample_rate, int reduction,
                         void* workspace, float* grad_a, float* grad_f, void* stream) {
    using namespace tac;
    const long long st[9] = {f_stride_r, f_stride_t, f_stride_n, a_stride_r, a_stride_t, a_stride_n, g_stride_r, g_stride_t, g_stride_n};
    const int rc = ob_check(f, a, rows, time, n, st, 9, sample_rate, reduction);
    if (rc != TAC_OK) return rc;
    if (!g || !grad_a || !grad_f || !workspace) return TAC_E_INVALID;
    ObArgs A = {};
    A.f = f, A.a = a, A.g = g;
    A.fr = f_stride_r, A.ft = f_stride_t, A.fn = f_stride_n, A.ar = a_stride_r, A.at = a_stride_t, A.an = a_stride_n;
    A.gr = g_stride_r, A.gt = g_stride_t, A.gn = reduction == 2 ? g_stride_n : 0;
    A.rows = rows, A.T = time, A.N = n;
    A.span = ob_span(rows, time);
    A.spans = (time + A.span - 1) / A.span;
    A.sr = sample_rate, A.half_sr = 0.5 * sample_rate, A.dscale = 6.283185307179586476925286766559 / sample_rate;
    A.reduction = reduction;
    A.ws_inc = static_cast<ob_u64*>(workspace);
    A.ws_w = reinterpret_cast<double*>(A.ws_inc + rows * A.spans * n);
    A.ga = grad_a, A.gf = grad_f;
    int r = launch_kernel(oscbank_kernel<0>, rows * A.spans, OB_THREADS, ob_lds_bytes(0, n), (hipStream_t)stream, A);
    if (r != TAC_OK) return r;
    if (A.spans > 1) {
        r = launch_kernel(oscbank_kernel<2>, rows * A.spans, OB_THREADS, ob_lds_bytes(2, n), (hipStream_t)stream, A);
        if (r != TAC_OK) return r;
    }
    return launch_kernel(oscbank_kernel<3>, rows * A.spans, OB_THREADS, ob_lds_bytes(3, n), (hipStream_t)stream, A);
}

int32_t tac_filter_waveform_tile(void) { return tac::FW_TILE; }
int32_t tac_filter_waveform_max_taps(void) { return tac::FW_MAX_TAPS; }
int32_t tac_filter_waveform_piece(void) { return tac::FW_PIECE; }

int tac_filter_waveform_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const float* h, int64_t h_div,
                            int64_t h_stride_outer, int64_t h_stride_inner, int64_t h_stride_f, int64_t h_stride_k, int64_t n_filters,
                            int64_t taps, int64_t shift, int adjoint, float* out, void* stream) {
    using namespace tac;
    if (!x || !h || !out || rows <= 0 || length <= 0 || n_filters <= 0 || taps <= 0 || h_div <= 0) return TAC_E_INVALID;
    if (shift < 0 || shift > taps - 1 || stride_r < 0 || h_stride_outer < 0 || h_stride_inner < 0 || h_stride_f < 0 || h_stride_k < 0)
        return TAC_E_INVALID;
    if (taps > FW_MAX_TAPS) return TAC_E_UNSUPPORTED;
    FwArgs A = {};
    A.x = x, A.x_r = stride_r, A.h = h;
    A.h_div = h_div, A.h_outer = h_stride_outer, A.h_inner = h_stride_inner, A.h_f = h_stride_f, A.h_k = h_stride_k;
    A.rows = rows, A.T = length, A.F = n_filters, A.K = taps, A.C = fw_chunk(length, n_filters), A.s = shift;
    A.tiles = (length + FW_TILE - 1) / FW_TILE;
    A.out = out;
    if (rows * A.tiles > 0x7fffffffLL) return TAC_E_UNSUPPORTED;
    return adjoint ? launch_kernel(filter_waveform_kernel<true>, rows * A.tiles, FW_THREADS, 0, (hipStream_t)stream, A)
                   : launch_kernel(filter_waveform_kernel<false>, rows * A.tiles, FW_THREADS, 0, (hipStream_t)stream, A);
}

int64_t tac_filter_waveform_pieces(int64_t length, int64_t n_filters) {
    if (length <= 0 || n_filters <= 0) return 0;
    return (tac::fw_chunk(length, n_filters) + tac::FW_PIECE - 1) / tac::FW_PIECE;
}

int tac_filter_waveform_grad_kernels_f32(const float* x, int64_t stride_r, const float* g, int64_t g_stride_r, int64_t rows,
                                         int64_t length, int64_t n_filters, int64_t taps, int64_t shift, float* part, void* stream) {
    using namespace tac;
    if (!x || !g || !part || rows <= 0 || length <= 0 || n_filters <= 0 || taps <= 0 || stride_r < 0 || g_stride_r < 0)
        return TAC_E_INVALID;
    if (shift < 0 || shift > taps - 1) return TAC_E_INVALID;
    if (taps > FW_MAX_TAPS) return TAC_E_UNSUPPORTED;
    const long long P = tac_filter_waveform_pieces(length, n_filters);
    if (rows * n_filters * P > 0x7fffffffLL) return TAC_E_UNSUPPORTED;
    return launch_kernel(filter_waveform_grad_kernels_kernel, rows * n_filters * P, FW_THREADS, 0, (hipStream_t)stream, x,
                         (long long)stride_r, g, (long long)g_stride_r, (long long)length, (long long)n_filters, (long long)taps,
                         fw_chunk(length, n_filters), (long long)shift, P, part);
}

}  // extern "C"
