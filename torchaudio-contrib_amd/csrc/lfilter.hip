// lfilter.hip — functional.lfilter (and the biquads, pre-emphasis and de-emphasis on top of it): a recursive filter of order <= 2
// along the last axis and, with `reverse`, its adjoint (the same filter run from the end of the row), one streaming kernel.
//
//   y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2]          (coefficients already divided by a0; zero initial state)
//
// A row is walked from its start to its end by ONE workgroup, in tiles of LF_TILE = 1024 * LF_C consecutive samples; no workgroup
// ever waits on another.  Per tile
//   global -> xs           the tile, coalesced (16 bytes per lane where the row is aligned), stored in time order
//   pass 1                 lane l owns samples [l*C, l*C + C): v[n] = sum b_k x[n-k] (the two samples before the chunk come from the
//                          neighbour's part of xs, or from the carried tail of the previous tile), then the all-pole recursion from
//                          ZERO state; only the end state s_l = (y[last], y[last-1]) is kept
//   scan                   the true end states are S_l = M^C S_{l-1} + s_l with M = [[-a1, -a2], [1, 0]]: every lane has the same
//                          linear part, so Kogge-Stone needs only the ten matrices M^(C 2^i) (host, float64) — six steps across the
//                          lanes of a wave with cross-lane moves, four across the 16 waves through the LDS.  The carry of the
//                          previous tile enters by linearity: s_0 += M^C carry.
//   pass 2                 the recursion again from the lane's true incoming state; clamp; into xs; coalesced stores
//   carry                  the last lane's state and last two x, for the workgroup's next tile of the same row
// The recursion, the scan and the state are float64, only loads and stores float32: with float32 state the rounded powers of a
// matrix with a near-double eigenvalue (poles next to z = 1, a 20 Hz high-pass at 48 kHz) cancel so badly that the scan loses the
// result.  Nothing is shared between rows and a lane's incoming state depends on earlier samples only, so a
// non-finite sample reaches the samples after it in its own row and nothing else.  No atomics, no workspace, one writer per
// element: bit-identical from run to run.
//
// xs is skewed by one float per C (index i lives at i + i / C): lane l's chunk starts at 17 l, so the lanes of a wave read and write
// different banks.  Coefficients that are exactly zero are not multiplied (a1 == a2 == 0 — pre-emphasis, any FIR — skips pass 1 and
// the scan altogether).
#include <math.h>

#include "host_common.hpp"

namespace tac {

typedef float lf_f4 __attribute__((ext_vector_type(4)));

constexpr int LF_C_LOG = 4;
constexpr int LF_C = 1 << LF_C_LOG;             // samples per lane
constexpr int LF_THREADS = 1024;
constexpr int LF_WAVES = LF_THREADS / 64;
constexpr int LF_TILE = LF_THREADS * LF_C;      // samples per tile
constexpr int LF_XS = LF_TILE + LF_TILE / LF_C + 1;
constexpr int LF_STEPS = 10;                    // log2(LF_THREADS): M^(C 2^i), i < 10
static_assert(LF_WAVES == 16 && (1 << LF_STEPS) == LF_THREADS, "the scan is six steps in a wave and four across sixteen waves");

struct LfMat { double a, b, c, d; };            // [[a, b], [c, d]]
struct LfParams {
    double b0, b1, b2, a1, a2;
    LfMat p[LF_STEPS];                          // p[i] = M^(C 2^i)
};

__device__ __forceinline__ int lf_at(int i) { return i + (i >> LF_C_LOG); }

__device__ __forceinline__ void lf_apply(const LfMat& m, double u0, double u1, double& s0, double& s1) {
    s0 += m.a * u0 + m.b * u1;
    s1 += m.c * u0 + m.d * u1;
}

template <bool RECUR, bool VEC>
__global__ void __launch_bounds__(LF_THREADS)
lfilter_kernel(const float* __restrict__ x, long long rows, long long length, long long stride_r, LfParams P, int clamp, int reverse,
               float* __restrict__ out) {
    // Dynamic LDS: wave_state[2][16][2] doubles ([0] the waves' own end states, [1] scanned across the waves) | carry_state[2]
    // doubles | carry_x[2] floats (+ 2 of padding) | xs[LF_XS]
    extern __shared__ __attribute__((aligned(16))) double lf_lds[];
    double (*wave_state)[LF_WAVES][2] = reinterpret_cast<double (*)[LF_WAVES][2]>(lf_lds);
    double* carry_state = lf_lds + 4 * LF_WAVES;
    float* carry_x = reinterpret_cast<float*>(carry_state + 2);
    float* xs = carry_x + 4;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int c0 = tid * LF_C;                          // the lane's first sample, in time order within the tile
    const long long tiles = (length + LF_TILE - 1) / LF_TILE;

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* src = x + row * stride_r;
        float* dst = out + row * length;
        for (long long t = 0; t < tiles; ++t) {
            const long long n0 = t * LF_TILE;                                   // first sample of the tile in time order
            const int nt = (int)(length - n0 < LF_TILE ? length - n0 : LF_TILE);
            const long long p0 = reverse ? length - n0 - nt : n0;               // ... and where the tile starts in memory
            // ---- global -> xs, time order: memory offset j of the tile is sample (reverse ? nt - 1 - j : j)
            if constexpr (VEC) {
                const long long a0f = p0 & ~3LL;
                const int lead = (int)(p0 - a0f);
                for (int q = tid; q < ((lead + nt + 3) >> 2); q += LF_THREADS) {
                    const long long g = a0f + 4 * q;
                    lf_f4 v;
                    if (g + 3 < length) {
                        v = *reinterpret_cast<const lf_f4*>(src + g);
                    } else {
                        v.x = g < length ? src[g] : 0.0f;
                        v.y = g + 1 < length ? src[g + 1] : 0.0f;
                        v.z = g + 2 < length ? src[g + 2] : 0.0f;
                        v.w = 0.0f;
                    }
                    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = 4 * q + k - lead;
                        if (j >= 0 && j < nt) xs[lf_at(reverse ? nt - 1 - j : j)] = e[k];
                    }
                }
            } else {
                for (int j = tid; j < nt; j += LF_THREADS) xs[lf_at(reverse ? nt - 1 - j : j)] = src[p0 + j];
            }
            __syncthreads();

            // ---- the lane's chunk and the two samples before it (zero before the row and behind its end)
            float xr[LF_C];
#pragma unroll
            for (int k = 0; k < LF_C; ++k) xr[k] = c0 + k < nt ? xs[lf_at(c0 + k)] : 0.0f;
            float xm1 = 0.0f, xm2 = 0.0f;
            double in0 = 0.0, in1 = 0.0;                 // the state the lane's chunk starts from: (y[c0 - 1], y[c0 - 2])
            if (tid > 0) {
                if (c0 - 1 < nt) xm1 = xs[lf_at(c0 - 1)];
                if (c0 - 2 < nt) xm2 = xs[lf_at(c0 - 2)];
            } else if (t > 0) {
                xm1 = carry_x[0];
                xm2 = carry_x[1];
                if constexpr (RECUR) {
                    in0 = carry_state[0];
                    in1 = carry_state[1];
                }
            }
            double v[LF_C];
#pragma unroll
            for (int k = 0; k < LF_C; ++k) {
                const float p1 = k >= 1 ? xr[k - 1] : xm1;
                const float p2 = k >= 2 ? xr[k - 2] : (k == 1 ? xm1 : xm2);
                double acc = P.b0 * (double)xr[k];
                if (P.b1 != 0.0) acc = fma(P.b1, (double)p1, acc);
                if (P.b2 != 0.0) acc = fma(P.b2, (double)p2, acc);
                v[k] = acc;
            }

            if constexpr (RECUR) {
                // ---- pass 1: zero-state response of the chunk, end state only
                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int k = 0; k < LF_C; ++k) {
                    const double y = fma(-P.a1, s0, fma(-P.a2, s1, v[k]));
                    s1 = s0;
                    s0 = y;
                }
                if (tid == 0) lf_apply(P.p[0], in0, in1, s0, s1);       // the previous tile's carry, by linearity (zero in tile 0)
                // ---- scan across the lanes of the wave
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const double u0 = __shfl_up(s0, 1 << i), u1 = __shfl_up(s1, 1 << i);
                    if (lane >= (1 << i)) lf_apply(P.p[i], u0, u1, s0, s1);
                }
                double e0 = __shfl_up(s0, 1), e1 = __shfl_up(s1, 1);     // the wave-local state before the lane's chunk
                if (lane == 0) e0 = e1 = 0.0;
                if (lane == 63) {
                    wave_state[0][wave][0] = s0;
                    wave_state[0][wave][1] = s1;
                }
                __syncthreads();
                // ---- ... and across the sixteen waves
                if (wave == 0) {
                    double w0 = lane < LF_WAVES ? wave_state[0][lane][0] : 0.0;
                    double w1 = lane < LF_WAVES ? wave_state[0][lane][1] : 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double u0 = __shfl_up(w0, 1 << i), u1 = __shfl_up(w1, 1 << i);
                        if (lane >= (1 << i)) lf_apply(P.p[6 + i], u0, u1, w0, w1);
                    }
                    if (lane < LF_WAVES) {
                        wave_state[1][lane][0] = w0;
                        wave_state[1][lane][1] = w1;
                    }
                }
                __syncthreads();
                // the state at the end of the previous wave, carried over the lane's `lane` chunks: M^(C lane) by the bits of lane
                if (tid > 0) {
                    in0 = e0;
                    in1 = e1;
                }
                if (wave > 0) {
                    double u0 = wave_state[1][wave - 1][0], u1 = wave_state[1][wave - 1][1];
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        if ((lane >> i) & 1) {
                            double m0 = 0.0, m1 = 0.0;
                            lf_apply(P.p[i], u0, u1, m0, m1);
                            u0 = m0;
                            u1 = m1;
                        }
                    }
                    in0 += u0;
                    in1 += u1;
                }
            } else {
                __syncthreads();                        // every lane has read its neighbour's samples: xs may be overwritten
            }

            // ---- pass 2: the chunk from its true incoming state, into xs
#pragma unroll
            for (int k = 0; k < LF_C; ++k) {
                double y = v[k];
                if constexpr (RECUR) {
                    y = fma(-P.a1, in0, fma(-P.a2, in1, y));
                    in1 = in0;
                    in0 = y;
                }
                float yf = (float)y;
                if (clamp) yf = yf < -1.0f ? -1.0f : (yf > 1.0f ? 1.0f : yf);      // (a NaN stays a NaN)
                if (c0 + k < nt) xs[lf_at(c0 + k)] = yf;
            }
            if (tid == LF_THREADS - 1) {                // read by lane 0 in the next tile, behind the barriers in between
                if constexpr (RECUR) {
                    carry_state[0] = in0;
                    carry_state[1] = in1;
                }
                carry_x[0] = xr[LF_C - 1];
                carry_x[1] = xr[LF_C - 2];
            }
            __syncthreads();
            for (int j = tid; j < nt; j += LF_THREADS) dst[p0 + j] = xs[lf_at(reverse ? nt - 1 - j : j)];
            __syncthreads();                            // nobody reads xs any more: the next tile may overwrite it
        }
    }
}

inline LfMat lf_mul(const LfMat& x, const LfMat& y) {
    return LfMat{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}

// Normalises by a[0] and fills the ten powers; TAC_E_UNSUPPORTED where one of them is not finite (a pole so far outside the unit
// circle (a radius of about 1.09) that M^(C 2^9) overflows float64: the scan would turn a silent row into NaN).
inline int lf_params(const double* b, const double* a, int n, LfParams* P) {
    if (!b || !a || n < 1) return TAC_E_INVALID;
    if (n > 3) return TAC_E_UNSUPPORTED;
    if (!(a[0] != 0.0) || !isfinite(a[0])) return TAC_E_INVALID;
    double bn[3] = {0.0, 0.0, 0.0}, an[3] = {1.0, 0.0, 0.0};
    for (int k = 0; k < n; ++k) {
        bn[k] = b[k] / a[0];
        an[k] = a[k] / a[0];
        if (!isfinite(bn[k]) || !isfinite(an[k])) return TAC_E_INVALID;
    }
    P->b0 = bn[0];
    P->b1 = bn[1];
    P->b2 = bn[2];
    P->a1 = an[1];
    P->a2 = an[2];
    const LfMat m{-an[1], -an[2], 1.0, 0.0};
    LfMat q = m;
    for (int k = 1; k < LF_C; ++k) q = lf_mul(q, m);
    for (int i = 0; i < LF_STEPS; ++i) {
        if (!isfinite(q.a) || !isfinite(q.b) || !isfinite(q.c) || !isfinite(q.d)) return TAC_E_UNSUPPORTED;
        P->p[i] = q;
        q = lf_mul(q, q);
    }
    return TAC_OK;
}

}  // namespace tac

extern "C" {

int32_t tac_lfilter_chunk(void) { return tac::LF_C; }

int tac_lfilter_supported(const double* b, const double* a, int32_t n_coeffs) {
    tac::LfParams P;
    return tac::lf_params(b, a, n_coeffs, &P);
}

int tac_lfilter_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const double* b, const double* a,
                    int32_t n_coeffs, int clamp, int reverse, float* out, void* stream) {
    using namespace tac;
    if (!x || !out || rows <= 0 || length <= 0) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    LfParams P;
    const int rc = lf_params(b, a, n_coeffs, &P);
    if (rc != TAC_OK) return rc;
    const bool recur = P.a1 != 0.0 || P.a2 != 0.0;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_r & 3) == 0;
    // 68 KiB of LDS and 16 waves per workgroup: two workgroups share a CU where the registers allow it
    const size_t bytes = (4 * LF_WAVES + 2) * sizeof(double) + (4 + LF_XS) * sizeof(float);
    const long long blocks = persistent_blocks(rows, 1, (long long)device_cu_count() * 2);
    auto kern = recur ? (vec ? lfilter_kernel<true, true> : lfilter_kernel<true, false>)
                      : (vec ? lfilter_kernel<false, true> : lfilter_kernel<false, false>);
    return launch_kernel(kern, blocks, LF_THREADS, bytes, (hipStream_t)stream, x, (long long)rows, (long long)length,
                         (long long)stride_r, P, clamp ? 1 : 0, reverse ? 1 : 0, out);
}

}  // extern "C"
