// biquad_scan.hpp — the tile walk shared by the kernels that run a recursion of order <= 2 along a row: lfilter.hip, sosfilt.hip,
// loudness.hip and (geometry and tile load only) overdrive in sox_effects.hip.
//
// A row belongs to ONE workgroup of BQ_THREADS lanes, which walks it in tiles of BQ_TILE = 1024 * BQ_C consecutive samples; lane l
// owns samples [l*C, l*C + C) of the tile.  The tile is staged in an LDS array of BQ_XS floats skewed by one float per chunk (index
// i lives at bq_at(i) = i + i / C): lane l's chunk starts at 17 l, so the lanes of a wave read and write different banks.
//
//   y[n] = v[n] - a1 y[n-1] - a2 y[n-2],  v the feed-forward part          (coefficients already divided by a0)
//   pass 1     the chunk from ZERO state; only the end state s_l = (y[last], y[last-1]) is kept
//   scan       the true end states are S_l = M^C S_{l-1} + s_l with M = [[-a1, -a2], [1, 0]]: every lane has the same linear part,
//              so Kogge-Stone needs only the ten matrices M^(C 2^i) (host, float64: bq_section) — six steps across the lanes of a
//              wave with cross-lane moves, four across the sixteen waves through the LDS.  The carry of the previous tile enters
//              by linearity: s_0 += M^C carry.
//   pass 2     the caller's: the chunk again from its true incoming state
// bq_incoming_published is pass 1 and the scan in the form where wave 0 scans the sixteen wave states and publishes them (two
// barriers, [2][16][2] doubles of LDS); lfilter.hip and loudness.hip call it.  sosfilt.hip's one-barrier form, where every wave
// scans the sixteen states for itself, takes bq_pass1 and bq_apply from here and keeps its scan written out.  The scan steps are
// not functions of their own: split into per-step helpers, the sosfilt and loudness kernels measured 0.3 .. 1.6 % slower
// (profiles/biquad_scan).  State and scan are float64.
#pragma once
#include <math.h>

#include "host_common.hpp"

namespace tac {

constexpr int BQ_C_LOG = 4;
constexpr int BQ_C = 1 << BQ_C_LOG;             // samples per lane
constexpr int BQ_THREADS = 1024;
constexpr int BQ_WAVES = BQ_THREADS / 64;
constexpr int BQ_TILE = BQ_THREADS * BQ_C;      // samples per tile
constexpr int BQ_XS = BQ_TILE + BQ_TILE / BQ_C + 1;
constexpr int BQ_STEPS = 10;                    // log2(BQ_THREADS): M^(C 2^i), i < 10
static_assert(BQ_WAVES == 16 && (1 << BQ_STEPS) == BQ_THREADS, "the scan is six steps in a wave and four across sixteen waves");

struct BqMat { double a, b, c, d; };            // [[a, b], [c, d]]
struct BqSection {                              // 45 doubles
    double b0, b1, b2, a1, a2;
    BqMat p[BQ_STEPS];                          // p[i] = M^(C 2^i), M = [[-a1, -a2], [1, 0]]
};

inline BqMat bq_mul(const BqMat& x, const BqMat& y) {
    return BqMat{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}

// b[n], a[n] (1 <= n <= 3, the missing ones zero) normalised by a[0], and the ten powers.  TAC_E_INVALID for a zero or non-finite
// a[0] or a coefficient that is not finite after the division; TAC_E_UNSUPPORTED where a power is not finite (a pole so far outside
// the unit circle (a radius of about 1.09) that M^(C 2^9) overflows float64: the scan would turn a silent row into NaN).
inline int bq_section(const double* b, const double* a, int n, BqSection* P) {
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
    const BqMat m{-an[1], -an[2], 1.0, 0.0};
    BqMat q = m;
    for (int k = 1; k < BQ_C; ++k) q = bq_mul(q, m);
    for (int i = 0; i < BQ_STEPS; ++i) {
        if (!isfinite(q.a) || !isfinite(q.b) || !isfinite(q.c) || !isfinite(q.d)) return TAC_E_UNSUPPORTED;
        P->p[i] = q;
        q = bq_mul(q, q);
    }
    return TAC_OK;
}

typedef float bq_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int bq_at(int i) { return i + (i >> BQ_C_LOG); }

// global -> LDS for `count` samples that start at row offset p0 (p0 >= 0, p0 + count <= length): 16 bytes per lane where the row
// is aligned (VEC), a float per lane otherwise.  put(j, value) stores sample p0 + j.
template <bool VEC, int THREADS, class Put>
__device__ __forceinline__ void bq_load(const float* __restrict__ src, long long length, long long p0, int count, int tid, Put put) {
    if constexpr (VEC) {
        const long long a0f = p0 & ~3LL;
        const int lead = (int)(p0 - a0f);
        for (int q = tid; q < ((lead + count + 3) >> 2); q += THREADS) {
            const long long g = a0f + 4 * q;
            bq_f4 v;
            if (g + 3 < length) {
                v = *reinterpret_cast<const bq_f4*>(src + g);
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
                if (j >= 0 && j < count) put(j, e[k]);
            }
        }
    } else {
        for (int j = tid; j < count; j += THREADS) put(j, src[p0 + j]);
    }
}

__device__ __forceinline__ void bq_apply(const BqMat& m, double u0, double u1, double& s0, double& s1) {
    s0 += m.a * u0 + m.b * u1;
    s1 += m.c * u0 + m.d * u1;
}

// pass 1: the zero-state response of the chunk whose feed-forward part is v, end state only
__device__ __forceinline__ void bq_pass1(const BqSection& P, const double (&v)[BQ_C], double& s0, double& s1) {
    s0 = s1 = 0.0;
#pragma unroll
    for (int k = 0; k < BQ_C; ++k) {
        const double y = fma(-P.a1, s0, fma(-P.a2, s1, v[k]));
        s1 = s0;
        s0 = y;
    }
}

// The state (y[c0 - 1], y[c0 - 2]) the lane's chunk starts from, given the chunk's feed-forward part v and the state (in0, in1) the
// TILE starts from (used by thread 0 alone).  Wave 0 scans the waves' end states and publishes them: two barriers.
__device__ __forceinline__ void bq_incoming_published(const BqSection& P, const double (&v)[BQ_C], double (*wave_state)[BQ_WAVES][2],
                                                      int tid, double& in0, double& in1) {
    const int lane = tid & 63, wave = tid >> 6;
    double s0, s1;
    bq_pass1(P, v, s0, s1);
    if (tid == 0) bq_apply(P.p[0], in0, in1, s0, s1);           // the previous tile's carry, by linearity (zero in tile 0)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double u0 = __shfl_up(s0, 1 << i), u1 = __shfl_up(s1, 1 << i);
        if (lane >= (1 << i)) bq_apply(P.p[i], u0, u1, s0, s1);
    }
    double e0 = __shfl_up(s0, 1), e1 = __shfl_up(s1, 1);         // the wave-local state before the lane's chunk
    if (lane == 0) e0 = e1 = 0.0;
    if (lane == 63) {
        wave_state[0][wave][0] = s0;
        wave_state[0][wave][1] = s1;
    }
    __syncthreads();
    if (wave == 0) {
        double w0 = lane < BQ_WAVES ? wave_state[0][lane][0] : 0.0;
        double w1 = lane < BQ_WAVES ? wave_state[0][lane][1] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double u0 = __shfl_up(w0, 1 << i), u1 = __shfl_up(w1, 1 << i);
            if (lane >= (1 << i)) bq_apply(P.p[6 + i], u0, u1, w0, w1);
        }
        if (lane < BQ_WAVES) {
            wave_state[1][lane][0] = w0;
            wave_state[1][lane][1] = w1;
        }
    }
    __syncthreads();
    if (tid > 0) {
        in0 = e0;
        in1 = e1;
    }
    if (wave > 0) {             // the state at the end of the previous wave, carried over the lane's `lane` chunks: M^(C lane) by its bits
        double u0 = wave_state[1][wave - 1][0], u1 = wave_state[1][wave - 1][1];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if ((lane >> i) & 1) {
                double m0 = 0.0, m1 = 0.0;
                bq_apply(P.p[i], u0, u1, m0, m1);
                u0 = m0;
                u1 = m1;
            }
        }
        in0 += u0;
        in1 += u1;
    }
}

}  // namespace tac
