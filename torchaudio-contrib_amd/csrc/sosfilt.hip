// sosfilt.hip — functional.sosfilt (and filtfilt above order 2): a cascade of up to SOS_MAX second-order sections along the last
// axis and, with `reverse`, its adjoint (the sections in reverse order, each run from the end of the row), in ONE launch.
//
//   section s:  y_s[n] = b0 u_s[n] + b1 u_s[n-1] + b2 u_s[n-2] - a1 y_s[n-1] - a2 y_s[n-2],   u_0 = x,  u_{s+1} = y_s
//   (each section's coefficients already divided by its a0; zero initial state)
//
// The tile walk is lfilter.hip's: a row belongs to ONE workgroup, which walks it in tiles of SO_TILE = 1024 * SO_C samples; lane l
// owns samples [l*C, l*C + C) of the tile.  What is new is that the lane keeps its chunk as C doubles in registers across all
// sections: the waveform is read once as float32 and written once as float32, and nothing between two sections is ever rounded to
// float32 or leaves the chip.  Per tile
//   global -> xs           as lfilter.hip (16 bytes per lane where the row is aligned), stored in time order; chunk -> registers
//   for each section       numerator taps in place (from the chunk's last sample down, so every tap still reads the section's
//                          input); pass 1 from zero state; the Kogge-Stone scan over M_s^(C 2^i) — six steps in the wave by
//                          cross-lane moves, then the sixteen wave states through the LDS, scanned by EVERY wave for itself (four
//                          steps on sixteen lanes: cheaper than a second barrier) — and pass 2 in place.  One barrier per section.
//   history                the two samples a section's numerator needs from before the lane's chunk are the preceding section's
//                          outputs there, y_{s-1}[c0 - 1], y_{s-1}[c0 - 2]: exactly the state that section's scan handed the lane
//                          for its pass 2, so they cost nothing.  (Behind a section without recursion, whose scan is skipped, they
//                          come from the neighbouring lane by a one-lane shift, and across waves through the LDS.)
//   carry                  hist[tile & 1][s]: the last lane's last two inputs of section s (= outputs of section s - 1, = that
//                          section's state), s = 0 .. S, for lane 0 of the workgroup's next tile of the same row; two copies by the
//                          tile's parity, so a tile never overwrites what it still reads.
//   registers -> xs        rounded to float32 once, clamped; coalesced stores
// Coefficients that are exactly zero are not multiplied, as in lfilter.hip, and a section with a1 == a2 == 0 skips pass 1 and the
// scan.  Nothing is shared between rows and the scan moves values to later lanes only, so a non-finite sample reaches the samples
// after it in its own row and nothing else.  No atomics, no workspace, one writer per element: bit-identical from run to run.
//
// The sections' parameters (45 doubles each, 2880 bytes for eight) are a kernel argument: the section loop indexes it with a
// wave-uniform counter, which the compiler turns into scalar loads from the kernarg segment — no table to upload or cache.
//
// (The tile geometry, a section's parameters and the routine that fills them restate lfilter.hip's under names of their own: that
// file's text is pinned by tests/grid_rules.py and stays as it is.  tac_sosfilt_tile() == 1024 * tac_lfilter_chunk() is asserted by
// the Python side.)
#include <math.h>

#include "host_common.hpp"

namespace tac {

typedef float so_f4 __attribute__((ext_vector_type(4)));

constexpr int SO_C_LOG = 4;
constexpr int SO_C = 1 << SO_C_LOG;             // samples per lane
constexpr int SO_THREADS = 1024;
constexpr int SO_WAVES = SO_THREADS / 64;
constexpr int SO_TILE = SO_THREADS * SO_C;      // samples per tile
constexpr int SO_XS = SO_TILE + SO_TILE / SO_C + 1;
constexpr int SO_STEPS = 10;                    // log2(SO_THREADS): M^(C 2^i), i < 10
static_assert(SO_WAVES == 16 && (1 << SO_STEPS) == SO_THREADS, "the scan is six steps in a wave and four across sixteen waves");
constexpr int SOS_MAX = 8;                      // sections per launch: order 16
constexpr int SOS_BLOCKS_PER_CU = 2;            // the persistent grid's cap (70 KB of LDS and 16 waves per workgroup)

struct SoMat { double a, b, c, d; };            // [[a, b], [c, d]]
struct SoSection {
    double b0, b1, b2, a1, a2;
    SoMat p[SO_STEPS];                          // p[i] = M^(C 2^i), M = [[-a1, -a2], [1, 0]]
};
struct SosParams { SoSection sec[SOS_MAX]; };   // in the order the kernel runs them (reversed by the host for the adjoint)

__device__ __forceinline__ int so_at(int i) { return i + (i >> SO_C_LOG); }     // xs is skewed by one float per chunk, as lfilter's

__device__ __forceinline__ void so_apply(const SoMat& m, double u0, double u1, double& s0, double& s1) {
    s0 += m.a * u0 + m.b * u1;
    s1 += m.c * u0 + m.d * u1;
}
static_assert(sizeof(SosParams) == SOS_MAX * 45 * sizeof(double) && sizeof(SosParams) + 64 <= 4096, "a kernel argument");

constexpr int SOS_HEAD = 4 * SO_WAVES + 4 * (SOS_MAX + 1);      // doubles in front of xs: wave_pair[2][16][2] | hist[2][S + 1][2]

template <bool VEC>
__global__ void __launch_bounds__(SO_THREADS)
sosfilt_kernel(const float* __restrict__ x, long long rows, long long length, long long stride_r, SosParams P, int n_sections,
               int clamp, int reverse, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double so_lds[];
    double (*wave_pair)[SO_WAVES][2] = reinterpret_cast<double (*)[SO_WAVES][2]>(so_lds);
    double (*hist)[SOS_MAX + 1][2] = reinterpret_cast<double (*)[SOS_MAX + 1][2]>(so_lds + 4 * SO_WAVES);
    float* xs = reinterpret_cast<float*>(so_lds + SOS_HEAD);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int c0 = tid * SO_C;                          // the lane's first sample, in time order within the tile
    const long long tiles = (length + SO_TILE - 1) / SO_TILE;

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* src = x + row * stride_r;
        float* dst = out + row * length;
        for (long long t = 0; t < tiles; ++t) {
            const long long n0 = t * SO_TILE;                                   // first sample of the tile in time order
            const int nt = (int)(length - n0 < SO_TILE ? length - n0 : SO_TILE);
            const long long p0 = reverse ? length - n0 - nt : n0;               // ... and where the tile starts in memory
            const int cur = (int)(t & 1);
            // ---- global -> xs, time order: memory offset j of the tile is sample (reverse ? nt - 1 - j : j)
            if constexpr (VEC) {
                const long long a0f = p0 & ~3LL;
                const int lead = (int)(p0 - a0f);
                for (int q = tid; q < ((lead + nt + 3) >> 2); q += SO_THREADS) {
                    const long long g = a0f + 4 * q;
                    so_f4 v;
                    if (g + 3 < length) {
                        v = *reinterpret_cast<const so_f4*>(src + g);
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
                        if (j >= 0 && j < nt) xs[so_at(reverse ? nt - 1 - j : j)] = e[k];
                    }
                }
            } else {
                for (int j = tid; j < nt; j += SO_THREADS) xs[so_at(reverse ? nt - 1 - j : j)] = src[p0 + j];
            }
            __syncthreads();

            // ---- the lane's chunk and the two samples before it (zero before the row and behind its end)
            double v[SO_C];
#pragma unroll
            for (int k = 0; k < SO_C; ++k) v[k] = c0 + k < nt ? (double)xs[so_at(c0 + k)] : 0.0;
            double h1 = 0.0, h2 = 0.0;                   // the running section's input at c0 - 1 and c0 - 2
            if (tid > 0) {
                if (c0 - 1 < nt) h1 = (double)xs[so_at(c0 - 1)];
                if (c0 - 2 < nt) h2 = (double)xs[so_at(c0 - 2)];
            } else if (t > 0) {
                h1 = hist[cur ^ 1][0][0];
                h2 = hist[cur ^ 1][0][1];
            }
            if (tid == SO_THREADS - 1) {
                hist[cur][0][0] = v[SO_C - 1];
                hist[cur][0][1] = v[SO_C - 2];
            }

            int buf = 0;                                 // which half of wave_pair this section's barrier guards
#pragma unroll 1
            for (int s = 0; s < n_sections; ++s) {
                const SoSection& Q = P.sec[s];
                // ---- numerator, in place from the last sample down: v[k - 1], v[k - 2] are still the section's input
#pragma unroll
                for (int k = SO_C - 1; k >= 0; --k) {
                    const double p1 = k >= 1 ? v[k - 1] : h1;
                    const double p2 = k >= 2 ? v[k - 2] : (k == 1 ? h1 : h2);
                    double acc = Q.b0 * v[k];
                    if (Q.b1 != 0.0) acc = fma(Q.b1, p1, acc);
                    if (Q.b2 != 0.0) acc = fma(Q.b2, p2, acc);
                    v[k] = acc;
                }
                double in0 = 0.0, in1 = 0.0;             // the section's output at c0 - 1 and c0 - 2: the state the chunk starts from
                if (tid == 0 && t > 0) {
                    in0 = hist[cur ^ 1][s + 1][0];
                    in1 = hist[cur ^ 1][s + 1][1];
                }
                if (Q.a1 != 0.0 || Q.a2 != 0.0) {
                    // ---- pass 1: zero-state response of the chunk, end state only
                    double s0 = 0.0, s1 = 0.0;
#pragma unroll
                    for (int k = 0; k < SO_C; ++k) {
                        const double y = fma(-Q.a1, s0, fma(-Q.a2, s1, v[k]));
                        s1 = s0;
                        s0 = y;
                    }
                    if (tid == 0) so_apply(Q.p[0], in0, in1, s0, s1);       // the previous tile's carry, by linearity (zero in tile 0)
                    // ---- scan across the lanes of the wave
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        const double u0 = __shfl_up(s0, 1 << i), u1 = __shfl_up(s1, 1 << i);
                        if (lane >= (1 << i)) so_apply(Q.p[i], u0, u1, s0, s1);
                    }
                    double e0 = __shfl_up(s0, 1), e1 = __shfl_up(s1, 1);     // the wave-local state before the lane's chunk
                    if (lane == 0) e0 = e1 = 0.0;
                    if (lane == 63) {
                        wave_pair[buf][wave][0] = s0;
                        wave_pair[buf][wave][1] = s1;
                    }
                    __syncthreads();
                    // ---- ... and across the sixteen waves: every wave scans the sixteen states for itself
                    double w0 = lane < SO_WAVES ? wave_pair[buf][lane][0] : 0.0;
                    double w1 = lane < SO_WAVES ? wave_pair[buf][lane][1] : 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double u0 = __shfl_up(w0, 1 << i), u1 = __shfl_up(w1, 1 << i);
                        if (lane >= (1 << i)) so_apply(Q.p[6 + i], u0, u1, w0, w1);
                    }
                    double u0 = __shfl(w0, wave > 0 ? wave - 1 : 0), u1 = __shfl(w1, wave > 0 ? wave - 1 : 0);
                    if (tid > 0) {
                        in0 = e0;
                        in1 = e1;
                    }
                    // the state at the end of the previous wave, carried over the lane's `lane` chunks: M^(C lane) by the bits of lane
                    if (wave > 0) {
#pragma unroll
                        for (int i = 0; i < 6; ++i) {
                            if ((lane >> i) & 1) {
                                double m0 = 0.0, m1 = 0.0;
                                so_apply(Q.p[i], u0, u1, m0, m1);
                                u0 = m0;
                                u1 = m1;
                            }
                        }
                        in0 += u0;
                        in1 += u1;
                    }
                    h1 = in0;                            // the next section's input before the chunk
                    h2 = in1;
                    // ---- pass 2: the chunk from its true incoming state, in place
#pragma unroll
                    for (int k = 0; k < SO_C; ++k) {
                        const double y = fma(-Q.a1, in0, fma(-Q.a2, in1, v[k]));
                        in1 = in0;
                        in0 = y;
                        v[k] = y;
                    }
                } else {
                    // ---- no recursion: the chunk is done; the next section's history comes from the neighbouring lane
                    double n1 = __shfl_up(v[SO_C - 1], 1), n2 = __shfl_up(v[SO_C - 2], 1);
                    if (lane == 63) {
                        wave_pair[buf][wave][0] = v[SO_C - 1];
                        wave_pair[buf][wave][1] = v[SO_C - 2];
                    }
                    __syncthreads();
                    if (lane == 0) {
                        n1 = wave > 0 ? wave_pair[buf][wave - 1][0] : in0;
                        n2 = wave > 0 ? wave_pair[buf][wave - 1][1] : in1;
                    }
                    h1 = n1;
                    h2 = n2;
                }
                buf ^= 1;
                if (tid == SO_THREADS - 1) {             // read by lane 0 in the next tile, behind the barriers in between
                    hist[cur][s + 1][0] = v[SO_C - 1];
                    hist[cur][s + 1][1] = v[SO_C - 2];
                }
            }

            // ---- registers -> xs (every lane read its neighbour's samples before the first section's barrier)
#pragma unroll
            for (int k = 0; k < SO_C; ++k) {
                float yf = (float)v[k];
                if (clamp) yf = yf < -1.0f ? -1.0f : (yf > 1.0f ? 1.0f : yf);      // (a NaN stays a NaN)
                if (c0 + k < nt) xs[so_at(c0 + k)] = yf;
            }
            __syncthreads();
            for (int j = tid; j < nt; j += SO_THREADS) dst[p0 + j] = xs[so_at(reverse ? nt - 1 - j : j)];
            __syncthreads();                            // nobody reads xs any more: the next tile may overwrite it
        }
    }
}

inline SoMat so_mul(const SoMat& x, const SoMat& y) {
    return SoMat{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}

// One section, normalised by its a0, and its ten powers — lfilter.hip's lf_params rule: TAC_E_INVALID for a zero or non-finite a0
// (or a coefficient that is not finite after the division), TAC_E_UNSUPPORTED where a power is not finite.
inline int so_section(const double* b, const double* a, SoSection* P) {
    if (!(a[0] != 0.0) || !isfinite(a[0])) return TAC_E_INVALID;
    double bn[3], an[3];
    for (int k = 0; k < 3; ++k) {
        bn[k] = b[k] / a[0];
        an[k] = a[k] / a[0];
        if (!isfinite(bn[k]) || !isfinite(an[k])) return TAC_E_INVALID;
    }
    P->b0 = bn[0];
    P->b1 = bn[1];
    P->b2 = bn[2];
    P->a1 = an[1];
    P->a2 = an[2];
    const SoMat m{-an[1], -an[2], 1.0, 0.0};
    SoMat q = m;
    for (int k = 1; k < SO_C; ++k) q = so_mul(q, m);
    for (int i = 0; i < SO_STEPS; ++i) {
        if (!isfinite(q.a) || !isfinite(q.b) || !isfinite(q.c) || !isfinite(q.d)) return TAC_E_UNSUPPORTED;
        P->p[i] = q;
        q = so_mul(q, q);
    }
    return TAC_OK;
}

// The sections of `sos` (rows b0 b1 b2 a0 a1 a2) in the order the kernel runs them.
inline int sos_params(const double* sos, int n_sections, int reverse, SosParams* P) {
    if (!sos || n_sections < 1) return TAC_E_INVALID;
    if (n_sections > SOS_MAX) return TAC_E_UNSUPPORTED;
    *P = SosParams{};
    int worst = TAC_OK;
    for (int s = 0; s < n_sections; ++s) {
        const double* row = sos + 6 * (reverse ? n_sections - 1 - s : s);
        const int rc = so_section(row, row + 3, &P->sec[s]);
        if (rc == TAC_E_INVALID) return rc;
        if (rc != TAC_OK) worst = rc;
    }
    return worst;
}

}  // namespace tac

extern "C" {

int32_t tac_sosfilt_max_sections(void) { return tac::SOS_MAX; }
int32_t tac_sosfilt_tile(void) { return tac::SO_TILE; }
int32_t tac_sosfilt_blocks_per_cu(void) { return tac::SOS_BLOCKS_PER_CU; }

int tac_sosfilt_supported(const double* sos, int32_t n_sections) {
    tac::SosParams P;
    return tac::sos_params(sos, n_sections, 0, &P);
}

int tac_sosfilt_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const double* sos, int32_t n_sections,
                    int clamp, int reverse, float* out, void* stream) {
    using namespace tac;
    if (!x || !out || rows <= 0 || length <= 0) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    SosParams P;
    const int rc = sos_params(sos, n_sections, reverse ? 1 : 0, &P);
    if (rc != TAC_OK) return rc;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_r & 3) == 0;
    const size_t bytes = SOS_HEAD * sizeof(double) + SO_XS * sizeof(float);
    const long long blocks = persistent_blocks(rows, 1, (long long)device_cu_count() * SOS_BLOCKS_PER_CU);
    auto kern = vec ? sosfilt_kernel<true> : sosfilt_kernel<false>;
    return launch_kernel(kern, blocks, SO_THREADS, bytes, (hipStream_t)stream, x, (long long)rows, (long long)length,
                         (long long)stride_r, P, (int)n_sections, clamp ? 1 : 0, reverse ? 1 : 0, out);
}

}  // extern "C"
