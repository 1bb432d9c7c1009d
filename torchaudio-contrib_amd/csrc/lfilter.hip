// lfilter.hip — functional.lfilter (and the biquads, pre-emphasis and de-emphasis on top of it): a recursive filter of order <= 2
// along the last axis and, with `reverse`, its adjoint (the same filter run from the end of the row), one streaming kernel.
//
//   y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2]          (coefficients already divided by a0; zero initial state)
//
// A row is walked from its start to its end by ONE workgroup, in tiles of BQ_TILE = 1024 * BQ_C consecutive samples; no workgroup
// ever waits on another.  The tile geometry, the skewed LDS array xs, the tile load, pass 1 and the scan are biquad_scan.hpp's.
// Per tile
//   global -> xs           the tile, coalesced (16 bytes per lane where the row is aligned), stored in time order
//   feed-forward           lane l owns samples [l*C, l*C + C): v[n] = sum b_k x[n-k] (the two samples before the chunk come from the
//                          neighbour's part of xs, or from the carried tail of the previous tile)
//   pass 1, scan           bq_incoming_published: the state the lane's chunk starts from, the carry of the previous tile entering
//                          by linearity
//   pass 2                 the recursion from the lane's true incoming state; clamp; into xs; coalesced stores
//   carry                  the last lane's state and last two x, for the workgroup's next tile of the same row
// The recursion, the scan and the state are float64, only loads and stores float32: with float32 state the rounded powers of a
// matrix with a near-double eigenvalue (poles next to z = 1, a 20 Hz high-pass at 48 kHz) cancel so badly that the scan loses the
// result.  Nothing is shared between rows and a lane's incoming state depends on earlier samples only, so a
// non-finite sample reaches the samples after it in its own row and nothing else.  No atomics, no workspace, one writer per
// element: bit-identical from run to run.
//
// Coefficients that are exactly zero are not multiplied (a1 == a2 == 0 — pre-emphasis, any FIR — skips pass 1 and the scan
// altogether).
#include "biquad_scan.hpp"

namespace tac {

// The tile in the words tests/grid_rules.py quotes, held to the shared header's; the kernel below uses the header's names.
constexpr int LF_C = BQ_C, LF_THREADS = BQ_THREADS;
constexpr int LF_TILE = LF_THREADS * LF_C;      // samples per tile
static_assert(LF_TILE == BQ_TILE, "lfilter walks biquad_scan.hpp's tile");

template <bool RECUR, bool VEC>
__global__ void __launch_bounds__(BQ_THREADS)
lfilter_kernel(const float* __restrict__ x, long long rows, long long length, long long stride_r, BqSection P, int clamp, int reverse,
               float* __restrict__ out) {
    // Dynamic LDS: wave_state[2][16][2] doubles ([0] the waves' own end states, [1] scanned across the waves) | carry_state[2]
    // doubles | carry_x[2] floats (+ 2 of padding) | xs[BQ_XS]
    extern __shared__ __attribute__((aligned(16))) double lf_lds[];
    double (*wave_state)[BQ_WAVES][2] = reinterpret_cast<double (*)[BQ_WAVES][2]>(lf_lds);
    double* carry_state = lf_lds + 4 * BQ_WAVES;
    float* carry_x = reinterpret_cast<float*>(carry_state + 2);
    float* xs = carry_x + 4;
    const int tid = threadIdx.x;
    const int c0 = tid * BQ_C;                          // the lane's first sample, in time order within the tile
    const long long tiles = (length + BQ_TILE - 1) / BQ_TILE;

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* src = x + row * stride_r;
        float* dst = out + row * length;
        for (long long t = 0; t < tiles; ++t) {
            const long long n0 = t * BQ_TILE;                                   // first sample of the tile in time order
            const int nt = (int)(length - n0 < BQ_TILE ? length - n0 : BQ_TILE);
            const long long p0 = reverse ? length - n0 - nt : n0;               // ... and where the tile starts in memory
            // ---- global -> xs, time order: memory offset j of the tile is sample (reverse ? nt - 1 - j : j)
            bq_load<VEC, BQ_THREADS>(src, length, p0, nt, tid, [=](int j, float e) { xs[bq_at(reverse ? nt - 1 - j : j)] = e; });
            __syncthreads();

            // ---- the lane's chunk and the two samples before it (zero before the row and behind its end)
            float xr[BQ_C];
#pragma unroll
            for (int k = 0; k < BQ_C; ++k) xr[k] = c0 + k < nt ? xs[bq_at(c0 + k)] : 0.0f;
            float xm1 = 0.0f, xm2 = 0.0f;
            double in0 = 0.0, in1 = 0.0;                 // the state the lane's chunk starts from: (y[c0 - 1], y[c0 - 2])
            if (tid > 0) {
                if (c0 - 1 < nt) xm1 = xs[bq_at(c0 - 1)];
                if (c0 - 2 < nt) xm2 = xs[bq_at(c0 - 2)];
            } else if (t > 0) {
                xm1 = carry_x[0];
                xm2 = carry_x[1];
                if constexpr (RECUR) {
                    in0 = carry_state[0];
                    in1 = carry_state[1];
                }
            }
            double v[BQ_C];
#pragma unroll
            for (int k = 0; k < BQ_C; ++k) {
                const float p1 = k >= 1 ? xr[k - 1] : xm1;
                const float p2 = k >= 2 ? xr[k - 2] : (k == 1 ? xm1 : xm2);
                double acc = P.b0 * (double)xr[k];
                if (P.b1 != 0.0) acc = fma(P.b1, (double)p1, acc);
                if (P.b2 != 0.0) acc = fma(P.b2, (double)p2, acc);
                v[k] = acc;
            }

            if constexpr (RECUR) {
                bq_incoming_published(P, v, wave_state, tid, in0, in1);     // pass 1 and the scan
            } else {
                __syncthreads();                        // every lane has read its neighbour's samples: xs may be overwritten
            }

            // ---- pass 2: the chunk from its true incoming state, into xs
#pragma unroll
            for (int k = 0; k < BQ_C; ++k) {
                double y = v[k];
                if constexpr (RECUR) {
                    y = fma(-P.a1, in0, fma(-P.a2, in1, y));
                    in1 = in0;
                    in0 = y;
                }
                float yf = (float)y;
                if (clamp) yf = yf < -1.0f ? -1.0f : (yf > 1.0f ? 1.0f : yf);      // (a NaN stays a NaN)
                if (c0 + k < nt) xs[bq_at(c0 + k)] = yf;
            }
            if (tid == BQ_THREADS - 1) {                // read by lane 0 in the next tile, behind the barriers in between
                if constexpr (RECUR) {
                    carry_state[0] = in0;
                    carry_state[1] = in1;
                }
                carry_x[0] = xr[BQ_C - 1];
                carry_x[1] = xr[BQ_C - 2];
            }
            __syncthreads();
            for (int j = tid; j < nt; j += BQ_THREADS) dst[p0 + j] = xs[bq_at(reverse ? nt - 1 - j : j)];
            __syncthreads();                            // nobody reads xs any more: the next tile may overwrite it
        }
    }
}

// bq_section behind the limit of this entry: at most three coefficients per side
inline int lf_params(const double* b, const double* a, int n, BqSection* P) {
    if (!b || !a || n < 1) return TAC_E_INVALID;
    if (n > 3) return TAC_E_UNSUPPORTED;
    return bq_section(b, a, n, P);
}

}  // namespace tac

extern "C" {

int32_t tac_lfilter_chunk(void) { return tac::LF_C; }

int tac_lfilter_supported(const double* b, const double* a, int32_t n_coeffs) {
    tac::BqSection P;
    return tac::lf_params(b, a, n_coeffs, &P);
}

int tac_lfilter_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const double* b, const double* a,
                    int32_t n_coeffs, int clamp, int reverse, float* out, void* stream) {
    using namespace tac;
    if (!x || !out || rows <= 0 || length <= 0) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    BqSection P;
    const int rc = lf_params(b, a, n_coeffs, &P);
    if (rc != TAC_OK) return rc;
    const bool recur = P.a1 != 0.0 || P.a2 != 0.0;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_r & 3) == 0;
    // 68 KiB of LDS and 16 waves per workgroup: two workgroups share a CU where the registers allow it
    const size_t bytes = (4 * BQ_WAVES + 2) * sizeof(double) + (4 + BQ_XS) * sizeof(float);
    const long long blocks = persistent_blocks(rows, 1, (long long)device_cu_count() * 2);
    auto kern = recur ? (vec ? lfilter_kernel<true, true> : lfilter_kernel<true, false>)
                      : (vec ? lfilter_kernel<false, true> : lfilter_kernel<false, false>);
    return launch_kernel(kern, blocks, BQ_THREADS, bytes, (hipStream_t)stream, x, (long long)rows, (long long)length,
                         (long long)stride_r, P, clamp ? 1 : 0, reverse ? 1 : 0, out);
}

}  // extern "C"
