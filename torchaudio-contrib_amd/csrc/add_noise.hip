// add_noise.hip — functional.add_noise / AddNoise: noise mixed into a waveform at a given signal-to-noise ratio, and its gradient.
//
//   m_t   = t < len_r                  (len_r = L without lengths, else lengths[r] clamped to [0, L])
//   E_s   = sum_t (w_t m_t)^2          E_n = sum_t (n_t m_t)^2
//   scale = sqrt(E_s / E_n) 10^(-snr_r / 20)              (= 10^((10 (log10 E_s - log10 E_n) - snr_r) / 20))
//   out_t = w_t + scale n_t            for EVERY t < L, masked or not
//
// A row (10 s at 16 kHz: 1.28 MB of waveform and noise) does not stay on a CU between its sums and its mix, and a row per workgroup
// would leave most CUs idle on a few long rows.  So there is ONE form, uniform in the shape: three launches on the caller's stream
// behind one entry point, no host wait between them.  A unit is one tile of AN_TILE samples of one row.
//
//   an_reduce_kernel   persistent over the units.  Each thread accumulates its samples in float64 (the products of two floats are
//                      exact there), in a fixed order: per lane by ascending position, per wave by a butterfly of xor shuffles, per
//                      tile wave 0 .. 3.  The tile's (E_s, E_n, d) go to a float64 workspace [rows][tiles][3].  Samples at or
//                      behind len_r are SELECTED out, not multiplied out, and a tile wholly behind len_r writes zeros without a
//                      load: a NaN or padding garbage behind a row's length does not reach its scale.
//   an_scale_kernel    a wave per row sums the row's partials — lane l the tiles l, l + 64, … in ascending order, then the same
//                      butterfly — forms scale in float64 and writes the row's coefficients behind the partials.  (A tiny third
//                      kernel rather than a last-workgroup step of the first: no counters, no fences, nothing to zero per call,
//                      and a row of 704 tiles is not summed again by each of its 704 units.)
//   an_mix_kernel      the same units; reads the row's coefficients (every workgroup of a row the same bits), rounds scale to
//                      float32 ONCE and writes out = fma(scale32, n, w).  It walks the units in the REVERSE of the reduce kernel's
//                      order (TAC_AN_MIX_REVERSE, measured: DESIGN 3.18), so that the tiles read last are re-read first.
//
// Special values are those of the float64 expression: E_s = 0 gives 0, E_n = 0 gives inf, both (a row with len_r = 0) NaN.
//
// Gradient (tac_add_noise_grad_f32): the same three kernels in adjoint mode.  The reduce kernel takes grad_out as a third operand
// and adds d = sum_t g_t n_t over ALL t; with c_w = (scale / E_s) d and c_n = (scale / E_n) d in float64, rounded once,
//   g_wave_t  = fma(c_w, w_t, g_t)  under the mask,  g_t        behind it
//   g_noise_t = scale g_t - c_n n_t under the mask,  scale g_t  behind it
//   g_snr     = -(ln 10 / 20) scale d                            (written by an_scale_kernel)
// and the mix kernel writes both gradients in one pass over g, w and n.
//
// Loads and stores are 16-byte chunks where every operand has unit time stride, a base and a row stride that keep the chunks
// aligned, and L % 4 == 0; dwords otherwise (any positive time stride).  Row r = o * rows_inner + i of an operand starts at
// o * stride_o + i * stride_r, and either stride may be 0: one noise row for every row, or one per batch entry for its channels.  snr (float32) and lengths (int32 or int64) are DEVICE tables of one entry or one per row.  One writer per element,
// no atomics: bit-identical from run to run.
#include "host_common.hpp"

#ifndef TAC_AN_MIX_REVERSE
#define TAC_AN_MIX_REVERSE 1
#endif
#ifndef TAC_AN_PER_CU
#define TAC_AN_PER_CU 32
#endif

namespace tac {

typedef float an_f4 __attribute__((ext_vector_type(4)));

constexpr int AN_THREADS = 256;
constexpr int AN_PASSES = 4;
constexpr int AN_TILE = AN_THREADS * 4 * AN_PASSES;
constexpr int AN_WAVES = AN_THREADS / 64;
constexpr int AN_ROW_SLOTS = 4;                  // float64 per row behind the partials: scale, c_w, c_n, (free)

struct AnGeom {
    long long rows, L;
    long long w_so, w_sr, w_st, n_so, n_sr, n_st, g_so, g_sr, g_st;  // outer, row and time strides, in floats
    unsigned tiles, inner;                       // tiles per row; rows per outer index: row r lies at (r / inner) so + (r % inner) sr
    long long snr_stride, len_stride;            // 0: one entry for every row; 1: one per row
    unsigned units;                              // rows * tiles
    int len_i64;
};

__device__ __forceinline__ long long an_len(const AnGeom& g, const void* __restrict__ lengths, long long row) {
    if (!lengths) return g.L;
    const long long i = row * g.len_stride;
    const long long v = g.len_i64 ? static_cast<const long long*>(lengths)[i] : (long long)static_cast<const int*>(lengths)[i];
    return v < 0 ? 0 : (v > g.L ? g.L : v);
}

// where row r of an operand starts: one noise row per batch entry serves its channels with so = its row stride, sr = 0
__device__ __forceinline__ long long an_row(const AnGeom& g, unsigned row, long long so, long long sr) {
    return (long long)(row / g.inner) * so + (long long)(row % g.inner) * sr;
}

__device__ __forceinline__ double an_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// samples of the tile starting at t0 that lie below `end`: 0 .. AN_TILE
__device__ __forceinline__ int an_below(long long end, long long t0) {
    const long long k = end - t0;
    return (int)(k < 0 ? 0 : (k > AN_TILE ? AN_TILE : k));
}

template <bool VEC, bool GRAD>
__global__ void __launch_bounds__(AN_THREADS)
an_reduce_kernel(const float* __restrict__ w, const float* __restrict__ n, const float* __restrict__ go, AnGeom g,
                 const void* __restrict__ lengths, double* __restrict__ ws) {
    __shared__ double part[2][AN_WAVES][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int par = 0;
    for (unsigned u = blockIdx.x; u < g.units; u += gridDim.x, par ^= 1) {
        const unsigned row = u / g.tiles;
        const long long t0 = (long long)(u % g.tiles) * AN_TILE;
        const int in_mask = an_below(an_len(g, lengths, row), t0), in_row = an_below(g.L, t0);
        const int n_end = GRAD ? in_row : in_mask;               // d runs over all of the row
        const float* wp = w + an_row(g, row, g.w_so, g.w_sr);
        const float* np = n + an_row(g, row, g.n_so, g.n_sr);
        const float* gp = GRAD ? go + an_row(g, row, g.g_so, g.g_sr) : nullptr;
        double es = 0.0, en = 0.0, d = 0.0;
        if constexpr (VEC) {
            an_f4 wv[AN_PASSES], nv[AN_PASSES], gv[AN_PASSES];
#pragma unroll
            for (int p = 0; p < AN_PASSES; ++p) {
                const int i = (p * AN_THREADS + tid) * 4;
                wv[p] = nv[p] = gv[p] = an_f4{0.0f, 0.0f, 0.0f, 0.0f};
                if (i < in_mask) wv[p] = *reinterpret_cast<const an_f4*>(wp + t0 + i);
                if (i < n_end) nv[p] = *reinterpret_cast<const an_f4*>(np + t0 + i);
                if constexpr (GRAD)
                    if (i < in_row) gv[p] = *reinterpret_cast<const an_f4*>(gp + t0 + i);
            }
#pragma unroll
            for (int p = 0; p < AN_PASSES; ++p) {
                const int i = (p * AN_THREADS + tid) * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool m = i + j < in_mask;
                    const double a = m ? (double)wv[p][j] : 0.0, b = (double)nv[p][j], bm = m ? b : 0.0;
                    es = fma(a, a, es);
                    en = fma(bm, bm, en);
                    if constexpr (GRAD) d = fma((double)gv[p][j], b, d);
                }
            }
        } else {
            constexpr int N = 4 * AN_PASSES;
            float wv[N], nv[N], gv[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int i = j * AN_THREADS + tid;
                wv[j] = nv[j] = gv[j] = 0.0f;
                if (i < in_mask) wv[j] = wp[(t0 + i) * g.w_st];
                if (i < n_end) nv[j] = np[(t0 + i) * g.n_st];
                if constexpr (GRAD)
                    if (i < in_row) gv[j] = gp[(t0 + i) * g.g_st];
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const bool m = j * AN_THREADS + tid < in_mask;
                const double a = m ? (double)wv[j] : 0.0, b = (double)nv[j], bm = m ? b : 0.0;
                es = fma(a, a, es);
                en = fma(bm, bm, en);
                if constexpr (GRAD) d = fma((double)gv[j], b, d);
            }
        }
        es = an_wave_sum(es);
        en = an_wave_sum(en);
        if constexpr (GRAD) d = an_wave_sum(d);
        if (lane == 0) {
            part[par][wave][0] = es;
            part[par][wave][1] = en;
            part[par][wave][2] = d;
        }
        __syncthreads();                 // (the buffer of the unit before this one is free again: two buffers, one barrier a unit)
        if (tid < 3) {
            double s = part[par][0][tid];
#pragma unroll
            for (int k = 1; k < AN_WAVES; ++k) s += part[par][k][tid];
            ws[(size_t)u * 3 + tid] = s;
        }
    }
}

// a wave per row: the row's partials in a fixed order, then its coefficients
template <bool GRAD>
__global__ void __launch_bounds__(64)
an_scale_kernel(AnGeom g, const float* __restrict__ snr, double* __restrict__ ws, float* __restrict__ grad_snr) {
    const int lane = threadIdx.x;
    double* fin = ws + (size_t)g.units * 3;
    for (long long row = blockIdx.x; row < g.rows; row += gridDim.x) {
        const double* p = ws + (size_t)row * g.tiles * 3;
        double es = 0.0, en = 0.0, d = 0.0;
        for (long long t = lane; t < g.tiles; t += 64) {
            es += p[t * 3];
            en += p[t * 3 + 1];
            if constexpr (GRAD) d += p[t * 3 + 2];
        }
        es = an_wave_sum(es);
        en = an_wave_sum(en);
        if constexpr (GRAD) d = an_wave_sum(d);
        if (lane == 0) {
            const double scale = sqrt(es / en) * pow(10.0, -(double)snr[row * g.snr_stride] / 20.0);
            fin[row * AN_ROW_SLOTS] = scale;
            if constexpr (GRAD) {
                fin[row * AN_ROW_SLOTS + 1] = scale / es * d;
                fin[row * AN_ROW_SLOTS + 2] = scale / en * d;
                if (grad_snr) grad_snr[row] = (float)(-0.11512925464970228420 * scale * d);      // ln 10 / 20
            }
        }
    }
}

// Forward: a = w, b = n, out = fma(scale, n, w).  GRAD: a = w, b = n, go = grad_out; out = grad_wave and out2 = grad_noise, either
// may be null.
template <bool VEC, bool GRAD, bool REVERSE>
__global__ void __launch_bounds__(AN_THREADS)
an_mix_kernel(const float* __restrict__ w, const float* __restrict__ n, const float* __restrict__ go, AnGeom g,
              const void* __restrict__ lengths, const double* __restrict__ ws, float* __restrict__ out, float* __restrict__ out2) {
    const int tid = threadIdx.x;
    const double* fin = ws + (size_t)g.units * 3;
    for (unsigned v = blockIdx.x; v < g.units; v += gridDim.x) {
        const unsigned u = REVERSE ? g.units - 1 - v : v;
        const unsigned row = u / g.tiles;
        const long long t0 = (long long)(u % g.tiles) * AN_TILE;
        const int in_row = an_below(g.L, t0);
        const float scale = (float)fin[(size_t)row * AN_ROW_SLOTS];
        const float* wp = w + an_row(g, row, g.w_so, g.w_sr);
        const float* np = n + an_row(g, row, g.n_so, g.n_sr);
        float* op = out + (long long)row * g.L + t0;
        if constexpr (!GRAD) {
            if constexpr (VEC) {
                an_f4 wv[AN_PASSES], nv[AN_PASSES];
#pragma unroll
                for (int p = 0; p < AN_PASSES; ++p) {
                    const int i = (p * AN_THREADS + tid) * 4;
                    if (i < in_row) {
                        wv[p] = *reinterpret_cast<const an_f4*>(wp + t0 + i);
                        nv[p] = *reinterpret_cast<const an_f4*>(np + t0 + i);
                    }
                }
#pragma unroll
                for (int p = 0; p < AN_PASSES; ++p) {
                    const int i = (p * AN_THREADS + tid) * 4;
                    if (i < in_row) {
                        an_f4 r;
#pragma unroll
                        for (int j = 0; j < 4; ++j) r[j] = __builtin_fmaf(scale, nv[p][j], wv[p][j]);
                        *reinterpret_cast<an_f4*>(op + i) = r;
                    }
                }
            } else {
#pragma unroll 1
                for (int h = 0; h < AN_PASSES; ++h) {            // four dwords of each operand in flight
                    float wv[4], nv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = (h * 4 + j) * AN_THREADS + tid;
                        if (i < in_row) {
                            wv[j] = wp[(t0 + i) * g.w_st];
                            nv[j] = np[(t0 + i) * g.n_st];
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = (h * 4 + j) * AN_THREADS + tid;
                        if (i < in_row) op[i] = __builtin_fmaf(scale, nv[j], wv[j]);
                    }
                }
            }
        } else {
            const int in_mask = an_below(an_len(g, lengths, row), t0);
            const float c_w = (float)fin[(size_t)row * AN_ROW_SLOTS + 1], c_n = (float)fin[(size_t)row * AN_ROW_SLOTS + 2];
            const float* gp = go + an_row(g, row, g.g_so, g.g_sr);
            float* op2 = out2 + (long long)row * g.L + t0;
            if constexpr (VEC) {
#pragma unroll 1
                for (int p = 0; p < AN_PASSES; ++p) {
                    const int i = (p * AN_THREADS + tid) * 4;
                    if (i >= in_row) continue;
                    const an_f4 zero = an_f4{0.0f, 0.0f, 0.0f, 0.0f};
                    const an_f4 gv = *reinterpret_cast<const an_f4*>(gp + t0 + i);
                    const an_f4 wv = (out && i < in_mask) ? *reinterpret_cast<const an_f4*>(wp + t0 + i) : zero;
                    const an_f4 nv = (out2 && i < in_mask) ? *reinterpret_cast<const an_f4*>(np + t0 + i) : zero;
                    an_f4 r, r2;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool m = i + j < in_mask;
                        r[j] = m ? __builtin_fmaf(c_w, wv[j], gv[j]) : gv[j];
                        r2[j] = m ? __builtin_fmaf(scale, gv[j], -(c_n * nv[j])) : scale * gv[j];
                    }
                    if (out) *reinterpret_cast<an_f4*>(op + i) = r;
                    if (out2) *reinterpret_cast<an_f4*>(op2 + i) = r2;
                }
            } else {
#pragma unroll 1
                for (int h = 0; h < AN_PASSES; ++h) {
                    float gv[4], wv[4], nv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = (h * 4 + j) * AN_THREADS + tid;
                        gv[j] = wv[j] = nv[j] = 0.0f;
                        if (i < in_row) gv[j] = gp[(t0 + i) * g.g_st];
                        if (out && i < in_mask) wv[j] = wp[(t0 + i) * g.w_st];
                        if (out2 && i < in_mask) nv[j] = np[(t0 + i) * g.n_st];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = (h * 4 + j) * AN_THREADS + tid;
                        if (i < in_row) {
                            const bool m = i < in_mask;
                            if (out) op[i] = m ? __builtin_fmaf(c_w, wv[j], gv[j]) : gv[j];
                            if (out2) op2[i] = m ? __builtin_fmaf(scale, gv[j], -(c_n * nv[j])) : scale * gv[j];
                        }
                    }
                }
            }
        }
    }
}

struct AnOperand {
    const float* p;
    long long so, sr, st;                        // outer, row and time stride
};

inline bool an_chunks(const AnOperand& a) {
    return a.st == 1 && a.so % 4 == 0 && a.sr % 4 == 0 && (reinterpret_cast<uintptr_t>(a.p) & 15) == 0;
}

// the three launches of one call; go.p == nullptr: the forward
static int an_launch(AnOperand go, AnOperand w, AnOperand n, long long rows, long long inner, long long L, const float* snr,
                     long long snr_rows, const void* lengths, long long len_rows, int len_i64, void* work, float* out, float* out2,
                     float* grad_snr, hipStream_t stream) {
    const bool grad = go.p != nullptr;
    if (!w.p || !n.p || !snr || !work || rows <= 0 || L <= 0 || inner <= 0 || rows % inner != 0) return TAC_E_INVALID;
    if (grad ? (!out && !out2 && !grad_snr) : !out) return TAC_E_INVALID;
    if ((snr_rows != 1 && snr_rows != rows) || (lengths && len_rows != 1 && len_rows != rows)) return TAC_E_INVALID;
    for (AnOperand* a : {&go, &w, &n}) {
        if (inner == 1) a->sr = 0;
        if (inner == rows) a->so = 0;
        if (L == 1) a->st = 1;
        if (a->p && (a->so < 0 || a->sr < 0 || a->st <= 0)) return TAC_E_INVALID;
    }
    AnGeom g;
    g.rows = rows, g.L = L;
    g.w_so = w.so, g.w_sr = w.sr, g.w_st = w.st, g.n_so = n.so, g.n_sr = n.sr, g.n_st = n.st, g.g_so = go.so, g.g_sr = go.sr, g.g_st = go.st;
    g.snr_stride = snr_rows == rows && rows > 1 ? 1 : 0;
    g.len_stride = lengths && len_rows == rows && rows > 1 ? 1 : 0;
    g.len_i64 = len_i64 ? 1 : 0;
    const long long tiles = (L + AN_TILE - 1) / AN_TILE;
    if ((double)rows * (double)tiles > 2147483647.0) return TAC_E_UNSUPPORTED;
    const long long units = rows * tiles;
    g.tiles = (unsigned)tiles, g.inner = (unsigned)inner, g.units = (unsigned)units;
    const bool vec = L % 4 == 0 && an_chunks(w) && an_chunks(n) && (!grad || an_chunks(go)) &&
                     (!out || (reinterpret_cast<uintptr_t>(out) & 15) == 0) && (!out2 || (reinterpret_cast<uintptr_t>(out2) & 15) == 0);
    const long long blocks = persistent_blocks(units, 1, (long long)device_cu_count() * TAC_AN_PER_CU);
    const long long row_blocks = persistent_blocks(rows, 1, (long long)device_cu_count() * TAC_AN_PER_CU);
    double* ws = static_cast<double*>(work);
    int rc;
    if (grad) {
        rc = launch_kernel(vec ? an_reduce_kernel<true, true> : an_reduce_kernel<false, true>, blocks, AN_THREADS, 0, stream, w.p, n.p,
                           go.p, g, lengths, ws);
        if (rc != TAC_OK) return rc;
        rc = launch_kernel(an_scale_kernel<true>, row_blocks, 64, 0, stream, g, snr, ws, grad_snr);
        if (rc != TAC_OK || (!out && !out2)) return rc;
        return launch_kernel(vec ? an_mix_kernel<true, true, TAC_AN_MIX_REVERSE != 0> : an_mix_kernel<false, true, TAC_AN_MIX_REVERSE != 0>,
                             blocks, AN_THREADS, 0, stream, w.p, n.p, go.p, g, lengths, (const double*)ws, out, out2);
    }
    rc = launch_kernel(vec ? an_reduce_kernel<true, false> : an_reduce_kernel<false, false>, blocks, AN_THREADS, 0, stream, w.p, n.p,
                       go.p, g, lengths, ws);
    if (rc != TAC_OK) return rc;
    rc = launch_kernel(an_scale_kernel<false>, row_blocks, 64, 0, stream, g, snr, ws, grad_snr);
    if (rc != TAC_OK) return rc;
    return launch_kernel(vec ? an_mix_kernel<true, false, TAC_AN_MIX_REVERSE != 0> : an_mix_kernel<false, false, TAC_AN_MIX_REVERSE != 0>,
                         blocks, AN_THREADS, 0, stream, w.p, n.p, go.p, g, lengths, (const double*)ws, out, out2);
}

}  // namespace tac

extern "C" {

int64_t tac_add_noise_tile(void) { return tac::AN_TILE; }

int64_t tac_add_noise_work_bytes(int64_t rows, int64_t length) {
    if (rows <= 0 || length <= 0) return 0;
    const long long tiles = (length + tac::AN_TILE - 1) / tac::AN_TILE;
    if ((double)rows * (double)tiles > 2147483647.0) return 0;
    return (int64_t)sizeof(double) * (rows * tiles * 3 + rows * tac::AN_ROW_SLOTS);
}

int tac_add_noise_f32(const float* waveform, int64_t w_stride_o, int64_t w_stride_r, int64_t w_stride_t, const float* noise,
                      int64_t n_stride_o, int64_t n_stride_r, int64_t n_stride_t, int64_t rows, int64_t rows_inner, int64_t length,
                      const float* snr, int64_t snr_rows, const void* lengths, int64_t length_rows, int32_t lengths_i64, void* work,
                      float* out, void* stream) {
    return tac::an_launch({nullptr, 0, 0, 1}, {waveform, w_stride_o, w_stride_r, w_stride_t}, {noise, n_stride_o, n_stride_r, n_stride_t},
                          rows, rows_inner, length, snr, snr_rows, lengths, length_rows, lengths_i64, work, out, nullptr, nullptr,
                          (hipStream_t)stream);
}

int tac_add_noise_grad_f32(const float* grad_out, int64_t g_stride_o, int64_t g_stride_r, int64_t g_stride_t, const float* waveform,
                           int64_t w_stride_o, int64_t w_stride_r, int64_t w_stride_t, const float* noise, int64_t n_stride_o,
                           int64_t n_stride_r, int64_t n_stride_t, int64_t rows, int64_t rows_inner, int64_t length, const float* snr,
                           int64_t snr_rows, const void* lengths, int64_t length_rows, int32_t lengths_i64, void* work,
                           float* grad_waveform, float* grad_noise, float* grad_snr, void* stream) {
    if (!grad_out) return TAC_E_INVALID;
    return tac::an_launch({grad_out, g_stride_o, g_stride_r, g_stride_t}, {waveform, w_stride_o, w_stride_r, w_stride_t},
                          {noise, n_stride_o, n_stride_r, n_stride_t}, rows, rows_inner, length, snr, snr_rows, lengths, length_rows,
                          lengths_i64, work, grad_waveform, grad_noise, grad_snr, (hipStream_t)stream);
}

}  // extern "C"
