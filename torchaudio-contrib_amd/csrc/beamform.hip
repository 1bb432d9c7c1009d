// beamform.hip — functional.psd / mvdr_weights_souden / apply_beamforming and the MVDR layer: torchaudio's mask-based Souden MVDR.
//
// A spectrogram is complex pairs X[b][c][f][t][2] with C = 2 .. 8 channels, read where it lies (four strides in floats).  A SYSTEM is
// one (batch entry, bin): g = b F + f, G = B F of them.  Lanes run along g, so with the frame-major layout the STFT kernels write
// (bins of a frame contiguous) a wave's 64 loads of one channel and frame are 512 contiguous bytes, and a lane reduces over time in
// its own registers: no cross-lane step in any of the Souden launches.
//
// Launch 1, psd_partial_kernel<C, NM>.  A wave takes 64 systems over one piece of 64 frames — the cut depends on nothing but the
// frame count, so a system's sums do not depend on what else is in the batch — and keeps, per PSD, the Hermitian triangle of
// sum_t m[t] X[c][t] conj(X[e][t]) in registers: C real and C (C - 1) / 2 complex float32 sums, and the mask sum in float64.  NM = 0: no mask; 1: one mask; 2: two PSDs from ONE pass over X,
// the second mask given or formed as 1 - m in the kernel.  A mask with a unit time stride (a contiguous (F, T) mask) is loaded
// along time into an LDS tile of 32 frames x 64 systems (row stride 65 words: conflict-free both ways) and read back along the
// systems; any other mask (frame-major) is read directly, coalesced.  The piece's sums go to part[psd][piece][component][g].
// Launch 2, psd_combine_kernel<C>.  A lane per (psd, component, system) adds the pieces in ascending order in float64, divides by
// the float64 mask sum + eps where normalize is set, rounds once and stores both triangles from the one value.  No atomics, a
// fixed order.
//
// mvdr_weights_kernel<C>.  A workgroup takes 16 systems: all 256 lanes fill the augmented matrices [psd_n | psd_s], C x 2C complex
// float64 in the LDS (element-major, system-minor: conflict-free 8-byte accesses), then a lane per system runs diagonal loading, elimination with partial pivoting (pivot: largest |re| +
// |im|), back substitution for the C right-hand sides, the complex trace, the division and the reference contraction, all float64;
// the result is rounded to float32 once.  It reads the float32 PSDs — or, inside tac_mvdr_souden_f32, the pieces of launch 1, which
// it sums by the very function launch 2 uses, so the fused entry gives the bits of the three entries called one after the other.
//
// apply_kernel<C>.  A wave takes 64 systems over 32 frames, the C conjugated weights in registers: out = sum_c conj(w[c]) X[c] as one
// fused multiply-add chain per component; every X element is read once, every output written once, as an 8-byte pair.
//
// rtf_evd_kernel<C>, rtf_power_kernel<C>, mvdr_weights_rtf_kernel<C>: the steering-vector (RTF) half, one launch each, float32 in,
// float64 on chip, one rounding per output, a system's result a function of that system alone.  rtf_power and mvdr_weights_rtf
// share the layout and the elimination of mvdr_weights_kernel; rtf_evd is Jacobi with a group of lanes per system, rows in
// registers and shuffles inside the group — the only cross-lane steps of this file.  tac_rtf_mvdr_f32 is mvdr_weights_rtf_kernel
// followed by apply_kernel.
#include <math.h>

#include <utility>

#include "host_common.hpp"

namespace tac {

constexpr int BF_THREADS = 256;
constexpr int BF_WAVES = BF_THREADS / 64;
constexpr int BF_TS = 32;                          // frames of a staged mask tile
constexpr int BF_LD = 65;                          // its row stride in words
constexpr int BF_TILE = BF_TS * BF_LD;             // words of one tile
constexpr int BF_CHUNK = 64;                       // frames of a piece of time: one wave's share of a system's sum
constexpr int BF_AP_FRAMES = 32;                   // frames of an apply unit
constexpr int BF_MAX_C = 8;
constexpr long long BF_MAX_FRAMES = (1LL << 31) - 1, BF_MAX_SYSTEMS = 1LL << 40;

inline int psd_plan(long long frames, int* chunk, int* chunks) {
    if (frames < 1 || frames > BF_MAX_FRAMES) return TAC_E_INVALID;
    *chunk = BF_CHUNK;
    *chunks = (int)((frames + BF_CHUNK - 1) / BF_CHUNK);
    return TAC_OK;
}

inline int bf_grid(int which, int cus) {
    if (cus <= 0) cus = device_cu_count();
    return which == 0 ? 2 * cus : 8 * cus;
}

struct SpecRef { const float* p; long long sb, sc, sf, st; };
struct MaskRef { const float* p; long long sb, sf, st; int staged; };

struct PsdArgs {
    SpecRef x;
    MaskRef ma, mb;
    long long F, T, G;
    long long wave_units, units;            // wave_units = tiles * chunks; a workgroup takes BF_WAVES consecutive ones
    int chunk, chunks, complement;
    float* part;                            // [psd][chunks][C * C][G]
    double* msum;                           // [psd][chunks][G]
};

struct PsdParts {
    const float* part;
    const double* msum;
    long long G;
    int chunks, normalize;
    double eps;
};

// the sum of a system's mask over every piece, + eps
__device__ __forceinline__ double psd_denominator(const PsdParts& P, int m, long long g) {
    double s = 0.0;
#pragma unroll 4
    for (int p = 0; p < P.chunks; ++p) s += P.msum[((long long)m * P.chunks + p) * P.G + g];
    return s + P.eps;
}

// component q of a system's PSD: the pieces in ascending order in float64, normalised, rounded once
__device__ __forceinline__ float psd_value(const PsdParts& P, int CC, int m, int q, long long g, double denom) {
    double s = 0.0;
#pragma unroll 8
    for (int p = 0; p < P.chunks; ++p) s += (double)P.part[(((long long)m * P.chunks + p) * CC + q) * P.G + g];
    return (float)(P.normalize ? s / denom : s);
}

// one frame into one PSD's sums: d[c] += w |x_c|^2, (re, im)[c (c - 1) / 2 + e] += w x_c conj(x_e) for e < c
template <int C, bool WEIGHTED>
__device__ __forceinline__ void psd_frame(const float2 (&x)[C], float w, float (&d)[C], float (&re)[C * (C - 1) / 2 + 1],
                                          float (&im)[C * (C - 1) / 2 + 1]) {
    int k = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float yr = WEIGHTED ? w * x[c].x : x[c].x, yi = WEIGHTED ? w * x[c].y : x[c].y;
        d[c] = fmaf(yr, x[c].x, fmaf(yi, x[c].y, d[c]));
#pragma unroll
        for (int e = 0; e < c; ++e, ++k) {
            re[k] = fmaf(yr, x[e].x, fmaf(yi, x[e].y, re[k]));
            im[k] = fmaf(yi, x[e].x, fmaf(-yr, x[e].y, im[k]));
        }
    }
}

// a wave's tile of a time-contiguous mask: frames [ts, t1) x the wave's 64 systems, loaded along time, zero outside.  rowoff is
// the calling lane's OWN row offset b stride_b + f stride_f (-1: the lane has no system); the row of system gl comes by a
// shuffle, and every load is unconditional (a clamped address, the value selected afterwards) so that all of them are in flight
// together.  Called by whole waves.
__device__ __forceinline__ void bf_stage(float* tile, const MaskRef& M, long long rowoff, long long ts, long long t1, int lane) {
    const int tk = lane & (BF_TS - 1), half = lane >> 5;
    const long long tt = ts + tk;
    const bool in_time = tt < t1;
#pragma unroll 8
    for (int i = 0; i < 32; ++i) {
        const int gl = half + 2 * i;
        const long long off = __shfl(rowoff, gl, 64);
        const bool take = in_time && off >= 0;
        const float v = M.p[take ? off + tt * M.st : 0];
        tile[tk * BF_LD + gl] = take ? v : 0.0f;
    }
}

template <int C, int NM>
__global__ void __launch_bounds__(BF_THREADS)
psd_partial_kernel(const PsdArgs A) {
    extern __shared__ __align__(16) unsigned char bf_lds[];
    constexpr int NP = NM == 2 ? 2 : 1, TRI = C * (C - 1) / 2, CC = C * C;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* tile_a = reinterpret_cast<float*>(bf_lds) + wave * BF_TILE;
    float* tile_b = reinterpret_cast<float*>(bf_lds) + (BF_WAVES + wave) * BF_TILE;
    const bool stage_a = NM >= 1 && A.ma.staged, stage_b = NM == 2 && !A.complement && A.mb.staged;
    const int subs = (A.chunk + BF_TS - 1) / BF_TS;

    for (long long u = blockIdx.x; u < A.units; u += gridDim.x) {          // (the same trips for every wave: the barriers below)
        const long long wu = u * BF_WAVES + wave;
        const bool live = wu < A.wave_units;
        const long long tl = live ? wu / A.chunks : 0;
        const int p = live ? (int)(wu - tl * A.chunks) : 0;
        const long long g0 = tl * 64, g = g0 + lane;
        const bool on = live && g < A.G;
        const long long b = on ? g / A.F : 0, f = on ? g - b * A.F : 0;
        const long long t0 = (long long)p * A.chunk;
        const long long t1 = t0 + A.chunk < A.T ? t0 + A.chunk : A.T;
        const float* xg = A.x.p + b * A.x.sb + f * A.x.sf;
        const float* ag = NM >= 1 ? A.ma.p + b * A.ma.sb + f * A.ma.sf : nullptr;
        const float* bg = (NM == 2 && !A.complement) ? A.mb.p + b * A.mb.sb + f * A.mb.sf : nullptr;

        float d[NP][C], re[NP][TRI + 1], im[NP][TRI + 1];
        double ms[NP];
#pragma unroll
        for (int m = 0; m < NP; ++m) {
            ms[m] = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) d[m][c] = 0.0f;
#pragma unroll
            for (int k = 0; k <= TRI; ++k) re[m][k] = 0.0f, im[m][k] = 0.0f;
        }

        for (int s = 0; s < subs; ++s) {
            const long long ts = t0 + (long long)s * BF_TS;
            if (stage_a || stage_b) {
                __syncthreads();                                            // the tile's readers of the last round are through
                if (live && stage_a) bf_stage(tile_a, A.ma, on ? b * A.ma.sb + f * A.ma.sf : -1, ts, t1, lane);
                if (live && stage_b) bf_stage(tile_b, A.mb, on ? b * A.mb.sb + f * A.mb.sf : -1, ts, t1, lane);
                __syncthreads();
            }
            const long long left = t1 - ts;
            const int n = left < BF_TS ? (int)left : BF_TS;
            if (on && n > 0) {
                float2 next[C];                                             // the frame after the one in hand: its loads fly while this one is summed
#pragma unroll
                for (int c = 0; c < C; ++c) next[c] = *reinterpret_cast<const float2*>(xg + c * A.x.sc + ts * A.x.st);
#pragma unroll 1
                for (int k = 0; k < n; ++k) {
                    const long long t = ts + k, ahead = k + 1 < n ? t + 1 : t;    // (the last frame is loaded twice: no branch round a load)
                    float2 x[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) x[c] = next[c];
#pragma unroll
                    for (int c = 0; c < C; ++c) next[c] = *reinterpret_cast<const float2*>(xg + c * A.x.sc + ahead * A.x.st);
                    if constexpr (NM == 0) {
                        psd_frame<C, false>(x, 1.0f, d[0], re[0], im[0]);
                        ms[0] += 1.0;
                    } else {
                        const float wa = stage_a ? tile_a[k * BF_LD + lane] : ag[t * A.ma.st];
                        psd_frame<C, true>(x, wa, d[0], re[0], im[0]);
                        ms[0] += (double)wa;
                        if constexpr (NM == 2) {
                            const float wb = A.complement ? 1.0f - wa : (stage_b ? tile_b[k * BF_LD + lane] : bg[t * A.mb.st]);
                            psd_frame<C, true>(x, wb, d[1], re[1], im[1]);
                            ms[1] += (double)wb;
                        }
                    }
                }
            }
        }
        if (on) {
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                float* out = A.part + (((long long)m * A.chunks + p) * CC) * A.G + g;
#pragma unroll
                for (int c = 0; c < C; ++c) out[(long long)c * A.G] = d[m][c];
#pragma unroll
                for (int k = 0; k < TRI; ++k) {
                    out[(long long)(C + 2 * k) * A.G] = re[m][k];
                    out[(long long)(C + 2 * k + 1) * A.G] = im[m][k];
                }
                A.msum[((long long)m * A.chunks + p) * A.G + g] = ms[m];
            }
        }
    }
}

// the (row, column) of the k-th entry below the diagonal, rows in order: k = c (c - 1) / 2 + e, e < c
__device__ __forceinline__ void bf_tri(int k, int& c, int& e) {
    c = 1;
    while (c * (c + 1) / 2 <= k) ++c;
    e = k - c * (c - 1) / 2;
}

template <int C>
__global__ void __launch_bounds__(BF_THREADS)
psd_combine_kernel(const PsdParts P, int n_psd, float* out_a, float* out_b) {
    constexpr int CC = C * C;
    const long long total = (long long)n_psd * CC * P.G;                       // a lane per (psd, component, system), systems fastest
    for (long long i = (long long)blockIdx.x * BF_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * BF_THREADS) {
        const long long mq = i / P.G, g = i - mq * P.G;
        const int m = (int)(mq / CC), q = (int)(mq - (long long)m * CC);
        float* o = (m ? out_b : out_a) + g * CC * 2;
        const double denom = P.normalize ? psd_denominator(P, m, g) : 1.0;
        const float v = psd_value(P, CC, m, q, g, denom);
        if (q < C) {
            o[(q * C + q) * 2] = v, o[(q * C + q) * 2 + 1] = 0.0f;
        } else {
            int c, e;
            bf_tri((q - C) >> 1, c, e);
            if ((q - C) & 1) o[(c * C + e) * 2 + 1] = v, o[(e * C + c) * 2 + 1] = -v;
            else o[(c * C + e) * 2] = v, o[(e * C + c) * 2] = v;
        }
    }
}

struct WeightArgs {
    const float* psd_s;          // [G][C][C][2], or null: the pieces of launch 1 (psd 0 = speech, 1 = noise)
    const float* psd_n;
    PsdParts parts;
    long long G, F;
    const float* ref;            // u[b * ref_sb + c], or null: ref_channel
    long long ref_sb;
    int ref_channel, loading;
    double diag_eps, eps;
    float* w;                    // [G][C][2]
};

constexpr int BF_WS = 16;        // systems of a weights workgroup: 512 C^2 bytes of LDS, so that small batches still fill the chip

template <int C>
__global__ void __launch_bounds__(BF_THREADS)
mvdr_weights_kernel(const WeightArgs A) {
    extern __shared__ __align__(16) unsigned char bf_lds[];
    double* L = reinterpret_cast<double*>(bf_lds);                  // [C][2 C][2][BF_WS], then the denominators [2][BF_WS]
    constexpr int W = 2 * C, CC = C * C;
    double* den_lds = L + C * W * 2 * BF_WS;
    const int tid = threadIdx.x;
#define BF_M(i, j, r, s) L[((((i) * W) + (j)) * 2 + (r)) * BF_WS + (s)]
    const long long tiles = (A.G + BF_WS - 1) / BF_WS;
    for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const long long g0 = tl * BF_WS;
        // 1. [psd_n | psd_s] in float64, filled by the whole workgroup
        if (A.psd_s) {
            for (int idx = tid; idx < 2 * BF_WS * CC; idx += BF_THREADS) {
                const int m = idx / (BF_WS * CC), rest = idx - m * BF_WS * CC, s = rest / CC, ij = rest - s * CC;
                const int i = ij / C, j = ij - i * C, col = m ? 0 : C;
                if (g0 + s < A.G) {
                    const float2 v = *reinterpret_cast<const float2*>((m ? A.psd_n : A.psd_s) + ((g0 + s) * CC + ij) * 2);
                    BF_M(i, col + j, 0, s) = (double)v.x, BF_M(i, col + j, 1, s) = (double)v.y;
                }
            }
        } else {
            if (tid < 2 * BF_WS) {
                const int m = tid / BF_WS, s = tid - m * BF_WS;
                if (g0 + s < A.G) den_lds[tid] = A.parts.normalize ? psd_denominator(A.parts, m, g0 + s) : 1.0;
            }
            __syncthreads();
            const int s = tid & (BF_WS - 1);
            const long long g = g0 + s;
            if (g < A.G)
                for (int mq = tid / BF_WS; mq < 2 * CC; mq += BF_THREADS / BF_WS) {
                    const int m = mq / CC, q = mq - m * CC, col = m ? 0 : C;       // psd 0 (speech) is the right-hand side
                    const float v = psd_value(A.parts, CC, m, q, g, den_lds[m * BF_WS + s]);
                    if (q < C) {
                        BF_M(q, col + q, 0, s) = (double)v, BF_M(q, col + q, 1, s) = 0.0;
                    } else {
                        int c, e;
                        bf_tri((q - C) >> 1, c, e);
                        if ((q - C) & 1) BF_M(c, col + e, 1, s) = (double)v, BF_M(e, col + c, 1, s) = (double)(-v);
                        else BF_M(c, col + e, 0, s) = (double)v, BF_M(e, col + c, 0, s) = (double)v;
                    }
                }
        }
        __syncthreads();
        const long long g = g0 + tid;
        if (tid < BF_WS && g < A.G) {                                // a lane per system from here on
            const int s = tid;
            // 2. diagonal loading
            if (A.loading) {
                double tr = 0.0;
                for (int i = 0; i < C; ++i) tr += BF_M(i, i, 0, s);
                const double load = A.diag_eps * tr + 1e-8;
                for (int i = 0; i < C; ++i) BF_M(i, i, 0, s) += load;
            }
            // 3. elimination with partial pivoting
#pragma unroll 1
            for (int k = 0; k < C; ++k) {
                int piv = k;
                double best = fabs(BF_M(k, k, 0, s)) + fabs(BF_M(k, k, 1, s));
                for (int i = k + 1; i < C; ++i) {
                    const double v = fabs(BF_M(i, k, 0, s)) + fabs(BF_M(i, k, 1, s));
                    if (v > best) best = v, piv = i;
                }
                if (piv != k)
                    for (int j = k; j < W; ++j) {
                        const double r0 = BF_M(k, j, 0, s), i0 = BF_M(k, j, 1, s);
                        BF_M(k, j, 0, s) = BF_M(piv, j, 0, s), BF_M(k, j, 1, s) = BF_M(piv, j, 1, s);
                        BF_M(piv, j, 0, s) = r0, BF_M(piv, j, 1, s) = i0;
                    }
                const double pr = BF_M(k, k, 0, s), pi = BF_M(k, k, 1, s), den = pr * pr + pi * pi;
                for (int i = k + 1; i < C; ++i) {
                    const double ar = BF_M(i, k, 0, s), ai = BF_M(i, k, 1, s);
                    const double fr = (ar * pr + ai * pi) / den, fi = (ai * pr - ar * pi) / den;
                    for (int j = k + 1; j < W; ++j) {
                        const double r = BF_M(k, j, 0, s), q = BF_M(k, j, 1, s);
                        BF_M(i, j, 0, s) -= fr * r - fi * q;
                        BF_M(i, j, 1, s) -= fr * q + fi * r;
                    }
                }
            }
            // 4. back substitution: column C + c becomes column c of N = psd_n^-1 psd_s
#pragma unroll 1
            for (int c = C; c < W; ++c)
                for (int i = C - 1; i >= 0; --i) {
                    double sr = BF_M(i, c, 0, s), si = BF_M(i, c, 1, s);
                    for (int j = i + 1; j < C; ++j) {
                        const double ar = BF_M(i, j, 0, s), ai = BF_M(i, j, 1, s), xr = BF_M(j, c, 0, s), xi = BF_M(j, c, 1, s);
                        sr -= ar * xr - ai * xi;
                        si -= ar * xi + ai * xr;
                    }
                    const double pr = BF_M(i, i, 0, s), pi = BF_M(i, i, 1, s), den = pr * pr + pi * pi;
                    BF_M(i, c, 0, s) = (sr * pr + si * pi) / den;
                    BF_M(i, c, 1, s) = (si * pr - sr * pi) / den;
                }
            // 5. W = N / (tr N + eps), then column ref_channel or the contraction with u
            double tr = A.eps, ti = 0.0;
            for (int c = 0; c < C; ++c) tr += BF_M(c, C + c, 0, s), ti += BF_M(c, C + c, 1, s);
            const double den = tr * tr + ti * ti;
            const float* u = A.ref ? A.ref + (g / A.F) * A.ref_sb : nullptr;
            float* out = A.w + g * C * 2;
            for (int i = 0; i < C; ++i) {
                double wr = 0.0, wi = 0.0;
                if (u) {
                    for (int c = 0; c < C; ++c) {
                        const double nr = BF_M(i, C + c, 0, s), ni = BF_M(i, C + c, 1, s), uc = (double)u[c];
                        wr += (nr * tr + ni * ti) / den * uc;
                        wi += (ni * tr - nr * ti) / den * uc;
                    }
                } else {
                    const double nr = BF_M(i, C + A.ref_channel, 0, s), ni = BF_M(i, C + A.ref_channel, 1, s);
                    wr = (nr * tr + ni * ti) / den;
                    wi = (ni * tr - nr * ti) / den;
                }
                out[2 * i] = (float)wr, out[2 * i + 1] = (float)wi;
            }
        }
        __syncthreads();                                             // the next tile overwrites the matrices
    }
#undef BF_M
}

struct ApplyArgs {
    const float* w;              // [G][C][2]
    SpecRef x;
    long long F, T, G;
    long long pieces, wave_units, units;        // pieces of BF_AP_FRAMES frames; wave_units = tiles * pieces
    float* y;
    long long ob, of, ot;
};

template <int C>
__global__ void __launch_bounds__(BF_THREADS)
apply_kernel(const ApplyArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long u = blockIdx.x; u < A.units; u += gridDim.x) {
        const long long wu = u * BF_WAVES + wave;
        if (wu >= A.wave_units) continue;                            // (no barrier in this kernel)
        const long long tl = wu / A.pieces, p = wu - tl * A.pieces;
        const long long g = tl * 64 + lane;
        if (g >= A.G) continue;
        const long long b = g / A.F, f = g - b * A.F;
        float wr[C], wi[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float2 v = *reinterpret_cast<const float2*>(A.w + (g * C + c) * 2);
            wr[c] = v.x, wi[c] = v.y;
        }
        const float* xg = A.x.p + b * A.x.sb + f * A.x.sf;
        float* yg = A.y + b * A.ob + f * A.of;
        const long long t0 = p * BF_AP_FRAMES;
        const long long t1 = t0 + BF_AP_FRAMES < A.T ? t0 + BF_AP_FRAMES : A.T;
#pragma unroll 4
        for (long long t = t0; t < t1; ++t) {
            float2 x[C];
#pragma unroll
            for (int c = 0; c < C; ++c) x[c] = *reinterpret_cast<const float2*>(xg + c * A.x.sc + t * A.x.st);
            float yr = 0.0f, yi = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {                            // conj(w) x = (wr xr + wi xi) + i (wr xi - wi xr)
                yr = fmaf(wi[c], x[c].y, fmaf(wr[c], x[c].x, yr));
                yi = fmaf(-wi[c], x[c].x, fmaf(wr[c], x[c].y, yi));
            }
            *reinterpret_cast<float2*>(yg + t * A.ot) = make_float2(yr, yi);
        }
    }
}

// ----------------------------------------------------------------------------- rtf_evd / rtf_power / mvdr_weights_rtf
// rtf_power and mvdr_weights_rtf keep the layout of mvdr_weights_kernel: BF_WS systems a workgroup, an LDS matrix of C rows and W
// complex float64 columns per system, element-major and system-minor, filled by all 256 lanes, then a lane per system.  rtf_evd, two
// orders of magnitude more arithmetic, gives a system a group of lanes instead (below).
#define RT_M(i, j, r, s) L[((((i) * W) + (j)) * 2 + (r)) * BF_WS + (s)]

constexpr int BF_EVD_SWEEPS = 16;      // most Jacobi sweeps; the convergence test only leaves earlier
constexpr int BF_MAX_ITER = 64;        // most n_iter of rtf_power

// columns [col0, col0 + C) of the systems [g0, g0 + BF_WS) from a float32 [G][C][C][2] tensor; called by the whole workgroup
template <int C, int W>
__device__ __forceinline__ void rt_fill(double* L, const float* src, int col0, long long g0, long long G, int tid) {
    constexpr int CC = C * C;
    for (int idx = tid; idx < BF_WS * CC; idx += BF_THREADS) {
        const int s = idx / CC, ij = idx - s * CC, i = ij / C, j = ij - i * C;
        if (g0 + s < G) {
            const float2 v = *reinterpret_cast<const float2*>(src + ((g0 + s) * CC + ij) * 2);
            RT_M(i, col0 + j, 0, s) = (double)v.x, RT_M(i, col0 + j, 1, s) = (double)v.y;
        }
    }
}

// columns [0, C) += (diag_eps Re tr + 1e-8) I; returns what was added
template <int C, int W>
__device__ __forceinline__ double rt_load(double* L, int s, double diag_eps) {
    double tr = 0.0;
    for (int i = 0; i < C; ++i) tr += RT_M(i, i, 0, s);
    const double load = diag_eps * tr + 1e-8;
    for (int i = 0; i < C; ++i) RT_M(i, i, 0, s) += load;
    return load;
}

// columns [C, C + NR) become M^-1 times themselves, M the columns [0, C): elimination with partial pivoting (pivot: largest |re| +
// |im|) and back substitution, the steps of mvdr_weights_kernel; columns from C + NR on are left alone
template <int C, int W, int NR>
__device__ __forceinline__ void rt_solve(double* L, int s) {
    constexpr int EW = C + NR;
#pragma unroll 1
    for (int k = 0; k < C; ++k) {
        int piv = k;
        double best = fabs(RT_M(k, k, 0, s)) + fabs(RT_M(k, k, 1, s));
        for (int i = k + 1; i < C; ++i) {
            const double v = fabs(RT_M(i, k, 0, s)) + fabs(RT_M(i, k, 1, s));
            if (v > best) best = v, piv = i;
        }
        if (piv != k)
            for (int j = k; j < EW; ++j) {
                const double r0 = RT_M(k, j, 0, s), i0 = RT_M(k, j, 1, s);
                RT_M(k, j, 0, s) = RT_M(piv, j, 0, s), RT_M(k, j, 1, s) = RT_M(piv, j, 1, s);
                RT_M(piv, j, 0, s) = r0, RT_M(piv, j, 1, s) = i0;
            }
        const double pr = RT_M(k, k, 0, s), pi = RT_M(k, k, 1, s), den = pr * pr + pi * pi;
        for (int i = k + 1; i < C; ++i) {
            const double ar = RT_M(i, k, 0, s), ai = RT_M(i, k, 1, s);
            const double fr = (ar * pr + ai * pi) / den, fi = (ai * pr - ar * pi) / den;
            for (int j = k + 1; j < EW; ++j) {
                const double r = RT_M(k, j, 0, s), q = RT_M(k, j, 1, s);
                RT_M(i, j, 0, s) -= fr * r - fi * q;
                RT_M(i, j, 1, s) -= fr * q + fi * r;
            }
        }
    }
#pragma unroll 1
    for (int c = C; c < EW; ++c)
        for (int i = C - 1; i >= 0; --i) {
            double sr = RT_M(i, c, 0, s), si = RT_M(i, c, 1, s);
            for (int j = i + 1; j < C; ++j) {
                const double ar = RT_M(i, j, 0, s), ai = RT_M(i, j, 1, s), xr = RT_M(j, c, 0, s), xi = RT_M(j, c, 1, s);
                sr -= ar * xr - ai * xi;
                si -= ar * xi + ai * xr;
            }
            const double pr = RT_M(i, i, 0, s), pi = RT_M(i, i, 1, s), den = pr * pr + pi * pi;
            RT_M(i, c, 0, s) = (sr * pr + si * pi) / den;
            RT_M(i, c, 1, s) = (si * pr - sr * pi) / den;
        }
}

// rtf_evd: Jacobi on the Hermitian matrix (its lower triangle is the data, as LAPACK's 'L') in float64, a GROUP of lanes per system:
// lane i of a group of GL (2, 4 or 8) keeps row i of A and of V in registers, no LDS.  A rotation (p, q) with A[p][q] = b w, |w| = 1,
// is J = D R, D = diag(.., conj(w) at q, ..), R the real rotation that annihilates b; A <- J^H A J, V <- V J.  The N - 1 steps of a
// round-robin schedule over N = C rounded up to even hold N / 2 disjoint rotations each (pairs with the dummy index of an odd C are
// skipped), all applied at once: the lane that owns row p forms the rotation from its own A[p][q] and diagonal and the partner's
// diagonal, every lane gets the parameters of every pair by shuffles and rotates columns p, q of its rows of A and V, then the
// lanes of a pair exchange their rows of A and mix them, and the 2 x 2 block is set in closed form.  The diagonal is kept in `diag`
// (the slot A[i][i] of the row is never read).  Sums over a group are xor butterflies: an addition commutes, so every lane of the
// group holds the same bits and the group leaves the sweeps together.  No spectral gap is needed: an exactly diagonal A (zero,
// identity) leaves at once with V = I.  A NaN fails every comparison, so the sweeps end at once, and the 0 * input sum added to every
// output turns the whole system, and only it, into NaNs.  Every access to a row is a value select on a compile-time index, so the
// rows stay in registers.  (The form with a lane per system and [A | V] in the LDS, cyclic by rows, gave the same bounds and took
// 4.4 x as long at (16, 8, 257, 1000) and 4.0 x at (8, 8, 2049, 2813): DESIGN 3.22.)
constexpr int rr_n(int C) { return (C + 1) & ~1; }
constexpr int rr_lanes(int C) { return C <= 2 ? 2 : (C <= 4 ? 4 : 8); }
constexpr int rr_p(int n, int r, int m) { return m == 0 ? n - 1 : (r + m) % (n - 1); }
constexpr int rr_q(int n, int r, int m) { return m == 0 ? r : (r - m + n - 1) % (n - 1); }

template <int N>
struct EvdRow {
    double ar[N], ai[N], vr[N], vi[N], diag;
};
template <int H>
struct EvdRot {
    double c[H], sn[H], wr[H], wi[H];
};

template <int GL>
__device__ __forceinline__ double group_sum(double x) {
#pragma unroll
    for (int d = 1; d < GL; d <<= 1) x += __shfl_xor(x, d, GL);
    return x;
}

// the largest value over the group and the lowest lane index that holds it
template <int GL>
__device__ __forceinline__ void group_top(double& x, int& at) {
#pragma unroll
    for (int d = 1; d < GL; d <<= 1) {
        const double y = __shfl_xor(x, d, GL);
        const int o = __shfl_xor(at, d, GL);
        if (y > x || (y == x && o < at)) x = y, at = o;
    }
}

template <int C, int N, int P, int Q>
__device__ __forceinline__ void evd_role(const EvdRow<N>& S, int i, int& partner, bool& is_p, double& pr, double& pi) {
    if constexpr (P < C && Q < C) {
        const double qr = S.ar[Q], qi = S.ai[Q];                     // (read by every lane, then selected: no pointer is selected)
        const bool p = i == P;
        partner = p ? Q : (i == Q ? P : partner);
        is_p = is_p || p, pr = p ? qr : pr, pi = p ? qi : pi;
    }
}

template <int C, int N, int GL, int M, int P, int Q>
__device__ __forceinline__ void evd_columns(EvdRow<N>& S, EvdRot<N / 2>& R, int i, double c, double sn, double wr, double wi,
                                            double& my_c, double& my_sn, double& my_wr, double& my_wi) {
    if constexpr (P < C && Q < C) {
        R.c[M] = __shfl(c, P, GL), R.sn[M] = __shfl(sn, P, GL), R.wr[M] = __shfl(wr, P, GL), R.wi[M] = __shfl(wi, P, GL);
        const bool mine = i == P || i == Q;
        my_c = mine ? R.c[M] : my_c, my_sn = mine ? R.sn[M] : my_sn, my_wr = mine ? R.wr[M] : my_wr, my_wi = mine ? R.wi[M] : my_wi;
        const double ar = R.sn[M] * R.wr[M], ai = -R.sn[M] * R.wi[M], br = R.c[M] * R.wr[M], bi = -R.c[M] * R.wi[M];
        {
            const double xr = S.ar[P], xi = S.ai[P], yr = S.ar[Q], yi = S.ai[Q];
            S.ar[P] = R.c[M] * xr - (ar * yr - ai * yi), S.ai[P] = R.c[M] * xi - (ar * yi + ai * yr);
            S.ar[Q] = R.sn[M] * xr + (br * yr - bi * yi), S.ai[Q] = R.sn[M] * xi + (br * yi + bi * yr);
        }
        {
            const double xr = S.vr[P], xi = S.vi[P], yr = S.vr[Q], yi = S.vi[Q];
            S.vr[P] = R.c[M] * xr - (ar * yr - ai * yi), S.vi[P] = R.c[M] * xi - (ar * yi + ai * yr);
            S.vr[Q] = R.sn[M] * xr + (br * yr - bi * yi), S.vi[Q] = R.sn[M] * xi + (br * yi + bi * yr);
        }
    }
}

template <int C, int N, int P, int Q>
__device__ __forceinline__ void evd_clear(EvdRow<N>& S, int i) {
    if constexpr (P < C && Q < C) {
        S.ar[Q] = i == P ? 0.0 : S.ar[Q], S.ai[Q] = i == P ? 0.0 : S.ai[Q];
        S.ar[P] = i == Q ? 0.0 : S.ar[P], S.ai[P] = i == Q ? 0.0 : S.ai[P];
    }
}

template <int C, int N, int GL, int R, int... M>
__device__ __forceinline__ void evd_step(EvdRow<N>& S, int i, std::integer_sequence<int, M...>) {
    int partner = i;
    bool is_p = false;
    double pr = 0.0, pi = 0.0;
    (evd_role<C, N, rr_p(N, R, M), rr_q(N, R, M)>(S, i, partner, is_p, pr, pi), ...);
    const double other = __shfl(S.diag, partner, GL);
    const double b = sqrt(pr * pr + pi * pi);
    const bool rot = is_p && b > 0.0;
    const double theta = (other - S.diag) / (2.0 * b);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c1 = 1.0 / sqrt(t * t + 1.0);
    const double c = rot ? c1 : 1.0, sn = rot ? t * c1 : 0.0, wr = rot ? pr / b : 1.0, wi = rot ? pi / b : 0.0, tb = rot ? t * b : 0.0;
    EvdRot<N / 2> rots;
    double my_c = 1.0, my_sn = 0.0, my_wr = 1.0, my_wi = 0.0;
    (evd_columns<C, N, GL, M, rr_p(N, R, M), rr_q(N, R, M)>(S, rots, i, c, sn, wr, wi, my_c, my_sn, my_wr, my_wi), ...);
    // rows: p' = c p - sn w q, q' = sn p + c w q; a lane without a pair keeps its row (1 * mine + 0 * mine)
    const bool paired = partner != i;
    const double alr = !paired ? 1.0 : (is_p ? my_c : my_c * my_wr), ali = (!paired || is_p) ? 0.0 : my_c * my_wi;
    const double ber = !paired ? 0.0 : (is_p ? -my_sn * my_wr : my_sn), bei = (paired && is_p) ? -my_sn * my_wi : 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double orr = __shfl(S.ar[j], partner, GL), oi = __shfl(S.ai[j], partner, GL);
        const double mr = S.ar[j], mi = S.ai[j];
        S.ar[j] = (alr * mr - ali * mi) + (ber * orr - bei * oi);
        S.ai[j] = (alr * mi + ali * mr) + (ber * oi + bei * orr);
    }
    const double tb_other = __shfl(tb, partner, GL);
    S.diag = is_p ? S.diag - tb : S.diag + (paired ? tb_other : 0.0);
    (evd_clear<C, N, rr_p(N, R, M), rr_q(N, R, M)>(S, i), ...);
}

template <int C, int N, int GL, int... R>
__device__ __forceinline__ void evd_sweep(EvdRow<N>& S, int i, std::integer_sequence<int, R...>) {
    (evd_step<C, N, GL, R>(S, i, std::make_integer_sequence<int, N / 2>{}), ...);
}

template <int C>
__global__ void __launch_bounds__(BF_THREADS)
rtf_evd_kernel(const float* psd, long long G, float* out) {
    constexpr int N = rr_n(C), GL = rr_lanes(C), SPW = BF_THREADS / GL;
    const int i = threadIdx.x % GL, sub = threadIdx.x / GL;
    const long long tiles = (G + SPW - 1) / SPW;
    for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const long long g = tl * SPW + sub;
        if (g >= G) continue;                                       // (a whole group at once)
        EvdRow<N> S;
        double poison = 0.0;
        S.diag = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float2 v = make_float2(0.0f, 0.0f);                     // the lower triangle is the data: A[i][j] = conj(A[j][i]) above it
            if (j < C && i < C) v = *reinterpret_cast<const float2*>(psd + ((g * C + (j <= i ? i : j)) * C + (j <= i ? j : i)) * 2);
            S.diag = j == i ? (double)v.x : S.diag;
            S.ar[j] = j == i ? 0.0 : (double)v.x, S.ai[j] = j == i ? 0.0 : (j < i ? (double)v.y : -(double)v.y);
            S.vr[j] = j == i ? 1.0 : 0.0, S.vi[j] = 0.0;
            poison += 0.0 * (double)v.x + 0.0 * (double)v.y;
        }
        poison = group_sum<GL>(poison);
#pragma unroll 1
        for (int sweep = 0; sweep < BF_EVD_SWEEPS; ++sweep) {
            double off = 0.0;
#pragma unroll
            for (int j = 0; j < C; ++j) off += j == i ? 0.0 : S.ar[j] * S.ar[j] + S.ai[j] * S.ai[j];
            off = group_sum<GL>(off);
            const double dg = group_sum<GL>(S.diag * S.diag);
            if (!(off > 2e-32 * dg)) break;                          // converged, or a NaN (off counts both triangles)
            evd_sweep<C, N, GL>(S, i, std::make_integer_sequence<int, N - 1>{});
        }
        double lam = i < C ? S.diag : -INFINITY;
        int top = i;
        group_top<GL>(lam, top);
        double vr = 0.0, vi = 0.0;
#pragma unroll
        for (int j = 0; j < C; ++j) vr = j == top ? S.vr[j] : vr, vi = j == top ? S.vi[j] : vi;
        double big = i < C ? vr * vr + vi * vi : -1.0;
        const double nrm = group_sum<GL>(i < C ? big : 0.0);
        int lead = i;
        group_top<GL>(big, lead);
        const double hr = __shfl(vr, lead, GL), hi = __shfl(vi, lead, GL);
        const double scale = 1.0 / (sqrt(nrm) * sqrt(big));
        if (i < C) {
            const double re = (vr * hr + vi * hi) * scale, im = i == lead ? 0.0 : (vi * hr - vr * hi) * scale;
            *reinterpret_cast<float2*>(out + (g * C + i) * 2) = make_float2((float)(re + poison), (float)(im + poison));
        }
    }
}

struct RtfPowerArgs {
    const float* psd_s;          // [G][C][C][2]
    const float* psd_n;
    long long G, F;
    const float* ref;            // u[b * ref_sb + c], or null: ref_channel
    long long ref_sb;
    int ref_channel, loading, n_iter;
    double diag_eps;
    float* rtf;                  // [G][C][2]
};

// rtf_power: [psd_n | psd_s | K] with K = psd_s (n_iter >= 2) or the loaded psd_n (n_iter == 1), which the elimination leaves alone
template <int C>
__global__ void __launch_bounds__(BF_THREADS)
rtf_power_kernel(const RtfPowerArgs A) {
    extern __shared__ __align__(16) unsigned char bf_lds[];
    double* L = reinterpret_cast<double*>(bf_lds);                  // [C][3 C][2][BF_WS]
    constexpr int W = 3 * C;
    const int tid = threadIdx.x;
    const long long tiles = (A.G + BF_WS - 1) / BF_WS;
    for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const long long g0 = tl * BF_WS;
        rt_fill<C, W>(L, A.psd_n, 0, g0, A.G, tid);
        rt_fill<C, W>(L, A.psd_s, C, g0, A.G, tid);
        rt_fill<C, W>(L, A.n_iter >= 2 ? A.psd_s : A.psd_n, 2 * C, g0, A.G, tid);
        __syncthreads();
        const long long g = g0 + tid;
        if (tid < BF_WS && g < A.G) {
            const int s = tid;
            if (A.loading) {
                const double load = rt_load<C, W>(L, s, A.diag_eps);
                if (A.n_iter < 2)
                    for (int i = 0; i < C; ++i) RT_M(i, 2 * C + i, 0, s) += load;
            }
            rt_solve<C, W, C>(L, s);                                 // columns [C, 2 C): phi = psd_n^-1 psd_s
            double rr[C], ri[C], nr[C], ni[C];
            const float* u = A.ref ? A.ref + (g / A.F) * A.ref_sb : nullptr;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                if (u) {
                    double ar = 0.0, ai = 0.0;
                    for (int c = 0; c < C; ++c) {
                        const double uc = (double)u[c];
                        ar += RT_M(i, C + c, 0, s) * uc, ai += RT_M(i, C + c, 1, s) * uc;
                    }
                    rr[i] = ar, ri[i] = ai;
                } else {
                    rr[i] = RT_M(i, C + A.ref_channel, 0, s), ri[i] = RT_M(i, C + A.ref_channel, 1, s);
                }
            }
#pragma unroll 1
            for (int it = 0; it <= BF_MAX_ITER; ++it) {              // n_iter - 2 products with phi, then the one with K
                const bool last = it >= A.n_iter - 2;
                const int col = last ? 2 * C : C;
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    double ar = 0.0, ai = 0.0;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const double mr = RT_M(i, col + c, 0, s), mi = RT_M(i, col + c, 1, s);
                        ar += mr * rr[c] - mi * ri[c];
                        ai += mr * ri[c] + mi * rr[c];
                    }
                    nr[i] = ar, ni[i] = ai;
                }
#pragma unroll
                for (int i = 0; i < C; ++i) rr[i] = nr[i], ri[i] = ni[i];
                if (last) break;
            }
            float* o = A.rtf + g * C * 2;
#pragma unroll
            for (int i = 0; i < C; ++i) o[2 * i] = (float)rr[i], o[2 * i + 1] = (float)ri[i];
        }
        __syncthreads();
    }
}

struct RtfWeightArgs {
    const float* rtf;            // [G][C][2]
    const float* psd_n;          // [G][C][C][2]
    long long G, F;
    const float* ref;            // u[b * ref_sb + c], or null: ref_channel (< 0: no scaling)
    long long ref_sb;
    int ref_channel, loading;
    double diag_eps, eps;
    float* w;                    // [G][C][2]
};

// mvdr_weights_rtf: [psd_n | d | d]; the first copy of d becomes a = psd_n^-1 d, w = a / (Re d^H a + eps), times conj(d[ref]) or
// sum_c conj(d_c) u_c
template <int C>
__global__ void __launch_bounds__(BF_THREADS)
mvdr_weights_rtf_kernel(const RtfWeightArgs A) {
    extern __shared__ __align__(16) unsigned char bf_lds[];
    double* L = reinterpret_cast<double*>(bf_lds);                  // [C][C + 2][2][BF_WS]
    constexpr int W = C + 2;
    const int tid = threadIdx.x;
    const long long tiles = (A.G + BF_WS - 1) / BF_WS;
    for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        const long long g0 = tl * BF_WS;
        rt_fill<C, W>(L, A.psd_n, 0, g0, A.G, tid);
        for (int idx = tid; idx < BF_WS * C; idx += BF_THREADS) {
            const int s = idx / C, i = idx - s * C;
            if (g0 + s < A.G) {
                const float2 v = *reinterpret_cast<const float2*>(A.rtf + ((g0 + s) * C + i) * 2);
                RT_M(i, C, 0, s) = (double)v.x, RT_M(i, C, 1, s) = (double)v.y;
                RT_M(i, C + 1, 0, s) = (double)v.x, RT_M(i, C + 1, 1, s) = (double)v.y;
            }
        }
        __syncthreads();
        const long long g = g0 + tid;
        if (tid < BF_WS && g < A.G) {
            const int s = tid;
            if (A.loading) rt_load<C, W>(L, s, A.diag_eps);
            rt_solve<C, W, 1>(L, s);
            double q = A.eps;                                        // Re d^H a + eps
            for (int c = 0; c < C; ++c) q += RT_M(c, C + 1, 0, s) * RT_M(c, C, 0, s) + RT_M(c, C + 1, 1, s) * RT_M(c, C, 1, s);
            double sr = 1.0, si = 0.0;
            bool scaled = true;
            if (A.ref) {
                const float* u = A.ref + (g / A.F) * A.ref_sb;
                double ur = 0.0, ui = 0.0;
                for (int c = 0; c < C; ++c) ur += RT_M(c, C + 1, 0, s) * (double)u[c], ui += RT_M(c, C + 1, 1, s) * (double)u[c];
                sr = ur, si = -ui;
            } else if (A.ref_channel >= 0) {
                sr = RT_M(A.ref_channel, C + 1, 0, s), si = -RT_M(A.ref_channel, C + 1, 1, s);
            } else {
                scaled = false;
            }
            float* o = A.w + g * C * 2;
            for (int i = 0; i < C; ++i) {
                const double wr = RT_M(i, C, 0, s) / q, wi = RT_M(i, C, 1, s) / q;
                o[2 * i] = (float)(scaled ? wr * sr - wi * si : wr), o[2 * i + 1] = (float)(scaled ? wr * si + wi * sr : wi);
            }
        }
        __syncthreads();
    }
}
#undef RT_M

// ----------------------------------------------------------------------------- host side
inline bool bf_stride_ok(long long n, long long& stride, bool pairs) {
    if (n == 1) { stride = 0; return true; }
    return stride > 0 && (!pairs || (stride & 1) == 0);
}

// TAC_OK and the normalised reference, or why not
inline int bf_spec(const float* spec, long long batch, int channels, long long bins, long long frames, long long sb, long long sc,
                   long long sf, long long st, SpecRef* x) {
    if (!spec || batch < 1 || bins < 1 || frames < 1 || channels < 1) return TAC_E_INVALID;
    if (channels < 2 || channels > BF_MAX_C) return TAC_E_UNSUPPORTED;
    if (frames > BF_MAX_FRAMES || batch > BF_MAX_SYSTEMS / bins) return TAC_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(spec) & 7) != 0) return TAC_E_INVALID;
    if (!bf_stride_ok(batch, sb, true) || !bf_stride_ok(channels, sc, true) || !bf_stride_ok(bins, sf, true) ||
        !bf_stride_ok(frames, st, true))
        return TAC_E_INVALID;
    x->p = spec, x->sb = sb, x->sc = sc, x->sf = sf, x->st = st;
    return TAC_OK;
}

inline int bf_mask(const float* mask, long long batch, long long bins, long long frames, long long sb, long long sf, long long st,
                   MaskRef* m) {
    if (!mask) return TAC_E_INVALID;
    if (!bf_stride_ok(batch, sb, false) || !bf_stride_ok(bins, sf, false) || !bf_stride_ok(frames, st, false)) return TAC_E_INVALID;
    m->p = mask, m->sb = sb, m->sf = sf, m->st = st;
    m->staged = (frames > 1 && st == 1) ? 1 : 0;
    return TAC_OK;
}

template <int C>
inline int psd_partial_go(int nm, const PsdArgs& A, long long blocks, size_t lds, hipStream_t stream) {
    if (nm == 0) return launch_kernel(psd_partial_kernel<C, 0>, blocks, BF_THREADS, 0, stream, A);
    if (nm == 1) return launch_kernel(psd_partial_kernel<C, 1>, blocks, BF_THREADS, lds, stream, A);
    return launch_kernel(psd_partial_kernel<C, 2>, blocks, BF_THREADS, lds, stream, A);
}

#define BF_BY_CHANNELS(C, CALL)                          \
    switch (C) {                                         \
        case 2: return CALL(2);                          \
        case 3: return CALL(3);                          \
        case 4: return CALL(4);                          \
        case 5: return CALL(5);                          \
        case 6: return CALL(6);                          \
        case 7: return CALL(7);                          \
        case 8: return CALL(8);                          \
        default: return TAC_E_UNSUPPORTED;               \
    }

// launch 1: nm = 0 (no mask), 1 or 2 PSDs
inline int psd_launch_partial(const SpecRef& x, int channels, long long batch, long long bins, long long frames, const MaskRef* ma,
                              const MaskRef* mb, int nm, int complement, int chunks, float* part, double* msum, hipStream_t stream) {
    if (!part || !msum || chunks != (frames + BF_CHUNK - 1) / BF_CHUNK) return TAC_E_INVALID;   // not the cut tac_psd_plan makes
    const long long len = BF_CHUNK;
    PsdArgs A;
    A.x = x;
    A.ma = ma ? *ma : MaskRef{nullptr, 0, 0, 0, 0};
    A.mb = mb ? *mb : MaskRef{nullptr, 0, 0, 0, 0};
    A.F = bins, A.T = frames, A.G = batch * bins;
    A.chunk = (int)len, A.chunks = chunks, A.complement = complement;
    A.wave_units = ((A.G + 63) / 64) * chunks;
    A.units = (A.wave_units + BF_WAVES - 1) / BF_WAVES;
    A.part = part, A.msum = msum;
    const bool stage_b = nm == 2 && !complement && A.mb.staged;
    const bool stage_a = nm >= 1 && A.ma.staged;
    const size_t lds = (stage_b ? 2 : (stage_a ? 1 : 0)) * (size_t)BF_WAVES * BF_TILE * sizeof(float);
    const long long blocks = persistent_blocks(A.units, 1, bf_grid(0, 0));
#define BF_CALL(C) psd_partial_go<C>(nm, A, blocks, lds, stream)
    BF_BY_CHANNELS(channels, BF_CALL)
#undef BF_CALL
}

inline int psd_launch_combine(int channels, const PsdParts& P, int n_psd, float* out_a, float* out_b, hipStream_t stream) {
    const long long blocks = persistent_blocks((long long)n_psd * channels * channels * P.G, BF_THREADS, bf_grid(1, 0));
#define BF_CALL(C) launch_kernel(psd_combine_kernel<C>, blocks, BF_THREADS, 0, stream, P, n_psd, out_a, out_b)
    BF_BY_CHANNELS(channels, BF_CALL)
#undef BF_CALL
}

inline int weights_launch(int channels, const WeightArgs& A, hipStream_t stream) {
    const long long blocks = persistent_blocks((A.G + BF_WS - 1) / BF_WS, 1, bf_grid(1, 0));
    const size_t lds = ((size_t)channels * 2 * channels * 2 + 2) * BF_WS * sizeof(double);
#define BF_CALL(C) launch_kernel(mvdr_weights_kernel<C>, blocks, BF_THREADS, lds, stream, A)
    BF_BY_CHANNELS(channels, BF_CALL)
#undef BF_CALL
}

inline int weights_check(long long batch, long long bins, int channels, const float* ref_vector, long long& ref_sb, int ref_channel) {
    if (batch < 1 || bins < 1 || channels < 1) return TAC_E_INVALID;
    if (channels < 2 || channels > BF_MAX_C || batch > BF_MAX_SYSTEMS / bins) return TAC_E_UNSUPPORTED;
    if (!ref_vector && (ref_channel < 0 || ref_channel >= channels)) return TAC_E_INVALID;
    if (batch == 1) ref_sb = 0;
    if (ref_vector && ref_sb < 0) return TAC_E_INVALID;
    return TAC_OK;
}

inline int apply_launch(const float* weights, const SpecRef& x, int channels, long long batch, long long bins, long long frames,
                        float* out, long long ob, long long of, long long ot, hipStream_t stream) {
    if (!weights || !out || (reinterpret_cast<uintptr_t>(out) & 7) != 0 || (reinterpret_cast<uintptr_t>(weights) & 7) != 0)
        return TAC_E_INVALID;
    if (!bf_stride_ok(batch, ob, true) || !bf_stride_ok(bins, of, true) || !bf_stride_ok(frames, ot, true)) return TAC_E_INVALID;
    ApplyArgs A;
    A.w = weights, A.x = x;
    A.F = bins, A.T = frames, A.G = batch * bins;
    A.pieces = (frames + BF_AP_FRAMES - 1) / BF_AP_FRAMES;
    A.wave_units = ((A.G + 63) / 64) * A.pieces;
    A.units = (A.wave_units + BF_WAVES - 1) / BF_WAVES;
    A.y = out, A.ob = ob, A.of = of, A.ot = ot;
    const long long blocks = persistent_blocks(A.units, 1, bf_grid(1, 0));
#define BF_CALL(C) launch_kernel(apply_kernel<C>, blocks, BF_THREADS, 0, stream, A)
    BF_BY_CHANNELS(channels, BF_CALL)
#undef BF_CALL
}

inline bool rt_aligned(const void* a, const void* b) {
    return a && b && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7) == 0;
}

// a workgroup per BF_WS systems with `columns` complex float64 columns a row in the LDS
inline long long rt_blocks(long long G) { return persistent_blocks((G + BF_WS - 1) / BF_WS, 1, bf_grid(1, 0)); }
inline size_t rt_lds(int channels, int columns) { return (size_t)channels * columns * 2 * BF_WS * sizeof(double); }

inline int rtf_weights_launch(int channels, const RtfWeightArgs& A, hipStream_t stream) {
#define BF_CALL(C) launch_kernel(mvdr_weights_rtf_kernel<C>, rt_blocks(A.G), BF_THREADS, rt_lds(C, C + 2), stream, A)
    BF_BY_CHANNELS(channels, BF_CALL)
#undef BF_CALL
}

// as weights_check, with ref_channel < 0 (and no vector) for "no reference"
inline int rtf_weights_args(const float* rtf, const float* psd_n, long long batch, long long bins, int channels, const float* ref_vector,
                            long long ref_sb, int ref_channel, int loading, double diag_eps, double eps, float* weights,
                            RtfWeightArgs* A) {
    const int rc = weights_check(batch, bins, channels, ref_vector, ref_sb, ref_channel < 0 ? 0 : ref_channel);
    if (rc != TAC_OK) return rc;
    if (!rt_aligned(rtf, psd_n) || !rt_aligned(weights, weights)) return TAC_E_INVALID;
    A->rtf = rtf, A->psd_n = psd_n, A->G = batch * bins, A->F = bins;
    A->ref = ref_vector, A->ref_sb = ref_sb, A->ref_channel = ref_channel < 0 ? -1 : ref_channel, A->loading = loading ? 1 : 0;
    A->diag_eps = diag_eps, A->eps = eps, A->w = weights;
    return TAC_OK;
}

}  // namespace tac

extern "C" {

int tac_rtf_evd_f32(const float* psd_s, int64_t batch, int64_t bins, int32_t channels, float* rtf, void* stream) {
    using namespace tac;
    long long ref_sb = 0;
    const int rc = weights_check(batch, bins, channels, nullptr, ref_sb, 0);
    if (rc != TAC_OK) return rc;
    if (!rt_aligned(psd_s, rtf)) return TAC_E_INVALID;
    const long long G = batch * bins;
#define BF_CALL(C)                                                                                                        \
    launch_kernel(rtf_evd_kernel<C>, persistent_blocks((G * rr_lanes(C) + BF_THREADS - 1) / BF_THREADS, 1, bf_grid(1, 0)), \
                  BF_THREADS, 0, (hipStream_t)stream, psd_s, G, rtf)
    BF_BY_CHANNELS(channels, BF_CALL)
#undef BF_CALL
}

int32_t tac_rtf_power_max_iter(void) { return tac::BF_MAX_ITER; }

int tac_rtf_power_f32(const float* psd_s, const float* psd_n, int64_t batch, int64_t bins, int32_t channels, const float* ref_vector,
                      int64_t ref_stride_b, int32_t ref_channel, int32_t n_iter, int32_t diagonal_loading, double diag_eps, float* rtf,
                      void* stream) {
    using namespace tac;
    long long ref_sb = ref_stride_b;
    const int rc = weights_check(batch, bins, channels, ref_vector, ref_sb, ref_channel);
    if (rc != TAC_OK) return rc;
    if (n_iter < 1 || !rt_aligned(psd_s, psd_n) || !rt_aligned(rtf, rtf)) return TAC_E_INVALID;
    if (n_iter > BF_MAX_ITER) return TAC_E_UNSUPPORTED;
    RtfPowerArgs A;
    A.psd_s = psd_s, A.psd_n = psd_n, A.G = batch * bins, A.F = bins;
    A.ref = ref_vector, A.ref_sb = ref_sb, A.ref_channel = ref_channel, A.loading = diagonal_loading ? 1 : 0, A.n_iter = n_iter;
    A.diag_eps = diag_eps, A.rtf = rtf;
#define BF_CALL(C) launch_kernel(rtf_power_kernel<C>, rt_blocks(A.G), BF_THREADS, rt_lds(C, 3 * C), (hipStream_t)stream, A)
    BF_BY_CHANNELS(channels, BF_CALL)
#undef BF_CALL
}

int tac_mvdr_weights_rtf_f32(const float* rtf, const float* psd_n, int64_t batch, int64_t bins, int32_t channels,
                             const float* ref_vector, int64_t ref_stride_b, int32_t ref_channel, int32_t diagonal_loading,
                             double diag_eps, double eps, float* weights, void* stream) {
    using namespace tac;
    RtfWeightArgs A;
    const int rc = rtf_weights_args(rtf, psd_n, batch, bins, channels, ref_vector, ref_stride_b, ref_channel, diagonal_loading,
                                    diag_eps, eps, weights, &A);
    if (rc != TAC_OK) return rc;
    return rtf_weights_launch(channels, A, (hipStream_t)stream);
}

int tac_rtf_mvdr_f32(const float* spec, int64_t batch, int32_t channels, int64_t bins, int64_t frames, int64_t stride_b,
                     int64_t stride_c, int64_t stride_f, int64_t stride_t, const float* rtf, const float* psd_n,
                     const float* ref_vector, int64_t ref_stride_b, int32_t ref_channel, int32_t diagonal_loading, double diag_eps,
                     double eps, float* weights, float* out, int64_t out_b, int64_t out_f, int64_t out_t, void* stream) {
    using namespace tac;
    SpecRef x;
    int rc = bf_spec(spec, batch, channels, bins, frames, stride_b, stride_c, stride_f, stride_t, &x);
    if (rc != TAC_OK) return rc;
    RtfWeightArgs A;
    if ((rc = rtf_weights_args(rtf, psd_n, batch, bins, channels, ref_vector, ref_stride_b, ref_channel, diagonal_loading, diag_eps,
                               eps, weights, &A)) != TAC_OK)
        return rc;
    if (!out) return TAC_E_INVALID;
    if ((rc = rtf_weights_launch(channels, A, (hipStream_t)stream)) != TAC_OK) return rc;
    return apply_launch(weights, x, channels, batch, bins, frames, out, out_b, out_f, out_t, (hipStream_t)stream);
}

int tac_psd_plan(int64_t frames, int32_t* chunk_frames, int32_t* chunks) {
    int len = 0, n = 0;
    const int rc = tac::psd_plan(frames, &len, &n);
    if (rc != TAC_OK) return rc;
    if (chunk_frames) *chunk_frames = len;
    if (chunks) *chunks = n;
    return TAC_OK;
}

int32_t tac_beamform_grid(int32_t which, int32_t cus) { return tac::bf_grid(which, cus); }

int tac_psd_f32(const float* spec, int64_t batch, int32_t channels, int64_t bins, int64_t frames, int64_t stride_b, int64_t stride_c,
                int64_t stride_f, int64_t stride_t, const float* mask_a, int64_t a_stride_b, int64_t a_stride_f, int64_t a_stride_t,
                const float* mask_b, int64_t b_stride_b, int64_t b_stride_f, int64_t b_stride_t, int32_t n_psd, int32_t complement,
                int32_t normalize, double eps, int32_t chunks, float* part, double* msum, float* psd_a, float* psd_b, void* stream) {
    using namespace tac;
    SpecRef x;
    int rc = bf_spec(spec, batch, channels, bins, frames, stride_b, stride_c, stride_f, stride_t, &x);
    if (rc != TAC_OK) return rc;
    if (!psd_a || n_psd < 1 || n_psd > 2 || (n_psd == 2 && (!psd_b || !mask_a || (!complement && !mask_b)))) return TAC_E_INVALID;
    MaskRef ma, mb;
    if (mask_a && (rc = bf_mask(mask_a, batch, bins, frames, a_stride_b, a_stride_f, a_stride_t, &ma)) != TAC_OK) return rc;
    const bool second = n_psd == 2 && !complement;
    if (second && (rc = bf_mask(mask_b, batch, bins, frames, b_stride_b, b_stride_f, b_stride_t, &mb)) != TAC_OK) return rc;
    const int nm = mask_a ? n_psd : 0;
    rc = psd_launch_partial(x, channels, batch, bins, frames, mask_a ? &ma : nullptr, second ? &mb : nullptr, nm,
                            n_psd == 2 && complement, chunks, part, msum, (hipStream_t)stream);
    if (rc != TAC_OK) return rc;
    const PsdParts P{part, msum, batch * bins, chunks, (mask_a && normalize) ? 1 : 0, eps};
    return psd_launch_combine(channels, P, n_psd, psd_a, psd_b, (hipStream_t)stream);
}

int tac_mvdr_weights_souden_f32(const float* psd_s, const float* psd_n, int64_t batch, int64_t bins, int32_t channels,
                                const float* ref_vector, int64_t ref_stride_b, int32_t ref_channel, int32_t diagonal_loading,
                                double diag_eps, double eps, float* weights, void* stream) {
    using namespace tac;
    long long ref_sb = ref_stride_b;
    const int rc = weights_check(batch, bins, channels, ref_vector, ref_sb, ref_channel);
    if (rc != TAC_OK) return rc;
    if (!psd_s || !psd_n || !weights || ((reinterpret_cast<uintptr_t>(psd_s) | reinterpret_cast<uintptr_t>(psd_n)) & 7) != 0)
        return TAC_E_INVALID;
    WeightArgs A;
    A.psd_s = psd_s, A.psd_n = psd_n;
    A.parts = PsdParts{nullptr, nullptr, 0, 0, 0, 0.0};
    A.G = batch * bins, A.F = bins;
    A.ref = ref_vector, A.ref_sb = ref_sb, A.ref_channel = ref_channel, A.loading = diagonal_loading ? 1 : 0;
    A.diag_eps = diag_eps, A.eps = eps, A.w = weights;
    return weights_launch(channels, A, (hipStream_t)stream);
}

int tac_apply_beamforming_f32(const float* weights, const float* spec, int64_t batch, int32_t channels, int64_t bins, int64_t frames,
                              int64_t stride_b, int64_t stride_c, int64_t stride_f, int64_t stride_t, float* out, int64_t out_b,
                              int64_t out_f, int64_t out_t, void* stream) {
    using namespace tac;
    SpecRef x;
    const int rc = bf_spec(spec, batch, channels, bins, frames, stride_b, stride_c, stride_f, stride_t, &x);
    if (rc != TAC_OK) return rc;
    return apply_launch(weights, x, channels, batch, bins, frames, out, out_b, out_f, out_t, (hipStream_t)stream);
}

int tac_mvdr_souden_f32(const float* spec, int64_t batch, int32_t channels, int64_t bins, int64_t frames, int64_t stride_b,
                        int64_t stride_c, int64_t stride_f, int64_t stride_t, const float* mask_s, int64_t s_stride_b,
                        int64_t s_stride_f, int64_t s_stride_t, const float* mask_n, int64_t n_stride_b, int64_t n_stride_f,
                        int64_t n_stride_t, double psd_eps, const float* ref_vector, int64_t ref_stride_b, int32_t ref_channel,
                        int32_t diagonal_loading, double diag_eps, double eps, int32_t chunks, float* part, double* msum,
                        float* weights, float* out, int64_t out_b, int64_t out_f, int64_t out_t, void* stream) {
    using namespace tac;
    SpecRef x;
    int rc = bf_spec(spec, batch, channels, bins, frames, stride_b, stride_c, stride_f, stride_t, &x);
    if (rc != TAC_OK) return rc;
    long long ref_sb = ref_stride_b;
    if ((rc = weights_check(batch, bins, channels, ref_vector, ref_sb, ref_channel)) != TAC_OK) return rc;
    if (!weights || !out) return TAC_E_INVALID;
    MaskRef ms, mn;
    if ((rc = bf_mask(mask_s, batch, bins, frames, s_stride_b, s_stride_f, s_stride_t, &ms)) != TAC_OK) return rc;
    if (mask_n && (rc = bf_mask(mask_n, batch, bins, frames, n_stride_b, n_stride_f, n_stride_t, &mn)) != TAC_OK) return rc;
    rc = psd_launch_partial(x, channels, batch, bins, frames, &ms, mask_n ? &mn : nullptr, 2, mask_n ? 0 : 1, chunks, part, msum,
                            (hipStream_t)stream);
    if (rc != TAC_OK) return rc;
    WeightArgs A;
    A.psd_s = nullptr, A.psd_n = nullptr;
    A.parts = PsdParts{part, msum, batch * bins, chunks, 1, psd_eps};
    A.G = batch * bins, A.F = bins;
    A.ref = ref_vector, A.ref_sb = ref_sb, A.ref_channel = ref_channel, A.loading = diagonal_loading ? 1 : 0;
    A.diag_eps = diag_eps, A.eps = eps, A.w = weights;
    if ((rc = weights_launch(channels, A, (hipStream_t)stream)) != TAC_OK) return rc;
    return apply_launch(weights, x, channels, batch, bins, frames, out, out_b, out_f, out_t, (hipStream_t)stream);
}

}  // extern "C"
