// vad.hip — functional.vad / vad_start: the SoX voice-activity detector of torchaudio behind the |X| rows of tac_spectrogram_f32.
//
// Per row, with the |X_t| of frame t at the spectrum bins [s0, s1) (nb of them), S = N = 0 and t = 0, 1, …:
//     m  = t / (1 + t) while t <= boot_max (the boot frames), else `smooth`;        S = S m + |X_t| (1 - m),   d = S^2
//     m2 = 0 in a boot frame, else `up` where d > N and `down` elsewhere;            N = N m2 + d (1 - m2)
//     e  = sqrt(max(0, d - nra N)),   buf[b] = e[b] win[b] at [s0, s1) of M = dft / 2 entries, zeros elsewhere
//     c_q = sum_b buf[b] exp(-2 pi i b q / M),   r = sum_{q in [c0, c1)} |c_q|^2,   meas[t] = r > 0 ? max(0, 21 + log(r / (c1 - c0))) : 0
//
// Launch 2, vad_measure_kernel<BPL>.  A workgroup of 1024 lanes per row, rows on a persistent grid.  Lane l keeps S and N of the bins
// l and l + 1024 (BPL = 1 or 2) in registers.  A tile is VD_TF = 8 consecutive frames:
//   A. the tile's |X| values of the lane's bins are loaded up front (8 BPL independent, coalesced loads at VD_TF = 8; the next tile's are
//      requested before stage B of this one), then the recursion runs 8 frames a bin and leaves e win as two 16-byte LDS stores
//      E[bin][0..8).  Only this stage is serial along time.
//   B. the cepstral bins of the whole tile: task (part p, bin q) of `tasks = parts nq` walks the bins of part p once, reads
//      cos and sin of the angle as ONE 8-byte gather from the table tab[i] = (cos, sin)(2 pi i / M) in the LDS (the index b q mod M
//      advances by q and wraps by a mask), the eight frames of a bin as two 16-byte broadcast reads, and makes 16 FMAs: the
//      angle's two table reads are shared by the tile's frames, which is what a tile buys over one frame at a time.
//      The parts of a bin are then added in ascending order, |c_q|^2 formed, and lane f adds the nq powers of frame f in ascending q.
// Roundings, all float32: m and 1 - m are the float64 values rounded once (so are the four decay factors and their complements,
// by the caller); S = fma(S, m, |X| (1 - m)); d = S S; N = fma(N, m2, d (1 - m2)); d - nra N is one fma; sqrtf; e win one product;
// the table is float64 cosines and sines rounded once; every partial sum is a chain of fmas in ascending bin order; |c|^2 = fma(re, re, im im);
// r / (c1 - c0) is one division and logf the library's.  No atomics, one writer per element, the order of every sum fixed and
// independent of the batch: the same bits every run.  A NaN or Inf sample makes S NaN from its frame on: r is NaN and the measure 0.
//
// Launch 3, vad_decide_kernel.  A wave per group of C consecutive rows (the channels).  The decayed mean of a channel is the
// first-order scan mean_k = trig mean_(k-1) + (1 - trig) meas_k, done 64 frames at a time with shuffles (pairs (a, b) of the affine
// map composed in a fixed order); a ballot finds the channel's first frame at or above the level, and a later channel is only
// scanned up to the frame an earlier one found, so that the lowest channel of the earliest frame wins.  Then lane i runs the backward
// search of at most n steps for channel i >= i*, a shuffle maximum gives `flush`, and lane 0 stores start and triggered.
#include <math.h>

#include "host_common.hpp"

namespace tac {

constexpr int VD_THREADS = 1024;               // 16 waves: a row has a CU to itself, and only waves hide the LDS latency of stage B
#ifndef VD_TILE_FRAMES
#define VD_TILE_FRAMES 8                      // (4 and 16 build too: the A/B of tools/ablation/README.md)
#endif
constexpr int VD_TF = VD_TILE_FRAMES;         // frames per tile, a multiple of 4
static_assert(VD_TF % 4 == 0 && VD_TF >= 4 && VD_TF <= 64, "a tile is whole 16-byte groups of frames, one lane a frame at the end");
constexpr int VD_MAX_BPL = 2;                 // spectrum bins per lane, at most: 2048 bins
constexpr int VD_MAX_NQ = 512;                // cepstrum bins, at most
constexpr int VD_MAX_PARTS = 32;              // parts the bins are cut into for stage B
constexpr int VD_MAX_TASKS = 1024;            // parts times cepstrum bins, at most
constexpr int VD_LDS_BYTES = 144 * 1024;      // what a workgroup may take
constexpr int VD_PER_CU = 2;                  // workgroups per CU the persistent grid is capped at
constexpr int VD_MAX_SEARCH = 1024;           // launch 3: backward steps, at most

struct VadPlan {
    int nb, bpl, nq, parts, chunk, tasks, M;
    int lds_bytes;
};

// TAC_OK and the plan, or TAC_E_UNSUPPORTED where the bins are beyond the lanes' registers or the LDS
inline int vad_plan(int dft, int s0, int s1, int c0, int c1, VadPlan* pl) {
    if (dft < 16 || !is_pow2(dft) || dft > 65536 || s0 < 1 || s1 <= s0 || s1 > dft / 2 || c0 < 0 || c1 <= c0 || c1 > dft / 4) return TAC_E_INVALID;
    const int nb = s1 - s0, nq = c1 - c0;
    const int bpl = (nb + VD_THREADS - 1) / VD_THREADS;
    if (bpl > VD_MAX_BPL || nq > VD_MAX_NQ) return TAC_E_UNSUPPORTED;
    int best = 0;
    double best_use = 0.0;
    for (int p = 1; p <= VD_MAX_PARTS; ++p) {                        // the fewest parts among the best lane uses
        const int tasks = p * nq;
        if (p > 1 && tasks > VD_MAX_TASKS) break;
        const double use = (double)tasks / (double)(((tasks + VD_THREADS - 1) / VD_THREADS) * VD_THREADS);
        if (use > best_use + 1e-9) best = p, best_use = use;
    }
    pl->nb = nb, pl->bpl = bpl, pl->nq = nq, pl->parts = best, pl->chunk = (nb + best - 1) / best, pl->tasks = best * nq, pl->M = dft / 2;
    const long long floats = 2LL * pl->M + (long long)nb * VD_TF + 2LL * pl->tasks * VD_TF + (long long)nq * VD_TF;
    if (4 * floats > VD_LDS_BYTES) return TAC_E_UNSUPPORTED;
    pl->lds_bytes = (int)(4 * floats);
    return TAC_OK;
}

struct VadMeasureArgs {
    const float* mag;          // [rows][T][n_bins]: |X| rows, frame-major
    const float* win;          // [nb]: the cepstral window, scaled
    const float* tab;          // [M][2]: cos and sin of 2 pi i / M
    float* meas;               // [rows][T]
    long long rows, T, n_bins;
    int s0, nb, M, c0, nq, parts, chunk, tasks, boot_max;
    float smooth, osmooth, up, oup, down, odown, nra;
};

template <int BPL>
__global__ void __launch_bounds__(VD_THREADS)
vad_measure_kernel(const VadMeasureArgs A) {
    extern __shared__ __align__(16) unsigned char vd_lds[];
    float2* tab = reinterpret_cast<float2*>(vd_lds);                 // [M]: M is a multiple of 8, what follows stays 16-byte aligned
    float* E = reinterpret_cast<float*>(tab + A.M);                                           // [nb][VD_TF]
    float* part = E + A.nb * VD_TF;                                 // [tasks][2][VD_TF]
    float* pw = part + 2 * A.tasks * VD_TF;                          // [nq][VD_TF]
    const int tid = threadIdx.x;
    const int nb = A.nb, nq = A.nq, mask = A.M - 1;
    const long long T = A.T;
    const float nqf = (float)nq;

    for (int i = tid; i < A.M; i += VD_THREADS) tab[i] = reinterpret_cast<const float2*>(A.tab)[i];
    float w[BPL];
#pragma unroll
    for (int j = 0; j < BPL; ++j) {
        const int b = j * VD_THREADS + tid;
        w[j] = b < nb ? A.win[b] : 0.0f;
    }

    for (long long row = blockIdx.x; row < A.rows; row += gridDim.x) {
        const float* mrow = A.mag + row * T * A.n_bins + A.s0;
        float S[BPL], N[BPL], xv[BPL][VD_TF];
#pragma unroll
        for (int j = 0; j < BPL; ++j) S[j] = 0.0f, N[j] = 0.0f;
        // the first tile's |X|
#pragma unroll
        for (int j = 0; j < BPL; ++j) {
            const int b = j * VD_THREADS + tid;
#pragma unroll
            for (int f = 0; f < VD_TF; ++f) xv[j][f] = (b < nb && f < T) ? mrow[(long long)f * A.n_bins + b] : 0.0f;
        }
        for (long long t0 = 0; t0 < T; t0 += VD_TF) {
            const int nf = T - t0 < VD_TF ? (int)(T - t0) : VD_TF;
            // A. the recursion of the lane's bins over the tile's frames
#pragma unroll
            for (int j = 0; j < BPL; ++j) {
                const int b = j * VD_THREADS + tid;
                float ev[VD_TF];
#pragma unroll
                for (int f = 0; f < VD_TF; ++f) {
                    const long long t = t0 + f;
                    const bool boot = A.boot_max < 0 || t <= A.boot_max;
                    float m = A.smooth, om = A.osmooth;
                    if (boot) {
                        const double md = (double)t / (double)(t + 1);
                        m = (float)md, om = (float)(1.0 - md);
                    }
                    float e = 0.0f;
                    if (f < nf && b < nb) {
                        S[j] = fmaf(S[j], m, xv[j][f] * om);
                        const float d = S[j] * S[j];
                        const bool rise = d > N[j];
                        const float m2 = boot ? 0.0f : (rise ? A.up : A.down), om2 = boot ? 1.0f : (rise ? A.oup : A.odown);
                        N[j] = fmaf(N[j], m2, d * om2);
                        const float v = fmaf(-A.nra, N[j], d);
                        e = (v < 0.0f ? 0.0f : sqrtf(v)) * w[j];                 // (a NaN stays one)
                    }
                    ev[f] = e;
                }
                if (b < nb) {
                    float4* dst = reinterpret_cast<float4*>(E + (size_t)b * VD_TF);
#pragma unroll
                    for (int v = 0; v < VD_TF / 4; ++v) dst[v] = make_float4(ev[4 * v], ev[4 * v + 1], ev[4 * v + 2], ev[4 * v + 3]);
                }
            }
            __syncthreads();
            // the next tile's |X|: nothing below waits for it
            if (t0 + VD_TF < T) {
#pragma unroll
                for (int j = 0; j < BPL; ++j) {
                    const int b = j * VD_THREADS + tid;
#pragma unroll
                    for (int f = 0; f < VD_TF; ++f) {
                        const long long t = t0 + VD_TF + f;
                        xv[j][f] = (b < nb && t < T) ? mrow[t * A.n_bins + b] : 0.0f;
                    }
                }
            }
            // B. task (part p, cepstral bin q): the partial sums over the part's bins, eight frames at a time
            for (int task = tid; task < A.tasks; task += VD_THREADS) {
                const int p = task / nq, qi = task - p * nq, q = A.c0 + qi;
                const int b0 = p * A.chunk, b1 = b0 + A.chunk < nb ? b0 + A.chunk : nb;
                int idx = (int)(((long long)(A.s0 + b0) * q) & mask);
                float re[VD_TF], im[VD_TF];
#pragma unroll
                for (int f = 0; f < VD_TF; ++f) re[f] = 0.0f, im[f] = 0.0f;
#pragma unroll 4
                for (int b = b0; b < b1; ++b) {
                    const float2 cs = tab[idx];
                    const float c = cs.x, s = cs.y;
#pragma unroll
                    for (int v = 0; v < VD_TF / 4; ++v) {
                        const float4 e4 = *reinterpret_cast<const float4*>(E + (size_t)b * VD_TF + 4 * v);
                        const float ef[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                        for (int f = 0; f < 4; ++f) re[4 * v + f] = fmaf(ef[f], c, re[4 * v + f]), im[4 * v + f] = fmaf(ef[f], s, im[4 * v + f]);
                    }
                    idx = (idx + q) & mask;
                }
                float4* dst = reinterpret_cast<float4*>(part + (size_t)task * 2 * VD_TF);
#pragma unroll
                for (int v = 0; v < VD_TF / 4; ++v) {
                    dst[v] = make_float4(re[4 * v], re[4 * v + 1], re[4 * v + 2], re[4 * v + 3]);
                    dst[VD_TF / 4 + v] = make_float4(im[4 * v], im[4 * v + 1], im[4 * v + 2], im[4 * v + 3]);
                }
            }
            __syncthreads();
            // the parts of (q, frame) in ascending order, and the power
            for (int it = tid; it < nq * VD_TF; it += VD_THREADS) {
                const int qi = it / VD_TF, f = it - qi * VD_TF;
                float re = 0.0f, im = 0.0f;
                for (int p = 0; p < A.parts; ++p) {
                    const float* src = part + (size_t)(p * nq + qi) * 2 * VD_TF;
                    re += src[f], im += src[VD_TF + f];
                }
                pw[it] = fmaf(re, re, im * im);
            }
            __syncthreads();
            if (tid < nf) {
                float r = 0.0f;
                for (int qi = 0; qi < nq; ++qi) r += pw[qi * VD_TF + tid];
                A.meas[row * T + t0 + tid] = r > 0.0f ? fmaxf(0.0f, 21.0f + logf(r / nqf)) : 0.0f;
            }
            // (E is next written behind the two barriers above, `part` and `pw` behind the next tile's first)
        }
        __syncthreads();
    }
}

struct VadDecideArgs {
    const float* meas;         // [groups][C][T]
    long long groups, C, T, time, period, pre, keep;
    int n, gap;
    float level, trig, otrig;
    long long* start;          // [groups]
    unsigned char* triggered;  // [groups]
};

__global__ void __launch_bounds__(64)
vad_decide_kernel(const VadDecideArgs A) {
    const int lane = threadIdx.x;
    const long long T = A.T;
    for (long long g = blockIdx.x; g < A.groups; g += gridDim.x) {
        const float* mg = A.meas + g * A.C * T;
        long long best = T, istar = 0;
        for (long long c = 0; c < A.C && best > 0; ++c) {
            const float* mr = mg + c * T;
            const long long limit = best;                              // a later channel wins only with an earlier frame
            float carry = 0.0f;
            for (long long k0 = 0; k0 < limit; k0 += 64) {
                const long long k = k0 + lane;
                float a = A.trig, b = k < limit ? mr[k] * A.otrig : 0.0f;
#pragma unroll
                for (int d = 1; d < 64; d *= 2) {
                    const float ao = __shfl_up(a, d, 64), bo = __shfl_up(b, d, 64);
                    if (lane >= d) b = fmaf(bo, a, b), a = ao * a;
                }
                const float mean = fmaf(carry, a, b);
                const unsigned long long hits = __ballot(k < limit && mean >= A.level);
                if (hits) {
                    best = k0 + (__ffsll((long long)hits) - 1);
                    istar = c;
                    break;
                }
                carry = __shfl(mean, 63, 64);
            }
        }
        const bool trg = best < T;
        long long start = A.time - A.keep;
        if (trg) {
            int flush = 0;
            for (long long i0 = istar; i0 < A.C; i0 += 64) {
                const long long i = i0 + lane;
                int f = 0;
                if (i < A.C) {
                    int jT = A.n, jZ = A.n;
                    for (int j = 0; j < A.n; ++j) {
                        const long long kk = best - j;
                        const float v = kk >= 0 ? mg[i * T + kk] : 0.0f;
                        if (v >= A.level && j <= jT + A.gap) jZ = jT = j;
                        else if (v == 0.0f && jT >= jZ) jZ = j;
                    }
                    f = jZ < A.n - 1 ? jZ : A.n - 1;
                }
#pragma unroll
                for (int d = 32; d >= 1; d /= 2) {
                    const int o = __shfl_xor(f, d, 64);
                    f = o > f ? o : f;
                }
                flush = f > flush ? f : flush;
            }
            start = (best - flush) * A.period - A.pre;
        }
        if (lane == 0) {
            A.start[g] = start < 0 ? 0 : start;
            A.triggered[g] = trg ? 1 : 0;
        }
    }
}

template <int BPL>
inline int vad_launch_measure_as(const VadMeasureArgs& A, long long blocks, int lds_bytes, hipStream_t stream) {
    return launch_kernel(vad_measure_kernel<BPL>, blocks, VD_THREADS, (size_t)lds_bytes, stream, A);
}

inline int vad_launch_measures(const float* mag, int64_t rows, int64_t n_frames, int32_t dft, int32_t s0, int32_t s1, int32_t c0, int32_t c1,
                               int32_t boot_max, const float* decay, float nra, const float* win, const float* tab, float* meas,
                               hipStream_t stream) {
    if (!mag || !decay || !win || !tab || !meas || rows <= 0 || n_frames <= 0) return TAC_E_INVALID;
    VadPlan pl;
    const int rc = vad_plan(dft, s0, s1, c0, c1, &pl);
    if (rc != TAC_OK) return rc;
    VadMeasureArgs A;
    A.mag = mag, A.win = win, A.tab = tab, A.meas = meas;
    A.rows = rows, A.T = n_frames, A.n_bins = dft / 2 + 1;
    A.s0 = s0, A.nb = pl.nb, A.M = pl.M, A.c0 = c0, A.nq = pl.nq, A.parts = pl.parts, A.chunk = pl.chunk, A.tasks = pl.tasks;
    A.boot_max = boot_max;
    A.smooth = decay[0], A.osmooth = decay[1], A.up = decay[2], A.oup = decay[3], A.down = decay[4], A.odown = decay[5];
    A.nra = nra;
    const long long blocks = persistent_blocks(rows, 1, (long long)device_cu_count() * VD_PER_CU);
    switch (pl.bpl) {
        case 1: return vad_launch_measure_as<1>(A, blocks, pl.lds_bytes, stream);
        default: return vad_launch_measure_as<2>(A, blocks, pl.lds_bytes, stream);
    }
}

inline int vad_launch_decide(const float* meas, int64_t groups, int64_t channels, int64_t n_frames, int64_t time, int32_t n_search,
                             int32_t gap, int64_t period, int64_t pre, int64_t keep, float level, float trig, float otrig,
                             int64_t* start, unsigned char* triggered, hipStream_t stream) {
    if (!start || !triggered || groups <= 0 || channels <= 0 || n_frames < 0 || (n_frames > 0 && !meas) || n_search < 1 || gap < 0 ||
        period < 1 || pre < 0 || time < 0)
        return TAC_E_INVALID;
    if (n_search > VD_MAX_SEARCH) return TAC_E_UNSUPPORTED;
    VadDecideArgs A;
    A.meas = meas, A.groups = groups, A.C = channels, A.T = n_frames, A.time = time, A.period = period, A.pre = pre, A.keep = keep;
    A.n = n_search, A.gap = gap < n_search ? gap : n_search;               // (j <= jT + gap holds for every j < n from there on)
    A.level = level, A.trig = trig, A.otrig = otrig;
    A.start = reinterpret_cast<long long*>(start), A.triggered = triggered;
    const long long blocks = persistent_blocks(groups, 1, (long long)device_cu_count() * 8);
    return launch_kernel(vad_decide_kernel, blocks, 64, 0, stream, A);
}

}  // namespace tac

extern "C" {

int tac_vad_plan(int32_t dft, int32_t s0, int32_t s1, int32_t c0, int32_t c1, int32_t* bins_per_lane, int32_t* parts, int32_t* lds_bytes,
                 int32_t* max_search, int32_t* blocks_per_cu) {
    tac::VadPlan pl;
    if (max_search) *max_search = tac::VD_MAX_SEARCH;
    if (blocks_per_cu) *blocks_per_cu = tac::VD_PER_CU;
    const int rc = tac::vad_plan(dft, s0, s1, c0, c1, &pl);
    if (rc != TAC_OK) return rc;
    if (bins_per_lane) *bins_per_lane = pl.bpl;
    if (parts) *parts = pl.parts;
    if (lds_bytes) *lds_bytes = pl.lds_bytes;
    return TAC_OK;
}

int tac_vad_measures_f32(const float* mag, int64_t rows, int64_t n_frames, int32_t dft, int32_t s0, int32_t s1, int32_t c0, int32_t c1,
                         int32_t boot_max, const float* decay, float nra, const float* win, const float* tab, float* meas, void* stream) {
    return tac::vad_launch_measures(mag, rows, n_frames, dft, s0, s1, c0, c1, boot_max, decay, nra, win, tab, meas, (hipStream_t)stream);
}

int tac_vad_decide_f32(const float* meas, int64_t groups, int64_t channels, int64_t n_frames, int64_t time, int32_t n_search, int32_t gap,
                       int64_t period, int64_t pre, int64_t keep, float level, float trig, float otrig, int64_t* start, void* triggered,
                       void* stream) {
    return tac::vad_launch_decide(meas, groups, channels, n_frames, time, n_search, gap, period, pre, keep, level, trig, otrig, start,
                                  (unsigned char*)triggered, (hipStream_t)stream);
}

int tac_vad_start_f32(const float* mag, int64_t groups, int64_t channels, int64_t n_frames, int64_t time, int32_t dft, int32_t s0, int32_t s1,
                      int32_t c0, int32_t c1, int32_t boot_max, const float* decay, float nra, const float* win, const float* tab,
                      int32_t n_search, int32_t gap, int64_t period, int64_t pre, int64_t keep, float level, float trig, float otrig,
                      float* meas, int64_t* start, void* triggered, void* stream) {
    using namespace tac;
    if (groups <= 0 || channels <= 0 || n_frames <= 0 || n_search < 1) return TAC_E_INVALID;
    if (n_search > VD_MAX_SEARCH) return TAC_E_UNSUPPORTED;
    const int rc = vad_launch_measures(mag, groups * channels, n_frames, dft, s0, s1, c0, c1, boot_max, decay, nra, win, tab, meas,
                                       (hipStream_t)stream);
    if (rc != TAC_OK) return rc;
    return vad_launch_decide(meas, groups, channels, n_frames, time, n_search, gap, period, pre, keep, level, trig, otrig, start,
                             (unsigned char*)triggered, (hipStream_t)stream);
}

}  // extern "C"
