// resample.hip — functional.resample: polyphase windowed-sinc resampling and its adjoint, one streaming kernel.
//
//   y[r][j*P + p] = sum_{k < run[p]} B[k][p] * x[r][j*S + off[p] + k]        0 <= j*P + p < L_out,  x zero outside [0, L_in)
//
// Forward: P = new, S = orig (the rates divided by their gcd), B[.][p] the taps of phase p with |t| < lowpass_filter_width and
// off[p] the first such d.  Gradient w.r.t. the waveform: the same kernel with P = orig, S = new and the transposed bank (offsets may
// be negative).  The full new x (2 width + orig) bank of the conv1d formulation is mostly zeros (44100 -> 16000: 160 x 34 of
// 160 x 475); the compact one fits the LDS, which makes this a streaming kernel: the input is read once, the output written once.
//
// Workgroup = 256 threads, a persistent grid over tiles of TO = 1024 / 512 / 256 consecutive outputs of one row.  Per tile
//   global -> xs[span]     the ONE contiguous input span the tile's outputs read (zeros outside the row), starting at a multiple of
//                          four samples so that aligned rows are fetched 16 bytes per lane
//   xs x bs -> out         lane = output sample (coalesced stores); each output is one fused multiply-add chain over k ascending.
//                          bs is tap-major (bs[k * P + p]): consecutive lanes are consecutive phases, i.e. consecutive banks.
// Taps behind a phase's run (the zero padding up to K = max run) are never multiplied, so a NaN or inf in the input reaches exactly
// the outputs whose |t| < lpw taps read it.  No atomics, one writer per element: bit-identical from run to run.
//
// P == 1 (48000 -> 16000, every integer decimation, the gradient of every integer interpolation): the tap is the same for all lanes,
// so it is read through the scalar cache from global memory instead of the LDS, and the x reads of a wave are at stride S floats:
// for even S that is a 2- to 32-way bank conflict on the 32 banks of ds_read_b32, removed by skewing xs by one float per 32
// (SKEW: index i lives at i + i / 32 — stride 2, 4, 8, 12, 16 then touch 32 different banks per 32 lanes).
#include "host_common.hpp"

namespace tac {

typedef float rs_f4 __attribute__((ext_vector_type(4)));

constexpr int RS_THREADS = 256;
constexpr int RESAMPLE_MAX_BANK = 20480;        // floats of bank (P * K): 80 KiB, half the LDS
constexpr int RESAMPLE_MAX_PHASES = 2048;       // off[] and run[] beside it: 16 KiB
constexpr int RS_SPAN_WIDE = 8192;              // floats of input span a 1024- or 512-output tile may take
constexpr int RS_SPAN_MAX = 14336;              // ... and a 256-output tile: 80 + 16 + 58 KiB <= 160 KiB
constexpr int RS_LDS_BYTES = 160 * 1024;

template <bool SKEW>
__device__ __forceinline__ int rs_at(int i) { return SKEW ? i + (i >> 5) : i; }

// Dynamic LDS: bs[K * P] (not with P1) | offs[P] | runs[P] | xs[skewed span]
template <bool P1, bool SKEW, bool VEC>
__global__ void __launch_bounds__(RS_THREADS)
polyphase_kernel(const float* __restrict__ x, long long stride_r, long long l_in, const float* __restrict__ bank,
                 const int* __restrict__ table, int P, int K, int k_min, int S, int off_min, int off_max, int tile_log,
                 long long tiles_per_row, long long units, long long l_out, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int tid = threadIdx.x;
    float* bs = rs_lds;
    int* offs = reinterpret_cast<int*>(rs_lds + (P1 ? 0 : K * P));
    int* runs = offs + P;
    float* xs = reinterpret_cast<float*>(runs + P);

    if constexpr (!P1)
        for (int e = tid; e < K * P; e += RS_THREADS) bs[e] = bank[e];
    for (int p = tid; p < P; p += RS_THREADS) {
        // clamped to what the launcher sized the span for: whatever the table holds, every xs index below stays inside the span
        const int o = table[p], r = table[P + p];
        offs[p] = (o < off_min ? off_min : (o > off_max ? off_max : o)) - off_min;
        runs[p] = r < 0 ? 0 : (r > K ? K : r);
    }
    if (k_min > K) k_min = K;

    const int TO = 1 << tile_log;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long row = u / tiles_per_row;
        const long long n0 = (u - row * tiles_per_row) << tile_log;
        const int nt = (int)(l_out - n0 < TO ? l_out - n0 : TO);
        const long long j_lo = n0 / P;
        const int m0 = (int)(n0 - j_lo * P);                    // phase of the tile's first output
        const int j_span = (m0 + nt - 1) / P;                   // blocks of P outputs the tile reaches into, minus one
        const long long a0 = j_lo * S + off_min;                // first input sample any output of the tile reads
        const long long a0f = a0 & ~3LL;
        const int lead = (int)(a0 - a0f);
        const int span = lead + j_span * S + (off_max - off_min) + K;
        const float* src = x + row * stride_r;
        if constexpr (VEC) {
            for (int q = tid; q < ((span + 3) >> 2); q += RS_THREADS) {
                const long long g = a0f + 4 * q;
                rs_f4 v;
                if (g >= 0 && g + 3 < l_in) {
                    v = *reinterpret_cast<const rs_f4*>(src + g);
                } else {
                    v.x = (g >= 0 && g < l_in) ? src[g] : 0.0f;
                    v.y = (g + 1 >= 0 && g + 1 < l_in) ? src[g + 1] : 0.0f;
                    v.z = (g + 2 >= 0 && g + 2 < l_in) ? src[g + 2] : 0.0f;
                    v.w = (g + 3 >= 0 && g + 3 < l_in) ? src[g + 3] : 0.0f;
                }
                xs[rs_at<SKEW>(4 * q)] = v.x;
                xs[rs_at<SKEW>(4 * q + 1)] = v.y;
                xs[rs_at<SKEW>(4 * q + 2)] = v.z;
                xs[rs_at<SKEW>(4 * q + 3)] = v.w;
            }
        } else {
            for (int i = tid; i < span; i += RS_THREADS) {
                const long long g = a0f + i;
                xs[rs_at<SKEW>(i)] = (g >= 0 && g < l_in) ? src[g] : 0.0f;
            }
        }
        __syncthreads();                                        // the span (and, the first time round, the tables) is in the LDS
        float* dst = out + row * l_out + n0;
        for (int o = tid; o < nt; o += RS_THREADS) {
            const int m = m0 + o;
            const int jl = P1 ? m : m / P;
            const int p = P1 ? 0 : m - jl * P;
            const int xi = lead + jl * S + offs[p];
            const int run = runs[p];
            float acc = 0.0f;
#pragma unroll 4
            for (int k = 0; k < k_min; ++k)
                acc = __builtin_fmaf(P1 ? bank[k] : bs[k * P + p], xs[rs_at<SKEW>(xi + k)], acc);
            for (int k = k_min; k < K; ++k)                     // the one or two taps only the longer phases have
                if (k < run) acc = __builtin_fmaf(P1 ? bank[k] : bs[k * P + p], xs[rs_at<SKEW>(xi + k)], acc);
            dst[o] = acc;
        }
        __syncthreads();                                        // nobody reads xs any more: the next tile may overwrite it
    }
}

// floats of xs a tile of 1 << tile_log outputs needs at most: any first phase, any alignment of the span's start
inline long long rs_span_cap(int P, int K, int S, int off_min, int off_max, int tile_log) {
    const long long j_span = ((long long)P - 1 + (1LL << tile_log) - 1) / P;
    const long long span = 3 + j_span * S + ((long long)off_max - off_min) + K;
    return (span + 3) & ~3LL;
}

template <bool P1, bool SKEW>
inline auto rs_pick(bool vec) {
    return vec ? polyphase_kernel<P1, SKEW, true> : polyphase_kernel<P1, SKEW, false>;
}

}  // namespace tac

extern "C" {

int tac_polyphase_f32(const float* x, int64_t rows, int64_t l_in, int64_t stride_r, const float* bank, const int32_t* table,
                      int32_t phases, int32_t taps, int32_t taps_min, int32_t step, int32_t off_min, int32_t off_max,
                      int64_t l_out, float* out, void* stream) {
    using namespace tac;
    if (!x || !bank || !table || !out) return TAC_E_INVALID;
    if (rows <= 0 || l_in <= 0 || l_out <= 0 || phases <= 0 || taps <= 0 || step <= 0) return TAC_E_INVALID;
    if (taps_min < 0 || taps_min > taps || off_min > off_max) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    if (phases > RESAMPLE_MAX_PHASES || (long long)phases * taps > RESAMPLE_MAX_BANK) return TAC_E_UNSUPPORTED;
    int tile_log = -1;
    long long cap = 0;
    for (int t = 10; t >= 8 && tile_log < 0; --t) {
        cap = rs_span_cap(phases, taps, step, off_min, off_max, t);
        if (cap <= (t == 8 ? RS_SPAN_MAX : RS_SPAN_WIDE)) tile_log = t;
    }
    if (tile_log < 0) return TAC_E_UNSUPPORTED;
    const bool p1 = phases == 1;
    const bool skew = (step & 1) == 0;
    const size_t bytes = 4 * ((size_t)(p1 ? 0 : phases * taps) + 2 * (size_t)phases + (size_t)(cap + (cap >> 5) + 1));
    if (bytes > (size_t)RS_LDS_BYTES) return TAC_E_UNSUPPORTED;
    const long long tiles_per_row = (l_out + (1LL << tile_log) - 1) >> tile_log;
    const long long units = rows * tiles_per_row;
    long long per_cu = (long long)(RS_LDS_BYTES / bytes);
    per_cu = per_cu > 8 ? 8 : per_cu;                           // 8 workgroups of 4 waves fill a CU's 32 wave slots
    const long long blocks = persistent_blocks(units, 1, (long long)device_cu_count() * per_cu);
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_r & 3) == 0;
    auto kern = p1 ? (skew ? rs_pick<true, true>(vec) : rs_pick<true, false>(vec))
                   : (skew ? rs_pick<false, true>(vec) : rs_pick<false, false>(vec));
    return launch_kernel(kern, blocks, RS_THREADS, bytes, (hipStream_t)stream, x, (long long)stride_r, (long long)l_in, bank,
                         (const int*)table, (int)phases, (int)taps, (int)taps_min, (int)step, (int)off_min, (int)off_max,
                         tile_log, tiles_per_row, units, (long long)l_out, out);
}

}  // extern "C"
