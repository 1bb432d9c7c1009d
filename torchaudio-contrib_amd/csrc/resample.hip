// resample.hip — functional.resample: polyphase windowed-sinc resampling and its adjoint, one streaming kernel; below it the same
// sums for banks the LDS cannot hold (tac_polyphase_wide_f32: resample_fit, the last stage of pitch_shift).
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

// ---------------------------------------------------------------------------------------------------------------- wide banks
// tac_polyphase_wide_f32 — the same sums for banks the LDS cannot hold (pitch_shift's 10079 : 8000, 42763 : 48000: up to 4 MB of
// taps, which an XCD's L2 and the Infinity Cache behind it do hold).  What changes against polyphase_kernel:
//   taps, off, run     read from global memory by the lane that uses them: consecutive lanes are consecutive n, i.e. consecutive
//                      addresses of bank[k * P + p] except at a wrap p = P - 1 -> 0.  A lane's taps are fetched ONCE per unit into
//                      registers (compile-time buckets of K) and serve every row of the unit.
//   unit               a tile of TO consecutive outputs times a group of up to RSW_ROWS rows, whose spans are staged together:
//                      one barrier pair a unit.
//   span per tile      starts at the first input the tile's FIRST output reads, j0 * S + off[p0]: the host plan
//                      (_hip.resample_wide_plan) has checked that the starts j * S + off[p] never decrease in n and hands over the
//                      largest span any tile start needs.  off / run are clamped to that span: whatever the table holds, every LDS
//                      index stays inside the row's slot (span + K floats behind a lead of at most 3).
//   out_len            outputs per row that are WRITTEN: n < min(n_out, out_len) are sums, the rest exact zeros.
// The arithmetic is polyphase_kernel's — one __builtin_fmaf chain over k ascending from 0, only k < run[p] — so the bits are too.
// Measured on an MI355X, (256, 160000) at 10079 : 8000 (profiles/pitch_shift): 0.167 ms with four rows a unit against 0.273 ms
// with one, where every row fetches its taps from L2 again (tools/ablation/README.md); K = 34 is the one case one row is level.
constexpr int RSW_ROWS = 4;                     // rows of a unit
constexpr int RSW_MAX_TAPS = 64;                // K
constexpr long long RSW_MAX_BANK = 1LL << 20;   // floats of bank (P * K): 4 MB
constexpr int RSW_SPAN_MAX = 8192;              // floats of input span a tile may take: four rows of it are 128 KiB

template <int KB, bool VEC>
__global__ void __launch_bounds__(RS_THREADS)
polyphase_wide_kernel(const float* __restrict__ x, long long stride_r, long long l_in, long long rows,
                      const float* __restrict__ bank, const int* __restrict__ table, int P, int K, int S, int span, int pitch,
                      int tile_log, long long tiles_per_row, long long units, long long n_out, long long out_len,
                      float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int tid = threadIdx.x;
    const int TO = 1 << tile_log;
    const int span4 = (3 + span + 3) >> 2;                          // 16-byte groups staged per row: lead + span, rounded up
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long grp = u / tiles_per_row;
        const long long n0 = (u - grp * tiles_per_row) << tile_log;
        const long long row0 = grp * RSW_ROWS;
        const int rg = (int)(rows - row0 < RSW_ROWS ? rows - row0 : RSW_ROWS);
        const int nt = (int)(out_len - n0 < TO ? out_len - n0 : TO);        // outputs the tile writes ...
        const long long left = n_out - n0;
        const int nv = left <= 0 ? 0 : (left < nt ? (int)left : nt);        // ... of which the first nv are sums
        const long long j0 = n0 / P;
        const int p0 = (int)(n0 - j0 * P);
        const long long start0 = (long long)table[p0];                      // off of the tile's first output
        const long long a0 = j0 * S + start0;                               // first input sample the tile reads
        const long long a0f = a0 & ~3LL;
        const int lead = (int)(a0 - a0f);
        if (nv > 0) {
            // the rows' spans as ONE index space: every lane has loads in flight whatever the span's length
            if constexpr (VEC) {
                for (int e = tid; e < rg * span4; e += RS_THREADS) {
                    const int r = e / span4, q = e - r * span4;
                    const float* src = x + (row0 + r) * stride_r;
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
                    *reinterpret_cast<rs_f4*>(rs_lds + r * pitch + 4 * q) = v;
                }
            } else {
                for (int e = tid; e < rg * 4 * span4; e += RS_THREADS) {
                    const int r = e / (4 * span4), i = e - r * (4 * span4);
                    const long long g = a0f + i;
                    rs_lds[r * pitch + i] = (g >= 0 && g < l_in) ? x[(row0 + r) * stride_r + g] : 0.0f;
                }
            }
            __syncthreads();                                        // the spans of the unit's rows are in the LDS
        }
        for (int o = tid; o < nt; o += RS_THREADS) {
            float acc[RSW_ROWS];
#pragma unroll
            for (int r = 0; r < RSW_ROWS; ++r) acc[r] = 0.0f;
            if (o < nv) {
                const int m = p0 + o;
                const int jl = m / P;
                const int p = m - jl * P;
                // clamped to what the plan sized the span for: 0 <= xi <= span and run <= K, so xi + k < span + K
                long long xl = (long long)jl * S + (long long)table[p] - start0;
                xl = xl < 0 ? 0 : (xl > span ? span : xl);
                const int xi = lead + (int)xl;
                int run = table[P + p];
                run = run < 0 ? 0 : (run > K ? K : run);
                float w[KB];
#pragma unroll
                for (int k = 0; k < KB; ++k) w[k] = k < run ? bank[(long long)k * P + p] : 0.0f;
#pragma unroll
                for (int r = 0; r < RSW_ROWS; ++r) {
                    if (r < rg) {
                        const float* xs = rs_lds + r * pitch + xi;
                        float a = 0.0f;
#pragma unroll
                        for (int k = 0; k < KB; ++k)
                            if (k < run) a = __builtin_fmaf(w[k], xs[k], a);
                        acc[r] = a;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RSW_ROWS; ++r)
                if (r < rg) out[(row0 + r) * out_len + n0 + o] = acc[r];
        }
        if (nv > 0) __syncthreads();                                // nobody reads the spans any more
    }
}

template <int KB>
inline auto rsw_pick(bool vec) {
    return vec ? polyphase_wide_kernel<KB, true> : polyphase_wide_kernel<KB, false>;
}

static int launch_polyphase_wide(const float* x, long long rows, long long l_in, long long stride_r, const float* bank, const int* table,
                                 int phases, int taps, int step, int span, int tile_log, long long n_out, long long out_len, float* out,
                                 hipStream_t stream) {
    const int pitch = (3 + span + taps + 3) & ~3;
    const size_t bytes = 4 * (size_t)RSW_ROWS * (size_t)pitch;
    if (bytes > (size_t)RS_LDS_BYTES) return TAC_E_UNSUPPORTED;
    const long long tiles_per_row = (out_len + (1LL << tile_log) - 1) >> tile_log;
    const long long groups = (rows + RSW_ROWS - 1) / RSW_ROWS;
    const long long units = groups * tiles_per_row;
    long long per_cu = (long long)(RS_LDS_BYTES / bytes);
    per_cu = per_cu > 8 ? 8 : per_cu;
    const long long blocks = persistent_blocks(units, 1, (long long)device_cu_count() * per_cu);
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_r & 3) == 0;
    auto kern = taps <= 16 ? rsw_pick<16>(vec) : (taps <= 32 ? rsw_pick<32>(vec) : (taps <= 48 ? rsw_pick<48>(vec)
                                                                                                  : rsw_pick<64>(vec)));
    return launch_kernel(kern, blocks, RS_THREADS, bytes, stream, x, stride_r, l_in, rows, bank, table, phases, taps, step, span, pitch,
                         tile_log, tiles_per_row, units, n_out, out_len, out);
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

int tac_polyphase_wide_f32(const float* x, int64_t rows, int64_t l_in, int64_t stride_r, const float* bank, const int32_t* table,
                           int32_t phases, int32_t taps, int32_t step, int32_t span, int32_t tile, int64_t n_out, int64_t out_len,
                           float* out, void* stream) {
    using namespace tac;
    if (!x || !bank || !table || !out) return TAC_E_INVALID;
    if (rows <= 0 || l_in <= 0 || n_out <= 0 || out_len <= 0 || phases <= 0 || taps <= 0 || step <= 0 || span <= 0) return TAC_E_INVALID;
    if (tile != 1024 && tile != 512 && tile != 256) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    if (taps > RSW_MAX_TAPS || (long long)phases * taps > RSW_MAX_BANK || span > RSW_SPAN_MAX) return TAC_E_UNSUPPORTED;
    const int tile_log = tile == 1024 ? 10 : (tile == 512 ? 9 : 8);
    return launch_polyphase_wide(x, rows, l_in, stride_r, bank, (const int*)table, phases, taps, step, span, tile_log, n_out, out_len, out,
                                 (hipStream_t)stream);
}

}  // extern "C"
