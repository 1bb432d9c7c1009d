// specaug.hip — SpecAugment's masks (functional.mask_along_axis / mask_along_axis_iid, TimeMasking, FrequencyMasking, SpecAugment):
// EVERY mask of a call in ONE streaming launch, "copy, except inside a few index intervals".
//
//   out[r][a][b] = fill                              if an A-span of row r holds a or a B-span of row r holds b
//                = x[r*sr + a*sa + b*sb]             otherwise
//
// spans: DEVICE int32[span_rows][k_a + k_b][2], the first k_a along A, the rest along B, each [start, end); span_rows is rows or 1
// (one table shared by every row).  An index is tested as start <= i < end for 0 <= i < n only, so a span reaching outside the axis
// is clamped to it and one with end <= start is empty, whatever the table holds.  fill is *value_ptr where the pointer is given (a
// mean computed on the device never visits the host), else the immediate.  The masked value is SELECTED, never multiplied in, and a
// masked element is not loaded: a NaN (or the poison pattern) under a mask cannot reach the output.
//
// A persistent grid walks units (row, A-block, B-chunk).  Per unit the workgroup first turns the row's spans into bit masks — one
// bit per line of the A-block (64 at most) and one per column of the B-chunk (256 at most): thread t tests column b0 + t, a wave
// ballot packs 64 answers into a word of the LDS; the span table is read with wave-uniform addresses (scalar loads), once per unit
// and not once per element.  The masks are double-buffered by the parity of the unit count, so a unit costs one barrier.
//
// mask_rows_kernel (lanes along B, the output's unit stride; every layout but the transposed one): a line segment is LPL = 64 / 32 /
// 16 lanes wide (the widest that pads B by an eighth at most, else the one that pads it the least: 80 columns = 20 16-byte
// chunks take 32 lanes), a workgroup covers 256 / LPL lines per pass and four passes per unit: 16 KB of output.  Four loads of
// a thread are issued before its first store.
//   VEC   x has unit stride along B, B % 4 == 0 and base and strides keep every chunk 16-byte aligned: a lane owns four consecutive
//         columns, one 16-byte load and one 16-byte store.  A line inside an A-span and a chunk wholly inside B-spans are stored
//         without a load; a straddling chunk selects per element.
//   else  a lane owns the columns seg + j LPL, j < 4 (dword accesses, consecutive lanes on consecutive columns): any positive
//         strides, any alignment, any B.
// mask_turn_kernel (x has its unit stride along A: the transposed view of a (T, F) Kaldi matrix): a 64 x 64 tile is loaded with lanes
// along A into LDS rows of odd pitch (65 words: the column writes of the load and the row reads of the store are both free of bank
// conflicts) and stored with lanes along B.  Masked elements of the tile are neither loaded nor read back from the LDS.
// One writer per element, no atomics, no workspace: bit-identical from run to run.
#include "host_common.hpp"

namespace tac {

constexpr int MS_THREADS = 256;
constexpr int MS_PASSES = 4;
constexpr int MS_TURN = 64;                      // tile edge of the turned load
constexpr int MS_TURN_PITCH = MS_TURN + 1;

struct MaskGeom {
    long long rows, A, B, sr, sa, sb;
    long long span_stride;                       // ints between the tables of two rows: 2 (k_a + k_b), or 0 for a shared table
    int k_a, k_b;
    unsigned n_ab, n_bc, units;                  // (a unit is 16 KB of output: 2^31 of them are beyond any memory)
};

// true where one of spans [first, last) of table sp holds index i
__device__ __forceinline__ bool ms_held(const int* __restrict__ sp, int first, int last, long long i) {
    bool m = false;
#pragma unroll 1
    for (int s = first; s < last; ++s) m |= (i >= (long long)sp[2 * s]) & (i < (long long)sp[2 * s + 1]);
    return m;
}

// The bit masks of one unit: word 4 the lines a0 .. a0 + 63, words 0 .. 3 the columns b0 .. b0 + 255.  Indices beyond the axis
// get whatever the comparison gives: no thread uses those bits.
__device__ __forceinline__ void ms_unit_masks(const MaskGeom& g, const int* __restrict__ sp, long long a0, long long b0,
                                              unsigned long long* __restrict__ m) {
    const int tid = threadIdx.x;
    const unsigned long long cols = __ballot(ms_held(sp, g.k_a, g.k_a + g.k_b, b0 + tid));
    if ((tid & 63) == 0) m[tid >> 6] = cols;
    if (tid < 64) {
        const unsigned long long lines = __ballot(ms_held(sp, 0, g.k_a, a0 + tid));
        if (tid == 0) m[4] = lines;
    }
}

template <bool VEC, int LPL_LOG>
__global__ void __launch_bounds__(MS_THREADS)
mask_rows_kernel(const float* __restrict__ x, MaskGeom g, const int* __restrict__ spans, const float* __restrict__ value_ptr,
                 float value, float* __restrict__ out) {
    __shared__ unsigned long long masks[2][5];
    const float fill = value_ptr ? *value_ptr : value;
    const int tid = threadIdx.x;
    constexpr int lpl = 1 << LPL_LOG, lp = MS_THREADS >> LPL_LOG;
    constexpr long long width = 4LL * lpl, ab_lines = (long long)lp * MS_PASSES;
    const int seg = tid & (lpl - 1), line0 = tid >> LPL_LOG;
    int par = 0;
    for (unsigned u = blockIdx.x; u < g.units; u += gridDim.x, par ^= 1) {
        const unsigned bc = u % g.n_bc, t = u / g.n_bc;
        const long long ab = t % g.n_ab, row = t / g.n_ab;
        const long long a0 = ab * ab_lines, b0 = (long long)bc * width;
        ms_unit_masks(g, spans + row * g.span_stride, a0, b0, masks[par]);
        __syncthreads();
        const unsigned long long am = masks[par][4];
        const float* src = x + row * g.sr;
        float* dst = out + row * g.A * g.B;
        if constexpr (VEC) {
            const int col = seg * 4;
            const unsigned cb = (unsigned)(masks[par][col >> 6] >> (col & 63)) & 0xFu;
            const long long b = b0 + col;
            float4 v[MS_PASSES];
#pragma unroll
            for (int p = 0; p < MS_PASSES; ++p) {
                const int li = line0 + p * lp;
                const long long a = a0 + li;
                v[p] = make_float4(fill, fill, fill, fill);
                if (a < g.A && b < g.B && !((am >> li) & 1) && cb != 0xFu)
                    v[p] = *reinterpret_cast<const float4*>(src + a * g.sa + b);
            }
#pragma unroll
            for (int p = 0; p < MS_PASSES; ++p) {
                const int li = line0 + p * lp;
                const long long a = a0 + li;
                if (a < g.A && b < g.B) {
                    float4 r = v[p];
                    r.x = (cb & 1u) ? fill : r.x;
                    r.y = (cb & 2u) ? fill : r.y;
                    r.z = (cb & 4u) ? fill : r.z;
                    r.w = (cb & 8u) ? fill : r.w;
                    *reinterpret_cast<float4*>(dst + a * g.B + b) = r;
                }
            }
        } else {
            unsigned cb = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = seg + j * lpl;
                cb |= ((unsigned)(masks[par][col >> 6] >> (col & 63)) & 1u) << j;
            }
            // a column at a time: the loads of its four lines are in flight before the first store
            const float* sp = src + (a0 + line0) * g.sa + (b0 + seg) * g.sb;
            float* dp = dst + (a0 + line0) * g.B + b0 + seg;
            const long long la = g.A - a0 - line0, lb = g.B - b0 - seg;
            const int lines_left = (int)(la < 4096 ? la : 4096), cols_left = (int)(lb < 4096 ? lb : 4096);
            const unsigned long long lm = am >> line0;             // bit p * lp: the line of pass p
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const bool col_in = j * lpl < cols_left, col_on = col_in && !((cb >> j) & 1u);
                float v[MS_PASSES];
#pragma unroll
                for (int p = 0; p < MS_PASSES; ++p) {
                    v[p] = fill;
                    if (col_on && p * lp < lines_left && !((lm >> (p * lp)) & 1u)) v[p] = sp[p * lp * g.sa];
                }
#pragma unroll
                for (int p = 0; p < MS_PASSES; ++p)
                    if (col_in && p * lp < lines_left) dp[p * lp * g.B] = v[p];
                sp += lpl * g.sb;
                dp += lpl;
            }
        }
    }
}

__global__ void __launch_bounds__(MS_THREADS)
mask_turn_kernel(const float* __restrict__ x, MaskGeom g, const int* __restrict__ spans, const float* __restrict__ value_ptr,
                 float value, float* __restrict__ out) {
    __shared__ unsigned long long masks[2][5];
    __shared__ float tile[MS_TURN * MS_TURN_PITCH];
    const float fill = value_ptr ? *value_ptr : value;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int par = 0;
    for (unsigned u = blockIdx.x; u < g.units; u += gridDim.x, par ^= 1) {
        const unsigned bc = u % g.n_bc, t = u / g.n_bc;
        const long long ab = t % g.n_ab, row = t / g.n_ab;
        const long long a0 = ab * MS_TURN, b0 = (long long)bc * MS_TURN;
        ms_unit_masks(g, spans + row * g.span_stride, a0, b0, masks[par]);
        __syncthreads();                 // the masks are there, and every thread has left the tile of the unit before
        const unsigned long long am = masks[par][4], bm = masks[par][0];
        const float* src = x + row * g.sr;
        float* dst = out + row * g.A * g.B;
        // lanes along A, a wave per column of the tile
        const bool a_on = a0 + lane < g.A && !((am >> lane) & 1);
        const float* sp = src + (a0 + lane) * g.sa + (b0 + wave) * g.sb;
        const long long lb = g.B - b0;
        const int cols_left = (int)(lb < MS_TURN ? lb : MS_TURN);
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {            // eight loads of a thread in flight
            float v[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int bb = (h * 8 + p) * 4 + wave;
                v[p] = 0.0f;
                if (a_on && bb < cols_left && !((bm >> bb) & 1)) v[p] = sp[(h * 8 + p) * 4 * g.sb];
            }
#pragma unroll
            for (int p = 0; p < 8; ++p) tile[((h * 8 + p) * 4 + wave) * MS_TURN_PITCH + lane] = v[p];
        }
        __syncthreads();
        // lanes along B, a wave per line
        const bool b_in = b0 + lane < g.B, b_on = !((bm >> lane) & 1);
#pragma unroll
        for (int p = 0; p < MS_TURN / 4; ++p) {
            const int aa = p * 4 + wave;
            if (b_in && a0 + aa < g.A) {
                float r = fill;
                if (b_on && !((am >> aa) & 1)) r = tile[lane * MS_TURN_PITCH + aa];
                dst[(a0 + aa) * g.B + b0 + lane] = r;
            }
        }
    }
}

// lanes per line segment: the widest of 64 / 32 / 16 that pads the 16-byte chunks of a line by an eighth at most, else the one that
// pads them the least (the widest among equals)
inline int ms_lpl_log(long long B) {
    const long long q = (B + 3) / 4;
    int best = 6;
    long long waste = -1;
    for (int l = 6; l >= 4; --l) {
        const long long w = ((q + (1LL << l) - 1) >> l << l) - q;
        if (8 * w <= q) return l;
        if (waste < 0 || w < waste) {
            waste = w;
            best = l;
        }
    }
    return best;
}

}  // namespace tac

extern "C" {

int tac_mask_spans_supported(int32_t k_a, int32_t k_b) {
    if (k_a < 0 || k_b < 0) return TAC_E_INVALID;
    if ((long long)k_a + (long long)k_b > TAC_MASK_MAX_SPANS) return TAC_E_UNSUPPORTED;
    return TAC_OK;
}

int tac_mask_spans_f32(const float* x, int64_t rows, int64_t n_a, int64_t n_b, int64_t stride_r, int64_t stride_a, int64_t stride_b,
                       const int32_t* spans, int64_t span_rows, int32_t k_a, int32_t k_b, const float* value_ptr, float value,
                       float* out, void* stream) {
    using namespace tac;
    if (!x || !out || rows <= 0 || n_a <= 0 || n_b <= 0) return TAC_E_INVALID;
    const int rc = tac_mask_spans_supported(k_a, k_b);
    if (rc != TAC_OK) return rc;
    if (k_a + k_b > 0 && (!spans || (span_rows != 1 && span_rows != rows))) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (n_a == 1) stride_a = 0;
    if (n_b == 1) stride_b = 0;
    if ((rows > 1 && stride_r <= 0) || (n_a > 1 && stride_a <= 0) || (n_b > 1 && stride_b <= 0)) return TAC_E_INVALID;
    MaskGeom g;
    g.rows = rows, g.A = n_a, g.B = n_b, g.sr = stride_r, g.sa = stride_a, g.sb = stride_b;
    g.span_stride = (k_a + k_b > 0 && span_rows == rows && rows > 1) ? 2LL * (k_a + k_b) : 0;
    g.k_a = k_a, g.k_b = k_b;
    const bool turn = stride_a == 1 && stride_b != 1 && n_a > 1 && n_b > 1;
    const int lpl_log = ms_lpl_log(n_b);
    const long long ab_lines = turn ? MS_TURN : (long long)(MS_THREADS >> lpl_log) * MS_PASSES;
    const long long width = turn ? MS_TURN : 4LL << lpl_log;
    const long long n_ab = (n_a + ab_lines - 1) / ab_lines, n_bc = (n_b + width - 1) / width;
    if ((double)rows * (double)n_ab * (double)n_bc > 2147483647.0) return TAC_E_UNSUPPORTED;
    const long long units = rows * n_ab * n_bc;
    g.n_ab = (unsigned)n_ab, g.n_bc = (unsigned)n_bc, g.units = (unsigned)units;
    const bool vec = !turn && stride_b == 1 && n_b % 4 == 0 && stride_a % 4 == 0 && stride_r % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    // Four times the workgroups a CU holds at once (8 of the 16-byte form, 7 of the other two): the dispatcher hands a CU its next
    // workgroup as one leaves, which evens out what a grid of resident workgroups alone leaves uneven (measured: DESIGN 3.17)
    const long long blocks = persistent_blocks(units, 1, (long long)device_cu_count() * 32);
    if (turn)
        return launch_kernel(mask_turn_kernel, blocks, MS_THREADS, 0, (hipStream_t)stream, x, g, (const int*)spans, value_ptr, value, out);
    auto kern = lpl_log == 6 ? (vec ? mask_rows_kernel<true, 6> : mask_rows_kernel<false, 6>)
              : lpl_log == 5 ? (vec ? mask_rows_kernel<true, 5> : mask_rows_kernel<false, 5>)
                             : (vec ? mask_rows_kernel<true, 4> : mask_rows_kernel<false, 4>);
    return launch_kernel(kern, blocks, MS_THREADS, 0, (hipStream_t)stream, x, g, (const int*)spans, value_ptr, value, out);
}

}  // extern "C"
