// mfcc.hip — functional.dct: rows times a small matrix, the DCT-II behind Melspectrogram -> AmplitudeToDb (MFCC) and its adjoint.
//
// out[i][c] = sum_{m < n_in} x(i, m) * mat[m][c] for the rows * n_frames frames i, x element (r, m, t) at
// x[r*stride_r + m*stride_m + t*stride_t] (the convention of tac_apply_filterbank_f32), out dense and frame-major.  The sizes are
// those of a cepstral front end (128 -> 40, 80 -> 13): 2 * n_out flops per input float, i.e. a streaming kernel — the frames are read
// once, the coefficients written once, and the matrix (n_in * n_out <= 32768 floats) stays in the LDS of a persistent workgroup.
//
// Workgroup = 256 threads over a tile of TF frames (64 where the LDS holds it beside the matrix, else 32 or 16).  A tile goes
//   global -> xs[TF][n_in | 1]      lane = frame reads of an odd-pitched row are free of bank conflicts
//   xs x ms[n_in][ldm] -> registers thread (frame = tid % TF, column group = tid / TF) accumulates its group's columns over m in
//                                   ascending order, 16 / 8 / 4 columns at a time; the matrix row is read 16 bytes at a time from an
//                                   address all lanes of a column group share (a broadcast; with TF = 64 a group is a wave)
//   registers -> os[TF][n_out]      the tile as it lies in `out`, copied out with consecutive lanes on consecutive floats
// Every output element is one fused multiply-add chain over m = 0 .. n_in - 1 in one thread: no atomics, one writer per element,
// bit-identical from run to run, and a NaN (or 0 * inf) in a frame reaches every coefficient of that frame as in a dense matmul —
// zero matrix entries are multiplied like any other.
#include "host_common.hpp"

namespace tac {

typedef float dct_f4 __attribute__((ext_vector_type(4)));

constexpr int DCT_THREADS = 256, DCT_MAX_DIM = 256, DCT_MAX_MATRIX = 32768, DCT_LDS_BYTES = 160 * 1024;

// how a tile is fetched: consecutive lanes on consecutive m of a frame (stride_m == 1) as floats or 16 bytes at a time, or
// consecutive lanes on consecutive frames of one m (stride_t == 1, and every other layout)
enum { DCT_LOAD_M = 0, DCT_LOAD_M4 = 1, DCT_LOAD_T = 2 };

template <int NC>
__device__ __forceinline__ void dct_columns(const float* __restrict__ xr, const float* __restrict__ mc, int n_in, int ldm,
                                            float* __restrict__ orow, int c, int n_out) {
    float acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.0f;
#pragma unroll 4
    for (int m = 0; m < n_in; ++m) {
        const float xv = xr[m];
        const dct_f4* b = reinterpret_cast<const dct_f4*>(mc + m * ldm);
#pragma unroll
        for (int j = 0; j < NC / 4; ++j) {
            const dct_f4 v = b[j];
            acc[4 * j + 0] = __builtin_fmaf(xv, v.x, acc[4 * j + 0]);
            acc[4 * j + 1] = __builtin_fmaf(xv, v.y, acc[4 * j + 1]);
            acc[4 * j + 2] = __builtin_fmaf(xv, v.z, acc[4 * j + 2]);
            acc[4 * j + 3] = __builtin_fmaf(xv, v.w, acc[4 * j + 3]);
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (c + j < n_out) orow[c + j] = acc[j];            // (columns n_out .. ldm - 1 are the zero padding of a matrix row)
}

// Dynamic LDS: ms[n_in][ldm] | xs[TF][pitch] | os[TF][n_out], ldm = n_out rounded up to 4, pitch = n_in | 1, TF = 1 << tf_log.
// units = rows * tiles_per_row tiles, walked by a persistent grid.
template <int LOAD>
__global__ void __launch_bounds__(DCT_THREADS)
dct_rows_kernel(const float* __restrict__ x, long long stride_r, long long stride_m, long long stride_t, int n_in,
                long long n_frames, long long tiles_per_row, long long units, int tf_log, const float* __restrict__ mat,
                int n_out, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float dct_lds[];
    const int tid = threadIdx.x;
    const int TF = 1 << tf_log;
    const int ldm = (n_out + 3) & ~3, pitch = n_in | 1;
    float* ms = dct_lds;
    float* xs = ms + n_in * ldm;
    float* os = xs + TF * pitch;

    for (int e = tid; e < n_in * ldm; e += DCT_THREADS) {
        const int r = e / ldm, c = e - r * ldm;
        ms[e] = c < n_out ? mat[r * n_out + c] : 0.0f;
    }

    // this thread's frame of the tile and its share of the columns: a multiple of four per column group
    const int f = tid & (TF - 1), cg = tid >> tf_log;
    const int cw = (((n_out + (DCT_THREADS >> tf_log) - 1) >> (8 - tf_log)) + 3) & ~3;
    const int c_lo = cg * cw, c_hi = c_lo + cw < ldm ? c_lo + cw : ldm;

    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long row = u / tiles_per_row;
        const long long f0 = (u - row * tiles_per_row) << tf_log;
        const int nf = (int)(n_frames - f0 < TF ? n_frames - f0 : TF);
        const float* src = x + row * stride_r + f0 * stride_t;
        if constexpr (LOAD == DCT_LOAD_M4) {
            const int nq = n_in >> 2;
#pragma unroll 4
            for (int e = tid; e < nf * nq; e += DCT_THREADS) {
                const int i = e / nq, q = e - i * nq;
                const dct_f4 v = *reinterpret_cast<const dct_f4*>(src + i * stride_t + 4 * q);
                float* d = xs + i * pitch + 4 * q;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        } else if constexpr (LOAD == DCT_LOAD_M) {
#pragma unroll 4
            for (int e = tid; e < nf * n_in; e += DCT_THREADS) {
                const int i = e / n_in, m = e - i * n_in;
                xs[i * pitch + m] = src[i * stride_t + m];
            }
        } else {
#pragma unroll 4
            for (int e = tid; e < (n_in << tf_log); e += DCT_THREADS) {
                const int m = e >> tf_log, i = e & (TF - 1);
                if (i < nf) xs[i * pitch + m] = src[m * stride_m + i * stride_t];
            }
        }
        __syncthreads();                                    // the tile (and, the first time round, the matrix) is in the LDS
        // (frames nf .. TF - 1 of a row's last tile multiply whatever the LDS holds: their rows of `os` are never copied out)
        for (int c = c_lo; c < c_hi;) {
            const int left = c_hi - c;
            if (left >= 16) {
                dct_columns<16>(xs + f * pitch, ms + c, n_in, ldm, os + f * n_out, c, n_out);
                c += 16;
            } else if (left >= 8) {
                dct_columns<8>(xs + f * pitch, ms + c, n_in, ldm, os + f * n_out, c, n_out);
                c += 8;
            } else {
                dct_columns<4>(xs + f * pitch, ms + c, n_in, ldm, os + f * n_out, c, n_out);
                c += 4;
            }
        }
        __syncthreads();                                    // os is complete; nobody reads xs any more
        float* dst = out + (row * n_frames + f0) * n_out;
        for (int e = tid; e < nf * n_out; e += DCT_THREADS) dst[e] = os[e];
        // (the next tile's os is written only behind the next barrier, which every thread reaches after this copy)
    }
}

// frames per tile: the largest of 64 / 32 / 16 whose tile fits beside the matrix.  16 always does: in floats n_in * ldm <=
// 32768 + 3 * 256 and n_in + n_out <= 256 + 128 under the cap, so at most 33536 + 16 * 385 = 39696 of the 40960 there are.
inline int dct_tile_log(int n_in, int n_out, size_t* bytes) {
    const size_t ldm = (size_t)((n_out + 3) & ~3), pitch = (size_t)(n_in | 1);
    for (int tf_log = 6; tf_log >= 4; --tf_log) {
        *bytes = 4 * ((size_t)n_in * ldm + ((size_t)(pitch + n_out) << tf_log));
        if (*bytes <= (size_t)DCT_LDS_BYTES) return tf_log;
    }
    return -1;
}

}  // namespace tac

extern "C" {

int tac_dct_rows_f32(const float* x, int64_t rows, int32_t n_in, int64_t n_frames, int64_t stride_r, int64_t stride_m,
                     int64_t stride_t, const float* mat, int32_t n_out, float* out, void* stream) {
    using namespace tac;
    if (!x || !mat || !out) return TAC_E_INVALID;
    if (rows <= 0 || n_in <= 0 || n_frames <= 0 || n_out <= 0) return TAC_E_INVALID;
    if (n_in > DCT_MAX_DIM || n_out > DCT_MAX_DIM || n_in * n_out > DCT_MAX_MATRIX) return TAC_E_UNSUPPORTED;
    // an axis of one element has no stride to speak of
    if (rows == 1) stride_r = 0;
    if (n_in == 1) stride_m = 1;
    if (n_frames == 1) stride_t = n_in;
    if ((rows > 1 && stride_r <= 0) || stride_m <= 0 || stride_t <= 0) return TAC_E_INVALID;
    // rows whose frames continue each other in memory are one long run of frames: no partly filled tile at the end of every row
    if (rows > 1 && stride_r == n_frames * stride_t) {
        n_frames *= rows;
        rows = 1;
        stride_r = 0;
    }
    size_t bytes = 0;
    const int tf_log = dct_tile_log(n_in, n_out, &bytes);
    if (tf_log < 0) return TAC_E_UNSUPPORTED;
    const long long tiles_per_row = (n_frames + (1LL << tf_log) - 1) >> tf_log;
    const long long units = rows * tiles_per_row;
    long long per_cu = (long long)(DCT_LDS_BYTES / bytes);
    per_cu = per_cu > 8 ? 8 : per_cu;                       // 8 workgroups of 4 waves fill a CU's 32 wave slots
    const long long blocks = persistent_blocks(units, 1, (long long)device_cu_count() * per_cu);
    const bool along_m = stride_m == 1;
    const bool quads = along_m && (n_in & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_t & 3) == 0 &&
                       (stride_r & 3) == 0;
    auto kern = quads ? dct_rows_kernel<DCT_LOAD_M4> : (along_m ? dct_rows_kernel<DCT_LOAD_M> : dct_rows_kernel<DCT_LOAD_T>);
    return launch_kernel(kern, blocks, DCT_THREADS, bytes, (hipStream_t)stream, x, (long long)stride_r, (long long)stride_m,
                         (long long)stride_t, n_in, (long long)n_frames, tiles_per_row, units, tf_log, mat, n_out, out);
}

}  // extern "C"
