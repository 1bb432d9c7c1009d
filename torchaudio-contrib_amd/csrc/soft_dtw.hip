// soft_dtw.hip — soft-DTW (functional.soft_dtw, SoftDTW; Cuturi & Blondel 2017) between x (B, N, D) and y (B, M, D) with the squared
// Euclidean cost, its gradient by both inputs and the expected alignment, read and written through element strides.
//
//   delta[i][j] = sum_d (x[i][d] - y[j][d])^2
//   R[i][j] = delta[i][j] + softmin_gamma(R[i-1][j], R[i][j-1], R[i-1][j-1]),  R[-1][-1] = 0, +inf on the rest of the border
//   value = R[Nb-1][Mb-1];  Q: the same recursion from (Nb-1, Mb-1) downwards
//   E[i][j] = exp(-(R + Q - delta - value) / gamma);  grad_x[i] = 2 g (x[i] sum_j E[i][j] - sum_j E[i][j] y[j]), grad_y likewise
//
// THE SKEWED LAYOUT.  delta, R and Q are float32 [B][N + M - 1][N]: element (i, j) lies in row k = i + j at position i.  Step k of
// the wavefront then reads and writes one contiguous run of its row, and a 32 x 32 tile of (i, j) is 63 runs of up to 32 dwords.
// Every element of the three arrays is written: ZERO wherever (k - i) is no column of the entry or i no row of it.
//
// (1) sd_cost_kernel: a workgroup owns 32 positions i by 32 diagonals k, which meet 63 columns j.  It stages the 32 x rows and the
//     63 y rows SD_COST_DC features at a time in the LDS — 16-byte loads where base, strides and D allow, dwords otherwise, the
//     same values in the same places, zeros behind D and outside the entry — and a thread sums (x - y)^2 for four cells in the
//     order of d.  The difference form, not |x|^2 + |y|^2 - 2 x.y: that one cancels where DTW paths run.  Coalesced stores.
// (2) sd_lattice_kernel: one workgroup per (entry, direction); the R workgroups alone when neither gradient nor alignment is
//     wanted, and then nothing but the value is written.  A lane owns ROWS consecutive rows (1, 2 or 4: 4096 rows fit 1024
//     lanes) and at step k computes its cells of diagonal k, which depend on step k - 1 and k - 2 only.  It keeps both earlier
//     values of its rows in registers; the row below its first comes from the lower lane by a one-lane wave shift, across
//     waves through two alternating LDS rows with one barrier a step, and that value of the step before is the diagonal
//     predecessor.  Q RUNS THE SAME CODE ON THE MIRRORED ENTRY (i, j) -> (Nb - 1 - i, Mb - 1 - j): only the addresses differ.
//     Costs are loaded SD_RING steps ahead into a register ring at clamped indices.  N + M - 1 dependent steps.
// (3) sd_grad_kernel: a workgroup per (entry, side, tile of 32 rows of that side) walks the other axis in tiles of 32.  Per tile
//     its 256 threads read R, Q and delta of four cells each along the diagonals (two contiguous runs per half wave), form E
//     and put it into the LDS de-skewed (for the y side transposed); lanes 0..31 add up the rows in the order of the columns;
//     each of the four waves multiplies the E tile with its two 32-column blocks of the other sequence on
//     v_mfma_f32_32x32x2_f32, the other sequence loaded into the B operand straight from memory with zeros behind D and behind
//     the entry.  E never goes to memory.  sd_align_kernel is the same E evaluation stored (B, N, M) for return_alignment.
//
// No atomics; every sum has one fixed order; a workgroup reads nothing of another entry.  An entry with Nb outside [1, N] or Mb
// outside [1, M] gets a NaN value, NaN R / Q / E and NaN gradients over its blocks, and no address is formed from such a length.
#include <math.h>

#include "host_common.hpp"
#include "soft_dtw_plan.hpp"

// the 16-byte and the dword form of the cost launch must round alike
#pragma clang fp contract(off)

namespace tac {

typedef float sd_f32x16 __attribute__((ext_vector_type(16)));
typedef float sd_f4 __attribute__((ext_vector_type(4)));

struct SdGeom {
    long long xb, xn, xd;                       // element strides of x (B, N, D)
    long long yb, ym, yd;                       // and of y (B, M, D)
    int B, N, M, D, K;                          // K = N + M - 1 diagonals
    float gamma, inv_gamma;
};

struct SdGradOut {
    float* gx;
    float* gy;
    long long gxb, gxn, gxd, gyb, gym, gyd;
};

// lane i receives lane i - 1's value (lane 0: unspecified, replaced by the caller)
__device__ __forceinline__ float sd_from_lower_lane(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

// -gamma log(e^{-a/gamma} + e^{-b/gamma} + e^{-c/gamma}) around the minimum; three +inf give +inf
__device__ __forceinline__ float sd_softmin(float a, float b, float c, float gamma, float inv_gamma) {
    const float m = fminf(fminf(a, b), c), mm = m == INFINITY ? 0.0f : m;
    const float s = (__expf((mm - a) * inv_gamma) + __expf((mm - b) * inv_gamma)) + __expf((mm - c) * inv_gamma);
    return m - gamma * __logf(s);
}

__device__ __forceinline__ bool sd_entry(const SdGeom& g, int b, const int* __restrict__ xlen, const int* __restrict__ ylen, int& Nb,
                                         int& Mb) {
    Nb = xlen[b], Mb = ylen[b];
    return Nb >= 1 && Nb <= g.N && Mb >= 1 && Mb <= g.M;
}

// ---------------------------------------------------------------------------------------------------------------- (1) the costs
template <bool VEC>
__device__ __forceinline__ void sd_stage(float* __restrict__ lds, const float* __restrict__ src, long long sr, long long sd, int row0,
                                         int rows, int valid_rows, int d0, int D, int tid) {
    if constexpr (VEC) {
        for (int e = tid; e < rows * (SD_COST_DC / 4); e += 64 * SD_WAVES) {
            const int r = e / (SD_COST_DC / 4), c = 4 * (e % (SD_COST_DC / 4)), row = row0 + r;
            sd_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (row >= 0 && row < valid_rows && d0 + c < D) v = *reinterpret_cast<const sd_f4*>(src + row * sr + (d0 + c));
            float* at = lds + r * (SD_COST_DC + 1) + c;
            at[0] = v.x, at[1] = v.y, at[2] = v.z, at[3] = v.w;
        }
    } else {
        for (int e = tid; e < rows * SD_COST_DC; e += 64 * SD_WAVES) {
            const int r = e / SD_COST_DC, c = e % SD_COST_DC, row = row0 + r;
            float v = 0.0f;
            if (row >= 0 && row < valid_rows && d0 + c < D) v = src[row * sr + (d0 + c) * sd];
            lds[r * (SD_COST_DC + 1) + c] = v;
        }
    }
}

template <bool VX, bool VY>
__global__ void __launch_bounds__(64 * SD_WAVES)
sd_cost_kernel(const float* __restrict__ x_all, const float* __restrict__ y_all, SdGeom g, const int* __restrict__ xlen,
               const int* __restrict__ ylen, float* __restrict__ delta_all, int tiles_i, int tiles_k) {
    __shared__ float xs[SD_TILE * (SD_COST_DC + 1)];
    __shared__ float ys[(2 * SD_TILE - 1) * (SD_COST_DC + 1)];
    const int tid = threadIdx.x, li = tid & 31, grp = tid >> 5;
    const int ti = blockIdx.x % tiles_i, rest = blockIdx.x / tiles_i, tk = rest % tiles_k, b = rest / tiles_k;
    const int i0 = ti * SD_TILE, k0 = tk * SD_TILE, jlo = k0 - i0 - (SD_TILE - 1);   // columns jlo .. jlo + 62
    const int W = g.N;
    float* __restrict__ delta = delta_all + (long long)b * g.K * W;
    int Nb, Mb;
    const bool ok = sd_entry(g, b, xlen, ylen, Nb, Mb);
    const int i = i0 + li;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool dead = !ok || i0 >= Nb || jlo + 2 * SD_TILE - 2 < 0 || jlo >= Mb;    // (the same in every thread)
    if (!dead) {
        const float* __restrict__ x = x_all + b * g.xb;
        const float* __restrict__ y = y_all + b * g.yb;
        for (int d0 = 0; d0 < g.D; d0 += SD_COST_DC) {
            sd_stage<VX>(xs, x, g.xn, g.xd, i0, SD_TILE, Nb, d0, g.D, tid);
            sd_stage<VY>(ys, y, g.ym, g.yd, jlo, 2 * SD_TILE - 1, Mb, d0, g.D, tid);
            __syncthreads();
            const int dlen = min(SD_COST_DC, g.D - d0);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float* __restrict__ xr = xs + li * (SD_COST_DC + 1);
                const float* __restrict__ yr = ys + (grp + 8 * c - li + SD_TILE - 1) * (SD_COST_DC + 1);
                float a = acc[c];
                for (int d = 0; d < dlen; ++d) {
                    const float t = xr[d] - yr[d];
                    a += t * t;
                }
                acc[c] = a;
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = k0 + grp + 8 * c, j = k - i;
        if (i < W && k < g.K) delta[(long long)k * W + i] = (!dead && i < Nb && j >= 0 && j < Mb) ? acc[c] : 0.0f;
    }
}

// -------------------------------------------------------------------------------------------------------------- (2) the lattice
template <int ROWS, bool MANY, bool STORE>      // MANY: more than one wave; STORE: R and Q are wanted
__global__ void __launch_bounds__(MANY ? SD_LANES : 64)
sd_lattice_kernel(const float* __restrict__ delta_all, SdGeom g, const int* __restrict__ xlen, const int* __restrict__ ylen,
                  float* __restrict__ r_all, float* __restrict__ q_all, float* __restrict__ value) {
    __shared__ float edge[2][SD_LANES / 64];
    const int b = STORE ? blockIdx.x >> 1 : blockIdx.x, dir = STORE ? blockIdx.x & 1 : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = g.N, K = g.K;
    const float inf = INFINITY, gamma = g.gamma, inv_gamma = g.inv_gamma;
    const float* __restrict__ delta = delta_all + (long long)b * K * W;
    float* __restrict__ out = STORE ? (dir ? q_all : r_all) + (long long)b * K * W : nullptr;

    int Nb, Mb;
    if (!sd_entry(g, b, xlen, ylen, Nb, Mb)) {  // (the same in every thread)
        if constexpr (STORE)
            for (long long e = tid; e < (long long)K * W; e += blockDim.x) out[e] = NAN;
        if (dir == 0 && tid == 0) value[b] = NAN;
        return;
    }
    const int nsteps = Nb + Mb - 1;
    if constexpr (STORE)
        for (long long e = (long long)nsteps * W + tid; e < (long long)K * W; e += blockDim.x) out[e] = 0.0f;

    // the lane's rows in the walk's own (mirrored for Q) numbering, and where they lie
    int at[ROWS];                               // position in a row of the arrays; -1: none
    int from[ROWS];                             // position the cost is loaded from (clamped into the entry)
#pragma unroll
    for (int a = 0; a < ROWS; ++a) {
        const int iw = tid * ROWS + a, ic = min(iw, Nb - 1);
        at[a] = iw < Nb ? (dir ? Nb - 1 - iw : iw) : (iw < W ? iw : -1);
        from[a] = dir ? Nb - 1 - ic : ic;
    }
    auto row_of = [&](int step) {               // step d of the walk is diagonal d, or nsteps - 1 - d for Q
        const int sc = min(step, nsteps - 1);
        return (long long)(dir ? nsteps - 1 - sc : sc) * W;
    };
    float DL[SD_RING][ROWS];                    // a ring of steps, every index static
#pragma unroll
    for (int s = 0; s < SD_RING; ++s)
#pragma unroll
        for (int a = 0; a < ROWS; ++a) DL[s][a] = delta[row_of(s) + from[a]];

    float cur[ROWS], old[ROWS];                 // the rows' values of step d - 1 and d - 2
#pragma unroll
    for (int a = 0; a < ROWS; ++a) cur[a] = old[a] = inf;
    float below_old = tid == 0 ? 0.0f : inf;    // the row below the lane's first at step d - 2; R[-1][-1] = 0 starts the walk
#pragma unroll 1
    for (int d0 = 0; d0 < nsteps; d0 += SD_RING) {
#pragma unroll
        for (int s = 0; s < SD_RING; ++s) {
            const int d = d0 + s;
            if (d >= nsteps) break;             // (the same in every thread)
            float dl[ROWS];
#pragma unroll
            for (int a = 0; a < ROWS; ++a) dl[a] = DL[s][a];
            const long long ahead = row_of(d + SD_RING);
#pragma unroll
            for (int a = 0; a < ROWS; ++a) DL[s][a] = delta[ahead + from[a]];
            float below = sd_from_lower_lane(cur[ROWS - 1]);
            if constexpr (MANY) {
                if (lane == 63) edge[d & 1][wave] = cur[ROWS - 1];
                __syncthreads();
                if (lane == 0 && wave > 0) below = edge[d & 1][wave - 1];
            }
            if (tid == 0) below = inf;
            float nw[ROWS];
            bool live[ROWS];
#pragma unroll
            for (int a = 0; a < ROWS; ++a) {
                const int iw = tid * ROWS + a, jw = d - iw;
                live[a] = iw < Nb && jw >= 0 && jw < Mb;
                const float up = a == 0 ? below : cur[a - 1], diag = a == 0 ? below_old : old[a - 1];
                const float v = dl[a] + sd_softmin(up, cur[a], diag, gamma, inv_gamma);
                nw[a] = live[a] ? v : inf;
            }
            below_old = below;
#pragma unroll
            for (int a = 0; a < ROWS; ++a) old[a] = cur[a], cur[a] = nw[a];
            if constexpr (STORE) {
                float* __restrict__ row = out + row_of(d);
#pragma unroll
                for (int a = 0; a < ROWS; ++a)
                    if (at[a] >= 0) row[at[a]] = live[a] ? cur[a] : 0.0f;
            }
        }
    }
    if (dir == 0) {
#pragma unroll
        for (int a = 0; a < ROWS; ++a)
            if (tid * ROWS + a == Nb - 1) value[b] = cur[a];
    }
}

// ------------------------------------------------------------------------------------------------- (3) gradient and alignment
// E of cell (i, j) of a live entry from the skewed arrays; zero outside the entry without a read
__device__ __forceinline__ float sd_e_cell(const float* __restrict__ delta, const float* __restrict__ r, const float* __restrict__ q,
                                           int W, int i, int j, int Nb, int Mb, float val, float inv_gamma) {
    if (i >= Nb || j >= Mb) return 0.0f;
    const long long at = (long long)(i + j) * W + i;
    const float excess = ((r[at] + q[at]) - delta[at]) - val;
    const float arg = -excess * inv_gamma;
    return __expf(arg > 0.0f ? 0.0f : arg);     // (a NaN stays a NaN)
}

__global__ void __launch_bounds__(64 * SD_WAVES)
sd_grad_kernel(const float* __restrict__ x_all, const float* __restrict__ y_all, SdGeom g, SdGradOut o, const int* __restrict__ xlen,
               const int* __restrict__ ylen, const float* __restrict__ delta_all, const float* __restrict__ r_all,
               const float* __restrict__ q_all, const float* __restrict__ value, const float* __restrict__ grad_value, int tiles_n,
               int tiles_m) {
    __shared__ float es[SD_TILE * SD_E_STRIDE];
    __shared__ float sums[SD_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = tid & 31, grp = tid >> 5, lk = lane >> 5;
    const int per = tiles_n + tiles_m, b = blockIdx.x / per, t = blockIdx.x - b * per;
    const bool ys = t >= tiles_n;               // the side: rows of y (columns of the lattice), else rows of x
    const int r0 = (ys ? t - tiles_n : t) * SD_TILE;
    const int W = g.N, D = g.D;
    float* __restrict__ gout = ys ? o.gy : o.gx;
    if (!gout) return;                          // (the same in every thread)
    const long long gb = ys ? o.gyb : o.gxb, gr = ys ? o.gym : o.gxn, gd = ys ? o.gyd : o.gxd;
    const long long base = (long long)b * g.K * W;
    const float* __restrict__ delta = delta_all + base;
    const float* __restrict__ rr = r_all + base;
    const float* __restrict__ qq = q_all + base;
    int Nb, Mb;
    const bool ok = sd_entry(g, b, xlen, ylen, Nb, Mb);
    const int rows_all = ys ? g.M : g.N, rows = ok ? (ys ? Mb : Nb) : 0, others = ok ? (ys ? Nb : Mb) : 0;
    gout += b * gb;
    if (!ok || r0 >= rows) {                    // an invalid entry: NaN over its block; rows behind the entry: zeros
        const float fill = ok ? 0.0f : NAN;
        for (int e = tid; e < SD_TILE * D; e += blockDim.x) {
            const int row = r0 + e / D, d = e % D;
            if (row < rows_all) gout[row * gr + d * gd] = fill;
        }
        return;
    }
    const float* __restrict__ self = ys ? y_all + b * g.yb : x_all + b * g.xb;
    const float* __restrict__ other = ys ? x_all + b * g.xb : y_all + b * g.yb;
    const long long self_r = ys ? g.ym : g.xn, self_d = ys ? g.yd : g.xd, other_r = ys ? g.xn : g.ym, other_d = ys ? g.xd : g.yd;
    const float val = value[b], inv_gamma = g.inv_gamma;

    sd_f32x16 acc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.0f;
    float rowsum = 0.0f;
    const int i_base = ys ? 0 : r0, j_base = ys ? r0 : 0;
    for (int o0 = 0; o0 < others; o0 += SD_TILE) {
        // ---- E of the tile: thread (li, dd) has row li of x's side and the column (dd - li) mod 32, so that 32 lanes read two runs
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int jl = (grp + 8 * c - li) & (SD_TILE - 1);
            const int i = i_base + (ys ? o0 : 0) + li, j = j_base + (ys ? 0 : o0) + jl;
            const float e = sd_e_cell(delta, rr, qq, W, i, j, Nb, Mb, val, inv_gamma);
            es[ys ? jl * SD_E_STRIDE + li : li * SD_E_STRIDE + jl] = e;
        }
        __syncthreads();
        if (tid < SD_TILE) {
            const float* __restrict__ er = es + tid * SD_E_STRIDE;
            for (int c = 0; c < SD_TILE; ++c) rowsum += er[c];
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int c0 = (wave + SD_WAVES * c) * SD_TILE;
            if (c0 >= D) break;                 // (the same in a wave)
            const int d = c0 + li;
            float bv[SD_TILE / 2];
#pragma unroll
            for (int s = 0; s < SD_TILE / 2; ++s) {
                const int orow = o0 + 2 * s + lk;
                bv[s] = (orow < others && d < D) ? other[orow * other_r + d * other_d] : 0.0f;
            }
#pragma unroll
            for (int s = 0; s < SD_TILE / 2; ++s)
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(es[li * SD_E_STRIDE + 2 * s + lk], bv[s], acc[c], 0, 0, 0);
        }
        __syncthreads();
    }
    if (tid < SD_TILE) sums[tid] = rowsum;
    __syncthreads();
    // D[i][j] of a 32 x 32 block: j = lane % 32, i = 8 (r / 4) + 4 (lane / 32) + r % 4
    const float two_g = 2.0f * grad_value[b];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int d = (wave + SD_WAVES * c) * SD_TILE + li;
        if (d >= D) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = 8 * (r >> 2) + 4 * lk + (r & 3), row = r0 + rl;
            if (row >= rows_all) continue;
            float v = 0.0f;
            if (row < rows) v = two_g * (self[row * self_r + d * self_d] * sums[rl] - acc[c][r]);
            gout[row * gr + d * gd] = v;
        }
    }
}

__global__ void __launch_bounds__(64 * SD_WAVES)
sd_align_kernel(SdGeom g, const int* __restrict__ xlen, const int* __restrict__ ylen, const float* __restrict__ delta_all,
                const float* __restrict__ r_all, const float* __restrict__ q_all, const float* __restrict__ value,
                float* __restrict__ e_all, int tiles_n, int tiles_m) {
    __shared__ float es[SD_TILE * SD_E_STRIDE];
    const int tid = threadIdx.x, li = tid & 31, grp = tid >> 5;
    const int tj = blockIdx.x % tiles_m, rest = blockIdx.x / tiles_m, ti = rest % tiles_n, b = rest / tiles_n;
    const int i0 = ti * SD_TILE, j0 = tj * SD_TILE, W = g.N;
    const long long base = (long long)b * g.K * W;
    int Nb, Mb;
    const bool ok = sd_entry(g, b, xlen, ylen, Nb, Mb);
    if (ok && i0 < Nb && j0 < Mb) {             // (the same in every thread)
        const float val = value[b];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int jl = (grp + 8 * c - li) & (SD_TILE - 1);
            es[li * SD_E_STRIDE + jl] = sd_e_cell(delta_all + base, r_all + base, q_all + base, W, i0 + li, j0 + jl, Nb, Mb, val, g.inv_gamma);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) es[li * SD_E_STRIDE + ((grp + 8 * c - li) & (SD_TILE - 1))] = ok ? 0.0f : NAN;
    }
    __syncthreads();
    float* __restrict__ e_out = e_all + (long long)b * g.N * g.M;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int i = i0 + grp + 8 * c, j = j0 + li;
        if (i < g.N && j < g.M) e_out[(long long)i * g.M + j] = es[(grp + 8 * c) * SD_E_STRIDE + li];
    }
}

inline bool sd_strides_ok(int64_t batch, int64_t rows, int64_t d, int64_t& sb, int64_t& sr, int64_t& sd) {
    if (batch == 1) sb = 0;
    if (rows == 1) sr = 0;
    if (d == 1) sd = 0;
    return !((batch > 1 && sb <= 0) || (rows > 1 && sr <= 0) || (d > 1 && sd <= 0));
}

inline int sd_geometry(const float* x, const float* y, int64_t batch, int64_t n, int64_t m, int64_t d, int64_t xb, int64_t xn,
                       int64_t xd, int64_t yb, int64_t ym, int64_t yd, float gamma, SdGeom* g) {
    const int status = sd_shape_status(batch, n, m, d);
    if (!x || !y || status == 1 || !(gamma > 0.0f) || !isfinite(gamma)) return TAC_E_INVALID;
    if (!sd_strides_ok(batch, n, d, xb, xn, xd) || !sd_strides_ok(batch, m, d, yb, ym, yd)) return TAC_E_INVALID;
    if (status == 2) return TAC_E_UNSUPPORTED;
    g->xb = xb, g->xn = xn, g->xd = xd, g->yb = yb, g->ym = ym, g->yd = yd;
    g->B = (int)batch, g->N = (int)n, g->M = (int)m, g->D = (int)d, g->K = (int)sd_diagonals(n, m);
    g->gamma = gamma, g->inv_gamma = (float)(1.0 / (double)gamma);
    return TAC_OK;
}

inline bool sd_vec(const float* p, long long sb, long long sr, long long sd, int D) {
    return D % 4 == 0 && sd == 1 && sb % 4 == 0 && sr % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace tac

extern "C" {

int32_t tac_soft_dtw_max_len(void) { return tac::SD_MAX_LEN; }

int32_t tac_soft_dtw_max_dim(void) { return tac::SD_MAX_DIM; }

int32_t tac_soft_dtw_lanes(void) { return tac::SD_LANES; }

int32_t tac_soft_dtw_tile(void) { return tac::SD_TILE; }

int32_t tac_soft_dtw_rows_per_lane(int64_t rows) { return tac::sd_rows_per_lane(rows); }

int tac_soft_dtw_f32(const float* x, const float* y, int64_t batch, int64_t n, int64_t m, int64_t d, int64_t x_stride_b,
                     int64_t x_stride_n, int64_t x_stride_d, int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d,
                     const int32_t* x_lengths, const int32_t* y_lengths, float gamma, float* cost, float* r, float* q, float* value,
                     void* stream) {
    using namespace tac;
    SdGeom g;
    int rc = sd_geometry(x, y, batch, n, m, d, x_stride_b, x_stride_n, x_stride_d, y_stride_b, y_stride_m, y_stride_d, gamma, &g);
    if (rc != TAC_OK) return rc;
    if (!x_lengths || !y_lengths || !cost || !value || (r == nullptr) != (q == nullptr)) return TAC_E_INVALID;
    const int tiles_i = (int)sd_tiles(n), tiles_k = (int)sd_tiles(g.K);
    const bool vx = sd_vec(x, g.xb, g.xn, g.xd, g.D), vy = sd_vec(y, g.yb, g.ym, g.yd, g.D);
#define SD_COST(VX, VY)                                                                                                           \
    launch_kernel(sd_cost_kernel<VX, VY>, sd_cost_blocks(batch, n, m), 64 * SD_WAVES, 0, (hipStream_t)stream, x, y, g,            \
                  (const int*)x_lengths, (const int*)y_lengths, cost, tiles_i, tiles_k)
    rc = vx ? (vy ? SD_COST(true, true) : SD_COST(true, false)) : (vy ? SD_COST(false, true) : SD_COST(false, false));
#undef SD_COST
    if (rc != TAC_OK) return rc;
    const bool store = r != nullptr;
    const int rows = sd_rows_per_lane(n), threads = sd_threads(n);
    const long long blocks = store ? 2 * batch : batch;
#define SD_LAT(ROWS, MANY, STORE)                                                                                          \
    launch_kernel(sd_lattice_kernel<ROWS, MANY, STORE>, blocks, threads, 0, (hipStream_t)stream, (const float*)cost, g,    \
                  (const int*)x_lengths, (const int*)y_lengths, r, q, value)
#define SD_PICK(ROWS, MANY) (store ? SD_LAT(ROWS, MANY, true) : SD_LAT(ROWS, MANY, false))
    if (rows == 4) return SD_PICK(4, true);
    if (rows == 2) return SD_PICK(2, true);
    return threads > 64 ? SD_PICK(1, true) : SD_PICK(1, false);
#undef SD_PICK
#undef SD_LAT
}

int tac_soft_dtw_grad_f32(const float* x, const float* y, int64_t batch, int64_t n, int64_t m, int64_t d, int64_t x_stride_b,
                          int64_t x_stride_n, int64_t x_stride_d, int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d,
                          const int32_t* x_lengths, const int32_t* y_lengths, float gamma, const float* cost, const float* r,
                          const float* q, const float* value, const float* grad_value, float* grad_x, int64_t gx_stride_b,
                          int64_t gx_stride_n, int64_t gx_stride_d, float* grad_y, int64_t gy_stride_b, int64_t gy_stride_m,
                          int64_t gy_stride_d, void* stream) {
    using namespace tac;
    SdGeom g;
    const int rc = sd_geometry(x, y, batch, n, m, d, x_stride_b, x_stride_n, x_stride_d, y_stride_b, y_stride_m, y_stride_d, gamma, &g);
    if (rc != TAC_OK) return rc;
    if (!x_lengths || !y_lengths || !cost || !r || !q || !value || !grad_value || (!grad_x && !grad_y)) return TAC_E_INVALID;
    if (grad_x && !sd_strides_ok(batch, n, d, gx_stride_b, gx_stride_n, gx_stride_d)) return TAC_E_INVALID;
    if (grad_y && !sd_strides_ok(batch, m, d, gy_stride_b, gy_stride_m, gy_stride_d)) return TAC_E_INVALID;
    const SdGradOut o = {grad_x, grad_y, gx_stride_b, gx_stride_n, gx_stride_d, gy_stride_b, gy_stride_m, gy_stride_d};
    return launch_kernel(sd_grad_kernel, sd_grad_blocks(batch, n, m), 64 * SD_WAVES, 0, (hipStream_t)stream, x, y, g, o,
                         (const int*)x_lengths, (const int*)y_lengths, cost, r, q, value, grad_value, (int)sd_tiles(n), (int)sd_tiles(m));
}

int tac_soft_dtw_alignment_f32(int64_t batch, int64_t n, int64_t m, const int32_t* x_lengths, const int32_t* y_lengths, float gamma,
                               const float* cost, const float* r, const float* q, const float* value, float* alignment, void* stream) {
    using namespace tac;
    if (sd_shape_status(batch, n, m, 1) == 1 || !(gamma > 0.0f) || !isfinite(gamma)) return TAC_E_INVALID;
    if (sd_shape_status(batch, n, m, 1) == 2 || sd_align_blocks(batch, n, m) > 0x7fffffff) return TAC_E_UNSUPPORTED;
    if (!x_lengths || !y_lengths || !cost || !r || !q || !value || !alignment) return TAC_E_INVALID;
    SdGeom g = {};
    g.B = (int)batch, g.N = (int)n, g.M = (int)m, g.D = 1, g.K = (int)sd_diagonals(n, m);
    g.gamma = gamma, g.inv_gamma = (float)(1.0 / (double)gamma);
    return launch_kernel(sd_align_kernel, sd_align_blocks(batch, n, m), 64 * SD_WAVES, 0, (hipStream_t)stream, g, (const int*)x_lengths,
                         (const int*)y_lengths, cost, r, q, value, alignment, (int)sd_tiles(n), (int)sd_tiles(m));
}

}  // extern "C"
