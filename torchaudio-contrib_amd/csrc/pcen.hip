// pcen.hip — functional.pcen: per-channel energy normalisation (Wang et al. 2017, librosa.pcen at max_size = 1) and its gradient.
//
//   M[0] = E[0],  M[t] = a M[t-1] + s E[t],  a = 1 - s
//   out  = bias^power expm1(power log1p(E exp(-gain log(eps + M)) / bias))          (= (E / (eps + M)^gain + bias)^power - bias^power)
//
// Work: a UNIT is one row together with a block of PC_BANDS = 64 bands; a lane owns one band, time runs down the lane's registers.
// The four waves of a workgroup walk the unit's frames in TILES of PC_TILE = 64 frames: wave w holds the w-th CHUNK of PC_C = 16
// consecutive frames of the tile in registers.  The recursion is linear, so a tile costs two short passes and ONE barrier:
//   pass 1   every wave runs its chunk from zero state; the four end states meet in LDS (double-buffered by tile parity);
//   fix-up   state entering wave w = carry a^(C w) + sum_{v < w} end_v a^(C (w - 1 - v)), evaluated by Horner steps with a^C (four
//            squarings of a in float64, in the lane); every wave also forms the tile's outgoing carry, so the carry stays in registers;
//   pass 2   the chunk again from its true state; M is rounded ONCE to float32 and the four transcendentals run in float32.
// State, carries and a^C are float64 ("float64 state, one rounding").  The grid is persistent over units.
//
// Layouts: the input is read where it lies through element strides (row, band, frame).  Frame-major storage (band stride 1: what
// the spectral ops of this library return) makes a frame of the block one coalesced 256-byte segment, loaded straight into the
// owning lanes.  Time-contiguous storage (frame stride 1: a dense (…, F, T) tensor) is loaded along time, coalesced, into a
// [64 bands][64 + 1 frames] LDS array whose skew of one word makes both the store (lanes along time) and the read (lanes along
// bands) conflict-free.  Outputs are frame-major [rows][T][F].
//
// Backward: the same structure walked from the END of the row (tile k holds frames T - 1 - 64 k downwards), one launch:
//   u = eps + M, w = E u^-gain, z = w + bias
//   direct = power z^(power-1) u^-gain,  q = g power z^(power-1) (-gain w / u)
//   lam[t] = q[t] + a lam[t+1],  gE[t] = g direct + (t == 0 ? 1 : s) lam[t]
// with z^(power-1) = bias^(power-1) exp((power-1) log1p(w / bias)).  The four per-band parameter sums
//   d_gain = sum -g power z^(power-1) w log u          d_bias = sum g power bias^(power-1) expm1((power-1) log1p(w / bias))
//   d_power = sum g bias^power (em log bias + (1 + em) l1),  l1 = log1p(w / bias), em = expm1(power l1)      (= z^p log z - b^p log b)
//   d_b = sum_{t >= 1} lam[t] (E[t] - M[t-1])
// are float64 per lane; the four waves' parts are added through LDS in wave order and written per (row, band) to a workspace that
// a small second launch adds over rows in row order.  Nothing is atomic: the same bits from run to run, whatever else is in the batch.
// The bias and power sums use the difference-free forms above: for w << bias the subtractive ones cancel.
//
// NaN: a non-finite E[t] enters M[t] and the carry, so it reaches frames t… of its own (row, band) and nothing else; the gradient's
// lam carries it towards t = 0 of the same (row, band).
#include "host_common.hpp"

namespace tac {

constexpr int PC_THREADS = 256, PC_WAVES = 4;
constexpr int PC_C = 16;                        // frames per chunk: one wave's registers
constexpr int PC_TILE = PC_WAVES * PC_C;        // frames per tile
constexpr int PC_BANDS = 64;                    // bands per unit: one per lane
constexpr int PC_SKEW = PC_TILE + 1;            // row pitch of the turned tile in LDS
constexpr int PC_BLOCKS_PER_CU = 4;             // the forward launch: 104 VGPRs, 20.7 KB of LDS
constexpr int PC_BWD_BLOCKS_PER_CU = 2;         // the backward launch: 200 VGPRs and 45.6 KB of LDS leave two workgroups resident
constexpr int PC_LANES = 64;                    // the wave: PC_BANDS lanes, one band each
static_assert(PC_BANDS == PC_LANES, "a lane owns a band");
static_assert((PC_TILE & (PC_TILE - 1)) == 0, "the turn splits its index by PC_TILE with a mask");
constexpr long long PC_MAX_AXIS = 1LL << 30;    // bands and frames: the in-row indices of the launch stay far inside 64 bits

struct PcSrc {
    const float* p;
    long long sr, sf, st;       // element strides of row, band, frame
    int along_time;             // frame stride 1: tiles are turned through LDS
};

// The chunk's PC_C values of tile [t_lo, t_lo + PC_TILE) of (row, bands f0 …): register c holds frame t_lo + pos(c), pos(c) =
// w C + c, or PC_TILE - 1 - (w C + c) under REV (the backward walk).  Zero outside [0, T) x [0, F).  All threads call it together.
template <bool REV>
__device__ __forceinline__ void pc_load(const PcSrc& S, long long row, int f0, int F, long long t_lo, long long T, int w, int lane,
                                        int tid, float* stage, float (&v)[PC_C]) {
    const float* base = S.p + row * S.sr;
    if (S.along_time) {
        __syncthreads();                                            // (the previous tile is still being read)
        for (int i = tid; i < PC_BANDS * PC_TILE; i += PC_THREADS) {
            const int b = i / PC_TILE, tt = i & (PC_TILE - 1);
            const long long t = t_lo + tt;
            const int f = f0 + b;
            const bool in = f < F && t >= 0 && t < T;
            const float x = base[in ? (long long)f * S.sf + t * S.st : 0];
            stage[b * PC_SKEW + tt] = in ? x : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < PC_C; ++c) v[c] = stage[lane * PC_SKEW + (REV ? PC_TILE - 1 - (w * PC_C + c) : w * PC_C + c)];
    } else {
        const int f = f0 + lane;
#pragma unroll
        for (int c = 0; c < PC_C; ++c) {
            const long long t = t_lo + (REV ? PC_TILE - 1 - (w * PC_C + c) : w * PC_C + c);
            const bool in = f < F && t >= 0 && t < T;
            const float x = base[in ? (long long)f * S.sf + t * S.st : 0];
            v[c] = in ? x : 0.0f;
        }
    }
}

// state entering wave w and the tile's outgoing carry from the incoming carry and the four zero-state chunk ends
__device__ __forceinline__ double pc_fixup(const double (*ends)[PC_LANES], int w, int lane, double aC, double& carry) {
    double st = carry, in = carry;
#pragma unroll
    for (int v = 0; v < PC_WAVES; ++v) {
        if (v == w) in = st;
        st = st * aC + ends[v][lane];
    }
    carry = st;
    return in;
}

__device__ __forceinline__ double pc_pow_chunk(double a) {
#pragma unroll
    for (int i = 0; i < 4; ++i) a *= a;         // a^16 = a^PC_C
    return a;
}
static_assert(PC_C == 16, "pc_pow_chunk squares four times");

struct PcenArgs {
    PcSrc E;
    long long rows, T;
    int F, blocks;
    const float* table;         // [4][F]: gain, bias, power, s
    float eps;
    float* out;                 // [rows][T][F]
    float* M;                   // [rows][T][F] or null
};

__global__ void __launch_bounds__(PC_THREADS) pcen_forward_kernel(PcenArgs A) {
    __shared__ float stage[PC_BANDS * PC_SKEW];
    __shared__ double ends[2][PC_WAVES][PC_LANES];
    const int tid = threadIdx.x, lane = tid & (PC_LANES - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / PC_LANES);
    const long long units = A.rows * A.blocks;
    const int F = A.F;
    const long long T = A.T;
    int par = 0;

    for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const long long row = unit / A.blocks;
        const int f0 = (int)(unit - row * A.blocks) * PC_BANDS;
        const int f = f0 + lane;
        const bool live = f < F;
        const int fc = live ? f : F - 1;
        const float gain = A.table[fc], bias = A.table[F + fc], power = A.table[2 * F + fc];
        const double s = (double)A.table[3 * F + fc], a = 1.0 - s, aC = pc_pow_chunk(a);
        const float bp = expf(power * logf(bias));                  // bias^power
        double carry = 0.0;

        for (long long t0 = 0; t0 < T; t0 += PC_TILE, par ^= 1) {
            float e[PC_C];
            pc_load<false>(A.E, row, f0, F, t0, T, w, lane, tid, stage, e);
            const long long tw = t0 + w * PC_C;
            double m = 0.0;
#pragma unroll
            for (int c = 0; c < PC_C; ++c) m = a * m + (tw + c == 0 ? 1.0 : s) * (double)e[c];
            ends[par][w][lane] = m;
            __syncthreads();
            m = pc_fixup(ends[par], w, lane, aC, carry);
#pragma unroll
            for (int c = 0; c < PC_C; ++c) {
                const long long t = tw + c;
                m = a * m + (t == 0 ? 1.0 : s) * (double)e[c];
                if (live && t < T) {
                    const float m32 = (float)m;
                    const long long at = (row * T + t) * F + f;
                    A.out[at] = bp * expm1f(power * log1pf(e[c] * expf(-gain * logf(A.eps + m32)) / bias));
                    if (A.M) A.M[at] = m32;
                }
            }
        }
    }
}

struct PcenBwdArgs {
    PcSrc E, G;
    const float* M;             // [rows][T][F]
    long long rows, T;
    int F, blocks;
    const float* table;
    float eps;
    int want;                   // bit j: the sum of parameter j (gain, bias, power, s) is formed
    float* gE;                  // [rows][T][F] or null
    double* ws;                 // [4][rows][F]
};

__global__ void __launch_bounds__(PC_THREADS) pcen_backward_kernel(PcenBwdArgs A) {
    __shared__ float stage_e[PC_BANDS * PC_SKEW];
    __shared__ float stage_g[PC_BANDS * PC_SKEW];
    __shared__ double ends[2][PC_WAVES][PC_LANES];
    __shared__ double psum[PC_WAVES][4][PC_LANES];
    const int tid = threadIdx.x, lane = tid & (PC_LANES - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / PC_LANES);
    const long long units = A.rows * A.blocks;
    const int F = A.F;
    const long long T = A.T;
    const long long tiles = (T + PC_TILE - 1) / PC_TILE;
    int par = 0;

    for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const long long row = unit / A.blocks;
        const int f0 = (int)(unit - row * A.blocks) * PC_BANDS;
        const int f = f0 + lane;
        const bool live = f < F;
        const int fc = live ? f : F - 1;
        const float gain = A.table[fc], bias = A.table[F + fc], power = A.table[2 * F + fc];
        const double s = (double)A.table[3 * F + fc], a = 1.0 - s, aC = pc_pow_chunk(a);
        const float lb = logf(bias), bp = expf(power * lb), bpm1 = expf((power - 1.0f) * lb);
        const float* Mrow = A.M + row * T * F;
        double carry = 0.0;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};

        for (long long k = 0; k < tiles; ++k, par ^= 1) {
            const long long t_lo = T - PC_TILE - k * PC_TILE;
            const long long tw = t_lo + PC_TILE - 1 - w * PC_C;     // the frame of register 0; register c holds tw - c
            float e[PC_C], g[PC_C], m[PC_C + 1], q[PC_C], direct[PC_C];
            pc_load<true>(A.E, row, f0, F, t_lo, T, w, lane, tid, stage_e, e);
            pc_load<true>(A.G, row, f0, F, t_lo, T, w, lane, tid, stage_g, g);
#pragma unroll
            for (int c = 0; c <= PC_C; ++c) {
                const long long t = tw - c;
                const bool in = live && t >= 0;                     // (t < T always: tw <= T - 1)
                const float x = Mrow[in ? t * F + f : fc];
                m[c] = in ? x : 0.0f;
            }
            double lam = 0.0;
#pragma unroll
            for (int c = 0; c < PC_C; ++c) {
                const float u = A.eps + m[c], lu = logf(u), ug = expf(-gain * lu);
                const float wv = e[c] * ug, l1 = log1pf(wv / bias);
                const float pz = power * bpm1 * expf((power - 1.0f) * l1);
                direct[c] = pz * ug;
                q[c] = g[c] * pz * (-gain * wv / u);
                if (live && tw - c >= 0) {
                    if (A.want & 1) acc[0] += (double)(-g[c] * pz * wv * lu);
                    if (A.want & 2) acc[1] += (double)(g[c] * power * bpm1 * expm1f((power - 1.0f) * l1));
                    if (A.want & 4) {
                        const float em = expm1f(power * l1);
                        acc[2] += (double)(g[c] * bp * (em * lb + (1.0f + em) * l1));
                    }
                }
                lam = a * lam + (double)q[c];
            }
            ends[par][w][lane] = lam;
            __syncthreads();
            lam = pc_fixup(ends[par], w, lane, aC, carry);
#pragma unroll
            for (int c = 0; c < PC_C; ++c) {
                const long long t = tw - c;
                lam = a * lam + (double)q[c];
                if (live && t >= 0) {
                    if (A.gE) A.gE[(row * T + t) * F + f] = (float)((double)(g[c] * direct[c]) + (t == 0 ? 1.0 : s) * lam);
                    if ((A.want & 8) && t >= 1) acc[3] += lam * ((double)e[c] - (double)m[c + 1]);
                }
            }
        }

        if (A.want) {                                               // the four waves' parts, added in wave order by wave 0
#pragma unroll
            for (int j = 0; j < 4; ++j) psum[w][j][lane] = acc[j];
            __syncthreads();
            if (w == 0 && live) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (A.want >> j & 1)
                        A.ws[((long long)j * A.rows + row) * F + f] = ((psum[0][j][lane] + psum[1][j][lane]) + psum[2][j][lane]) + psum[3][j][lane];
            }
            // (psum is written again only behind the next unit's tile barrier, which wave 0 reaches after these reads)
        }
    }
}

// grad_table[j][f] = the workspace summed over rows in row order, zero for a parameter whose sum was not formed
__global__ void __launch_bounds__(PC_THREADS) pcen_reduce_kernel(const double* ws, long long rows, int F, int want, float* grad_table) {
    const long long i = (long long)blockIdx.x * PC_THREADS + threadIdx.x;
    if (i >= 4LL * F) return;
    const int j = (int)(i / F), f = (int)(i - (long long)j * F);
    double sum = 0.0;
    if (want >> j & 1) {
        const double* p = ws + (long long)j * rows * F + f;
        for (long long r = 0; r < rows; ++r) sum += p[r * F];
    }
    grad_table[i] = (float)sum;
}

inline PcSrc pc_src(const float* p, long long sr, long long sf, long long st, long long F, long long T) {
    PcSrc s;
    s.p = p; s.sr = sr; s.sf = sf; s.st = st;
    s.along_time = (T > 1 && st == 1 && (F == 1 || sf != 1)) ? 1 : 0;
    return s;
}

inline int pc_shape_error(long long rows, long long F, long long T) {
    if (rows <= 0 || F <= 0 || T <= 0) return TAC_E_INVALID;
    if (F > PC_MAX_AXIS || T > PC_MAX_AXIS || rows > (1LL << 40) / ((F + PC_BANDS - 1) / PC_BANDS)) return TAC_E_UNSUPPORTED;
    return TAC_OK;
}

}  // namespace tac

extern "C" {

int32_t tac_pcen_chunk_frames(void) { return tac::PC_C; }
int32_t tac_pcen_tile_frames(void) { return tac::PC_TILE; }
int32_t tac_pcen_block_bands(void) { return tac::PC_BANDS; }
int32_t tac_pcen_blocks_per_cu(void) { return tac::PC_BLOCKS_PER_CU; }
int64_t tac_pcen_max_axis(void) { return tac::PC_MAX_AXIS; }

int tac_pcen_f32(const float* specgram, int64_t rows, int64_t n_bands, int64_t n_frames, int64_t stride_r, int64_t stride_f,
                 int64_t stride_t, const float* table, float eps, float* out, float* smoother, void* stream) {
    using namespace tac;
    if (!specgram || !table || !out) return TAC_E_INVALID;
    const int rc = pc_shape_error(rows, n_bands, n_frames);
    if (rc != TAC_OK) return rc;
    if (stride_r < 0 || stride_f < 0 || stride_t < 0) return TAC_E_INVALID;
    PcenArgs a;
    a.E = pc_src(specgram, stride_r, stride_f, stride_t, n_bands, n_frames);
    a.rows = rows; a.T = n_frames; a.F = (int)n_bands; a.blocks = (int)((n_bands + PC_BANDS - 1) / PC_BANDS);
    a.table = table; a.eps = eps; a.out = out; a.M = smoother;
    const long long blocks = persistent_blocks(rows * a.blocks, 1, (long long)device_cu_count() * PC_BLOCKS_PER_CU);
    return launch_kernel(pcen_forward_kernel, blocks, PC_THREADS, 0, (hipStream_t)stream, a);
}

int tac_pcen_backward_f32(const float* grad_out, int64_t grad_stride_r, int64_t grad_stride_f, int64_t grad_stride_t,
                          const float* specgram, int64_t rows, int64_t n_bands, int64_t n_frames, int64_t stride_r, int64_t stride_f,
                          int64_t stride_t, const float* smoother, const float* table, float eps, int32_t want, float* grad_specgram,
                          double* workspace, float* grad_table, void* stream) {
    using namespace tac;
    if (!grad_out || !specgram || !smoother || !table) return TAC_E_INVALID;
    const int rc = pc_shape_error(rows, n_bands, n_frames);
    if (rc != TAC_OK) return rc;
    if (stride_r < 0 || stride_f < 0 || stride_t < 0 || grad_stride_r < 0 || grad_stride_f < 0 || grad_stride_t < 0) return TAC_E_INVALID;
    if (want < 0 || want > 15 || (want && (!workspace || !grad_table)) || (!want && !grad_specgram)) return TAC_E_INVALID;
    PcenBwdArgs a;
    a.E = pc_src(specgram, stride_r, stride_f, stride_t, n_bands, n_frames);
    a.G = pc_src(grad_out, grad_stride_r, grad_stride_f, grad_stride_t, n_bands, n_frames);
    a.M = smoother; a.rows = rows; a.T = n_frames; a.F = (int)n_bands; a.blocks = (int)((n_bands + PC_BANDS - 1) / PC_BANDS);
    a.table = table; a.eps = eps; a.want = want; a.gE = grad_specgram; a.ws = workspace;
    const long long blocks = persistent_blocks(rows * a.blocks, 1, (long long)device_cu_count() * PC_BWD_BLOCKS_PER_CU);
    const int launched = launch_kernel(pcen_backward_kernel, blocks, PC_THREADS, 0, (hipStream_t)stream, a);
    if (launched != TAC_OK || !want) return launched;
    return launch_kernel(pcen_reduce_kernel, (4 * n_bands + PC_THREADS - 1) / PC_THREADS, PC_THREADS, 0, (hipStream_t)stream,
                         (const double*)workspace, (long long)rows, (int)n_bands, (int)want, grad_table);
}

}  // extern "C"
