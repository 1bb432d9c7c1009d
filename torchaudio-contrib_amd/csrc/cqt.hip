// cqt.hip — functional.cqt: the time-domain constant-Q / variable-Q transform as a band-sparse fp32 MFMA GEMM, one launch.
//
//   C[k][t] = sum_j x_pad[c_t + j - floor(N_k / 2)] conj(g_k[j])
//
// is a GEMM whose one operand is the complex wavelet bank (built, normalised, scaled and conjugated on the host in float64,
// _cqt.py) and whose other operand is a Toeplitz view of the waveform: frame t reads the samples t hop + e, e the TAP AXIS every
// wavelet is laid on with its centre at e = c0 = floor(N_0 / 2).  Bin k lives on [c0 - floor(N_k / 2), c0 - floor(N_k / 2) + N_k):
// the supports nest, the lowest octave holds half of all taps.
//
// Bank: bins are cut into GROUPS of 8 consecutive bins = 16 real columns (re / im interleaved), the M side of
// v_mfma_f32_16x16x4_f32.  A group spans [E_g, E_g + 16 steps_g) of the tap axis, E_g a multiple of 16, zero-filled outside each
// bin's own support.  Per group and STEP of 16 taps the host stores one 1 KiB block of 64 lanes x 16 bytes: lane (kk = lane / 16,
// i = lane % 16) holds column i at taps E_g + 16 s + 4 kk + {0, 1, 2, 3}.  One coalesced 16-byte load per lane feeds FOUR matrix
// instructions: instruction m takes component m, i.e. K slot kk of instruction m is tap 4 kk + m of the step.  The waveform operand
// is read under the same permutation — lane (kk, n) takes 16 bytes at n hop + e + 4 kk — so no value is moved between lanes.
//
// Work: a unit is (row, tile of CQ_FT = 32 consecutive frames = two MFMA column tiles); the grid is persistent over units.  The tap
// axis is walked in CHUNKS of up to TC taps; a chunk's samples, (FT - 1) hop + TC of them, are staged once in LDS (reflect / zero
// padding is the index arithmetic of that load: there is no padded copy) and read by every frame that overlaps them.  Within a
// chunk every (group, step) costs the same — one bank load, two LDS reads, eight MFMAs — and the groups' supports nest, so a deal
// of whole groups to waves would leave three waves idle in the outer chunks, where only the longest group has taps.  Instead every
// wave takes every fourth STEP of every group (the tap-split the balance needs, taken to its end): each wave accumulates partial
// sums of all groups of a pass (CQ_GMAX = 16 groups = 128 bins, 128 accumulator registers), and the four partial sums are added
// through LDS, in wave order, by the wave that stores the group.  More than 128 bins take further passes over the (shorter)
// support of their own first group.
//
// LDS layout: sample a of the staged window lies at p(a) = a + 4 sk floor(a / hop).  The 16 lanes of one ds_read_b128 phase (one
// kk, n = 0 … 15) read 16 bytes at word n (hop + 4 sk) + const: they fall into 16 different 4-bank groups of the 64 banks iff
// hop / 4 + sk is odd.  sk = 0 where hop / 4 is odd, 1 where it is even: conflict-free by construction in both cases (unskewed,
// hop = 512 puts all 16 frames on the same four banks: 16-way).  hop % 4 == 0 keeps a 16-byte read inside one skew step.
//
// 0 * NaN: the zero fill of a group multiplies samples its shorter bins do not cover, so a non-finite sample inside a group's span
// reaches all 8 bins of that group for the frame; outside the group's span nothing is read.
#include "host_common.hpp"

namespace tac {

typedef float cq_f4 __attribute__((ext_vector_type(4)));
typedef float cq_f2 __attribute__((ext_vector_type(2)));

constexpr int CQ_THREADS = 256, CQ_WAVES = 4;
constexpr int CQ_FT = 32;                   // frames per unit: two 16-frame MFMA column tiles
constexpr int CQ_GROUP_BINS = 8;            // bins per group: 16 real columns
constexpr int CQ_STEP = 16;                 // taps per bank block
constexpr int CQ_GMAX = 16;                 // groups per pass (accumulators: 8 registers a group)
constexpr int CQ_TC = 2048, CQ_TC_SMALL = 512;   // taps per chunk, and where the window of CQ_TC would not fit
constexpr int CQ_LDS_FLOATS = 40960;        // 160 KB
constexpr int CQ_MIN_LDS_FLOATS = 4 * CQ_WAVES * 8 * 64;   // the reduction's scratch: 4 groups x 4 waves x 8 registers x 64 lanes
constexpr int CQ_BLOCKS_PER_CU = 2;
constexpr int CQ_MAX_HOP = 1300;            // (FT - 1)(hop + 4) + CQ_TC_SMALL + skew of the chunk's own taps <= CQ_LDS_FLOATS

// floor(u / hop) for 0 <= u < 2^16, inv = 1.0f / hop: (u + 0.5) / hop is at least 0.5 / hop away from an integer, the three float
// roundings move it by at most u 2^-22 / hop
__device__ __forceinline__ int cq_div(int u, float inv) { return (int)(((float)u + 0.5f) * inv); }

// LDS floats of the staged window of a chunk of tc taps
inline long long cq_window_floats(int hop, int tc) {
    const long long w = (long long)(CQ_FT - 1) * hop + tc;
    const int sk = ((hop / 4) & 1) ? 0 : 1;
    return w + (sk ? 4 * ((w - 4) / hop) : 0);
}

struct CqtArgs {
    const float* x;
    long long rows, length, stride_r;
    const float* bank;          // [steps][64 lanes][4]
    const int* groups;          // [n_groups][4]: E_g, steps_g, first block, bins
    int n_groups, n_bins, hop, tc, span;
    long long n_frames, tiles, origin;
    int reflect, power;
    float* out;
};

__global__ void __launch_bounds__(CQ_THREADS, 2) cqt_kernel(CqtArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kk = lane >> 4, n = lane & 15;
    const int hop = A.hop;
    const int sk = ((hop >> 2) & 1) ? 0 : 1;
    const float inv_hop = 1.0f / (float)hop;
    const long long units = A.rows * A.tiles;
    const cq_f4* bank4 = reinterpret_cast<const cq_f4*>(A.bank);

    for (long long unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const long long row = unit / A.tiles;
        const long long t0 = (unit - row * A.tiles) * CQ_FT;
        const float* xr = A.x + row * A.stride_r;

        for (int g0 = 0; g0 < A.n_groups; g0 += CQ_GMAX) {
            const int ng = A.n_groups - g0 < CQ_GMAX ? A.n_groups - g0 : CQ_GMAX;
            cq_f4 acc[CQ_GMAX][2];
#pragma unroll
            for (int gi = 0; gi < CQ_GMAX; ++gi) acc[gi][0] = acc[gi][1] = cq_f4{0.0f, 0.0f, 0.0f, 0.0f};

            // the pass's stretch of the tap axis is its first (longest) group's: the others' lie inside
            const int e_lo = A.groups[4 * g0];
            int e_hi = e_lo + CQ_STEP * A.groups[4 * g0 + 1];
            e_hi = e_hi < A.span ? e_hi : A.span;
            for (int cs = (e_lo / A.tc) * A.tc; cs < e_hi; cs += A.tc) {
                const int lo = cs > e_lo ? cs : e_lo, hi = cs + A.tc < e_hi ? cs + A.tc : e_hi;
                const int W = (CQ_FT - 1) * hop + (hi - lo);
                const long long sbase = t0 * hop + lo + A.origin;       // the sample at a = 0
                __syncthreads();                                         // (the window or the scratch is still being read)
                for (int a = 4 * tid; a < W; a += 4 * CQ_THREADS) {
                    cq_f4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        long long i = sbase + a + j;
                        if (A.reflect) i = i < 0 ? -i : (i >= A.length ? 2 * (A.length - 1) - i : i);
                        const bool in = i >= 0 && i < A.length;
                        const float s = xr[in ? i : 0];
                        v[j] = in ? s : 0.0f;
                    }
                    *reinterpret_cast<cq_f4*>(lds + a + (sk ? 4 * cq_div(a, inv_hop) : 0)) = v;
                }
                __syncthreads();

#pragma unroll
                for (int gi = 0; gi < CQ_GMAX; ++gi) {
                    if (gi < ng) {
                        const int* gp = A.groups + 4 * (g0 + gi);
                        const int E = gp[0], steps = gp[1];
                        const long long first = gp[2];
                        const int ga = E > lo ? E : lo, gb = E + CQ_STEP * steps < hi ? E + CQ_STEP * steps : hi;
                        const int s_end = (gb - E) / CQ_STEP;
                        int s = (ga - E) / CQ_STEP + w;
                        if (ga < gb && s < s_end) {
                            cq_f4 b = bank4[(first + s) * 64 + lane];
                            for (; s < s_end; s += CQ_WAVES) {
                                const int sn = s + CQ_WAVES < s_end ? s + CQ_WAVES : s;
                                const cq_f4 bn = bank4[(first + sn) * 64 + lane];      // (the next step's block, requested early)
                                const int u = E + CQ_STEP * s - lo + 4 * kk;           // the lane's four taps within the window
                                const int a0 = n * hop + u;
                                const int p0 = a0 + (sk ? 4 * (n + cq_div(u, inv_hop)) : 0);
                                const int p1 = p0 + 16 * (hop + 4 * sk);
                                const cq_f4 x0 = *reinterpret_cast<const cq_f4*>(lds + p0);
                                const cq_f4 x1 = *reinterpret_cast<const cq_f4*>(lds + p1);
#pragma unroll
                                for (int m = 0; m < 4; ++m) {
                                    acc[gi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[m], x0[m], acc[gi][0], 0, 0, 0);
                                    acc[gi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[m], x1[m], acc[gi][1], 0, 0, 0);
                                }
                                b = bn;
                            }
                        }
                    }
                }
            }

            // the four waves' partial sums of four groups at a time through LDS; wave w adds (in wave order) and stores group 4 q + w.
            // D rows 4 kk + r of column n: r = 0, 1 the pair of bin 2 kk, r = 2, 3 that of bin 2 kk + 1, frame n of the tile
#pragma unroll
            for (int q = 0; q < CQ_GMAX / 4; ++q) {
                if (4 * q < ng) {
                    __syncthreads();
#pragma unroll
                    for (int gl = 0; gl < 4; ++gl)
#pragma unroll
                        for (int r = 0; r < 8; ++r)
                            lds[((gl * CQ_WAVES + w) * 8 + r) * 64 + lane] = acc[4 * q + gl][r >> 2][r & 3];
                    __syncthreads();
                    if (4 * q + w < ng) {
                        float v[8];
#pragma unroll
                        for (int r = 0; r < 8; ++r) {
                            float sum = lds[((w * CQ_WAVES + 0) * 8 + r) * 64 + lane];
#pragma unroll
                            for (int ws = 1; ws < CQ_WAVES; ++ws) sum += lds[((w * CQ_WAVES + ws) * 8 + r) * 64 + lane];
                            v[r] = sum;
                        }
                        const int bin0 = (g0 + 4 * q + w) * CQ_GROUP_BINS + 2 * kk;
#pragma unroll
                        for (int tt = 0; tt < 2; ++tt) {
                            const long long frame = t0 + 16 * tt + n;
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                const int bin = bin0 + h;
                                if (frame < A.n_frames && bin < A.n_bins) {
                                    const float re = v[4 * tt + 2 * h], im = v[4 * tt + 2 * h + 1];
                                    const long long at = (row * A.n_bins + bin) * A.n_frames + frame;
                                    if (A.power == 0) *reinterpret_cast<cq_f2*>(A.out + 2 * at) = cq_f2{re, im};
                                    else if (A.power == 1) A.out[at] = __builtin_sqrtf(re * re + im * im);
                                    else A.out[at] = re * re + im * im;
                                }
                            }
                        }
                    }
                }
            }
        }
    }
}

}  // namespace tac

extern "C" {

int32_t tac_cqt_frames_per_tile(void) { return tac::CQ_FT; }
int32_t tac_cqt_group_bins(void) { return tac::CQ_GROUP_BINS; }
int32_t tac_cqt_step(void) { return tac::CQ_STEP; }
int32_t tac_cqt_max_hop(void) { return tac::CQ_MAX_HOP; }
int32_t tac_cqt_blocks_per_cu(void) { return tac::CQ_BLOCKS_PER_CU; }

int tac_cqt_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const float* bank, const int32_t* groups,
                int32_t n_groups, int32_t n_bins, int32_t span, int32_t hop, int64_t n_frames, int64_t origin, int reflect, int power,
                float* out, void* stream) {
    using namespace tac;
    if (!x || !bank || !groups || !out) return TAC_E_INVALID;
    if (rows <= 0 || length <= 0 || n_frames <= 0 || n_groups <= 0 || n_bins <= 0 || span <= 0 || (span % CQ_STEP) != 0)
        return TAC_E_INVALID;
    if (n_bins > n_groups * CQ_GROUP_BINS || power < 0 || power > 2) return TAC_E_INVALID;
    if (hop < 4 || (hop & 3) != 0 || hop > CQ_MAX_HOP) return TAC_E_UNSUPPORTED;
    if (span > (1 << 24) || n_frames > (1LL << 40)) return TAC_E_UNSUPPORTED;
    int tc = CQ_TC;
    if (cq_window_floats(hop, tc < span ? tc : span) > CQ_LDS_FLOATS) tc = CQ_TC_SMALL;
    long long floats = cq_window_floats(hop, tc < span ? tc : span);
    if (floats > CQ_LDS_FLOATS) return TAC_E_UNSUPPORTED;
    if (floats < CQ_MIN_LDS_FLOATS) floats = CQ_MIN_LDS_FLOATS;
    CqtArgs a;
    a.x = x; a.rows = rows; a.length = length; a.stride_r = stride_r;
    a.bank = bank; a.groups = groups; a.n_groups = n_groups; a.n_bins = n_bins; a.hop = hop; a.tc = tc; a.span = span;
    a.n_frames = n_frames; a.tiles = (n_frames + CQ_FT - 1) / CQ_FT; a.origin = origin;
    a.reflect = reflect ? 1 : 0; a.power = power; a.out = out;
    const long long units = rows * a.tiles;
    const long long blocks = persistent_blocks(units, 1, (long long)device_cu_count() * CQ_BLOCKS_PER_CU);
    return launch_kernel(cqt_kernel, blocks, CQ_THREADS, (size_t)floats * sizeof(float), (hipStream_t)stream, a);
}

}  // extern "C"
