// loudness.hip — functional.loudness / Loudness: ITU-R BS.1770-4 gated loudness (LKFS) of a waveform (…, channels, time), two launches
// behind one entry, the waveform read once.
//
//   w1 = clip(shelf(x))  w2 = clip(highpass(w1))                  the K-weighting: two biquads, each clipped to [-1, 1] as biquad() is
//   E[c][k] = mean of w2^2 over samples [k step, k step + gate)   blocks of gate = 4 step samples, 75 % overlap, nb of them
//   l_k = -0.691 + 10 log10 sum_c g_c E[c][k]                     g = (1, 1, 1, 1.41, 1.41)
//   the absolute gate keeps l_k > -70, the relative gate l_k > the level of the kept blocks' mean energy - 10; the result is the
//   level of the mean energy of the blocks both gates keep (no block: 0 / 0 = NaN)
//
// loudness_energy_kernel   A row (one channel of one entry) is walked from its start by ONE workgroup in tiles of LO_TILE = 1024 *
//                          LO_C consecutive samples, lane l owning samples [l C, l C + C) of the tile.  Per tile and per stage the
//                          recursion runs as in lfilter.hip: the chunk from zero state, a Kogge-Stone scan of the end states over the
//                          host-computed powers M^(C 2^i) — six steps in a wave, four across the sixteen waves through the LDS — the
//                          previous tile's carry entering by linearity, then the chunk again from its true incoming state.  State,
//                          scan and the stage outputs are float64: the shelf's output is clipped IN float64, stays in registers (the
//                          neighbour's last two values come by a cross-lane move, a wave's by the LDS) and feeds the high-pass, whose
//                          clipped float64 output is squared and summed.  Nothing between the float32 load and the sums is rounded
//                          to float32 and nothing but the sums leaves the workgroup.
//                          The sums are bins of `step` consecutive samples (a block is four bins).  A bin edge falls anywhere in a
//                          lane's chunk (step >= C: at most one per chunk), so a lane forms the sum in front of the edge and the sum
//                          behind it, in ascending order; a segmented Kogge-Stone scan joins the lanes of a wave (a bin that ends in
//                          a lane is complete there but for what earlier waves hold); the waves' open sums are joined in ascending
//                          order through the LDS, and a bin open at the end of a tile is carried to the next one like the filter
//                          state.  One writer per bin, no atomics, a fixed order: bit-identical from run to run.  Only the nb + 3
//                          bins some block reads are written — float64 [rows][nb + 3] — and the samples behind the last block are
//                          not read.
// loudness_gate_kernel     a wave per entry: lane l takes blocks l, l + 64, … in ascending order, then a butterfly of xor
//                          shuffles.  Block energies (four bins / gate), the channel weights, l_k, both gates and the result are
//                          float64, log10 included; a block is gated by MULTIPLYING its energy by 0 or 1, so a NaN energy makes the
//                          entry NaN as the definition does.  The result is rounded to float32 once.  No host wait between the two.
//
// Nothing is shared between rows or entries and a lane's incoming state depends on earlier samples only: a non-finite sample
// reaches its own entry and nothing else.
#include <math.h>

#include "host_common.hpp"

namespace tac {

typedef float lo_f4 __attribute__((ext_vector_type(4)));

constexpr int LO_C_LOG = 4;
constexpr int LO_C = 1 << LO_C_LOG;             // samples per lane
constexpr int LO_THREADS = 1024;
constexpr int LO_WAVES = LO_THREADS / 64;
constexpr int LO_TILE = LO_THREADS * LO_C;      // samples per tile
constexpr int LO_XS = LO_TILE + LO_TILE / LO_C + 1;
constexpr int LO_STEPS = 10;                    // log2(LO_THREADS): M^(C 2^i), i < 10
constexpr int LO_MAX_CHANNELS = 5;
static_assert(LO_WAVES == 16 && (1 << LO_STEPS) == LO_THREADS, "the scans are six steps in a wave and four across sixteen waves");

struct LoMat { double a, b, c, d; };            // [[a, b], [c, d]]
struct LoStage {
    double b0, b1, b2, a1, a2;
    LoMat p[LO_STEPS];                          // p[i] = M^(C 2^i)
};
struct LoParams { LoStage s[2]; };              // the shelf, the high-pass

// LDS of the energy kernel, in doubles from its base; the float part (carry_x, xs) lies behind
constexpr int LO_D_WAVE_STATE = 0;                              // [2][16][2]: the waves' own end states, and scanned
constexpr int LO_D_CARRY = LO_D_WAVE_STATE + 4 * LO_WAVES;      // [2][2]: the filter state at the end of the tile, per stage
constexpr int LO_D_CARRY_Y = LO_D_CARRY + 4;                    // [2]: the last two clipped shelf outputs of the tile
constexpr int LO_D_TAIL = LO_D_CARRY_Y + 2;                     // [16][2]: the last two clipped shelf outputs of each wave
constexpr int LO_D_OPEN = LO_D_TAIL + 2 * LO_WAVES;             // [16]: the sum of the bin open at the end of each wave
constexpr int LO_D_CARRY_BIN = LO_D_OPEN + LO_WAVES;            // [2]: ... and at the end of the tile, by tile parity
constexpr int LO_D_CLOSED = LO_D_CARRY_BIN + 2;                 // [16] ints in 8 doubles: whether a bin ends in the wave
constexpr int LO_D_END = LO_D_CLOSED + LO_WAVES / 2;
constexpr size_t LO_LDS_BYTES = LO_D_END * sizeof(double) + (4 + LO_XS) * sizeof(float);

__device__ __forceinline__ int lo_at(int i) { return i + (i >> LO_C_LOG); }

__device__ __forceinline__ void lo_apply(const LoMat& m, double u0, double u1, double& s0, double& s1) {
    s0 += m.a * u0 + m.b * u1;
    s1 += m.c * u0 + m.d * u1;
}

__device__ __forceinline__ double lo_clip(double y) { return y < -1.0 ? -1.0 : (y > 1.0 ? 1.0 : y); }      // (a NaN stays a NaN)

// The state (y[c0 - 1], y[c0 - 2]) the lane's chunk starts from, given the chunk's feed-forward part v and the state (in0, in1) the
// TILE starts from (used by thread 0 alone): lfilter.hip's pass 1 and scan.  Two barriers.
__device__ __forceinline__ void lo_incoming(const LoStage& P, const double (&v)[LO_C], double (*wave_state)[LO_WAVES][2], int tid,
                                            double& in0, double& in1) {
    const int lane = tid & 63, wave = tid >> 6;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k < LO_C; ++k) {
        const double y = fma(-P.a1, s0, fma(-P.a2, s1, v[k]));
        s1 = s0;
        s0 = y;
    }
    if (tid == 0) lo_apply(P.p[0], in0, in1, s0, s1);           // the previous tile's carry, by linearity (zero in tile 0)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double u0 = __shfl_up(s0, 1 << i), u1 = __shfl_up(s1, 1 << i);
        if (lane >= (1 << i)) lo_apply(P.p[i], u0, u1, s0, s1);
    }
    double e0 = __shfl_up(s0, 1), e1 = __shfl_up(s1, 1);         // the wave-local state before the lane's chunk
    if (lane == 0) e0 = e1 = 0.0;
    if (lane == 63) {
        wave_state[0][wave][0] = s0;
        wave_state[0][wave][1] = s1;
    }
    __syncthreads();
    if (wave == 0) {
        double w0 = lane < LO_WAVES ? wave_state[0][lane][0] : 0.0;
        double w1 = lane < LO_WAVES ? wave_state[0][lane][1] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double u0 = __shfl_up(w0, 1 << i), u1 = __shfl_up(w1, 1 << i);
            if (lane >= (1 << i)) lo_apply(P.p[6 + i], u0, u1, w0, w1);
        }
        if (lane < LO_WAVES) {
            wave_state[1][lane][0] = w0;
            wave_state[1][lane][1] = w1;
        }
    }
    __syncthreads();
    if (tid > 0) {
        in0 = e0;
        in1 = e1;
    }
    if (wave > 0) {             // the state at the end of the previous wave, carried over the lane's `lane` chunks
        double u0 = wave_state[1][wave - 1][0], u1 = wave_state[1][wave - 1][1];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if ((lane >> i) & 1) {
                double m0 = 0.0, m1 = 0.0;
                lo_apply(P.p[i], u0, u1, m0, m1);
                u0 = m0;
                u1 = m1;
            }
        }
        in0 += u0;
        in1 += u1;
    }
}

// Row r is channel r % channels of entry r / channels: it starts at (r / channels) stride_b + (r % channels) stride_c, unit time
// stride.  used = nbins * step samples of it are read; bins: float64 [rows][nbins].
template <bool VEC>
__global__ void __launch_bounds__(LO_THREADS)
loudness_energy_kernel(const float* __restrict__ x, long long rows, int channels, long long stride_b, long long stride_c,
                       long long used, long long step, long long nbins, LoParams P, double* __restrict__ bins) {
    extern __shared__ __attribute__((aligned(16))) double lo_lds[];
    double (*wave_state)[LO_WAVES][2] = reinterpret_cast<double (*)[LO_WAVES][2]>(lo_lds + LO_D_WAVE_STATE);
    double (*carry_state)[2] = reinterpret_cast<double (*)[2]>(lo_lds + LO_D_CARRY);
    double* carry_y = lo_lds + LO_D_CARRY_Y;
    double (*wave_tail)[2] = reinterpret_cast<double (*)[2]>(lo_lds + LO_D_TAIL);
    double* wave_open = lo_lds + LO_D_OPEN;
    double* carry_bin = lo_lds + LO_D_CARRY_BIN;
    int* wave_closed = reinterpret_cast<int*>(lo_lds + LO_D_CLOSED);
    float* carry_x = reinterpret_cast<float*>(lo_lds + LO_D_END);
    float* xs = carry_x + 4;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int c0 = tid * LO_C;                          // the lane's first sample within the tile
    const long long tiles = (used + LO_TILE - 1) / LO_TILE;

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* src = x + (row / channels) * stride_b + (row % channels) * stride_c;
        double* dst = bins + row * nbins;
        for (long long t = 0; t < tiles; ++t) {
            const long long n0 = t * LO_TILE;
            const int nt = (int)(used - n0 < LO_TILE ? used - n0 : LO_TILE);
            // the last two clipped shelf outputs of the previous tile, before this tile's are written
            double ym1 = 0.0, ym2 = 0.0;
            if (tid == 0 && t > 0) {
                ym1 = carry_y[0];
                ym2 = carry_y[1];
            }
            // ---- global -> xs
            if constexpr (VEC) {
                for (int q = tid; q < ((nt + 3) >> 2); q += LO_THREADS) {       // (n0 is a multiple of the tile: chunks stay aligned)
                    const long long g = n0 + 4 * q;
                    lo_f4 v;
                    if (g + 3 < used) {
                        v = *reinterpret_cast<const lo_f4*>(src + g);
                    } else {
                        v.x = g < used ? src[g] : 0.0f;
                        v.y = g + 1 < used ? src[g + 1] : 0.0f;
                        v.z = g + 2 < used ? src[g + 2] : 0.0f;
                        v.w = 0.0f;
                    }
                    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int j = 4 * q + k;
                        if (j < nt) xs[lo_at(j)] = e[k];
                    }
                }
            } else {
                for (int j = tid; j < nt; j += LO_THREADS) xs[lo_at(j)] = src[n0 + j];
            }
            __syncthreads();

            // ---- the shelf: the lane's chunk and the two samples before it (zero before the row and behind the samples read)
            double v[LO_C];
            double in0 = 0.0, in1 = 0.0;
            {
                float xr[LO_C];
#pragma unroll
                for (int k = 0; k < LO_C; ++k) xr[k] = c0 + k < nt ? xs[lo_at(c0 + k)] : 0.0f;
                float xm1 = 0.0f, xm2 = 0.0f;
                if (tid > 0) {
                    if (c0 - 1 < nt) xm1 = xs[lo_at(c0 - 1)];
                    if (c0 - 2 < nt) xm2 = xs[lo_at(c0 - 2)];
                } else if (t > 0) {
                    xm1 = carry_x[0];
                    xm2 = carry_x[1];
                    in0 = carry_state[0][0];
                    in1 = carry_state[0][1];
                }
                const LoStage& S = P.s[0];
#pragma unroll
                for (int k = 0; k < LO_C; ++k) {
                    const float p1 = k >= 1 ? xr[k - 1] : xm1;
                    const float p2 = k >= 2 ? xr[k - 2] : (k == 1 ? xm1 : xm2);
                    v[k] = fma(S.b2, (double)p2, fma(S.b1, (double)p1, S.b0 * (double)xr[k]));
                }
                lo_incoming(S, v, wave_state, tid, in0, in1);
#pragma unroll
                for (int k = 0; k < LO_C; ++k) {
                    const double y = fma(-S.a1, in0, fma(-S.a2, in1, v[k]));
                    in1 = in0;
                    in0 = y;
                    v[k] = lo_clip(y);                  // the state goes on unclipped, as lfilter's does
                }
                if (tid == LO_THREADS - 1) {            // read by thread 0 in the next tile, behind the barriers in between
                    carry_state[0][0] = in0;
                    carry_state[0][1] = in1;
                    carry_x[0] = xr[LO_C - 1];
                    carry_x[1] = xr[LO_C - 2];
                    carry_y[0] = v[LO_C - 1];
                    carry_y[1] = v[LO_C - 2];
                }
            }

            // ---- the high-pass on the clipped float64 values: the neighbour's last two by a cross-lane move, a wave's by the LDS
            {
                const double n1 = __shfl_up(v[LO_C - 1], 1), n2 = __shfl_up(v[LO_C - 2], 1);
                if (lane == 63) {
                    wave_tail[wave][0] = v[LO_C - 1];
                    wave_tail[wave][1] = v[LO_C - 2];
                }
                __syncthreads();
                if (lane > 0) {
                    ym1 = n1;
                    ym2 = n2;
                } else if (wave > 0) {
                    ym1 = wave_tail[wave - 1][0];
                    ym2 = wave_tail[wave - 1][1];
                }
                const LoStage& S = P.s[1];
                in0 = in1 = 0.0;
                if (tid == 0 && t > 0) {
                    in0 = carry_state[1][0];
                    in1 = carry_state[1][1];
                }
#pragma unroll
                for (int k = LO_C - 1; k >= 0; --k) {   // in place, from the end: v[k - 1] and v[k - 2] are still the shelf's
                    const double p1 = k >= 1 ? v[k - 1] : ym1;
                    const double p2 = k >= 2 ? v[k - 2] : (k == 1 ? ym1 : ym2);
                    v[k] = fma(S.b2, p2, fma(S.b1, p1, S.b0 * v[k]));
                }
                lo_incoming(S, v, wave_state, tid, in0, in1);
#pragma unroll
                for (int k = 0; k < LO_C; ++k) {
                    const double y = fma(-S.a1, in0, fma(-S.a2, in1, v[k]));
                    in1 = in0;
                    in0 = y;
                    const double w = lo_clip(y);
                    v[k] = c0 + k < nt ? w * w : 0.0;   // (nothing behind the samples read reaches a sum)
                }
                if (tid == LO_THREADS - 1) {
                    carry_state[1][0] = in0;
                    carry_state[1][1] = in1;
                }
            }

            // ---- bins: the lane's sum in front of the bin edge in its chunk (bin q0) and behind it (bin q0 + 1)
            const long long g0 = n0 + c0;
            const long long q0 = g0 / step;
            const long long to_edge = (q0 + 1) * step - g0;     // 1 .. step samples of the chunk's first bin are left
            const int closes = to_edge <= LO_C;                 // bin q0 ends in this chunk (step >= LO_C: no second one does)
            const int split = closes ? (int)to_edge : LO_C;
            double front = 0.0, behind = 0.0;
#pragma unroll
            for (int k = 0; k < LO_C; ++k) {
                if (k < split) front += v[k];
                else behind += v[k];
            }
            // segmented scan: s = the sum of the bin open at the end of the lane, over the lanes of the wave it has crossed
            double s = closes ? behind : front;
            int f = closes;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double u = __shfl_up(s, 1 << i);
                const int uf = __shfl_up(f, 1 << i);
                if (lane >= (1 << i)) {
                    if (!f) s += u;
                    f |= uf;
                }
            }
            double before = __shfl_up(s, 1);                    // ... at the end of the lane in front
            if (lane == 0) before = 0.0;
            const unsigned long long closing = __ballot(closes);
            const int first = closing ? __ffsll((long long)closing) - 1 : 64;
            if (lane == 63) {
                wave_open[wave] = s;
                wave_closed[wave] = closing != 0ULL;
            }
            double total = before + front;                      // bin q0, as far as this wave holds it
            if (closes && lane != first && q0 < nbins) dst[q0] = total;
            __syncthreads();
            // what the waves in front hold of the bin open at the start of this wave, in ascending order, behind the tile's carry
            if ((closes && lane == first) || tid == LO_THREADS - 1) {
                double r = t > 0 ? carry_bin[t & 1] : 0.0;
                for (int w = 0; w < wave; ++w) r = wave_closed[w] ? wave_open[w] : r + wave_open[w];
                if (closes && lane == first && q0 < nbins) dst[q0] = r + total;
                if (tid == LO_THREADS - 1) carry_bin[(t + 1) & 1] = closing ? s : r + s;
            }
        }
        __syncthreads();                                        // (the next row's first tile shares no LDS word with this one's end)
    }
}

__device__ __forceinline__ double lo_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// block k of an entry: the channels' energies e[c] and the block's level
__device__ __forceinline__ double lo_block(const double* __restrict__ b, int channels, long long nbins, long long k, double gate,
                                           double (&e)[LO_MAX_CHANNELS]) {
    const double weight[LO_MAX_CHANNELS] = {1.0, 1.0, 1.0, 1.41, 1.41};
    double z = 0.0;
#pragma unroll
    for (int c = 0; c < LO_MAX_CHANNELS; ++c) {
        e[c] = 0.0;
        if (c < channels) {
            const double* p = b + c * nbins + k;
            e[c] = (((p[0] + p[1]) + p[2]) + p[3]) / gate;
            z += weight[c] * e[c];
        }
    }
    return -0.691 + 10.0 * log10(z);
}

__device__ __forceinline__ double lo_level(const double (&sum)[LO_MAX_CHANNELS], double count) {
    const double weight[LO_MAX_CHANNELS] = {1.0, 1.0, 1.0, 1.41, 1.41};
    double z = 0.0;
#pragma unroll
    for (int c = 0; c < LO_MAX_CHANNELS; ++c) z += weight[c] * (sum[c] / count);      // (a channel that is not there: 0 / count)
    return -0.691 + 10.0 * log10(z);
}

__global__ void __launch_bounds__(64)
loudness_gate_kernel(const double* __restrict__ bins, long long entries, int channels, long long nb, double gate,
                     float* __restrict__ out) {
    const int lane = threadIdx.x;
    const long long nbins = nb + 3;
    for (long long entry = blockIdx.x; entry < entries; entry += gridDim.x) {
        const double* b = bins + entry * channels * nbins;
        double gamma = -70.0, level = 0.0;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {                  // the absolute gate, then both
            double sum[LO_MAX_CHANNELS] = {0.0, 0.0, 0.0, 0.0, 0.0}, count = 0.0;
            for (long long k = lane; k < nb; k += 64) {
                double e[LO_MAX_CHANNELS];
                const double l = lo_block(b, channels, nbins, k, gate, e);
                const double keep = (l > -70.0 && (pass == 0 || l > gamma)) ? 1.0 : 0.0;
                count += keep;
#pragma unroll
                for (int c = 0; c < LO_MAX_CHANNELS; ++c) sum[c] += keep * e[c];    // (0 * NaN: a NaN block makes the entry NaN)
            }
            count = lo_wave_sum(count);
#pragma unroll
            for (int c = 0; c < LO_MAX_CHANNELS; ++c) sum[c] = lo_wave_sum(sum[c]);
            level = lo_level(sum, count);
            gamma = level - 10.0;
        }
        if (lane == 0) out[entry] = (float)level;
    }
}

inline LoMat lo_mul(const LoMat& x, const LoMat& y) {
    return LoMat{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}

// b[3], a[3] normalised by a[0] and the ten powers; TAC_E_INVALID for a zero a[0] or a non-finite coefficient, TAC_E_UNSUPPORTED
// where one of the powers is not finite
inline int lo_stage(const double* b, const double* a, LoStage* S) {
    if (!(a[0] != 0.0) || !isfinite(a[0])) return TAC_E_INVALID;
    double bn[3], an[3];
    for (int k = 0; k < 3; ++k) {
        bn[k] = b[k] / a[0];
        an[k] = a[k] / a[0];
        if (!isfinite(bn[k]) || !isfinite(an[k])) return TAC_E_INVALID;
    }
    S->b0 = bn[0], S->b1 = bn[1], S->b2 = bn[2], S->a1 = an[1], S->a2 = an[2];
    const LoMat m{-an[1], -an[2], 1.0, 0.0};
    LoMat q = m;
    for (int k = 1; k < LO_C; ++k) q = lo_mul(q, m);
    for (int i = 0; i < LO_STEPS; ++i) {
        if (!isfinite(q.a) || !isfinite(q.b) || !isfinite(q.c) || !isfinite(q.d)) return TAC_E_UNSUPPORTED;
        S->p[i] = q;
        q = lo_mul(q, q);
    }
    return TAC_OK;
}

// blocks of `gate` samples every `step` in `length`, or 0
inline long long lo_blocks(long long length, long long gate, long long step) {
    return (gate <= 0 || step <= 0 || length < gate) ? 0 : (length - gate) / step + 1;
}

}  // namespace tac

extern "C" {

int64_t tac_loudness_tile(void) { return tac::LO_TILE; }

int64_t tac_loudness_work_bytes(int64_t entries, int32_t channels, int64_t length, int64_t gate, int64_t step) {
    const long long nb = tac::lo_blocks(length, gate, step);
    if (entries <= 0 || channels < 1 || channels > tac::LO_MAX_CHANNELS || nb <= 0 || gate != 4 * step || step < tac::LO_C) return 0;
    return (int64_t)sizeof(double) * entries * channels * (nb + 3);
}

int tac_loudness_f32(const float* waveform, int64_t entries, int32_t channels, int64_t length, int64_t stride_b, int64_t stride_c,
                     int64_t gate, int64_t step, const double* coeffs, void* work, float* out, void* stream) {
    using namespace tac;
    if (!waveform || !coeffs || !work || !out || entries <= 0 || channels < 1 || channels > LO_MAX_CHANNELS || length <= 0 ||
        gate <= 0 || step <= 0)
        return TAC_E_INVALID;
    if (length < gate) return TAC_E_SHORT_INPUT;
    if (gate != 4 * step || step < LO_C) return TAC_E_UNSUPPORTED;
    if (entries == 1) stride_b = 0;
    if (channels == 1) stride_c = 0;
    if ((entries > 1 && stride_b <= 0) || (channels > 1 && stride_c <= 0)) return TAC_E_INVALID;
    LoParams P;
    for (int i = 0; i < 2; ++i) {
        const int rc = lo_stage(coeffs + 6 * i, coeffs + 6 * i + 3, &P.s[i]);
        if (rc != TAC_OK) return rc;
    }
    const long long nb = lo_blocks(length, gate, step), nbins = nb + 3;
    const long long rows = (long long)entries * channels;
    const bool vec = (reinterpret_cast<uintptr_t>(waveform) & 15) == 0 && (stride_b & 3) == 0 && (stride_c & 3) == 0;
    double* bins = static_cast<double*>(work);
    // 69 KiB of LDS and more than 64 registers a lane: one workgroup of sixteen waves per CU
    const long long blocks = persistent_blocks(rows, 1, (long long)device_cu_count());
    int rc = launch_kernel(vec ? loudness_energy_kernel<true> : loudness_energy_kernel<false>, blocks, LO_THREADS, LO_LDS_BYTES,
                           (hipStream_t)stream, waveform, rows, (int)channels, (long long)stride_b, (long long)stride_c, nbins * step,
                           (long long)step, nbins, P, bins);
    if (rc != TAC_OK) return rc;
    const long long gate_blocks = persistent_blocks(entries, 1, (long long)device_cu_count() * 8);
    return launch_kernel(loudness_gate_kernel, gate_blocks, 64, 0, (hipStream_t)stream, (const double*)bins, (long long)entries,
                         (int)channels, nb, (double)gate, out);
}

}  // extern "C"
