// sox_effects.hip — functional.overdrive / phaser / flanger: the three SoX effects whose definition is a loop over time, each in
// ONE launch.  float32 is read once and written once; everything between is float64 on chip and rounded once.
//
//   overdrive   t = shape(g x + c);  v[n] = t[n] - t[n-1] + 0.995 v[n-1];  out = clamp(0.5 x + 0.75 v)
//               lfilter.hip's tile walk: a row belongs to ONE workgroup, which walks it in tiles of OD_TILE = 1024 * OD_C samples;
//               lane l owns samples [l C, l C + C).  The shaping runs on load, pass 1 gives the chunk's zero-state end value, a
//               Kogge-Stone scan over the SCALAR powers a^(C 2^i) (six steps in the wave by cross-lane moves, then the sixteen
//               wave values through the LDS, scanned by every wave for itself) gives the state the chunk starts from, pass 2
//               runs the chunk from it, and 0.5 x + 0.75 v and the clamp run on store.  The last v and the last t of a tile are
//               carried to lane 0 of the next one (two copies by the tile's parity).
//
//   phaser      y[n] = gain_in x[n] + decay y[n - d(n)],  d(n) = L - m[n mod P] + 1 in [1, L];  out = clamp(gain_out y)
//               every sample has ONE parent.  A workgroup walks a row in tiles of PH_TILE samples held in the LDS as
//               (value, coefficient, parent) triples and jumps pointers in float64:
//                   value[j] += coefficient[j] value[parent[j]];  coefficient[j] *= coefficient[parent[j]];  parent[j] = parent[parent[j]]
//               for every j whose parent lies inside the tile, all reads of a round before a barrier and all writes behind it,
//               until no parent lies inside (at most log2(PH_TILE) + 1 rounds; the round's barrier also carries the vote).
//               What is left is coefficient[j] y[parent[j]] with the parent among the last L samples of the previous tile, which
//               stay in the LDS.  phaser_seq_kernel is the obvious alternative kept for the ablation: one LANE per row, the
//               recursion run sample by sample over a ring of L doubles per lane.
//
//   flanger     w[i] = x[i] + fb delayed[i-1];  delayed[i] = interpolation of w[i-k], w[i-k-1] (, w[i-k-2]) at D = lfo[(i + phi_c) mod P],
//               k = floor(D), fr = D - k;  out = clamp(in_gain x + delay_gain delayed)
//               fb == 0: w = x, a time-varying FIR of two or three taps.  (row, tile) units over a persistent grid; a unit stages its
//               tile and the Lb samples before it in the LDS.
//               fb != 0: a wave per row, w in an LDS ring of doubles.  delayed[i-1] reaches back at least 1 + tmin samples, so the
//               W = min(64, 1 + tmin) slots [s, s + W) need only w before s: lane j takes slot s + j, computes delayed[i-1] from the
//               ring, stores out[i-1] and then w[i]; one barrier per step.  x, the lfo values and out are staged by the whole wave
//               in chunks of FL_CHUNK samples.  W = 1 (delay = 0) is one sample per step: latency-bound by construction.
//               In the quadratic form the tap k + 2 == Lb wraps onto w[i] itself; that happens only with fr == 0, where its
//               weight is exactly zero, and it is left out.
//
// Nothing is shared between rows and values move to later samples only: a non-finite sample reaches nothing in another row and
// nothing before it in its own.  No atomics, no workspace, one writer per element: bit-identical from run to run.
// (The tile geometry and the 16-byte loads restate lfilter.hip's under names of their own: that file's text is pinned by
// tests/grid_rules.py and stays as it is.)
#include <math.h>

#include "host_common.hpp"

namespace tac {

typedef float sx_f4 __attribute__((ext_vector_type(4)));

// global -> LDS for `count` samples that start at row offset p0 (p0 >= 0, p0 + count <= length): 16 bytes per lane where the row
// is aligned (VEC), a float per lane otherwise.  put(j, value) stores sample p0 + j.
template <bool VEC, int THREADS, class Put>
__device__ __forceinline__ void sx_load(const float* __restrict__ src, long long length, long long p0, int count, int tid, Put put) {
    if constexpr (VEC) {
        const long long a0f = p0 & ~3LL;
        const int lead = (int)(p0 - a0f);
        for (int q = tid; q < ((lead + count + 3) >> 2); q += THREADS) {
            const long long g = a0f + 4 * q;
            sx_f4 v;
            if (g + 3 < length) {
                v = *reinterpret_cast<const sx_f4*>(src + g);
            } else {
                v.x = g < length ? src[g] : 0.0f;
                v.y = g + 1 < length ? src[g + 1] : 0.0f;
                v.z = g + 2 < length ? src[g + 2] : 0.0f;
                v.w = 0.0f;
            }
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 4 * q + k - lead;
                if (j >= 0 && j < count) put(j, e[k]);
            }
        }
    } else {
        for (int j = tid; j < count; j += THREADS) put(j, src[p0 + j]);
    }
}

__device__ __forceinline__ float sx_clamp(double v) {
    const float f = (float)v;
    return f < -1.0f ? -1.0f : (f > 1.0f ? 1.0f : f);          // (a NaN stays a NaN)
}

// ============================================================================= overdrive
constexpr int OD_C_LOG = 4;
constexpr int OD_C = 1 << OD_C_LOG;             // samples per lane
constexpr int OD_THREADS = 1024;
constexpr int OD_WAVES = OD_THREADS / 64;
constexpr int OD_TILE = OD_THREADS * OD_C;
constexpr int OD_XS = OD_TILE + OD_TILE / OD_C + 1;
constexpr int OD_STEPS = 10;                    // a^(C 2^i), i < 10
constexpr int OD_BLOCKS_PER_CU = 2;
constexpr double OD_A = 0.995;
static_assert(OD_WAVES == 16 && (1 << OD_STEPS) == OD_THREADS, "the scan is six steps in a wave and four across sixteen waves");

struct OdParams {
    double g, c;
    double p[OD_STEPS];                         // 0.995^(C 2^i)
};

__device__ __forceinline__ int od_at(int i) { return i + (i >> OD_C_LOG); }     // xs is skewed by one float per chunk

__device__ __forceinline__ double od_shape(float x, double g, double c) {
    const double t = g * (double)x + c;
    if (t < -1.0) return -2.0 / 3.0;
    if (t > 1.0) return 2.0 / 3.0;
    return t - t * t * t / 3.0;                 // (a NaN takes this branch and stays one)
}

constexpr int OD_HEAD = OD_WAVES + 4;           // doubles in front of xs: wave_state[16] | hist[2][2] (last v, last t)

template <bool VEC>
__global__ void __launch_bounds__(OD_THREADS)
overdrive_kernel(const float* __restrict__ x, long long rows, long long length, long long stride_r, OdParams P,
                 float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double od_lds[];
    double* wave_state = od_lds;
    double (*hist)[2] = reinterpret_cast<double (*)[2]>(od_lds + OD_WAVES);
    float* xs = reinterpret_cast<float*>(od_lds + OD_HEAD);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int c0 = tid * OD_C;
    const long long tiles = (length + OD_TILE - 1) / OD_TILE;

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* src = x + row * stride_r;
        float* dst = out + row * length;
        for (long long t = 0; t < tiles; ++t) {
            const long long n0 = t * OD_TILE;
            const int nt = (int)(length - n0 < OD_TILE ? length - n0 : OD_TILE);
            const int cur = (int)(t & 1);
            sx_load<VEC, OD_THREADS>(src, length, n0, nt, tid, [&](int j, float v) { xs[od_at(j)] = v; });
            __syncthreads();

            // ---- the shaping on load: the lane's chunk of t, and t just before it (zero before the row)
            double v[OD_C];
#pragma unroll
            for (int k = 0; k < OD_C; ++k) v[k] = c0 + k < nt ? od_shape(xs[od_at(c0 + k)], P.g, P.c) : 0.0;
            double tprev = 0.0, in = 0.0;
            if (tid > 0) {
                if (c0 - 1 < nt) tprev = od_shape(xs[od_at(c0 - 1)], P.g, P.c);
            } else if (t > 0) {
                in = hist[cur ^ 1][0];
                tprev = hist[cur ^ 1][1];
            }
            if (tid == OD_THREADS - 1) hist[cur][1] = v[OD_C - 1];
            // ---- u[k] = t[k] - t[k - 1], in place from the last sample down
#pragma unroll
            for (int k = OD_C - 1; k >= 0; --k) v[k] -= k >= 1 ? v[k - 1] : tprev;
            // ---- pass 1: the chunk's end value from zero state
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < OD_C; ++k) s = fma(OD_A, s, v[k]);
            if (tid == 0) s = fma(P.p[0], in, s);           // the previous tile's carry, by linearity (zero in tile 0)
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double u = __shfl_up(s, 1 << i);
                if (lane >= (1 << i)) s = fma(P.p[i], u, s);
            }
            double e = __shfl_up(s, 1);                     // the wave-local state before the lane's chunk
            if (lane == 0) e = 0.0;
            if (lane == 63) wave_state[wave] = s;
            __syncthreads();
            double w = lane < OD_WAVES ? wave_state[lane] : 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double u = __shfl_up(w, 1 << i);
                if (lane >= (1 << i)) w = fma(P.p[6 + i], u, w);
            }
            double u = __shfl(w, wave > 0 ? wave - 1 : 0);
            if (tid > 0) in = e;
            if (wave > 0) {                                 // the previous wave's end state over the lane's `lane` chunks
#pragma unroll
                for (int i = 0; i < 6; ++i)
                    if ((lane >> i) & 1) u *= P.p[i];
                in += u;
            }
            // ---- pass 2 from the true incoming state; 0.5 x + 0.75 v and the clamp on store
#pragma unroll
            for (int k = 0; k < OD_C; ++k) {
                in = fma(OD_A, in, v[k]);
                v[k] = in;
            }
            if (tid == OD_THREADS - 1) hist[cur][0] = v[OD_C - 1];
#pragma unroll
            for (int k = 0; k < OD_C; ++k)
                if (c0 + k < nt) xs[od_at(c0 + k)] = sx_clamp(0.5 * (double)xs[od_at(c0 + k)] + 0.75 * v[k]);
            __syncthreads();
            for (int j = tid; j < nt; j += OD_THREADS) dst[n0 + j] = xs[od_at(j)];
            __syncthreads();
        }
    }
}

inline int od_params(double g, double c, OdParams* P) {
    if (!isfinite(g) || !isfinite(c)) return TAC_E_INVALID;
    P->g = g;
    P->c = c;
    double q = 1.0;
    for (int k = 0; k < OD_C; ++k) q *= OD_A;
    for (int i = 0; i < OD_STEPS; ++i) {
        P->p[i] = q;
        q *= q;
    }
    return TAC_OK;
}

// ============================================================================= phaser
constexpr int PH_THREADS = 1024;
constexpr int PH_K = 4;                         // samples per thread, interleaved: j = tid + PH_THREADS q
constexpr int PH_TILE = PH_THREADS * PH_K;
constexpr int PH_MAX_L = 1024;                  // delay samples the carry area holds (5 ms at 204.8 kHz)
constexpr int PH_BLOCKS_PER_CU = 1;             // 88 KB of LDS and 16 waves per workgroup
constexpr size_t PH_LDS = (size_t)PH_TILE * (2 * sizeof(double) + sizeof(int)) + PH_MAX_L * sizeof(double);
static_assert(PH_MAX_L <= PH_TILE && PH_LDS <= 160 * 1024, "the carry comes from one tile; everything fits the LDS");

template <bool VEC>
__global__ void __launch_bounds__(PH_THREADS)
phaser_kernel(const float* __restrict__ x, long long rows, long long length, long long stride_r, const int* __restrict__ mod,
              int P, int L, double gain_in, double decay, double gain_out, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double ph_lds[];
    double* val = ph_lds;
    double* coef = ph_lds + PH_TILE;
    double* prev = ph_lds + 2 * PH_TILE;                    // y of the L samples before the tile
    int* par = reinterpret_cast<int*>(ph_lds + 2 * PH_TILE + PH_MAX_L);
    const int tid = threadIdx.x;
    const long long tiles = (length + PH_TILE - 1) / PH_TILE;

    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* src = x + row * stride_r;
        float* dst = out + row * length;
        for (long long t = 0; t < tiles; ++t) {
            const long long n0 = t * PH_TILE;
            const int nt = (int)(length - n0 < PH_TILE ? length - n0 : PH_TILE);
            const unsigned m0 = (unsigned)(n0 % P);
            sx_load<VEC, PH_THREADS>(src, length, n0, nt, tid, [&](int j, float v) { val[j] = gain_in * (double)v; });
#pragma unroll
            for (int q = 0; q < PH_K; ++q) {
                const int j = tid + PH_THREADS * q;
                if (j < nt) {
                    int d = L - mod[(m0 + (unsigned)j) % (unsigned)P] + 1;
                    d = d < 1 ? 1 : (d > L ? L : d);
                    coef[j] = decay;
                    par[j] = j - d;
                }
            }
            __syncthreads();
            // ---- pointer jumping: every read of a round before its barrier, every write behind it
            for (;;) {
                double nv[PH_K], nc[PH_K];
                int np[PH_K];
                int any = 0;
#pragma unroll
                for (int q = 0; q < PH_K; ++q) {
                    const int j = tid + PH_THREADS * q;
                    np[q] = -1;
                    nv[q] = nc[q] = 0.0;
                    if (j < nt) {
                        const int p = par[j];
                        if (p >= 0) {
                            const double c = coef[j];
                            nv[q] = fma(c, val[p], val[j]);
                            nc[q] = c * coef[p];
                            np[q] = par[p];
                            any = 1;
                        } else {
                            np[q] = -1 - PH_TILE;           // nothing to write
                        }
                    }
                }
                if (!__syncthreads_or(any)) break;
#pragma unroll
                for (int q = 0; q < PH_K; ++q) {
                    const int j = tid + PH_THREADS * q;
                    if (j < nt && np[q] != -1 - PH_TILE) {
                        val[j] = nv[q];
                        coef[j] = nc[q];
                        par[j] = np[q];
                    }
                }
                __syncthreads();
            }
            // ---- the part that comes from before the tile, gain_out and the clamp on store
#pragma unroll
            for (int q = 0; q < PH_K; ++q) {
                const int j = tid + PH_THREADS * q;
                if (j < nt) {
                    double y = val[j];
                    const int p = par[j];                   // in [-L, -1]
                    if (n0 + p >= 0) y = fma(coef[j], prev[L + p], y);
                    val[j] = y;
                    dst[n0 + j] = sx_clamp(gain_out * y);
                }
            }
            __syncthreads();
            if (nt == PH_TILE)
                for (int i = tid; i < L; i += PH_THREADS) prev[i] = val[PH_TILE - L + i];
            __syncthreads();
        }
    }
}

// The ablation variant: one lane per row, sample by sample, over a ring of L doubles per lane (lane-interleaved in the LDS).
constexpr int PHS_THREADS = 64;
constexpr int PHS_MAX_L = 256;                  // 64 lanes x 256 doubles = 128 KB

__global__ void __launch_bounds__(PHS_THREADS)
phaser_seq_kernel(const float* __restrict__ x, long long rows, long long length, long long stride_r, const int* __restrict__ mod,
                  int P, int L, double gain_in, double decay, double gain_out, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double phs_ring[];
    const int lane = threadIdx.x;
    for (long long base = (long long)blockIdx.x * PHS_THREADS; base < rows; base += (long long)gridDim.x * PHS_THREADS) {
        const long long row = base + lane;
        if (row < rows) {
            for (int i = 0; i < L; ++i) phs_ring[i * PHS_THREADS + lane] = 0.0;
            const float* src = x + row * stride_r;
            float* dst = out + row * length;
            int pos = 0, mp = 0;                            // n mod L, n mod P
            for (long long n = 0; n < length; ++n) {
                int d = L - mod[mp] + 1;
                d = d < 1 ? 1 : (d > L ? L : d);
                int at = pos - d;                           // y[n - d] lies at (n - d) mod L
                at = at < 0 ? at + L : at;
                const double y = fma(decay, phs_ring[at * PHS_THREADS + lane], gain_in * (double)src[n]);
                phs_ring[pos * PHS_THREADS + lane] = y;
                dst[n] = sx_clamp(gain_out * y);
                pos = pos + 1 == L ? 0 : pos + 1;
                mp = mp + 1 == P ? 0 : mp + 1;
            }
        }
    }
}

// ============================================================================= flanger
constexpr int FL_MAX_LB = 4096;                 // ring samples: (delay + depth) = 40 ms at 102 kHz
constexpr int FL_MAX_BLOCK = 64;                // W: the lanes of a wave
constexpr int FL_MAX_CHANNELS = 4;
constexpr int FL_THREADS = 256;                 // the FIR path
constexpr int FL_TILE = 4096;
constexpr int FL_BLOCKS_PER_CU = 4;
constexpr int FL_CHUNK = 1024;                  // the feedback path: samples staged per chunk by the wave
constexpr int FLB_BLOCKS_PER_CU = 8;

struct FlParams {
    int P, Lb, W, quadratic, channels;
    int phase[FL_MAX_CHANNELS];
    double fb, in_gain, delay_gain;
};

// delayed = the interpolation at D of taps(0), taps(1), taps(2), the samples k, k + 1, k + 2 back
template <class Tap>
__device__ __forceinline__ double fl_delayed(float D, int Lb, int quadratic, Tap tap) {
    int k = (int)D;                                         // D >= 0: the floor
    k = k < 0 ? 0 : (k > Lb - 2 ? Lb - 2 : k);
    const double fr = (double)(D - (float)k);
    const double d0 = tap(k), d1 = tap(k + 1);
    if (!quadratic) return d0 + (d1 - d0) * fr;
    const double d2 = (k + 2 < Lb ? tap(k + 2) : 0.0) - d0;    // (k + 2 == Lb: fr == 0, the tap's weight is exactly zero)
    const double e1 = d1 - d0;
    return d0 + ((d2 * 0.5 - e1) * fr + (2.0 * e1 - d2 * 0.5)) * fr;
}

template <bool VEC>
__global__ void __launch_bounds__(FL_THREADS)
flanger_fir_kernel(const float* __restrict__ x, long long rows, long long length, long long stride_r,
                   const float* __restrict__ lfo, FlParams Q, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float fl_xs[];          // [Lb halo | FL_TILE]
    const int tid = threadIdx.x;
    const long long tiles = (length + FL_TILE - 1) / FL_TILE;
    const int halo = Q.Lb;
    for (long long unit = blockIdx.x; unit < rows * tiles; unit += gridDim.x) {
        const long long row = unit / tiles, t = unit - row * tiles;
        const float* src = x + row * stride_r;
        float* dst = out + row * length;
        const long long n0 = t * FL_TILE;
        const int nt = (int)(length - n0 < FL_TILE ? length - n0 : FL_TILE);
        const int back = (int)(n0 < halo ? n0 : halo);      // samples before the tile that exist
        sx_load<VEC, FL_THREADS>(src, length, n0 - back, back + nt, tid, [&](int j, float v) { fl_xs[halo - back + j] = v; });
        __syncthreads();
        const unsigned m0 = (unsigned)((n0 + Q.phase[row % Q.channels]) % Q.P);
        for (int j = tid; j < nt; j += FL_THREADS) {
            const float D = lfo[(m0 + (unsigned)j) % (unsigned)Q.P];
            const double xi = (double)fl_xs[halo + j];
            const double dl = fl_delayed(D, Q.Lb, Q.quadratic, [&](int k) {
                return n0 + j - k >= 0 ? (double)fl_xs[halo + j - k] : 0.0;
            });
            dst[n0 + j] = sx_clamp(Q.in_gain * xi + Q.delay_gain * dl);
        }
        __syncthreads();
    }
}

// slot i (1 <= i <= length): delayed[i - 1] from the ring, out[i - 1], then w[i] (i < length).  Slot 0 is w[0] = x[0].
__global__ void __launch_bounds__(64)
flanger_fb_kernel(const float* __restrict__ x, long long rows, long long length, long long stride_r,
                  const float* __restrict__ lfo, FlParams Q, int ring, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double fl_w[];           // [ring] doubles, ring a power of two >= Lb + W
    float* xs = reinterpret_cast<float*>(fl_w + ring);                      // x[n0 .. n0 + FL_CHUNK]
    float* ls = xs + FL_CHUNK + 1;                                          // lfo at n0 .. n0 + FL_CHUNK - 1
    float* os = ls + FL_CHUNK;                                              // out[n0 .. n0 + FL_CHUNK - 1]
    const int lane = threadIdx.x;
    const int mask = ring - 1;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* src = x + row * stride_r;
        float* dst = out + row * length;
        const int phi = Q.phase[row % Q.channels];
        for (int i = lane; i < ring; i += 64) fl_w[i] = 0.0;
        __syncthreads();
        for (long long n0 = 0; n0 < length; n0 += FL_CHUNK) {
            const int nt = (int)(length - n0 < FL_CHUNK ? length - n0 : FL_CHUNK);      // outputs n0 .. n0 + nt - 1
            const unsigned m0 = (unsigned)((n0 + phi) % Q.P);
            for (int j = lane; j <= nt; j += 64) {
                if (n0 + j < length) xs[j] = src[n0 + j];
                if (j < nt) ls[j] = lfo[(m0 + (unsigned)j) % (unsigned)Q.P];
            }
            __syncthreads();
            if (n0 == 0 && lane == 0) fl_w[0] = (double)xs[0];
            __syncthreads();
            // slots n0 + 1 .. n0 + nt in steps of W
            for (int s = 1; s <= nt; s += Q.W) {
                const int j = s + lane;                     // the slot, relative to n0
                if (lane < Q.W && j <= nt) {
                    const long long i = n0 + j;
                    const double dl = fl_delayed(ls[j - 1], Q.Lb, Q.quadratic, [&](int k) {
                        return i - 1 - k >= 0 ? fl_w[(int)((i - 1 - k) & mask)] : 0.0;
                    });
                    os[j - 1] = sx_clamp(Q.in_gain * (double)xs[j - 1] + Q.delay_gain * dl);
                    if (i < length) fl_w[(int)(i & mask)] = (double)xs[j] + Q.fb * dl;
                }
                __syncthreads();
            }
            for (int j = lane; j < nt; j += 64) dst[n0 + j] = os[j];
            __syncthreads();
        }
    }
}

inline bool fl_supported(int Lb, int P, int W, int channels) {
    return Lb >= 2 && Lb <= FL_MAX_LB && P >= 1 && W >= 1 && W <= FL_MAX_BLOCK && W <= Lb - 1 &&
           channels >= 1 && channels <= FL_MAX_CHANNELS;
}

}  // namespace tac

extern "C" {

int32_t tac_overdrive_tile(void) { return tac::OD_TILE; }
int32_t tac_overdrive_blocks_per_cu(void) { return tac::OD_BLOCKS_PER_CU; }

int tac_overdrive_supported(double g, double c) {
    tac::OdParams P;
    return tac::od_params(g, c, &P);
}

int tac_overdrive_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, double g, double c, float* out, void* stream) {
    using namespace tac;
    if (!x || !out || rows <= 0 || length <= 0) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    OdParams P;
    const int rc = od_params(g, c, &P);
    if (rc != TAC_OK) return rc;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_r & 3) == 0;
    const size_t bytes = OD_HEAD * sizeof(double) + OD_XS * sizeof(float);
    const long long blocks = persistent_blocks(rows, 1, (long long)device_cu_count() * OD_BLOCKS_PER_CU);
    auto kern = vec ? overdrive_kernel<true> : overdrive_kernel<false>;
    return launch_kernel(kern, blocks, OD_THREADS, bytes, (hipStream_t)stream, x, (long long)rows, (long long)length,
                         (long long)stride_r, P, out);
}

int32_t tac_phaser_tile(void) { return tac::PH_TILE; }
int32_t tac_phaser_max_delay(void) { return tac::PH_MAX_L; }
int32_t tac_phaser_seq_max_delay(void) { return tac::PHS_MAX_L; }
int32_t tac_phaser_blocks_per_cu(void) { return tac::PH_BLOCKS_PER_CU; }

int tac_phaser_supported(int32_t L, int32_t P) {
    if (L < 1 || P < 1) return TAC_E_INVALID;
    return L <= tac::PH_MAX_L ? TAC_OK : TAC_E_UNSUPPORTED;
}

int tac_phaser_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const int32_t* mod, int32_t P, int32_t L,
                   double gain_in, double decay, double gain_out, float* out, void* stream) {
    using namespace tac;
    if (!x || !out || !mod || rows <= 0 || length <= 0) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    const int rc = tac_phaser_supported(L, P);
    if (rc != TAC_OK) return rc;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_r & 3) == 0;
    const long long blocks = persistent_blocks(rows, 1, (long long)device_cu_count() * PH_BLOCKS_PER_CU);
    auto kern = vec ? phaser_kernel<true> : phaser_kernel<false>;
    return launch_kernel(kern, blocks, PH_THREADS, PH_LDS, (hipStream_t)stream, x, (long long)rows, (long long)length,
                         (long long)stride_r, (const int*)mod, (int)P, (int)L, gain_in, decay, gain_out, out);
}

int tac_phaser_seq_f32(const float* x, int64_t rows, int64_t length, int64_t stride_r, const int32_t* mod, int32_t P, int32_t L,
                       double gain_in, double decay, double gain_out, float* out, void* stream) {
    using namespace tac;
    if (!x || !out || !mod || rows <= 0 || length <= 0) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    if (L < 1 || P < 1) return TAC_E_INVALID;
    if (L > PHS_MAX_L) return TAC_E_UNSUPPORTED;
    const long long blocks = persistent_blocks(rows, PHS_THREADS, (long long)device_cu_count());
    return launch_kernel(phaser_seq_kernel, blocks, PHS_THREADS, (size_t)L * PHS_THREADS * sizeof(double), (hipStream_t)stream, x,
                         (long long)rows, (long long)length, (long long)stride_r, (const int*)mod, (int)P, (int)L, gain_in, decay,
                         gain_out, out);
}

int32_t tac_flanger_tile(void) { return tac::FL_TILE; }
int32_t tac_flanger_chunk(void) { return tac::FL_CHUNK; }
int32_t tac_flanger_max_block(void) { return tac::FL_MAX_BLOCK; }
int32_t tac_flanger_max_delay(void) { return tac::FL_MAX_LB; }
int32_t tac_flanger_blocks_per_cu(void) { return tac::FL_BLOCKS_PER_CU; }
int32_t tac_flanger_fb_blocks_per_cu(void) { return tac::FLB_BLOCKS_PER_CU; }

int tac_flanger_supported(int32_t Lb, int32_t P, int32_t W, int32_t channels) {
    if (Lb < 2 || P < 1 || W < 1 || channels < 1) return TAC_E_INVALID;
    return tac::fl_supported(Lb, P, W, channels) ? TAC_OK : TAC_E_UNSUPPORTED;
}

int tac_flanger_f32(const float* x, int64_t rows, int32_t channels, int64_t length, int64_t stride_r, const float* lfo, int32_t P,
                    const int32_t* phases, int32_t Lb, int32_t W, double fb, double in_gain, double delay_gain, int quadratic,
                    float* out, void* stream) {
    using namespace tac;
    if (!x || !out || !lfo || !phases || rows <= 0 || length <= 0) return TAC_E_INVALID;
    if (rows == 1) stride_r = 0;
    if (rows > 1 && stride_r <= 0) return TAC_E_INVALID;
    const int rc = tac_flanger_supported(Lb, P, W, channels);
    if (rc != TAC_OK) return rc;
    if (!isfinite(fb) || !isfinite(in_gain) || !isfinite(delay_gain)) return TAC_E_INVALID;
    FlParams Q{};
    Q.P = P;
    Q.Lb = Lb;
    Q.W = W;
    Q.quadratic = quadratic ? 1 : 0;
    Q.channels = channels;
    for (int c = 0; c < channels; ++c) {
        if (phases[c] < 0) return TAC_E_INVALID;
        Q.phase[c] = phases[c];
    }
    Q.fb = fb;
    Q.in_gain = in_gain;
    Q.delay_gain = delay_gain;
    if (fb == 0.0) {
        const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_r & 3) == 0;
        const long long tiles = (length + FL_TILE - 1) / FL_TILE;
        const long long blocks = persistent_blocks(rows * tiles, 1, (long long)device_cu_count() * FL_BLOCKS_PER_CU);
        auto kern = vec ? flanger_fir_kernel<true> : flanger_fir_kernel<false>;
        return launch_kernel(kern, blocks, FL_THREADS, (size_t)(Lb + FL_TILE) * sizeof(float), (hipStream_t)stream, x,
                             (long long)rows, (long long)length, (long long)stride_r, lfo, Q, out);
    }
    int ring = 64;
    while (ring < Lb + W) ring <<= 1;
    const size_t bytes = (size_t)ring * sizeof(double) + (size_t)(3 * FL_CHUNK + 1) * sizeof(float);
    const long long blocks = persistent_blocks(rows, 1, (long long)device_cu_count() * FLB_BLOCKS_PER_CU);
    return launch_kernel(flanger_fb_kernel, blocks, 64, bytes, (hipStream_t)stream, x, (long long)rows, (long long)length,
                         (long long)stride_r, lfo, Q, ring, out);
}

}  // extern "C"
