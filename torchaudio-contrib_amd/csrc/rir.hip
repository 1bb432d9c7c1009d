// rir.hip — functional.simulate_rir_ism: image-source room impulse responses, a batch of rooms in one launch.
//
// Per room (size r, source s, both D = 2 or 3 floats), image X of the table img[n_img][D] (int8, the integer vectors with sum |X_d| <=
// max_order in cartesian_prod order), band b and microphone c, everything in float64 from the float32 inputs as given:
//     loc_d = r_d (X_d + 1) - s_d where X_d is odd, else r_d X_d + s_d
//     att_b = prod_d tr[b][2 d]^|floor(X_d / 2)| tr[b][2 d + 1]^|floor((X_d + 1) / 2)|,   tr = sqrt(1 - absorption)
//     dist = |loc - mic_c|,  amp_b = att_b / dist,  delay = dist sample_rate / sound_speed,  di = ceil(delay),  f = di - delay in [0, 1)
// and amp_b w(m + f), m = -P … P, w(x) = sinc(x) cos^2(pi x / 2P) for |x| <= P, is added to sample di + m + P of the raw response
// of (room, b, c).  The launch writes samples [start, start + length) of every raw response, zeros included.
//
// rir_ism_kernel<NB>: output-stationary.  A wave owns a tile of RIR_TILE samples of one (room, channel) row, all NB bands of it, in
// the LDS (128 … 2048 samples, chosen per launch by rir_pick_tile).  It walks the room's images in index order, 64 at a time: lane l forms image i0 + l's geometry in float64 and tests its
// support [di, di + L) against the tile; the hits are taken in image order from the ballot.  For a hit the lanes run over the taps
// (lane l has the taps l, l + 64, … for the whole launch: their table values stay in registers), and add amp_b w to the tile of
// every band: the taps are shared between the bands.  The order of every output's sum is the image order, whatever the tile, the
// grid or the batch: the same bits every run.  No atomics, one writer per output element.
// Roundings: f and amp_b are the float64 values rounded once per (image, channel), sinpi(f) and (cos, sin)(pi f / 2P) float64 functions of
// that ROUNDED f rounded once (x = m + f and sin(pi x) then speak of the same x, also where x is tiny); a tap is float32:
//     x = m + f;   sin(pi x) = (-1)^m sinpi(f);   c = cos(pi m / 2P) cos(pi f / 2P) - sin(pi m / 2P) sin(pi f / 2P) (the table of m in float64, rounded once)
//     w = (-1)^m sinpi(f) / (pi x) c^2 (1 at x = 0, 0 for x > P);   tile = fma(amp_b, w, tile)
// nothing in it cancels.  A microphone on an image has dist = 0: amp = inf, f = 0, and the row gets the inf and the NaNs (inf 0) of
// the formulas; no other row reads anything of it.  A non-finite delay (NaN inputs) adds nothing.
//
// rir_span_kernel: max over (room, image, channel) of di, plus L - P: the natural length.  One workgroup, an int64 on the device.
#include <math.h>

#include "host_common.hpp"

namespace tac {

constexpr int RIR_MIN_TILE = 128, RIR_MAX_TILE = 2048;     // samples of a row a wave owns: a power of two between them, chosen per launch
constexpr int RIR_WAVES = 4;                  // waves (units) per workgroup: nothing is shared between them
constexpr int RIR_MAX_BANDS = 8;
constexpr int RIR_MAX_L = 255;                // taps: four per lane at most
constexpr int RIR_SLOTS = (RIR_MAX_L + 63) / 64;
constexpr int RIR_MAX_ORDER = 32;
constexpr int RIR_SPAN_THREADS = 1024;

struct RirArgs {
    const float* room;         // [B][D]
    const float* source;       // [B][D]
    const float* mic;          // [B][M][D]
    const float* absorb;       // [B or 1][nb][2 D]
    const signed char* img;    // [n_img][D]
    const float* tab;          // [L][2]: cos and sin of pi m / 2P, m = -P … P
    float* out;                // [B][nb][M][length]
    long long B, M, n_img, start, length, tiles, absorb_stride;
    int D, nb, P, L, E;        // E: entries of a wall's power table, 0 … (max_order + 1) / 2
    double rate, speed;
};

struct RirImage {
    double dist, delay;
    long long di;              // ceil(delay); only where `finite`
    bool finite;
};

// the float64 geometry of (image X, microphone): separate roundings for every product and sum, as torch's operators make them
__device__ inline RirImage rir_image(const double* r, const double* s, const double* mic, const signed char* X, int D, double rate, double speed) {
#pragma clang fp contract(off)
    double sq = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {                                       // (a third axis of a 2-D room: 0 0 + 0 - 0, which adds an exact 0)
        const int x = d < D ? X[d] : 0;
        const double loc = (x & 1) ? r[d] * (double)(x + 1) - s[d] : r[d] * (double)x + s[d];
        const double df = loc - mic[d];
        sq = sq + df * df;
    }
    RirImage g;
    g.dist = sqrt(sq);
    g.delay = g.dist * rate / speed;
    const double up = ceil(g.delay);
    g.finite = up >= 0.0 && up < 4.0e18;
    g.di = g.finite ? (long long)up : 0;
    return g;
}

template <int NB, int RIR_TILE>
__global__ void __launch_bounds__(RIR_WAVES * 64)
rir_ism_kernel(const RirArgs A) {
    extern __shared__ __align__(16) unsigned char rir_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long unit = (long long)blockIdx.x * RIR_WAVES + wave;
    if (unit >= A.B * A.M * A.tiles) return;                          // (no workgroup barrier anywhere below)
    const int D = A.D, P = A.P, L = A.L, E = A.E;
    const int ptab_n = NB * 2 * D * E;
    const size_t wave_bytes = (size_t)NB * RIR_TILE * 4 + (((size_t)ptab_n * 8 + 15) & ~(size_t)15);
    float* tile = reinterpret_cast<float*>(rir_lds + wave * wave_bytes);                  // [NB][RIR_TILE]
    double* ptab = reinterpret_cast<double*>(tile + NB * RIR_TILE);                     // [NB][2 D][E]: tr^e

    const long long row = unit / A.tiles, tidx = unit - row * A.tiles;
    const long long room = row / A.M, ch = row - room * A.M;
    const long long t0 = tidx * RIR_TILE;                               // of the output; raw sample = start + t0 + …

    double r[3], s[3], mc[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        r[d] = d < D ? (double)A.room[room * D + d] : 0.0;
        s[d] = d < D ? (double)A.source[room * D + d] : 0.0;
        mc[d] = d < D ? (double)A.mic[(room * A.M + ch) * D + d] : 0.0;
    }
    // the powers of the walls' reflection coefficients, a lane per (band, wall)
    {
        const float* ab = A.absorb + room * A.absorb_stride;
        if (lane < NB * 2 * D) {
            const double tr = sqrt(1.0 - (double)ab[lane]);
            double p = 1.0;
            for (int e = 0; e < E; ++e) {
                ptab[lane * E + e] = p;
                p *= tr;
            }
        }
        for (int i = lane; i < NB * RIR_TILE; i += 64) tile[i] = 0.0f;
    }
    // the lane's taps j = lane + 64 k: m = j - P, its sign, and cos / sin of pi m / 2P
    float mf[RIR_SLOTS], sg[RIR_SLOTS], cm[RIR_SLOTS], sm[RIR_SLOTS];
#pragma unroll
    for (int k = 0; k < RIR_SLOTS; ++k) {
        const int j = lane + 64 * k;
        const bool in = j < L;
        mf[k] = (float)(j - P);
        sg[k] = ((j - P) & 1) ? -1.0f : 1.0f;
        cm[k] = in ? A.tab[2 * j] : 0.0f;
        sm[k] = in ? A.tab[2 * j + 1] : 0.0f;
    }
    const int slots = (L + 63) / 64;
    const float pi_f = 3.14159265358979323846f, Pf = (float)P;
    const double quarter = 0.5 / (double)P;                            // pi f / 2P = pi (f quarter)
    const long long lo = A.start + t0;                                  // the tile's first raw sample
    __builtin_amdgcn_wave_barrier();

    for (long long i0 = 0; i0 < A.n_img; i0 += 64) {
        const long long i = i0 + lane;
        bool hit = false;
        int rel = 0;                                                    // di - lo where it is a hit: in (-L, RIR_TILE)
        float f = 0.0f, sp = 0.0f, cf = 1.0f, sf = 0.0f, amp[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) amp[b] = 0.0f;
        if (i < A.n_img) {
            const signed char* X = A.img + i * D;
            const RirImage g = rir_image(r, s, mc, X, D, A.rate, A.speed);
            const long long first = g.di - lo;
            hit = g.finite && first > -(long long)L && first < RIR_TILE;
            if (hit) {
                rel = (int)first;
                f = (float)((double)g.di - g.delay);
                const double fd = (double)f;                            // everything below is of the ROUNDED f: x = m + f is what sinpi sees
                sp = (float)sinpi(fd);
                cf = (float)cospi(fd * quarter);
                sf = (float)sinpi(fd * quarter);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    double att = 1.0;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        if (d >= D) continue;
                        const int x = X[d];
                        const int e_lo = abs(x >> 1), e_hi = abs((x + 1) >> 1);
                        att = att * ptab[(b * 2 * D + 2 * d) * E + e_lo] * ptab[(b * 2 * D + 2 * d + 1) * E + e_hi];
                    }
                    amp[b] = (float)(att / g.dist);
                }
            }
        }
        unsigned long long hits = __ballot(hit);
        while (hits) {
            const int src = __ffsll((long long)hits) - 1;
            hits &= hits - 1;
            const int h_rel = __shfl(rel, src, 64);
            const float h_f = __shfl(f, src, 64), h_sp = __shfl(sp, src, 64), h_cf = __shfl(cf, src, 64), h_sf = __shfl(sf, src, 64);
            float h_amp[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) h_amp[b] = __shfl(amp[b], src, 64);
#pragma unroll
            for (int k = 0; k < RIR_SLOTS; ++k) {
                if (k < slots) {
                    const int j = lane + 64 * k, t = h_rel + j;
                    if (j < L && t >= 0 && t < RIR_TILE) {
                        const float x = mf[k] + h_f;
                        const float c = fmaf(cm[k], h_cf, -(sm[k] * h_sf));
                        float w = x == 0.0f ? 1.0f : (sg[k] * h_sp) / (pi_f * x);
                        w = x > Pf ? 0.0f : w * (c * c);
#pragma unroll
                        for (int b = 0; b < NB; ++b) tile[b * RIR_TILE + t] = fmaf(h_amp[b], w, tile[b * RIR_TILE + t]);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();                            // the next hit's lanes read what these wrote
        }
    }

    // the tile, written once: 16 bytes a lane where the row's offset allows
    const long long left = A.length - t0;
    const int n = left < RIR_TILE ? (int)left : RIR_TILE;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const long long base = ((room * NB + b) * A.M + ch) * A.length + t0;
        float* dst = A.out + base;
        const float* src = tile + b * RIR_TILE;
        if ((base & 3) == 0) {
            for (int q = lane; 4 * q < n; q += 64) {
                if (4 * q + 4 <= n) {
                    *reinterpret_cast<float4*>(dst + 4 * q) = *reinterpret_cast<const float4*>(src + 4 * q);
                } else {
                    for (int t = 4 * q; t < n; ++t) dst[t] = src[t];
                }
            }
        } else {
            for (int t = lane; t < n; t += 64) dst[t] = src[t];
        }
    }
}

struct RirSpanArgs {
    const float* room;
    const float* source;
    const float* mic;
    const signed char* img;
    long long* out;
    long long B, M, n_img;
    int D, P, L;
    double rate, speed;
};

__global__ void __launch_bounds__(RIR_SPAN_THREADS)
rir_span_kernel(const RirSpanArgs A) {
    __shared__ long long best[RIR_SPAN_THREADS];
    const int tid = threadIdx.x, D = A.D;
    const long long per_room = A.M * A.n_img, total = A.B * per_room;
    long long top = 0;
    for (long long it = tid; it < total; it += RIR_SPAN_THREADS) {
        const long long room = it / per_room, rest = it - room * per_room;
        const long long ch = rest / A.n_img, i = rest - ch * A.n_img;
        double r[3], s[3], mc[3];
        for (int d = 0; d < 3; ++d) {
            r[d] = d < D ? (double)A.room[room * D + d] : 0.0;
            s[d] = d < D ? (double)A.source[room * D + d] : 0.0;
            mc[d] = d < D ? (double)A.mic[(room * A.M + ch) * D + d] : 0.0;
        }
        const RirImage g = rir_image(r, s, mc, A.img + i * D, D, A.rate, A.speed);
        if (g.finite && g.di > top) top = g.di;
    }
    best[tid] = top;
    __syncthreads();
    for (int half = RIR_SPAN_THREADS / 2; half >= 1; half /= 2) {
        if (tid < half && best[tid + half] > best[tid]) best[tid] = best[tid + half];
        __syncthreads();
    }
    if (tid == 0) A.out[0] = best[0] + A.L - A.P;
}

inline int rir_check(int64_t rooms, int64_t mics, int32_t dims, int64_t n_img, int32_t filter_length, double sound_speed, double sample_rate) {
    if (rooms <= 0 || mics <= 0 || n_img <= 0 || (dims != 2 && dims != 3) || filter_length < 1 || !(filter_length & 1) ||
        !(sound_speed > 0.0) || !(sample_rate > 0.0))
        return TAC_E_INVALID;
    if (filter_length < 3 || filter_length > RIR_MAX_L) return TAC_E_UNSUPPORTED;
    return TAC_OK;
}

template <int NB, int TILE>
inline int rir_launch_as(RirArgs& A, hipStream_t stream) {
    A.tiles = (A.length + TILE - 1) / TILE;
    const long long rows = A.B * A.M;
    if (rows > (1LL << 40) / A.tiles) return TAC_E_UNSUPPORTED;
    const long long blocks = (rows * A.tiles + RIR_WAVES - 1) / RIR_WAVES;
    if (blocks >= (1LL << 31)) return TAC_E_UNSUPPORTED;
    const size_t wave_bytes = (size_t)NB * TILE * 4 + (((size_t)NB * 2 * A.D * A.E * 8 + 15) & ~(size_t)15);
    return launch_kernel(rir_ism_kernel<NB, TILE>, blocks, RIR_WAVES * 64, wave_bytes * RIR_WAVES, stream, A);
}

template <int NB>
inline int rir_launch_bands(RirArgs& A, int tile, hipStream_t stream) {
    switch (tile) {
        case 128: return rir_launch_as<NB, 128>(A, stream);
        case 256: return rir_launch_as<NB, 256>(A, stream);
        case 512: return rir_launch_as<NB, 512>(A, stream);
        case 1024: if constexpr (NB <= 4) return rir_launch_as<NB, 1024>(A, stream); else return TAC_E_INVALID;
        case 2048: if constexpr (NB <= 2) return rir_launch_as<NB, 2048>(A, stream); else return TAC_E_INVALID;
        default: return TAC_E_INVALID;
    }
}

// the longest tile a wave may own with n_band bands: 64 KiB of tiles a workgroup at most
inline int rir_max_tile(int n_band) { return n_band <= 2 ? 2048 : n_band <= 4 ? 1024 : 512; }

// The tile of a launch: the longest that still leaves four waves a SIMD (16 a CU) on the whole device.  A wave walks every image of
// its room whatever its tile, so long tiles divide that walk among fewer waves; short ones are for the launches with few rows.  The
// sums do not depend on it: an output's terms arrive in image order in any tile.
inline int rir_pick_tile(long long rows, long long length, int n_band) {
    const long long want = 16LL * device_cu_count();
    for (int tile = rir_max_tile(n_band); tile > RIR_MIN_TILE; tile /= 2)
        if (rows * ((length + tile - 1) / tile) >= want) return tile;
    return RIR_MIN_TILE;
}

}  // namespace tac

extern "C" {

int tac_rir_limits(int32_t* min_tile, int32_t* max_bands, int32_t* max_filter_length, int32_t* max_order) {
    if (min_tile) *min_tile = tac::RIR_MIN_TILE;
    if (max_bands) *max_bands = tac::RIR_MAX_BANDS;
    if (max_filter_length) *max_filter_length = tac::RIR_MAX_L;
    if (max_order) *max_order = tac::RIR_MAX_ORDER;
    return TAC_OK;
}

int tac_rir_tile(int64_t rows, int64_t length, int32_t n_band, int32_t* tile, int32_t* max_tile) {
    if (rows <= 0 || length <= 0 || n_band < 1 || n_band > tac::RIR_MAX_BANDS) return TAC_E_INVALID;
    if (tile) *tile = tac::rir_pick_tile(rows, length, n_band);
    if (max_tile) *max_tile = tac::rir_max_tile(n_band);
    return TAC_OK;
}

int tac_rir_ism_f32(const float* room, const float* source, const float* mic, const float* absorption, int64_t absorption_stride,
                    const void* images, const float* tap_table, int64_t rooms, int64_t mics, int32_t dims, int32_t n_band, int64_t n_img,
                    int32_t max_order, int64_t start, int64_t length, int32_t filter_length, double sound_speed, double sample_rate,
                    int32_t tile, float* out, void* stream) {
    using namespace tac;
    if (!room || !source || !mic || !absorption || !images || !tap_table || !out || n_band < 1 || max_order < 0 || start < 0 || length <= 0 ||
        (absorption_stride != 0 && absorption_stride != (int64_t)n_band * 2 * dims))
        return TAC_E_INVALID;
    const int rc = rir_check(rooms, mics, dims, n_img, filter_length, sound_speed, sample_rate);
    if (rc != TAC_OK) return rc;
    if (n_band > RIR_MAX_BANDS || max_order > RIR_MAX_ORDER) return TAC_E_UNSUPPORTED;
    RirArgs A;
    A.room = room, A.source = source, A.mic = mic, A.absorb = absorption, A.img = (const signed char*)images, A.tab = tap_table, A.out = out;
    A.B = rooms, A.M = mics, A.n_img = n_img, A.start = start, A.length = length, A.absorb_stride = absorption_stride;
    A.tiles = 0;
    A.D = dims, A.nb = n_band, A.P = filter_length / 2, A.L = filter_length, A.E = (max_order + 1) / 2 + 1;
    A.rate = sample_rate, A.speed = sound_speed;
    if (tile == 0) tile = rir_pick_tile(rooms * mics, length, n_band);
    if (tile < RIR_MIN_TILE || tile > rir_max_tile(n_band) || !is_pow2(tile)) return TAC_E_INVALID;
    switch (n_band) {
        case 1: return rir_launch_bands<1>(A, tile, (hipStream_t)stream);
        case 2: return rir_launch_bands<2>(A, tile, (hipStream_t)stream);
        case 3: return rir_launch_bands<3>(A, tile, (hipStream_t)stream);
        case 4: return rir_launch_bands<4>(A, tile, (hipStream_t)stream);
        case 5: return rir_launch_bands<5>(A, tile, (hipStream_t)stream);
        case 6: return rir_launch_bands<6>(A, tile, (hipStream_t)stream);
        case 7: return rir_launch_bands<7>(A, tile, (hipStream_t)stream);
        default: return rir_launch_bands<8>(A, tile, (hipStream_t)stream);
    }
}

int tac_rir_span_f32(const float* room, const float* source, const float* mic, const void* images, int64_t rooms, int64_t mics, int32_t dims,
                     int64_t n_img, int32_t filter_length, double sound_speed, double sample_rate, int64_t* out, void* stream) {
    using namespace tac;
    if (!room || !source || !mic || !images || !out) return TAC_E_INVALID;
    const int rc = rir_check(rooms, mics, dims, n_img, filter_length, sound_speed, sample_rate);
    if (rc != TAC_OK && !(rc == TAC_E_UNSUPPORTED && filter_length >= 1)) return rc;       // (any odd length has a span)
    RirSpanArgs A;
    A.room = room, A.source = source, A.mic = mic, A.img = (const signed char*)images, A.out = reinterpret_cast<long long*>(out);
    A.B = rooms, A.M = mics, A.n_img = n_img, A.D = dims, A.P = filter_length / 2, A.L = filter_length;
    A.rate = sample_rate, A.speed = sound_speed;
    return launch_kernel(rir_span_kernel, 1LL, RIR_SPAN_THREADS, 0, (hipStream_t)stream, A);
}

}  // extern "C"
