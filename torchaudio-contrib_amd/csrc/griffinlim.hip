// griffinlim.hip — the Griffin-Lim iteration (functional.griffinlim / GriffinLim) around tac_stft_f32 and tac_istft_f32:
//
//   S = specgram^(1 / power);  A = angles0 or 1;  Rprev = 0
//   n_iter times:  y = istft(S A);  R = stft(y);  A = R - m Rprev;  A = A / (|A| + 1e-16);  Rprev = R
//   y = istft(S A)
//
// Everything between the two transforms is elementwise over frame-major rows [rows][T][F], the layout tac_stft_f32 writes and
// tac_istft_f32 reads in place.
//
// gl_prepare_kernel, once per call: reads specgram[r*sr + f*sf + t*st] where it lies (any positive element strides), applies the
// root, and writes the frame-major magnitude M [rows][T][F] and the first iterate X0 [rows][T][F][2] = (M, 0), or M angles0.  A
// time-contiguous input (st == 1: the (…, F, T) tensor a model emits) is turned in the LDS, as specaug.hip / beamform.hip turn
// theirs: a 64 x 64 tile is loaded with lanes along time into rows of odd pitch and read back with lanes along frequency, so
// both the loads and the stores are coalesced.  angles0 (complex pairs, its own strides) is turned likewise.  With M == NULL only
// X0 is written (the input IS the frame-major magnitude already).
//
// gl_update_kernel, once per iteration: X = M (R - m Rprev) / (|R - m Rprev| + 1e-16) by gl_project (griffinlim_project.hpp).  A
// thread owns two consecutive bins: one 16-byte load of R and of Rprev, 8 bytes of M, one 16-byte store, where all four pointers
// allow it; dword accesses otherwise (any alignment).  Grid-stride over the pairs.
//
// The same projection folded into the frame load of the fused fft_length-2048 inverse (X never stored, two launches a step) was
// built and measured slower than this kernel followed by tac_istft_f32 at all three hops: tools/ablation/README.md.
#include "host_common.hpp"
#include "griffinlim_project.hpp"

namespace tac {
namespace {

constexpr int GL_THREADS = 256;
constexpr int GL_TILE = 64;
constexpr int GL_PITCH = GL_TILE + 1;
enum { GL_ROOT_NONE = 0, GL_ROOT_SQRT = 1, GL_ROOT_POW = 2 };

struct GlPrep {
    long long rows, F, T;
    long long sr, sf, st;            // specgram, in floats
    long long ar, af, at;            // angles0, in complex pairs
    int turn_s, turn_a, root;
    float q;                         // 1 / power
    unsigned n_fb, n_tb, units;
};

__device__ __forceinline__ float gl_root(float s, int root, float q) {
    return root == GL_ROOT_NONE ? s : (root == GL_ROOT_SQRT ? __builtin_sqrtf(s) : powf(s, q));
}

__global__ void __launch_bounds__(GL_THREADS)
gl_prepare_kernel(const float* __restrict__ spec, const cf* __restrict__ angles, GlPrep g, float* __restrict__ mag,
                  cf* __restrict__ x0) {
    __shared__ float tile_s[GL_TILE * GL_PITCH];
    __shared__ cf tile_a[GL_TILE * GL_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool turn = g.turn_s || g.turn_a;
    for (unsigned u = blockIdx.x; u < g.units; u += gridDim.x) {
        const unsigned tb = u % g.n_tb, v = u / g.n_tb;
        const long long fb = v % g.n_fb, row = v / g.n_fb;
        const long long f0 = fb * GL_TILE, t0 = (long long)tb * GL_TILE;
        const float* src = spec + row * g.sr;
        const cf* ang = angles ? angles + row * g.ar : nullptr;
        if (turn) {
            __syncthreads();             // every thread has left the tiles of the unit before
            // lanes along time, a wave per frequency line
            const bool t_in = t0 + lane < g.T;
#pragma unroll 4
            for (int p = 0; p < GL_TILE / 4; ++p) {
                const int ff = p * 4 + wave;
                if (t_in && f0 + ff < g.F) {
                    if (g.turn_s) tile_s[ff * GL_PITCH + lane] = src[(f0 + ff) * g.sf + (t0 + lane) * g.st];
                    if (g.turn_a) tile_a[ff * GL_PITCH + lane] = ang[(f0 + ff) * g.af + (t0 + lane) * g.at];
                }
            }
            __syncthreads();
        }
        // lanes along frequency, a wave per frame
        const bool f_in = f0 + lane < g.F;
#pragma unroll 4
        for (int p = 0; p < GL_TILE / 4; ++p) {
            const int tt = p * 4 + wave;
            if (f_in && t0 + tt < g.T) {
                const float s = g.turn_s ? tile_s[lane * GL_PITCH + tt] : src[(f0 + lane) * g.sf + (t0 + tt) * g.st];
                const float mv = gl_root(s, g.root, g.q);
                const long long o = (row * g.T + t0 + tt) * g.F + f0 + lane;
                if (mag) mag[o] = mv;
                cf x = mkc(mv, 0.0f);
                if (ang) {
                    const cf a = g.turn_a ? tile_a[lane * GL_PITCH + tt] : ang[(f0 + lane) * g.af + (t0 + tt) * g.at];
                    x = mkc(mv * a.x, mv * a.y);
                }
                x0[o] = x;
            }
        }
    }
}

// units = ceil(n / 2) pairs of bins
template <bool VEC>
__global__ void __launch_bounds__(GL_THREADS)
gl_update_kernel(const float* __restrict__ r, const float* __restrict__ rprev, const float* __restrict__ mag, float m, long long n,
                 float* __restrict__ x) {
    typedef float f4a __attribute__((ext_vector_type(4)));
    typedef float f2a __attribute__((ext_vector_type(2)));
    const bool prev = rprev != nullptr;
    const long long units = (n + 1) >> 1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += (long long)gridDim.x * blockDim.x) {
        const long long b = 2 * i;
        if (VEC && b + 1 < n) {
            const f4a rv = *reinterpret_cast<const f4a*>(r + 2 * b);
            f4a pv = {0.0f, 0.0f, 0.0f, 0.0f};
            if (prev) pv = *reinterpret_cast<const f4a*>(rprev + 2 * b);
            const f2a mv = *reinterpret_cast<const f2a*>(mag + b);
            const cf x0 = gl_project(mkc(rv[0], rv[1]), mkc(pv[0], pv[1]), m, mv[0], prev);
            const cf x1 = gl_project(mkc(rv[2], rv[3]), mkc(pv[2], pv[3]), m, mv[1], prev);
            *reinterpret_cast<f4a*>(x + 2 * b) = f4a{x0.x, x0.y, x1.x, x1.y};
        } else {
            for (long long k = b; k < b + 2 && k < n; ++k) {
                const cf rv = mkc(r[2 * k], r[2 * k + 1]);
                const cf pv = prev ? mkc(rprev[2 * k], rprev[2 * k + 1]) : mkc(0.0f, 0.0f);
                const cf xv = gl_project(rv, pv, m, mag[k], prev);
                x[2 * k] = xv.x;
                x[2 * k + 1] = xv.y;
            }
        }
    }
}

}  // namespace
}  // namespace tac

extern "C" {

int tac_griffinlim_prepare_f32(const float* spec, int64_t rows, int64_t n_freqs, int64_t n_frames, int64_t stride_r, int64_t stride_f,
                               int64_t stride_t, const float* angles, int64_t astride_r, int64_t astride_f, int64_t astride_t,
                               float power, float* mag, float* x0, void* stream) {
    using namespace tac;
    if (!spec || !x0 || rows <= 0 || n_freqs <= 0 || n_frames <= 0 || !(power > 0.0f)) return TAC_E_INVALID;
    if (rows == 1) stride_r = astride_r = 0;
    if (n_freqs == 1) stride_f = astride_f = 0;
    if (n_frames == 1) stride_t = astride_t = 0;
    if ((rows > 1 && stride_r <= 0) || (n_freqs > 1 && stride_f <= 0) || (n_frames > 1 && stride_t <= 0)) return TAC_E_INVALID;
    if (angles && ((rows > 1 && astride_r <= 0) || (n_freqs > 1 && astride_f <= 0) || (n_frames > 1 && astride_t <= 0))) return TAC_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(spec) & 3u) || (reinterpret_cast<uintptr_t>(angles) & 7u) || (reinterpret_cast<uintptr_t>(mag) & 3u) ||
        (reinterpret_cast<uintptr_t>(x0) & 7u))
        return TAC_E_UNSUPPORTED;
    const long long n_fb = (n_freqs + GL_TILE - 1) / GL_TILE, n_tb = (n_frames + GL_TILE - 1) / GL_TILE;
    if ((double)rows * (double)n_fb * (double)n_tb > 2147483647.0) return TAC_E_UNSUPPORTED;
    GlPrep g;
    g.rows = rows, g.F = n_freqs, g.T = n_frames;
    g.sr = stride_r, g.sf = stride_f, g.st = stride_t;
    g.ar = astride_r, g.af = astride_f, g.at = astride_t;
    g.turn_s = stride_f != 1 && n_freqs > 1 && n_frames > 1 && stride_t == 1;
    g.turn_a = angles && astride_f != 1 && n_freqs > 1 && n_frames > 1 && astride_t == 1;
    g.root = power == 1.0f ? GL_ROOT_NONE : (power == 2.0f ? GL_ROOT_SQRT : GL_ROOT_POW);
    g.q = (float)(1.0 / (double)power);
    g.n_fb = (unsigned)n_fb, g.n_tb = (unsigned)n_tb, g.units = (unsigned)(rows * n_fb * n_tb);
    const int rc = launch_kernel(gl_prepare_kernel, persistent_blocks(g.units, 1, (long long)device_cu_count() * 8), GL_THREADS, 0,
                                 (hipStream_t)stream, spec, reinterpret_cast<const cf*>(angles), g, mag, reinterpret_cast<cf*>(x0));
    if (rc != TAC_OK) return rc;
    set_last_route("gl_prepare_kernel<turn=%d/%d, root=%d, mag=%d>", g.turn_s, g.turn_a, g.root, mag ? 1 : 0);
    return TAC_OK;
}

int tac_griffinlim_update_f32(const float* r, const float* rprev, const float* mag, int64_t n_bins, float m, float* x, void* stream) {
    using namespace tac;
    if (!r || !mag || !x || n_bins <= 0) return TAC_E_INVALID;
    if (m == 0.0f) rprev = nullptr;
    const uintptr_t all = reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(rprev) | reinterpret_cast<uintptr_t>(x);
    if ((all & 3u) || (reinterpret_cast<uintptr_t>(mag) & 3u)) return TAC_E_UNSUPPORTED;
    const bool vec = (all & 15u) == 0 && (reinterpret_cast<uintptr_t>(mag) & 7u) == 0;
    const long long blocks = persistent_blocks((n_bins + 1) / 2, GL_THREADS, (long long)device_cu_count() * 4);
    const int rc = vec ? launch_kernel(gl_update_kernel<true>, blocks, GL_THREADS, 0, (hipStream_t)stream, r, rprev, mag, m, (long long)n_bins, x)
                       : launch_kernel(gl_update_kernel<false>, blocks, GL_THREADS, 0, (hipStream_t)stream, r, rprev, mag, m, (long long)n_bins, x);
    if (rc != TAC_OK) return rc;
    set_last_route("gl_update_kernel<vec=%d>", vec ? 1 : 0);
    return TAC_OK;
}

}  // extern "C"
