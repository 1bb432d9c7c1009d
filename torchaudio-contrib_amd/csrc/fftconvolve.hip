// fftconvolve.hip — functional.fftconvolve / convolve: uniformly partitioned overlap-save on the STFT kernels.
//
// With B = N / 2, P = ceil(M / B) partitions of the kernel and T = ceil(l_full / B) output blocks:
//   xp        = [B zeros | x | zeros up to (T + 1) B]                                       fc_pad_kernel
//   X_t       = rfft_N(xp[t B .. t B + N))        (frame t holds input blocks t - 1 and t)   tac_stft_f32, window of ones, hop B
//   H_p       = rfft_N([h[p B .. (p + 1) B) | B zeros])                                      tac_fftconvolve_spectra_f32 (cached)
//   Y_t       = sum_{p <= min(P - 1, t)} X_{t-p} H_p                                         tac_spectral_mac_f32   <- the new kernel
//   out block t = the SECOND half of irfft_N(Y_t)                                            frame kernels (inverse mode) + fc_keep_kernel
//
// The inverse is the frame kernel of tac_istft_f32's general route with its own gather, not tac_istft_f32 itself: the overlap-add
// of istft multiplies the discarded first half of a frame by a window of zeros and ADDS it to the block before, and 0 * NaN is
// NaN — a non-finite input block would then reach one output block more than the delay line lets it.  fc_keep_kernel never reads
// the discarded halves.
//
// spectral_mac kernels: every bin is independent.  A wave owns 64 adjacent bins of one row over a tile of consecutive frames
// (512 contiguous bytes per load / store); a lane owns one bin.  Both parts of an output are one fused multiply-add chain in
// ascending p, two terms per p; frames before the row's first are neither read nor multiplied; one writer per output, no
// atomics, no LDS, no barrier: bit-identical from run to run.
//   P <= 16 (buckets 4 / 8 / 16): the lane keeps H_0 .. H_{P-1} of its bin and the last PB frames of X in registers — a ring
//     indexed at compile time (the frame loop is unrolled PB times, tiles start at multiples of PB).  X is read once per tile
//     plus a halo of P - 1 frames.
//   16 < P <= 64: H is streamed (one coalesced load per p, L2-resident: P F 8 bytes <= 2.1 MB): the lane holds 16 outputs'
//     accumulators and a sliding window of 16 X frames, and walks p upwards; X is re-read (P + 15) / 16 times per output, from
//     the caches.
#include "host_common.hpp"

namespace tac {

int launch_istft_frames(int n_fft, const FrameGeom& g, const float* spec, float* frames, hipStream_t s);   // backward.hip

namespace {

constexpr int MAC_WAVES = 4;
constexpr int MAC_MAX_PARTS = 64;
constexpr int MAC_SUB = 16;                                   // outputs per lane and pass of the streamed kernel
constexpr long long FC_WORKSPACE_CAP = 1LL << 30;             // bytes tac_fftconvolve_workspace asks for at most

__device__ __forceinline__ void cmac(float& re, float& im, const cf x, const cf h) {
    re = __builtin_fmaf(x.x, h.x, re);
    re = __builtin_fmaf(-x.y, h.y, re);
    im = __builtin_fmaf(x.x, h.y, im);
    im = __builtin_fmaf(x.y, h.x, im);
}

struct MacArgs {
    const cf* X;
    const cf* H;
    const int* hrow;
    cf* Y;
    long long rows;
    int T, F, P, h_rows, conj, tile, tiles, bin_tiles;
    long long units;
};

__device__ __forceinline__ const cf* mac_kernel_row(const MacArgs& a, long long row) {
    int hr = a.hrow ? a.hrow[row] : 0;
    hr = hr < 0 ? 0 : (hr >= a.h_rows ? a.h_rows - 1 : hr);     // a wrong map gives wrong sums, never an access outside H
    return a.H + (long long)hr * a.P * a.F;
}

template <int PB>
__global__ void __launch_bounds__(MAC_WAVES * 64)
spectral_mac_reg_kernel(MacArgs a) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int P = a.P;
    for (long long unit = (long long)blockIdx.x * MAC_WAVES + w; unit < a.units; unit += (long long)gridDim.x * MAC_WAVES) {
        const int bt = (int)(unit % a.bin_tiles);
        const long long rest = unit / a.bin_tiles;
        const int tile = (int)(rest % a.tiles);
        const long long row = rest / a.tiles;
        const int f = bt * 64 + lane;
        if (f >= a.F) continue;
        const cf* const Hr = mac_kernel_row(a, row) + f;
        const cf* const Xr = a.X + row * a.T * (long long)a.F + f;
        cf* const Yr = a.Y + row * a.T * (long long)a.F + f;
        cf h[PB], ring[PB];
#pragma unroll
        for (int p = 0; p < PB; ++p) {
            h[p] = mkc(0.0f, 0.0f);
            ring[p] = mkc(0.0f, 0.0f);
            if (p < P) {
                const cf v = Hr[(long long)p * a.F];
                h[p] = mkc(v.x, a.conj ? -v.y : v.y);
            }
        }
        const int t0 = tile * a.tile;                           // a multiple of PB
        const int t1 = t0 + a.tile < a.T ? t0 + a.tile : a.T;
#pragma unroll
        for (int p = 1; p < PB; ++p)                            // the halo: frames t0 - 1 .. t0 - (P - 1)
            if (p < P && t0 - p >= 0) ring[PB - p] = Xr[(long long)(t0 - p) * a.F];
        for (int tb = t0; tb < t1; tb += PB) {
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const int t = tb + j;
                if (t < t1) {
                    ring[j] = Xr[(long long)t * a.F];
                    const int np = t + 1 < P ? t + 1 : P;       // partitions that reach back to a frame of the row
                    float re = 0.0f, im = 0.0f;
#pragma unroll
                    for (int p = 0; p < PB; ++p)
                        if (p < np) cmac(re, im, ring[(j - p + PB) % PB], h[p]);
                    Yr[(long long)t * a.F] = mkc(re, im);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(MAC_WAVES * 64)
spectral_mac_stream_kernel(MacArgs a) {
    constexpr int S = MAC_SUB;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int P = a.P, T = a.T;
    for (long long unit = (long long)blockIdx.x * MAC_WAVES + w; unit < a.units; unit += (long long)gridDim.x * MAC_WAVES) {
        const int bt = (int)(unit % a.bin_tiles);
        const long long rest = unit / a.bin_tiles;
        const int tile = (int)(rest % a.tiles);
        const long long row = rest / a.tiles;
        const int f = bt * 64 + lane;
        if (f >= a.F) continue;
        const cf* const Hr = mac_kernel_row(a, row) + f;
        const cf* const Xr = a.X + row * T * (long long)a.F + f;
        cf* const Yr = a.Y + row * T * (long long)a.F + f;
        const int t0 = tile * a.tile;
        const int t1 = t0 + a.tile < T ? t0 + a.tile : T;
        for (int ts = t0; ts < t1; ts += S) {                   // outputs ts .. ts + S - 1
            float re[S], im[S];
            cf win[S];                                          // frame i lives in slot (i - ts) mod S
#pragma unroll
            for (int j = 0; j < S; ++j) {
                re[j] = im[j] = 0.0f;
                win[j] = ts + j < t1 ? Xr[(long long)(ts + j) * a.F] : mkc(0.0f, 0.0f);
            }
            const int reach = ts + S < P ? ts + S : P;          // p < reach: some output of this pass has a frame t - p >= 0
            for (int pc = 0; pc < reach; pc += S) {
#pragma unroll
                for (int pp = 0; pp < S; ++pp) {
                    const int p = pc + pp;
                    if (p < reach) {
                        if (p > 0 && ts - p >= 0)               // frame ts - p replaces frame ts - p + S, used up at p - 1
                            win[(S - pp) % S] = Xr[(long long)(ts - p) * a.F];
                        cf h = Hr[(long long)p * a.F];
                        if (a.conj) h.y = -h.y;
#pragma unroll
                        for (int j = 0; j < S; ++j)
                            if (ts + j >= p) cmac(re[j], im[j], win[(j - pp + S) % S], h);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < S; ++j)
                if (ts + j < t1) Yr[(long long)(ts + j) * a.F] = mkc(re[j], im[j]);
        }
    }
}

inline int mac_bucket(int P) { return P <= 4 ? 4 : (P <= 8 ? 8 : (P <= 16 ? 16 : 0)); }

// frames per time tile: four times the halo, a multiple of the unroll
inline int mac_tile(int P) {
    const int pb = mac_bucket(P);
    if (pb) return 4 * pb;
    return ((4 * P + MAC_SUB - 1) / MAC_SUB) * MAC_SUB;
}

int launch_spectral_mac(const float* X, const float* H, const int32_t* hrow, long long rows, long long T, int F, int P, int h_rows,
                        int conj, float* Y, hipStream_t s) {
    MacArgs a{};
    a.X = reinterpret_cast<const cf*>(X);
    a.H = reinterpret_cast<const cf*>(H);
    a.hrow = hrow;
    a.Y = reinterpret_cast<cf*>(Y);
    a.rows = rows;
    a.T = (int)T;
    a.F = F;
    a.P = P;
    a.h_rows = h_rows;
    a.conj = conj ? 1 : 0;
    a.tile = mac_tile(P);
    a.tiles = (int)((T + a.tile - 1) / a.tile);
    a.bin_tiles = (F + 63) / 64;
    a.units = rows * a.tiles * (long long)a.bin_tiles;
    const long long blocks = persistent_blocks(a.units, MAC_WAVES, (long long)device_cu_count() * 8);
    switch (mac_bucket(P)) {
        case 4: return launch_kernel(spectral_mac_reg_kernel<4>, blocks, MAC_WAVES * 64, 0, s, a);
        case 8: return launch_kernel(spectral_mac_reg_kernel<8>, blocks, MAC_WAVES * 64, 0, s, a);
        case 16: return launch_kernel(spectral_mac_reg_kernel<16>, blocks, MAC_WAVES * 64, 0, s, a);
        default: return launch_kernel(spectral_mac_stream_kernel, blocks, MAC_WAVES * 64, 0, s, a);
    }
}

int mac_check(const void* X, const void* H, const void* Y, int64_t rows, int64_t T, int32_t F, int32_t P, int32_t h_rows) {
    if (!X || !H || !Y) return TAC_E_INVALID;
    if (rows <= 0 || T <= 0 || F <= 0 || P <= 0 || h_rows <= 0) return TAC_E_INVALID;
    if (P > MAC_MAX_PARTS) return TAC_E_UNSUPPORTED;
    if (T >= 0x7fffffffLL - 1024 || rows >= 0x7fffffffLL) return TAC_E_UNSUPPORTED;     // 32-bit frame indices in-kernel
    if ((reinterpret_cast<uintptr_t>(X) & 7u) || (reinterpret_cast<uintptr_t>(H) & 7u) || (reinterpret_cast<uintptr_t>(Y) & 7u))
        return TAC_E_UNSUPPORTED;
    return TAC_OK;
}

// dst[r][i] = src[r][i - lead] for 0 <= i - lead < length, else 0     (n positions per row)
__global__ void __launch_bounds__(256)
fc_pad_kernel(const float* __restrict__ src, long long stride_r, long long length, long long rows, long long lead, long long n,
              float* __restrict__ dst) {
    const long long total = rows * n;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long row = idx / n;
        const long long i = idx - row * n - lead;
        dst[idx] = (i >= 0 && i < length) ? src[row * stride_r + i] : 0.0f;
    }
}

// dst[hr][p][n] = h[hr][p B + n] for n < B and p B + n < M (h read from its end when `reverse`), else 0 (n < N = 2 B);
// ones[n] = 1 for n < N
__global__ void __launch_bounds__(256)
fc_kernel_blocks_kernel(const float* __restrict__ y, long long stride_r, long long M, long long h_rows, int P, int B, int reverse,
                        float* __restrict__ dst, float* __restrict__ ones) {
    const long long per_row = (long long)P * 2 * B;
    const long long total = h_rows * per_row;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long hr = idx / per_row;
        const long long q = idx - hr * per_row;
        const int p = (int)(q / (2 * B));
        const int n = (int)(q - (long long)p * 2 * B);
        const long long m = (long long)p * B + n;
        float v = 0.0f;
        if (n < B && m < M) v = y[hr * stride_r + (reverse ? M - 1 - m : m)];
        dst[idx] = v;
        if (idx < 2 * B) ones[idx] = 1.0f;
    }
}

// out[r][j] = frames[r][t][B + n] with t B + n = j + offset   (the kept second halves; j < l_out)
__global__ void __launch_bounds__(256)
fc_keep_kernel(const float* __restrict__ frames, long long rows, long long T, int B, long long offset, long long l_out,
               long long out_stride, float* __restrict__ out) {
    const long long total = rows * l_out;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long row = idx / l_out;
        const long long j = idx - row * l_out;
        const long long i = j + offset;
        const long long t = i / B;
        const int n = (int)(i - t * B);
        out[row * out_stride + j] = frames[(row * T + t) * (2LL * B) + B + n];
    }
}

__global__ void __launch_bounds__(256)
fc_fill_kernel(float* __restrict__ dst, int n, float v) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = v;
}

inline long long fc_grid(long long work) { return persistent_blocks(work, 256, (long long)device_cu_count() * 8); }

inline long long round16(long long floats) { return (floats + 15) & ~15LL; }

struct FcPlan {
    int N, B, F, P;
    long long T;
    long long xp_floats, spec_floats, per_row_floats;          // per row: the padded copy, one dense spectrum, all three areas
    long long fixed_floats;                                     // the window of ones and the rounding of the two spectrum areas
};

int fc_plan(int64_t l_in, int64_t m, int32_t n_fft, int64_t offset, int64_t l_out, FcPlan* pl) {
    if (l_in <= 0 || m <= 0 || offset < 0 || l_out <= 0) return TAC_E_INVALID;
    if (n_fft != 2048 && n_fft != 4096 && n_fft != 8192) return TAC_E_UNSUPPORTED;
    if (l_in >= 0x7fffffffLL - 4 * 8192 || m >= 0x7fffffffLL - 4 * 8192 || l_in + m >= 0x7fffffffLL - 4 * 8192) return TAC_E_UNSUPPORTED;
    if (offset + l_out > l_in + m - 1) return TAC_E_INVALID;
    pl->N = n_fft;
    pl->B = n_fft / 2;
    pl->F = n_fft / 2 + 1;
    const long long parts = (m + pl->B - 1) / pl->B;
    if (parts > MAC_MAX_PARTS) return TAC_E_UNSUPPORTED;
    pl->P = (int)parts;
    pl->T = (offset + l_out + pl->B - 1) / pl->B;
    pl->xp_floats = (pl->T + 1) * pl->B;                       // (a multiple of 1024: rows stay 16-byte aligned)
    pl->spec_floats = pl->T * pl->F * 2;                       // (>= T N floats: the frames of the inverse reuse X's area)
    pl->per_row_floats = pl->xp_floats + 2 * pl->spec_floats;
    pl->fixed_floats = pl->N + 32;
    return TAC_OK;
}

}  // namespace
}  // namespace tac

extern "C" {

int32_t tac_spectral_mac_tile(int32_t n_parts) {
    if (n_parts <= 0 || n_parts > tac::MAC_MAX_PARTS) return TAC_E_UNSUPPORTED;
    return tac::mac_tile(n_parts);
}

int tac_spectral_mac_f32(const float* X, const float* H, const int32_t* hrow, int64_t rows, int64_t n_frames, int32_t n_bins,
                         int32_t n_parts, int32_t h_rows, int conj, float* Y, void* stream) {
    const int rc = tac::mac_check(X, H, Y, rows, n_frames, n_bins, n_parts, h_rows);
    if (rc != TAC_OK) return rc;
    return tac::launch_spectral_mac(X, H, hrow, rows, n_frames, n_bins, n_parts, h_rows, conj, Y, (hipStream_t)stream);
}

int32_t tac_fftconvolve_default_n_fft(int64_t m) {
    for (int n = 2048; n < 8192; n *= 2)
        if ((m + n / 2 - 1) / (n / 2) <= 8) return n;
    return 8192;
}

int tac_fftconvolve_supported(int64_t l_in, int64_t m, int32_t n_fft) {
    tac::FcPlan pl;
    const int rc = tac::fc_plan(l_in, m, n_fft, 0, l_in + m - 1, &pl);
    if (rc != TAC_OK) return rc;
    return (pl.per_row_floats + pl.fixed_floats) * 4 > tac::FC_WORKSPACE_CAP ? TAC_E_UNSUPPORTED : TAC_OK;
}

int64_t tac_fftconvolve_spectra_workspace(int64_t h_rows, int64_t m, int32_t n_fft) {
    tac::FcPlan pl;
    const int rc = tac::fc_plan(1, m, n_fft, 0, m, &pl);
    if (rc != TAC_OK) return rc;
    if (h_rows <= 0) return TAC_E_INVALID;
    return ((int64_t)pl.N + h_rows * pl.P * (int64_t)pl.N) * 4;
}

int tac_fftconvolve_spectra_f32(const float* y, int64_t h_rows, int64_t m, int64_t stride_r, int32_t n_fft, int reverse,
                                void* workspace, int64_t workspace_bytes, float* H, void* stream) {
    using namespace tac;
    if (!y || !workspace || !H) return TAC_E_INVALID;
    const int64_t need = tac_fftconvolve_spectra_workspace(h_rows, m, n_fft);
    if (need < 0) return (int)need;
    if (workspace_bytes < need || (h_rows > 1 && stride_r < m)) return TAC_E_INVALID;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return TAC_E_UNSUPPORTED;
    FcPlan pl;
    fc_plan(1, m, n_fft, 0, m, &pl);
    hipStream_t s = (hipStream_t)stream;
    float* ones = static_cast<float*>(workspace);
    float* blocks = ones + pl.N;
    int rc = launch_kernel(fc_kernel_blocks_kernel, fc_grid(h_rows * pl.P * (long long)pl.N), 256, 0, s, y, (long long)stride_r,
                           (long long)m, (long long)h_rows, pl.P, pl.B, reverse ? 1 : 0, blocks, ones);
    if (rc != TAC_OK) return rc;
    // partition p = frame p of the blocks at a hop of one whole frame
    tac_stft_desc d{};
    d.rows = h_rows;
    d.length = d.row_stride = (int64_t)pl.P * pl.N;
    d.n_fft = d.hop = d.win_length = pl.N;
    d.center = 0;
    d.pad_mode = TAC_PAD_CONSTANT;
    d.normalized = 0;
    d.onesided = 1;
    return tac_stft_f32(blocks, ones, &d, H, stream);
}

int64_t tac_fftconvolve_workspace(int64_t rows, int64_t l_in, int64_t m, int32_t n_fft, int64_t offset, int64_t l_out) {
    tac::FcPlan pl;
    const int rc = tac::fc_plan(l_in, m, n_fft, offset, l_out, &pl);
    if (rc != TAC_OK) return rc;
    if (rows <= 0) return TAC_E_INVALID;
    const int64_t fixed = pl.fixed_floats * 4, per_row = pl.per_row_floats * 4;
    if (fixed + per_row > tac::FC_WORKSPACE_CAP) return TAC_E_UNSUPPORTED;
    const int64_t fit = (tac::FC_WORKSPACE_CAP - fixed) / per_row;
    return fixed + (rows < fit ? rows : fit) * per_row;
}

int tac_fftconvolve_f32(const float* x, int64_t rows, int64_t l_in, int64_t stride_r, const float* H, const int32_t* hrow,
                        int32_t h_rows, int64_t m, int32_t n_fft, int conj, int64_t offset, int64_t l_out, void* workspace,
                        int64_t workspace_bytes, float* out, int64_t out_stride, void* stream) {
    using namespace tac;
    if (!x || !H || !out || !workspace) return TAC_E_INVALID;
    if (rows <= 0 || h_rows <= 0 || (rows > 1 && stride_r < l_in) || out_stride < l_out) return TAC_E_INVALID;
    FcPlan pl;
    int rc = fc_plan(l_in, m, n_fft, offset, l_out, &pl);
    if (rc != TAC_OK) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return TAC_E_UNSUPPORTED;
    const int64_t fixed = pl.fixed_floats * 4, per_row = pl.per_row_floats * 4;
    if (workspace_bytes < fixed + per_row) return TAC_E_INVALID;
    const int64_t chunk = (workspace_bytes - fixed) / per_row;
    // what the delay line will be given, before anything is launched (X and Y lie in the 16-byte aligned workspace)
    if (mac_check(workspace, H, workspace, chunk < rows ? chunk : rows, pl.T, pl.F, pl.P, h_rows) != TAC_OK) return TAC_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    float* const ones = static_cast<float*>(workspace);
    rc = launch_kernel(fc_fill_kernel, 1, 256, 0, s, ones, pl.N, 1.0f);
    if (rc != TAC_OK) return rc;
    for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
        const int64_t rn = rows - r0 < chunk ? rows - r0 : chunk;
        float* const xp = ones + pl.N;
        float* const X = xp + rn * pl.xp_floats;
        float* const Y = X + round16(rn * pl.spec_floats);
        float* const frames = X;
        // 1. the padded copy: B zeros, the row, zeros up to (T + 1) B
        rc = launch_kernel(fc_pad_kernel, fc_grid(rn * pl.xp_floats), 256, 0, s, x + r0 * (rows > 1 ? stride_r : 0), (long long)stride_r,
                           (long long)l_in, (long long)rn, (long long)pl.B, (long long)pl.xp_floats, xp);
        if (rc != TAC_OK) return rc;
        // 2. X_t: frames at a hop of B, no centre padding, a window of ones: T of them
        tac_stft_desc d{};
        d.rows = rn;
        d.length = d.row_stride = pl.xp_floats;
        d.n_fft = d.win_length = pl.N;
        d.hop = pl.B;
        d.center = 0;
        d.pad_mode = TAC_PAD_CONSTANT;
        d.normalized = 0;
        d.onesided = 1;
        rc = tac_stft_f32(xp, ones, &d, X, stream);
        if (rc != TAC_OK) return rc;
        // 4. the delay line
        rc = launch_spectral_mac(X, H, hrow ? hrow + r0 : nullptr, rn, pl.T, pl.F, pl.P, h_rows, conj, Y, s);
        if (rc != TAC_OK) return rc;
        // 5. irfft of every frame (the frame kernels of tac_istft_f32, window of ones, 1 / N), then the kept halves
        FrameGeom g{};
        g.wave = Y;
        g.row_stride = pl.spec_floats;
        g.length = (long long)pl.B * (pl.T - 1) + pl.N;
        g.window = ones;
        g.win_length = pl.N;
        g.win_offset = 0;
        g.hop = pl.B;
        g.center_pad = pl.B;
        g.pad_mode = TAC_PAD_CONSTANT;
        g.vec2_ok = g.vec4_ok = 0;
        g.n_frames = pl.T;
        g.rows = rn;
        g.scale = (float)(2.0 / (double)pl.N);
        rc = launch_istft_frames(pl.N, g, Y, frames, s);
        if (rc != TAC_OK) return rc;
        rc = launch_kernel(fc_keep_kernel, fc_grid(rn * l_out), 256, 0, s, (const float*)frames, (long long)rn, pl.T, pl.B,
                           (long long)offset, (long long)l_out, (long long)out_stride, out + r0 * out_stride);
        if (rc != TAC_OK) return rc;
    }
    set_last_route("spectral-%d", pl.N);
    return TAC_OK;
}

int tac_fftconvolve_direct_f32(const float* x, int64_t rows, int64_t l_in, int64_t stride_r, const float* bank, const int32_t* table,
                               int64_t m, int64_t offset, int64_t l_out, float* out, void* stream) {
    if (m <= 0 || m > 0x7fffffffLL / 2 || offset < 0 || offset > m - 1 + l_in) return TAC_E_INVALID;
    // one phase at step 1: out[j] = sum_k bank[k] x[j + offset - (m - 1) + k], bank the kernel from its end
    const int32_t off = (int32_t)(offset - (m - 1));
    const int rc = tac_polyphase_f32(x, rows, l_in, stride_r, bank, table, 1, (int32_t)m, (int32_t)m, 1, off, off, l_out, out, stream);
    if (rc == TAC_OK) tac::set_last_route("direct");
    return rc;
}

}  // extern "C"
