// istft.hip — the inverse STFT (the inverse of functional.py:48-113, what torch.istft computes):
//
//   y_t[n]  = irfft_N(X_t)[n] * (sqrt(N) if normalized else 1)
//   num[j]  = sum_t w[j - t hop] y_t[j - t hop]            (0 <= j - t hop < N)
//   env[j]  = sum_t w[j - t hop]^2
//   out[i]  = num[i + pad] / env[i + pad],   i < hop (T - 1) + N - 2 pad — or, with a length, i < min(length, hop (T - 1) + N - pad)
//             (torch.istft slices [pad, pad + length) of the padded positions), zeros from there up to the length
//
// General route, two launches (the fused one-launch route for fft_length 2048 is further down).  (1) The frame kernels of tac_stft_backward_f32 in their inverse operand mode (SRC_INV, fft_core.hpp):
// the adjoint of the one-sided forward transform and irfft are the same C2R transform up to the weight of the DC and Nyquist
// bins and a constant — with C2R(H)[n] = H[0] + H[NC] (-1)^n + 2 Re sum_{0<k<NC} H[k] e^{+2 pi i k n / N},
//     adjoint = (scale / 2) C2R(H),  H[0] = 2 Re G[0], H[NC] = 2 Re G[NC], H[k] = G[k]
//     irfft   = (1 / N)     C2R(H),  H[0] =   Re X[0], H[NC] =   Re X[NC], H[k] = X[k]
// so the inverse mode leaves the two end bins undoubled and the geometry carries scale = 2 / N (times sqrt(N) when
// normalized).  They write the windowed frames [rows][T][N] into the caller's workspace.  (2) istft_ola_kernel gathers every
// output sample from the <= ceil(N / hop) frames covering it, multiplies by 1 / env and writes the zero tail: every output
// element is written, none twice, no atomics.  1 / env depends on the window and the geometry only
// (istft_envelope_kernel, cached by the caller).
// The gradient w.r.t. the spectrum is the forward stft of grad_out / env (zero-extended to the padded length, center = 0
// framing, same window) times per-bin weights — istft_grad_input_kernel and istft_grad_bins_kernel around tac_stft_f32.
#include "host_common.hpp"

#include <cmath>

namespace tac {

int launch_istft_frames(int n_fft, const FrameGeom& g, const float* spec, float* frames, hipStream_t s);   // backward.hip
bool stft_smooth_covers(int n_fft);                                                                         // stft_smooth.hip

namespace {

inline long long grid_for(long long work) { return persistent_blocks(work, 256, (long long)device_cu_count() * 8); }

// env[p] = sum over the frames covering padded position p of w[p - t hop]^2 (accumulated in double: a constant table), and
// its reciprocal.  P = hop (T - 1) + N positions.
__global__ void __launch_bounds__(256)
istft_envelope_kernel(const float* __restrict__ window, int win_length, int win_offset, int n_fft, int hop, int T, int P,
                      float* __restrict__ inv_env, float* __restrict__ env) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        int t1 = p / hop;
        if (t1 > T - 1) t1 = T - 1;
        const int t0 = p - n_fft + 1 <= 0 ? 0 : (p - n_fft + hop) / hop;     // ceil((p - n_fft + 1) / hop)
        double acc = 0.0;
        for (int tt = t0; tt <= t1; ++tt) {
            const int wi = p - tt * hop - win_offset;
            if (wi >= 0 && wi < win_length) {
                const double w = (double)window[wi];
                acc += w * w;
            }
        }
        const float e = (float)acc;
        if (env) env[p] = e;
        inv_env[p] = 1.0f / e;
    }
}

// out[row][j] = inv_env[j + pad] * sum over frames t covering j + pad of frames[row][t][j + pad - t hop] for j < valid,
// 0 for valid <= j < L.  A thread owns four consecutive samples; vec4 (host-checked: hop, pad, n_fft multiples of four,
// `frames` and `inv_env` 16-byte aligned): the same frames cover all four at a 16-byte aligned offset, one 16-byte load per
// covering frame (as overlap_add_kernel, backward.hip).
__global__ void __launch_bounds__(256)
istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ inv_env, float* __restrict__ out,
                 long long out_stride, long long rows, int T, int n_fft, int hop, int pad, int L, int valid, int vec4) {
    const int groups = (L + 3) >> 2;
    const long long total = rows * (long long)groups;
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    typedef float f4a __attribute__((ext_vector_type(4)));
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const long long row = idx / groups;
        const int j0 = 4 * (int)(idx - row * groups);
        const float* fr = frames + row * T * (long long)n_fft;
        float* orow = out + row * out_stride;
        if (vec4 && j0 + 3 < valid) {
            const int p = j0 + pad;                                         // multiple of 4
            int t1 = p / hop;                                               // the same frames cover p .. p + 3
            if (t1 > T - 1) t1 = T - 1;
            const int t0 = p + 3 - n_fft + 1 <= 0 ? 0 : (p + 3 - n_fft + hop) / hop;
            f4a acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int tt = t0; tt <= t1; ++tt) acc += *reinterpret_cast<const f4a*>(fr + (long long)tt * n_fft + (p - tt * hop));
            acc *= *reinterpret_cast<const f4a*>(inv_env + p);
            *reinterpret_cast<f4u*>(orow + j0) = acc;
        } else {
            for (int u = 0; u < 4 && j0 + u < L; ++u) {
                const int j = j0 + u;
                float v = 0.0f;
                if (j < valid) {
                    const int p = j + pad;
                    int t1 = p / hop;
                    if (t1 > T - 1) t1 = T - 1;
                    const int t0 = p - n_fft + 1 <= 0 ? 0 : (p - n_fft + hop) / hop;
                    float acc = 0.0f;
                    for (int tt = t0; tt <= t1; ++tt) acc += fr[(long long)tt * n_fft + (p - tt * hop)];
                    v = acc * inv_env[p];
                }
                orow[j] = v;
            }
        }
    }
}

// padded[row][p] = grad_out[row][p - pad] * inv_env[p] for pad <= p < pad + valid, else 0   (P positions per row)
__global__ void __launch_bounds__(256)
istft_grad_input_kernel(const float* __restrict__ grad_out, long long grad_stride, const float* __restrict__ inv_env,
                        long long rows, int P, int pad, int valid, float* __restrict__ padded) {
    const long long total = rows * (long long)P;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const long long row = idx / P;
        const int p = (int)(idx - row * P);
        const int j = p - pad;
        padded[idx] = (j >= 0 && j < valid) ? grad_out[row * grad_stride + j] * inv_env[p] : 0.0f;
    }
}

// spec[frame][k] *= (scale, 0) for k = 0 and k = NC (irfft ignores their imaginary parts), 2 scale for the bins between
__global__ void __launch_bounds__(256)
istft_grad_bins_kernel(float* __restrict__ spec, long long n_frames_total, int n_bins, float scale) {
    const long long total = n_frames_total * n_bins;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(idx % n_bins);
        const bool end = (k == 0 || k == n_bins - 1);
        cf v = *reinterpret_cast<cf*>(spec + 2 * idx);
        v = end ? mkc(v.x * scale, 0.0f) : mkc(v.x * (2.0f * scale), v.y * (2.0f * scale));
        *reinterpret_cast<cf*>(spec + 2 * idx) = v;
    }
}

// ---------------------------------------------------------------- fused route: fft_length 2048, hop 256 / 512 / 1024, center
// One launch, no frame in memory.  A WAVE owns a segment of consecutive frames of one row: per frame it loads the (k, NC - k)
// pairs of the spectrum row, forms the C2R operands (inverse mode of stft_backward_kernel), runs the 1024-point wave-level
// transform in its LDS exchange area and ADDS the windowed samples into its own ring of N floats in LDS (slot = padded
// position mod N: frame t covers every slot exactly once).  After frame t has been added the run of `hop` positions
// [t hop, (t + 1) hop) is complete — no later frame reaches it — so it leaves, times 1 / env, as 16-byte stores and its slots
// are cleared for the run N positions further on.  Nothing is shared between waves: no barrier, no atomics, no second launch.
// Segment borders: a segment first re-transforms the R = N / hop - 1 frames before its own (their runs are discarded), so every
// run it stores holds all of its frames, added in ascending frame order as the general route's gather does.  The last segment
// of a row also stores the R runs behind the last frame and the zero tail.
constexpr int IF_WAVES = 4;

template <int HOP>
__global__ void __launch_bounds__(IF_WAVES * 64, 2)
istft_fused_kernel(FrameGeom g, Tables tb, const float* __restrict__ spec, const float* __restrict__ inv_env,
                   float* __restrict__ out, long long out_stride, int L, int valid, int seg_frames, int segs_per_row) {
    constexpr int NC = 1024, E = 16, N = 2048, NBINS = NC + 1, R = N / HOP - 1, PAD = N / 2;
    using F = WaveFft<NC, E>;
    static_assert(F::LPF == 64 && F::G == 1, "one frame per wave");
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    typedef float f4a __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int t = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int WAVE_SLOTS = ((F::PADDED + 1) / 2) * 2;
    cf* const lds = reinterpret_cast<cf*>(smem_raw) + w * WAVE_SLOTS;
    float* const ring = reinterpret_cast<float*>(reinterpret_cast<cf*>(smem_raw) + IF_WAVES * WAVE_SLOTS) + w * N;
    constexpr int R0 = radix_at(NC, 0), NB = E / R0;
    const float wscale = 0.5f * g.scale;
    cf tw_h[F::NTW], wk_h[E], win_h[E];
    F::load_twiddles(tw_h, tb.w_nc, t);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < R0; ++q) {
            const int k = t + b * F::LPF + q * (NC / R0);
            const cf wk = tb.w_n[k <= NC / 2 ? k : NC - k];                 // w_{NC-k} = -conj(w_k)
            wk_h[b * R0 + q] = k <= NC / 2 ? wk : mkc(-wk.x, wk.y);
        }
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const cf wn = window_pair(g, t + j * F::LPF);
        win_h[j] = mkc(wn.x * wscale, -wn.y * wscale);                      // (y[2m + 1] = -Im R[m])
    }
    const int T = (int)g.n_frames;
    // run b = padded positions [b HOP, (b + 1) HOP): to the output (times 1 / env, clipped to the kept range) when `store`,
    // and its ring slots cleared either way
    auto leave = [&](int b, bool store, float* orow) {
        for (int c = t; c < HOP / 4; c += 64) {
            const int p = b * HOP + 4 * c;
            f4a* const slot = reinterpret_cast<f4a*>(ring + (p & (N - 1)));
            const f4a a = *slot;
            *slot = f4a{0.0f, 0.0f, 0.0f, 0.0f};
            if (!store) continue;
            const int j = p - PAD;
            if (j >= 0 && j + 3 < valid) {
                *reinterpret_cast<f4u*>(orow + j) = a * *reinterpret_cast<const f4a*>(inv_env + p);
            } else {
                for (int u = 0; u < 4; ++u)
                    if (j + u >= 0 && j + u < valid) orow[j + u] = a[u] * inv_env[p + u];
            }
        }
    };
    const long long total = g.rows * (long long)segs_per_row;
    for (long long unit = (long long)blockIdx.x * IF_WAVES + w; unit < total; unit += (long long)gridDim.x * IF_WAVES) {
        const long long row = unit / segs_per_row;
        const int seg = (int)(unit - row * segs_per_row);
        const int f0 = seg * seg_frames;
        const int f1 = f0 + seg_frames < T ? f0 + seg_frames : T;
        float* const orow = out + row * out_stride;
        for (int c = t; c < N / 4; c += 64) reinterpret_cast<f4a*>(ring)[c] = f4a{0.0f, 0.0f, 0.0f, 0.0f};
        wave_lds_fence();
        for (int f = f0 - R < 0 ? 0 : f0 - R; f < f1; ++f) {
            const cf* G = reinterpret_cast<const cf*>(spec) + (row * T + f) * NBINS;
            cf v[1][E];
            cf* const ldsv[1] = {lds};
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int q = 0; q < R0; ++q) {
                    const int k = t + b * F::LPF + q * (NC / R0);           // first-pass order (fft_core.hpp)
                    cf hk = G[k], hm = G[NC - k];
                    if (b == 0 && q == 0) {
                        if (k == 0) {                                       // irfft takes Re X[0], Re X[NC] once
                            hk = mkc(hk.x, 0.0f);
                            hm = mkc(hm.x, 0.0f);
                        }
                    }
                    v[0][b * R0 + q] = c2r_operand(hk, hm, wk_h[b * R0 + q]);
                }
            F::template run<1>(v, ldsv, tw_h, t);                           // R[] in natural order at lds[lds_pad(i)]
            const int base = f * HOP;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int m = t + j * F::LPF;
                const cf r = lds[lds_pad(m)];
                cf* const a = reinterpret_cast<cf*>(ring + ((base + 2 * m) & (N - 1)));
                const cf prod = mkc(r.x * win_h[j].x, r.y * win_h[j].y);   // the frame value the general route stores
                *a = mkc(a->x + prod.x, a->y + prod.y);
            }
            wave_lds_fence();
            leave(f, f >= f0, orow);
            wave_lds_fence();
        }
        if (seg == segs_per_row - 1) {
            for (int b = T; b < T + R; ++b) leave(b, true, orow);
            for (int j = valid + t; j < L; j += 64) orow[j] = 0.0f;
        }
        wave_lds_fence();
    }
}

// frames per segment and segments per row of the fused route: about one unit per resident wave of the device, no segment
// shorter than four times its R re-transformed frames
void istft_fused_plan(long long rows, int T, int hop, int* seg_frames, int* segs_per_row) {
    const int R = 2048 / hop - 1;
    const int min_seg = 4 * R > 8 ? 4 * R : 8;
    long long want = ((long long)device_cu_count() * 2 * IF_WAVES + rows - 1) / rows;
    long long most = (T + min_seg - 1) / min_seg;
    if (want > most) want = most;
    if (want < 1) want = 1;
    int sf = (int)((T + want - 1) / want);
    *seg_frames = sf;
    *segs_per_row = (T + sf - 1) / sf;
}

bool istft_fused_geometry(const tac_stft_desc* d) {
    return d->n_fft == 2048 && (d->hop == 256 || d->hop == 512 || d->hop == 1024) && d->center && d->onesided &&
           (d->row_stride & 3) == 0;
}

template <int HOP>
int launch_istft_fused(const FrameGeom& g, const Tables& tb, const float* spec, const float* inv_env, float* out,
                       long long out_stride, int L, int valid, hipStream_t s) {
    using F = WaveFft<1024, 16>;
    int seg_frames = 0, segs_per_row = 0;
    istft_fused_plan(g.rows, (int)g.n_frames, HOP, &seg_frames, &segs_per_row);
    const size_t lds_bytes = (size_t)IF_WAVES * ((((F::PADDED + 1) / 2) * 2) * sizeof(cf) + 2048 * sizeof(float));
    const long long units = g.rows * segs_per_row;
    const int rc = launch_kernel(istft_fused_kernel<HOP>, persistent_blocks(units, IF_WAVES, (long long)device_cu_count() * 2), IF_WAVES * 64,
                                 lds_bytes, s, g, tb, spec, inv_env, out, out_stride, L, valid, seg_frames, segs_per_row);
    if (rc != TAC_OK) return rc;
    set_last_route("istft_fused_kernel<%d>", HOP);
    return TAC_OK;
}

bool istft_covers(int n_fft) {
    return (is_pow2(n_fft) && n_fft >= 32 && n_fft <= 4096) || n_fft == 400 || n_fft == 8192 || stft_smooth_covers(n_fft);
}

// validates what the entry points share; *P = padded positions per row, *valid = leading samples of a row the frames determine
int istft_check(const tac_stft_desc* d, int64_t n_frames, int64_t* P, int64_t* valid) {
    if (!d || n_frames <= 0) return TAC_E_INVALID;
    if (d->rows <= 0 || d->length <= 0 || d->hop <= 0 || d->n_fft <= 0 || d->row_stride < d->length) return TAC_E_INVALID;
    if (d->win_length <= 0 || d->win_length > d->n_fft) return TAC_E_INVALID;
    if (!d->onesided || !istft_covers(d->n_fft)) return TAC_E_UNSUPPORTED;
    const int64_t pad = d->center ? d->n_fft / 2 : 0;
    const int64_t p = (int64_t)d->hop * (n_frames - 1) + d->n_fft;
    if (p >= 0x7fffffffLL - 8 || d->length >= 0x7fffffffLL - 8) return TAC_E_UNSUPPORTED;     // 32-bit positions in-kernel
    if (p - 2 * pad <= 0) return TAC_E_SHORT_INPUT;
    *P = p;
    // (torch.istft keeps [pad, pad + length) of the padded positions: a length beyond hop (T - 1) + n_fft - 2 pad reads on into the
    // trailing half frame before the zeros start)
    *valid = p - pad < d->length ? p - pad : d->length;
    return TAC_OK;
}

}  // namespace
}  // namespace tac

extern "C" {

int64_t tac_istft_workspace(const tac_stft_desc* d, int64_t n_frames) {
    int64_t P = 0, valid = 0;
    const int rc = tac::istft_check(d, n_frames, &P, &valid);
    if (rc != TAC_OK) return rc;
    if (tac::istft_fused_geometry(d)) return 0;             // one launch, nothing in memory between the transform and the output
    return d->rows * n_frames * (int64_t)d->n_fft * (int64_t)sizeof(float);
}

int tac_istft_envelope_f32(const float* window, const tac_stft_desc* d, int64_t n_frames, float* inv_env, float* env,
                           void* stream) {
    if (!window || !inv_env) return TAC_E_INVALID;
    int64_t P = 0, valid = 0;
    const int rc = tac::istft_check(d, n_frames, &P, &valid);
    if (rc != TAC_OK) return rc;
    return tac::launch_kernel(tac::istft_envelope_kernel, tac::grid_for(P), 256, 0, (hipStream_t)stream, window, d->win_length,
                              (d->n_fft - d->win_length) / 2, d->n_fft, d->hop, (int)n_frames, (int)P, inv_env, env);
}

int tac_istft_f32(const float* spec, int64_t stride_r, int64_t stride_t, int64_t n_frames, const float* window,
                  const float* inv_env, const tac_stft_desc* d, void* workspace, int64_t workspace_bytes, float* out,
                  void* stream) {
    if (!spec || !window || !inv_env || !out) return TAC_E_INVALID;
    int64_t P = 0, valid = 0;
    const int rc = tac::istft_check(d, n_frames, &P, &valid);
    if (rc != TAC_OK) return rc;
    const int64_t row_floats = 2 * (int64_t)(d->n_fft / 2 + 1);
    // the frame kernels address dense frame-major rows; any other layout is the caller's to copy
    if (stride_t != row_floats || (d->rows > 1 && stride_r != n_frames * row_floats)) return TAC_E_UNSUPPORTED;
    const int64_t need = d->rows * n_frames * (int64_t)d->n_fft * (int64_t)sizeof(float);
    // no workspace: the fused route (where tac_istft_workspace returns 0).  A workspace of rows x T x n_fft floats selects the
    // general route for any geometry.
    const bool fused = workspace == nullptr;
    if (fused && !tac::istft_fused_geometry(d)) return TAC_E_INVALID;
    if (!fused && workspace_bytes < need) return TAC_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(spec) & 7u) || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return TAC_E_UNSUPPORTED;
    if (fused && ((reinterpret_cast<uintptr_t>(out) & 15u) || (reinterpret_cast<uintptr_t>(inv_env) & 15u))) return TAC_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    float* frames = static_cast<float*>(workspace);
    tac::FrameGeom g{};
    g.wave = spec;
    g.row_stride = n_frames * row_floats;
    g.length = P;
    g.window = window;
    g.win_length = d->win_length;
    g.win_offset = (d->n_fft - d->win_length) / 2;
    g.hop = d->hop;
    g.center_pad = d->center ? d->n_fft / 2 : 0;
    g.pad_mode = TAC_PAD_CONSTANT;
    g.vec2_ok = g.vec4_ok = 0;
    g.n_frames = n_frames;
    g.rows = d->rows;
    g.scale = (float)((d->normalized ? std::sqrt((double)d->n_fft) : 1.0) * 2.0 / (double)d->n_fft);
    if (fused) {
        tac::Tables tb;
        const int rt = tac::get_tables(2048, &tb);
        if (rt != TAC_OK) return rt;
        switch (d->hop) {
            case 256: return tac::launch_istft_fused<256>(g, tb, spec, inv_env, out, d->row_stride, (int)d->length, (int)valid, s);
            case 512: return tac::launch_istft_fused<512>(g, tb, spec, inv_env, out, d->row_stride, (int)d->length, (int)valid, s);
            default: return tac::launch_istft_fused<1024>(g, tb, spec, inv_env, out, d->row_stride, (int)d->length, (int)valid, s);
        }
    }
    const int rf = tac::launch_istft_frames(d->n_fft, g, spec, frames, s);
    if (rf != TAC_OK) return rf;
    const int vec4 = (d->hop % 4 == 0) && (g.center_pad % 4 == 0) && (d->n_fft % 4 == 0) &&
                     (reinterpret_cast<uintptr_t>(inv_env) & 15u) == 0;
    const long long work = d->rows * ((d->length + 3) / 4);
    const int ro = tac::launch_kernel(tac::istft_ola_kernel, tac::grid_for(work), 256, 0, s, frames, inv_env, out, (long long)d->row_stride,
                                      (long long)d->rows, (int)n_frames, d->n_fft, d->hop, g.center_pad, (int)d->length, (int)valid, vec4);
    if (ro != TAC_OK) return ro;
    tac::set_last_route("istft_general<%d>: frame kernel (inverse mode) + istft_ola_kernel<vec4=%d>", d->n_fft, vec4);
    return TAC_OK;
}

int tac_istft_grad_input_f32(const float* grad_out, int64_t grad_stride, const float* inv_env, const tac_stft_desc* d,
                             int64_t n_frames, float* padded, void* stream) {
    if (!grad_out || !inv_env || !padded) return TAC_E_INVALID;
    int64_t P = 0, valid = 0;
    const int rc = tac::istft_check(d, n_frames, &P, &valid);
    if (rc != TAC_OK) return rc;
    if (grad_stride < d->length) return TAC_E_INVALID;
    return tac::launch_kernel(tac::istft_grad_input_kernel, tac::grid_for(d->rows * P), 256, 0, (hipStream_t)stream, grad_out,
                              (long long)grad_stride, inv_env, (long long)d->rows, (int)P, d->center ? d->n_fft / 2 : 0, (int)valid, padded);
}

int tac_istft_grad_bins_f32(float* spec, int64_t n_frames_total, int n_fft, int normalized, void* stream) {
    if (!spec || n_frames_total <= 0 || n_fft <= 0 || (n_fft & 1)) return TAC_E_INVALID;
    const float scale = (float)((normalized ? std::sqrt((double)n_fft) : 1.0) / (double)n_fft);
    return tac::launch_kernel(tac::istft_grad_bins_kernel, tac::grid_for(n_frames_total * (n_fft / 2 + 1)), 256, 0, (hipStream_t)stream,
                              spec, (long long)n_frames_total, n_fft / 2 + 1, scale);
}

}  // extern "C"
