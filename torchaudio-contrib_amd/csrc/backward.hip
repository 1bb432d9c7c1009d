// backward.hip — gradient kernels of the path.  The reference differentiates through stock
// torch ops (functional.py:99-107 stft, :126-128 norm/pow, :183-184 matmul, :291-296 dB); these are the adjoints
// of this library's forward kernels, written against the same frame-major layouts:
//
//   tac_stft_backward_f32        g_spec[rows][T][F][2] -> windowed frame gradients [rows][T][N]: per frame one inverse
//                                real FFT of the one-sided gradient spectrum (the C2R form of the forward R2C split,
//                                evaluated with the SAME wave-level forward FFT on conjugated data), times the window.
//   tac_overlap_add_f32          frame gradients -> g_wave[rows][L]: the adjoint of framing + padding as a GATHER
//                                (every output sample sums the <= 3 padded positions that map to it over the frames
//                                covering them), so it is deterministic and needs no atomics.
//   tac_stft_norm_backward_f32 / tac_spectrogram_backward_f32   the same kernel forming the gradient spectrum on load —
//                                from the spectrum and the gradient of |z|^p, or with the spectrum itself recomputed
//                                from the waveform inside the kernel (nothing but 4·F bytes of gradient read per frame).
//   tac_spectrogram_backward_ola_f32   fft_length 2048, hop = 128·H: that kernel with the overlap-add in an LDS ring
//                                over segments of consecutive frames + ola_fold_kernel (unpadding, segment borders):
//                                the whole adjoint of Spectrogram with no per-frame data in memory.
//   tac_complex_norm_backward_f32, tac_magphase_backward_f32, tac_amplitude_to_db_backward_f32, tac_db_to_amplitude_backward_f32   elementwise.
//   tac_apply_filterbank_adjoint_f32   the filterbank stage's adjoint for banks with <= 2 non-zero weights per bin (mel
//                                banks); other banks: the forward GEMM with the transposed matrix (tac_apply_filterbank_f32).
#include "host_common.hpp"
#include "ola_plan.hpp"
#include "ola_runs.hpp"

#include <algorithm>
#include <cstdio>
#include <type_traits>

namespace tac {

int launch_n400_backward(const FrameGeom& g, const float* gspec, const float* gnorm, float power, float* frames,
                         hipStream_t stream, bool from_wave, const AdjEntry* adj = nullptr, int n_mels = 0, float* gpad = nullptr,
                         float* edge = nullptr, const OlaPlan* plan = nullptr, bool inverse = false);     // stft_n400.hip

constexpr int BW_WAVES = 4;

// One frame (group) per wave-iteration.  y[n] = Re sum_{k=0}^{N/2} G[k] e^{+2 pi i k n / N}:
//   H[k] = G[k] (0 < k < NC), H[0] = 2 Re G[0], H[NC] = 2 Re G[NC]            (the common 1/2 is folded into the window)
//   conj(Z[k]) = (conj(H[k]) + H[NC-k]) - i w_k (conj(H[k]) - H[NC-k]),  w_k = e^{-2 pi i k / N}
//   R = FFT_NC(conj Z);  y[2m] = Re R[m],  y[2m+1] = -Im R[m].
// (norm_pow_grad and c2r_operand: fft_core.hpp, shared with the fft_length-400 form in stft_n400.hip)
// SRC_NORM: `gspec` is the spectrum z itself and `gnorm` the gradient of |z|^power: the gradient spectrum
// gnorm * d|z|^power/dz is formed on load (tac_stft_norm_backward_f32: the adjoint of Spectrogram in one pass, no
// gradient spectrum in memory).
// SRC_WAVE: there is no spectrum in memory either — the frame is fetched from the WAVEFORM (g.wave), windowed and
// transformed by the same wave-level FFT, z[k] is formed from the exchange area by the R2C split as the inverse's operands
// are gathered, and the inverse FFT then runs in the same buffer (tac_spectrogram_backward_f32: per frame 4·hop bytes of
// samples + 4·F of gradient in, 4·N of frame gradient out; the recomputation costs one FFT and saves writing and reading
// 8·F bytes of spectrum per frame plus a launch).

// POW2: power == 2 (the Melspectrogram chain, layers.py:335): the adjoint's factor is the constant 2
template <int NC, int E, int SRC, bool POW2>
__global__ void __launch_bounds__(BW_WAVES * 64, 2)
stft_backward_kernel(FrameGeom g, Tables tb, const float* __restrict__ gspec, const float* __restrict__ gnorm, float power,
                     float* __restrict__ frames) {
    using F = WaveFft<NC, E>;
    constexpr bool NORM = (SRC == SRC_NORM || SRC == SRC_WAVE);
    constexpr int N = 2 * NC, NBINS = NC + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane / F::LPF;
    const int t = lane % F::LPF;
    constexpr int WAVE_SLOTS = ((F::G * F::PADDED + 1) / 2) * 2;
    cf* lds = reinterpret_cast<cf*>(smem_raw) + w * WAVE_SLOTS + sub * F::PADDED;
    // SRC_WAVE: the window pairs and the R2C / C2R twiddles w_k (k <= NC/2) live in LDS behind the exchange areas — the
    // kernel reads each of them twice per frame, and as global (L1 / L2) loads they were most of a frame's latency
    cf* const win_lds = reinterpret_cast<cf*>(smem_raw) + BW_WAVES * WAVE_SLOTS;
    cf* const wk_lds = win_lds + NC;
    if constexpr (SRC == SRC_WAVE) {
        for (int m = threadIdx.x; m < NC; m += BW_WAVES * 64) win_lds[m] = window_pair(g, m);
        for (int k = threadIdx.x; k <= NC / 2; k += BW_WAVES * 64) wk_lds[k] = tb.w_n[k];
        __syncthreads();
    }

    const long long groups_per_row = (g.n_frames + F::G - 1) / F::G;
    const long long total = g.rows * groups_per_row;
    const float wscale = 0.5f * g.scale;
    constexpr int R0 = radix_at(NC, 0), NB = E / R0;
    // lane-dependent tables stay in registers for the kernel's lifetime where they fit (16 elements per lane): the FFT's
    // inter-pass twiddles, the C2R twiddles of the lane's sixteen (k, NC - k) pairs, its sixteen window pairs
    constexpr bool HOIST = (E == 16);
    constexpr bool HOIST_WIN = HOIST && !NORM;             // (the NORM form keeps 32 more loads in flight per frame)
    constexpr bool HOIST_WK = HOIST && SRC != SRC_WAVE;    // (the forward transform's window needs those registers)
    cf tw_h[HOIST ? F::NTW : 1], wk_h[HOIST_WK ? E : 1], win_h[HOIST_WIN ? E : 1];
    if constexpr (HOIST) F::load_twiddles(tw_h, tb.w_nc, t);
    if constexpr (HOIST_WK) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const int k = t + b * F::LPF + q * (NC / R0);
                const cf wk = tb.w_n[k <= NC / 2 ? k : NC - k];            // w_{NC-k} = -conj(w_k)
                wk_h[b * R0 + q] = k <= NC / 2 ? wk : mkc(-wk.x, wk.y);
            }
    }
    if constexpr (HOIST) {
        if constexpr (HOIST_WIN) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const cf wn = window_pair(g, t + j * F::LPF);
                win_h[j] = mkc(wn.x * wscale, -wn.y * wscale);
            }
        }
    }
    // SRC_WAVE: the next unit's samples (raw, unwindowed) and gradient row are requested while this unit's inverse
    // transform runs — neither HBM round trip opens a frame
    cf raw[SRC == SRC_WAVE ? E : 1];
    float gk[SRC == SRC_WAVE ? E : 1], gm[SRC == SRC_WAVE ? E : 1];
    bool pre = false;
    // (Every load is issued unconditionally, from a clamped address where the unit does not exist or its frame touches the
    // padding: a conditional request would keep the previous unit's 64 registers alive through the whole iteration.)
    const bool can_prefetch = g.vec2_ok && g.length >= N;                   // wave-uniform
    auto request = [&](long long u) {
        if constexpr (SRC == SRC_WAVE) {
            const long long uu = u < total ? u : total - 1;
            const long long r = uu / groups_per_row;
            const long long f = (uu - r * groups_per_row) * F::G + sub;
            const bool lv = f < g.n_frames;
            const float* gn = gnorm + (r * g.n_frames + (lv ? f : 0)) * NBINS;
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int q = 0; q < R0; ++q) {
                    const int k = t + b * F::LPF + q * (NC / R0);
                    gk[b * R0 + q] = gn[k];
                    gm[b * R0 + q] = gn[NC - k];
                }
            const long long start = f * (long long)g.hop - g.center_pad;
            bool ok = can_prefetch && lv && start >= 0 && start + N <= g.length;
            if constexpr (F::G > 1) ok = __builtin_amdgcn_ballot_w64(ok) == ~0ull;      // all of the wave's frames or none
            const cf* src = reinterpret_cast<const cf*>(g.wave + r * g.row_stride + (ok ? start : 0));
            if (can_prefetch) {
#pragma unroll
                for (int q = 0; q < E; ++q) raw[q] = src[t + q * F::LPF];
            } else {
#pragma unroll
                for (int q = 0; q < E; ++q) raw[q] = mkc(0.0f, 0.0f);
            }
            pre = ok;
        }
    };
    const long long stride = (long long)gridDim.x * BW_WAVES;
    request((long long)blockIdx.x * BW_WAVES + w);
    for (long long unit = (long long)blockIdx.x * BW_WAVES + w; unit < total; unit += stride) {
        const long long row = unit / groups_per_row;
        const long long frame = (unit - row * groups_per_row) * F::G + sub;
        const bool live = frame < g.n_frames;
        const cf* G = reinterpret_cast<const cf*>(gspec) + (row * g.n_frames + (live ? frame : 0)) * NBINS;
        const float* GN = NORM ? gnorm + (row * g.n_frames + (live ? frame : 0)) * NBINS : nullptr;
        cf tw_l[HOIST ? 1 : F::NTW];
        if constexpr (!HOIST) F::load_twiddles(tw_l, tb.w_nc, t);
        const cf* const tw = HOIST ? tw_h : tw_l;
        cf v[1][E];
        cf* const ldsv[1] = {lds};
        if constexpr (SRC == SRC_WAVE) {
            // forward transform of this frame: Z (the FFT of the packed real frame) in natural order in the exchange area
            int tl = t;
            asm volatile("" : "+v"(tl));          // launder: the window reads stay inside the loop (register budget)
            cf win[E];
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int q = 0; q < R0; ++q) win[b * R0 + q] = win_lds[tl + b * F::LPF + q * (NC / R0)];
            if (pre) apply_window<F>(v[0], raw, win);
            else load_frame<F, true>(v[0], g, win, lds, row, live ? frame : g.n_frames, t);  // edge frames; past the end: zeros
            F::template run<1>(v, ldsv, tw, t);
        }
        const float xscale = 0.5f * g.scale;                                               // the R2C split returns 2·X
        int tg = t;
        // SRC_WAVE: the operand addresses (twiddle table, exchange area) are recomputed from an opaque copy of the lane
        // number every iteration — as loop invariants they would occupy (and spill) 48 registers
        if constexpr (SRC == SRC_WAVE) asm volatile("" : "+v"(tg));
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const int k = tg + b * F::LPF + q * (NC / R0);             // first-pass order (fft_core.hpp)
                cf wkk;
                if constexpr (HOIST_WK) {
                    wkk = wk_h[b * R0 + q];
                } else {
                    const int kt = k <= NC / 2 ? k : NC - k;                // w_{NC-k} = -conj(w_k)
                    const cf wk = (SRC == SRC_WAVE) ? wk_lds[kt] : tb.w_n[kt];
                    wkk = k <= NC / 2 ? wk : mkc(-wk.x, wk.y);
                }
                cf hk, hm;
                if constexpr (SRC == SRC_WAVE) {
                    F::r2c_pair(lds, k, wkk, hk, hm);                       // 2·z[k], 2·z[NC-k] of this frame
                    hk = cscale(hk, xscale);
                    hm = cscale(hm, xscale);
                } else {
                    hk = G[k];
                    hm = G[NC - k];
                }
                if constexpr (SRC == SRC_WAVE) {
                    hk = norm_pow_grad<POW2>(hk, gk[b * R0 + q], power);
                    hm = norm_pow_grad<POW2>(hm, gm[b * R0 + q], power);
                } else if constexpr (NORM) {
                    hk = norm_pow_grad<POW2>(hk, GN[k], power);
                    hm = norm_pow_grad<POW2>(hm, GN[NC - k], power);
                }
                if (b == 0 && q == 0) {                                    // (k == 0 can only be the lane's first element)
                    if (k == 0) {
                        constexpr float ends = (SRC == SRC_INV) ? 1.0f : 2.0f;   // irfft takes Re X[0], Re X[NC] once
                        hk = mkc(ends * hk.x, 0.0f);
                        hm = mkc(ends * hm.x, 0.0f);
                    }
                }
                if (!live) hk = hm = mkc(0.0f, 0.0f);
                v[0][b * R0 + q] = c2r_operand(hk, hm, wkk);
                // (eight pairs' exchange-area reads in flight at a time: all sixteen at once no longer fit the registers; the
                // empty asm pins each operand's arithmetic here — LLVM's IR passes otherwise sink it below the barrier)
                if constexpr (SRC == SRC_WAVE) {
                    asm volatile("" : "+v"(v[0][b * R0 + q]));
                    if ((q & 7) == 7) __builtin_amdgcn_sched_barrier(0);
                }
            }
        if constexpr (SRC == SRC_WAVE) {
            wave_lds_fence();                                               // every Z read precedes the inverse's first writes
            __builtin_amdgcn_sched_barrier(0);
            request(unit + stride);
            __builtin_amdgcn_sched_barrier(0);
        }
        F::template run<1>(v, ldsv, tw, t);                                 // R[] in natural order at lds[lds_pad(i)]
        float* out = frames + (row * g.n_frames + frame) * N;
        if (live) {
            if constexpr (HOIST_WIN) {
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    const int m = t + j * F::LPF;
                    const cf r = lds[lds_pad(m)];
                    *reinterpret_cast<cf*>(out + 2 * m) = mkc(r.x * win_h[j].x, r.y * win_h[j].y);
                }
            } else {
#pragma unroll 4
                for (int m = t; m < NC; m += F::LPF) {
                    const cf r = lds[lds_pad(m)];
                    const cf wn = (SRC == SRC_WAVE) ? win_lds[m] : window_pair(g, m);
                    *reinterpret_cast<cf*>(out + 2 * m) = mkc(r.x * wn.x * wscale, -r.y * wn.y * wscale);
                }
            }
        }
        wave_lds_fence();
    }
}

// ---------------------------------------------------------------- Spectrogram backward with the overlap-add in LDS
// fft_length 2048, hop a multiple of 128 (tac_spectrogram_backward_ola_f32).  The kernel above writes 4·N bytes of frame
// gradient per frame and overlap_add_kernel reads them back: 16 of the 20 bytes per sample the pair moves.  Here a wave
// walks a SEGMENT of consecutive frames of one row and keeps the running overlap-add of the last N positions in a ring
// in LDS: after frame f is added, positions [f·hop, (f+1)·hop) of the padded signal are complete and leave for
// gpad[row][·]; the slots they occupied take the next frame's newest positions.  hop = 128·H makes the position class
// of an output (complete / still open / new) a function of the register index j alone, and the ring slot a rotation
// of it.  Segment borders: a segment's first N - hop positions miss the previous segment's last frames — that
// segment writes what it has for them (its ring at the end) to edge[row][segment][·] and ola_fold_kernel, which maps
// the padded gradient back onto the waveform (reflect / replicate / circular images), adds the two partial sums:
// every value has exactly one writer, no atomics, deterministic.
constexpr int OLA_WAVES = 4;
constexpr int OLA_NC = 1024, OLA_E = 16, OLA_N = 2048;

// FUSE: `gnorm` is the gradient of the MEL values, (rows, T, n_mels) frame-major, and the filterbank adjoint
// (grad_mel . fb^T, two multiply-adds per bin through `adj`) happens here, per frame, out of a 16 KB LDS table: the
// 4 F bytes per frame of gradient spectrogram that fb_adjoint_kernel writes and this kernel reads back never exist.
// What makes room for the table is the ring: of a frame's 16 chunks of 128 samples the first H = hop / 128 complete at once,
// so 16 - H slots are ever live (plan.ring_slots; 16 in the unfused form, whose two 4-wave workgroups per CU do not share tables).
struct OlaFuse {
    const AdjEntry* adj;   // [n_freqs]
    int n_mels;            // <= 256
    int mel_stride;        // floats per wave of mel-gradient row in LDS (n_mels rounded up to 64)
    int ring_slots;        // R
};

template <bool POW2, bool FUSE, int WAVES>
__global__ void __launch_bounds__(WAVES * 64, 2)
spectrogram_backward_ola_kernel(FrameGeom g, Tables tb, const float* __restrict__ gnorm, float power,
                                float* __restrict__ gpad, float* __restrict__ edge, OlaPlan plan, OlaFuse fz) {
    using F = WaveFft<OLA_NC, OLA_E>;
    constexpr int NC = OLA_NC, E = OLA_E, N = OLA_N, NBINS = NC + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int t = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int WAVE_SLOTS = ((F::PADDED + 1) / 2) * 2;
    cf* const lds = reinterpret_cast<cf*>(smem_raw) + w * WAVE_SLOTS;
    const int R = fz.ring_slots;
    cf* const ring = reinterpret_cast<cf*>(smem_raw) + WAVES * WAVE_SLOTS + w * (R << 6);   // R slots of 64 sample pairs per wave
    cf* const win_lds = reinterpret_cast<cf*>(smem_raw) + WAVES * (WAVE_SLOTS + (R << 6));
    cf* const wk_lds = win_lds + NC;
    // FUSE: the per-bin adjoint table (16-byte entries) and one mel-gradient row per wave behind the twiddles
    const AdjEntry* const adj_lds = reinterpret_cast<const AdjEntry*>(wk_lds + NC / 2 + 2);
    float* const grow = reinterpret_cast<float*>(const_cast<AdjEntry*>(adj_lds) + NBINS) + w * fz.mel_stride;
    if constexpr (FUSE)
        for (int k = threadIdx.x; k < NBINS; k += WAVES * 64) const_cast<AdjEntry*>(adj_lds)[k] = fz.adj[k];
    for (int m = threadIdx.x; m < NC; m += WAVES * 64) win_lds[m] = window_pair(g, m);
    for (int k = threadIdx.x; k <= NC / 2; k += WAVES * 64) wk_lds[k] = tb.w_n[k];
    __syncthreads();

    const int T = (int)g.n_frames, hop = g.hop, H = hop >> 7, S = plan.seg_frames, spr = plan.segs_per_row;
    const long long nseg_total = g.rows * (long long)spr;
    const long long stride = (long long)gridDim.x * WAVES;
    const float wscale = 0.5f * g.scale, xscale = 0.5f * g.scale;
    cf tw[F::NTW];
    F::load_twiddles(tw, tb.w_nc, t);

    long long seg = (long long)blockIdx.x * WAVES + w;
    if (seg >= nseg_total) return;
    int row = (int)(seg / spr), sidx = (int)(seg - (long long)row * spr);
    int f0 = sidx * S, f1 = f0 + S < T ? f0 + S : T, f = f0;

    cf raw[E];
    float gk[E], gm[E];
    float gq[4];                                            // FUSE: the frame's mel-gradient row, 64 bands per register
    bool pre = false;
    const bool can_prefetch = g.vec2_ok && g.length >= N;
    auto request = [&](int r, int fr) {                     // samples + gradient row of (row r, frame fr), unconditionally
        if constexpr (FUSE) {
            const float* gn = gnorm + ((long long)r * T + fr) * fz.n_mels;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b = t + 64 * i;
                gq[i] = gn[b < fz.n_mels ? b : fz.n_mels - 1];
            }
        } else {
            const float* gn = gnorm + ((long long)r * T + fr) * NBINS;
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int k = t + q * (NC / E);
                gk[q] = gn[k];
                gm[q] = gn[NC - k];
            }
        }
        const long long start = (long long)fr * hop - g.center_pad;
        const bool ok = can_prefetch && start >= 0 && start + N <= g.length;
        const cf* src = reinterpret_cast<const cf*>(g.wave + r * g.row_stride + (ok ? start : 0));
        if (can_prefetch) {
#pragma unroll
            for (int q = 0; q < E; ++q) raw[q] = src[t + q * F::LPF];
        } else {
#pragma unroll
            for (int q = 0; q < E; ++q) raw[q] = mkc(0.0f, 0.0f);
        }
        pre = ok;
    };
    request(row, f);
    int rot = 0;
    while (true) {
        // the item after this one: next frame of the segment, or the first frame of this wave's next segment
        long long nseg = seg;
        int nrow = row, nsidx = sidx, nf0 = f0, nf1 = f1, nf = f + 1;
        bool more = true;
        if (nf >= f1) {
            nseg = seg + stride;
            if (nseg >= nseg_total) {
                more = false;
                nf = f;
            } else {
                nrow = (int)(nseg / spr);
                nsidx = (int)(nseg - (long long)nrow * spr);
                nf0 = nsidx * S;
                nf1 = nf0 + S < T ? nf0 + S : T;
                nf = nf0;
            }
        }
        const bool first = (f == f0), last = (f + 1 == f1);

        // ---- forward transform of the frame
        cf v[1][E];
        cf* const ldsv[1] = {lds};
        {
            int tl = t;
            asm volatile("" : "+v"(tl));
            cf win[E];
#pragma unroll
            for (int q = 0; q < E; ++q) win[q] = win_lds[tl + q * (NC / E)];
            if (pre) apply_window<F>(v[0], raw, win);
            else load_frame<F, true>(v[0], g, win, lds, row, f, t);
            F::template run<1>(v, ldsv, tw, t);
        }
        // ---- gradient spectrum -> operands of the inverse transform (see stft_backward_kernel)
        int tg = t;
        asm volatile("" : "+v"(tg));
        if constexpr (FUSE) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (tg + 64 * i < fz.n_mels) grow[tg + 64 * i] = gq[i];
            wave_lds_fence();
        }
#pragma unroll
        for (int q = 0; q < E; ++q) {
            const int k = tg + q * (NC / E);
            const int kt = k <= NC / 2 ? k : NC - k;
            const cf wk = wk_lds[kt];
            const cf wkk = k <= NC / 2 ? wk : mkc(-wk.x, wk.y);
            cf hk, hm;
            F::r2c_pair(lds, k, wkk, hk, hm);
            float gkq, gmq;
            if constexpr (FUSE) {                                           // (grad_mel . fb^T)[k], [NC - k]
                const AdjEntry ek = adj_lds[k], em = adj_lds[NC - k];
                gkq = __builtin_fmaf(ek.w0, grow[ek.b0], ek.w1 * grow[ek.b1]);
                gmq = __builtin_fmaf(em.w0, grow[em.b0], em.w1 * grow[em.b1]);
            } else {
                gkq = gk[q];
                gmq = gm[q];
            }
            hk = norm_pow_grad<POW2>(cscale(hk, xscale), gkq, power);
            hm = norm_pow_grad<POW2>(cscale(hm, xscale), gmq, power);
            if (q == 0) {
                if (k == 0) {
                    hk = mkc(2.0f * hk.x, 0.0f);
                    hm = mkc(2.0f * hm.x, 0.0f);
                }
            }
            v[0][q] = c2r_operand(hk, hm, wkk);
            asm volatile("" : "+v"(v[0][q]));
            if ((q & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
        wave_lds_fence();
        __builtin_amdgcn_sched_barrier(0);
        request(nrow, nf);
        __builtin_amdgcn_sched_barrier(0);
        F::template run<1>(v, ldsv, tw, t);                 // R[] in natural order at lds[lds_pad(i)]

        // ---- windowed frame gradient into the ring; complete positions out
        // slot of chunk j = (j + rot) mod R; rot advances by H per frame of the segment (only differences within a segment matter)
        // (wave-uniform; ola_direct() with the segment already known: no division)
        bool direct = false;
        if (plan.direct && (sidx == 0 || (f - f0) * hop >= N - hop)) {
            const int jlo = f * hop - g.center_pad, jhi = jlo + hop - 1, L = (int)g.length;
            direct = (g.center_pad == 0 || g.pad_mode == PAD_CONSTANT) ? (jlo >= 0 && jhi < L)
                                                                      : (jlo > g.center_pad && jhi < L - 1 - g.center_pad);
        }
        float* const prow = gpad + (long long)row * plan.pad_len + (long long)f * hop;           // position f·hop
        float* const drow = direct ? plan.gwave + (long long)row * plan.gstride + ((long long)f * hop - g.center_pad) : prow;
        const bool row_end = (f1 == T);
        float* const tail = row_end ? prow : edge + ((long long)row * (spr - 1) + sidx) * (N - hop) - hop;   // + n
        int sl = rot;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int m = t + j * 64;                                       // samples n = 2m, 2m + 1 of the frame
            const cf r = lds[lds_pad(m)];
            const cf wn = win_lds[m];
            cf acc = cmul_elem(cmul_elem(r, wn), mkc(wscale, -wscale));     // (Re, -Im) R[m] · window / 2
            cf* const slot = ring + (sl << 6) + t;
            sl = sl + 1 == R ? 0 : sl + 1;
            if (!(first || j >= 16 - H)) {
                const cf old = *slot;
                acc = cadd(acc, old);
            }
            if (j < H) *reinterpret_cast<cf*>(drow + 2 * m) = acc;          // complete (clean interior: the waveform gradient itself)
            else if (last) *reinterpret_cast<cf*>(tail + 2 * m) = acc;      // the segment's open positions
            else *slot = acc;
        }
        wave_lds_fence();
        if (!more) break;
        rot = (nf == nf0) ? 0 : rot + H;
        while (rot >= R) rot -= R;
        seg = nseg; row = nrow; sidx = nsidx; f0 = nf0; f1 = nf1; f = nf;
    }
}

}  // namespace tac
#include "backward_ring3_multi.hpp"
namespace tac {

// The same for fft_length 256 / 512 / 1024, where a wave carries G = 64 / LPF frames side by side: its G lane groups walk G
// different SEGMENTS (each with its own ring), so nothing in the ring update crosses lane groups; hop is a multiple of
// 2·LPF = n_fft / 16.  A group whose segment is shorter than its neighbours' idles (recomputes, stores nothing) until the
// longest is done.  Frame, row and the "last frame of the segment" flag are per lane here, so this form has no
// one-frame-ahead requests and more predication than the fft_length 2048 kernel above.
template <int NC, bool POW2>
__global__ void __launch_bounds__(OLA_WAVES * 64, 2)
spectrogram_backward_ola_multi_kernel(FrameGeom g, Tables tb, const float* __restrict__ gnorm, float power,
                                      float* __restrict__ gpad, float* __restrict__ edge, OlaPlan plan) {
    using F = WaveFft<NC, OLA_E>;
    constexpr int E = OLA_E, N = 2 * NC, NBINS = NC + 1, G = F::G, LPF = F::LPF;
    static_assert(G > 1 && radix_at(NC, 0) == E, "several frames per wave, one first-pass butterfly per lane");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = lane / LPF, t = lane % LPF;
    constexpr int WAVE_SLOTS = ((G * F::PADDED + 1) / 2) * 2;
    cf* const lds = reinterpret_cast<cf*>(smem_raw) + w * WAVE_SLOTS + sub * F::PADDED;
    cf* const ring = reinterpret_cast<cf*>(smem_raw) + OLA_WAVES * WAVE_SLOTS + (w * G + sub) * NC;   // N floats per stream
    cf* const win_lds = reinterpret_cast<cf*>(smem_raw) + OLA_WAVES * (WAVE_SLOTS + G * NC);
    cf* const wk_lds = win_lds + NC;
    for (int m = threadIdx.x; m < NC; m += OLA_WAVES * 64) win_lds[m] = window_pair(g, m);
    for (int k = threadIdx.x; k <= NC / 2; k += OLA_WAVES * 64) wk_lds[k] = tb.w_n[k];
    __syncthreads();

    const int T = (int)g.n_frames, hop = g.hop, H = hop / (2 * LPF), S = plan.seg_frames, spr = plan.segs_per_row;
    const long long nseg_total = g.rows * (long long)spr;
    const long long ngroups = (nseg_total + G - 1) / G;
    const float wscale = 0.5f * g.scale, xscale = 0.5f * g.scale;
    cf tw[F::NTW];
    F::load_twiddles(tw, tb.w_nc, t);
    cf* const ldsv[1] = {lds};

    for (long long gi = (long long)blockIdx.x * OLA_WAVES + w; gi < ngroups; gi += (long long)gridDim.x * OLA_WAVES) {
        const long long seg = gi * G + sub;
        const bool seg_ok = seg < nseg_total;
        const long long segc = seg_ok ? seg : nseg_total - 1;
        const int row = (int)(segc / spr), sidx = (int)(segc - (long long)row * spr);
        const int f0 = sidx * S, f1 = f0 + S < T ? f0 + S : T;
        const int len_lane = seg_ok ? f1 - f0 : 0;
        int len = 0;                                                       // the longest of the wave's segments
#pragma unroll
        for (int s2 = 0; s2 < G; ++s2) {
            const int l2 = __builtin_amdgcn_readlane(len_lane, s2 * LPF);
            len = l2 > len ? l2 : len;
        }
        const bool row_end = (f1 == T);
        for (int i = 0; i < len; ++i) {
            const bool live = i < len_lane, last = (i + 1 == len_lane), first = (i == 0);
            const int f = live ? f0 + i : f0;
            // the frame's gradient row is requested first: its HBM round trip runs behind the forward transform
            const float* gn = gnorm + ((long long)row * T + f) * NBINS;
            float gk[E], gm[E];
#pragma unroll
            for (int q = 0; q < E; ++q) {
                gk[q] = gn[t + q * (NC / E)];
                gm[q] = gn[NC - t - q * (NC / E)];
            }
            // ---- forward transform of the frame
            cf v[1][E];
            {
                int tl = t;
                asm volatile("" : "+v"(tl));
                cf win[E];
#pragma unroll
                for (int q = 0; q < E; ++q) win[q] = win_lds[tl + q * (NC / E)];
                load_frame<F, true>(v[0], g, win, lds, row, f, t);
                F::template run<1>(v, ldsv, tw, t);
            }
            // ---- gradient spectrum -> operands of the inverse transform
            int tg = t;
            asm volatile("" : "+v"(tg));
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int k = tg + q * (NC / E);
                const int kt = k <= NC / 2 ? k : NC - k;
                const cf wk = wk_lds[kt];
                const cf wkk = k <= NC / 2 ? wk : mkc(-wk.x, wk.y);
                cf hk, hm;
                F::r2c_pair(lds, k, wkk, hk, hm);
                hk = norm_pow_grad<POW2>(cscale(hk, xscale), gk[q], power);
                hm = norm_pow_grad<POW2>(cscale(hm, xscale), gm[q], power);
                if (q == 0) {
                    if (k == 0) {
                        hk = mkc(2.0f * hk.x, 0.0f);
                        hm = mkc(2.0f * hm.x, 0.0f);
                    }
                }
                v[0][q] = c2r_operand(hk, hm, wkk);
                asm volatile("" : "+v"(v[0][q]));
                if ((q & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
            wave_lds_fence();
            F::template run<1>(v, ldsv, tw, t);
            // ---- windowed frame gradient into this stream's ring; complete positions out
            const int rot = (int)(((long long)f * H) & 15);
            float* const prow = gpad + (long long)row * plan.pad_len + (long long)f * hop;
            float* const tail = row_end ? prow : edge + ((long long)row * (spr - 1) + sidx) * (N - hop) - hop;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int m = t + j * LPF;
                const cf r = lds[lds_pad(m)];
                const cf wn = win_lds[m];
                cf acc = cmul_elem(cmul_elem(r, wn), mkc(wscale, -wscale));     // (Re, -Im) R[m] · window / 2
                cf* const slot = ring + ((j + rot) & 15) * LPF + t;
                if (!(first || j >= 16 - H)) {
                    const cf old = *slot;
                    acc = cadd(acc, old);
                }
                if (live) {
                    if (j < H) *reinterpret_cast<cf*>(prow + 2 * m) = acc;
                    else if (last) *reinterpret_cast<cf*>(tail + 2 * m) = acc;
                    else *slot = acc;
                }
            }
            wave_lds_fence();
        }
    }
}

// g_wave[row][j] = sum over the padded positions i with source(i) == j of P[row][i + pad], where
// P = gpad + (inside a segment's first N - hop positions) the previous segment's edge sums; positions no frame covers are 0.
// Four consecutive samples j .. j + 3 of one row: where none of them has a padding image or straddles a segment-border zone
// they move as one 16-byte access (global accesses need dword alignment only).
// (s, o): segment and offset inside it of padded position j + pad — wave-uniform work for the caller that walks runs.
__device__ __forceinline__ void ola_fold_quad(const FrameGeom& g, const OlaPlan& plan, const float* __restrict__ prow,
                                              const float* __restrict__ erow, float* __restrict__ orow, int j, int s, int o) {
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    const int L = (int)g.length, T = (int)g.n_frames;
    const int pad = g.center_pad, hop = g.hop;
    const int covered = (T - 1) * hop + plan.n_fft;        // positions [0, covered) are touched by some frame
    const int seg_span = plan.seg_frames * hop, open = plan.n_fft - hop, spr = plan.segs_per_row;
    auto one = [&](int jj) -> float {
        float acc = 0.0f;
        auto add_position = [&](int i) {
            const int p = i + pad;
            if (p < 0 || p >= covered) return;
            float v = prow[p];
            const int s = (int)((unsigned)p / (unsigned)seg_span), o = p - s * seg_span;
            if (s >= 1 && s < spr && o < open) v += erow[(long long)(s - 1) * open + o];
            acc += v;
        };
        add_position(jj);
        if (pad > 0) {
            if (g.pad_mode == PAD_REFLECT) {
                if (jj >= 1 && jj <= pad) add_position(-jj);
                if (jj <= L - 2 && jj >= L - 1 - pad) add_position(2 * (L - 1) - jj);
            } else if (g.pad_mode == PAD_REPLICATE) {
                if (jj == 0) for (int i = -pad; i < 0; ++i) add_position(i);
                if (jj == L - 1) for (int i = L; i < L + pad; ++i) add_position(i);
            } else if (g.pad_mode == PAD_CIRCULAR) {
                if (jj >= L - pad) add_position(jj - L);
                if (jj < pad) add_position(jj + L);
            }
        }
        return acc;
    };
    const int p = j + pad;
    const bool images = pad > 0 && (j <= pad || j + 3 >= L - 1 - pad);      // some sample has a padding image
    const bool in_zone = s >= 1 && s < spr && o + 3 < open, out_zone = s < 1 || s >= spr || (o >= open && o + 3 < seg_span);
    if (j + 3 < L && p + 3 < covered && !images && (in_zone || out_zone)) {
        f4u v = *reinterpret_cast<const f4u*>(prow + p);
        if (in_zone) v += *reinterpret_cast<const f4u*>(erow + (long long)(s - 1) * open + o);
        *reinterpret_cast<f4u*>(orow + j) = v;
    } else {
        // up to three padded positions per sample (itself and its reflect / circular images): every address first, then all
        // loads back to back — taken one sample at a time these were a chain of ~16 dependent memory round trips per thread,
        // most of this kernel's time.  (replicate: the two end samples own `pad` images each and take the loop above)
        int pos[4][3];
        bool use[4][3], zone[4][3];
        float val[4][3], edg[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j + u;
            int cand[3] = {jj, 0, 0};
            bool ok[3] = {jj < L, false, false};
            if (pad > 0 && g.pad_mode == PAD_REFLECT) {
                cand[1] = -jj;
                ok[1] = jj >= 1 && jj <= pad;
                cand[2] = 2 * (L - 1) - jj;
                ok[2] = jj <= L - 2 && jj >= L - 1 - pad;
            } else if (pad > 0 && g.pad_mode == PAD_CIRCULAR) {
                cand[1] = jj - L;
                ok[1] = jj >= L - pad;
                cand[2] = jj + L;
                ok[2] = jj < pad;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int pc = cand[c] + pad;
                use[u][c] = jj < L && ok[c] && pc >= 0 && pc < covered;
                pos[u][c] = use[u][c] ? pc : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int pc = pos[u][c];
                const int sc = (int)((unsigned)pc / (unsigned)seg_span), oc = pc - sc * seg_span;
                zone[u][c] = use[u][c] && sc >= 1 && sc < spr && oc < open;
                val[u][c] = prow[pc];
                const float* ea = zone[u][c] ? erow + ((long long)(sc - 1) * open + oc) : prow;
                edg[u][c] = *ea;
            }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j + u;
            if (jj >= L) break;
            if (pad > 0 && g.pad_mode == PAD_REPLICATE && (jj == 0 || jj == L - 1)) {
                orow[jj] = one(jj);
                continue;
            }
            float acc = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (use[u][c]) acc += val[u][c] + (zone[u][c] ? edg[u][c] : 0.0f);
            }
            orow[jj] = acc;
        }
    }
}

// every sample of every row (grid: x over the samples of a row, y over rows — no division by L per sample, 32-bit positions)
__global__ void __launch_bounds__(256)
ola_fold_kernel(FrameGeom g, const float* __restrict__ gpad, const float* __restrict__ edge, OlaPlan plan,
                float* __restrict__ gwave, long long gwave_row_stride) {
    const int L = (int)g.length, T = (int)g.n_frames;
    const int pad = g.center_pad, hop = g.hop;
    const int open = plan.n_fft - hop, spr = plan.segs_per_row;
    for (long long row = blockIdx.y; row < g.rows; row += gridDim.y) {
        const float* prow = gpad + row * plan.pad_len;
        const float* erow = edge + row * (spr - 1) * open;
        float* orow = gwave + row * gwave_row_stride;
        for (int j = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x); j < L; j += 4 * (int)(gridDim.x * blockDim.x)) {
            if (plan.direct) {                               // already stored by the backward kernel (hop and pad are multiples of 4)
                const int fc = (j + pad) / hop;
                if (fc < T && ola_direct(g, plan, fc)) continue;
            }
            const int p = j + pad, seg_span = plan.seg_frames * hop;
            const int s = (int)((unsigned)p / (unsigned)seg_span);
            ola_fold_quad(g, plan, prow, erow, orow, j, s, p - s * seg_span);
        }
    }
}

// plan.direct: the backward kernel stored most runs itself — visit only the hop-runs it left (OlaRuns, host-computed):
// the row's head and tail (padding images, the border of the frames' reach) and the first `zone_frames` runs of every segment
// but the first.  Run k of a row -> frame slot fc; a thread owns four samples of one run.
__global__ void __launch_bounds__(256)
ola_fold_runs_kernel(FrameGeom g, const float* __restrict__ gpad, const float* __restrict__ edge, OlaPlan plan, OlaRuns runs,
                     int zone_blocks, float* __restrict__ gwave, long long gwave_row_stride) {
    // rows on grid y.  Blocks [0, zone_blocks): the segments' border zones, one thread per quad (one integer division per
    // thread; a zone whose runs are all clean — no padding image, inside the row and the frames' reach — is two loads and a
    // store).  Blocks behind them: one wave per head / tail run (frame slot, segment and offset wave-uniform).  The first
    // version — one thread per quad of ANY run with three divisions and the general path — was instruction-bound (25 us at
    // cfg-2); one wave per zone was latency-bound on its many tiny waves (50 us at fft_length 400).
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    const int L = (int)g.length, pad = g.center_pad, hop = g.hop;
    const int open = plan.n_fft - hop, spr = plan.segs_per_row, quads = hop >> 2, S = plan.seg_frames;
    const int n_tail = runs.last_run + 1 - runs.tail_first;
    const int nq = runs.zone_frames * quads;                                 // quads per zone (< n_fft / 4)
    const bool quad_aligned = (open & 3) == 0;                               // no quad straddles the end of the zone
    for (long long row = blockIdx.y; row < g.rows; row += gridDim.y) {
        const float* prow = gpad + row * plan.pad_len;
        const float* erow = edge + row * (spr - 1) * open;
        float* orow = gwave + row * gwave_row_stride;
        if ((int)blockIdx.x < zone_blocks) {
            const unsigned total = (unsigned)(spr - 1) * (unsigned)nq;
            for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += (unsigned)zone_blocks * 256u) {
                const int z = (int)(idx / (unsigned)nq), q = (int)(idx - (unsigned)z * (unsigned)nq);
                const int s = z + 1, first = s * S, o = 4 * q, p = first * hop + o;
                if (quad_aligned && first >= runs.head && first + runs.zone_frames <= runs.tail_first) {
                    f4u v = *reinterpret_cast<const f4u*>(prow + p);
                    if (o + 3 < open) v += *reinterpret_cast<const f4u*>(erow + (long long)(s - 1) * open + o);
                    *reinterpret_cast<f4u*>(orow + (p - pad)) = v;
                } else {
                    const int fc = first + q / quads, j = p - pad;
                    if (fc < runs.head || fc >= runs.tail_first || j < 0 || j >= L) continue;   // (head / tail runs: below)
                    ola_fold_quad(g, plan, prow, erow, orow, j, s, o);
                }
            }
        } else {
            const int lane = threadIdx.x & 63;
            const int k = ((int)blockIdx.x - zone_blocks) * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
            if (k >= runs.head + n_tail) continue;
            const int fc = k < runs.head ? k : runs.tail_first + (k - runs.head);
            const int s = fc / S, o0 = (fc - s * S) * hop;
            for (int i = lane; i < quads; i += 64) {
                const int j = fc * hop + 4 * i - pad;
                if (j < 0 || j >= L) continue;
                ola_fold_quad(g, plan, prow, erow, orow, j, s, o0 + 4 * i);
            }
        }
    }
}

// g_wave[row][j] = sum over padded positions i with source(i) == j of sum over frames t covering i of
// frames[row][t][i + pad - t*hop]   (source(): torch.nn.functional.pad semantics, fft_core.hpp padded_index).
__global__ void __launch_bounds__(256)
overlap_add_kernel(FrameGeom g, int n_fft, const float* __restrict__ frames, float* __restrict__ gwave,
                   long long gwave_row_stride, int vec4) {
    // positions inside a row are 32-bit (L < 2^31 - 2 n_fft, host-checked): only the final addresses are 64-bit — the
    // 64-bit divisions of the first version were most of this kernel's time.  A thread owns FOUR consecutive samples:
    // where hop, pad and n_fft are multiples of four (vec4, host-checked together with the alignment of `frames`) and none
    // of the four has a padding image, every frame that covers one of them covers all four at a 16-byte aligned offset,
    // so the gather is one 16-byte load per covering frame instead of four 4-byte ones (round 3: 0.193 -> ~0.1 ms for
    // fft_length 400 / hop 160 at 256 x 160 000 samples).
    const int L = (int)g.length, T = (int)g.n_frames;
    const int pad = g.center_pad, hop = g.hop;
    const int groups = (L + 3) >> 2;
    const long long total = g.rows * (long long)groups;
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    typedef float f4a __attribute__((ext_vector_type(4)));
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(idx / groups);
        const int j0 = 4 * (int)(idx - (long long)row * groups);
        const float* fr = frames + (long long)row * T * n_fft;
        float* orow = gwave + row * gwave_row_stride;
        auto one = [&](int j) -> float {
            float acc = 0.0f;
            auto add_position = [&](int i) {                            // i: position in the padded signal minus pad
                const int p = i + pad;                                  // 0 <= p < L + 2 pad
                int t1 = p / hop;
                if (t1 > T - 1) t1 = T - 1;
                int t0 = p - n_fft + 1 <= 0 ? 0 : (p - n_fft + hop) / hop;  // ceil((p - n_fft + 1) / hop)
                for (int tt = t0; tt <= t1; ++tt) acc += fr[(long long)tt * n_fft + (p - tt * hop)];
            };
            add_position(j);
            if (pad > 0) {
                if (g.pad_mode == PAD_REFLECT) {
                    if (j >= 1 && j <= pad) add_position(-j);
                    if (j <= L - 2 && j >= L - 1 - pad) add_position(2 * (L - 1) - j);
                } else if (g.pad_mode == PAD_REPLICATE) {
                    if (j == 0) for (int i = -pad; i < 0; ++i) add_position(i);
                    if (j == L - 1) for (int i = L; i < L + pad; ++i) add_position(i);
                } else if (g.pad_mode == PAD_CIRCULAR) {
                    if (j >= L - pad) add_position(j - L);
                    if (j < pad) add_position(j + L);
                }
            }
            return acc;
        };
        const bool images = pad > 0 && g.pad_mode != PAD_CONSTANT && (j0 <= pad || j0 + 3 >= L - 1 - pad);
        if (vec4 && j0 + 3 < L && !images) {
            const int p = j0 + pad;                                     // multiple of 4
            int t1 = p / hop;                                           // the same frames cover p .. p + 3
            if (t1 > T - 1) t1 = T - 1;
            const int t0 = p + 3 - n_fft + 1 <= 0 ? 0 : (p + 3 - n_fft + hop) / hop;
            f4a acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int tt = t0; tt <= t1; ++tt) acc += *reinterpret_cast<const f4a*>(fr + (long long)tt * n_fft + (p - tt * hop));
            *reinterpret_cast<f4u*>(orow + j0) = acc;
        } else {
            for (int u = 0; u < 4 && j0 + u < L; ++u) orow[j0 + u] = one(j0 + u);
        }
    }
}

// Gradient of the window (functional.py:99-107 differentiates through every argument): with gfr the gradient w.r.t.
// the WINDOWED frame, g_window[n] = sum over (row, frame) of gfr[row][t][n] * padded[row][t*hop + n].  A workgroup owns
// a chunk of consecutive frames of the flattened (row, frame) index and writes one partial row of n_fft sums
// (tac_sum_slabs_f32 adds the partial rows up: fixed order, deterministic).
__global__ void __launch_bounds__(256)
window_grad_kernel(FrameGeom g, int n_fft, const float* __restrict__ gfr, long long frames_per_block,
                   float* __restrict__ partial) {
    const int L = (int)g.length, T = (int)g.n_frames;
    const long long total = g.rows * (long long)T;
    const long long f0 = (long long)blockIdx.x * frames_per_block;
    const long long f1 = f0 + frames_per_block < total ? f0 + frames_per_block : total;
    for (int n = threadIdx.x; n < n_fft; n += blockDim.x) {
        float acc = 0.0f;
        for (long long fi = f0; fi < f1; ++fi) {
            const long long row = fi / T;
            const int t = (int)(fi - row * T);
            bool zero;
            const int j = padded_index(t * g.hop + n - g.center_pad, L, g.pad_mode, &zero);
            const float x = zero ? 0.0f : g.wave[row * g.row_stride + j];
            acc = __builtin_fmaf(gfr[fi * n_fft + n], x, acc);
        }
        partial[(long long)blockIdx.x * n_fft + n] = acc;
    }
}

// d/dz of |z|^power lives above (norm_pow_grad)
__global__ void __launch_bounds__(256)
complex_norm_backward_kernel(const float* __restrict__ z, const float* __restrict__ gout, long long n, float power,
                             float* __restrict__ gz) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        *reinterpret_cast<cf*>(gz + 2 * i) = norm_pow_grad(*reinterpret_cast<const cf*>(z + 2 * i), gout[i], power);
}

// d/dx of 10 (log10(clamp(x^2, amin)) - log10 ref) (functional.py:291-296): 20 / (ln 10 * x) where x^2 >= amin, else 0.
// A NaN input stays NaN, as it does through the forward clamp (amp_to_db) and through torch's autograd of the formula: the
// compare alone would send it to 0, and a gradient of 0 is what hides a diverged input from whoever checks the gradients.
// VEC: 16 bytes per lane and stream (all three pointers 16-byte aligned; the tail runs scalar).
template <bool VEC>
__global__ void __launch_bounds__(256)
amplitude_to_db_backward_kernel(const float* __restrict__ x, const float* __restrict__ gout, long long n, float amin,
                                float* __restrict__ gx) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    auto one = [&](float v, float g) { return (v * v >= amin) ? g * (8.6858896380650366f / v) : (v == v ? 0.0f : v); };
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
    const long long n4 = VEC ? n >> 2 : 0;
    for (long long i = tid; i < n4; i += nth) {
        const f4 v = reinterpret_cast<const f4*>(x)[i], g = reinterpret_cast<const f4*>(gout)[i];
        f4 r;
        r.x = one(v.x, g.x); r.y = one(v.y, g.y); r.z = one(v.z, g.z); r.w = one(v.w, g.w);
        reinterpret_cast<f4*>(gx)[i] = r;
    }
    for (long long i = 4 * n4 + tid; i < n; i += nth) gx[i] = one(x[i], gout[i]);
}

// d/dz of (|z|^power, atan2(im, re)) (functional.py:187-201): g_mag power |z|^(power-2) z + g_phase (-im, re) / |z|^2, both 0 at
// z == 0 (what torch's norm / atan2 gradients give there); either gradient may be absent
__global__ void __launch_bounds__(256)
magphase_backward_kernel(const float* __restrict__ z, const float* __restrict__ gmag, const float* __restrict__ gphase, long long n,
                         float power, float* __restrict__ gz) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const cf v = *reinterpret_cast<const cf*>(z + 2 * i);
        cf r = gmag ? norm_pow_grad(v, gmag[i], power) : mkc(0.0f, 0.0f);
        if (gphase) {
            const float s = v.x * v.x + v.y * v.y;
            const float f = s == 0.0f ? 0.0f : gphase[i] / s;
            r.x -= f * v.y;
            r.y += f * v.x;
        }
        *reinterpret_cast<cf*>(gz + 2 * i) = r;
    }
}

// d/dx of (10^(x/10 + log10 ref))^0.5 (functional.py:299-314) = y ln(10) / 20, y re-evaluated as the forward kernel does
__global__ void __launch_bounds__(256)
db_to_amplitude_backward_kernel(const float* __restrict__ x, const float* __restrict__ gout, long long n, float log10_ref,
                                float* __restrict__ gx) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        gx[i] = gout[i] * (0.11512925464970229f * exp2f((x[i] / 10.0f + log10_ref) * 1.6609640474436813f));
}

template <int NC, int E>
static int launch_stft_backward(const FrameGeom& g, const Tables& tb, const float* gspec, const float* gnorm, float power,
                                float* frames, hipStream_t stream, bool from_wave, bool inverse = false) {
    using F = WaveFft<NC, E>;
    const size_t lds_bytes = (size_t)BW_WAVES * (((F::G * F::PADDED + 1) / 2) * 2) * sizeof(cf) +
                             (from_wave ? (size_t)(NC + NC / 2 + 2) * sizeof(cf) : 0);
    const long long groups = g.rows * ((g.n_frames + F::G - 1) / F::G);
    const bool pow2 = (power == 2.0f);
    void (*kern)(FrameGeom, Tables, const float*, const float*, float, float*);
    if (from_wave) {
        if constexpr (radix_at(NC, 0) == E)
            kern = pow2 ? stft_backward_kernel<NC, E, SRC_WAVE, true> : stft_backward_kernel<NC, E, SRC_WAVE, false>;
        else
            return TAC_E_UNSUPPORTED;                  // (32 elements per lane: no registers for two transforms)
    } else if (inverse) {
        kern = stft_backward_kernel<NC, E, SRC_INV, false>;
    } else if (gnorm) {
        kern = pow2 ? stft_backward_kernel<NC, E, SRC_NORM, true> : stft_backward_kernel<NC, E, SRC_NORM, false>;
    } else {
        kern = stft_backward_kernel<NC, E, SRC_GRAD, false>;
    }
    const int rc = launch_kernel(kern, persistent_blocks(groups, BW_WAVES, (long long)device_cu_count() * 2), BW_WAVES * 64, lds_bytes, stream, g, tb,
                                 gspec, gnorm, power, frames);
    if (rc != TAC_OK) return rc;
    set_last_route("stft_backward_kernel<%d, %d, %s, %s>", NC, E, from_wave ? "SRC_WAVE" : (inverse ? "SRC_INV" : (gnorm ? "SRC_NORM" : "SRC_GRAD")),
                   pow2 && (from_wave || (gnorm && !inverse)) ? "true" : "false");
    return TAC_OK;
}

bool stft_smooth_covers(int n_fft);                                                                           // stft_smooth.hip
int launch_stft_smooth_backward(int n_fft, const FrameGeom& g, const float* grad_spec, float* grad_frames, hipStream_t stream,
                                bool inverse = false);

static int stft_backward_entry(const float* spec, const float* gnorm, float power, const float* window, const tac_stft_desc* d,
                               float* grad_frames, void* stream, bool from_wave = false, const AdjEntry* adj = nullptr,
                               int n_mels = 0) {
    if (!spec || !grad_frames || !d) return TAC_E_INVALID;
    if (!d->onesided) return TAC_E_UNSUPPORTED;
    FrameGeom g;
    int64_t T = 0;
    // from_wave: `spec` IS the waveform.  Otherwise the geometry helper wants a waveform pointer for its alignment flags
    // only and the spectrum stands in.
    // even lengths with a 7-smooth half (stft_smooth.hip): the plain form only — frame gradients from a gradient spectrum
    // (and fft_length 8192, whose forward kernel is stft_big.hip: radix-4 / 2 passes, one frame per workgroup)
    const bool smooth = !gnorm && !from_wave && !adj && (stft_smooth_covers(d->n_fft) || d->n_fft == 8192);
    int rc = make_geometry(spec, window, d, &g, &T, smooth);
    if (rc != TAC_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (smooth) return launch_stft_smooth_backward(d->n_fft, g, spec, grad_frames, s);
    if (d->n_fft == 400)                                   // the mixed-radix form (stft_n400.hip)
        return launch_n400_backward(g, spec, gnorm, power, grad_frames, s, from_wave, adj, n_mels);
    if (adj) return TAC_E_UNSUPPORTED;                     // (the filterbank adjoint inside the frame-gradient kernel: fft_length 400 only)
    Tables tb;
    rc = get_tables(d->n_fft, &tb);
    if (rc != TAC_OK) return rc;
    switch (d->n_fft) {
        case 32: return launch_stft_backward<16, 16>(g, tb, spec, gnorm, power, grad_frames, s, from_wave);
        case 64: return launch_stft_backward<32, 16>(g, tb, spec, gnorm, power, grad_frames, s, from_wave);
        case 128: return launch_stft_backward<64, 16>(g, tb, spec, gnorm, power, grad_frames, s, from_wave);
        case 256: return launch_stft_backward<128, 16>(g, tb, spec, gnorm, power, grad_frames, s, from_wave);
        case 512: return launch_stft_backward<256, 16>(g, tb, spec, gnorm, power, grad_frames, s, from_wave);
        case 1024: return launch_stft_backward<512, 16>(g, tb, spec, gnorm, power, grad_frames, s, from_wave);
        case 2048: return launch_stft_backward<1024, 16>(g, tb, spec, gnorm, power, grad_frames, s, from_wave);
        case 4096: return launch_stft_backward<2048, 32>(g, tb, spec, gnorm, power, grad_frames, s, from_wave);
        default: return TAC_E_UNSUPPORTED;
    }
}

// The frame kernels in inverse mode (istft.hip): spec[rows][T][F][2] -> frames[rows][T][N] = window * irfft(X_t) with the factor
// 2 / N (times sqrt(N) when normalized) in g.scale — the gradient mode's window factor g.scale / 2 then is the 1 / N of irfft.
int launch_istft_frames(int n_fft, const FrameGeom& g, const float* spec, float* frames, hipStream_t s) {
    if (stft_smooth_covers(n_fft) || n_fft == 8192) return launch_stft_smooth_backward(n_fft, g, spec, frames, s, true);
    if (n_fft == 400) return launch_n400_backward(g, spec, nullptr, 0.0f, frames, s, false, nullptr, 0, nullptr, nullptr, nullptr, true);
    Tables tb;
    const int rc = get_tables(n_fft, &tb);
    if (rc != TAC_OK) return rc;
    switch (n_fft) {
        case 32: return launch_stft_backward<16, 16>(g, tb, spec, nullptr, 0.0f, frames, s, false, true);
        case 64: return launch_stft_backward<32, 16>(g, tb, spec, nullptr, 0.0f, frames, s, false, true);
        case 128: return launch_stft_backward<64, 16>(g, tb, spec, nullptr, 0.0f, frames, s, false, true);
        case 256: return launch_stft_backward<128, 16>(g, tb, spec, nullptr, 0.0f, frames, s, false, true);
        case 512: return launch_stft_backward<256, 16>(g, tb, spec, nullptr, 0.0f, frames, s, false, true);
        case 1024: return launch_stft_backward<512, 16>(g, tb, spec, nullptr, 0.0f, frames, s, false, true);
        case 2048: return launch_stft_backward<1024, 16>(g, tb, spec, nullptr, 0.0f, frames, s, false, true);
        case 4096: return launch_stft_backward<2048, 32>(g, tb, spec, nullptr, 0.0f, frames, s, false, true);
        default: return TAC_E_UNSUPPORTED;
    }
}

// ---------------------------------------------------------------- band-sparse adjoint of the filterbank stage
// d/d spec of spec·fb (functional.py:183-184) is grad_mel·fb^T.  A mel bank has at most two non-zero weights per BIN
// (the falling edge of one triangle, the rising edge of the next), so the adjoint is two multiply-adds per output instead
// of a GEMM row: fb_adjoint_pack_kernel builds {w0, w1, band0, band1} per bin on the device (and counts the non-zeros of
// the fullest bin: banks with more than two keep the GEMM), fb_adjoint_kernel streams frames through it — a wave per
// frame, the frame's mel-gradient row in LDS, 4·F bytes out per frame: write-bound.

__global__ void __launch_bounds__(256)
fb_adjoint_pack_kernel(const float* __restrict__ fb, int n_freqs, int n_mels, AdjEntry* __restrict__ table,
                       int* __restrict__ max_nnz) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_freqs) return;
    AdjEntry e{0.0f, 0.0f, 0, 0};
    int n = 0;
    for (int m = 0; m < n_mels; ++m) {
        const float wv = fb[(long long)f * n_mels + m];
        if (wv != 0.0f) {
            if (n == 0) { e.w0 = wv; e.b0 = m; }
            else if (n == 1) { e.w1 = wv; e.b1 = m; }
            ++n;
        }
    }
    table[f] = e;
    atomicMax(max_nnz, n);
}

constexpr int ADJ_WAVES = 4;

__global__ void __launch_bounds__(ADJ_WAVES * 64)
fb_adjoint_kernel(const float* __restrict__ gmel, long long n_rows_frames, int n_mels, const AdjEntry* __restrict__ table,
                  int n_freqs, float* __restrict__ gspec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    AdjEntry* const tl = reinterpret_cast<AdjEntry*>(smem_raw);                       // [n_freqs]
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* const grow = reinterpret_cast<float*>(tl + n_freqs) + w * n_mels;          // this wave's mel-gradient row
    for (int f = threadIdx.x; f < n_freqs; f += ADJ_WAVES * 64) tl[f] = table[f];
    __syncthreads();
    const long long stride = (long long)gridDim.x * ADJ_WAVES;
    const int per_lane = (n_mels + 63) >> 6;                                          // <= 8 (n_mels <= 512)
    float nxt[8];
    long long u = (long long)blockIdx.x * ADJ_WAVES + w;
    auto fetch = [&](long long unit) {
        const float* src = gmel + (unit < n_rows_frames ? unit : n_rows_frames - 1) * n_mels;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = lane + 64 * i;
            nxt[i] = (i < per_lane && m < n_mels) ? src[m] : 0.0f;
        }
    };
    if (u < n_rows_frames) fetch(u);
    for (; u < n_rows_frames; u += stride) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = lane + 64 * i;
            if (i < per_lane && m < n_mels) grow[m] = nxt[i];
        }
        fetch(u + stride);                                          // the next frame's row travels behind this frame's work
        wave_lds_fence();
        float* out = gspec + u * n_freqs;
        for (int f = lane; f < n_freqs; f += 64) {
            const AdjEntry e = tl[f];
            out[f] = __builtin_fmaf(e.w0, grow[e.b0], e.w1 * grow[e.b1]);
        }
        wave_lds_fence();
    }
}

// segmentation of the LDS overlap-add form; TAC_E_UNSUPPORTED for geometries it does not cover
static int ola_plan(const tac_stft_desc* d, const FrameGeom& g, OlaPlan* plan, int waves_per_cu = 2 * OLA_WAVES) {
    const int n = d->n_fft;
    if (n != 2048 && n != 1024 && n != 512 && n != 256 && n != 400) return TAC_E_UNSUPPORTED;
    if (!d->onesided || d->hop <= 0 || d->hop > n) return TAC_E_UNSUPPORTED;
    if (n == 400 ? ((d->hop & 3) || (g.center_pad & 3) || d->hop < 50) : (d->hop % (n / 16)) != 0) return TAC_E_UNSUPPORTED;
    if (g.length >= 0x7fffffffLL - 2 * n || g.n_frames < 1 || g.n_frames >= 0x7fffffffLL / n) return TAC_E_UNSUPPORTED;
    const int T = (int)g.n_frames;
    if (n == 400) {                         // stft_n400_backward_kernel<.., OLA>: a segment is one unit of eight frames
        plan->seg_frames = 8;
        plan->segs_per_row = (T + 7) / 8;
        plan->pad_len = g.length + 2LL * g.center_pad;
        plan->n_fft = n;
        plan->direct = 0;
        plan->gwave = nullptr;
        plan->gstride = 0;
        return TAC_OK;
    }
    const int s_min = std::max(1, (n - d->hop + d->hop - 1) / d->hop);
    // one segment per resident frame stream (a wave carries 2048 / n_fft of them)
    const long long target = (long long)device_cu_count() * waves_per_cu * (OLA_N / n);
    long long spr = (target + g.rows - 1) / g.rows;
    spr = std::max(1LL, std::min(spr, (long long)std::max(1, T / s_min)));
    int S = (int)((T + spr - 1) / spr);
    if (S < s_min) S = s_min;
    plan->seg_frames = S;
    plan->segs_per_row = (T + S - 1) / S;
    plan->pad_len = g.length + 2LL * g.center_pad;
    plan->n_fft = n;
    plan->direct = 0;
    plan->gwave = nullptr;
    plan->gstride = 0;
    return TAC_OK;
}

static long long ola_workspace_floats(const FrameGeom& g, const OlaPlan& plan, int hop) {
    return g.rows * plan.pad_len + g.rows * (long long)(plan.segs_per_row - 1) * (plan.n_fft - hop);
}

static long long bw_blocks(long long n) { return persistent_blocks(n, 256, (long long)device_cu_count() * 16); }

}  // namespace tac

extern "C" {

int tac_stft_backward_f32(const float* grad_spec, const float* window, const tac_stft_desc* d, float* grad_frames,
                          void* stream) {
    return tac::stft_backward_entry(grad_spec, nullptr, 0.0f, window, d, grad_frames, stream);
}

int tac_stft_norm_backward_f32(const float* spec, const float* grad_norm, float power, const float* window,
                               const tac_stft_desc* d, float* grad_frames, void* stream) {
    if (!grad_norm) return TAC_E_INVALID;
    return tac::stft_backward_entry(spec, grad_norm, power, window, d, grad_frames, stream);
}

int tac_spectrogram_backward_f32(const float* wave, const float* window, const tac_stft_desc* d, const float* grad_norm,
                                 float power, float* grad_frames, void* stream) {
    if (!grad_norm) return TAC_E_INVALID;
    return tac::stft_backward_entry(wave, grad_norm, power, window, d, grad_frames, stream, true);
}

int tac_melspectrogram_backward_f32(const float* wave, const float* window, const tac_stft_desc* d, const float* grad_mel,
                                    int32_t n_mels, const void* adjoint_table, int32_t n_freqs, float power, float* grad_frames,
                                    void* stream) {
    if (!grad_mel || !adjoint_table || !d) return TAC_E_INVALID;
    if (n_freqs != d->n_fft / 2 + 1 || n_mels < 1) return TAC_E_INVALID;
    if (d->n_fft != 400 || n_mels > 128) return TAC_E_UNSUPPORTED;
    return tac::stft_backward_entry(wave, grad_mel, power, window, d, grad_frames, stream, true,
                                    static_cast<const tac::AdjEntry*>(adjoint_table), n_mels);
}

int tac_filterbank_adjoint_pack(const float* fb, int32_t n_freqs, int32_t n_mels, void* table, int32_t* max_nonzeros_host,
                                void* stream) {
    using namespace tac;
    if (!fb || !table || !max_nonzeros_host || n_freqs <= 0 || n_mels <= 0) return TAC_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    // the counter sits behind the table (caller allocates 16·n_freqs + 16 bytes)
    int* counter = reinterpret_cast<int*>(static_cast<AdjEntry*>(table) + n_freqs);
    TAC_HIP(hipMemsetAsync(counter, 0, sizeof(int), s));
    const int rc = launch_kernel(fb_adjoint_pack_kernel, (n_freqs + 255) / 256, 256, 0, s, fb, (int)n_freqs, (int)n_mels,
                                 static_cast<AdjEntry*>(table), counter);
    if (rc != TAC_OK) return rc;
    TAC_HIP(hipMemcpyAsync(max_nonzeros_host, counter, sizeof(int), hipMemcpyDeviceToHost, s));
    TAC_HIP(hipStreamSynchronize(s));
    return TAC_OK;
}

int tac_apply_filterbank_adjoint_f32(const float* grad_mel, int64_t rows_times_frames, int32_t n_mels, const void* table,
                                     int32_t n_freqs, float* grad_spec, void* stream) {
    using namespace tac;
    if (rows_times_frames == 0) return TAC_OK;
    if (!grad_mel || !table || !grad_spec || rows_times_frames < 0 || n_mels <= 0 || n_freqs <= 0) return TAC_E_INVALID;
    if (n_mels > 512) return TAC_E_UNSUPPORTED;
    const size_t lds_bytes = (size_t)n_freqs * sizeof(AdjEntry) + (size_t)ADJ_WAVES * n_mels * sizeof(float);
    if (lds_bytes > 64 * 1024) return TAC_E_UNSUPPORTED;
    return launch_kernel(fb_adjoint_kernel, persistent_blocks(rows_times_frames, ADJ_WAVES, (long long)device_cu_count() * 4), ADJ_WAVES * 64,
                         lds_bytes, (hipStream_t)stream, grad_mel, (long long)rows_times_frames, (int)n_mels,
                         static_cast<const AdjEntry*>(table), (int)n_freqs, grad_spec);
}

int64_t tac_spectrogram_backward_ola_workspace(const tac_stft_desc* d) {
    using namespace tac;
    if (!d) return TAC_E_INVALID;
    FrameGeom g;
    int64_t T = 0;
    float dummy = 0.0f;
    int rc = make_geometry(&dummy, &dummy, d, &g, &T);
    if (rc != TAC_OK) return rc;
    OlaPlan plan;
    rc = ola_plan(d, g, &plan);
    if (rc != TAC_OK) return rc;
    long long floats = ola_workspace_floats(g, plan, d->hop);
    if (d->n_fft == 2048 || d->n_fft == 1024 || d->n_fft == 512) {      // the twelve-wave forms cut more segments per row: room for either
        OlaPlan p12;
        if (ola_plan(d, g, &p12, BR_WAVES) == TAC_OK) floats = std::max(floats, ola_workspace_floats(g, p12, d->hop));
    }
    return (int64_t)floats * (int64_t)sizeof(float);
}

}  // extern "C"

namespace tac {
// shared body of tac_spectrogram_backward_ola_f32 and tac_melspectrogram_backward_ola_f32 (adj != nullptr: `grad` is the
// gradient of the mel values and the filterbank adjoint is folded into the kernel; fft_length 2048 only)
static int ola_backward_entry(const float* wave, const float* window, const tac_stft_desc* d, const float* grad, float power,
                              const AdjEntry* adj, int n_mels, void* workspace, int64_t workspace_bytes, float* grad_wave,
                              int64_t grad_row_stride, void* stream) {
    if (!wave || !window || !d || !grad || !workspace || !grad_wave) return TAC_E_INVALID;
    FrameGeom g;
    int64_t T = 0;
    int rc = make_geometry(wave, window, d, &g, &T);
    if (rc != TAC_OK) return rc;
    OlaPlan plan;
    rc = ola_plan(d, g, &plan);
    if (rc != TAC_OK) return rc;
    if (workspace_bytes < (int64_t)(ola_workspace_floats(g, plan, d->hop) * (long long)sizeof(float))) return TAC_E_INVALID;
    Tables tb;
    rc = get_tables(d->n_fft, &tb);
    if (rc != TAC_OK) return rc;
    float* gpad = static_cast<float*>(workspace);
    float* edge = gpad + g.rows * plan.pad_len;
    plan.gwave = grad_wave;
    plan.gstride = grad_row_stride;
    plan.direct = ((d->n_fft == 2048 || d->n_fft == 400) && (d->hop & 3) == 0 && (g.center_pad & 3) == 0) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const bool pow2 = (power == 2.0f);
    if (d->n_fft == 400) {
        rc = launch_n400_backward(g, nullptr, grad, power, nullptr, s, true, adj, n_mels, gpad, edge, &plan);
        if (rc != TAC_OK) return rc;
    } else {
    rc = TAC_OK;
    OlaFuse fz{nullptr, 0, 0, 16};
    char route[96] = "";                                   // the instantiation launched below (tac_last_route)
    const char* const p2 = pow2 ? "true" : "false";
    // units of work: the segments of all rows, `streams_per_wave` of them a wave
    auto units = [&](int streams_per_wave) { return (g.rows * (long long)plan.segs_per_row + streams_per_wave - 1) / streams_per_wave; };
    auto launch = [&](auto kern, size_t lds_bytes, int streams_per_wave, int waves = OLA_WAVES) {
        return launch_kernel(kern, persistent_blocks(units(streams_per_wave), waves, (long long)device_cu_count() * 2 * OLA_WAVES / waves),
                             waves * 64, lds_bytes, s, g, tb, grad, power, gpad, edge, plan, fz);
    };
    auto launch_multi = [&](auto kern, size_t lds_bytes, int streams_per_wave) {
        return launch_kernel(kern, persistent_blocks(units(streams_per_wave), OLA_WAVES, (long long)device_cu_count() * 2), OLA_WAVES * 64,
                             lds_bytes, s, g, tb, grad, power, gpad, edge, plan);
    };
    // LDS: per wave the exchange area(s) of its frame(s) + N floats of ring per frame stream (8 KB either way), then the
    // window pairs and the R2C twiddles
    auto lds_for = [](int nc, int padded, int gframes) {
        return (size_t)OLA_WAVES * ((size_t)(((gframes * padded + 1) / 2) * 2) + (size_t)gframes * nc) * sizeof(cf) +
               (size_t)(nc + nc / 2 + 2) * sizeof(cf);
    };
    static const bool lds_ring = [] { const char* e = getenv("TAC_BWD_LDS_RING"); return e && e[0] == '1'; }();
    if (d->n_fft == 2048 && (!adj || (n_mels >= 1 && n_mels <= 256)) && !lds_ring && g.length >= OLA_N &&
        (d->hop == 256 || d->hop == 512 || d->hop == 1024)) {
        // twelve waves per CU, the ring in registers (backward_ring3.hpp): its own segmentation, one segment per wave
        OlaPlan p12;
        rc = ola_plan(d, g, &p12, BR_WAVES);
        if (rc != TAC_OK) return rc;
        if (workspace_bytes < (int64_t)(ola_workspace_floats(g, p12, d->hop) * (long long)sizeof(float))) return TAC_E_INVALID;
        p12.gwave = plan.gwave;
        p12.gstride = plan.gstride;
        p12.direct = plan.direct;
        plan = p12;
        edge = gpad + g.rows * plan.pad_len;
        fz.adj = adj;
        fz.n_mels = adj ? n_mels : 0;
        fz.mel_stride = adj ? (n_mels + 63) & ~63 : 0;
        fz.ring_slots = 16 - (d->hop >> 7);
        const size_t lds = ring3_lds_bytes<OLA_NC, OLA_E>(fz.mel_stride);
        auto go = [&](auto kern) {
            return launch_kernel(kern, persistent_blocks(units(1), BR_WAVES, device_cu_count()), BR_WAVES * 64, lds, s, g, tb, grad, power, gpad,
                                 edge, plan, fz);
        };
        auto pick = [&](auto h_tag) -> int {
            constexpr int HH = decltype(h_tag)::value;
            if (adj) return pow2 ? go(melspec_backward_ring3_kernel<true, HH, true>) : go(melspec_backward_ring3_kernel<false, HH, true>);
            return pow2 ? go(melspec_backward_ring3_kernel<true, HH, false>) : go(melspec_backward_ring3_kernel<false, HH, false>);
        };
        switch (d->hop) {
            case 256: rc = pick(std::integral_constant<int, 2>{}); break;
            case 512: rc = pick(std::integral_constant<int, 4>{}); break;
            default: rc = pick(std::integral_constant<int, 8>{}); break;
        }
        snprintf(route, sizeof(route), "melspec_backward_ring3_kernel<%s, %d, %s>", p2, d->hop >> 7, adj ? "true" : "false");
    } else if ((d->n_fft == 1024 || d->n_fft == 512) && (!adj || (n_mels >= 1 && n_mels <= 128)) && !lds_ring &&
               g.length >= d->n_fft && (d->hop == d->n_fft / 8 || d->hop == d->n_fft / 4 || d->hop == d->n_fft / 2)) {
        // fft_length 512 / 1024: the same on 4 / 2 lane groups per wave (backward_ring3_multi.hpp)
        OlaPlan p12;
        rc = ola_plan(d, g, &p12, BR_WAVES);
        if (rc != TAC_OK) return rc;
        if (workspace_bytes < (int64_t)(ola_workspace_floats(g, p12, d->hop) * (long long)sizeof(float))) return TAC_E_INVALID;
        p12.gwave = plan.gwave;
        p12.gstride = plan.gstride;
        p12.direct = ((d->hop & 3) == 0 && (g.center_pad & 3) == 0) ? 1 : 0;
        plan = p12;
        edge = gpad + g.rows * plan.pad_len;
        fz.adj = adj;
        fz.n_mels = adj ? n_mels : 0;
        fz.mel_stride = adj ? (n_mels + 63) & ~63 : 0;
        fz.ring_slots = 0;
        const int G = 2048 / d->n_fft;
        const size_t lds = d->n_fft == 1024 ? ring3_multi_lds_bytes<512>(fz.mel_stride) : ring3_multi_lds_bytes<256>(fz.mel_stride);
        if (lds > 160 * 1024) return TAC_E_UNSUPPORTED;
        auto go = [&](auto kern) {
            return launch_kernel(kern, persistent_blocks(units(G), BR_WAVES, device_cu_count()), BR_WAVES * 64, lds, s, g, tb, grad, power, gpad,
                                 edge, plan, fz);
        };
        auto pick = [&](auto nc_tag, auto h_tag) -> int {
            constexpr int NCC = decltype(nc_tag)::value, HH = decltype(h_tag)::value;
            if (adj) return pow2 ? go(melspec_backward_ring3_multi_kernel<NCC, true, HH, true>) : go(melspec_backward_ring3_multi_kernel<NCC, false, HH, true>);
            return pow2 ? go(melspec_backward_ring3_multi_kernel<NCC, true, HH, false>) : go(melspec_backward_ring3_multi_kernel<NCC, false, HH, false>);
        };
        const int Hh = d->hop / (d->n_fft / 16);
        if (d->n_fft == 1024) {
            using NCT = std::integral_constant<int, 512>;
            rc = Hh == 2 ? pick(NCT{}, std::integral_constant<int, 2>{}) : (Hh == 4 ? pick(NCT{}, std::integral_constant<int, 4>{}) : pick(NCT{}, std::integral_constant<int, 8>{}));
        } else {
            using NCT = std::integral_constant<int, 256>;
            rc = Hh == 2 ? pick(NCT{}, std::integral_constant<int, 2>{}) : (Hh == 4 ? pick(NCT{}, std::integral_constant<int, 4>{}) : pick(NCT{}, std::integral_constant<int, 8>{}));
        }
        snprintf(route, sizeof(route), "melspec_backward_ring3_multi_kernel<%d, %s, %d, %s>", d->n_fft / 2, p2, Hh == 2 || Hh == 4 ? Hh : 8,
                 adj ? "true" : "false");
    } else if (adj) {
        // one 8-wave workgroup per CU around one copy of the tables; the ring shrinks to its 16 - H live slots
        using F = WaveFft<OLA_NC, OLA_E>;
        constexpr int FW = 2 * OLA_WAVES;
        if (d->n_fft != 2048 || n_mels < 1 || n_mels > 256) return TAC_E_UNSUPPORTED;
        const int H = d->hop >> 7;
        fz.adj = adj;
        fz.n_mels = n_mels;
        fz.mel_stride = (n_mels + 63) & ~63;
        fz.ring_slots = H >= 16 ? 1 : 16 - H;
        const size_t lds = (size_t)FW * ((size_t)(((F::PADDED + 1) / 2) * 2) + (size_t)fz.ring_slots * 64) * sizeof(cf) +
                           (size_t)(OLA_NC + OLA_NC / 2 + 2) * sizeof(cf) + (size_t)(OLA_NC + 1) * sizeof(AdjEntry) +
                           (size_t)FW * fz.mel_stride * sizeof(float);
        if (lds > 160 * 1024) return TAC_E_UNSUPPORTED;
        rc = pow2 ? launch(spectrogram_backward_ola_kernel<true, true, FW>, lds, 1, FW)
                  : launch(spectrogram_backward_ola_kernel<false, true, FW>, lds, 1, FW);
        snprintf(route, sizeof(route), "spectrogram_backward_ola_kernel<%s, true, %d>", p2, FW);
    } else
    switch (d->n_fft) {
        case 2048: {
            using F = WaveFft<OLA_NC, OLA_E>;
            fz.ring_slots = 16;
            rc = pow2 ? launch(spectrogram_backward_ola_kernel<true, false, OLA_WAVES>, lds_for(OLA_NC, F::PADDED, 1), 1)
                      : launch(spectrogram_backward_ola_kernel<false, false, OLA_WAVES>, lds_for(OLA_NC, F::PADDED, 1), 1);
            snprintf(route, sizeof(route), "spectrogram_backward_ola_kernel<%s, false, %d>", p2, OLA_WAVES);
            break;
        }
        case 1024: {
            using F = WaveFft<512, OLA_E>;
            rc = pow2 ? launch_multi(spectrogram_backward_ola_multi_kernel<512, true>, lds_for(512, F::PADDED, F::G), F::G)
                      : launch_multi(spectrogram_backward_ola_multi_kernel<512, false>, lds_for(512, F::PADDED, F::G), F::G);
            snprintf(route, sizeof(route), "spectrogram_backward_ola_multi_kernel<512, %s>", p2);
            break;
        }
        case 512: {
            using F = WaveFft<256, OLA_E>;
            rc = pow2 ? launch_multi(spectrogram_backward_ola_multi_kernel<256, true>, lds_for(256, F::PADDED, F::G), F::G)
                      : launch_multi(spectrogram_backward_ola_multi_kernel<256, false>, lds_for(256, F::PADDED, F::G), F::G);
            snprintf(route, sizeof(route), "spectrogram_backward_ola_multi_kernel<256, %s>", p2);
            break;
        }
        case 256: {
            using F = WaveFft<128, OLA_E>;
            rc = pow2 ? launch_multi(spectrogram_backward_ola_multi_kernel<128, true>, lds_for(128, F::PADDED, F::G), F::G)
                      : launch_multi(spectrogram_backward_ola_multi_kernel<128, false>, lds_for(128, F::PADDED, F::G), F::G);
            snprintf(route, sizeof(route), "spectrogram_backward_ola_multi_kernel<128, %s>", p2);
            break;
        }
        default: return TAC_E_UNSUPPORTED;
    }
    if (rc == TAC_OK) set_last_route("%s", route);
    }
    if (rc != TAC_OK) return rc;
    const unsigned fold_y = (unsigned)std::min<long long>(g.rows, 65535);
    const long long per_row = std::max<long long>(1, (long long)device_cu_count() * 16 / fold_y);
    if (plan.direct && g.length + g.center_pad < 0x40000000LL) {
        // only the runs the backward kernel did not store itself (the complement of ola_direct(); the gradient tests run
        // with NaN-filled outputs, so a run nobody writes cannot pass)
        const int hop = d->hop, pad = g.center_pad, L = (int)g.length, Tn = (int)g.n_frames;
        const bool plain = pad == 0 || g.pad_mode == PAD_CONSTANT;
        const OlaRuns runs = ola_runs_for(L, pad, hop, plan.n_fft, Tn, plain);
        const int ht_blocks = (runs.head + (runs.last_run + 1 - runs.tail_first) + 3) / 4;
        const long long zone_quads = (long long)(plan.segs_per_row - 1) * runs.zone_frames * (hop >> 2);
        if (zone_quads >= 0x7fffffffLL) return TAC_E_UNSUPPORTED;
        const int zone_blocks = (int)std::min<long long>((zone_quads + 255) / 256, 2 * per_row);
        if (ht_blocks + zone_blocks == 0) return TAC_OK;
        return launch_kernel(ola_fold_runs_kernel, dim3((unsigned)(zone_blocks + ht_blocks), fold_y), 256, 0, s, g, gpad, edge, plan, runs,
                             zone_blocks, grad_wave, (long long)grad_row_stride);
    }
    // ~16 workgroups per CU in flight, each thread walking its row with a stride: rows on y, a row's samples on x
    const unsigned fold_x = (unsigned)std::min<long long>((g.length + 1023) / 1024, per_row);
    return launch_kernel(ola_fold_kernel, dim3(fold_x, fold_y), 256, 0, s, g, gpad, edge, plan, grad_wave, (long long)grad_row_stride);
}
}  // namespace tac

extern "C" {

int tac_spectrogram_backward_ola_f32(const float* wave, const float* window, const tac_stft_desc* d, const float* grad_norm,
                                     float power, void* workspace, int64_t workspace_bytes, float* grad_wave,
                                     int64_t grad_row_stride, void* stream) {
    return tac::ola_backward_entry(wave, window, d, grad_norm, power, nullptr, 0, workspace, workspace_bytes, grad_wave,
                                   grad_row_stride, stream);
}

int tac_melspectrogram_backward_ola_f32(const float* wave, const float* window, const tac_stft_desc* d, const float* grad_mel,
                                        int32_t n_mels, const void* adjoint_table, int32_t n_freqs, float power,
                                        void* workspace, int64_t workspace_bytes, float* grad_wave, int64_t grad_row_stride,
                                        void* stream) {
    if (!adjoint_table || !d) return TAC_E_INVALID;
    if (n_freqs != d->n_fft / 2 + 1) return TAC_E_INVALID;
    return tac::ola_backward_entry(wave, window, d, grad_mel, power, static_cast<const tac::AdjEntry*>(adjoint_table), n_mels,
                                   workspace, workspace_bytes, grad_wave, grad_row_stride, stream);
}

int tac_overlap_add_f32(const float* grad_frames, const tac_stft_desc* d, float* grad_wave, int64_t grad_row_stride,
                        void* stream) {
    using namespace tac;
    if (!grad_frames || !grad_wave || !d) return TAC_E_INVALID;
    FrameGeom g;
    int64_t T = 0;
    float dummy_window = 0.0f;
    int rc = make_geometry(grad_frames, &dummy_window, d, &g, &T, true);     // framing only: any fft_length
    if (rc != TAC_OK) return rc;
    const int vec4 = ((d->hop & 3) == 0 && (d->n_fft & 3) == 0 && (g.center_pad & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(grad_frames) & 15u) == 0) ? 1 : 0;
    return launch_kernel(overlap_add_kernel, bw_blocks(g.rows * ((g.length + 3) / 4)), 256, 0, (hipStream_t)stream, g, (int)d->n_fft,
                         grad_frames, grad_wave, (long long)grad_row_stride, vec4);
}

int64_t tac_window_grad_partials(const tac_stft_desc* d) {
    if (!d || d->rows <= 0 || d->n_fft <= 0) return TAC_E_INVALID;
    const int64_t T = tac_num_frames(d->length, d->n_fft, d->hop, d->center);
    if (T <= 0) return TAC_E_SHORT_INPUT;
    const int64_t total = d->rows * T;
    const int64_t want = (int64_t)tac::device_cu_count() * 4;
    return total < want ? total : want;
}

int tac_window_grad_f32(const float* grad_frames_unwindowed, const float* wave, const tac_stft_desc* d, float* partial,
                        int64_t n_partials, void* stream) {
    using namespace tac;
    if (!grad_frames_unwindowed || !wave || !d || !partial || n_partials <= 0) return TAC_E_INVALID;
    FrameGeom g;
    int64_t T = 0;
    float dummy_window = 0.0f;
    int rc = make_geometry(wave, &dummy_window, d, &g, &T, true);
    if (rc != TAC_OK) return rc;
    const long long total = g.rows * (long long)T;
    const long long per = (total + n_partials - 1) / n_partials;
    return launch_kernel(window_grad_kernel, n_partials, 256, 0, (hipStream_t)stream, g, (int)d->n_fft, grad_frames_unwindowed, per, partial);
}

int tac_complex_norm_backward_f32(const float* z, const float* grad_out, int64_t n, float power, float* grad_z,
                                  void* stream) {
    using namespace tac;
    if (n == 0) return TAC_OK;
    if (!z || !grad_out || !grad_z || n < 0) return TAC_E_INVALID;
    return launch_kernel(complex_norm_backward_kernel, bw_blocks(n), 256, 0, (hipStream_t)stream, z, grad_out, (long long)n, power, grad_z);
}

int tac_magphase_backward_f32(const float* z, const float* grad_mag, const float* grad_phase, int64_t n, float power,
                              float* grad_z, void* stream) {
    using namespace tac;
    if (n == 0) return TAC_OK;
    if (!z || !grad_z || (!grad_mag && !grad_phase) || n < 0) return TAC_E_INVALID;
    return launch_kernel(magphase_backward_kernel, bw_blocks(n), 256, 0, (hipStream_t)stream, z, grad_mag, grad_phase, (long long)n, power,
                         grad_z);
}

int tac_db_to_amplitude_backward_f32(const float* x, const float* grad_out, int64_t n, float ref, float* grad_x, void* stream) {
    using namespace tac;
    if (n == 0) return TAC_OK;
    if (!x || !grad_out || !grad_x || n < 0 || !(ref > 0.0f)) return TAC_E_INVALID;
    return launch_kernel(db_to_amplitude_backward_kernel, bw_blocks(n), 256, 0, (hipStream_t)stream, x, grad_out, (long long)n, log10f(ref),
                         grad_x);
}

int tac_amplitude_to_db_backward_f32(const float* x, const float* grad_out, int64_t n, float amin, float* grad_x,
                                     void* stream) {
    using namespace tac;
    if (n == 0) return TAC_OK;
    if (!x || !grad_out || !grad_x || n < 0) return TAC_E_INVALID;
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(grad_x)) & 15u) == 0;
    return launch_kernel(vec ? amplitude_to_db_backward_kernel<true> : amplitude_to_db_backward_kernel<false>, bw_blocks(vec ? (n + 3) / 4 : n),
                         256, 0, (hipStream_t)stream, x, grad_out, (long long)n, amin, grad_x);
}

}  // extern "C"
