// rnnt.hip — the transducer loss (functional.rnnt_loss, RNNTLoss; Graves 2012, torchaudio's semantics) and its gradient over
// (B, T, U + 1, V) logits: three launches, the logits read once forward and once backward.
//
//   lp[t,u,v]  = logits[t,u,v] - denom[t,u],  denom = logsumexp_v logits[t,u,:]        (fused) or lp = logits, denom = 0
//   alpha[0,0] = 0,  alpha[t,u] = logaddexp(alpha[t-1,u] + lp[t-1,u,blank], alpha[t,u-1] + lp[t,u-1,targets[u-1]])
//   beta[Tb-1,Ub] = lp[Tb-1,Ub,blank],  beta[t,u] = logaddexp(beta[t+1,u] + lp[t,u,blank], beta[t,u+1] + lp[t,u,targets[u]])
//   cost = -(alpha[Tb-1,Ub] + lp[Tb-1,Ub,blank])
//
// (1) rnnt_rows_kernel: a group of G = 1 .. 64 lanes per (b, t, u) row, G chosen from V alone so that a lane owns up to four
//     16-byte chunks of the row per batch; a wave takes 64 / G rows.  Chunk c of a batch belongs to lane c % G (consecutive lanes on
//     consecutive chunks); a row of up to 16 G classes is one batch — read once, its maximum and its sum taken from registers — and
//     a longer row is reduced online over its batches (running maximum, rescaled sum), still in one read.  The lane owns the same
//     elements and adds them in the same order whether a chunk arrives as one 16-byte load (VEC: V % 4 == 0 and base and strides
//     keep every chunk aligned) or as four dwords, so both forms give the same bits.  The launch also gathers lp_blank and
//     lp_label, so the dynamic program never touches the logits, and writes zeros (denominator, both log-probabilities, alpha and
//     beta) for a row with t >= Tb or u > Ub without reading it.
// (2) rnnt_lattice_kernel: one workgroup per (entry, direction), lane u on column u (the mirrored column for beta), one
//     anti-diagonal per step: the lane keeps its own previous value in a register and takes its neighbour's by a one-lane wave
//     shift (DPP); from 65 columns on, waves hand their last lane's value over through two alternating LDS rows, one barrier a step.
//     The two log-probabilities of a step are loaded four groups of eight steps before their use; loads and stores are
//     unconditional at clamped indices, so that nothing on the chain of dependent steps waits for memory.  Fixed order, no atomics.
// (3) rnnt_grad_kernel: lanes as in (1); the four scalars of a row (alpha + cost - denom, beta[t,u], beta[t+1,u], beta[t,u+1]) are
//     loaded once, grad = exp(g + beta[t,u]) minus the blank and label terms, clamp, times grad_costs[b]; rows outside (Tb, Ub + 1)
//     are stored as zeros without being read.  Every element of grad_logits is written.
//
// An entry with Tb outside [1, T], Ub outside [0, U] or a used target outside [0, V) gets a NaN cost, NaN alpha / beta and a NaN
// gradient over its whole block; no address is formed from such a value.  Element offsets into the logits are 64-bit.
#include <math.h>

#include "host_common.hpp"

// the 16-byte and the dword form of a row must round alike: no contraction the compiler is free to apply in one and not the other
#pragma clang fp contract(off)

namespace tac {

constexpr int RN_THREADS = 256;
constexpr int RN_BATCH = 4;                     // 16-byte chunks of a lane per batch
constexpr int RN_MAX_TARGETS = 1024;            // the most U + 1: one lane per column in one workgroup
constexpr int RN_AHEAD = 8;                     // steps of the lattice in a group: their log-probabilities are loaded together,
constexpr int RN_DEPTH = 4;                     // this many groups ahead of their use

struct RnntGeom {
    long long sb, st, su;                       // element strides of the logits (the class axis has unit stride)
    int B, T, U1, V;                            // U1 = U + 1
    int blank;
    unsigned rows;                              // B T U1 < 2^31
};

// chunk c (elements 4c .. 4c + 3) of a row: one 16-byte load, or four dwords with -inf past the row's end
template <bool VEC>
__device__ __forceinline__ void rn_load_chunk(const float* __restrict__ row, int c, int V, int nchunks, float* x) {
    const float ninf = -INFINITY;
    x[0] = x[1] = x[2] = x[3] = ninf;
    if (c < nchunks) {
        if constexpr (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(row + 4 * (long long)c);
            x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
        } else {
            const int e = 4 * c;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (e + i < V) x[i] = row[e + i];
        }
    }
}

struct RnntRow {
    unsigned r;
    int b, t, u, Tb, Ub;
    bool in, entry_ok, inside;
};

__device__ __forceinline__ RnntRow rn_row(const RnntGeom& g, unsigned long long r64, const int* __restrict__ tlen,
                                          const int* __restrict__ ulen) {
    RnntRow w;
    w.in = r64 < g.rows;
    w.r = w.in ? (unsigned)r64 : 0u;
    const unsigned bt = w.r / (unsigned)g.U1;
    w.u = (int)(w.r - bt * (unsigned)g.U1);
    w.b = (int)(bt / (unsigned)g.T);
    w.t = (int)(bt - (unsigned)w.b * (unsigned)g.T);
    w.Tb = tlen[w.b];
    w.Ub = ulen[w.b];
    w.entry_ok = w.Tb >= 1 && w.Tb <= g.T && w.Ub >= 0 && w.Ub <= g.U1 - 1;
    w.inside = w.in && w.entry_ok && w.t < w.Tb && w.u <= w.Ub;
    return w;
}

template <int LOG_G, bool VEC, bool FUSED>
__global__ void __launch_bounds__(RN_THREADS)
rnnt_rows_kernel(const float* __restrict__ logits, RnntGeom g, const int* __restrict__ targets, const int* __restrict__ tlen,
                 const int* __restrict__ ulen, float* __restrict__ denom, float* __restrict__ lp_blank, float* __restrict__ lp_label,
                 float* __restrict__ alphas, float* __restrict__ betas) {
    constexpr int G = 1 << LOG_G, RPB = RN_THREADS >> LOG_G;
    const int lane = threadIdx.x & (G - 1), sub = threadIdx.x >> LOG_G;
    const int nchunks = (g.V + 3) >> 2;
    const float ninf = -INFINITY;
    for (unsigned long long r0 = (unsigned long long)blockIdx.x * RPB; r0 < g.rows; r0 += (unsigned long long)gridDim.x * RPB) {
        const RnntRow w = rn_row(g, r0 + sub, tlen, ulen);          // (the same in every lane of a group)
        float d = 0.0f, pb = 0.0f, pl = 0.0f;
        if (w.inside) {
            const float* row = logits + w.b * g.sb + w.t * g.st + w.u * g.su;
            if constexpr (FUSED) {
                float m = ninf, s = 0.0f;
#pragma unroll 1
                for (int c0 = 0; c0 < nchunks; c0 += RN_BATCH * G) {
                    float x[4 * RN_BATCH];
#pragma unroll
                    for (int j = 0; j < RN_BATCH; ++j) rn_load_chunk<VEC>(row, c0 + j * G + lane, g.V, nchunks, x + 4 * j);
                    float bm = x[0];
#pragma unroll
                    for (int i = 1; i < 4 * RN_BATCH; ++i) bm = fmaxf(bm, x[i]);
                    const float mn = fmaxf(m, bm), mm = mn == ninf ? 0.0f : mn;
                    float acc = 0.0f;
#pragma unroll
                    for (int i = 0; i < 4 * RN_BATCH; ++i) acc += __expf(x[i] - mm);
                    s = s * __expf(m - mm) + acc;
                    m = mn;
                }
                float ma = m;
#pragma unroll
                for (int off = G >> 1; off > 0; off >>= 1) ma = fmaxf(ma, __shfl_xor(ma, off));
                const float mm = ma == ninf ? 0.0f : ma;
                s = s * __expf(m - mm);
#pragma unroll
                for (int off = G >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off);
                d = mm + logf(s);
            }
            if (lane == 0) {
                pb = row[g.blank] - d;
                if (w.u < w.Ub) {
                    const int lab = targets[(long long)w.b * (g.U1 - 1) + w.u];
                    pl = (lab >= 0 && lab < g.V) ? row[lab] - d : NAN;
                }
            }
        }
        if (w.in && lane == 0) {
            denom[w.r] = d;
            lp_blank[w.r] = pb;
            lp_label[w.r] = pl;
            if (!w.inside) alphas[w.r] = betas[w.r] = w.entry_ok ? 0.0f : NAN;
        }
    }
}

// logaddexp with logaddexp(-inf, -inf) = -inf; a NaN on either side stays a NaN
__device__ __forceinline__ float rn_logaddexp(float a, float b) {
    const float d = a == b ? 0.0f : a - b;
    return fmaxf(a, b) + __logf(1.0f + __expf(-fabsf(d)));
}

// lane i receives lane i - 1's value (lane 0: unspecified, replaced by the caller)
__device__ __forceinline__ float rn_from_lower_lane(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

template <bool MANY>                            // more than one wave: the boundary value goes through the LDS, a barrier a step
__global__ void __launch_bounds__(MANY ? RN_MAX_TARGETS : 64)
rnnt_lattice_kernel(RnntGeom g, const int* __restrict__ targets, const int* __restrict__ tlen, const int* __restrict__ ulen,
                    const float* __restrict__ lp_blank, const float* __restrict__ lp_label, float* __restrict__ alphas,
                    float* __restrict__ betas, float* __restrict__ costs) {
    __shared__ float edge[2][RN_MAX_TARGETS / 64];
    const int b = blockIdx.x >> 1, dir = blockIdx.x & 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = g.T, U1 = g.U1;
    const int Tb = tlen[b], Ub = ulen[b];
    const long long base = (long long)b * T * U1;
    float* __restrict__ out = (dir ? betas : alphas) + base;
    const float* __restrict__ pb = lp_blank + base;
    const float* __restrict__ pl = lp_label + base;
    const float ninf = -INFINITY;

    int bad = Tb < 1 || Tb > T || Ub < 0 || Ub > U1 - 1;
    if (!bad)
        for (int u = tid; u < Ub; u += blockDim.x) {
            const int lab = targets[(long long)b * (U1 - 1) + u];
            bad |= lab < 0 || lab >= g.V;
        }
    bad = __syncthreads_or(bad);
    if (bad) {
        for (int i = tid; i < T * U1; i += blockDim.x) out[i] = NAN;
        if (dir == 0 && tid == 0) costs[b] = NAN;
        return;
    }

    // Thread tid (there are U + 1) on column tid of its direction; step d visits the cell with row index tt = d - tid.  For alpha
    // (row, column) = (t, u); for beta they count from the far corner: (Tb - 1 - t, Ub - u).  Every load and the store of a step are
    // unconditional, at an index clamped into the entry's own lattice, and the values are selected afterwards: the loads of a
    // group of steps are then in flight together and nothing on the chain waits for a store.  A thread ahead of its first cell
    // stores -inf there and overwrites it when it arrives (stores of one thread to one address keep their order); behind its
    // last cell it stores that cell's value again; a thread on a column beyond Ub stores the zeros those cells already hold.
    const bool col = tid <= Ub;
    const int cu = col ? (dir ? Ub - tid : tid) : tid;
    const int nsteps = Tb + Ub;
    auto cell_of = [&](int tt) {
        const int ttc = min(max(tt, 0), Tb - 1);
        return (dir ? Tb - 1 - ttc : ttc) * U1 + cu;
    };
    // the two log-probabilities of step d: P beside the thread's own previous value, L beside its neighbour's
    auto fetch = [&](int d, float& P, float& L) {
        const int cell = cell_of(d - tid);
        P = pb[dir ? cell : max(cell - U1, cu)];
        L = pl[dir ? cell : max(cell - 1, 0)];
    };
    float a = col ? ninf : 0.0f;
    float P[RN_DEPTH][RN_AHEAD], L[RN_DEPTH][RN_AHEAD];             // a ring of groups of steps, every index static
#pragma unroll
    for (int s = 0; s < RN_DEPTH; ++s)
#pragma unroll
        for (int k = 0; k < RN_AHEAD; ++k) fetch(s * RN_AHEAD + k, P[s][k], L[s][k]);
#pragma unroll 1
    for (int d0 = 0; d0 < nsteps; d0 += RN_DEPTH * RN_AHEAD) {
#pragma unroll
        for (int s = 0; s < RN_DEPTH; ++s) {
            const int ds = d0 + s * RN_AHEAD;
            if (ds >= nsteps) break;                                // (the same in every thread; a last group may run past nsteps:
                                                                    //  those steps visit no cell)
            float Pc[RN_AHEAD], Lc[RN_AHEAD];
#pragma unroll
            for (int k = 0; k < RN_AHEAD; ++k) Pc[k] = P[s][k], Lc[k] = L[s][k];
#pragma unroll
            for (int k = 0; k < RN_AHEAD; ++k) fetch(ds + RN_DEPTH * RN_AHEAD + k, P[s][k], L[s][k]);
#pragma unroll
            for (int k = 0; k < RN_AHEAD; ++k) {
                const int d = ds + k, tt = d - tid;
                float left = rn_from_lower_lane(a);
                if constexpr (MANY) {
                    if (lane == 63) edge[d & 1][wave] = a;
                    __syncthreads();
                    if (lane == 0 && wave > 0) left = edge[d & 1][wave - 1];
                }
                const bool on = col && tt >= 0 && tt < Tb;
                const float up = (dir ? (tt >= 1 || tid == 0) : tt >= 1) ? a + Pc[k] : ninf;     // (the far corner itself is lp_blank)
                const float lf = tid >= 1 ? left + Lc[k] : ninf;
                float v = rn_logaddexp(up, lf);
                if (d == 0 && tid == 0) v = dir ? Pc[k] : 0.0f;
                a = on ? v : a;
                out[cell_of(tt)] = a;
            }
        }
    }
    if (dir == 0 && tid == Ub) costs[b] = -(a + pb[(Tb - 1) * U1 + Ub]);
}

template <int LOG_G, bool VEC, bool FUSED>
__global__ void __launch_bounds__(RN_THREADS)
rnnt_grad_kernel(const float* __restrict__ logits, RnntGeom g, const int* __restrict__ targets, const int* __restrict__ tlen,
                 const int* __restrict__ ulen, const float* __restrict__ alphas, const float* __restrict__ betas,
                 const float* __restrict__ denom, const float* __restrict__ costs, const float* __restrict__ grad_costs, float clamp,
                 float* __restrict__ grad) {
    constexpr int G = 1 << LOG_G, RPB = RN_THREADS >> LOG_G;
    const int lane = threadIdx.x & (G - 1), sub = threadIdx.x >> LOG_G;
    const int nchunks = (g.V + 3) >> 2;
    const float ninf = -INFINITY;
    for (unsigned long long r0 = (unsigned long long)blockIdx.x * RPB; r0 < g.rows; r0 += (unsigned long long)gridDim.x * RPB) {
        const RnntRow w = rn_row(g, r0 + sub, tlen, ulen);
        if (!w.in) continue;
        float* __restrict__ dst = grad + (long long)w.r * g.V;
        const float cost = costs[w.b];
        const bool lost = !w.entry_ok || cost != cost;              // (an entry the lattice launch marked: NaN over its whole block)
        const bool live = w.inside && !lost;
        const float* row = logits + w.b * g.sb + w.t * g.st + w.u * g.su;
        float c = 0.0f, bt = 0.0f, sb = ninf, sl = ninf, gc = 0.0f;
        int lab = -1;
        if (live) {
            c = (alphas[w.r] + cost) - denom[w.r];
            bt = betas[w.r];
            sb = w.t < w.Tb - 1 ? betas[w.r + g.U1] : (w.u == w.Ub ? 0.0f : ninf);
            if (w.u < w.Ub) {
                sl = betas[w.r + 1];
                lab = targets[(long long)w.b * (g.U1 - 1) + w.u];
            }
            gc = grad_costs[w.b];
        }
        const float fill = lost ? NAN : 0.0f;
#pragma unroll 1
        for (int c0 = 0; c0 < nchunks; c0 += RN_BATCH * G) {
            float x[4 * RN_BATCH];
            if (FUSED && live) {
#pragma unroll
                for (int j = 0; j < RN_BATCH; ++j) rn_load_chunk<VEC>(row, c0 + j * G + lane, g.V, nchunks, x + 4 * j);
            }
#pragma unroll
            for (int j = 0; j < RN_BATCH; ++j) {
                const int ch = c0 + j * G + lane, e = 4 * ch;
                if (ch >= nchunks) continue;
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = fill;
                if (live) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = FUSED ? __expf((x[4 * j + i] + c) + bt) : 0.0f;
                    if ((unsigned)(g.blank - e) < 4u || (unsigned)(lab - e) < 4u) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            if (e + i == g.blank || e + i == lab) {
                                const float xv = FUSED ? x[4 * j + i] : row[e + i];
                                if (e + i == g.blank) v[i] -= __expf((xv + c) + sb);
                                if (e + i == lab) v[i] -= __expf((xv + c) + sl);
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (clamp > 0.0f) v[i] = fminf(fmaxf(v[i], -clamp), clamp);
                        v[i] *= gc;
                    }
                }
                if constexpr (VEC) {
                    *reinterpret_cast<float4*>(dst + e) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (e + i < g.V) dst[e + i] = v[i];
                }
            }
        }
    }
}

// lanes per row: the fewest (a power of two, 64 at most) that hold the row's 16-byte chunks in one batch
inline int rn_log_g(long long V) {
    const long long chunks = (V + 3) / 4;
    int l = 0;
    while (l < 6 && (long long)RN_BATCH << l < chunks) ++l;
    return l;
}

inline int rn_geometry(const float* logits, int64_t batch, int64_t frames, int64_t targets1, int64_t classes, int64_t stride_b,
                       int64_t stride_t, int64_t stride_u, int32_t blank, RnntGeom* g) {
    if (!logits || batch <= 0 || frames <= 0 || targets1 <= 0 || classes <= 0) return TAC_E_INVALID;
    if (blank < 0 || blank >= classes) return TAC_E_INVALID;
    if (batch == 1) stride_b = 0;
    if (frames == 1) stride_t = 0;
    if (targets1 == 1) stride_u = 0;
    if ((batch > 1 && stride_b <= 0) || (frames > 1 && stride_t <= 0) || (targets1 > 1 && stride_u <= 0)) return TAC_E_INVALID;
    if (targets1 > RN_MAX_TARGETS || classes > 0x3fffffff) return TAC_E_UNSUPPORTED;
    if ((double)batch * (double)frames * (double)targets1 >= 2147483648.0) return TAC_E_UNSUPPORTED;
    g->sb = stride_b, g->st = stride_t, g->su = stride_u;
    g->B = (int)batch, g->T = (int)frames, g->U1 = (int)targets1, g->V = (int)classes;
    g->blank = blank;
    g->rows = (unsigned)(batch * frames * targets1);
    return TAC_OK;
}

inline bool rn_vec(const RnntGeom& g, const float* logits) {
    return g.V % 4 == 0 && g.sb % 4 == 0 && g.st % 4 == 0 && g.su % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
}

inline long long rn_blocks(const RnntGeom& g, int log_g) {
    return persistent_blocks((long long)g.rows, RN_THREADS >> log_g, (long long)device_cu_count() * 32);
}

#define RN_PICK(KERNEL, FUSED, kern)                                                                       \
    do {                                                                                                   \
        switch (log_g) {                                                                                   \
            case 0: kern = vec ? KERNEL<0, true, FUSED> : KERNEL<0, false, FUSED>; break;                  \
            case 1: kern = vec ? KERNEL<1, true, FUSED> : KERNEL<1, false, FUSED>; break;                  \
            case 2: kern = vec ? KERNEL<2, true, FUSED> : KERNEL<2, false, FUSED>; break;                  \
            case 3: kern = vec ? KERNEL<3, true, FUSED> : KERNEL<3, false, FUSED>; break;                  \
            case 4: kern = vec ? KERNEL<4, true, FUSED> : KERNEL<4, false, FUSED>; break;                  \
            case 5: kern = vec ? KERNEL<5, true, FUSED> : KERNEL<5, false, FUSED>; break;                  \
            default: kern = vec ? KERNEL<6, true, FUSED> : KERNEL<6, false, FUSED>; break;                 \
        }                                                                                                  \
    } while (0)

}  // namespace tac

extern "C" {

int32_t tac_rnnt_max_targets(void) { return tac::RN_MAX_TARGETS; }

int tac_rnnt_rows_f32(const float* logits, int64_t batch, int64_t frames, int64_t targets1, int64_t classes, int64_t stride_b,
                      int64_t stride_t, int64_t stride_u, const int32_t* targets, const int32_t* logit_lengths,
                      const int32_t* target_lengths, int32_t blank, int32_t fused, float* denominators, float* lp_blank,
                      float* lp_label, float* alphas, float* betas, void* stream) {
    using namespace tac;
    RnntGeom g;
    const int rc = rn_geometry(logits, batch, frames, targets1, classes, stride_b, stride_t, stride_u, blank, &g);
    if (rc != TAC_OK) return rc;
    if (!logit_lengths || !target_lengths || !denominators || !lp_blank || !lp_label || !alphas || !betas) return TAC_E_INVALID;
    if (targets1 > 1 && !targets) return TAC_E_INVALID;
    if (!fused) {                                                   // only the gather: a lane per row
        return launch_kernel(rnnt_rows_kernel<0, false, false>, rn_blocks(g, 0), RN_THREADS, 0, (hipStream_t)stream, logits, g,
                             (const int*)targets, (const int*)logit_lengths, (const int*)target_lengths, denominators, lp_blank,
                             lp_label, alphas, betas);
    }
    const int log_g = rn_log_g(g.V);
    const bool vec = rn_vec(g, logits);
    void (*kern)(const float*, RnntGeom, const int*, const int*, const int*, float*, float*, float*, float*, float*);
    RN_PICK(rnnt_rows_kernel, true, kern);
    return launch_kernel(kern, rn_blocks(g, log_g), RN_THREADS, 0, (hipStream_t)stream, logits, g, (const int*)targets,
                         (const int*)logit_lengths, (const int*)target_lengths, denominators, lp_blank, lp_label, alphas, betas);
}

int tac_rnnt_lattice_f32(int64_t batch, int64_t frames, int64_t targets1, int64_t classes, const int32_t* targets,
                         const int32_t* logit_lengths, const int32_t* target_lengths, const float* lp_blank, const float* lp_label,
                         float* alphas, float* betas, float* costs, void* stream) {
    using namespace tac;
    RnntGeom g;
    static const float dummy = 0.0f;
    const int rc = rn_geometry(&dummy, batch, frames, targets1, classes, 1, 1, 1, 0, &g);
    if (rc != TAC_OK) return rc;
    if (!logit_lengths || !target_lengths || !lp_blank || !lp_label || !alphas || !betas || !costs) return TAC_E_INVALID;
    if (targets1 > 1 && !targets) return TAC_E_INVALID;
    const int threads = (int)targets1;                              // a thread per column; the last wave may be partial
    return launch_kernel(threads > 64 ? rnnt_lattice_kernel<true> : rnnt_lattice_kernel<false>, 2 * batch, threads, 0, (hipStream_t)stream, g, (const int*)targets,
                         (const int*)logit_lengths, (const int*)target_lengths, lp_blank, lp_label, alphas, betas, costs);
}

int tac_rnnt_grad_f32(const float* logits, int64_t batch, int64_t frames, int64_t targets1, int64_t classes, int64_t stride_b,
                      int64_t stride_t, int64_t stride_u, const int32_t* targets, const int32_t* logit_lengths,
                      const int32_t* target_lengths, const float* alphas, const float* betas, const float* denominators,
                      const float* costs, const float* grad_costs, int32_t blank, float clamp, int32_t fused, float* grad_logits,
                      void* stream) {
    using namespace tac;
    RnntGeom g;
    const int rc = rn_geometry(logits, batch, frames, targets1, classes, stride_b, stride_t, stride_u, blank, &g);
    if (rc != TAC_OK) return rc;
    if (!logit_lengths || !target_lengths || !alphas || !betas || !denominators || !costs || !grad_costs || !grad_logits)
        return TAC_E_INVALID;
    if (targets1 > 1 && !targets) return TAC_E_INVALID;
    const int log_g = rn_log_g(g.V);
    const bool vec = rn_vec(g, logits) && (reinterpret_cast<uintptr_t>(grad_logits) & 15) == 0;
    void (*kern)(const float*, RnntGeom, const int*, const int*, const int*, const float*, const float*, const float*, const float*,
                 const float*, float, float*);
    if (fused)
        RN_PICK(rnnt_grad_kernel, true, kern);
    else
        RN_PICK(rnnt_grad_kernel, false, kern);
    return launch_kernel(kern, rn_blocks(g, log_g), RN_THREADS, 0, (hipStream_t)stream, logits, g, (const int*)targets,
                         (const int*)logit_lengths, (const int*)target_lengths, alphas, betas, denominators, costs, grad_costs, clamp,
                         grad_logits);
}

}  // extern "C"
