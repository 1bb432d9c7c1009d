// ctc_loss.hip — the CTC loss (functional.ctc_loss, CTCLoss; Graves 2006, torch.nn.functional.ctc_loss's semantics) and its gradient
// over time-major (T, N, C) log-probabilities read where they lie: one launch forward, one backward.
//
//   states s = 0 .. 2 Lb: even ones carry the blank, s = 2k + 1 carries targets[k]
//   alpha[0][0] = lp[0][blank], alpha[0][1] = lp[0][targets[0]], -inf elsewhere
//   alpha[t][s] = logsumexp(alpha[t-1][s], alpha[t-1][s-1], alpha[t-1][s-2] for odd s >= 3 whose label differs from the one before)
//                 + lp[t][label(s)]
//   beta: the same recursion from frame Tb - 1 and state 2 Lb downwards;  cost = -logaddexp(alpha[Tb-1][2 Lb], alpha[Tb-1][2 Lb - 1])
//   grad[t][c] = (exp(lp[t][c]) - exp(logsumexp_{s: label(s) = c}(alpha[t][s] + beta[t][s]) + cost - lp[t][c])) grad_costs[b]
//
// (1) ctc_lattice_kernel: one workgroup per (entry, direction); the alpha workgroups alone when no gradient is wanted, and then
//     nothing but the costs is written.  Lane q owns the PAIR (blank before label q, label q) as in align.hip; the one value a step
//     needs from another lane is label q - 1's, a one-lane wave shift, and from 65 pairs on the waves hand their last lane's value
//     over through two alternating LDS rows, one barrier a step.  BETA RUNS THE SAME CODE ON THE MIRRORED ENTRY: lane q of a beta
//     workgroup owns (blank after label Lb - 1 - q, label Lb - 1 - q) and walks the frames from Tb - 1 down — with states and time
//     reversed the beta recursion IS the alpha recursion, so the neighbour is again the lower lane and no second code path (and
//     no second, upward shift) exists.  A step of a lane is one two-way and one three-way logsumexp: a maximum, the exponentials of
//     the differences, one logarithm; an all -inf maximum is replaced by 0 before the differences, so -inf stays -inf and never
//     becomes NaN.  The first frame needs no case of its own: lane 0 starts from alpha_blank = 0 and the step gives lp[0][blank]
//     and lp[0][targets[0]] exactly.  Emissions (the blank's column through a lane register, so that it is a vector load) are
//     loaded CT_AHEAD steps at a time, CT_DEPTH groups ahead of their use, at clamped frames.
//     Outputs: alphas, betas float32 (N, T, 2 S + 1), every element written: ZERO outside an entry's (Tb, 2 Lb + 1) lattice.
// (2) ctc_grad_kernel: a workgroup per (entry, tile of frames), a wave per frame at a time.  Once per workgroup, in the LDS, from
//     the entry's targets: the labels ranked by (label, index) with a count-rank (order[]), the distinct labels numbered in
//     ascending order (slots 1 .., slot 0 is the blank), where each slot's group starts in order[], and the 16-bit table slot[c].
//     Per frame the wave puts alpha + beta of the 2 Lb + 1 states into its LDS row (coalesced), reduces the blank's Lb + 1 states by
//     a fixed tree (lane l takes states l, l + 64, … in turn, then a butterfly over the lanes) and each label slot's group in the
//     order of order[] by one lane (maximum, then the sum of exponentials), and then streams the class row: 16-byte loads and
//     stores where bases, strides and C % 4 allow, dwords otherwise, the same arithmetic on the same elements in both forms.
//     Frames t >= Tb are stored as zeros without a load.  No atomics anywhere; every sum has one fixed order.
//
// An entry with Tb outside [1, T], Lb outside [0, S], targets that leave their tensor, or a used target that is the blank or
// outside [0, C) gets a NaN cost, NaN alphas / betas and a NaN gradient over its whole block; no address is formed from such a
// value.  An infeasible entry (Tb < Lb + repeats) runs like any other and ends with cost +inf; its gradient is 0 everywhere with
// zero_infinity, else NaN for t < Tb and 0 behind, as torch gives on the CPU.  Element offsets are 64-bit.
#include <math.h>

#include "ctc_loss_plan.hpp"
#include "host_common.hpp"

// the 16-byte and the dword form of a class row must round alike
#pragma clang fp contract(off)

namespace tac {

struct CtcGeom {
    long long st, sn, sc;                       // element strides of log_probs (T, N, C)
    long long gt, gn, gc;                       // element strides of the gradient
    long long total;                            // elements of the targets tensor
    int T, N, C, S;                             // S: the target axis (the lattice arrays are 2 S + 1 wide)
    int blank;
    int tile;                                   // frames of a gradient tile
    int zero_inf;
};

// lane i receives lane i - 1's value (lane 0: unspecified, replaced by the caller)
__device__ __forceinline__ float ct_from_lower_lane(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

__device__ __forceinline__ float ct_lse2(float a, float b) {
    const float m = fmaxf(a, b), mm = m == -INFINITY ? 0.0f : m;
    return m + __logf(__expf(a - mm) + __expf(b - mm));
}

__device__ __forceinline__ float ct_lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c), mm = m == -INFINITY ? 0.0f : m;
    return m + __logf((__expf(a - mm) + __expf(b - mm)) + __expf(c - mm));
}

// the entry's lengths and where its targets start; false: outside the tensors (NaN)
template <typename IT>
__device__ __forceinline__ bool ct_entry(const CtcGeom& g, int b, const int* __restrict__ ilen, const int* __restrict__ tlen,
                                         const long long* __restrict__ offsets, int& Tb, int& Lb, long long& off) {
    Tb = ilen[b], Lb = tlen[b];
    off = offsets ? offsets[b] : (long long)b * g.S;
    bool ok = Tb >= 1 && Tb <= g.T && Lb >= 0;
    if (offsets)
        ok = ok && off >= 0 && off <= g.total && (long long)Lb <= g.total - off;
    else
        ok = ok && Lb <= g.S;
    return ok;
}

template <bool MANY, bool STORE, typename IT>   // MANY: more than one wave; STORE: the lattice arrays are wanted
__global__ void __launch_bounds__(MANY ? CT_MAX_TARGETS : 64)
ctc_lattice_kernel(const float* __restrict__ lp_all, CtcGeom g, const IT* __restrict__ targets_all, const int* __restrict__ ilen,
                   const int* __restrict__ tlen, const long long* __restrict__ offsets, float* __restrict__ alphas,
                   float* __restrict__ betas, float* __restrict__ costs) {
    __shared__ float edge[2][CT_MAX_TARGETS / 64];
    const int b = STORE ? blockIdx.x >> 1 : blockIdx.x, dir = STORE ? blockIdx.x & 1 : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = g.T, C = g.C, blank = g.blank, W = 2 * g.S + 1;
    const float ninf = -INFINITY;
    float* __restrict__ out = STORE ? (dir ? betas : alphas) + (long long)b * T * W : nullptr;

    int Tb, Lb;
    long long off;
    const bool lens_ok = ct_entry<IT>(g, b, ilen, tlen, offsets, Tb, Lb, off);
    const bool over = lens_ok && Lb > g.S;      // (concatenated targets only) more targets than frames: infeasible
    const IT* __restrict__ targets = targets_all + (lens_ok ? off : 0ll);

    // ---- lane q's label: targets[q] for alpha, targets[Lb - 1 - q] for beta; its range; whether it differs from the lane below's
    const int q = tid;
    const bool has_label = lens_ok && !over && q < Lb;
    int bad = !lens_ok, lab = blank;
    bool skip = false;
    if (has_label) {
        const int k = dir ? Lb - 1 - q : q;
        const long long v = (long long)targets[k];
        const bool in = v >= 0 && v < C && v != blank;
        bad |= !in;
        lab = in ? (int)v : blank;
        if (q >= 1) skip = (long long)targets[dir ? k + 1 : k - 1] != v;
    }
    bad = __syncthreads_or(bad);
    if (bad || over) {
        if constexpr (STORE)
            for (long long i = tid; i < (long long)T * W; i += blockDim.x) out[i] = bad ? NAN : 0.0f;
        if (dir == 0 && tid == 0) costs[b] = bad ? NAN : INFINITY;
        return;
    }

    // ---- where the lane's two values go: states (2q, 2q + 1), mirrored for beta; lane Lb has the last blank alone; the lanes
    // beyond fill states 2q - 1 and 2q with zeros, as all lanes fill the frames t >= Tb
    int s0, s1;
    if (q < Lb) s0 = dir ? 2 * Lb - 2 * q : 2 * q, s1 = dir ? s0 - 1 : s0 + 1;
    else if (q == Lb) s0 = dir ? 0 : 2 * Lb, s1 = -1;
    else s0 = 2 * q - 1, s1 = 2 * q;
    if (s0 >= W) s0 = -1;                       // (whole waves are launched: lanes beyond S own nothing)
    if (s1 >= W) s1 = -1;
    const bool inside = q <= Lb;
    if constexpr (STORE)
        for (long long i = (long long)Tb * W + tid; i < (long long)T * W; i += blockDim.x) out[i] = 0.0f;

    const float* __restrict__ lp = lp_all + b * g.sn;
    int vblank = blank;
    asm volatile("" : "+v"(vblank));            // the blank's column as a vector load, counted with the label's (align.hip)
    const long long offb = vblank * g.sc, offl = lab * g.sc;
    auto frame_of = [&](int i) {                // step i visits frame i (alpha) or Tb - 1 - i (beta)
        const int ic = min(i, Tb - 1);
        return dir ? Tb - 1 - ic : ic;
    };
    auto fetch = [&](int i, float& eb, float& el) {
        const float* row = lp + (long long)frame_of(i) * g.st;
        eb = row[offb];
        el = row[offl];
    };
    float ab = q == 0 ? 0.0f : ninf, al = ninf; // before the first frame: the step then yields lp[0][blank] and lp[0][targets[0]]
    float EB[CT_DEPTH][CT_AHEAD], EL[CT_DEPTH][CT_AHEAD];           // a ring of groups of steps, every index static
#pragma unroll
    for (int s = 0; s < CT_DEPTH; ++s)
#pragma unroll
        for (int k = 0; k < CT_AHEAD; ++k) fetch(s * CT_AHEAD + k, EB[s][k], EL[s][k]);
    const int nsteps = Tb;
#pragma unroll 1
    for (int d0 = 0; d0 < nsteps; d0 += CT_DEPTH * CT_AHEAD) {
#pragma unroll
        for (int s = 0; s < CT_DEPTH; ++s) {
            const int ds = d0 + s * CT_AHEAD;
            if (ds >= nsteps) break;                                // (the same in every thread)
            float eb[CT_AHEAD], el[CT_AHEAD];
#pragma unroll
            for (int k = 0; k < CT_AHEAD; ++k) eb[k] = EB[s][k], el[k] = EL[s][k];
#pragma unroll
            for (int k = 0; k < CT_AHEAD; ++k) fetch(ds + CT_DEPTH * CT_AHEAD + k, EB[s][k], EL[s][k]);
#pragma unroll
            for (int k = 0; k < CT_AHEAD; ++k) {
                const int d = ds + k;
                if (d >= nsteps) break;                             // (the same in every thread)
                float prev = ct_from_lower_lane(al);                // label q - 1
                if constexpr (MANY) {
                    if (lane == 63) edge[d & 1][wave] = al;
                    __syncthreads();
                    if (lane == 0 && wave > 0) prev = edge[d & 1][wave - 1];
                }
                if (q == 0) prev = ninf;
                const float nb = ct_lse2(ab, prev) + eb[k];
                const float nl = ct_lse3(al, ab, skip ? prev : ninf) + el[k];
                ab = inside ? nb : ninf;
                al = has_label ? nl : ninf;
                if constexpr (STORE) {
                    float* __restrict__ row = out + (long long)frame_of(d) * W;
                    if (s0 >= 0) row[s0] = inside ? ab : 0.0f;
                    if (s1 >= 0) row[s1] = inside ? al : 0.0f;
                }
            }
        }
    }
    if (dir == 0) {                             // the cost: lane Lb has the last blank, the last label comes from the lane below
        float prev = ct_from_lower_lane(al);
        if constexpr (MANY) {
            if (lane == 63) edge[nsteps & 1][wave] = al;
            __syncthreads();
            if (lane == 0 && wave > 0) prev = edge[nsteps & 1][wave - 1];
        }
        if (q == 0) prev = ninf;
        if (q == Lb) costs[b] = -ct_lse2(ab, prev);
    }
}

__device__ __forceinline__ void ct_wave_sync() {                    // a wave's lanes read what its other lanes put into the LDS
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float ct_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float ct_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one class row of the gradient: LIVE rows are read and corrected through slot[], the others filled
template <bool VEC, bool LIVE>
__device__ __forceinline__ void ct_row(const float* __restrict__ src, long long sc, float* __restrict__ dst, long long gc, int C,
                                       int lane, const unsigned short* __restrict__ slot, const float* __restrict__ corr, float go,
                                       float fill) {
    const int nchunks = (C + 3) >> 2;
#pragma unroll 1
    for (int c0 = 0; c0 < nchunks; c0 += 64 * CT_GRAD_BATCH) {
        float x[CT_GRAD_BATCH][4];
        if constexpr (LIVE) {
#pragma unroll
            for (int j = 0; j < CT_GRAD_BATCH; ++j) {
                const int ch = c0 + j * 64 + lane, e = 4 * ch;
                x[j][0] = x[j][1] = x[j][2] = x[j][3] = 0.0f;
                if (ch >= nchunks) continue;
                if constexpr (VEC) {
                    const float4 v = *reinterpret_cast<const float4*>(src + e);
                    x[j][0] = v.x, x[j][1] = v.y, x[j][2] = v.z, x[j][3] = v.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (e + i < C) x[j][i] = src[(e + i) * sc];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CT_GRAD_BATCH; ++j) {
            const int ch = c0 + j * 64 + lane, e = 4 * ch;
            if (ch >= nchunks) continue;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = fill;
                if constexpr (LIVE) {
                    if (e + i < C) {
                        const unsigned sl = slot[e + i];
                        float y = __expf(x[j][i]);
                        if (sl != 0xffffu) y -= __expf(corr[sl] - x[j][i]);
                        v[i] = y * go;
                    }
                }
            }
            if constexpr (VEC) {
                *reinterpret_cast<float4*>(dst + e) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (e + i < C) dst[(e + i) * gc] = v[i];
            }
        }
    }
}

template <bool VEC, typename IT>
__global__ void __launch_bounds__(64 * CT_GRAD_WAVES)
ctc_grad_kernel(const float* __restrict__ lp_all, CtcGeom g, CtcGradLds L, const IT* __restrict__ targets_all,
                const int* __restrict__ ilen, const int* __restrict__ tlen, const long long* __restrict__ offsets,
                const float* __restrict__ alphas, const float* __restrict__ betas, const float* __restrict__ costs,
                const float* __restrict__ grad_costs, float* __restrict__ grad_all, int tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = g.T, C = g.C, blank = g.blank, W = 2 * g.S + 1;
    const float ninf = -INFINITY;
    float* rowbuf = reinterpret_cast<float*>(lds + L.row) + wave * L.row_len;
    float* corr = reinterpret_cast<float*>(lds + L.corr) + wave * L.corr_len;
    int* labs = reinterpret_cast<int*>(lds + L.labs);
    unsigned short* order = reinterpret_cast<unsigned short*>(lds + L.order);
    unsigned short* start = reinterpret_cast<unsigned short*>(lds + L.start);
    unsigned short* first = reinterpret_cast<unsigned short*>(lds + L.first);
    unsigned short* slot = reinterpret_cast<unsigned short*>(lds + L.slot);
    __shared__ int nslots_s;

    int Tb, Lb;
    long long off;
    const bool lens_ok = ct_entry<IT>(g, b, ilen, tlen, offsets, Tb, Lb, off);
    const float cost = costs[b];
    // the entry's state: NaN over its block (outside the tensors, or marked by the lattice launch), no finite cost, or live
    int bad = !lens_ok || cost != cost;
    const bool infinite = !bad && (cost == INFINITY || cost == ninf || Lb > g.S);
    const bool live_entry = !bad && !infinite;  // (the same in every thread)
    const IT* __restrict__ targets = targets_all + (lens_ok ? off : 0ll);

    // ---- the tables, once per workgroup
    if (live_entry) {
        for (int k = tid; k < Lb; k += blockDim.x) {
            const long long v = (long long)targets[k];
            const bool in = v >= 0 && v < C && v != blank;
            bad |= !in;
            labs[k] = in ? (int)v : 0;
        }
        for (int c = tid; c < C; c += blockDim.x) slot[c] = 0xffffu;
    }
    bad = __syncthreads_or(bad);
    const bool live = live_entry && !bad;
    if (live) {
        if (tid == 0) slot[blank] = 0, nslots_s = 0;
        for (int k = tid; k < Lb; k += blockDim.x) {                // rank by (label, index); a first occurrence has nothing equal before
            const int v = labs[k];
            int less = 0, before = 0;
            for (int i = 0; i < Lb; ++i) {
                const int u = labs[i];
                less += u < v;
                before += (u == v) & (i < k);
            }
            order[less + before] = (unsigned short)k;
            first[k] = before == 0;
        }
    }
    __syncthreads();
    if (live) {
        for (int k = tid; k < Lb; k += blockDim.x) {                // the slot: distinct labels below this one, plus one for the blank
            const int v = labs[k];
            int less = 0, below = 0, behind = 0;
            for (int i = 0; i < Lb; ++i) {
                const int u = labs[i];
                less += u < v;
                below += (u < v) & (int)first[i];
                behind += (u > v) | ((u == v) & (i > k));
            }
            if (first[k]) {
                slot[v] = (unsigned short)(below + 1);
                start[below] = (unsigned short)less;                // (a first occurrence is the first of its group)
            }
            if (behind == 0) {                                      // the greatest label's last occurrence closes the table
                start[below + 1] = (unsigned short)Lb;
                nslots_s = below + 1;
            }
        }
    }
    __syncthreads();
    const int nslots = live ? nslots_s : 0;
    const float go = live ? grad_costs[b] : 0.0f;

    // ---- the frames of the tile, a wave on each
    const int t_end = min(T, (tile + 1) * g.tile);
    for (int t = tile * g.tile + wave; t < t_end; t += CT_GRAD_WAVES) {
        float* __restrict__ dst = grad_all + t * g.gt + b * g.gn;
        if (!live || t >= Tb) {
            const bool nan_row = bad || (infinite && !g.zero_inf && lens_ok && t < Tb);
            ct_row<VEC, false>(nullptr, 0, dst, g.gc, C, lane, slot, corr, 0.0f, nan_row ? NAN : 0.0f);
            continue;
        }
        const long long cell = ((long long)b * T + t) * W;
        for (int s = lane; s < 2 * Lb + 1; s += 64) rowbuf[s] = alphas[cell + s] + betas[cell + s];
        ct_wave_sync();
        float m = ninf;                                             // the blank: states 0, 2, …, 2 Lb
        for (int k = lane; k <= Lb; k += 64) m = fmaxf(m, rowbuf[2 * k]);
        m = ct_wave_max(m);
        const float mm = m == ninf ? 0.0f : m;
        float sum = 0.0f;
        for (int k = lane; k <= Lb; k += 64) sum += __expf(rowbuf[2 * k] - mm);
        sum = ct_wave_sum(sum);
        if (lane == 0) corr[0] = (m + __logf(sum)) + cost;
        for (int j = lane; j < nslots; j += 64) {                   // a label's states, in the order of order[]
            const int p0 = start[j], p1 = start[j + 1];
            float lm = ninf;
            for (int p = p0; p < p1; ++p) lm = fmaxf(lm, rowbuf[2 * order[p] + 1]);
            const float lmm = lm == ninf ? 0.0f : lm;
            float ls = 0.0f;
            for (int p = p0; p < p1; ++p) ls += __expf(rowbuf[2 * order[p] + 1] - lmm);
            corr[1 + j] = (lm + __logf(ls)) + cost;
        }
        ct_wave_sync();
        ct_row<VEC, true>(lp_all + t * g.st + b * g.sn, g.sc, dst, g.gc, C, lane, slot, corr, go, 0.0f);
        ct_wave_sync();                                             // the next frame overwrites the row and the sums
    }
}

inline int ct_geometry(const float* log_probs, int64_t frames, int64_t batch, int64_t classes, int64_t stride_t, int64_t stride_n,
                       int64_t stride_c, int64_t max_targets, int64_t targets_total, int32_t blank, CtcGeom* g) {
    const int status = ct_shape_status(frames, batch, classes, max_targets);
    if (!log_probs || status == 1 || targets_total < 0) return TAC_E_INVALID;
    if (blank < 0 || blank >= classes) return TAC_E_INVALID;
    if (frames == 1) stride_t = 0;
    if (batch == 1) stride_n = 0;
    if (classes == 1) stride_c = 0;
    if ((frames > 1 && stride_t <= 0) || (batch > 1 && stride_n <= 0) || (classes > 1 && stride_c <= 0)) return TAC_E_INVALID;
    if (status == 2) return TAC_E_UNSUPPORTED;
    g->st = stride_t, g->sn = stride_n, g->sc = stride_c;
    g->gt = g->gn = g->gc = 0;
    g->total = targets_total;
    g->T = (int)frames, g->N = (int)batch, g->C = (int)classes, g->S = (int)max_targets;
    g->blank = blank;
    g->tile = 1;
    g->zero_inf = 0;
    return TAC_OK;
}

inline bool ct_vec(const float* p, long long st, long long sn, long long sc, int C) {
    return C % 4 == 0 && (sc == 1 || C == 1) && st % 4 == 0 && sn % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace tac

extern "C" {

int32_t tac_ctc_loss_max_targets(void) { return tac::CT_MAX_TARGETS; }

int32_t tac_ctc_loss_max_classes(void) { return tac::CT_MAX_CLASSES; }

int32_t tac_ctc_loss_group_steps(void) { return tac::CT_AHEAD; }

int32_t tac_ctc_loss_ring_steps(void) { return tac::CT_AHEAD * tac::CT_DEPTH; }

int tac_ctc_loss_f32(const float* log_probs, int64_t frames, int64_t batch, int64_t classes, int64_t stride_t, int64_t stride_n,
                     int64_t stride_c, const void* targets, int64_t max_targets, int64_t targets_total, int32_t index64,
                     const int64_t* target_offsets, const int32_t* input_lengths, const int32_t* target_lengths, int32_t blank,
                     float* alphas, float* betas, float* costs, void* stream) {
    using namespace tac;
    CtcGeom g;
    const int rc = ct_geometry(log_probs, frames, batch, classes, stride_t, stride_n, stride_c, max_targets, targets_total, blank, &g);
    if (rc != TAC_OK) return rc;
    if (!input_lengths || !target_lengths || !costs || (targets_total > 0 && !targets)) return TAC_E_INVALID;
    if ((alphas == nullptr) != (betas == nullptr)) return TAC_E_INVALID;
    if (!target_offsets && targets_total != batch * max_targets) return TAC_E_INVALID;
    const bool store = alphas != nullptr;
    const int waves = ct_waves(max_targets + 1);
    const int threads = 64 * waves;                                 // whole waves: lanes beyond the pairs own nothing
    const long long blocks = store ? 2 * batch : batch;
#define CT_LAUNCH(MANY, STORE, IT)                                                                                              \
    launch_kernel(ctc_lattice_kernel<MANY, STORE, IT>, blocks, threads, 0, (hipStream_t)stream, log_probs, g, (const IT*)targets, \
                  (const int*)input_lengths, (const int*)target_lengths, (const long long*)target_offsets, alphas, betas, costs)
#define CT_PICK(IT)                                                                                   \
    (store ? (waves > 1 ? CT_LAUNCH(true, true, IT) : CT_LAUNCH(false, true, IT))                     \
           : (waves > 1 ? CT_LAUNCH(true, false, IT) : CT_LAUNCH(false, false, IT)))
    return index64 ? CT_PICK(long long) : CT_PICK(int);
#undef CT_PICK
#undef CT_LAUNCH
}

int tac_ctc_loss_grad_f32(const float* log_probs, int64_t frames, int64_t batch, int64_t classes, int64_t stride_t, int64_t stride_n,
                          int64_t stride_c, const void* targets, int64_t max_targets, int64_t targets_total, int32_t index64,
                          const int64_t* target_offsets, const int32_t* input_lengths, const int32_t* target_lengths, int32_t blank,
                          int32_t zero_infinity, const float* alphas, const float* betas, const float* costs, const float* grad_costs,
                          float* grad, int64_t grad_stride_t, int64_t grad_stride_n, int64_t grad_stride_c, void* stream) {
    using namespace tac;
    CtcGeom g;
    const int rc = ct_geometry(log_probs, frames, batch, classes, stride_t, stride_n, stride_c, max_targets, targets_total, blank, &g);
    if (rc != TAC_OK) return rc;
    if (!input_lengths || !target_lengths || !alphas || !betas || !costs || !grad_costs || !grad) return TAC_E_INVALID;
    if (targets_total > 0 && !targets) return TAC_E_INVALID;
    if (!target_offsets && targets_total != batch * max_targets) return TAC_E_INVALID;
    if (frames == 1) grad_stride_t = 0;
    if (batch == 1) grad_stride_n = 0;
    if (classes == 1) grad_stride_c = 0;
    if ((frames > 1 && grad_stride_t <= 0) || (batch > 1 && grad_stride_n <= 0) || (classes > 1 && grad_stride_c <= 0))
        return TAC_E_INVALID;
    g.gt = grad_stride_t, g.gn = grad_stride_n, g.gc = grad_stride_c;
    g.zero_inf = zero_infinity ? 1 : 0;
    g.tile = ct_tile_frames(batch, frames, device_cu_count());
    const int64_t tiles = ct_tiles(frames, g.tile);
    if (batch * tiles > 0x7fffffff) return TAC_E_UNSUPPORTED;
    const CtcGradLds L = ct_grad_lds(max_targets, classes);
    const bool vec = ct_vec(log_probs, g.st, g.sn, g.sc, g.C) && ct_vec(grad, g.gt, g.gn, g.gc, g.C);
#define CT_LAUNCH(VEC, IT)                                                                                                     \
    launch_kernel(ctc_grad_kernel<VEC, IT>, batch * tiles, 64 * CT_GRAD_WAVES, (size_t)L.bytes, (hipStream_t)stream, log_probs, g, L, \
                  (const IT*)targets, (const int*)input_lengths, (const int*)target_lengths, (const long long*)target_offsets,   \
                  alphas, betas, costs, grad_costs, grad, (int)tiles)
    if (index64) return vec ? CT_LAUNCH(true, long long) : CT_LAUNCH(false, long long);
    return vec ? CT_LAUNCH(true, int) : CT_LAUNCH(false, int);
#undef CT_LAUNCH
}

}  // extern "C"
