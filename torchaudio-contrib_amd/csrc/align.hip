// align.hip — CTC forced alignment (functional.forced_align; torchaudio's semantics without its state window): the Viterbi
// recursion over (B, T, C) log-probabilities, the backtrack and both outputs in ONE launch, a workgroup per batch entry.
//
//   states s = 0 .. 2 Lb: even ones carry the blank, s = 2k + 1 carries targets[k]
//   alpha[0][0] = lp[0][blank], alpha[0][1] = lp[0][targets[0]], -inf elsewhere
//   alpha[t][s] = (the first of x2, x1, x0 that is STRICTLY greater than both others, else x0) + lp[t][label(s)]
//       x0 = alpha[t-1][s], x1 = alpha[t-1][s-1], x2 = alpha[t-1][s-2] for odd s >= 3 whose label differs from the one before
//   end state 2 Lb if alpha[Tb-1][2 Lb] > alpha[Tb-1][2 Lb - 1], else 2 Lb - 1; back-pointers are followed down to t = 0
//
// Lanes.  Lane q owns the PAIR (2q, 2q + 1) — the blank before label q, and label q.  The one value a step needs from another
// lane is label q - 1's alpha (x1 of the blank, x2 of the label): a one-lane wave shift.  Up to 64 pairs one wave runs the time
// loop without a barrier; above, waves hand their last lane's value over through two alternating LDS rows, one barrier a step.
// (A lane with 2 or 4 consecutive pairs, one wave up to 256 pairs, was built first and measured slower from 65 pairs on: the
// pairs of a lane are worked one after the other, the waves of a workgroup side by side.  DESIGN 3.24.)  Selection is by ordered
// compares, never by a maximum: a NaN goes where the compares send it.
// Emissions.  lp[t][blank] and lp[t][targets[q]] do not depend on the recursion: they are loaded AL_AHEAD steps at a time,
// AL_DEPTH groups ahead of their use, at clamped indices.
// Back-pointers.  Three wave ballots per step (blank took x1; label took x1; label took x2): 24 bytes per wave and step, stored by
// the wave's first three lanes.  They stay in the LDS while the entry's Tb - 1 rows fit (AL_BP_WORDS); else they go to the
// entry's part of a global workspace and come back in chunks of whole rows, coalesced, before one lane walks a chunk.  The walked
// states are staged in the LDS and every lane then stores paths and gathers scores for the chunk.
// An entry with Tb outside [1, T], Lb outside [0, L], a used target that is the blank or outside [0, C), or Tb < Lb + repeats
// gets paths -1 and scores NaN on all T frames; no address is formed from such a value.  Frames t >= Tb: blank and 0.
#include <math.h>

#include "host_common.hpp"

namespace tac {

constexpr int AL_MAX_TARGETS = 1024;            // the most L + 1: a lane per pair of states in one workgroup
constexpr int AL_AHEAD = 8;                     // steps in a group: their emissions are loaded together,
constexpr int AL_DEPTH = 4;                     // this many groups ahead of their use
constexpr int AL_BP_WORDS = 6144;               // 64-bit back-pointer words in the LDS (48 KB)
constexpr int AL_STAGE = 2048;                  // the most rows of a chunk: states staged for the output pass (8 KB)

struct AlignGeom {
    long long sb, st, sc;                       // element strides of log_probs
    int B, T, L, C;
    int blank;
    int W;                                      // back-pointer words of a row (a step): 3 per wave
    int CH;                                     // rows of a chunk: min(AL_STAGE, AL_BP_WORDS / W)
};

// lane i receives lane i - 1's value (lane 0: unspecified, replaced by the caller)
__device__ __forceinline__ float al_from_lower_lane(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

template <bool MANY, typename IT>               // more than one wave: the boundary value goes through the LDS, a barrier a step
__global__ void __launch_bounds__(MANY ? AL_MAX_TARGETS : 64)
align_kernel(const float* __restrict__ lp_all, AlignGeom g, const IT* __restrict__ targets_all, const int* __restrict__ ilen,
             const int* __restrict__ tlen, unsigned long long* __restrict__ ws_all, IT* __restrict__ paths_all,
             float* __restrict__ scores_all) {
    __shared__ unsigned long long bpw[AL_BP_WORDS];
    __shared__ int stage[AL_STAGE];
    __shared__ float edge[2][AL_MAX_TARGETS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = g.T, L = g.L, C = g.C, blank = g.blank, W = g.W, CH = g.CH;
    const int Tb = ilen ? ilen[b] : T, Lb = tlen ? tlen[b] : L;
    const float* __restrict__ lp = lp_all + b * g.sb;
    const IT* __restrict__ targets = targets_all + (long long)b * L;
    IT* __restrict__ paths = paths_all + (long long)b * T;
    float* __restrict__ scores = scores_all + (long long)b * T;
    const float ninf = -INFINITY;

    // ---- the entry's lengths and targets: range, blank, repeats (thread q looks at targets[q] and the one before)
    const bool lens_ok = Tb >= 1 && Tb <= T && Lb >= 0 && Lb <= L;
    int bad = !lens_ok, lab = blank, rep = 0;
    bool skip = false;                                              // the label state may take x2
    if (lens_ok && tid < Lb) {
        const long long v = (long long)targets[tid];
        const bool in = v >= 0 && v < C && v != blank;
        bad |= !in;
        lab = in ? (int)v : blank;
        if (tid >= 1) {
            const bool same = (long long)targets[tid - 1] == v;
            rep = same, skip = !same;
        }
    }
    const int repeats = __syncthreads_count(rep);
    bad = __syncthreads_or(bad);
    if (bad || Tb < Lb + repeats) {
        for (int t = tid; t < T; t += blockDim.x) paths[t] = (IT)-1, scores[t] = NAN;
        return;
    }
    for (int t = Tb + tid; t < T; t += blockDim.x) paths[t] = (IT)blank, scores[t] = 0.0f;

    // ---- the recursion: row d of the back-pointers leads from frame d to frame d + 1
    // the blank's column through a lane register the compiler cannot see through: its emission is then a vector load like the
    // label's, counted with it — a scalar load's counter only knows "all returned", and every step would wait for the group of
    // loads just issued
    int vblank = blank;
    asm volatile("" : "+v"(vblank));
    const long long offb = vblank * g.sc, offl = lab * g.sc;
    float ab = ninf, al = ninf;                                     // the alphas of the blank and of the label state
    if (tid == 0) {
        ab = lp[offb];
        if (Lb >= 1) al = lp[offl];
    }
    const int nsteps = Tb - 1;
    const bool spill = nsteps > CH;                                 // (the same in every thread)
    unsigned long long* __restrict__ gw = ws_all + (spill ? (long long)b * (T - 1) * W : 0ll);
    auto fetch = [&](int d, float& eb, float& el) {                 // the emissions of step d, i.e. of frame d + 1
        const float* row = lp + (long long)min(d + 1, Tb - 1) * g.st;
        eb = row[offb];
        el = row[offl];
    };
    float EB[AL_DEPTH][AL_AHEAD], EL[AL_DEPTH][AL_AHEAD];           // a ring of groups of steps, every index static
#pragma unroll
    for (int s = 0; s < AL_DEPTH; ++s)
#pragma unroll
        for (int k = 0; k < AL_AHEAD; ++k) fetch(s * AL_AHEAD + k, EB[s][k], EL[s][k]);
#pragma unroll 1
    for (int d0 = 0; d0 < nsteps; d0 += AL_DEPTH * AL_AHEAD) {
#pragma unroll
        for (int s = 0; s < AL_DEPTH; ++s) {
            const int ds = d0 + s * AL_AHEAD;
            if (ds >= nsteps) break;                                // (the same in every thread)
            float eb[AL_AHEAD], el[AL_AHEAD];
#pragma unroll
            for (int k = 0; k < AL_AHEAD; ++k) eb[k] = EB[s][k], el[k] = EL[s][k];
#pragma unroll
            for (int k = 0; k < AL_AHEAD; ++k) fetch(ds + AL_DEPTH * AL_AHEAD + k, EB[s][k], EL[s][k]);
#pragma unroll
            for (int k = 0; k < AL_AHEAD; ++k) {
                const int d = ds + k;
                if (d >= nsteps) break;                             // (the same in every thread)
                float prev = al_from_lower_lane(al);                // label q - 1
                if constexpr (MANY) {
                    if (lane == 63) edge[d & 1][wave] = al;
                    __syncthreads();
                    if (lane == 0 && wave > 0) prev = edge[d & 1][wave - 1];
                }
                if (tid == 0) prev = ninf;
                const float x2 = skip ? prev : ninf;                // the label state: x0 = al, x1 = ab, x2 = label q - 1
                const bool pa = prev > ab, pn = prev > ninf;        // the blank state: x0 = ab, x1 = label q - 1, no x2
                const bool ta = x2 > ab, tl2 = x2 > al, ba = ab > al, bt = ab > x2;
                const bool b1 = pa && pn, c2 = ta && tl2, c1 = !c2 && ba && bt;
                // the wave's masks from the compares themselves (a compare writes its mask anyway), combined as scalars
                const unsigned long long m0 = __builtin_amdgcn_ballot_w64(pa) & __builtin_amdgcn_ballot_w64(pn);
                const unsigned long long m2 = __builtin_amdgcn_ballot_w64(ta) & __builtin_amdgcn_ballot_w64(tl2);
                const unsigned long long m1 = ~m2 & __builtin_amdgcn_ballot_w64(ba) & __builtin_amdgcn_ballot_w64(bt);
                al = (c2 ? x2 : (c1 ? ab : al)) + el[k];
                ab = (b1 ? prev : ab) + eb[k];
                if (lane < 3) {
                    const unsigned long long w = lane == 0 ? m0 : (lane == 1 ? m1 : m2);
                    if (spill)
                        gw[(long long)d * W + wave * 3 + lane] = w;
                    else
                        bpw[d * W + wave * 3 + lane] = w;
                }
            }
        }
    }

    // ---- the end state, from the last alphas of every pair
    __syncthreads();
    float* fin = reinterpret_cast<float*>(stage);                   // 2 blockDim <= AL_STAGE floats
    fin[2 * tid] = ab, fin[2 * tid + 1] = al;
    __syncthreads();
    int s = 0;                                                      // (thread 0's: the state at the frame being walked)
    if (tid == 0 && Lb >= 1) s = fin[2 * Lb] > fin[2 * Lb - 1] ? 2 * Lb : 2 * Lb - 1;
    __syncthreads();

    // ---- the backtrack, a chunk of rows at a time from the last
    for (int c = (nsteps + CH - 1) / CH - 1; c >= 0; --c) {
        const int r0 = c * CH, n = min(CH, nsteps - r0);
        if (spill) {
            const unsigned long long* __restrict__ src = gw + (long long)r0 * W;
            for (int i = tid; i < n * W; i += blockDim.x) bpw[i] = src[i];
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = n - 1; i >= 0; --i) {
                stage[i] = s;                                       // the state at frame r0 + i + 1
                const int q = s >> 1, word = i * W + (q >> 6) * 3, ln = q & 63;
                const unsigned long long m0 = bpw[word], m1 = bpw[word + 1], m2 = bpw[word + 2];
                s -= (s & 1) ? (int)((m1 >> ln) & 1) + 2 * (int)((m2 >> ln) & 1) : (int)((m0 >> ln) & 1);
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += blockDim.x) {
            const int t = r0 + i + 1, si = stage[i];
            const IT label = (si & 1) ? targets[si >> 1] : (IT)blank;
            paths[t] = label;
            scores[t] = lp[t * g.st + (long long)label * g.sc];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const IT label = (s & 1) ? targets[s >> 1] : (IT)blank;
        paths[0] = label;
        scores[0] = lp[(long long)label * g.sc];
    }
}

inline int al_waves(int64_t targets1) { return (int)((targets1 + 63) / 64); }

inline int al_chunk(int W) { return AL_BP_WORDS / W < AL_STAGE ? AL_BP_WORDS / W : AL_STAGE; }

}  // namespace tac

extern "C" {

int32_t tac_forced_align_max_targets(void) { return tac::AL_MAX_TARGETS; }

int64_t tac_forced_align_workspace(int64_t batch, int64_t frames, int64_t targets1) {
    using namespace tac;
    if (batch < 0 || frames < 1 || targets1 < 1 || targets1 > AL_MAX_TARGETS) return -1;
    const int W = 3 * al_waves(targets1);
    return frames - 1 > al_chunk(W) ? batch * (frames - 1) * W * 8 : 0;
}

int tac_forced_align_f32(const float* log_probs, int64_t batch, int64_t frames, int64_t classes, int64_t stride_b,
                         int64_t stride_t, int64_t stride_c, const void* targets, int64_t max_targets, int32_t index64,
                         const int32_t* input_lengths, const int32_t* target_lengths, int32_t blank, void* workspace, void* paths,
                         float* scores, void* stream) {
    using namespace tac;
    if (!log_probs || batch <= 0 || frames <= 0 || classes <= 0 || max_targets < 0 || !paths || !scores) return TAC_E_INVALID;
    if (blank < 0 || blank >= classes || (max_targets > 0 && !targets)) return TAC_E_INVALID;
    if (batch == 1) stride_b = 0;
    if (frames == 1) stride_t = 0;
    if (classes == 1) stride_c = 0;
    if ((batch > 1 && stride_b <= 0) || (frames > 1 && stride_t <= 0) || (classes > 1 && stride_c <= 0)) return TAC_E_INVALID;
    if (max_targets + 1 > AL_MAX_TARGETS) return TAC_E_UNSUPPORTED;
    if (batch > 0x7fffffff || frames > 0x3fffffff || classes > 0x3fffffff) return TAC_E_UNSUPPORTED;
    const int waves = al_waves(max_targets + 1);
    AlignGeom g;
    g.sb = stride_b, g.st = stride_t, g.sc = stride_c;
    g.B = (int)batch, g.T = (int)frames, g.L = (int)max_targets, g.C = (int)classes;
    g.blank = blank;
    g.W = 3 * waves;
    g.CH = al_chunk(g.W);
    if (frames - 1 > g.CH && !workspace) return TAC_E_INVALID;
    const int threads = 64 * waves;                                 // whole waves: lanes beyond the pairs hold states no path visits
#define AL_LAUNCH(MANY, IT)                                                                                                \
    launch_kernel(align_kernel<MANY, IT>, batch, threads, 0, (hipStream_t)stream, log_probs, g, (const IT*)targets,          \
                  (const int*)input_lengths, (const int*)target_lengths, (unsigned long long*)workspace, (IT*)paths, scores)
    if (index64) return waves > 1 ? AL_LAUNCH(true, long long) : AL_LAUNCH(false, long long);
    return waves > 1 ? AL_LAUNCH(true, int) : AL_LAUNCH(false, int);
#undef AL_LAUNCH
}

}  // extern "C"
