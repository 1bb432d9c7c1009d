// ctc_decode.hip — CTC prefix beam search without a language model (functional.ctc_beam_search / CTCBeamDecoder): the k best
// classes of every frame in one launch, the beam of every entry in a second.  Write K for the beam size, nS = min(K + 1, C - 1).
//
//   per entry, over frames t < length:   frame t is SKIPPED when exp(lp[t][blank]) > threshold (evaluated in float64)
//   S_t: the nS non-blank classes with the largest lp[t][c], ties to the lower class, in that order
//   the beam: at most K distinct prefixes, each with (pb, pnb), tot = logaddexp(pb, pnb); it starts as the empty prefix (0, -inf)
//   a step: prefix p with last token l   stays:    pb' (+)= tot + lp[blank];   non-empty: pnb' (+)= pnb + lp[l]
//                                        extends:  for c in S_t, and for c with p + c in the beam: pnb'(p + c) (+)= base + lp[c],
//                                                  base = pb if c == l else tot            ((+) is logaddexp, in float64)
//   the K prefixes with the largest tot' remain; tot' = -inf is dropped.
//
// Launch 1, ctc_tables_kernel: frames are independent and the logits are read once.  Every element becomes a 64-bit key
// (float bits made monotone, ~class): an unsigned maximum is then the arg-max with the tie rule in it, and "the next best" is
// the largest key below the last winner.  A wave owns a frame up to 512 classes (no LDS, no barrier), a workgroup up to CB_WIDE,
// both with the row's keys in registers (16-byte loads where the row is contiguous and aligned, dwords at the tail and
// elsewhere); longer rows are read again in each of the nS rounds.  Per frame it writes K + 2 pairs: (lp[blank], flag) and the
// (lp, class) of S_t.  flag: 0 kept, 1 skipped, 2 the frame holds a NaN.  Frames t >= length are neither read nor written.
//
// Launch 2, ctc_beam_kernel: ONE wave per entry, lane j is beam slot j, slots in descending tot by construction.
//   Identity is exact.  A prefix is a node of a trie: node 0 is the empty prefix, a prefix created by the extension chosen in
//   round r of kept step s is node 1 + s K + r, and its (parent node, token) is row s of the entry's node table.  "p + c is in the
//   beam" is "a slot has parent == node(p) and last == c", found by comparing registers across lanes; such a slot receives p's
//   extension in its own stay entry, and p's rank of c in S_t is masked.  A prefix that left the beam and is created again gets
//   a new node: slots one token longer that descend from the old one are found by their (token before last, grandparent) and
//   re-parented, by walking both chains in the node table where the grandparents differ as well.
//   Selection is K rounds of a wave arg-max over the lanes' heads.  A lane's candidates are its stay entry, its unmasked
//   extensions in the order of S_t (descending), and apart from them the extension by its own last token (base pb).
//   THE TIE RULE: among equal tot' the lower parent slot wins, in a slot staying before extending, then the lower rank in S_t.
//   lp[t][last] is the one data-dependent load; it is issued first in the step and used after the identity loops.
//   At the end lanes h < nbest walk their chains: tokens[h][len - 1 .. 0], -1 behind, tot rounded once to float32.
// An entry with a length outside [0, T] or a NaN in a frame t < length gets NaN scores and length 0 (tokens -1).
#include <math.h>

#include "host_common.hpp"

namespace tac {

constexpr int CB_MAX_BEAM = 32;                 // a lane per slot, and the arg-max runs over 32 lanes
constexpr int CB_THREADS = 256;                 // launch 1's workgroup
constexpr int CB_WIDE = CB_THREADS * 24;        // longest row whose keys stay in registers (24 a thread: unmeasured choice)
constexpr int CB_AHEAD = 4;                     // frame-table rows in flight in launch 2 (unmeasured choice)

struct CtcGeom {
    long long sb, st, sc;                       // element strides of log_probs
    double thr;                                 // the blank-skip threshold
    int B, T, C, K, nS, R, blank, nbest;        // R = K + 2: pairs in a frame's row of the tables
};

__device__ __forceinline__ unsigned long long cb_key(float x, int c) {
    x += 0.0f;                                  // -0 orders as +0
    unsigned u = __float_as_uint(x);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned)~c;
}

__device__ __forceinline__ unsigned long long cb_wave_max(unsigned long long m) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    return m;
}

// TPF threads own a frame (a wave or the workgroup); NE keys a thread in registers, 0: the row is read in every round
template <int TPF, int NE>
__global__ void __launch_bounds__(CB_THREADS)
ctc_tables_kernel(const float* __restrict__ lp_all, CtcGeom g, const int* __restrict__ lengths, int2* __restrict__ tables) {
    __shared__ unsigned long long red[2][CB_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = TPF == 64 ? lane : tid;
    const long long f = TPF == 64 ? (long long)blockIdx.x * (CB_THREADS / 64) + wave : (long long)blockIdx.x;
    if (f >= (long long)g.B * g.T) return;                          // (the same in every thread of the frame, like those below)
    const int b = (int)(f / g.T), t = (int)(f - (long long)b * g.T);
    const int Tb = lengths ? lengths[b] : g.T;
    if (Tb < 0 || Tb > g.T || t >= Tb) return;
    const float* __restrict__ row = lp_all + b * g.sb + t * g.st;
    const int C = g.C, blank = g.blank, nS = g.nS;
    bool nan = false;
    auto key_at = [&](int c) {
        const float x = row[c * g.sc];
        nan |= x != x;
        return c == blank ? 0ull : cb_key(x, c);
    };
    unsigned long long keys[NE > 0 ? NE : 1];
    if constexpr (NE > 0) {
        if (g.sc == 1 && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
#pragma unroll
            for (int i = 0; i < NE / 4; ++i) {
                const int c0 = 4 * (i * TPF + l);
                if (c0 + 3 < C) {
                    const float4 v = *reinterpret_cast<const float4*>(row + c0);
                    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        nan |= x[j] != x[j];
                        keys[4 * i + j] = c0 + j == blank ? 0ull : cb_key(x[j], c0 + j);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) keys[4 * i + j] = c0 + j < C ? key_at(c0 + j) : 0ull;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int c = i * TPF + l;
                keys[i] = c < C ? key_at(c) : 0ull;
            }
        }
    }
    unsigned long long below = ~0ull, mine = 0;                     // every key is below ~0: a class is below 2^30
    for (int r = 0; r < nS; ++r) {
        unsigned long long m = 0;
        if constexpr (NE > 0) {
#pragma unroll
            for (int i = 0; i < NE; ++i) m = (keys[i] < below && keys[i] > m) ? keys[i] : m;
        } else {
            for (int c = l; c < C; c += TPF) {
                const unsigned long long k = key_at(c);
                m = (k < below && k > m) ? k : m;
            }
        }
        m = cb_wave_max(m);
        if constexpr (TPF > 64) {                                   // two alternating rows: one barrier a round
            if (lane == 0) red[r & 1][wave] = m;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < CB_THREADS / 64; ++w) m = red[r & 1][w] > m ? red[r & 1][w] : m;
        }
        below = m;
        if (l == r) mine = m;
    }
    int any;
    if constexpr (TPF > 64)
        any = __syncthreads_or(nan);
    else
        any = __builtin_amdgcn_ballot_w64(nan) != 0;
    int2* __restrict__ out = tables + f * g.R;
    if (l < nS) {
        const unsigned u = (unsigned)(mine >> 32);
        out[1 + l] = make_int2((int)((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u), (int)~(unsigned)mine);
    }
    if (l == 63) {
        const float lpb = row[blank * g.sc];
        out[0] = make_int2(__float_as_int(lpb), any ? 2 : (exp((double)lpb) > g.thr ? 1 : 0));
    }
}

__device__ __forceinline__ double cb_lae(double a, double b) {
    const double m = fmax(a, b), n = fmin(a, b);
    return m == -INFINITY ? m : m + log1p(exp(n - m));
}

__device__ __forceinline__ int cb_lane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }   // src: the same in every lane

__device__ __forceinline__ double cb_lane(double v, int src) {
    return __hiloint2double(cb_lane(__double2hiint(v), src), cb_lane(__double2loint(v), src));
}

// a node's (parent, token), past the vector cache: other lanes of this wave stored it
__device__ __forceinline__ int2 cb_node(const int2* nodes, int id) {
    const unsigned long long v =
        __hip_atomic_load(reinterpret_cast<const unsigned long long*>(nodes + (id - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_int2((int)(unsigned)v, (int)(unsigned)(v >> 32));
}

__global__ void __launch_bounds__(64)
ctc_beam_kernel(const float* __restrict__ lp_all, CtcGeom g, const int* __restrict__ lengths, const int2* __restrict__ tables_all,
                int2* nodes_all, int* __restrict__ tokens_all, int* __restrict__ tlens_all, float* __restrict__ scores_all) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = g.T, K = g.K, nS = g.nS, R = g.R, nbest = g.nbest;
    const int Tb = lengths ? lengths[b] : T;
    const float* __restrict__ lp = lp_all + b * g.sb;
    const int2* __restrict__ tab = tables_all + (long long)b * T * R;
    int2* nodes = nodes_all + (long long)b * T * K;
    int* __restrict__ tokens = tokens_all + (long long)b * nbest * T;
    const double ninf = -INFINITY;
    bool bad = Tb < 0 || Tb > T;
    const int nT = bad ? 0 : Tb;

    // slot state; a dead slot holds -inf and ids no live slot refers to
    double pb = lane == 0 ? 0.0 : ninf, pnb = ninf;
    int last = -1, node = lane == 0 ? 0 : -2, parent = lane == 0 ? -1 : -3, gparent = -4, ptok = -1, len = 0;

    auto load_row = [&](int t) {
        int2 z = make_int2(0, 0);
        if (lane <= nS && nT > 0) z = tab[(long long)min(t, nT - 1) * R + lane];
        return z;
    };
    static_assert(CB_AHEAD == 4, "the ring below is written out");
    int2 r0 = load_row(0), r1 = load_row(1), r2 = load_row(2), r3 = load_row(3);
    int s = 0;                                                      // kept frames so far
#pragma unroll 1
    for (int t = 0; t < nT; ++t) {
        const int2 row = r0;
        r0 = r1, r1 = r2, r2 = r3;
        const int flag = __builtin_amdgcn_readfirstlane(row.y);
        if (flag == 1) {
            r3 = load_row(t + CB_AHEAD);
            continue;
        }
        if (flag == 2) {
            bad = true;
            break;
        }
        float elast = 0.0f;
        if (last >= 0) elast = lp[t * g.st + last * g.sc];
        r3 = load_row(t + CB_AHEAD);
        const float lpS = __int_as_float(row.x);                    // lane 1 + r: S_t's rank r
        const int clsS = row.y;
        const double lpb = (double)__int_as_float(__builtin_amdgcn_readfirstlane(row.x));
        const double tot = cb_lae(pb, pnb);

        // ---- identity: the rank of the own last token in S_t, the parent's slot, the ranks children own
        int rank = -1;
        for (int r = 0; r < nS; ++r) rank = cb_lane(clsS, r + 1) == last ? r : rank;
        int pslot = -1;
        unsigned long long owned = 0;
        for (int i = 0; i < K; ++i) {
            const int ni = cb_lane(node, i), pi = cb_lane(parent, i), ri = cb_lane(rank, i);
            pslot = parent == ni ? i : pslot;
            if (pi == node && ri >= 0) owned |= 1ull << ri;
        }

        // ---- the stay entry, with the parent's extension by the own last token
        const double el = (double)elast;
        const double spb = tot + lpb;
        double spnb = last >= 0 ? pnb + el : ninf;
        const int src = pslot >= 0 ? pslot : lane;
        const double ppb = __shfl(pb, src), ptot = __shfl(tot, src);
        const int plast = __shfl(last, src);
        if (pslot >= 0) spnb = cb_lae(spnb, (plast == last ? ppb : ptot) + el);
        const double stot = cb_lae(spb, spnb);

        // ---- the extensions: S_t's ranks no child owns, the own last token's apart (base pb)
        unsigned long long avail = ((1ull << nS) - 1) & ~owned;
        const float lrank = __shfl(lpS, rank >= 0 ? rank + 1 : 0);
        double hs = ninf;
        if (rank >= 0) {
            if ((avail >> rank) & 1) hs = pb + (double)lrank;
            avail &= ~(1ull << rank);
        }
        bool stay_open = true, spec_open = hs > ninf;

        double npb = ninf, npnb = ninf;
        int nlast = -1, nnode = -2, nparent = -3, ngp = -4, nptok = -1, nlen = 0, nsel = 0;
        for (int r = 0; r < K; ++r) {
            const int rn = avail ? __builtin_ctzll(avail) : 62;
            const float ln = __shfl(lpS, rn + 1);
            const double hn = avail ? tot + (double)ln : ninf;
            double v = stay_open ? stot : ninf;
            int ord = stay_open ? -1 : 99;                          // -1 the stay entry, else the rank
            if (hn > v || (hn == v && rn < ord)) v = hn, ord = rn;
            if (spec_open && (hs > v || (hs == v && rank < ord))) v = hs, ord = rank;
            double m = v;
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
            m = cb_lane(m, 0);                                      // lanes 32 .. 63 are dead slots
            if (m == ninf) break;
            const unsigned long long won = __builtin_amdgcn_ballot_w64(v == m) & 0xffffffffull;
            const int w = __builtin_amdgcn_readfirstlane(__builtin_ctzll(won));
            const int ow = cb_lane(ord, w);
            const int cls = cb_lane(clsS, ow >= 0 ? ow + 1 : 0);
            const double wspb = cb_lane(spb, w), wspnb = cb_lane(spnb, w);
            const int wlast = cb_lane(last, w), wnode = cb_lane(node, w), wparent = cb_lane(parent, w);
            const int wgp = cb_lane(gparent, w), wptok = cb_lane(ptok, w), wlen = cb_lane(len, w);
            if (lane == r) {
                if (ow >= 0) {
                    npb = ninf, npnb = m, nlast = cls, nnode = 1 + s * K + r, nparent = wnode, ngp = wparent, nptok = wlast;
                    nlen = wlen + 1;
                    nodes[(long long)s * K + r] = make_int2(wnode, cls);
                } else {
                    npb = wspb, npnb = wspnb, nlast = wlast, nnode = wnode, nparent = wparent, ngp = wgp, nptok = wptok, nlen = wlen;
                }
            }
            if (lane == w) {
                if (ow < 0)
                    stay_open = false;
                else if (ow == rank)
                    spec_open = false;
                else
                    avail &= avail - 1;
            }
            ++nsel;
        }
        pb = npb, pnb = npnb, last = nlast, node = nnode, parent = nparent, gparent = ngp, ptok = nptok, len = nlen;

        // ---- a prefix created again: slots one token longer that descend from its earlier node take the new one as parent
        const int first_new = 1 + s * K;
        for (int r = 0; r < nsel; ++r) {
            const int xn = cb_lane(node, r);
            if (xn < first_new) continue;
            const int xp = cb_lane(parent, r), xc = cb_lane(last, r), xl = cb_lane(len, r);
            if (len == xl + 1 && ptok == xc && parent != xn && node < first_new) {
                bool same = gparent == xp;
                if (!same) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    int a = gparent, c = xp;
                    same = true;
                    while (a != c) {
                        if (a <= 0 || c <= 0) {
                            same = false;
                            break;
                        }
                        const int2 ra = cb_node(nodes, a), rc = cb_node(nodes, c);
                        if (ra.y != rc.y) {
                            same = false;
                            break;
                        }
                        a = ra.x, c = rc.x;
                    }
                }
                if (same) parent = xn, gparent = xp;
            }
        }
        ++s;
    }

    // ---- results: -1 behind every hypothesis, then lanes h < nbest walk their chains
    for (int h = 0; h < nbest; ++h) {
        const int lh = bad ? 0 : cb_lane(len, h);
        for (int i = lh + lane; i < T; i += 64) tokens[(long long)h * T + i] = -1;
    }
    if (lane < nbest) {
        tlens_all[(long long)b * nbest + lane] = bad ? 0 : len;
        scores_all[(long long)b * nbest + lane] = bad ? NAN : (float)cb_lae(pb, pnb);
    }
    if (bad) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane < nbest) {
        int n = node;
        for (int i = len - 1; i >= 0; --i) {
            const int2 rec = cb_node(nodes, n);
            tokens[(long long)lane * T + i] = rec.y;
            n = rec.x;
        }
    }
}

inline bool cb_sizes_ok(int64_t batch, int64_t frames, int64_t beam) {
    return batch >= 1 && frames >= 1 && beam >= 1 && beam <= CB_MAX_BEAM && batch <= 0x7fffffff && frames < (1ll << 30) &&
           batch * frames <= 0x7fffffff && frames * beam < 0x7fffffff;
}

}  // namespace tac

extern "C" {

int32_t tac_ctc_beam_max_beam(void) { return tac::CB_MAX_BEAM; }

int32_t tac_ctc_beam_wide_classes(void) { return tac::CB_WIDE; }

int64_t tac_ctc_beam_workspace(int64_t batch, int64_t frames, int64_t beam) {
    if (!tac::cb_sizes_ok(batch, frames, beam)) return -1;
    return batch * frames * (2 * beam + 2) * 8;
}

int tac_ctc_beam_search_f32(const float* log_probs, int64_t batch, int64_t frames, int64_t classes, int64_t stride_b,
                            int64_t stride_t, int64_t stride_c, const int32_t* lengths, int32_t beam, int32_t nbest, int32_t blank,
                            double blank_skip_threshold, void* workspace, int32_t* tokens, int32_t* token_lengths, float* scores,
                            void* stream) {
    using namespace tac;
    if (!log_probs || batch <= 0 || frames <= 0 || classes < 2 || !workspace || !tokens || !token_lengths || !scores)
        return TAC_E_INVALID;
    if (blank < 0 || blank >= classes || beam < 1 || nbest < 1 || nbest > beam) return TAC_E_INVALID;
    if (batch == 1) stride_b = 0;
    if (frames == 1) stride_t = 0;
    if ((batch > 1 && stride_b <= 0) || (frames > 1 && stride_t <= 0) || stride_c <= 0) return TAC_E_INVALID;
    if (!cb_sizes_ok(batch, frames, beam) || classes >= (1ll << 30)) return TAC_E_UNSUPPORTED;
    CtcGeom g;
    g.sb = stride_b, g.st = stride_t, g.sc = stride_c;
    g.thr = blank_skip_threshold;
    g.B = (int)batch, g.T = (int)frames, g.C = (int)classes, g.K = beam, g.blank = blank, g.nbest = nbest;
    g.nS = (int)(beam + 1 < classes - 1 ? beam + 1 : classes - 1);
    g.R = beam + 2;
    int2* tables = (int2*)workspace;
    int2* nodes = tables + batch * frames * g.R;
    const long long F = batch * frames;
    hipStream_t st = (hipStream_t)stream;
    int rc;
#define CB_TABLES(TPF, NE)                                                                                               \
    launch_kernel(ctc_tables_kernel<TPF, NE>, TPF == 64 ? (F + CB_THREADS / 64 - 1) / (CB_THREADS / 64) : F, CB_THREADS, 0, st, \
                  log_probs, g, (const int*)lengths, tables)
    if (classes <= 64 * 4)
        rc = CB_TABLES(64, 4);
    else if (classes <= 64 * 8)
        rc = CB_TABLES(64, 8);
    else if (classes <= CB_THREADS * 8)
        rc = CB_TABLES(CB_THREADS, 8);
    else if (classes <= CB_THREADS * 16)
        rc = CB_TABLES(CB_THREADS, 16);
    else if (classes <= CB_WIDE)
        rc = CB_TABLES(CB_THREADS, 24);
    else
        rc = CB_TABLES(CB_THREADS, 0);
#undef CB_TABLES
    if (rc != TAC_OK) return rc;
    return launch_kernel(ctc_beam_kernel, batch, 64, 0, st, log_probs, g, (const int*)lengths, (const int2*)tables, nodes, (int*)tokens,
                         (int*)token_lengths, scores);
}

}  // extern "C"
