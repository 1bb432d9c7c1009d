// ctc_loss_plan.hpp — the host-side plan of csrc/ctc_loss.hip: limits, workgroup sizes, the tiling of the frames and the LDS layout
// of the gradient launch.  Plain C++ without a HIP type, so that a host program can include it and walk it on its own.
#pragma once
#include <stdint.h>

namespace tac {

constexpr int CT_MAX_TARGETS = 1024;            // the most S + 1: a lane per pair of states in one workgroup
constexpr int CT_MAX_CLASSES = 32768;           // the most C: the 16-bit class-to-slot table of the gradient launch is 2 C bytes of LDS
constexpr int CT_AHEAD = 8;                     // steps of the lattice in a group: their emissions are loaded together,
constexpr int CT_DEPTH = 4;                     // this many groups ahead of their use
constexpr int CT_GRAD_WAVES = 4;                // waves of a gradient workgroup, each on a frame of its own
constexpr int CT_GRAD_BATCH = 4;                // 16-byte chunks of a class row a lane has in flight
constexpr int CT_MIN_TILE = 16;                 // the fewest frames of a tile: the tables are built once per workgroup
constexpr int CT_LDS_LIMIT = 160 * 1024;

inline int ct_waves(int64_t targets1) { return (int)((targets1 + 63) / 64); }

// the LDS of a gradient workgroup, in bytes from its start (every part 8-byte aligned)
struct CtcGradLds {
    int row;                                    // float [waves][row_len]: alpha + beta of a frame
    int corr;                                   // float [waves][corr_len]: log-sum per slot (0: the blank) plus the entry's cost
    int labs;                                   // int32 [S]: the entry's labels
    int order;                                  // uint16 [S]: label indices sorted by (label, index)
    int start;                                  // uint16 [S + 1]: where a slot's group starts in order[]
    int first;                                  // uint16 [S]: 1 where a label occurs for the first time
    int slot;                                   // uint16 [C]: class -> slot, 0xffff for none
    int row_len, corr_len;
    int bytes;
};

inline int ct_align8(int64_t v) { return (int)((v + 7) & ~(int64_t)7); }

inline CtcGradLds ct_grad_lds(int64_t max_targets, int64_t classes) {
    CtcGradLds l;
    const int S = (int)max_targets;
    l.row_len = 2 * S + 2;                      // 2 S + 1 states, rounded to an even count
    l.corr_len = S + 2;                         // the blank and up to S distinct labels, rounded likewise
    if (l.corr_len & 1) ++l.corr_len;
    int at = 0;
    l.row = at, at += ct_align8((int64_t)CT_GRAD_WAVES * l.row_len * 4);
    l.corr = at, at += ct_align8((int64_t)CT_GRAD_WAVES * l.corr_len * 4);
    l.labs = at, at += ct_align8((int64_t)S * 4);
    l.order = at, at += ct_align8((int64_t)S * 2);
    l.start = at, at += ct_align8((int64_t)(S + 1) * 2);
    l.first = at, at += ct_align8((int64_t)S * 2);
    l.slot = at, at += ct_align8(classes * 2);
    l.bytes = at;
    return l;
}

// frames of a tile of the gradient launch: about eight workgroups per compute unit, never fewer than CT_MIN_TILE frames each
inline int ct_tile_frames(int64_t batch, int64_t frames, int64_t compute_units) {
    const int64_t want = compute_units * 8 > 0 ? compute_units * 8 : 1;
    int64_t per = (batch * frames + want - 1) / want;
    if (per < CT_MIN_TILE) per = CT_MIN_TILE;
    if (per > frames) per = frames;
    return (int)(per < 1 ? 1 : per);
}

inline int64_t ct_tiles(int64_t frames, int tile) { return (frames + tile - 1) / tile; }

// what both launches refuse: 0 fine, 1 invalid, 2 outside the kernels' limits
inline int ct_shape_status(int64_t frames, int64_t batch, int64_t classes, int64_t max_targets) {
    if (frames <= 0 || batch <= 0 || classes <= 0 || max_targets < 0) return 1;
    if (max_targets + 1 > CT_MAX_TARGETS || classes > CT_MAX_CLASSES) return 2;
    if (frames > 0x3fffffff || batch > 0x3fffffff) return 2;
    if (ct_grad_lds(max_targets, classes).bytes > CT_LDS_LIMIT) return 2;
    return 0;
}

}  // namespace tac
