// soft_dtw_plan.hpp — the host-side plan of csrc/soft_dtw.hip: limits, rows per lane and workgroup size of the lattice launch, the
// tile counts of the cost, gradient and alignment launches, the LDS of each and the size of the skewed arrays.  Plain C++ without a
// HIP type, so that a host program can include it and walk it on its own.
#pragma once
#include <stdint.h>

namespace tac {

constexpr int SD_MAX_LEN = 4096;                // the most N or M: SD_LANES lanes of SD_MAX_ROWS rows in ONE workgroup, so no strips
constexpr int SD_MAX_DIM = 256;                 // the most D: eight 32-column MFMA blocks, two for each wave of a gradient workgroup
constexpr int SD_LANES = 1024;                  // lanes of the largest lattice workgroup
constexpr int SD_MAX_ROWS = 4;                  // the most rows of the lattice a lane owns
constexpr int SD_RING = 8;                      // steps the lattice launch loads its costs ahead of their use
constexpr int SD_TILE = 32;                     // rows and columns of a gradient / alignment tile; positions and diagonals of a cost tile
constexpr int SD_COST_DC = 32;                  // features of x and y a cost workgroup stages at a time
constexpr int SD_WAVES = 4;                     // waves of a cost, gradient or alignment workgroup
constexpr int SD_E_STRIDE = 34;                 // floats between the rows of the E tile in the LDS (conflict-free skewed deposits)
constexpr int SD_LDS_LIMIT = 64 * 1024;

// rows of the lattice a lane owns: 1, 2 or 4 (a power of two keeps every loop over them unrolled), the least that fits the rows
inline int sd_rows_per_lane(int64_t rows) { return rows <= SD_LANES ? 1 : (rows <= 2 * SD_LANES ? 2 : SD_MAX_ROWS); }

// lanes of the lattice workgroup: whole waves over the row blocks
inline int sd_threads(int64_t rows) {
    const int r = sd_rows_per_lane(rows);
    const int64_t lanes = (rows + r - 1) / r;
    return (int)((lanes + 63) / 64 * 64);
}

inline int64_t sd_diagonals(int64_t n, int64_t m) { return n + m - 1; }

// elements of one skewed array (cost, R or Q): row k = i + j of N positions, position i
inline int64_t sd_skewed_elems(int64_t batch, int64_t n, int64_t m) { return batch * sd_diagonals(n, m) * n; }

inline int64_t sd_tiles(int64_t len) { return (len + SD_TILE - 1) / SD_TILE; }

inline int64_t sd_cost_blocks(int64_t batch, int64_t n, int64_t m) { return batch * sd_tiles(sd_diagonals(n, m)) * sd_tiles(n); }
inline int64_t sd_grad_blocks(int64_t batch, int64_t n, int64_t m) { return batch * (sd_tiles(n) + sd_tiles(m)); }
inline int64_t sd_align_blocks(int64_t batch, int64_t n, int64_t m) { return batch * sd_tiles(n) * sd_tiles(m); }

inline int sd_cost_lds_bytes() { return 4 * (SD_TILE + 2 * SD_TILE - 1) * (SD_COST_DC + 1); }     // x rows and y rows, padded by one
inline int sd_grad_lds_bytes() { return 4 * (SD_TILE * SD_E_STRIDE + SD_TILE); }                  // the E tile and its row sums
inline int sd_lattice_lds_bytes() { return 4 * 2 * (SD_LANES / 64); }                             // two rows of wave boundary values

// what the launches refuse: 0 fine, 1 invalid, 2 outside the kernels' limits
inline int sd_shape_status(int64_t batch, int64_t n, int64_t m, int64_t d) {
    if (batch <= 0 || n <= 0 || m <= 0 || d <= 0) return 1;
    if (n > SD_MAX_LEN || m > SD_MAX_LEN || d > SD_MAX_DIM) return 2;
    if (sd_cost_blocks(batch, n, m) > 0x7fffffff || batch > 0x3fffffff) return 2;
    return 0;
}

}  // namespace tac
