// Walks the host-side plan of csrc/soft_dtw.hip (csrc/soft_dtw_plan.hpp) over a grid of (N, M, D) on the CPU: build with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I torchaudio-contrib_amd/csrc \
//       tools/soft_dtw_plan_check.cpp -o soft_dtw_plan_check && ./soft_dtw_plan_check
// and it returns 0 when every accepted shape has a lattice workgroup of whole waves whose lanes cover every row exactly once, tile
// grids that cover every position, diagonal, row and column, skewed indices inside their array and LDS inside the limit.
#include <stdio.h>

#include "soft_dtw_plan.hpp"

using namespace tac;

static int fail(const char* what, long long a, long long b, long long c) {
    printf("FAILED: %s at (%lld, %lld, %lld)\n", what, a, b, c);
    return 1;
}

int main() {
    const int64_t lens[] = {1, 2, 31, 32, 33, 63, 64, 65, 400, SD_LANES - 1, SD_LANES, SD_LANES + 1, 2 * SD_LANES, 2 * SD_LANES + 1,
                            SD_MAX_LEN - 1, SD_MAX_LEN, SD_MAX_LEN + 1, (int64_t)1 << 33};
    const int64_t dims[] = {1, 3, 4, 5, 33, 80, SD_MAX_DIM, SD_MAX_DIM + 1};
    const int64_t batches[] = {1, 8, 64, 4096};
    long long accepted = 0;
    for (int64_t N : lens)
        for (int64_t M : lens)
            for (int64_t D : dims)
                for (int64_t B : batches) {
                    const int status = sd_shape_status(B, N, M, D);
                    const bool over = N > SD_MAX_LEN || M > SD_MAX_LEN || D > SD_MAX_DIM;
                    if (over != (status == 2) && sd_cost_blocks(B, N, M) <= 0x7fffffff) return fail("limits", N, M, D);
                    if (status != 0) continue;
                    ++accepted;
                    const int rows = sd_rows_per_lane(N), threads = sd_threads(N);
                    if (rows < 1 || rows > SD_MAX_ROWS || (rows & (rows - 1))) return fail("rows per lane", N, M, D);
                    if (threads % 64 || threads < 64 || threads > SD_LANES) return fail("workgroup", N, M, D);
                    if ((int64_t)threads * rows < N || ((int64_t)threads - 64) * rows >= N) return fail("row cover", N, M, D);
                    if (rows > 1 && (int64_t)SD_LANES * (rows / 2) >= N) return fail("rows per lane not least", N, M, D);
                    const int64_t K = sd_diagonals(N, M);
                    if ((N - 1 + M - 1) * N + (N - 1) >= K * N || sd_skewed_elems(B, N, M) != B * K * N) return fail("skewed index", N, M, D);
                    if (sd_tiles(N) * SD_TILE < N || (sd_tiles(N) - 1) * SD_TILE >= N) return fail("row tiles", N, M, D);
                    if (sd_tiles(K) * SD_TILE < K || (sd_tiles(K) - 1) * SD_TILE >= K) return fail("diagonal tiles", N, M, D);
                    if (sd_grad_blocks(B, N, M) != B * (sd_tiles(N) + sd_tiles(M)) || sd_grad_blocks(B, N, M) > 0x7fffffff)
                        return fail("gradient grid", N, M, D);
                    if (SD_MAX_DIM > 2 * SD_WAVES * SD_TILE) return fail("column blocks", N, M, D);
                }
    if (sd_cost_lds_bytes() > SD_LDS_LIMIT || sd_grad_lds_bytes() > SD_LDS_LIMIT || sd_lattice_lds_bytes() > SD_LDS_LIMIT)
        return fail("LDS", 0, 0, 0);
    if (sd_threads(SD_MAX_LEN) != SD_LANES || sd_rows_per_lane(SD_MAX_LEN) != SD_MAX_ROWS) return fail("longest row", SD_MAX_LEN, 0, 0);
    if (sd_shape_status(0, 4, 4, 4) != 1 || sd_shape_status(1, 0, 4, 4) != 1 || sd_shape_status(1, 4, 4, 0) != 1)
        return fail("refusals", 0, 0, 0);
    printf("soft_dtw plan: %lld shapes walked, all consistent\n", accepted);
    return 0;
}
