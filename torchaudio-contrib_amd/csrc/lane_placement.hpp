// lane_placement.hpp — host side of the one-frame-per-wave filterbank contractions (melspec_stream3.hpp at fft_length 2048,
// stft_n4096_s3.hpp at 4096): where each lane's band run starts in the |X|^p row so that a wave's 16-byte row reads do not collide.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>

namespace tac {

// Bank-aware placement: a slot runs more steps than most of its bands need, so a band's run may start up to that many quads
// earlier (zero weights in front).  The LDS serves a wave's 16-byte reads in four fixed groups of sixteen lanes, one cycle per
// group when the sixteen quads fall into sixteen different bank groups ((byte / 16) mod 16; equal addresses are one broadcast):
// within every such group the starts are chosen by bipartite matching (lane -> residue, each lane's candidates being its slack
// window) with the smallest possible load per residue.  A wave's conflict pattern is the same for every step of a slot, since all
// its lanes advance by one quad per step.  (Measured on the standard 128-band bank at 2048: 144 -> 84 LDS cycles per frame for the
// row reads, ideal 72.)
//   lo[64 s + l]: first bin of the band of slot s, lane l, a multiple of four; len[]: bins from there to the band's last non-zero
//   weight (0: no band); steps[s]: four-tap steps slot s runs.  Returns the chosen first bins.
inline std::vector<int> place_band_starts(int nslot, const int* steps, const std::vector<int>& lo, const std::vector<int>& len) {
    std::vector<int> start(lo);
    static const int kGroup[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    for (int s = 0; s < nslot; ++s)
        for (int gi = 0; gi < 4; ++gi) {
            int lanes[16];
            for (int i = 0; i < 16; ++i) lanes[i] = kGroup[gi & 1][i] + 32 * (gi >> 1);
            std::vector<int> cand[16];
            for (int i = 0; i < 16; ++i) {
                const int m = s * 64 + lanes[i];
                const int slack = std::max(0, std::min(steps[s] - (len[m] + 3) / 4, lo[m] / 4));
                for (int d = 0; d <= slack; ++d) cand[i].push_back(lo[m] - 4 * d);
            }
            for (int cap = 1; cap <= 16; ++cap) {
                std::vector<int> load[16];                               // lanes (indices into `lanes`) per residue
                int choice[16];
                // Kuhn's augmenting search with residue capacities: ONE visited set per top-level lane, shared by the whole
                // recursion (a residue that could not be freed once in this search cannot be freed later in it either), so
                // an infeasible cap is refused in O(lanes x candidates) instead of exploring every eviction order
                unsigned seen = 0;
                std::function<bool(int)> place = [&](int i) -> bool {
                    for (int c : cand[i]) {
                        const int r = (c / 4) & 15;
                        if (seen & (1u << r)) continue;
                        seen |= 1u << r;
                        if ((int)load[r].size() < cap) { load[r].push_back(i); choice[i] = c; return true; }
                        for (size_t q = 0; q < load[r].size(); ++q) {
                            const int other = load[r][q];
                            if (place(other)) {                       // `other` moved to another residue: its seat here goes to i
                                load[r].erase(std::find(load[r].begin(), load[r].end(), other));
                                load[r].push_back(i);
                                choice[i] = c;
                                return true;
                            }
                        }
                    }
                    return false;
                };
                bool ok = true;
                for (int i = 0; i < 16 && ok; ++i) {
                    seen = 0;
                    ok = place(i);
                }
                if (ok) {
                    for (int i = 0; i < 16; ++i) start[s * 64 + lanes[i]] = choice[i];
                    break;
                }
            }
        }
    return start;
}

// LDS cycles of a frame's row reads for chosen first bins: per slot and sixteen-lane group, steps x the largest number of DIFFERENT quads
// that share a bank group (what place_band_starts minimises per group; 4 x steps per slot is conflict-free)
inline int row_read_cycles(int nslot, const int* steps, const std::vector<int>& first) {
    static const int kGroup[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    int total = 0;
    for (int s = 0; s < nslot; ++s)
        for (int gi = 0; gi < 4; ++gi) {
            std::vector<int> quads[16];
            int worst = 1;
            for (int i = 0; i < 16; ++i) {
                const int q = first[s * 64 + kGroup[gi & 1][i] + 32 * (gi >> 1)] / 4;
                std::vector<int>& v = quads[q & 15];
                if (std::find(v.begin(), v.end(), q) == v.end()) v.push_back(q);
                worst = std::max(worst, (int)v.size());
            }
            total += steps[s] * worst;
        }
    return total;
}

}  // namespace tac
