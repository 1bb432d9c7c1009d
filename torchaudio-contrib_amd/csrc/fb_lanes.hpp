// fb_lanes.hpp — geometry of the wave-autonomous band-sparse contraction (one frame per wave, LANES = 64 of mel_lanes.hpp), shared by
// its two users: fb_lanes_kernel (melspec_sparse.hip: functional.apply_filterbank on a frame-major spectrogram) and
// stretch_mel_kernel (stretch.hip: the same contraction behind a loader that interpolates two source frames).  The packed layout
// depends on the steps in flight (lm_group), so tac_melbank_pack(..., n_fft = 0, ...) and both launches use these rules.
#pragma once
#include "mel_lanes.hpp"

namespace tac {

constexpr int FBL_CHUNKS = 5, FBL_CHUNKS_WIDE = 9;   // 16-byte chunks per lane and frame: up to 1280 / 2304 bins (fft_length 2048 / 4096)
__host__ __device__ inline bool fbl_is_wide(int n_freqs) { return (n_freqs + 3) / 4 > FBL_CHUNKS * 64; }
__host__ __device__ inline int fbl_waves(int n_freqs) { return fbl_is_wide(n_freqs) ? 8 : 16; }
__host__ __device__ inline int fbl_fly(int n_freqs) { return fbl_is_wide(n_freqs) ? 16 : 8; }
__host__ __device__ inline int fbl_pitch(int n_freqs) { return (n_freqs + 3 + 3) & ~3; }
inline size_t fbl_base_lds(int n_freqs) { return (size_t)fbl_waves(n_freqs) * (fbl_pitch(n_freqs) + LM_MAX_MELS + 4) * sizeof(float) + 16; }

}  // namespace tac
