"""Shared by tests/test_grid_rules_cpu.py and tests/test_grid_wrap_gpu.py (a plain module: no tests in here): the grid every
persistent side kernel is launched with, restated from its launcher, and the smallest shapes at which a workgroup of that grid
walks its loop more than once.

Every launcher here asks for ``persistent_blocks(units, per_block, cap)`` workgroups — ``min(ceil(units / per_block), cap)``, the
cap a multiple of the CU count — and a workgroup walks ``for (u = blockIdx.x; u < units; u += gridDim.x)``.  With ``work =
ceil(units / per_block)`` (the workgroups an unbounded grid would have) and ``grid`` the cap, a launch is held to one of

  * TWO_ROUNDS   ``work = 2 grid + r, 0 < r < grid``: every workgroup takes two units and a few take three; ``r`` is odd wherever
                 the unit count can be odd (a row of an even number of tiles makes ``work`` even like ``2 grid``: then ``r`` is even),
  * STREAMED     ``work >= 1.25 grid`` (the streamed MAC kernel only, whose tile of 80 frames makes two rounds a 350 MB spectrum),
  * ELEMENTS_2   ``work > 2 grid`` and ELEMENTS_1 ``work > grid``: the grid-stride element kernels, ``work = ceil(n / 256)``.

Beside each function stand the source file (under the package's ``csrc/``) and the launcher expressions it restates, verbatim:
tests/test_grid_rules_cpu.py looks every one of them up in that file, so that a retuned cap fails there and not by a GPU test that
silently stopped wrapping.  Where ``per_cu`` depends on the LDS bytes of a bank (``tac_polyphase_f32``) it is the launcher's own,
from the ``bytes`` formula restated in tests/polyphase_rules.py (``lds_variant``), as is the tile: 2 .. 8 workgroups per CU for the
banks used here, at 1024, 512 and 256 outputs per tile.

``shapes(cus)`` gives every size tests/test_grid_wrap_gpu.py uses on a device of ``cus`` compute units; ``launches_of(cus, case)`` computes
``(work, grid)`` from those sizes and ``assert_wraps`` holds them to the case's rule (the GPU tests call it before they launch).  The
numbers of distinct base rows and frames (5 and 67) share no factor with a grid (a power of two times 1 or 19): the successive
units of one workgroup hold different data.

The second half restates the launchers of the STFT chain itself (forward kernels, float64 chain, waveform gradients) for
tests/test_chain_grid_wrap_gpu.py and tests/test_chain_wrap_rules_cpu.py: ``CHAIN_SPECS`` names each instantiation with its
arguments and the route its launcher records, ``chain_shapes(cus)`` (a part of ``shapes``) finds for each the two smallest shapes of
two rounds — three long rows, and many rows of the fewest frames the launcher takes."""
import math

import polyphase_rules as PR
import resample_rules as RS

CU_COUNTS = (256, 304)
MAX_TENSOR_BYTES = 512 * 1000 * 1000
TWO_ROUNDS, STREAMED, ELEMENTS_2, ELEMENTS_1 = 'two rounds', 'streamed', 'elements x 2', 'elements'

BASE_ROWS = 5
BASE_FRAMES = 67


def ceil_div(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- host_common.hpp
PERSISTENT_BLOCKS = ('host_common.hpp', (
    'inline long long persistent_blocks(long long units, long long per_block, long long max_blocks) {',
    'const long long want = (units + per_block - 1) / per_block;',
    'const long long blocks = want < max_blocks ? want : max_blocks;',
    'return blocks < 1 ? 1 : blocks;',
))


def persistent_blocks(units, per_block, max_blocks):
    return max(1, min(ceil_div(units, per_block), max_blocks))


def _launch(units, per_block, cap):
    """(work, grid): the workgroups an unbounded grid would have, and the cap the launcher holds it to"""
    return ceil_div(units, per_block), cap


# ----------------------------------------------------------------------------- tac_lfilter_f32
LFILTER = ('lfilter.hip', (
    'constexpr int LF_TILE = LF_THREADS * LF_C;',
    'persistent_blocks(rows, 1, (long long)device_cu_count() * 2)',
    'for (long long row = blockIdx.x; row < rows; row += gridDim.x) {',
))
LFILTER_TILE = 1024 * 16


def lfilter_launch(cus, rows):
    """a unit is a row"""
    return _launch(rows, 1, 2 * cus)


# ----------------------------------------------------------------------------- tac_polyphase_f32
POLYPHASE = ('resample.hip', (
    'const long long tiles_per_row = (l_out + (1LL << tile_log) - 1) >> tile_log;',
    'const long long units = rows * tiles_per_row;',
    'long long per_cu = (long long)(RS_LDS_BYTES / bytes);',
    'per_cu = per_cu > 8 ? 8 : per_cu;',
    'persistent_blocks(units, 1, (long long)device_cu_count() * per_cu)',
    'for (long long u = blockIdx.x; u < units; u += gridDim.x) {',
))
POLYPHASE_TILE = 1024                   # outputs per tile for the short banks (the GPU tests assert it: _hip.resample_tile)
POLYPHASE_PER_CU = 8                    # the upper bound of per_cu


def polyphase_form(orig, new, adjoint=False):
    """(tile, per_cu) of the launch with the forward or the adjoint bank of ``orig -> new`` at the default filter"""
    v = PR.lds_variant(PR.geometry(orig, new, adjoint=adjoint), True)
    return v[0], v[4]


def polyphase_launch(cus, rows, l_out, tile=POLYPHASE_TILE, per_cu=POLYPHASE_PER_CU):
    """a unit is a tile of ``tile`` outputs of one row; ``per_cu`` the launcher's, from the LDS bytes of the bank"""
    assert 1 <= per_cu <= POLYPHASE_PER_CU
    return _launch(rows * ceil_div(l_out, tile), 1, per_cu * cus)


# ----------------------------------------------------------------------------- tac_dct_rows_f32
DCT = ('mfcc.hip', (
    'DCT_LDS_BYTES = 160 * 1024',
    'for (int tf_log = 6; tf_log >= 4; --tf_log) {',
    '*bytes = 4 * ((size_t)n_in * ldm + ((size_t)(pitch + n_out) << tf_log));',
    'if (rows > 1 && stride_r == n_frames * stride_t) {',
    'const long long tiles_per_row = (n_frames + (1LL << tf_log) - 1) >> tf_log;',
    'long long per_cu = (long long)(DCT_LDS_BYTES / bytes);',
    'per_cu = per_cu > 8 ? 8 : per_cu;',
    'persistent_blocks(units, 1, (long long)device_cu_count() * per_cu)',
    'for (long long u = blockIdx.x; u < units; u += gridDim.x) {',
))
DCT_LDS_BYTES = 160 * 1024


def dct_tile(n_in, n_out):
    """(frames per tile, LDS bytes of a workgroup): the largest of 64 / 32 / 16 frames whose tile fits beside the matrix"""
    ldm, pitch = (n_out + 3) & ~3, n_in | 1
    for tf_log in (6, 5, 4):
        nbytes = 4 * (n_in * ldm + ((pitch + n_out) << tf_log))
        if nbytes <= DCT_LDS_BYTES:
            return 1 << tf_log, nbytes
    raise ValueError('no tile of %d x %d fits' % (n_in, n_out))


def dct_launch(cus, rows, n_frames, n_in, n_out):
    """a unit is a tile of frames of one row; ``rows`` as the kernel sees them (rows whose frames are contiguous are merged into
    one by the launcher: pass 1 and their frames together)"""
    tile, nbytes = dct_tile(n_in, n_out)
    return _launch(rows * ceil_div(n_frames, tile), 1, min(8, DCT_LDS_BYTES // nbytes) * cus)


# ----------------------------------------------------------------------------- tac_spectral_mac_f32
MAC = ('fftconvolve.hip', (
    'constexpr int MAC_WAVES = 4;',
    'constexpr int MAC_SUB = 16;',
    'inline int mac_bucket(int P) { return P <= 4 ? 4 : (P <= 8 ? 8 : (P <= 16 ? 16 : 0)); }',
    'if (pb) return 4 * pb;',
    'return ((4 * P + MAC_SUB - 1) / MAC_SUB) * MAC_SUB;',
    'a.tiles = (int)((T + a.tile - 1) / a.tile);',
    'a.bin_tiles = (F + 63) / 64;',
    'a.units = rows * a.tiles * (long long)a.bin_tiles;',
    'persistent_blocks(a.units, MAC_WAVES, (long long)device_cu_count() * 8)',
    'unit < a.units; unit += (long long)gridDim.x * MAC_WAVES) {',
))
MAC_WAVES = 4


def mac_tile(parts):
    bucket = 4 if parts <= 4 else (8 if parts <= 8 else (16 if parts <= 16 else 0))
    return 4 * bucket if bucket else ceil_div(4 * parts, 16) * 16


def mac_launch(cus, rows, n_frames, n_bins, parts):
    """a unit is (row, time tile, 64 bins), one per wave of a workgroup of MAC_WAVES"""
    return _launch(rows * ceil_div(n_frames, mac_tile(parts)) * ceil_div(n_bins, 64), MAC_WAVES, 8 * cus)


# ----------------------------------------------------------------------------- fc_pad / fc_keep / fc_kernel_blocks
FC = ('fftconvolve.hip', (
    'inline long long fc_grid(long long work) { return persistent_blocks(work, 256, (long long)device_cu_count() * 8); }',
    'pl->T = (offset + l_out + pl->B - 1) / pl->B;',
    'pl->xp_floats = (pl->T + 1) * pl->B;',
    'fc_grid(rn * pl.xp_floats)',
    'fc_grid(rn * l_out)',
    'fc_grid(h_rows * pl.P * (long long)pl.N)',
    'idx < total; idx += (long long)gridDim.x * blockDim.x) {',
))


def fc_plan(l_in, m, n_fft, offset=0, l_out=None):
    """(T output blocks, floats of a row's padded copy, partitions of the kernel)"""
    b = n_fft // 2
    l_out = l_in + m - 1 - offset if l_out is None else l_out
    t = ceil_div(offset + l_out, b)
    return t, (t + 1) * b, ceil_div(m, b)


def fc_pad_launch(cus, rows, l_in, m, n_fft):
    return _launch(rows * fc_plan(l_in, m, n_fft)[1], 256, 8 * cus)


def fc_keep_launch(cus, rows, l_in, m, n_fft):
    return _launch(rows * (l_in + m - 1), 256, 8 * cus)


def fc_kernel_blocks_launch(cus, h_rows, m, n_fft):
    return _launch(h_rows * ceil_div(m, n_fft // 2) * n_fft, 256, 8 * cus)


# ----------------------------------------------------------------------------- istft_grad_input / istft_grad_bins
ISTFT_GRAD = ('istft.hip', (
    'inline long long grid_for(long long work) { return persistent_blocks(work, 256, (long long)device_cu_count() * 8); }',
    'tac::grid_for(d->rows * P)',
    'tac::grid_for(n_frames_total * (n_fft / 2 + 1))',
    'const int64_t p = (int64_t)d->hop * (n_frames - 1) + d->n_fft;',
))


def istft_grad_input_launch(cus, rows, n_frames, n_fft, hop):
    return _launch(rows * (hop * (n_frames - 1) + n_fft), 256, 8 * cus)


def istft_grad_bins_launch(cus, rows, n_frames, n_fft):
    return _launch(rows * n_frames * (n_fft // 2 + 1), 256, 8 * cus)


# ----------------------------------------------------------------------------- tac_hpss_backward_f32
HPSS_BACKWARD = ('hpss.hip', (
    'const long long total = rows * n_freqs * (long long)n_frames;',
    'launch_kernel(hpss_backward_kernel, persistent_blocks(total, 256, (long long)device_cu_count() * 16), 256, 0,',
    'e < total; e += (long long)gridDim.x * blockDim.x) {',
))


def hpss_backward_launch(cus, rows, n_freqs, n_frames):
    return _launch(rows * n_freqs * n_frames, 256, 16 * cus)


# ============================================================================= the STFT chain (tests/test_chain_grid_wrap_gpu.py)
# A chain case names its launcher as a tuple ``grid`` = (kind, parameters...); ``chain_launch(cus, grid, rows, n_frames)`` restates
# that launcher.  ``group`` is the number of frames a wave or workgroup takes at once (F::G, slots, plan.group): a row whose frame
# count is no multiple of it ends in a partial group.
LDS_BYTES = 160 * 1024
STFT_WAVES = 4

WAVE_FFT = ('fft_core.hpp', (
    'static constexpr int LPF = NC / E;',
    'static constexpr int G = 64 / LPF;',
    'static constexpr int PADDED = NC + NC / 16 + 1;',
))


def wave_fft(nc, e):
    """(frames per wave, LDS complex slots per frame) of WaveFft<NC, E>"""
    return 64 // (nc // e), nc + nc // 16 + 1


# ----------------------------------------------------------------------------- 1. stft_kernel<NC, E, MODE, 1, HOIST, 4 | 8>
STFT_GENERIC = ('stft_kernels.hip', (
    'constexpr int STFT_WAVES = 4;',
    'constexpr int NF = 1;',
    'const long long groups = g.rows * ((g.n_frames + NF * F::G - 1) / (NF * F::G));',
    'constexpr size_t wave_bytes = (size_t)(((NF * F::G * F::PADDED + 1) / 2) * 2) * sizeof(cf);',
    'constexpr bool WIDE_FITS = 2 * STFT_WAVES * wave_bytes + 16 <= 160 * 1024;',
    'const bool wide = WIDE_FITS && groups >= 2LL * STFT_WAVES * device_cu_count();',
    'const int waves = wide ? 2 * STFT_WAVES : STFT_WAVES;',
    'const size_t lds_bytes = (size_t)waves * wave_bytes + 16;',
    'int per_cu = wide ? 1 : (int)(160 * 1024 / lds_bytes);',
    'if (per_cu > 2) per_cu = 2;',
    'const long long blocks = persistent_blocks(groups, waves, (long long)device_cu_count() * per_cu);',
    'set_last_route("stft_kernel<%d, %d, %d, %d, %d, %d>", NC, E, MODE, NF, HOIST ? 1 : 0, waves);',
    'case 64: return launch_stft<32, 16, MODE>(g, tb, ep, s);',
    'return n_fft == 512 ? launch_stft<256, 16, MODE>(g, tb, ep, s) : launch_stft<512, 16, MODE>(g, tb, ep, s);',
    'case 2048: return launch_stft<1024, 16, MODE>(g, tb, ep, s);',
    'return launch_stft<2048, 32, MODE>(g, tb, ep, s);',
))
GENERIC_CORES = ((16, 16), (32, 16), (64, 16), (128, 16), (256, 16), (512, 16), (1024, 16), (2048, 32))   # every launch_stft<NC, E>


def generic_form(cus, rows, n_frames, nc, e):
    """(wave-iterations, waves of a workgroup, workgroups per CU) of ``launch_stft<NC, E>``"""
    g, padded = wave_fft(nc, e)
    groups = rows * ceil_div(n_frames, g)
    wave_bytes = (g * padded + 1) // 2 * 2 * 8
    wide = 2 * STFT_WAVES * wave_bytes + 16 <= LDS_BYTES and groups >= 2 * STFT_WAVES * cus
    waves = 2 * STFT_WAVES if wide else STFT_WAVES
    per_cu = 1 if wide else max(1, min(2, LDS_BYTES // (waves * wave_bytes + 16)))
    return groups, waves, per_cu


def generic_launch(cus, rows, n_frames, nc, e):
    groups, waves, per_cu = generic_form(cus, rows, n_frames, nc, e)
    return _launch(groups, waves, cus * per_cu)


def narrow_generic_never_wraps(cus, nc, e):
    """the 4-wave form is launched below ``2 STFT_WAVES CUs`` wave-iterations only, and every core's eight frame buffers fit the
    LDS (WIDE_FITS): its grid of ``per_cu CUs`` workgroups then holds them all — no shape walks ITS loop twice"""
    groups = 2 * STFT_WAVES * cus - 1                                               # the most the narrow form is given
    g = wave_fft(nc, e)[0]
    got, waves, per_cu = generic_form(cus, groups, g, nc, e)
    return got == groups and waves == STFT_WAVES and ceil_div(groups, waves) <= cus * per_cu


# ----------------------------------------------------------------------------- 2. stft_pipe_kernel, 3. stft_stream3_kernel / stft_ring3_kernel
STFT_2048 = ('stft_kernels.hip', (
    'constexpr int PIPE_WAVES = 8;',
    'const long long blocks = persistent_blocks(groups, WAVES, (long long)device_cu_count() * (8 / WAVES));',
    'if (two_wave || g.length < 2 * NC) return launch_pipe<NC, E, PMODE>(g, tb, ep, groups, stream);',
    'const int waves = waves_env ? waves_env : (PMODE == 0 ? 12 : 16);',
    'const long long blocks = persistent_blocks(groups, W, device_cu_count());',
    'const Stream3Launch lp{(frames_total + blocks - 1) / blocks, plain};',
    '#define TAC_S3_RING_TW 12',
    'const long long blocks = persistent_blocks(groups, TWv, device_cu_count());',
    'const int hpf = g.hop > 0 && (2 * NC) % g.hop == 0 ? 2 * NC / g.hop : 0;',
    'if (hpf == 4) return ring(std::integral_constant<int, 4>{});',
))
PIPE_WAVES = 8
RING_TW = 12


def waves_launch(cus, rows, n_frames, waves, group=1, per_cu=1):
    """one workgroup of ``waves`` waves per CU, a wave takes ``group`` frames of one row at a time: stft_pipe_kernel (8), the
    stream3 / ring3 kernels (12 | 16; their blocks take ``ceil(frames / blocks)`` consecutive frames across the rows), the
    small3 kernels (12 | 16, F::G frames a wave), stft_n4096_kernel (8); two workgroups of 4 waves per CU: the frame kernel of
    ``tac_stft_backward_f32``"""
    return _launch(rows * ceil_div(n_frames, group), waves, cus * per_cu)


# ----------------------------------------------------------------------------- 4. stft_small3_kernel<NC, MODE, false, 1, 12 | 16>
STFT_SMALL3 = ('stft_small.hip', (
    'const long long units = g.rows * ((g.n_frames + F::G - 1) / F::G);',
    'const long long cap = device_cu_count();',
    'return launch_kernel(k3, persistent_blocks(units, W, cap), W * 64, small3_lds_bytes<NC>(W), stream, g, tb, ep, LaneMel{},',
    'const int wv = getenv("TAC_SM3_WAVES") ? small3_waves() : (MODE == 0 ? 12 : 16);',
    'set_last_route("stft_small3_kernel<%d, %d, 0, 1, %d>", NC, MODE, wv == 12 ? 12 : 16);',
))

# ----------------------------------------------------------------------------- 5. stft_smooth_kernel / stft_smooth_backward_kernel
STFT_SMOOTH = ('stft_smooth.hip', (
    'constexpr int SM_THREADS = 256;',
    'const long long units = g.rows * g.n_frames;',
    'const int tpf = M <= 1024 ? 64 : 256, slots = SM_THREADS / tpf;',
    'const size_t lds_full = ((size_t)n_fft + 2 * (size_t)M * slots) * sizeof(cf), lds_half = lds_full - (size_t)(M - 1) * sizeof(cf);',
    'const bool full = !((160 * 1024) / lds_full < 2 && (160 * 1024) / lds_half >= 2);',
    'int per_cu = (int)((160 * 1024) / lds);',
    'per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);',
    'const long long blocks = persistent_blocks(units, slots, (long long)device_cu_count() * per_cu);',
    'set_last_route("stft_smooth_kernel<%d, %d%s>", mode == 0 ? 0 : 1, tpf, full ? "" : ", false");',
))


def smooth_form(n_fft):
    """(frames a workgroup takes at once, workgroups per CU, LDS form) of stft_smooth_kernel and its backward kernel: '64' (four
    frames of 64 threads), '256' (one frame, the whole buffer pair), '256 half' (one frame, the halved second buffer)"""
    m = n_fft // 2
    tpf = 64 if m <= 1024 else 256
    slots = 256 // tpf
    lds_full = (n_fft + 2 * m * slots) * 8
    lds_half = lds_full - (m - 1) * 8
    full = not (LDS_BYTES // lds_full < 2 and LDS_BYTES // lds_half >= 2)
    per_cu = max(1, min(8, LDS_BYTES // (lds_full if full else lds_half)))
    return slots, per_cu, '64' if tpf == 64 else ('256' if full else '256 half')


def smooth_launch(cus, rows, n_frames, n_fft):
    slots, per_cu, _ = smooth_form(n_fft)
    return _launch(rows * n_frames, slots, cus * per_cu)


# ----------------------------------------------------------------------------- 6. stft_big_kernel<S, MODE, WAVES>
STFT_BIG = ('stft_big.hip', (
    'const long long units = g.rows * g.n_frames;',
    'constexpr int WAVES = S == 16 ? 8 : S;',
    'const long long blocks = persistent_blocks(units, 1, (long long)device_cu_count() * (8 / WAVES));',
))


def big_launch(cus, rows, n_frames, n_fft):
    s = n_fft // 2048
    return _launch(rows * n_frames, 1, cus * (8 // (8 if s == 16 else s)))


# ----------------------------------------------------------------------------- 7. stft_n4096_kernel<0>: complex rows
STFT_N4096 = ('stft_n4096.hip', (
    'constexpr int N4K_WAVES = 8;',
    'const long long blocks = persistent_blocks(units, N4K_WAVES, device_cu_count());',
    'case 0: return launch_n4096<0>(g, tb1k, tb4k, ep, stream);',
))

# ----------------------------------------------------------------------------- 9. stft_f64_kernel<true | false>, stft_f64_direct_kernel, ew_f64_kernel
CHAIN_F64 = ('chain_f64.hip', (
    'if (n_fft < 4 || (n_fft & 1) || n_fft > 8192) return false;',
    'const int radices[4] = {4, 2, 3, 5};',
    'const int per = 1024 / (n_fft / 2);',
    'plan->group = per < 1 ? 1 : (per > 16 ? 16 : per);',
    'const long long cap = (long long)device_cu_count() * 8;',
    'const bool tw_lds = N <= 4096;',
    'persistent_blocks(units, plan.group, cap)',
    'rc = launch_kernel(stft_f64_direct_kernel, persistent_blocks(units, 1, cap), D_THREADS, lds, stream, g, tw, ep, out);',
    'persistent_blocks(n, 256, (long long)device_cu_count() * 16)',
    'i < n; i += (long long)gridDim.x * 256) {',
))


def f64_form(n_fft):
    """(frames a workgroup takes at once, kernel) of ``launch_stft_f64``"""
    m, ok = n_fft // 2, 4 <= n_fft <= 8192 and n_fft % 2 == 0
    for r in (4, 2, 3, 5):
        while ok and m % r == 0:
            m //= r
    if not (ok and m == 1):
        return 1, 'stft_f64_direct_kernel'
    group = max(1, min(16, 1024 // (n_fft // 2)))
    return group, 'stft_f64_kernel<%s>, group %d' % ('true' if n_fft <= 4096 else 'false', group)


def f64_launch(cus, rows, n_frames, n_fft):
    return _launch(rows * n_frames, f64_form(n_fft)[0], 8 * cus)


def ew_f64_launch(cus, n):
    return _launch(n, 256, 16 * cus)


# ----------------------------------------------------------------------------- 8. the waveform gradients (backward.hip)
BACKWARD = ('backward.hip', (
    'constexpr int BW_WAVES = 4;',
    'const long long groups = g.rows * ((g.n_frames + F::G - 1) / F::G);',
    'const int rc = launch_kernel(kern, persistent_blocks(groups, BW_WAVES, (long long)device_cu_count() * 2), BW_WAVES * 64, lds_bytes, stream, g, tb,',
    'static long long bw_blocks(long long n) { return persistent_blocks(n, 256, (long long)device_cu_count() * 16); }',
    'return launch_kernel(overlap_add_kernel, bw_blocks(g.rows * ((g.length + 3) / 4)), 256, 0, (hipStream_t)stream, g, (int)d->n_fft,',
    'constexpr int OLA_WAVES = 4;',
    'constexpr int OLA_NC = 1024, OLA_E = 16, OLA_N = 2048;',
    'const int s_min = std::max(1, (n - d->hop + d->hop - 1) / d->hop);',
    'const long long target = (long long)device_cu_count() * waves_per_cu * (OLA_N / n);',
    'long long spr = (target + g.rows - 1) / g.rows;',
    'spr = std::max(1LL, std::min(spr, (long long)std::max(1, T / s_min)));',
    'int S = (int)((T + spr - 1) / spr);',
    'if (S < s_min) S = s_min;',
    'plan->segs_per_row = (T + S - 1) / S;',
    'static int ola_plan(const tac_stft_desc* d, const FrameGeom& g, OlaPlan* plan, int waves_per_cu = 2 * OLA_WAVES) {',
    'auto units = [&](int streams_per_wave) { return (g.rows * (long long)plan.segs_per_row + streams_per_wave - 1) / streams_per_wave; };',
    'return launch_kernel(kern, persistent_blocks(units(streams_per_wave), waves, (long long)device_cu_count() * 2 * OLA_WAVES / waves),',
    'if (d->n_fft == 2048 && (!adj || (n_mels >= 1 && n_mels <= 256)) && !lds_ring && g.length >= OLA_N &&',
    '(d->hop == 256 || d->hop == 512 || d->hop == 1024)) {',
    'rc = ola_plan(d, g, &p12, BR_WAVES);',
    'return launch_kernel(kern, persistent_blocks(units(1), BR_WAVES, device_cu_count()), BR_WAVES * 64, lds, s, g, tb, grad, power, gpad,',
    'g.length >= d->n_fft && (d->hop == d->n_fft / 8 || d->hop == d->n_fft / 4 || d->hop == d->n_fft / 2)) {',
    'const int G = 2048 / d->n_fft;',
    'return launch_kernel(kern, persistent_blocks(units(G), BR_WAVES, device_cu_count()), BR_WAVES * 64, lds, s, g, tb, grad, power, gpad,',
    'return launch_kernel(fb_adjoint_kernel, persistent_blocks(rows_times_frames, ADJ_WAVES, (long long)device_cu_count() * 4), ADJ_WAVES * 64,',
    'constexpr int ADJ_WAVES = 4;',
    'return launch_kernel(kern, persistent_blocks(units(streams_per_wave), OLA_WAVES, (long long)device_cu_count() * 2), OLA_WAVES * 64,',
    'constexpr int FW = 2 * OLA_WAVES;',
    'rc = pow2 ? launch(spectrogram_backward_ola_kernel<true, true, FW>, lds, 1, FW)',
    'rc = pow2 ? launch_multi(spectrogram_backward_ola_multi_kernel<128, true>, lds_for(128, F::PADDED, F::G), F::G)',
    'if (n == 400 ? ((d->hop & 3) || (g.center_pad & 3) || d->hop < 50) : (d->hop % (n / 16)) != 0) return TAC_E_UNSUPPORTED;',
))
N400_BACKWARD = ('stft_n400.hip', (
    'constexpr int Q4_WAVES = 8;',
    'constexpr int Q4_G = 8;',
    'const long long units = g.rows * ((g.n_frames + Q4_G - 1) / Q4_G);',
    'const int rl = launch_kernel(kern, persistent_blocks(units, Q4_WAVES, device_cu_count()), Q4_WAVES * 64, bytes, stream, g, tb, gspec, gnorm,',
))
Q4_WAVES = Q4_G = 8
BR = ('backward_ring3.hpp', ('constexpr int BR_WAVES = 12;',))
BW_WAVES = OLA_WAVES = ADJ_WAVES = 4
BR_WAVES = 12


def overlap_add_launch(cus, rows, length):
    return _launch(rows * ceil_div(length, 4), 256, 16 * cus)


def fb_adjoint_launch(cus, rows_times_frames):
    return _launch(rows_times_frames, ADJ_WAVES, 4 * cus)


def ola_plan(cus, rows, n_frames, n_fft, hop, waves_per_cu):
    """(frames of a segment, segments of a row): about one segment per resident frame stream of the device, none shorter than
    the frames that overlap one"""
    s_min = max(1, (n_fft - hop + hop - 1) // hop)
    target = cus * waves_per_cu * (2048 // n_fft)
    spr = max(1, min(ceil_div(target, rows), max(1, n_frames // s_min)))
    seg = max(ceil_div(n_frames, spr), s_min)
    return seg, ceil_div(n_frames, seg)


def ola_form(n_fft, hop, adj=False):
    """(waves per CU the plan is made for, frame streams a wave carries, waves of a workgroup, workgroups per CU, kernel) of the
    overlap-add-in-kernel gradient: the register-ring kernels at 2048 (hop 256 / 512 / 1024) and 512 / 1024 (hop n / 8, / 4, / 2);
    at the other hops the LDS-ring kernel of 2048 (4 waves; 8 waves around one copy of the tables with the filterbank adjoint
    folded in, ``adj``) and the multi kernels of 1024 / 512 / 256 (2 / 4 / 8 frame streams a wave)"""
    if n_fft == 2048 and hop in (256, 512, 1024):
        return BR_WAVES, 1, BR_WAVES, 1, 'ring3'
    if n_fft in (512, 1024) and hop in (n_fft // 8, n_fft // 4, n_fft // 2):
        return BR_WAVES, 2048 // n_fft, BR_WAVES, 1, 'ring3_multi'
    if n_fft == 2048:
        assert hop % 128 == 0
        return (2 * OLA_WAVES, 1, 2 * OLA_WAVES, 1, 'ola 8') if adj else (2 * OLA_WAVES, 1, OLA_WAVES, 2, 'ola 4')
    assert n_fft in (1024, 512, 256) and hop % (n_fft // 16) == 0 and not adj
    return 2 * OLA_WAVES, 2048 // n_fft, OLA_WAVES, 2, 'ola_multi'


def ola_route(n_fft, hop, power, adj):
    """the instantiation ``ola_backward_entry`` records"""
    kind, p2, a = ola_form(n_fft, hop, adj)[4], 'true' if power == 2.0 else 'false', 'true' if adj else 'false'
    if kind == 'ring3':
        return 'melspec_backward_ring3_kernel<%s, %d, %s>' % (p2, hop >> 7, a)
    if kind == 'ring3_multi':
        return 'melspec_backward_ring3_multi_kernel<%d, %s, %d, %s>' % (n_fft // 2, p2, hop // (n_fft // 16), a)
    if kind == 'ola_multi':
        return 'spectrogram_backward_ola_multi_kernel<%d, %s>' % (n_fft // 2, p2)
    return 'spectrogram_backward_ola_kernel<%s, %s, %d>' % (p2, a, 8 if adj else 4)


def ola_launch(cus, rows, n_frames, n_fft, hop, adj=False):
    """a unit is a segment of consecutive frames of one row (rows of at least a frame)"""
    plan_waves, streams, waves, per_cu, _ = ola_form(n_fft, hop, adj)
    segs = ola_plan(cus, rows, n_frames, n_fft, hop, plan_waves)[1]
    return _launch(ceil_div(rows * segs, streams), waves, cus * per_cu)


# ----------------------------------------------------------------------------- 10. istft: the general and the fused route
ISTFT = ('istft.hip', (
    'const long long work = d->rows * ((d->length + 3) / 4);',
    'tac::launch_kernel(tac::istft_ola_kernel, tac::grid_for(work), 256, 0, s,',
    'constexpr int IF_WAVES = 4;',
    'const int R = 2048 / hop - 1;',
    'const int min_seg = 4 * R > 8 ? 4 * R : 8;',
    'long long want = ((long long)device_cu_count() * 2 * IF_WAVES + rows - 1) / rows;',
    'long long most = (T + min_seg - 1) / min_seg;',
    'if (want > most) want = most;',
    'int sf = (int)((T + want - 1) / want);',
    '*segs_per_row = (T + sf - 1) / sf;',
    'const long long units = g.rows * segs_per_row;',
    'persistent_blocks(units, IF_WAVES, (long long)device_cu_count() * 2)',
))
IF_WAVES = 4


def istft_length(n_frames, hop, trim=0):
    """the samples of a row that ``istft`` returns for ``n_frames`` centred frames, ``trim`` fewer with ``length=``"""
    return hop * (n_frames - 1) - trim


def istft_ola_launch(cus, rows, n_frames, hop, trim=0):
    """istft_ola_kernel of the general route: a thread takes four output samples of a row"""
    return _launch(rows * ceil_div(istft_length(n_frames, hop, trim), 4), 256, 8 * cus)


def istft_fused_plan(cus, rows, n_frames, hop):
    """(frames of a segment, segments of a row) of istft_fused_kernel<hop>: about one segment per resident wave"""
    r = 2048 // hop - 1
    min_seg = max(4 * r, 8)
    want = max(1, min(ceil_div(cus * 2 * IF_WAVES, rows), ceil_div(n_frames, min_seg)))
    seg = ceil_div(n_frames, want)
    return seg, ceil_div(n_frames, seg)


def istft_fused_launch(cus, rows, n_frames, hop):
    """a unit is a segment of one row, a wave takes one at a time"""
    return _launch(rows * istft_fused_plan(cus, rows, n_frames, hop)[1], IF_WAVES, 2 * cus)


def chain_launch(cus, grid, rows, n_frames):
    kind = grid[0]
    if kind == 'ola':
        return ola_launch(cus, rows, n_frames, *grid[1:])
    if kind == 'istft_ola':
        return istft_ola_launch(cus, rows, n_frames, *grid[1:])
    if kind == 'istft_fused':
        return istft_fused_launch(cus, rows, n_frames, grid[1])
    if kind == 'generic':
        return generic_launch(cus, rows, n_frames, grid[1], grid[2])
    if kind == 'waves':
        return waves_launch(cus, rows, n_frames, *grid[1:])
    if kind == 'smooth':
        return smooth_launch(cus, rows, n_frames, grid[1])
    if kind == 'big':
        return big_launch(cus, rows, n_frames, grid[1])
    if kind == 'f64':
        return f64_launch(cus, rows, n_frames, grid[1])
    raise KeyError(kind)


QUOTED = (PERSISTENT_BLOCKS, LFILTER, POLYPHASE, DCT, MAC, FC, ISTFT_GRAD, HPSS_BACKWARD,
          WAVE_FFT, STFT_GENERIC, STFT_2048, STFT_SMALL3, STFT_SMOOTH, STFT_BIG, STFT_N4096, CHAIN_F64, BACKWARD, BR, N400_BACKWARD, ISTFT)


def frames_of_length(length, n_fft, hop, center=True):
    return 1 + (length + (2 * (n_fft // 2) if center else 0) - n_fft) // hop


def _spec(family, n, hop, grid, group, entry, route, power=None, onesided=True, f64=False, db=False, min_len=0, max_len=None,
          forms=('long', 'short'), same_kernel=True, center=True, pad_mode='reflect', gradient=None, mels=0, launches=None,
          inverse=False, trim=0, also=()):
    """``launches``: every launch the op makes, by entry point ({entry: 1} unless given); ``also``: further (what, launcher) pairs of
    the case, held to more than one round (more than two for 'overlap-add'); ``inverse``: an istft case, ``trim`` samples cut by
    ``length=``"""
    return dict(family=family, n=n, hop=hop, grid=grid, group=group, entry=entry, route=route, power=power, onesided=onesided,
                f64=f64, db=db, min_len=max(min_len, n // 2 + 1 if center else n), max_len=max_len, forms=forms,
                same_kernel=same_kernel, center=center, pad_mode=pad_mode, gradient=gradient, mels=mels,
                launches=launches or {entry: 1}, inverse=inverse, trim=trim, also=tuple(also))


def _generic(n, nc, e, power=None, onesided=True):
    mode, hop = 0 if power is None else 1, n // 4
    route = 'stft_kernel<%d, %d, %d, 1, %d, 8>' % (nc, e, mode, 1 if e <= 16 else 0)
    return _spec(1, n, hop, ('generic', nc, e), wave_fft(nc, e)[0], 'tac_stft_f32' if power is None else 'tac_spectrogram_f32', route,
                 power=power, onesided=onesided, same_kernel=False)           # (the five base rows alone run the 4-wave form)


def _small3(n, pmode):
    waves, g = 12 if pmode == 0 else 16, wave_fft(n // 2, 16)[0]
    return _spec(4, n, n // 4, ('waves', waves, g), g, 'tac_stft_f32' if pmode == 0 else 'tac_spectrogram_f32',
                 'stft_small3_kernel<%d, %d, 0, 1, %d>' % (n // 2, pmode, waves), power=(None, 2.0, 1.0)[pmode], min_len=n)


def _smooth(n, mode):
    slots, _, form = smooth_form(n)
    return _spec(5, n, n // 4, ('smooth', n), slots, 'tac_spectrogram_f32' if mode else 'tac_stft_f32',
                 'stft_smooth_kernel<%d, %d%s>' % (mode, 256 // slots, ', false' if form == '256 half' else ''), power=2.0 if mode else None)


def _big(n, mode):
    s = n // 2048
    return _spec(6, n, n // 4, ('big', n), 1, 'tac_spectrogram_f32' if mode else 'tac_stft_f32',
                 'stft_big_kernel<%d, %d, %d>' % (s, mode, 8 if s == 16 else s), power=2.0 if mode else None)


def _f64(n, hop, onesided=True, power=None, db=False):
    group, route = f64_form(n)
    return _spec(9, n, hop, ('f64', n), group, 'tac_stft_f64' if power is None else 'tac_spectrogram_f64', route, power=power,
                 onesided=onesided, f64=True, db=db)


S3, RING = 'stft_stream3_kernel<1024, 16, %d, %d>', 'stft_ring3_kernel<1024, 16, %d, 12, 8>'
CHAIN_SPECS = {
    # 1. the generic kernel, always its 8-wave form (narrow_generic_never_wraps)
    'generic 64, complex': _generic(64, 32, 16),
    'generic 512, two-sided': _generic(512, 256, 16, onesided=False),
    'generic 2048, power 0.7': _generic(2048, 1024, 16, power=0.7),
    'generic 4096, two-sided': _generic(4096, 2048, 32, onesided=False),
    # 2. rows shorter than a frame at 2048: hop 1 gives three rows the frames of two rounds, hop 512 three frames a row
    'pipe 2048, hop 1': _spec(2, 2048, 1, ('waves', PIPE_WAVES), 1, 'tac_stft_f32', 'stft_pipe_kernel<1024, 16, 0, 8>', max_len=2047,
                              forms=('long',)),
    'pipe 2048, hop 512': _spec(2, 2048, 512, ('waves', PIPE_WAVES), 1, 'tac_spectrogram_f32', 'stft_pipe_kernel<1024, 16, 1, 8>',
                                power=2.0, max_len=2047, forms=('short',)),
    # 3. 2048 off hop 512: the ring at hop 256, stream3 at hop 500 (rows of at least a frame: the shortest has 9 / 5 frames)
    'ring 2048 / 256, complex': _spec(3, 2048, 256, ('waves', RING_TW), 1, 'tac_stft_f32', RING % 0, min_len=2048),
    'ring 2048 / 256, power': _spec(3, 2048, 256, ('waves', RING_TW), 1, 'tac_spectrogram_f32', RING % 1, power=2.0, min_len=2048),
    'stream3 2048 / 500, complex': _spec(3, 2048, 500, ('waves', 12), 1, 'tac_stft_f32', S3 % (0, 12), min_len=2048),
    'stream3 2048 / 500, magnitude': _spec(3, 2048, 500, ('waves', 16), 1, 'tac_spectrogram_f32', S3 % (2, 16), power=1.0, min_len=2048),
    # 4. 256 / 512 / 1024 plain epilogues
    'small3 256, complex': _small3(256, 0),
    'small3 512, power': _small3(512, 1),
    'small3 1024, magnitude': _small3(1024, 2),
    # 5. 7-smooth halves: the three LDS forms, both modes
    'smooth 300, complex': _smooth(300, 0), 'smooth 300, power': _smooth(300, 1),
    'smooth 4500, complex': _smooth(4500, 0), 'smooth 4500, power': _smooth(4500, 1),
    'smooth 6000, complex': _smooth(6000, 0), 'smooth 6000, power': _smooth(6000, 1),
    # 6. the four-step kernel
    'big 8192, complex': _big(8192, 0), 'big 16384, power': _big(16384, 1), 'big 32768, power': _big(32768, 1),
    # 7. 4096 complex rows
    'n4096, complex': _spec(7, 4096, 1024, ('waves', 8), 1, 'tac_stft_f32', 'stft_n4096_kernel<0>'),
    # 9. the float64 chain
    'f64 8': _f64(8, 2), 'f64 2048': _f64(2048, 512), 'f64 8192, magnitude': _f64(8192, 2048, power=1.0),
    'f64 6000, power': _f64(6000, 1500, power=2.0),
    'f64 direct 77': _f64(77, 20), 'f64 direct 134, two-sided': _f64(134, 33, onesided=False),
    'f64 2048, magnitude dB': _f64(2048, 512, power=1.0, db=True),
}


def _grad_frames(n, hop, grid, group, route, family=8, **kw):
    """the gradient of the complex rows: one inverse transform a frame (``tac_stft_backward_f32``), then the gather overlap-add"""
    return _spec(family, n, hop, grid, group, 'tac_stft_backward_f32', route, gradient='stft',
                 launches={'tac_stft_backward_f32': 1, 'tac_overlap_add_f32': 1}, **kw)


def _grad_smooth(n, **kw):
    slots, _, form = smooth_form(n)
    route = 'stft_smooth_backward_kernel<%d, %s, false>' % (256 // slots, 'false' if form == '256 half' else 'true')
    return _grad_frames(n, n // 4, ('smooth', n), slots, route, family=5, **kw)


def _grad_ola(n, hop, gradient, mels=0, power=None, fused_adjoint=True, **kw):
    """the gradient of |X|^p or mel rows with the overlap-add inside the kernel.  Its plan cuts a row into no more segments than
    the device has resident frame streams: three long rows never give its grid a second round, many rows of one segment do.
    ``fused_adjoint`` False: mel rows of an fft_length whose kernel does not fold the filterbank adjoint in — fb_adjoint_kernel
    runs first (a wave a frame), then the gradient of the power rows"""
    power = (1.0 if gradient == 'magnitude' else 2.0) if power is None else power
    adj = gradient == 'mel' and fused_adjoint
    entry = 'tac_melspectrogram_backward_ola_f32' if adj else 'tac_spectrogram_backward_ola_f32'
    launches = {entry: 1} if adj or gradient != 'mel' else {'tac_apply_filterbank_adjoint_f32': 1, entry: 1}
    return _spec(8, n, hop, ('ola', n, hop, adj), 1, entry, ola_route(n, hop, power, adj), power=power, gradient=gradient,
                 mels=mels, min_len=n, forms=('short',), launches=launches, also=(('fb_adjoint',),) if len(launches) == 2 else (), **kw)


def _istft_general(n, hop, frame_grid, trim=0):
    """the general route: the frame kernel of ``n`` in inverse mode, then istft_ola_kernel over four samples a thread"""
    return _spec(10, n, hop, ('istft_ola', hop, trim), 1, 'tac_istft_f32',
                 'istft_general<%d>: frame kernel (inverse mode) + istft_ola_kernel<vec4=1>' % n, inverse=True, trim=trim,
                 also=(('frames',) + frame_grid,))


def _istft_fused(hop):
    """istft_fused_kernel<hop>: like the overlap-add gradients, no more segments a row than the device has resident waves"""
    return _spec(10, 2048, hop, ('istft_fused', hop), 1, 'tac_istft_f32', 'istft_fused_kernel<%d>' % hop, inverse=True, forms=('short',))


CHAIN_SPECS.update({
    # 5. the gradients of the 7-smooth lengths: stft_smooth_backward_kernel in its three LDS forms
    'gradient smooth 300': _grad_smooth(300),
    'gradient smooth 4500': _grad_smooth(4500, pad_mode='constant'),
    'gradient smooth 6000': _grad_smooth(6000),
    # 8. the frame kernel of backward.hip (four frames a wave at 512; the E = 32 core at 4096, whose rows of a hop of 4096 also
    # take the gather overlap-add past two rounds of its element grid), without centring
    'gradient frames 512': _grad_frames(512, 128, ('waves', BW_WAVES, wave_fft(256, 16)[0], 2), wave_fft(256, 16)[0],
                                        'stft_backward_kernel<256, 16, SRC_GRAD, false>', center=False),
    'gradient frames 4096 / 4096': _grad_frames(4096, 4096, ('waves', BW_WAVES, 1, 2), 1, 'stft_backward_kernel<2048, 32, SRC_GRAD, false>',
                                                forms=('long',), also=(('overlap-add',),)),
    # ... the overlap-add-in-kernel forms off the 2048 / 512 mel training step.  The register-ring kernels: all three hops of
    # each fft_length (the HH of ``pick``; 2048 / 512 is the training step's), with and without the adjoint, at power 2 and 1
    'gradient ring3 2048 / 256, power': _grad_ola(2048, 256, 'power'),
    'gradient ring3 2048 / 1024, magnitude': _grad_ola(2048, 1024, 'magnitude', center=False),
    'gradient ring3 2048 / 256, mel': _grad_ola(2048, 256, 'mel', mels=64),
    'gradient ring3 2048 / 1024, mel': _grad_ola(2048, 1024, 'mel', mels=64),
    'gradient multi 1024 / 256, power': _grad_ola(1024, 256, 'power', pad_mode='replicate'),
    'gradient multi 512 / 64, magnitude': _grad_ola(512, 64, 'magnitude'),
    'gradient multi 1024 / 512, mel': _grad_ola(1024, 512, 'mel', mels=40),
    'gradient multi 1024 / 128, power': _grad_ola(1024, 128, 'power'),
    'gradient multi 512 / 128, mel magnitude': _grad_ola(512, 128, 'mel', mels=40, power=1.0),
    'gradient multi 512 / 256, power': _grad_ola(512, 256, 'power'),
    'gradient ring3 2048 / 1024, mel magnitude': _grad_ola(2048, 1024, 'mel', mels=64, power=1.0),
    # ... the LDS-ring kernel of 2048 at the other hops (4 waves; 8 waves with the adjoint), the multi kernels of 1024 / 512 / 256
    # at the hops the register ring is not built for — 256 has no other form, and its mel rows take fb_adjoint_kernel first
    'gradient lds ring 2048 / 384, power': _grad_ola(2048, 384, 'power'),
    'gradient lds ring 2048 / 384, mel': _grad_ola(2048, 384, 'mel', mels=64),
    'gradient ola multi 1024 / 192, power': _grad_ola(1024, 192, 'power'),
    'gradient ola multi 512 / 96, magnitude': _grad_ola(512, 96, 'magnitude'),
    'gradient ola multi 256 / 64, mel': _grad_ola(256, 64, 'mel', mels=20, fused_adjoint=False),
    # ... and fft_length 400 at a hop that is no multiple of four: frame gradients (eight frames a wave), then the gather overlap-add
    'gradient n400 / 150, power': _spec(8, 400, 150, ('waves', Q4_WAVES, Q4_G, 1), Q4_G, 'tac_spectrogram_backward_f32',
                                        'stft_n400_backward_kernel<SRC_WAVE, true, false, false>', power=2.0, gradient='power',
                                        launches={'tac_spectrogram_backward_f32': 1, 'tac_overlap_add_f32': 1}),
    # 10. istft off 2048 / 512: the general route at 960 / 240 (the 7-smooth frame kernel; ``length=`` cuts 3 hops and 5 samples) and
    # 400 / 160 (the mixed-radix one), the fused route at hop 256 and 1024
    'istft general 960 / 240, trimmed': _istft_general(960, 240, ('smooth', 960), trim=725),
    'istft general 400 / 160': _istft_general(400, 160, ('waves', Q4_WAVES, Q4_G, 1)),
    'istft fused 2048 / 256': _istft_fused(256),
    'istft fused 2048 / 1024': _istft_fused(1024),
})


def chain_length(spec, n_frames):
    """the length of a row of ``n_frames`` frames (a multiple of four wherever the hop is one of eight: the 16-byte loads), or
    None where the case's launcher does not take it"""
    if spec['inverse']:                              # the samples ``istft`` returns (at least two frames: one has none)
        length = istft_length(n_frames, spec['hop'], spec['trim'])
        return length if length > 0 else None
    length = (n_frames - 1) * spec['hop'] + spec['hop'] // 2 + (0 if spec['center'] else spec['n'])
    if length < spec['min_len'] or (spec['max_len'] is not None and length > spec['max_len']):
        return None
    return length


def _chain_case(cus, spec, form):
    """'long': three rows, the fewest frames a row with two rounds of the grid and a remainder; 'short': the fewest frames a row
    the launcher takes (1 ... 3 where rows may be that short), no multiple of ``group``, and the fewest rows with two rounds"""
    def fits(t):
        return chain_length(spec, t) is not None and (spec['group'] == 1 or t % spec['group'] != 0)

    def search(candidates):
        even = None
        for rows, t in candidates:
            if not fits(t):
                continue
            work, grid = chain_launch(cus, spec['grid'], rows, t)
            r = work - 2 * grid
            if r >= grid:
                break
            if r > 0 and r % 2 == 1:
                return rows, t
            if r > 0 and even is None:
                even = (rows, t)
        assert even is not None, 'no shape of two rounds for %r' % (spec,)
        return even

    if form == 'long':
        rows, t = search((3, t) for t in range(1, 1 << 20))
    else:
        t0 = next(t for t in range(1, 1 << 12) if fits(t))
        rows, t = search((rows, t0) for rows in range(1, 1 << 22))
    length = chain_length(spec, t)
    assert spec['inverse'] or frames_of_length(length, spec['n'], spec['hop'], spec['center']) == t
    bins = spec['n'] // 2 + 1 if spec['onesided'] else spec['n']
    out = rows * t * bins * (2 if spec['power'] is None else 1)
    if 'tac_overlap_add_f32' in spec['launches'] or spec['inverse']:     # frame gradients, the frames of the general inverse
        out = max(out, rows * t * (spec['n'] + 2))
    case = dict(spec, chain=True, rule=TWO_ROUNDS, form=form, rows=rows, n_frames=t, length=length,
                floats=max(out, rows * length) * (2 if spec['f64'] else 1))
    if spec['grid'][0] == 'ola':                    # the same bits only where the base rows alone are cut into the same segments
        waves = ola_form(spec['n'], spec['hop'], spec['grid'][3])[0]
        case['same_kernel'] = ola_plan(cus, rows, t, spec['n'], spec['hop'], waves) == ola_plan(cus, BASE_ROWS, t, spec['n'], spec['hop'], waves)
    return case


def chain_shapes(cus):
    """{name: case} of the STFT-chain kernels (a part of ``shapes``)"""
    out = {}
    for name, spec in CHAIN_SPECS.items():
        for form in spec['forms']:
            out['%s, %s rows' % (name, form)] = _chain_case(cus, spec, form)
    # tac_magphase_f64: the grid-stride element kernel of the float64 chain, on the complex rows of 'f64 2048, long rows'
    c = out['f64 2048, long rows']
    out['f64 magphase'] = dict(chain=True, family=9, entry='tac_magphase_f64', rule=ELEMENTS_2, of='f64 2048, long rows',
                               elements=c['rows'] * c['n_frames'] * (c['n'] // 2 + 1), floats=c['floats'])
    return out


# ----------------------------------------------------------------------------- the shapes
def _two_rounds_rows(grid, per_row=1):
    """fewest rows of ``per_row`` units each with more than two rounds of ``grid`` (an even number): an odd number of units where
    ``per_row`` is odd"""
    rows = 2 * grid // per_row + 1
    return rows + 1 if per_row % 2 == 1 and rows % 2 == 0 else rows


def _resample_case(cus, orig, new, adjoint=False):
    """five base rows whose OUTPUT is three tiles and a remainder (tests/test_resample_gpu.py's longest length) at the tile the
    forward bank takes; the gradient runs the adjoint bank from that output back to the input, whose tiles — of the adjoint bank's
    size — then count: at least three of those and a remainder too.  The grid is the real one: ``per_cu`` of the bank that runs."""
    tile, per_cu = polyphase_form(orig, new, adjoint)
    length = 3 * polyphase_form(orig, new)[0] * orig // new + orig // 2 + 5
    if adjoint:
        length = max(length, 3 * tile + orig // 2 + 5)
    n_out = RS.out_length(length, orig, new)
    per_row = ceil_div(length if adjoint else n_out, tile)
    rows = _two_rounds_rows(per_cu * cus, per_row)
    return dict(entry='tac_polyphase_f32', rule=TWO_ROUNDS, orig=orig, new=new, length=length, n_out=n_out, rows=rows,
                adjoint=adjoint, tile=tile, per_cu=per_cu, floats=rows * (max(length, n_out) + 3))


def _dct_case(cus, n_in, n_out, rows, gradient=False):
    """``rows`` 1: one row of two rounds of tiles, five more and one frame; 3: rows the launcher cannot merge, an odd number of
    tiles each (the last one of one frame) so that the three together leave an odd remainder.  The gradient multiplies by the
    transposed matrix: n_out -> n_in on the same frames."""
    k_in, k_out = (n_out, n_in) if gradient else (n_in, n_out)
    tile, nbytes = dct_tile(k_in, k_out)
    grid = min(8, DCT_LDS_BYTES // nbytes) * cus
    if rows == 1:
        tiles = 2 * grid + 5
    else:
        tiles = _two_rounds_rows(grid, 1) // rows + 1
        tiles += 1 - tiles % 2
    n_frames = (tiles - 1) * tile + 1
    return dict(entry='tac_dct_rows_f32', rule=TWO_ROUNDS, n_in=n_in, n_out=n_out, rows=rows, n_frames=n_frames, gradient=gradient,
                floats=rows * (n_frames + 1) * (max(n_in, n_out) + 3))


def _mac_case(cus, parts, rule):
    rows, n_bins = 7, 67
    per_tile = rows * ceil_div(n_bins, 64)
    need = (2 * 8 * cus + 1) if rule == TWO_ROUNDS else ceil_div(5 * 8 * cus, 4)     # workgroups
    tiles = ceil_div((need - 1) * MAC_WAVES + 1, per_tile)
    while rule == TWO_ROUNDS and ceil_div(tiles * per_tile, MAC_WAVES) % 2 == 0:      # (2 grid is even: an odd remainder)
        tiles += 1
    n_frames = (tiles - 1) * mac_tile(parts) + 1
    return dict(entry='tac_spectral_mac_f32', rule=rule, parts=parts, rows=rows, n_bins=n_bins, n_frames=n_frames, h_rows=3,
                floats=rows * n_frames * n_bins * 2)


def shapes(cus):
    """{name: case}: the sizes of every launch tests/test_grid_wrap_gpu.py makes on a device of ``cus`` compute units.  ``floats``
    is the largest tensor of the case, in float32 elements."""
    out = {}
    # 1. lfilter: a row is a unit; two tiles per row, the second one short — or full: only then does the last lane's chunk hold
    # samples of the row, and the carry (its state, its last two inputs) that the row leaves behind in the LDS is not zero
    rows = 2 * (2 * cus) + BASE_ROWS
    for tag, length in (('16-byte loads', LFILTER_TILE + 36), ('float loads', LFILTER_TILE + 37), ('full last tile', 2 * LFILTER_TILE)):
        out['lfilter, ' + tag] = dict(entry='tac_lfilter_f32', rule=TWO_ROUNDS, rows=rows, length=length, floats=rows * (length + 1))
    # 2. resample
    # 2. resample: 1024 outputs per tile; 12:1 takes 512 and 16:1 256 (2 - 3 times the LDS per workgroup: fewer per CU), and the
    # gradient of 1:12 runs the bank of 12:1
    for orig, new in ((2, 1), (3, 2), (160, 441), (12, 1), (16, 1)):
        out['resample %d:%d' % (orig, new)] = _resample_case(cus, orig, new)
    out['resample 3:2 gradient'] = _resample_case(cus, 3, 2, adjoint=True)
    out['resample 1:12 gradient'] = _resample_case(cus, 1, 12, adjoint=True)
    # 3. dct
    for n_in, n_out in ((40, 13), (256, 128)):
        for rows in (1, 3):
            out['dct %d x %d, %d row%s' % (n_in, n_out, rows, 's' * (rows > 1))] = _dct_case(cus, n_in, n_out, rows)
    out['dct 40 x 13 gradient'] = _dct_case(cus, 40, 13, 1, gradient=True)
    # 4. the delay line of fftconvolve
    for parts in (4, 8, 16):
        out['mac P %d' % parts] = _mac_case(cus, parts, TWO_ROUNDS)
    out['mac P 17'] = _mac_case(cus, 17, STREAMED)
    # 5. fftconvolve: the padded copy and the kept halves of one shared kernel, the partitions of per-row kernels
    l_in, m, n_fft = 10000, 3000, 2048
    elements = 2 * 256 * 8 * cus
    rows = elements // min(l_in + m - 1, fc_plan(l_in, m, n_fft)[1]) + 1
    out['fftconvolve shared'] = dict(entry='tac_fftconvolve_f32', rule=ELEMENTS_2, rows=rows, l_in=l_in, m=m, n_fft=n_fft,
                                     floats=rows * 2 * fc_plan(l_in, m, n_fft)[0] * (n_fft + 2))
    h_rows = elements // (ceil_div(m, n_fft // 2) * n_fft) + 1
    out['fftconvolve per-row'] = dict(entry='tac_fftconvolve_spectra_f32', rule=ELEMENTS_2, rows=h_rows, l_in=3000, m=m, n_fft=n_fft,
                                      floats=h_rows * ceil_div(m, n_fft // 2) * (n_fft + 2))
    # 7. hpss gradient: 3 x 600 x (1200 on a 256-CU part)
    n_freqs = 600
    n_frames = 100 * (2 * 256 * 16 * cus // (3 * n_freqs * 100) + 1)
    out['hpss gradient'] = dict(entry='tac_hpss_backward_f32', rule=ELEMENTS_2, rows=3, n_freqs=n_freqs, n_frames=n_frames,
                                floats=3 * n_freqs * n_frames)
    # 8. istft gradient: 2048 / 512, 140 frames, (8 rows on a 256-CU part)
    n_fft, hop, n_frames = 2048, 512, 140
    rows = 256 * 8 * cus // min(hop * (n_frames - 1) + n_fft, n_frames * (n_fft // 2 + 1)) + 1
    out['istft gradient'] = dict(entry='tac_istft_grad_input_f32', rule=ELEMENTS_1, rows=rows, n_fft=n_fft, hop=hop, n_frames=n_frames,
                                 floats=rows * n_frames * (n_fft + 2))
    # 9. the STFT chain
    out.update(chain_shapes(cus))
    return out


def launches_of(cus, c):
    """[(work, grid)] of the launches of case ``c`` that the case is about"""
    e = c['entry']
    if c.get('chain'):
        if e == 'tac_magphase_f64':
            return [ew_f64_launch(cus, c['elements'])]
        return [chain_launch(cus, c['grid'], c['rows'], c['n_frames'])]
    if e == 'tac_lfilter_f32':
        return [lfilter_launch(cus, c['rows'])]
    if e == 'tac_polyphase_f32':
        return [polyphase_launch(cus, c['rows'], c['length'] if c['adjoint'] else c['n_out'], c['tile'], c['per_cu'])]
    if e == 'tac_dct_rows_f32':
        k_in, k_out = (c['n_out'], c['n_in']) if c['gradient'] else (c['n_in'], c['n_out'])
        return [dct_launch(cus, c['rows'], c['n_frames'], k_in, k_out)]
    if e == 'tac_spectral_mac_f32':
        return [mac_launch(cus, c['rows'], c['n_frames'], c['n_bins'], c['parts'])]
    if e == 'tac_fftconvolve_f32':
        return [fc_pad_launch(cus, c['rows'], c['l_in'], c['m'], c['n_fft']), fc_keep_launch(cus, c['rows'], c['l_in'], c['m'], c['n_fft'])]
    if e == 'tac_fftconvolve_spectra_f32':
        return [fc_kernel_blocks_launch(cus, c['rows'], c['m'], c['n_fft'])]
    if e == 'tac_hpss_backward_f32':
        return [hpss_backward_launch(cus, c['rows'], c['n_freqs'], c['n_frames'])]
    if e == 'tac_istft_grad_input_f32':
        return [istft_grad_input_launch(cus, c['rows'], c['n_frames'], c['n_fft'], c['hop']),
                istft_grad_bins_launch(cus, c['rows'], c['n_frames'], c['n_fft'])]
    raise KeyError(e)


def can_be_odd(c):
    """False where every row is an even number of units and the remainder over two rounds is even with it"""
    if c['entry'] == 'tac_polyphase_f32':
        return ceil_div(c['length'] if c['adjoint'] else c['n_out'], c['tile']) % 2 == 1
    return True


def assert_wraps(cus, name, c):
    """every launch of the case runs its workgroups' loop as often as the case's rule says; returns the largest work / grid"""
    worst = 0.0
    for work, grid in launches_of(cus, c):
        what = '%s on %d CUs: %d workgroups of work on a grid of %d' % (name, cus, work, grid)
        if c['rule'] == TWO_ROUNDS:
            r = work - 2 * grid
            assert 0 < r < grid, what + ': not two rounds and a part of a third'
            assert r % 2 == 1 or not can_be_odd(c), what + ': an even remainder'
        elif c['rule'] == STREAMED:
            assert 4 * work >= 5 * grid, what + ': less than 1.25 rounds'
        elif c['rule'] == ELEMENTS_2:
            assert work > 2 * grid, what + ': no more than two rounds'
        else:
            assert c['rule'] == ELEMENTS_1 and work > grid, what + ': no second round'
        worst = max(worst, work / grid)
    for also in c.get('also', ()):                                                 # the case's other kernels
        if also[0] == 'overlap-add':                                               # (the gather overlap-add: to ELEMENTS_2)
            work, grid = overlap_add_launch(cus, c['rows'], c['length'])
            assert work > 2 * grid, '%s on %d CUs: the overlap-add has no more than two rounds' % (name, cus)
        else:
            work, grid = (fb_adjoint_launch(cus, c['rows'] * c['n_frames']) if also[0] == 'fb_adjoint' else
                          chain_launch(cus, also[1:], c['rows'], c['n_frames']))
            assert work > grid, '%s on %d CUs: %s, %d workgroups of work on a grid of %d: no second round' % (name, cus, also[0], work, grid)
    if c.get('chain') and c.get('grid', ('',))[0] == 'generic':                    # the 8-wave form, by the launcher's own condition
        groups, waves, per_cu = generic_form(cus, c['rows'], c['n_frames'], c['grid'][1], c['grid'][2])
        assert groups >= 2 * STFT_WAVES * cus and (waves, per_cu) == (2 * STFT_WAVES, 1), '%s on %d CUs: not the wide form' % (name, cus)
    assert 4 * c['floats'] < MAX_TENSOR_BYTES, '%s on %d CUs: a tensor of %d bytes' % (name, cus, 4 * c['floats'])
    assert math.gcd(BASE_ROWS, 8 * cus) == 1 and math.gcd(BASE_FRAMES, 8 * cus) == 1
    return worst
