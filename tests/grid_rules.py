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
silently stopped wrapping.  Where ``per_cu`` depends on the LDS bytes of a bank (``tac_polyphase_f32``) the upper bound 8 is taken:
a smaller real grid only wraps more often.

``shapes(cus)`` gives every size tests/test_grid_wrap_gpu.py uses on a device of ``cus`` compute units; ``launches_of(cus, case)`` computes
``(work, grid)`` from those sizes and ``assert_wraps`` holds them to the case's rule (the GPU tests call it before they launch).  The
numbers of distinct base rows and frames (5 and 67) share no factor with a grid (a power of two times 1 or 19): the successive
units of one workgroup hold different data."""
import math

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
POLYPHASE_TILE = 1024                   # outputs per tile for every bank used here (the GPU tests assert it: _hip.resample_tile)
POLYPHASE_PER_CU = 8                    # the upper bound of per_cu


def polyphase_launch(cus, rows, l_out, tile=POLYPHASE_TILE):
    """a unit is a tile of ``tile`` outputs of one row"""
    return _launch(rows * ceil_div(l_out, tile), 1, POLYPHASE_PER_CU * cus)


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


QUOTED = (PERSISTENT_BLOCKS, LFILTER, POLYPHASE, DCT, MAC, FC, ISTFT_GRAD, HPSS_BACKWARD)


# ----------------------------------------------------------------------------- the shapes
def _two_rounds_rows(grid, per_row=1):
    """fewest rows of ``per_row`` units each with more than two rounds of ``grid`` (an even number): an odd number of units where
    ``per_row`` is odd"""
    rows = 2 * grid // per_row + 1
    return rows + 1 if per_row % 2 == 1 and rows % 2 == 0 else rows


def _resample_case(cus, orig, new, adjoint=False):
    """five base rows whose OUTPUT is three tiles and a remainder (tests/test_resample_gpu.py's longest length); the gradient runs
    the adjoint bank from that output back to the input, whose tiles then count"""
    length = 3 * POLYPHASE_TILE * orig // new + orig // 2 + 5
    n_out = RS.out_length(length, orig, new)
    per_row = ceil_div(length if adjoint else n_out, POLYPHASE_TILE)
    rows = _two_rounds_rows(POLYPHASE_PER_CU * cus, per_row)
    return dict(entry='tac_polyphase_f32', rule=TWO_ROUNDS, orig=orig, new=new, length=length, n_out=n_out, rows=rows,
                adjoint=adjoint, floats=rows * (max(length, n_out) + 3))


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
    for orig, new in ((2, 1), (3, 2), (160, 441)):
        out['resample %d:%d' % (orig, new)] = _resample_case(cus, orig, new)
    out['resample 3:2 gradient'] = _resample_case(cus, 3, 2, adjoint=True)
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
    return out


def launches_of(cus, c):
    """[(work, grid)] of the launches of case ``c`` that the case is about"""
    e = c['entry']
    if e == 'tac_lfilter_f32':
        return [lfilter_launch(cus, c['rows'])]
    if e == 'tac_polyphase_f32':
        return [polyphase_launch(cus, c['rows'], c['length'] if c['adjoint'] else c['n_out'])]
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
        return ceil_div(c['length'] if c['adjoint'] else c['n_out'], POLYPHASE_TILE) % 2 == 1
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
    assert 4 * c['floats'] < MAX_TENSOR_BYTES, '%s on %d CUs: a tensor of %d bytes' % (name, cus, 4 * c['floats'])
    assert math.gcd(BASE_ROWS, 8 * cus) == 1 and math.gcd(BASE_FRAMES, 8 * cus) == 1
    return worst
