"""Shared by tests/test_polyphase_rules_cpu.py and the GPU files of the two polyphase kernels (a plain module: no tests in here):
which instantiation ``tac_polyphase_f32`` and ``tac_polyphase_wide_f32`` (csrc/resample.hip) launch for a bank, restated from the
launchers next to their verbatim lines as tests/grid_rules.py does for the grids; the case tables the GPU tests walk; and the
generator of the seeded sweeps.

* ``lds_variant(bank, vec)`` -> ``(tile, P1, SKEW, VEC, per_cu)``: 3 x 2 x 2 x 2 instantiations ``polyphase_kernel<P1, SKEW, VEC>`` at
  1024 / 512 / 256 outputs per tile.  ``wide_variant(bank, vec)`` -> ``(tile, KB, VEC, per_cu)``: 3 x 4 x 2 of
  ``polyphase_wide_kernel<KB, VEC>``, the tile from the host plan ``_hip.resample_wide_plan``.  None where the launcher refuses.
* ``geometry(orig, new, lpw, rolloff)``: phases, step, K, off and run of the forward and of the adjoint bank from the definition in
  numpy, without the taps — what the variant depends on (the window changes no tap's support, so neither method nor beta counts).
  tests/test_polyphase_rules_cpu.py holds it to the product's banks.
* ``census()`` searches ``LDS_GRID`` and ``WIDE_GRID`` below for the variants that public arguments reach, the forward and the
  adjoint bank counted separately; the tables must reach every one of them.

What the census finds unreachable (tests/test_polyphase_rules_cpu.py asserts exactly this list, on the grids below):

* wide ``(tile 256, KB 16)``, both VEC, forward and adjoint: a tile of 256 is taken only where 512 outputs' span exceeds 8192
  floats, i.e. a step / phases ratio above ~16, and a phase then has at least ``2 ratio lpw / rolloff - 1 >= 31`` taps.
  (``(512, 16)`` and ``(256, 32)`` are reached only at ``rolloff = 1.0`` and ``lowpass_filter_width = 1``: 8:1 has 15 taps, 16:1 has 31.)
* every other one of the 24 + 24 instantiations is reached by both banks.
"""
import collections
import math

import numpy as np

import resample_rules as R

LDS_ENTRY, WIDE_ENTRY = 'tac_polyphase_f32', 'tac_polyphase_wide_f32'
Geometry = collections.namedtuple('Geometry', 'phases step K off run')


# ----------------------------------------------------------------------------- the banks' geometry
def geometries(orig, new, lpw=6, rolloff=0.99):
    """``(forward, adjoint)`` ``Geometry`` of the compact bank of reduced rates ``orig -> new`` (tests/resample_rules.py's
    definition: the ``d`` in ``[-width, width + orig)`` with ``|t| < lpw``) and of its transpose: tap ``(p, d)`` lands at
    ``q = d mod orig``, ``e = p - floor(d / orig) * new``."""
    base, width, _ = R.filter_constants(orig, new, lpw, rolloff)
    p = np.arange(new, dtype=np.float64)[:, None]
    reach = width + 2
    first = np.floor(p * orig / new).astype(np.int64) - reach
    d = first + np.arange(2 * reach + 2, dtype=np.int64)[None, :]
    t = base * (d.astype(np.float64) / orig - p / new)
    valid = (np.abs(t) < lpw) & (d >= -width) & (d < width + orig)
    run = valid.sum(axis=1)
    off = d[np.arange(new), valid.argmax(axis=1)]
    forward = Geometry(new, orig, max(int(run.max()), 1), off.tolist(), run.tolist())
    pp = np.broadcast_to(np.arange(new, dtype=np.int64)[:, None], d.shape)[valid]
    dd = d[valid]
    block = dd // orig
    q, e = dd - block * orig, pp - block * new
    order = np.argsort(q, kind='stable')
    q, e = q[order], e[order]
    lo, hi, run = np.zeros(orig, dtype=np.int64), np.zeros(orig, dtype=np.int64), np.zeros(orig, dtype=np.int64)
    if len(q):
        starts = np.flatnonzero(np.r_[True, q[1:] != q[:-1]])
        seen = q[starts]
        lo[seen] = np.minimum.reduceat(e, starts)
        hi[seen] = np.maximum.reduceat(e, starts)
        run[seen] = hi[seen] - lo[seen] + 1
    return forward, Geometry(orig, new, max(int(run.max()), 1), lo.tolist(), run.tolist())


def geometry(orig, new, lpw=6, rolloff=0.99, adjoint=False):
    return geometries(orig, new, lpw, rolloff)[1 if adjoint else 0]


def taps_estimate(orig, new, lpw, rolloff):
    """a lower bound of K of either bank's longer side: an open interval of length ``2 lpw max(orig, new) / base`` holds at least
    that many integers minus one"""
    return int(2.0 * lpw * max(orig, new) / (min(orig, new) * rolloff)) - 1


# ----------------------------------------------------------------------------- tac_polyphase_f32
LDS = ('resample.hip', (
    'constexpr int RS_THREADS = 256;',
    'constexpr int RESAMPLE_MAX_BANK = 20480;',
    'constexpr int RESAMPLE_MAX_PHASES = 2048;',
    'constexpr int RS_SPAN_WIDE = 8192;',
    'constexpr int RS_SPAN_MAX = 14336;',
    'constexpr int RS_LDS_BYTES = 160 * 1024;',
    'const long long j_span = ((long long)P - 1 + (1LL << tile_log) - 1) / P;',
    'const long long span = 3 + j_span * S + ((long long)off_max - off_min) + K;',
    'return (span + 3) & ~3LL;',
    'if (phases > RESAMPLE_MAX_PHASES || (long long)phases * taps > RESAMPLE_MAX_BANK) return TAC_E_UNSUPPORTED;',
    'for (int t = 10; t >= 8 && tile_log < 0; --t) {',
    'cap = rs_span_cap(phases, taps, step, off_min, off_max, t);',
    'if (cap <= (t == 8 ? RS_SPAN_MAX : RS_SPAN_WIDE)) tile_log = t;',
    'if (tile_log < 0) return TAC_E_UNSUPPORTED;',
    'const bool p1 = phases == 1;',
    'const bool skew = (step & 1) == 0;',
    'const size_t bytes = 4 * ((size_t)(p1 ? 0 : phases * taps) + 2 * (size_t)phases + (size_t)(cap + (cap >> 5) + 1));',
    'if (bytes > (size_t)RS_LDS_BYTES) return TAC_E_UNSUPPORTED;',
    'long long per_cu = (long long)(RS_LDS_BYTES / bytes);',
    'per_cu = per_cu > 8 ? 8 : per_cu;',
    'const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (stride_r & 3) == 0;',
    'auto kern = p1 ? (skew ? rs_pick<true, true>(vec) : rs_pick<true, false>(vec))',
    ': (skew ? rs_pick<false, true>(vec) : rs_pick<false, false>(vec));',
))
RESAMPLE_MAX_BANK, RESAMPLE_MAX_PHASES = 20480, 2048
RS_SPAN_WIDE, RS_SPAN_MAX = 8192, 14336
RS_LDS_BYTES = 160 * 1024
TILES = (1024, 512, 256)


def rs_span_cap(phases, taps, step, off_min, off_max, tile_log):
    j_span = (phases - 1 + (1 << tile_log) - 1) // phases
    span = 3 + j_span * step + (off_max - off_min) + taps
    return (span + 3) & ~3


def lds_variant(b, vec):
    """``(tile, P1, SKEW, VEC, per_cu)`` of the launch of bank ``b`` (anything with phases, step, K, off), None where refused"""
    if b.phases > RESAMPLE_MAX_PHASES or b.phases * b.K > RESAMPLE_MAX_BANK:
        return None
    off_min, off_max = min(b.off), max(b.off)
    tile_log, cap = -1, 0
    for t in (10, 9, 8):
        if tile_log < 0:
            cap = rs_span_cap(b.phases, b.K, b.step, off_min, off_max, t)
            if cap <= (RS_SPAN_MAX if t == 8 else RS_SPAN_WIDE):
                tile_log = t
    if tile_log < 0:
        return None
    p1 = b.phases == 1
    skew = (b.step & 1) == 0
    nbytes = 4 * ((0 if p1 else b.phases * b.K) + 2 * b.phases + (cap + (cap >> 5) + 1))
    if nbytes > RS_LDS_BYTES:
        return None
    return 1 << tile_log, p1, skew, bool(vec), min(8, RS_LDS_BYTES // nbytes)


# ----------------------------------------------------------------------------- tac_polyphase_wide_f32
WIDE = ('resample.hip', (
    'constexpr int RSW_ROWS = 4;',
    'constexpr int RSW_MAX_TAPS = 64;',
    'constexpr long long RSW_MAX_BANK = 1LL << 20;',
    'constexpr int RSW_SPAN_MAX = 8192;',
    'if (taps > RSW_MAX_TAPS || (long long)phases * taps > RSW_MAX_BANK || span > RSW_SPAN_MAX) return TAC_E_UNSUPPORTED;',
    'const int tile_log = tile == 1024 ? 10 : (tile == 512 ? 9 : 8);',
    'const int pitch = (3 + span + taps + 3) & ~3;',
    'const size_t bytes = 4 * (size_t)RSW_ROWS * (size_t)pitch;',
    'if (bytes > (size_t)RS_LDS_BYTES) return TAC_E_UNSUPPORTED;',
    'long long per_cu = (long long)(RS_LDS_BYTES / bytes);',
    'per_cu = per_cu > 8 ? 8 : per_cu;',
    'auto kern = taps <= 16 ? rsw_pick<16>(vec) : (taps <= 32 ? rsw_pick<32>(vec) : (taps <= 48 ? rsw_pick<48>(vec)',
    ': rsw_pick<64>(vec)));',
))
RSW_ROWS, RSW_MAX_TAPS, RSW_MAX_BANK, RSW_SPAN_MAX = 4, 64, 1 << 20, 8192
BUCKETS = (16, 32, 48, 64)


def wide_variant(b, vec):
    """``(tile, KB, VEC, per_cu)`` of the wide launch of bank ``b`` (anything with phases, step, K, off, run) with the plan of
    ``_hip.resample_wide_plan``; None where there is no plan or the launcher refuses"""
    import torchaudio_contrib_amd as tac
    taps = b.K
    if taps > RSW_MAX_TAPS or b.phases * taps > RSW_MAX_BANK:
        return None
    plan = tac._hip.resample_wide_plan(b)
    if plan is None:
        return None
    span, tile = plan
    if taps > RSW_MAX_TAPS or b.phases * taps > RSW_MAX_BANK or span > RSW_SPAN_MAX or tile not in TILES:
        return None
    pitch = (3 + span + taps + 3) & ~3
    nbytes = 4 * RSW_ROWS * pitch
    if nbytes > RS_LDS_BYTES:
        return None
    kb = 16 if taps <= 16 else (32 if taps <= 32 else (48 if taps <= 48 else 64))
    return tile, kb, bool(vec), min(8, RS_LDS_BYTES // nbytes)


QUOTED = (LDS, WIDE)

# ----------------------------------------------------------------------------- the case tables of the GPU tests
HANN, WIDE_FILTER, KAISER = dict(), dict(lpw=16, rolloff=0.9), dict(method='sinc_interp_kaiser')
NARROW_FILTER = dict(lpw=10, rolloff=0.9)
# tests/test_resample_gpu.py, test_kernel_within_the_bound: (orig, new, filter).  Every layout of the file runs each case, so each
# stands for both VEC settings.  The first twelve take 1024 outputs per tile; then 512 (9:1 .. 441:40) and 256 (16:1 .. 48:1, the
# longest bank the kernel holds), with and without P1 and SKEW; a Kaiser window and a non-default width / rolloff on a narrow tile.
LDS_CASES = [(2, 1, HANN), (1, 2, HANN), (3, 1, HANN), (3, 2, HANN), (2, 3, HANN), (7, 5, HANN), (147, 160, HANN), (441, 160, HANN),
             (160, 441, HANN), (3, 2, WIDE_FILTER), (3, 2, KAISER), (441, 160, KAISER),
             (9, 1, HANN), (12, 1, HANN), (25, 2, HANN), (34, 3, HANN), (441, 40, HANN),
             (16, 1, HANN), (17, 1, HANN), (33, 2, HANN), (50, 3, HANN), (48, 1, HANN),
             (12, 1, KAISER), (8, 1, NARROW_FILTER)]
# test_gradient_is_the_kernel_with_the_adjoint_bank: the adjoint bank of b:a has the geometry of the forward bank of a:b, so the
# upsampling pairs put the gradient on the narrow tiles (their forward stays on 1024); 12:1 has the narrow forward
LDS_GRADIENT_CASES = [(3, 1, HANN), (2, 3, HANN), (441, 160, HANN), (1, 2, HANN), (1, 3, HANN), (3, 2, HANN),
                      (1, 12, HANN), (2, 25, HANN), (1, 9, HANN), (3, 34, HANN),
                      (1, 16, HANN), (3, 50, HANN), (1, 17, HANN), (2, 33, HANN), (12, 1, HANN)]
# tests/test_pitch_shift_gpu.py, test_wide_variants_within_the_bound: (orig, new, filter), forward AND gradient of each (the
# layouts of the file give both VEC settings).  Bucket 64 (K = 49, 61); the bucket edges K = 16 | 17, 32 | 33, 48 | 49 and 63, the
# last K but one the kernel takes; tile 512 (K = 25, 49, 37) and 256 (K = 41, 61); the flipped pairs put the same banks on the
# gradient; 8:1 and 16:1 at width 1, rolloff 1.0 are the only way to (512, 16) and (256, 32)
SHORT = dict(lpw=1, rolloff=1.0)
WIDE_CASES = [(4001, 1000, HANN), (5001, 1000, HANN), (2000, 2001, HANN),
              (2001, 2000, dict(lpw=8)), (2001, 2000, dict(lpw=16)), (2001, 2000, dict(lpw=24)), (2001, 2000, dict(lpw=31)),
              (12001, 1000, dict(lpw=1)), (12001, 1000, dict(lpw=2)), (9001, 1000, dict(lpw=2)),
              (20001, 1000, dict(lpw=1)), (30001, 1000, dict(lpw=1)),
              (1000, 4001, HANN), (1000, 12001, dict(lpw=1)), (1000, 9001, dict(lpw=2)), (1000, 12001, dict(lpw=2)),
              (1000, 20001, dict(lpw=1)), (1000, 30001, dict(lpw=1)),
              (8, 1, SHORT), (1, 8, SHORT), (16, 1, SHORT), (1, 16, SHORT)]
# the cases tests/test_pitch_shift_gpu.py had before (their table stays there): K = 13, 15, 16, 34 on tile 1024
WIDE_CASES_1024 = [(2000, 2001, HANN), (2001, 2000, HANN), (1873, 1575, HANN), (10079, 8000, HANN), (16000, 44101, HANN),
                   (44101, 16000, HANN), (1873, 1575, KAISER)]


#: outputs per tile of the FORWARD bank of a reduced pair at the default filter, where it is not 1024 (what the GPU tests pin by
#: pair; tests/test_polyphase_rules_cpu.py holds it to the rule).  The adjoint bank of b:a has the geometry of the forward of a:b.
NARROW_TILES = {(9, 1): 512, (12, 1): 512, (25, 2): 512, (34, 3): 512, (441, 40): 512,
                (16, 1): 256, (17, 1): 256, (33, 2): 256, (50, 3): 256, (48, 1): 256}


def pinned_tile(orig, new, adjoint=False):
    return NARROW_TILES.get((new, orig) if adjoint else (orig, new), 1024)


def case_id(c):
    return '%d:%d%s' % (c[0], c[1], ''.join('-%s' % v for v in c[2].values()))


def case_geometry(c, adjoint=False):
    return geometry(c[0], c[1], c[2].get('lpw', 6), c[2].get('rolloff', 0.99), adjoint=adjoint)


def lds_covers(c):
    return lds_variant(case_geometry(c), True) is not None and lds_variant(case_geometry(c, True), True) is not None


def wide_covers(c):
    return wide_variant(case_geometry(c), True) is not None and wide_variant(case_geometry(c, True), True) is not None


def reached_by_tables():
    """{(kernel, 'forward' | 'adjoint'): set of variants without per_cu} of the launches the tables above stand for.  Both VEC
    settings of every case, forward and gradient: the GPU tests hand each case, at each length, layouts that force either load
    form whatever the length (``layout_pad``: a row stride rounded up to four floats; a start one float into the allocation) —
    the input for the forward, grad_out for the gradient — and assert that both ran."""
    out = collections.defaultdict(set)
    for vec in (True, False):
        for c in LDS_CASES:
            out[LDS_ENTRY, 'forward'].add(lds_variant(case_geometry(c), vec)[:4])
        for c in LDS_GRADIENT_CASES:
            out[LDS_ENTRY, 'adjoint'].add(lds_variant(case_geometry(c, True), vec)[:4])
        for c in WIDE_CASES + WIDE_CASES_1024:
            out[WIDE_ENTRY, 'forward'].add(wide_variant(case_geometry(c), vec)[:3])
            out[WIDE_ENTRY, 'adjoint'].add(wide_variant(case_geometry(c, True), vec)[:3])
    return dict(out)


# ----------------------------------------------------------------------------- the census
#: the grid of public arguments the census searches.  Reduced pairs: every coprime a:b with a, b <= 12; every coprime a:b and b:a
#: with a <= 64, b <= 4 (the integer ratios among them: 48:1 is the last the LDS kernel covers); every pair of the eleven sample
#: rates _hip.py names; for the wide kernel also (1000 k + 1):1000 and back for k <= 32 and 2001:2000 and back, the shapes of
#: pitch_shift and speed.  Every lowpass_filter_width 1 .. 32 at the rolloffs below.  Both methods: the support of a tap is
#: ``|t| < lpw`` whatever the window, so the geometry is evaluated once and tests/test_polyphase_rules_cpu.py holds the product's
#: Kaiser banks to it.  A variant counts as reached where the public entry runs it: where the kernel covers BOTH banks of the pair.
RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)
WIDTHS = tuple(range(1, 33))
ROLLOFFS = (0.5, 0.99, 1.0)
METHODS = ('sinc_interp_hann', 'sinc_interp_kaiser')


def _pairs(wide):
    pairs = set()
    for a in range(1, 65):
        for b in range(1, 13 if a <= 12 else 5):
            if a != b and math.gcd(a, b) == 1:
                pairs.update(((a, b), (b, a)))
    for a in RATES:
        for b in RATES:
            if a != b:
                pairs.add(R.reduced(a, b))
    if wide:
        for k in range(1, 33):
            pairs.update(((1000 * k + 1, 1000), (1000, 1000 * k + 1)))
        pairs.update(((2001, 2000), (2000, 2001)))
    return sorted(pairs)


LDS_GRID, WIDE_GRID = _pairs(False), _pairs(True)


def census(kernel, check=None):
    """{'forward' | 'adjoint': {variant without per_cu: first (orig, new, lpw, rolloff) that reaches it}} over the kernel's grid.
    Pairs certain to be refused for their taps alone (``taps_estimate``) are not formed.  ``check(geometry, variant)`` is called
    for every bank that is."""
    lds = kernel == LDS_ENTRY
    rule = lds_variant if lds else wide_variant
    found = dict(forward={}, adjoint={})
    for orig, new in (LDS_GRID if lds else WIDE_GRID):
        for rolloff in ROLLOFFS:
            for lpw in WIDTHS:
                k_low = taps_estimate(orig, new, lpw, rolloff)
                if (k_low * min(orig, new) > RESAMPLE_MAX_BANK or k_low > RS_SPAN_MAX) if lds else k_low > RSW_MAX_TAPS:
                    break                                       # (and every wider filter of the pair with it)
                sides = geometries(orig, new, lpw, rolloff)
                variants = [rule(g, True) for g in sides]
                if check is not None:
                    for g, v in zip(sides, variants):
                        check(g, v)
                if variants[0] is None or variants[1] is None:
                    continue
                for side, g, v in zip(('forward', 'adjoint'), sides, variants):
                    for vec in (True, False):
                        found[side].setdefault(v[:-2] + (vec,), (orig, new, lpw, rolloff))
    return found


# ----------------------------------------------------------------------------- the sweeps
#: per (tile, P1, SKEW) of the LDS kernel and per (tile, KB) of the wide one: down-sampling pairs a:b whose FORWARD bank takes it
#: for some width and rolloff of the draw; b:a puts the same bank on the gradient
LDS_POOLS = {
    (1024, True, True): [(2, 1), (4, 1), (6, 1)], (1024, True, False): [(3, 1), (5, 1), (7, 1)],
    (1024, False, True): [(4, 3), (8, 3), (10, 7), (6, 5)], (1024, False, False): [(3, 2), (5, 3), (7, 5), (7, 2)],
    (512, True, True): [(10, 1), (12, 1)], (512, True, False): [(9, 1), (11, 1), (13, 1)],
    (512, False, True): [(34, 3), (28, 3), (32, 3), (52, 5)], (512, False, False): [(25, 2), (19, 2), (21, 2), (29, 3)],
    (256, True, True): [(18, 1), (20, 1), (24, 1)], (256, True, False): [(17, 1), (19, 1), (21, 1)],
    (256, False, True): [(50, 3), (56, 3), (52, 3)], (256, False, False): [(33, 2), (35, 2), (37, 2), (55, 3)],
}
WIDE_POOLS = {
    (1024, 16): [(2001, 2000), (1501, 1000), (3, 2)], (1024, 32): [(2001, 2000), (2001, 1000), (5, 3)],
    (1024, 48): [(2001, 2000), (4001, 1000), (3001, 1000)], (1024, 64): [(2001, 2000), (5001, 1000), (4001, 1000)],
    (512, 16): [(8, 1)], (512, 32): [(12001, 1000), (9, 1), (10001, 1000)], (512, 48): [(9001, 1000), (11, 1), (12001, 1000)],
    (512, 64): [(12001, 1000), (9001, 1000), (14001, 1000)],
    (256, 32): [(16, 1)], (256, 48): [(20001, 1000), (17, 1), (18001, 1000)], (256, 64): [(30001, 1000), (20001, 1000), (24001, 1000)],
}
#: by VEC.  'aligned': rows ``(-length) % 4`` floats apart (dense where the length allows); 'aligned, padded': four more;
#: 'odd stride': rows 3 floats apart, 1 where that makes the stride a multiple of four; 'misaligned': dense, one float into
#: its allocation
LAYOUTS = {True: ('aligned', 'aligned, padded'), False: ('odd stride', 'misaligned')}


def layout_pad(layout, length):
    """floats between the end of a row and the start of the next"""
    if layout in ('aligned', 'aligned, padded'):
        return (-length) % 4 + (4 if layout == 'aligned, padded' else 0)
    assert layout == 'odd stride'
    return 3 if (length + 3) % 4 else 1


SweepCase = collections.namedtuple('SweepCase', 'kernel orig new kw rows length out_len layout gradient variant seed')


def _draw_filter(rng, orig, new, lds, aim):
    """(lpw, rolloff, method, beta): rolloff in [0.5, 0.99], method and beta free; the width among those of 1 .. 32 whose estimated
    taps per phase ``2 lpw ratio / rolloff + 1`` the aim admits (the wide kernel's bucket of K, give or take two taps; the LDS
    kernel's bank limit) — this is the stratification, the launcher's own rule decides afterwards.  None where no width does."""
    method = METHODS[int(rng.integers(2))]
    beta = float(rng.uniform(4.0, 16.0)) if method == 'sinc_interp_kaiser' and rng.random() < 0.5 else None
    if not lds and aim in ((512, 16), (256, 32)):                # the two variants only lpw = 1, rolloff = 1.0 reaches
        return 1, 1.0, method, beta
    rolloff = float(rng.uniform(0.5, 0.99))
    ratio = max(orig, new) / float(min(orig, new))
    taps = [2.0 * w * ratio / rolloff + 1.0 for w in WIDTHS]
    if lds:
        widths = [w for w, k in zip(WIDTHS, taps) if k * min(orig, new) <= RESAMPLE_MAX_BANK and k <= 4096]
    else:
        widths = [w for w, k in zip(WIDTHS, taps) if aim[1] - 18 < k <= min(aim[1] + 2, RSW_MAX_TAPS)]
    if not widths:
        return None
    return widths[int(rng.integers(len(widths)))], rolloff, method, beta


def sweep(kernel, cases, seed):
    """``(cases, drawn, rejected)``: ``cases`` SweepCase of ``kernel``, case i aimed at reachable variant i mod their number — a
    pair from the variant's pool, forward or (flipped) gradient, then width, rolloff, method and beta drawn freely; a draw the
    kernel does not cover is REJECTED and counted; one it covers on another variant than the aim is drawn again.  Length: a
    random offset around 0 .. 3 tiles of the variant's own tile.  Forward or gradient is a coin per case: at the default count
    every reachable variant is launched by ONE of the two banks, not by each (that is the tables' part)."""
    lds = kernel == LDS_ENTRY
    rng = np.random.default_rng((20000 if lds else 30000) + seed)
    pools = LDS_POOLS if lds else WIDE_POOLS
    aims = [(k, vec) for k in sorted(pools, key=lambda k: (-k[0], k[1:])) for vec in (True, False)]
    out, drawn, rejected = [], 0, 0
    for i in range(cases):
        aim, vec = aims[i % len(aims)]
        for _ in range(200):
            a, b = pools[aim][int(rng.integers(len(pools[aim])))]
            gradient = bool(rng.random() < 0.5)
            orig, new = (b, a) if gradient else (a, b)
            filt = _draw_filter(rng, orig, new, lds, aim)
            if filt is None:
                continue
            lpw, rolloff, method, beta = filt
            drawn += 1
            c = (orig, new, dict(lpw=lpw, rolloff=rolloff))
            if not (lds_covers(c) if lds else wide_covers(c)):
                rejected += 1
                continue
            g = case_geometry(c, adjoint=gradient)
            v = lds_variant(g, vec) if lds else wide_variant(g, vec)
            if v[:-2] == aim:
                break
        else:
            raise AssertionError('no draw of %r reached %r' % (pools[aim], aim))
        tile = v[0]
        made = max(1, int(rng.integers(0, 4)) * tile + int(rng.integers(-9, 10)))      # outputs of the launch
        if gradient:
            length = made
        else:
            length = max(1, made * orig // new + int(rng.integers(0, 2)))
        n_out = R.out_length(length, orig, new)
        out_len = n_out if lds else max(1, n_out + int(rng.integers(-2, 3)) * int(rng.integers(1, 300)))
        if not lds and out_len == n_out and lds_covers(c):       # (resample_fit would take the LDS kernel: pad by at least one)
            out_len = n_out + int(rng.integers(1, 200))
        kw = dict(lpw=lpw, rolloff=rolloff, method=method)
        if beta is not None:
            kw['beta'] = beta
        rows = int(rng.integers(1, 7))
        layout = LAYOUTS[vec][int(rng.integers(2))]
        if rows == 1 and not vec:                                # (one row has no stride: only its start decides the loads)
            layout = 'misaligned'
        out.append(SweepCase(kernel, orig, new, kw, rows, length, out_len, layout, gradient, v,
                             int(rng.integers(1 << 30))))
    return out, drawn, rejected
