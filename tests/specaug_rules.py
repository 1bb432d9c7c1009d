"""Shared by tests/test_specaug_cpu.py and tests/test_specaug_gpu.py (a plain module: no tests in here): what SpecAugment's masks are,
written from the definition and without the package.

``reference``   the op: a numpy loop over rows and spans with plain slicing.  Nothing is computed, so every comparison against it is
                bit for bit (``assert_same`` compares integer views: NaNs outside the masks count too).
``sequential``  torchaudio's ``mask_along_axis`` / ``mask_along_axis_iid`` as the definition states them — the two draws per mask, in
                order, and one ``masked_fill`` per mask — under ``torch.manual_seed(seed)``.
``SHAPES``, ``span_sets``   the cases of the op; ``QUOTED``, ``launch``, ``wrap_rows``   the grid of ``tac_mask_spans_f32`` restated
                from its launcher (tests/test_specaug_cpu.py looks the quoted expressions up in csrc/specaug.hip) and the row count at
                which every workgroup walks its loop more than twice."""
import numpy as np
import torch

MAX_SPANS = 64
#: (rows, A, B): one element; odd sizes under one unit; a Kaldi-sized row of 1001 frames (dword path, several B-chunks); many short
#: lines (the 16-lane segments, several A-blocks); a long row of 4096 + 5 (seventeen B-chunks)
SHAPES = ((1, 1, 1), (3, 23, 67), (2, 80, 1001), (5, 257, 3), (2, 4, 4096 + 5))


def reference(x, spans, k_a, fill):
    """``x`` (rows, A, B); ``spans`` integer (R, k, 2) with R 1 or rows, the first ``k_a`` along A, each ``[start, end)`` clamped to its
    axis, empty where ``end <= start``; returns the masked copy"""
    x = np.asarray(x)
    out = x.copy()
    spans = np.asarray(spans)
    spans = spans.reshape((-1, spans.shape[-2], 2)) if spans.size else np.zeros((1, 0, 2), np.int64)
    rows, n_a, n_b = x.shape
    fill = np.asarray(fill, dtype=x.dtype)
    for r in range(rows):
        table = spans[r if spans.shape[0] > 1 else 0]
        for s in range(table.shape[0]):
            n = n_a if s < k_a else n_b
            lo = min(max(int(table[s, 0]), 0), n)
            hi = min(max(int(table[s, 1]), 0), n)
            if hi <= lo:
                continue
            if s < k_a:
                out[r, lo:hi, :] = fill
            else:
                out[r, :, lo:hi] = fill
    return out


def masked(shape, spans, k_a):
    """boolean (rows, A, B): where ``reference`` writes the fill"""
    probe = reference(np.zeros(shape, np.float32), spans, k_a, 1.0)
    return probe != 0


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same(got, want, what):
    """bit for bit, NaN positions included"""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, '%s: shape %r, expected %r' % (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), '%s: %d of %d elements differ, the first at %r' % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def values(shape, seed):
    """float32 values none of which is a fill value used by the tests (all are in (1, 2))"""
    return (1.0 + np.random.default_rng(seed).random(shape)).astype(np.float32)


def span_sets(rows, n_a, n_b, seed):
    """[(name, spans int32 (R, k, 2), k_a)]: the identity, an empty span, the whole axis, overlapping spans, spans reaching outside
    the axis, span counts 1 .. 64 on either axis and both, shared and per-row tables"""
    rng = np.random.default_rng(seed)

    def draw(r, k, n):
        start = rng.integers(-3, n + 3, size=(r, k))
        return np.stack([start, start + rng.integers(-2, max(n // 3, 2) + 3, size=(r, k))], axis=-1)

    def both(r, k_a, k_b):
        return np.concatenate([draw(r, k_a, n_a), draw(r, k_b, n_b)], axis=1).astype(np.int32), k_a

    sets = [('no spans', np.zeros((1, 0, 2), np.int32), 0),
            ('an empty span on each axis', np.array([[[2, 2], [5, 1]]], np.int32), 1),
            ('the whole of A', np.array([[[0, n_a]]], np.int32), 1),
            ('the whole of B', np.array([[[0, n_b]]], np.int32), 0),
            ('overlapping', np.array([[[0, 2], [1, 3], [n_b // 4, n_b // 2 + 1], [n_b // 3, n_b // 2 + 2], [n_b // 3, n_b // 3 + 1]]], np.int32), 2),
            ('outside the axes', np.array([[[-5, 1], [n_a - 1, n_a + 7], [n_a + 2, n_a + 9], [-9, -2], [-1, 2], [n_b - 2, 2 ** 31 - 1],
                                            [-2 ** 31, -2 ** 31 + 5]]], np.int32), 3)]
    for k_a, k_b in ((1, 0), (0, 1), (2, 2), (10, 2), (0, 64), (64, 0), (31, 33)):
        sets.append(('%d + %d spans, shared' % (k_a, k_b),) + both(1, k_a, k_b))
        sets.append(('%d + %d spans, per row' % (k_a, k_b),) + both(rows, k_a, k_b))
    return sets


# ----------------------------------------------------------------------------- the definition, mask by mask
def sequential(x, calls, seed, device=None):
    """``calls``: ``[(kind, mask_param, mask_value, axis, p)]`` with ``kind`` ``'iid'`` or ``'shared'``, applied one after the other to
    ``x`` (a torch tensor, moved to ``device``) under ``torch.manual_seed(seed)``"""
    x = x if device is None else x.to(device)
    torch.manual_seed(seed)
    for kind, mask_param, mask_value, axis, p in calls:
        assert axis in (x.dim() - 2, x.dim() - 1) and 0.0 <= p <= 1.0
        n = x.shape[axis]
        mask_param = mask_param if p == 1.0 else min(mask_param, int(n * p))
        if mask_param < 1:
            continue
        if kind == 'iid':
            lead = x.shape[:-2]
            value = torch.rand(lead, device=x.device, dtype=x.dtype) * mask_param
            min_value = torch.rand(lead, device=x.device, dtype=x.dtype) * (n - value)
            start = min_value.long()[..., None, None]
            end = start + value.long()[..., None, None]
        else:
            value = torch.rand(1) * mask_param
            min_value = torch.rand(1) * (n - value)
            start = min_value.long().squeeze()
            end = (min_value.long() + value.long()).squeeze()
            assert end - start < mask_param
            start, end = start.to(x.device), end.to(x.device)
        index = torch.arange(n, device=x.device)
        index = index.view(-1, 1) if axis == x.dim() - 2 else index
        x = x.masked_fill((index >= start) & (index < end), mask_value)
    return x.contiguous()


def spec_augment_calls(dim, n_time_masks, time_mask_param, n_freq_masks, freq_mask_param, iid_masks, p, mask_value):
    """the sequential calls SpecAugment stands for: the time masks, then the frequency masks; ``p`` on the time masks only"""
    kind = 'iid' if iid_masks and dim >= 3 else 'shared'
    return [(kind, time_mask_param, mask_value, dim - 1, p)] * n_time_masks + [(kind, freq_mask_param, mask_value, dim - 2, 1.0)] * n_freq_masks


# ----------------------------------------------------------------------------- the grid of tac_mask_spans_f32
QUOTED = ('specaug.hip', (
    'constexpr int MS_THREADS = 256;',
    'constexpr int MS_PASSES = 4;',
    'constexpr int MS_TURN = 64;',
    'const long long q = (B + 3) / 4;',
    'for (int l = 6; l >= 4; --l) {',
    'const long long w = ((q + (1LL << l) - 1) >> l << l) - q;',
    'if (8 * w <= q) return l;',
    'if (waste < 0 || w < waste) {',
    'const bool turn = stride_a == 1 && stride_b != 1 && n_a > 1 && n_b > 1;',
    'const long long ab_lines = turn ? MS_TURN : (long long)(MS_THREADS >> lpl_log) * MS_PASSES;',
    'const long long width = turn ? MS_TURN : 4LL << lpl_log;',
    'const long long n_ab = (n_a + ab_lines - 1) / ab_lines, n_bc = (n_b + width - 1) / width;',
    'const long long units = rows * n_ab * n_bc;',
    'persistent_blocks(units, 1, (long long)device_cu_count() * 32)',
    'for (unsigned u = blockIdx.x; u < g.units; u += gridDim.x, par ^= 1) {',
))
CU_COUNTS = (256, 304)
BASE_ROWS = 5
MAX_TENSOR_BYTES = 512 * 1000 * 1000            # as tests/grid_rules.py


def ceil_div(a, b):
    return -(-a // b)


def lpl_log(n_b):
    q = ceil_div(n_b, 4)
    best, waste = 6, -1
    for l in (6, 5, 4):
        w = ceil_div(q, 1 << l) * (1 << l) - q
        if 8 * w <= q:
            return l
        if waste < 0 or w < waste:
            best, waste = l, w
    return best


PER_CU = 32


def launch(cus, rows, n_a, n_b, turn=False):
    """(units, grid cap) of a launch: the units (row, A-block, B-chunk) and the most workgroups that walk them"""
    ab_lines = 64 if turn else (256 >> lpl_log(n_b)) * 4
    width = 64 if turn else 4 << lpl_log(n_b)
    return rows * ceil_div(n_a, ab_lines) * ceil_div(n_b, width), cus * PER_CU


def wrap_rows(cus):
    """rows of one unit each with which every workgroup walks its loop twice and an odd number of them a third time on ``cus``
    compute units"""
    return 2 * PER_CU * cus + BASE_ROWS


#: (name, A, B, transposed): one unit per row in each of the kernel's three forms (dword loads, 16-byte loads, the turned load)
WRAP_FORMS = (('dwords', 3, 5, False), ('16-byte chunks', 4, 8, False), ('turned', 3, 5, True))


def assert_wraps(cus):
    rows = wrap_rows(cus)
    for name, n_a, n_b, turn in WRAP_FORMS:
        units, grid = launch(cus, rows, n_a, n_b, turn)
        r = units - 2 * grid
        assert units == rows and 0 < r < grid and r % 2 == 1, '%s on %d CUs: %d units on a grid of %d' % (name, cus, units, grid)
        assert 4 * rows * n_a * n_b < MAX_TENSOR_BYTES
    return rows
