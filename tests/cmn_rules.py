"""What ``sliding_window_cmn`` and ``compute_deltas`` are held to, for tests/test_cmn_deltas_cpu.py and tests/test_cmn_deltas_gpu.py.

The references are written from the definitions, in float64, one frame at a time with every window summed directly (a numpy loop
per frame): they share no structure with the kernels' sliding sums, the composite's ``cumsum`` differences or its index gather.

    window of frame t, W = cmn_window, M = min_cmn_window
        center:     ws = min(max(t - W // 2, 0), max(T - W, 0)), we = min(ws + W, T)
        otherwise:  ws = max(t - W, 0), we = max(t + 1, M); where we > T: ws = max(ws - (we - T), 0), we = T
    out[t, f] = x[t, f] - mean(x[ws:we, f]);  norm_vars: times (sum(x^2) / n - (sum(x) / n)^2)^-1/2, and 0 where n == 1

    deltas: n = (win_length - 1) // 2, denom = n (n + 1)(2n + 1) / 3, out[t] = sum_{k=-n..n} k x[idx(t + k)] / denom, idx the index
    map of torch.nn.functional.pad

Per-element rules, u = 2^-24; every element is checked:

    CMN             |got - want| <= 2 u |want| + 2^-36 A,              A = max|x| over the element's window
    norm_vars       |got - want| <= 6 u |want| + 2^-36 A / sigma,      exactly 0 where n == 1; the inputs keep every window's variance
                    at or above ``min_ratio`` (1e-4) of its mean square
    deltas          |got - want| <= (2n + 2) u sum_k |k| |x[idx(t + k)]| / denom
    adjoints        the same rules on the adjoint: A = max|g| over the frames whose window holds the element; for the deltas the sum
                    runs over the (t, k) that read the element

The first CMN term is one rounding to float32 with margin; the second allows 2^17 float64 roundings of frame-sized terms and is
4096 times below what ONE float32 rounding of the mean would cost, so it does not depend on t or T: an implementation whose error
grows along the row fails it.  An output that must be non-finite (its window holds a NaN or an infinity) is required to be
non-finite, and every other output to be finite and within the rule."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -36
DELTAS_MODES = ('replicate', 'constant', 'reflect', 'circular')


def bounds(t, n_frames, cmn_window, min_cmn_window, center):
    """the closed form: (ws, we) of frame t"""
    if center:
        ws = min(max(t - cmn_window // 2, 0), max(n_frames - cmn_window, 0))
        return ws, min(ws + cmn_window, n_frames)
    ws, we = max(t - cmn_window, 0), max(t + 1, min_cmn_window)
    if we > n_frames:
        ws, we = max(ws - (we - n_frames), 0), n_frames
    return ws, we


def cmn_reference(x, cmn_window, min_cmn_window, center, norm_vars, min_ratio=1e-4):
    """(want, allowance, must_be_nan) for x (…, T, F), all float64 arrays of x's shape (must_be_nan: bool).  Each window is
    summed directly."""
    x = np.asarray(x, dtype=np.float64)
    n_frames = x.shape[-2]
    want, allow = np.zeros_like(x), np.zeros_like(x)
    nan = np.zeros(x.shape, dtype=bool)
    for t in range(n_frames):
        ws, we = bounds(t, n_frames, cmn_window, min_cmn_window, center)
        assert 0 <= ws <= t < we <= n_frames
        w = x[..., ws:we, :]
        n = we - ws
        bad = ~np.isfinite(w).all(axis=-2)
        w = np.where(bad[..., None, :], 0.0, w)
        mean = w.sum(axis=-2) / n
        a = np.abs(w).max(axis=-2)
        d = np.where(bad, 0.0, x[..., t, :]) - mean
        if norm_vars:
            if n == 1:
                want[..., t, :], allow[..., t, :] = 0.0, 0.0
            else:
                meansq = (w * w).sum(axis=-2) / n
                var = meansq - mean * mean
                ok = bad | (var >= min_ratio * meansq)
                assert ok.all(), 'the test input breaks the rule\'s precondition at frame %d: variance %g of mean square %g' % (
                    t, var[~ok].min(), meansq[~ok].max())
                sigma = np.sqrt(np.where(bad, 1.0, var))
                want[..., t, :] = d / sigma
                allow[..., t, :] = 6 * U * np.abs(d / sigma) + TINY * a / sigma
        else:
            want[..., t, :] = d
            allow[..., t, :] = 2 * U * np.abs(d) + TINY * a
        nan[..., t, :] = bad
    return want, allow, nan


def cmn_adjoint_reference(g, cmn_window, min_cmn_window, center):
    """(want, allowance) of the gradient w.r.t. the input for grad_out g (…, T, F), norm_vars off:
    g_x[s] = g[s] - sum over {t : ws(t) <= s < we(t)} of g[t] / n(t), each sum written out"""
    g = np.asarray(g, dtype=np.float64)
    n_frames = g.shape[-2]
    win = [bounds(t, n_frames, cmn_window, min_cmn_window, center) for t in range(n_frames)]
    want, allow = np.zeros_like(g), np.zeros_like(g)
    for s in range(n_frames):
        ts = [t for t in range(n_frames) if win[t][0] <= s < win[t][1]]
        assert ts == list(range(ts[0], ts[-1] + 1)) and ts[0] <= s <= ts[-1]        # an interval that holds s
        scale = np.array([1.0 / (win[t][1] - win[t][0]) for t in ts])
        part = g[..., ts[0]:ts[-1] + 1, :]
        want[..., s, :] = g[..., s, :] - (part * scale[:, None]).sum(axis=-2)
        allow[..., s, :] = 2 * U * np.abs(want[..., s, :]) + TINY * np.abs(part).max(axis=-2)
    return want, allow


def deltas_index(t, n_frames, mode):
    """source frame of padded position t, or None for a zero"""
    if 0 <= t < n_frames:
        return t
    if mode == 'replicate':
        return 0 if t < 0 else n_frames - 1
    if mode == 'constant':
        return None
    if mode == 'reflect':
        return -t if t < 0 else 2 * (n_frames - 1) - t
    return t % n_frames


def deltas_reference(x, win_length, mode):
    """(want, allowance) for x (…, F, T)"""
    x = np.asarray(x, dtype=np.float64)
    n_frames = x.shape[-1]
    n = (win_length - 1) // 2
    denom = n * (n + 1) * (2 * n + 1) / 3.0
    want, mass = np.zeros_like(x), np.zeros_like(x)
    for t in range(n_frames):
        for k in range(-n, n + 1):
            s = deltas_index(t + k, n_frames, mode)
            if s is not None and k != 0:
                assert 0 <= s < n_frames
                want[..., t] += k * x[..., s]
                mass[..., t] += abs(k) * np.abs(x[..., s])
    return want / denom, (2 * n + 2) * U * mass / denom


def deltas_adjoint_reference(g, win_length, mode):
    """(want, allowance) of the gradient w.r.t. the input for grad_out g (…, F, T): every (t, k) sends k g[t] / denom to idx(t + k)"""
    g = np.asarray(g, dtype=np.float64)
    n_frames = g.shape[-1]
    n = (win_length - 1) // 2
    denom = n * (n + 1) * (2 * n + 1) / 3.0
    want, mass = np.zeros_like(g), np.zeros_like(g)
    for t in range(n_frames):
        for k in range(-n, n + 1):
            s = deltas_index(t + k, n_frames, mode)
            if s is not None and k != 0:
                want[..., s] += k * g[..., t]
                mass[..., s] += abs(k) * np.abs(g[..., t])
    return want / denom, (2 * n + 2) * U * mass / denom


def assert_within(got, want, allow, what, must_be_nan=None):
    """Every element of ``got`` within ``allow`` of ``want`` (non-finite exactly where ``must_be_nan``); prints and returns the
    worst error / allowance ratio"""
    got = np.asarray(got.detach().cpu().numpy() if hasattr(got, 'detach') else got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    finite = np.isfinite(got)
    if must_be_nan is None:
        must_be_nan = np.zeros(got.shape, dtype=bool)
    assert np.array_equal(~finite, must_be_nan), '%s: %d output(s) non-finite where %d must be (first mismatch at %r)' % (
        what, int((~finite).sum()), int(must_be_nan.sum()), tuple(np.argwhere(finite == must_be_nan)[0]))
    err = np.where(must_be_nan, 0.0, np.abs(np.where(finite, got, 0.0) - want))
    exact = (allow == 0.0) & ~must_be_nan
    assert (err[exact] == 0.0).all(), '%s: an element that must be exact is off by %g' % (what, err[exact].max())
    ratio = np.where(exact | must_be_nan, 0.0, err / np.where(allow == 0.0, 1.0, allow))
    worst = float(ratio.max()) if ratio.size else 0.0
    print('%s: worst error / allowance %.4f' % (what, worst))
    assert worst <= 1.0, '%s: error %.3g of the allowance at %r' % (what, worst, tuple(np.unravel_index(ratio.argmax(), ratio.shape)))
    return worst


def float32_running_loop(x, cmn_window, min_cmn_window, center, norm_vars):
    """What the kernel replaces: the incremental add-one / drop-one procedure with float32 running sums (torchaudio's loop),
    kept to show that the CMN rule tells a drifting implementation from a sound one"""
    x = np.asarray(x, dtype=np.float32)
    n_frames = x.shape[-2]
    out = np.zeros_like(x)
    cur = np.zeros(x.shape[:-2] + x.shape[-1:], dtype=np.float32)
    cursq = np.zeros_like(cur)
    last_ws, last_we = 0, 0
    for t in range(n_frames):
        ws, we = bounds(t, n_frames, cmn_window, min_cmn_window, center)
        if last_we == 0:
            cur = x[..., ws:we, :].sum(axis=-2, dtype=np.float32)
            cursq = (x[..., ws:we, :] ** 2).sum(axis=-2, dtype=np.float32)
        else:
            for j in range(last_we, we):
                cur = cur + x[..., j, :]
                cursq = cursq + x[..., j, :] ** 2
            for j in range(last_ws, ws):
                cur = cur - x[..., j, :]
                cursq = cursq - x[..., j, :] ** 2
        last_ws, last_we = ws, we
        n = np.float32(we - ws)
        out[..., t, :] = x[..., t, :] - cur / n
        if norm_vars:
            out[..., t, :] = 0.0 if we - ws == 1 else out[..., t, :] * (cursq / n - (cur / n) ** 2) ** np.float32(-0.5)
    return out


def alternating(shape, seed, offset=0.0):
    """float32 (…, T, F): (-1)^t (1 + U(0, 0.5)) + offset — every window of two or more frames holds both signs, so its variance
    is a fixed share of its mean square (the precondition of the norm_vars rule holds by construction for |offset| <= 10)"""
    rng = np.random.default_rng(seed)
    sign = np.where(np.arange(shape[-2]) % 2 == 0, 1.0, -1.0)[:, None]
    return (sign * (1.0 + 0.5 * rng.random(shape)) + offset).astype(np.float32)
