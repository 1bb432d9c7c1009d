"""Not gpu: tests/polyphase_rules.py itself.  Every launcher line it restates stands verbatim in csrc/resample.hip; its geometry is
the product's banks'; the census of the instantiations public arguments reach agrees with ``_hip.resample_tile`` on every bank it
forms, and the case tables of tests/test_resample_gpu.py and tests/test_pitch_shift_gpu.py reach every reachable one — forward and
adjoint bank counted separately; the sweep generator draws valid cases that cover every reachable instantiation at the default
count and seed; and the float64 reference of tests/resample_rules.py agrees with the float64 stock-torch composite at the hundreds
of taps per phase of the narrow tiles."""
import os

import numpy as np
import pytest
import torch

import pitch_shift_rules as PS
import polyphase_rules as PR
import resample_rules as R

NAMES = dict(lpw='lowpass_filter_width', rolloff='rolloff', method='resampling_method', beta='beta')
DEFAULT_CASES = 24                      # TAC_FUZZ_CASES of tests/test_polyphase_sweeps_gpu.py

# every table case on a narrow tile or in bucket 64, with the instantiation (VEC aside) of its forward and of its adjoint bank:
# a case taken out of a table, or one that a retuned launcher moves, fails here.  The tables are restated ON PURPOSE: several
# cases share an instantiation, so the coverage assertion alone would let one of them go; an edit of a table is an edit here.
PINNED_LDS = {
    '9:1': ((512, True, False), (1024, False, False)), '12:1': ((512, True, True), (1024, False, False)),
    '25:2': ((512, False, False), (1024, False, True)), '34:3': ((512, False, True), (1024, False, False)),
    '441:40': ((512, False, False), (1024, False, True)), '16:1': ((256, True, True), (1024, False, False)),
    '17:1': ((256, True, False), (1024, False, False)), '33:2': ((256, False, False), (1024, False, True)),
    '50:3': ((256, False, True), (1024, False, False)), '48:1': ((256, True, True), (1024, False, False)),
    '12:1-sinc_interp_kaiser': ((512, True, True), (1024, False, False)), '8:1-10-0.9': ((512, True, True), (1024, False, False)),
}
PINNED_LDS_GRADIENT = {
    '1:12': (512, True, True), '2:25': (512, False, False), '1:9': (512, True, False), '3:34': (512, False, True),
    '1:16': (256, True, True), '3:50': (256, False, True), '1:17': (256, True, False), '2:33': (256, False, False),
}
PINNED_WIDE = {
    '4001:1000': ((1024, 64), (1024, 16)), '5001:1000': ((1024, 64), (1024, 16)), '2001:2000-24': ((1024, 64), (1024, 64)),
    '2001:2000-31': ((1024, 64), (1024, 64)), '12001:1000-1': ((512, 32), (1024, 16)), '12001:1000-2': ((512, 64), (1024, 16)),
    '9001:1000-2': ((512, 48), (1024, 16)), '20001:1000-1': ((256, 48), (1024, 16)), '30001:1000-1': ((256, 64), (1024, 16)),
    '1000:4001': ((1024, 16), (1024, 64)), '1000:12001-1': ((1024, 16), (512, 32)), '1000:9001-2': ((1024, 16), (512, 48)),
    '1000:12001-2': ((1024, 16), (512, 64)), '1000:20001-1': ((1024, 16), (256, 48)), '1000:30001-1': ((1024, 16), (256, 64)),
    '8:1-1-1.0': ((512, 16), (1024, 16)), '1:8-1-1.0': ((1024, 16), (512, 16)), '16:1-1-1.0': ((256, 32), (1024, 16)),
    '1:16-1-1.0': ((1024, 16), (256, 32)),
}
UNREACHABLE_WIDE = {(256, 16, True), (256, 16, False)}


@pytest.fixture(scope='module')
def tac():
    import torchaudio_contrib_amd as t
    return t


def product_banks(tac_, c):
    key = tac_._resample.constants(c[0], c[1], **{NAMES[k]: v for k, v in c[2].items()})
    return tac_._resample.bank(*key), tac_._resample.adjoint_bank(*key)


def same_geometry(b, g):
    return (b.phases, b.step, b.K, list(b.off), list(b.run)) == (g.phases, g.step, g.K, list(g.off), list(g.run))


# ----------------------------------------------------------------------------- the rules against the source and the product
def test_quoted_launcher_lines_are_in_the_source(tac):
    csrc = os.path.join(os.path.dirname(os.path.abspath(tac.__file__)), 'csrc')
    for name, quotes in PR.QUOTED:
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        for q in quotes:
            assert q in text, '%s no longer holds %r: tests/polyphase_rules.py restates a launcher that has changed' % (name, q)
    H = tac._hip
    assert (H.RESAMPLE_MAX_BANK, H.RESAMPLE_MAX_PHASES) == (PR.RESAMPLE_MAX_BANK, PR.RESAMPLE_MAX_PHASES)
    assert (H.RESAMPLE_WIDE_MAX_TAPS, H.RESAMPLE_WIDE_MAX_BANK, H.RESAMPLE_WIDE_SPAN_MAX, H.RESAMPLE_WIDE_ROWS) == \
        (PR.RSW_MAX_TAPS, PR.RSW_MAX_BANK, PR.RSW_SPAN_MAX, PR.RSW_ROWS)
    assert PS.WIDE_ROWS == PR.RSW_ROWS and PS.LDS_BYTES == PR.RS_LDS_BYTES


def test_geometry_is_the_products_banks(tac):
    """every table case, both banks, Hann and Kaiser (with a beta of its own): the window moves no tap's support"""
    cases = PR.LDS_CASES + PR.LDS_GRADIENT_CASES + PR.WIDE_CASES + PR.WIDE_CASES_1024
    cases = cases + [(9, 1, dict(method='sinc_interp_kaiser', beta=5.0)), (2, 33, dict(PR.KAISER, lpw=9, rolloff=0.7)),
                     (12001, 1000, dict(PR.KAISER, lpw=2)), (1000, 4001, PR.KAISER)]
    for c in cases:
        for b, g in zip(product_banks(tac, c), PR.geometries(c[0], c[1], c[2].get('lpw', 6), c[2].get('rolloff', 0.99))):
            assert same_geometry(b, g), PR.case_id(c)
            assert tac._hip.resample_tile(b) == (PR.lds_variant(g, True) or (None,))[0], PR.case_id(c)
            plan = tac._hip.resample_wide_plan(b)
            assert (plan is None) == (PR.wide_variant(b, True) is None) and (plan is None or plan[1] == PR.wide_variant(b, True)[0])


def test_the_rule_on_hand_made_banks():
    """the launcher's own limits, one at a time (banks no public argument gives: the rule, not the kernel, is exercised)"""
    G = PR.Geometry
    assert PR.lds_variant(G(1, 2, 25, [-12], [25]), True) == (1024, True, True, True, 8)
    assert PR.lds_variant(G(1, 2, 25, [-12], [25]), False) == (1024, True, True, False, 8)
    assert PR.lds_variant(G(2049, 1, 1, [0] * 2049, [1] * 2049), True) is None
    assert PR.lds_variant(G(2, 3, 10241, [0, 0], [10241] * 2), True) is None
    # span: 3 + 1023 S + K, rounded up to four, against 8192; then 511 S against 8192; then 255 S against 14336
    assert PR.lds_variant(G(1, 8, 5, [0], [5]), True)[0] == 1024 and PR.lds_variant(G(1, 8, 6, [0], [6]), True)[0] == 512
    assert PR.lds_variant(G(1, 16, 13, [0], [13]), True)[0] == 512 and PR.lds_variant(G(1, 16, 14, [0], [14]), True)[0] == 256
    assert PR.lds_variant(G(1, 56, 53, [0], [53]), True)[0] == 256 and PR.lds_variant(G(1, 56, 54, [0], [54]), True) is None
    # per_cu: 160 KiB over the bytes of bank, tables and skewed span
    assert PR.lds_variant(G(1, 56, 53, [0], [53]), True)[4] == 2
    assert PR.rs_span_cap(441, 13, 160, -7, 152, 10) == (3 + 3 * 160 + 159 + 13 + 3) & ~3


# ----------------------------------------------------------------------------- the census
@pytest.fixture(scope='module')
def lds_census(tac):
    seen = []

    def agree(g, v):
        seen.append(1)
        assert tac._hip.resample_tile(g) == (None if v is None else v[0]), (g.phases, g.step, g.K, v)

    return PR.census(PR.LDS_ENTRY, agree), len(seen)


@pytest.fixture(scope='module')
def wide_census(tac):
    return PR.census(PR.WIDE_ENTRY)


def test_lds_census_and_tables(tac, lds_census):
    found, banks = lds_census
    assert banks > 50000
    every = {(t, p1, skew, vec) for t in PR.TILES for p1 in (True, False) for skew in (True, False) for vec in (True, False)}
    tables = PR.reached_by_tables()
    for side in ('forward', 'adjoint'):
        assert set(found[side]) == every, 'unreachable on the grid: %r' % sorted(every - set(found[side]))
        missing = set(found[side]) - tables[PR.LDS_ENTRY, side]
        assert not missing, 'no %s case of the tables runs %r (reached by %r)' % (side, sorted(missing), [found[side][v] for v in missing])
    got = {PR.case_id(c): tuple(PR.lds_variant(PR.case_geometry(c, adj), True)[:3] for adj in (False, True))
           for c in PR.LDS_CASES if PR.lds_variant(PR.case_geometry(c), True)[0] != 1024}
    assert got == PINNED_LDS
    got = {PR.case_id(c): PR.lds_variant(PR.case_geometry(c, True), True)[:3]
           for c in PR.LDS_GRADIENT_CASES if PR.lds_variant(PR.case_geometry(c, True), True)[0] != 1024}
    assert got == PINNED_LDS_GRADIENT
    assert all(PR.lds_covers(c) for c in PR.LDS_CASES + PR.LDS_GRADIENT_CASES)
    # the tiles the GPU tests pin by pair
    assert PR.NARROW_TILES == {k[:2]: v[0][0] for k, v in ((tuple(int(n) for n in i.split(':')), v) for i, v in PINNED_LDS.items() if '-' not in i)}
    for c in PR.LDS_CASES[:22] + PR.LDS_GRADIENT_CASES:
        for adjoint in (False, True):
            assert PR.lds_variant(PR.case_geometry(c, adjoint), True)[0] == PR.pinned_tile(c[0], c[1], adjoint), (PR.case_id(c), adjoint)


def test_the_coverage_edge(tac):
    """48:1 is the last integer decimation the kernel holds (581 taps, 256 outputs per tile); 59:1 and 60:1 are beyond it"""
    for n, tile in ((48, 256), (59, None), (60, None)):
        key = tac._resample.constants(n, 1)
        b = tac._resample.bank(*key)
        v = PR.lds_variant(b, True)
        assert tac._hip.resample_tile(b) == tile == (None if v is None else v[0]), n
        assert tac._hip.resample_covers(*key) == (tile is not None) == PR.lds_covers((n, 1, PR.HANN))
    assert tac._resample.bank(*tac._resample.constants(48, 1)).K == 581
    # the 10 of the 110 ordered pairs of the eleven rates that run a 512 tile, forward or gradient
    narrow = set()
    for a in PR.RATES:
        for b in PR.RATES:
            if a != b:
                c = R.reduced(a, b) + (PR.HANN,)
                assert PR.lds_covers(c)
                tiles = {PR.lds_variant(PR.case_geometry(c, adj), True)[0] for adj in (False, True)}
                if tiles != {1024}:
                    assert tiles == {1024, 512}
                    narrow.add((a, b))
    low, high = (8000, 11025, 12000), (88200, 96000)
    assert narrow == {p for lo in low for hi in high for p in ((lo, hi), (hi, lo)) if (lo, hi) != (12000, 88200)}
    assert len(narrow) == 10


def test_wide_census_and_tables(tac, wide_census):
    every = {(t, kb, vec) for t in PR.TILES for kb in PR.BUCKETS for vec in (True, False)}
    tables = PR.reached_by_tables()
    for side in ('forward', 'adjoint'):
        assert every - set(wide_census[side]) == UNREACHABLE_WIDE, sorted(every - set(wide_census[side]))
        missing = set(wide_census[side]) - tables[PR.WIDE_ENTRY, side]
        assert not missing, 'no %s case of the tables runs %r' % (side, sorted(missing))
    got = {}
    for c in PR.WIDE_CASES:
        v = tuple(PR.wide_variant(PR.case_geometry(c, adj), True)[:2] for adj in (False, True))
        if any(t != 1024 or kb == 64 for t, kb in v):
            got[PR.case_id(c)] = v
    assert got == PINNED_WIDE
    assert all(PR.wide_covers(c) for c in PR.WIDE_CASES + PR.WIDE_CASES_1024)
    # the bucket edges: K = 16 | 17, 32 | 33, 48 | 49, and 63 | 65 around the last K the kernel takes (no width gives 64 at 2001:2000)
    taps = {lpw: PR.geometry(2001, 2000, lpw).K for lpw in (8, 16, 24, 31, 32)}
    assert taps == {8: 17, 16: 33, 24: 49, 31: 63, 32: 65} and PR.geometry(2000, 2001).K == 13
    assert PR.geometry(10079, 8000).K == 16 and PR.wide_variant(PR.geometry(10079, 8000), True)[1] == 16
    assert PR.wide_variant(PR.geometry(2001, 2000, 32), True) is None and not PR.wide_covers((2001, 2000, dict(lpw=32)))


# ----------------------------------------------------------------------------- the sweep generator
@pytest.mark.parametrize('kernel', [PR.LDS_ENTRY, PR.WIDE_ENTRY])
def test_sweep_draws_valid_cases_on_every_reachable_variant(tac, kernel, lds_census, wide_census):
    found = lds_census[0] if kernel == PR.LDS_ENTRY else wide_census
    reachable = set(found['forward']) | set(found['adjoint'])
    for seed in (0, 1, 2):
        cases, drawn, rejected = PR.sweep(kernel, DEFAULT_CASES, seed)
        assert len(cases) == DEFAULT_CASES and 4 * rejected <= drawn, (drawn, rejected)
        assert {c.variant[:-1] for c in cases} == reachable, seed         # by either bank: per bank is the tables' part, above
        assert {c.gradient for c in cases} == {False, True}
        for c in cases:
            key = tac._resample.constants(c.orig, c.new, **{NAMES[k]: v for k, v in c.kw.items()})
            assert 0.5 <= c.kw['rolloff'] <= 1.0 and 1 <= c.kw['lpw'] <= 32 and 1 <= c.rows <= 6 and c.length >= 1 and c.out_len >= 1
            n_out = R.out_length(c.length, c.orig, c.new)
            if kernel == PR.LDS_ENTRY:
                assert tac._hip.resample_covers(*key) and c.out_len == n_out
                rule = PR.lds_variant
            else:
                assert tac._hip.resample_fit_covers(key, c.length, c.out_len)
                assert c.out_len != n_out or not tac._hip.resample_covers(*key)        # ... and it is the wide kernel that runs
                rule = PR.wide_variant
            b = (tac._resample.adjoint_bank if c.gradient else tac._resample.bank)(*key)
            assert rule(b, c.variant[-2]) == c.variant, c
            assert (c.length if c.gradient else n_out) <= 3 * c.variant[0] + 9 + c.new and c.layout in PR.LAYOUTS[c.variant[-2]]
    assert PR.sweep(kernel, 7, 5) == PR.sweep(kernel, 7, 5) and PR.sweep(kernel, 7, 5)[0] != PR.sweep(kernel, 7, 6)[0]


def test_reference_is_the_float64_composite_on_narrow_tiles(tac):
    """the per-sample sum of tests/resample_rules.py against torch's float64 ``conv1d`` with the full bank at K in the hundreds
    (the narrow tiles' banks), forward and gradient: a few 1e-16 of the sum of absolute products, as
    tests/test_resample_cpu.py holds the short banks to"""
    cases, _, _ = PR.sweep(PR.LDS_ENTRY, DEFAULT_CASES, 0)
    narrow = [c for c in cases if c.variant[0] != 1024 and c.length > 30]
    assert len(narrow) >= 6 and max(PR.geometry(c.orig, c.new, c.kw['lpw'], c.kw['rolloff'], c.gradient).K for c in narrow) > 300
    for c in narrow[:8]:
        length = min(c.length, 4000)
        x = torch.from_numpy(R.waveform((2, length), seed=c.seed)).double()
        kw = {NAMES[k]: v for k, v in c.kw.items()}
        if not c.gradient:
            ref, bound = R.reference(x, c.orig, c.new, **c.kw)
            got = tac.resample(x, c.orig, c.new, **kw).numpy()
        else:
            x.requires_grad_(True)
            g = R.waveform((2, R.out_length(length, c.orig, c.new)), seed=c.seed + 1)
            ref, bound = R.adjoint_reference(g, length, c.orig, c.new, **c.kw)
            (got,) = torch.autograd.grad(tac.resample(x, c.orig, c.new, **kw), x, grad_outputs=torch.from_numpy(g).double())
            got = got.numpy()
        assert got.shape == ref.shape and (np.abs(got - ref) <= 1e-8 * bound + 1e-300).all(), c
