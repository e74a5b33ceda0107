"""cna.tl.coef_strata / cna_coef_strata on the device (run with -m gpu on an MI355X), against the numpy restatement of
tests/test_coef_strata_host.py (itself pinned to matplotlib there).

Exact: n, n_kept, n_pos, n_neg, min, max, median, and the densities of a level whose kept values are all equal.
mean: |got - want| <= m 2^-52 mean|v| (m = the level's kept cells): two float64 summations of the same m terms in any order.
ssd:  |got - want| <= 4 m 2^-52 ssd + m dm^2, dm = the bound on the mean above: the terms (v - mean)^2 are non-negative, each
      carries two roundings on either side, the sums differ by the order again; and sum (v - (mu + e))^2 = S + m e^2 for the
      exact mean mu, so two means that each lie within dm of mu move the sum by at most m dm^2.
vals: rtol 3e-9, atol 1e-300: a term exp(-E) has relative error about E * delta, E <= 745 (beyond that the term underflows),
      delta <= 8 (m + 8) 2^-53 the relative error of inv for m <= 4096 + 37 -- 2.7e-9; every group here is at most that large."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from test_coef_strata_host import restated_strata

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _constant(name):
    src = open(os.path.join(ROOT, 'cna_amd', 'csrc', 'strata.hip')).read()
    return int(re.search(r'constexpr int64_t %s = (\d+);' % name, src).group(1))


CHUNK = _constant('ST_CHUNK')                  # values of a bin per wave of the moment, select and density kernels
N_LONG = 2 * CHUNK + 37                        # more than two chunks, a multiple of nothing
assert N_LONG <= 4096 + 37                     # the group size the density tolerance is derived for
CELLS = [1, 63, 64, 65, 1000, N_LONG]
BINS = [1, 2, 50, 1024]
POINTS = [1, 2, 64, 65, 100, 1024]


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.drop_expression()


def columns_for(n, n_bins, seed, layout='mixed', outlier=False):
    """(v, fdr, codes): normal draws, 5 % NaN, one +inf and one -inf (n permitting), 10 % of the codes -1, one bin empty."""
    rs = np.random.RandomState(seed)
    v = rs.randn(n) * 0.05 + 0.01
    fdr = rs.rand(n) * 0.3
    fdr[rs.rand(n) < 0.05] = np.nan
    if outlier:
        v[n // 3] = 0.01 + 20 * 0.05
    v[rs.rand(n) < 0.05] = np.nan
    if n >= 63:
        v[5], v[n - 7] = np.inf, -np.inf
    if layout == 'one':
        return v, fdr, np.full(n, n_bins - 1, dtype=np.int32)
    c = rs.randint(0, n_bins, n).astype(np.int32)
    if n_bins >= 2:
        c[c == n_bins // 2] = 0                 # a bin without cells
    c[rs.rand(n) < 0.1] = -1                    # cells that are left out
    return v, fdr, c


def _run(eng, v, fdr, codes, n_bins, points, bw, thresh=0.1):
    kind, val = ('constant', bw) if isinstance(bw, float) else (bw or 'scott', 0.0)
    return eng.coef_strata(v, fdr, codes, n_bins, thresh, points, kind, val)


def _compare(got, want, v, codes, n_bins, tag):
    for k in ('n', 'n_kept', 'n_pos', 'n_neg', 'min', 'max', 'median'):
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s' % (tag, k))
    m = want['n_kept'].astype(np.float64)
    keep = (codes >= 0) & np.isfinite(v)
    absmean = np.bincount(codes[keep], weights=np.abs(v[keep]), minlength=n_bins) / np.maximum(m, 1)
    some = m > 0
    assert np.isnan(got['mean'][~some]).all() and np.isnan(got['ssd'][~some]).all(), tag
    dm = m * EPS * absmean
    err_mean = np.abs(got['mean'] - want['mean'])[some]
    err_ssd = np.abs(got['ssd'] - want['ssd'])[some]
    bound_ssd = (4 * m * EPS * want['ssd'] + m * dm ** 2)[some]
    if some.any():
        print('%s: mean err / bound %.3e, ssd err / bound %.3e' % (
            tag, np.max(err_mean / np.maximum(dm[some], 1e-300)), np.max(err_ssd / np.maximum(bound_ssd, 1e-300))))
    assert (err_mean <= dm[some]).all(), tag + ' mean'
    assert (err_ssd <= bound_ssd).all(), tag + ' ssd'
    flat = some & (want['min'] == want['max'])
    np.testing.assert_array_equal(got['vals'][flat], want['vals'][flat], err_msg=tag + ' fallback')
    np.testing.assert_array_equal(got['vals'][~some], 0.0, err_msg=tag + ' empty')
    gv, wv = got['vals'][some & ~flat], want['vals'][some & ~flat]
    if gv.size:
        big = wv > 1e-290
        print('%s: vals largest relative difference %.3e' % (tag, np.max(np.abs(gv[big] - wv[big]) / wv[big]) if big.any() else 0.0))
    np.testing.assert_allclose(gv, wv, rtol=3e-9, atol=1e-300, err_msg=tag + ' vals')


def _check(eng, v, fdr, codes, n_bins, points=100, bw=None, tag=''):
    got = _run(eng, v, fdr, codes, n_bins, points, bw)
    want = restated_strata(v, fdr, codes, n_bins, 0.1, points, bw)
    _compare(got, want, v, codes, n_bins, tag)
    return got, want


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize('n_bins', BINS)
def test_cells_and_bins(eng, n_bins):
    for n in CELLS:
        v, fdr, codes = columns_for(n, n_bins, seed=n + n_bins, outlier=n >= 1000)
        got, want = _check(eng, v, fdr, codes, n_bins, tag='%d cells %d bins' % (n, n_bins))
    assert n == N_LONG and np.isinf(v).sum() == 2 and np.isnan(v).any() and (codes == -1).any()
    if n_bins >= 2:
        assert want['n'][n_bins // 2] == 0 and (want['n'] > want['n_kept']).any() and want['n_pos'].sum() > 0 < want['n_neg'].sum()
    if n_bins <= 2:
        assert want['n_kept'].max() > CHUNK


def test_without_an_fdr_column(eng):
    v, fdr, codes = columns_for(1000, 50, seed=2)
    got, want = _check(eng, v, None, codes, 50, tag='no fdr')
    assert got['n_pos'].sum() == 0 and got['n_neg'].sum() == 0


def test_segments_of_one_two_and_equal_values_and_one_long_bin(eng):
    v, fdr, codes = columns_for(N_LONG + N_LONG // 8, 50, seed=4, layout='one', outlier=True)     # more than 2 chunks KEPT
    got, want = _check(eng, v, fdr, codes, 50, tag='every cell in one bin')
    assert want['n_kept'][49] > 2 * CHUNK and (want['n_kept'][:49] == 0).all()
    v, fdr, codes = columns_for(1000, 8, seed=5)
    codes[codes >= 5] = 1
    codes[[10, 11, 12]] = 5                       # one kept cell beside two that are not finite
    v[[10, 11, 12]] = [0.125, np.nan, np.inf]
    codes[[20, 21]] = 6                           # two
    v[[20, 21]] = [-0.25, 0.5]
    codes[30:47] = 7                              # all equal
    v[30:47] = 0.1
    got, want = _check(eng, v, fdr, codes, 8, tag='one, two, equal')
    assert want['n_kept'][5:].tolist() == [1, 2, 17] and want['n'][5] == 3
    np.testing.assert_array_equal(got['vals'][5], np.ones(100))
    np.testing.assert_array_equal(got['vals'][7], np.ones(100))
    assert got['ssd'][5] == 0.0 and got['median'][6] == 0.125 and got['mean'][5] == 0.125


@pytest.mark.parametrize('points', POINTS)
def test_points(eng, points):
    for n_bins in (2, 50):                        # ~850 kept cells in one bin (more than most grids) and ~18 per bin (fewer than most)
        v, fdr, codes = columns_for(1000, n_bins, seed=points + n_bins)
        got, want = _check(eng, v, fdr, codes, n_bins, points=points, tag='%d points %d bins' % (points, n_bins))
        assert got['vals'].shape == (n_bins, points)
    assert (want['n_kept'] <= points).any() or points < 64


@pytest.mark.parametrize('bw', [None, 'silverman', 0.3], ids=['scott', 'silverman', 'constant'])
def test_bandwidth_rules(eng, bw):
    v, fdr, codes = columns_for(1000, 7, seed=11)
    got, want = _check(eng, v, fdr, codes, 7, bw=bw, tag='bw %r' % (bw,))
    other = _run(eng, v, fdr, codes, 7, 100, 'silverman' if bw is None else None)
    assert (other['vals'] != got['vals']).any()


# ------------------------------------------------------------------ 2. determinism, independence
def test_same_bits_on_a_second_call(eng):
    v, fdr, codes = columns_for(N_LONG, 50, seed=13, outlier=True)
    a = _run(eng, v, fdr, codes, 50, 100, None)
    _run(eng, *columns_for(1000, 7, seed=1), 7, 65, 0.3)                       # another shape in between
    b = _run(eng, v, fdr, codes, 50, 100, None)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_on_a_context_that_never_saw_a_graph(eng):
    from cna_amd.engine import Engine
    e = Engine(device=0)
    try:
        v, fdr, codes = columns_for(1000, 50, seed=17)
        _check(e, v, fdr, codes, 50, tag='fresh engine')
        assert e.expression_shape()['format'] == 'none'
    finally:
        e.close()


def test_between_launch_and_fetch_of_a_local_null(eng):
    """coef_strata between cna_null_local_launch and cna_null_local_fetch: the pending pass returns what it returns
    without the call in between, bit for bit, and the statistics are right."""
    from cna_amd import synth
    from test_gpu_gene_corr import _walk
    N, P = 50, 640
    data, meta = synth.make_dataset(20000, N, k=15, seed=21)
    rs = np.random.RandomState(4)
    y = rs.randn(N)
    y = (y - y.mean()) / y.std()
    Y = np.column_stack([y, rs.randn(N, P)])
    v, fdr, codes = columns_for(N_LONG, 50, seed=6)
    out = []
    for insert in (False, True):
        eng.null_local_discard()
        eng.drop_graph()
        _walk(eng, data, N)
        nz, maxabs = eng.select_standardized(None, None, y=y)
        maxcorr = max(maxabs, 0.001)
        thr = np.arange(maxcorr / 4, maxcorr, maxcorr / 400)
        edges = thr ** 2 - 1e-8 - 1e-5 * thr ** 2
        eng.condition(np.eye(N), Y)
        eng.null_local_launch(1, P, edges, thr)
        if insert:
            _check(eng, v, fdr, codes, 50, tag='between launch and fetch')
        fetched = eng.null_local_fetch()
        out.append([np.asarray(f).copy() for f in fetched])
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 3. refusals, memory
def test_refusals_leave_the_next_call_right(eng):
    from cna_amd._ffi import CnaHipError
    v, fdr, codes = columns_for(1000, 50, seed=19)
    want = _run(eng, v, fdr, codes, 50, 100, None)
    for wrong in (50, -2, 2 ** 31 - 1):
        bad = codes.copy()
        bad[777] = wrong                                         # a code equal to n_bins, below -1, far outside
        with pytest.raises(CnaHipError, match='outside'):
            _run(eng, v, fdr, bad, 50, 100, None)
    for points in (0, 1025):
        with pytest.raises(CnaHipError, match='points'):
            _run(eng, v, fdr, codes, 50, points, None)
    for n_bins in (0, 1025):
        with pytest.raises(CnaHipError, match='n_bins'):
            _run(eng, v, fdr, np.zeros(1000, np.int32), n_bins, 100, None)
    with pytest.raises(CnaHipError, match='bw_value'):
        _run(eng, v, fdr, codes, 50, 100, -1.0)
    with pytest.raises(ValueError):
        _run(eng, v, fdr, codes[:-1], 50, 100, None)
    got = _run(eng, v, fdr, codes, 50, 100, None)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    _compare(got, restated_strata(v, fdr, codes, 50, 0.1, 100, None), v, codes, 50, 'after the refusals')


def test_device_memory_returns_after_the_release(eng):
    eng.drop_expression()
    base = eng.device_bytes()
    v, fdr, codes = columns_for(N_LONG, 50, seed=23)
    _run(eng, v, fdr, codes, 50, 100, None)
    grown = eng.device_bytes()
    assert grown - base >= v.nbytes + fdr.nbytes + codes.nbytes
    _run(eng, v, fdr, codes, 50, 100, None)
    assert eng.device_bytes() == grown                          # grow-only: the same shape allocates nothing
    eng.drop_expression()
    assert eng.device_bytes() == base


# ------------------------------------------------------------------ 4. end to end
def test_end_to_end_on_the_demo_like_dataset(eng):
    import cna_amd as cna
    from cna_amd import synth
    d, samplem = synth.make_demo_like(keep_expression=True)
    cna.tl.association(d, samplem['case'].astype(float), 'id', key_added='coef', Nnull=200, seed=0, engine=eng)
    G = d.X.shape[1]
    lo, hi = d.X[:, :G // 2].mean(axis=1), d.X[:, G // 2:].mean(axis=1)
    pop = np.where(hi > lo, 'B', np.where(lo > 1.2, 'C', 'A'))               # the three populations, as a clustering finds them
    d.obs['leiden'] = [p + str(i % 4) for p, i in zip(pop, np.random.RandomState(1).permutation(len(pop)))]
    frame, violin = cna.tl.coef_strata(d, 'leiden', return_violin=True, engine=eng)
    levels = list(pd.unique(d.obs['leiden']))
    assert len(levels) == 12 and list(frame.index) == levels
    v, fdr = d.obs['coef'].values.astype(np.float64), d.obs['coef_fdr'].values.astype(np.float64)
    codes = pd.factorize(d.obs['leiden'])[0].astype(np.int32)
    assert np.isfinite(v).sum() > 0.9 * len(v) and frame['n_kept'].max() <= 4096 + 37
    want = restated_strata(v, fdr, codes, 12, 0.1, 100, None)
    got = dict(n=frame['n'].values, n_kept=frame['n_kept'].values, n_pos=frame['n_pos'].values, n_neg=frame['n_neg'].values,
               mean=frame['mean'].values, min=frame['min'].values, median=frame['median'].values, max=frame['max'].values,
               ssd=frame['sd'].values ** 2 * (frame['n_kept'].values - 1.0), vals=np.stack([x['vals'] for x in violin]))
    assert len(violin) == 12
    _compare(got, want, v, codes, 12, 'demo-like')
    for x, b in zip(violin, range(12)):
        np.testing.assert_array_equal(x['coords'], np.linspace(want['min'][b], want['max'][b], 100))
    # cna.pl.umap_ncorr's mask (plotting/_umap.py:10) on the same frame
    passed = d.obs['coef_fdr'] <= 0.1
    assert int(frame['n_pos'].sum() + frame['n_neg'].sum()) == int(passed.sum())
    assert int(passed.sum()) > 0
