"""The integer counts of the local test on inputs where they have ONE right answer (run with -m gpu on an MI355X).

tests/exact_grid.py: X and Yc on a 2^-4 grid, so every dot product is exact in any order, on the matrix cores and in
numpy alike, and the cuts on the grid of the products, so that many outputs sit exactly ON a cut.  Every comparison here
is array_equal: tails, sums, ranks, num_detected, the FDR table and the per-cell column.  Each case prints how many of
its outputs are tied with a cut and asserts there are at least 50 (tests/test_exact_grid_host.py checks the helpers and
the same floor on the CPU); one ulp up on every edge moves exactly those outputs, one ulp down none.

- null counts at the row strides, sample counts and row counts the kernels branch on, f64 kernel and integer pass;
- T = 1, 2, 3, 63 ... 512 thresholds and P = 1, 15 ... 65 permutations; T = 513 is refused and changes nothing;
- observed counts with thresholds ON attained coefficients: ranks are inclusive, num_detected is strict;
- the FDR table and the per-cell column by three routes (bins ahead of the null + host expansion, the same through
  percell(), the device lookup), thresholds ON attained coefficients, a table with inf and NaN, and a device cell order.
"""
import numpy as np
import pytest

import exact_grid as eg

pytestmark = pytest.mark.gpu

REFUSED = r'more than 512 FDR thresholds are not supported'


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    return get_engine()


def _grid_y(N, seed):
    return eg.grid_matrix(np.random.RandomState(seed), N, 1)[:, 0]


def _ranges(P):
    """Sub-ranges (col0, count) of P resident columns."""
    if P < 3:
        return []
    col0 = 3 if P > 8 else 1
    return [(col0, P - col0 - 1)]


def _check_null(eng, c, edges, what, want_i8=None, prepared_thr=None, nc=None):
    """Tails (f64 kernel), sums (integer pass where it applies) and a sub-range of the resident columns against brute
    force; optionally the prepared pass with thresholds.  Returns the brute-force tails."""
    X, Yc, N = c['X'], c['Yc'], c['N']
    P = Yc.shape[1]
    want = eg.brute_tails(X, Yc, N, edges)
    tails = eng.null_local(Yc, edges)                              # leaves Yc resident
    np.testing.assert_array_equal(tails, want, err_msg=what + ': tails')
    sums = eng.null_local_resident(0, P, edges, sums_only=True)
    used, rechecked, fallback = eng.null_local_i8_stats()
    print('%s: integer pass used=%s rechecked=%d fallback=%s' % (what, used, rechecked, fallback))
    np.testing.assert_array_equal(sums, want.sum(axis=0), err_msg=what + ': sums')
    if want_i8 is not None:
        assert used == want_i8 and not fallback, (what, used, fallback)
    for col0, cnt in _ranges(P):
        np.testing.assert_array_equal(eng.null_local_resident(col0, cnt, edges), want[col0:col0 + cnt],
                                      err_msg=what + ': tails of a sub-range')
        np.testing.assert_array_equal(eng.null_local_resident(col0, cnt, edges, sums_only=True),
                                      want[col0:col0 + cnt].sum(axis=0), err_msg=what + ': sums of a sub-range')
    if prepared_thr is not None:
        eng.null_local_prepare(P, edges, prepared_thr)
        eng.null_local_launch(0, P, None)
        sums, ranks, numdet = eng.null_local_fetch()
        want_ranks, want_numdet = eg.brute_obs(nc, edges, prepared_thr)
        np.testing.assert_array_equal(sums, want.sum(axis=0), err_msg=what + ': sums of the prepared pass')
        np.testing.assert_array_equal(ranks, want_ranks, err_msg=what + ': ranks of the prepared pass')
        np.testing.assert_array_equal(numdet, want_numdet, err_msg=what + ': num_detected of the prepared pass')
    return want


def _upload(eng, c, seed=3):
    """X on the device, the coefficients of a grid phenotype taken (and exact)."""
    y = _grid_y(c['N'], seed)
    eng.null_local_discard()
    eng.upload_x(c['X'])
    nc, maxabs = eng.ncorrs(y, fetch=True)
    want = c['X'].dot(y) / c['N']
    np.testing.assert_array_equal(nc, want)
    assert maxabs == np.abs(want).max()
    return nc


@pytest.mark.parametrize('n,N,P', eg.NULL_SHAPES)
def test_null_counts_on_the_grid(eng, n, N, P):
    """Zero tolerance: the f64 kernel's tails and the sums-only pass equal the brute-force count on the edges, one ulp
    above them (every tied output leaves its bin) and one ulp below (nothing moves); the integer pass stands (used, no
    fallback) wherever there are at most 256 samples -- its recheck count is printed, not bounded: ties are rechecked
    by design.  Then edges ON attained values that are no arithmetic progression: the always-walk path."""
    c = eg.null_case(n, N, P)
    print('(%d, %d, %d): %d outputs tied with a cut' % (n, N, P, c['ties']))
    assert c['ties'] >= 50
    _upload(eng, c)
    e = c['edges']
    i8 = N <= 256
    want = _check_null(eng, c, e, 'edges', want_i8=i8)
    up = _check_null(eng, c, np.nextafter(e, np.inf), 'edges + 1 ulp', want_i8=i8)
    down = _check_null(eng, c, np.nextafter(e, -np.inf), 'edges - 1 ulp', want_i8=i8)
    assert int(want.sum()) - int(up.sum()) == c['ties']
    np.testing.assert_array_equal(down, want)
    pick, irr = eg.irregular_edges(np.random.RandomState(5), c['D'], N, 120)
    _check_null(eng, c, irr, 'attained, irregular', want_i8=False)


@pytest.mark.parametrize('T', eg.T_EDGES)
def test_null_and_observed_counts_at_the_table_sizes(eng, T):
    """T at and around what k_tail_sums (64 per block), k_suffix_sum / k_fdr_table (512 wide), guess_from_thr and
    exact_cuts (T = 1, 2, 3) branch on: tails, sums and the prepared pass with thresholds, all against brute force."""
    c = eg.edge_case(eg.EDGE_P_FOR_T, T)
    print('T = %d: %d outputs tied with a cut' % (T, c['ties']))
    assert c['ties'] >= 50
    nc = _upload(eng, c)
    thr = c['d'] / c['N']
    for what, e in (('edges', c['edges']), ('edges + 1 ulp', np.nextafter(c['edges'], np.inf))):
        _check_null(eng, c, e, what, prepared_thr=thr, nc=nc)
    ranks, numdet = eng.obs_counts(c['edges'], thr)
    want_ranks, want_numdet = eg.brute_obs(nc, c['edges'], thr)
    np.testing.assert_array_equal(ranks, want_ranks)
    np.testing.assert_array_equal(numdet, want_numdet)


@pytest.mark.parametrize('P', eg.P_EDGES)
def test_null_counts_at_the_permutation_counts(eng, P):
    """P at and around the 16 permutation groups of k_tail_sums and the 64-wide strips of the null kernels."""
    c = eg.edge_case(P, 300)
    print('P = %d: %d outputs tied with a cut' % (P, c['ties']))
    assert c['ties'] >= 50
    nc = _upload(eng, c)
    thr = c['d'] / c['N']
    want = _check_null(eng, c, c['edges'], 'edges', want_i8=True, prepared_thr=thr, nc=nc)
    up = _check_null(eng, c, np.nextafter(c['edges'], np.inf), 'edges + 1 ulp', want_i8=True, prepared_thr=thr, nc=nc)
    assert int(want.sum()) - int(up.sum()) == c['ties']


def test_more_than_512_thresholds_are_refused_and_change_nothing(eng):
    """T = 513: obs_counts, null_local and null_local_launch refuse with the library's message; the call made before
    the refusal, repeated after it, returns the same integers."""
    from cna_amd import _ffi
    c = eg.edge_case(17, 512)
    big = eg.edge_case(17, 513)
    P = 17
    nc = _upload(eng, c)
    thr, thr_big = c['d'] / c['N'], big['d'] / big['N']
    assert len(thr_big) == 513 and len(big['edges']) == 513

    def obs():
        return eng.obs_counts(c['edges'], thr)

    def tails():
        return (eng.null_local(c['Yc'], c['edges']),)

    def pass_():
        eng.null_local_launch(0, P, c['edges'], thr)
        return eng.null_local_fetch()
    refused = {
        'obs_counts': lambda: eng.obs_counts(big['edges'], thr_big),
        'null_local': lambda: eng.null_local(c['Yc'], big['edges']),
        'null_local_launch': lambda: eng.null_local_launch(0, P, big['edges'], thr_big),
    }
    for before, name in ((obs, 'obs_counts'), (tails, 'null_local'), (pass_, 'null_local_launch')):
        first = before()
        with pytest.raises(_ffi.CnaHipError, match=REFUSED):
            refused[name]()
        again = before()
        for a, b in zip(first, again):
            np.testing.assert_array_equal(a, b, err_msg=name)
    np.testing.assert_array_equal(tails()[0], eg.brute_tails(c['X'], c['Yc'], c['N'], c['edges']))
    sums, ranks, numdet = pass_()
    want_ranks, want_numdet = eg.brute_obs(nc, c['edges'], thr)
    np.testing.assert_array_equal(ranks, want_ranks)
    np.testing.assert_array_equal(numdet, want_numdet)


def test_observed_counts_with_thresholds_on_the_coefficients(eng):
    """ranks = #{nc^2 >= e} and the lookup are inclusive, num_detected = #{|nc| > thr} is strict: thresholds ON attained
    |nc| (with their neighbours one ulp either side), an arithmetic set on the grid, a duplicate in front (no step for
    the linear guess), thresholds above max |nc| (ranks 0) and T = 1, 2, 3; edges thr^2 exactly and the reference's."""
    o = eg.obs_case()
    nc_want, N = o['nc'], o['N']
    eng.null_local_discard()
    eng.upload_x(o['X'])
    nc, maxabs = eng.ncorrs(o['y'], fetch=True)
    np.testing.assert_array_equal(nc, nc_want)
    for name, thr in o['sets'].items():
        ties = eg.obs_ties(nc, thr)
        print('%s: %d thresholds, %d cells tied with one' % (name, len(thr), ties))
        if len(thr) > 3:
            assert ties >= 50, (name, ties)
        for kind, edges in (('thr^2', thr ** 2), ('reference', eg.reference_edges(thr))):
            ranks, numdet = eng.obs_counts(edges, thr)
            want_ranks, want_numdet = eg.brute_obs(nc, edges, thr)
            np.testing.assert_array_equal(ranks, want_ranks, err_msg='%s, %s: ranks' % (name, kind))
            np.testing.assert_array_equal(numdet, want_numdet, err_msg='%s, %s: num_detected' % (name, kind))
            if kind == 'thr^2':
                on = np.array([(np.abs(nc) == t).sum() for t in thr])
                assert (ranks - numdet >= on).all() and on.sum() >= ties and (ranks != numdet).any()
    top = o['sets']['above_max']
    ranks, numdet = eng.obs_counts(top ** 2, top)
    assert ranks[-4] == (np.abs(nc) == top[-4]).sum() >= 1 and ranks[-3:].tolist() == [0, 0, 0]
    assert numdet[-4:].tolist() == [0, 0, 0, 0]


# ----------------------------------------------------------------------- FDR table and per-cell column
N_T, P_T = 24, 64


def _walk(e, data, n_samples, nsteps=3):
    from cna_amd.tools._nam import sample_codes
    e.ensure_graph(data.obsp['connectivities'])
    e.colsums(1)
    codes, labels = sample_codes(data.obs['id'])
    assert len(labels) == n_samples
    e.set_samples(codes, n_samples, np.bincount(codes, minlength=n_samples).astype(float))
    e.nam_steps(nsteps)


@pytest.fixture(scope='module')
def cells():
    """3000 cells x 24 samples; about 5 % of the cells dropped (coefficient NaN, FDR 1); a phenotype without signal, so
    that the permutations reach as far as the observed coefficients do."""
    from cna_amd import synth
    data, meta = synth.make_dataset(3000, N_T, k=15, seed=2)
    rs = np.random.RandomState(6)
    y = rs.randn(N_T)
    y = (y - y.mean()) / y.std()
    Y = np.column_stack([y, rs.randn(N_T, P_T)])
    keep = rs.rand(3000) >= 0.05
    assert 100 < (~keep).sum() < 200
    return dict(data=data, y=y, Y=Y, keep=keep)


def _resident(e, cells):
    """Walk, selection, coefficients (k_ncorrs) and conditioned phenotypes on engine `e`; returns the coefficient column."""
    e.null_local_discard()
    _walk(e, cells['data'], N_T)
    nz, maxabs = e.select_standardized(cells['keep'], None, y=cells['y'])
    assert nz == 0
    e.ncorrs(cells['y'])
    e.condition(np.eye(N_T), cells['Y'])
    coef = e.percell()[0].copy()
    assert np.array_equal(np.isnan(coef), ~cells['keep'])
    assert maxabs == pytest.approx(np.nanmax(np.abs(coef)), rel=1e-12)
    return coef


def _attained_thresholds(coef, T, seed=8):
    """T ascending thresholds ON attained |coef| in [max / 4, max]: from T = 64 on, at least 50 attained values and for
    the rest a value with its neighbours one ulp either side."""
    rs = np.random.RandomState(seed + T)
    a = np.abs(coef[~np.isnan(coef)])
    vals = np.unique(a[a >= a.max() / 4])
    if T < 64:
        return np.sort(rs.choice(vals, size=T, replace=False))
    trip = max(0, min(T // 3, (T - 50) // 2))
    plain = T - 3 * trip
    pick = rs.choice(vals, size=plain + trip, replace=False)
    v = pick[:trip]
    return np.sort(np.concatenate([pick, np.nextafter(v, np.inf), np.nextafter(v, 0.0)]))


def _unrelated_edges(coef, thr):
    """Edges that are not the thresholds': the reference's for the lower half, then values above max coef^2 -- first
    within reach of the permutations (ranks 0, sums > 0: inf), then beyond everything (0 / 0: NaN)."""
    h = len(thr) // 2
    m2 = np.nanmax(np.abs(coef)) ** 2
    above = m2 * np.concatenate([1 + 1e-6 * (1 + np.arange(8)), np.linspace(1.2, 400.0, len(thr) - h - 8)])
    return np.concatenate([eg.reference_edges(thr[:h]), above])


def _table_sets(coef):
    maxcorr = max(np.nanmax(np.abs(coef)), 0.001)
    ref = np.arange(maxcorr / 4, maxcorr, maxcorr / 400)
    sets = [('attained, T = %d' % T, thr, eg.reference_edges(thr)) for T in (1, 2, 64, 300, 512)
            for thr in [_attained_thresholds(coef, T)]]
    sets.append(('reference', ref, eg.reference_edges(ref)))
    thr = _attained_thresholds(coef, 64)
    sets.append(('unrelated edges', thr, _unrelated_edges(coef, thr)))
    return sets


def _route(e, cells, thr, edges, how):
    """One pass over columns 1 .. P with thresholds, and the per-cell FDR column by route `how`:
    'early'   bins ahead of the null, table behind it, expanded on the host by percell_fdr_copy_early;
    'percell' the same pass, expanded by percell() itself;
    'device'  no percell_coef_launch: percell() looks the column up on the device (k_percell_fdr).
    Returns (sums, ranks, num_detected, coefficient column, FDR column)."""
    e.ncorrs(cells['y'])                      # (also withdraws an earlier percell_coef_launch)
    if how != 'device':
        assert e.percell_coef_launch()
    e.null_local_prepare(P_T, edges, thr)
    e.null_local_launch(1, P_T, None)
    dst = np.full(e.n, -1.0)
    if how == 'early':
        assert e.percell_fdr_copy_early(dst)
    sums, ranks, numdet = e.null_local_fetch()
    with np.errstate(all='ignore'):
        runmin = np.fmin.accumulate(sums / ranks / P_T)
    coef, fdr = e.percell(thr, runmin)
    coef, fdr = coef.copy(), fdr.copy()
    if how == 'early':
        assert e.percell_fdr_copied_early()
        np.testing.assert_array_equal(fdr, dst)
    else:
        assert not e.percell_fdr_copied_early() and (dst == -1.0).all()
    return sums, ranks, numdet, coef, fdr


def _check_table(e, cells, coef, name, thr, edges, routes, orc):
    from cna_amd.tools._association import _fdr_tables
    ties = eg.obs_ties(coef[cells['keep']], thr)
    print('%s: %d thresholds, %d cells tied with one' % (name, len(thr), ties))
    if not name.startswith('reference'):          # (a table of T thresholds ties at most T distinct coefficients)
        assert ties >= min(50, len(thr)), (name, ties)
    out = {}
    for how in routes:
        sums, ranks, numdet, coef_r, fdr = _route(e, cells, thr, edges, how)
        np.testing.assert_array_equal(coef_r, coef, err_msg='%s, %s: coef' % (name, how))
        want_ranks, want_numdet = eg.brute_obs(coef[cells['keep']], edges, thr)
        np.testing.assert_array_equal(ranks, want_ranks, err_msg='%s, %s: ranks' % (name, how))
        np.testing.assert_array_equal(numdet, want_numdet, err_msg='%s, %s: num_detected' % (name, how))
        with np.errstate(all='ignore'):
            table = sums / ranks / P_T
            runmin = np.fmin.accumulate(table)
        fdr_vals, t5, t10, run = _fdr_tables(sums, ranks, P_T, thr)
        np.testing.assert_array_equal(fdr_vals, table)
        np.testing.assert_array_equal(run, runmin)
        np.testing.assert_array_equal(fdr, orc.percell_fdr(coef, thr, table), err_msg='%s, %s: FDR column' % (name, how))
        assert (fdr[~cells['keep']] == 1.0).all()
        out[how] = (sums, ranks, numdet, fdr, table)
    first = out[routes[0]]
    for how in routes[1:]:
        for a, b in zip(first, out[how]):
            np.testing.assert_array_equal(a, b, err_msg='%s: %s against %s' % (name, how, routes[0]))
    return first


def test_fdr_table_and_percell_column_by_three_routes(eng, cells, monkeypatch):
    """Every route gives the column of the reference's lookup (_association.py:234-237 as oracle.percell_fdr states it:
    thr <= |coef| inclusive, pandas' NaN-skipping min, 1 where nothing qualifies or the cell was dropped) from the
    integers the pass returned, bit for bit; the table rebuilt from those integers is _fdr_tables'.  Thresholds ON
    attained |coef| at T = 1, 2, 64, 300, 512, the reference's arithmetic table, and a table with inf and NaN."""
    from oracle import cna_oracle as orc
    monkeypatch.setenv('CNA_REORDER', '0')
    coef = _resident(eng, cells)
    assert eng.perm is None
    for name, thr, edges in _table_sets(coef):
        sums, ranks, numdet, fdr, table = _check_table(eng, cells, coef, name, thr, edges, ['early', 'percell', 'device'], orc)
        if name == 'unrelated edges':
            assert np.isinf(table).any() and np.isnan(table).any() and np.isfinite(table[:len(thr) // 2]).all()
            passed = np.abs(coef) >= thr[len(thr) // 2]
            assert passed.sum() >= 50 and np.isfinite(fdr[passed]).all()


def test_percell_column_in_a_device_cell_order(eng, cells, monkeypatch):
    """The same pass on an engine that keeps the cells in a locality order: k_percell_bins then writes through a real
    `orig` map, and the column is the unordered engine's bit for bit."""
    from cna_amd.engine import Engine
    from oracle import cna_oracle as orc
    monkeypatch.setenv('CNA_REORDER', '0')
    coef = _resident(eng, cells)
    assert eng.perm is None
    sets = [s for s in _table_sets(coef) if s[0] in ('attained, T = 300', 'unrelated edges')]
    plain = [_check_table(eng, cells, coef, name, thr, edges, ['early'], orc) for name, thr, edges in sets]
    eng.drop_graph()                          # (the next user of the shared engine uploads in its own order)
    monkeypatch.setenv('CNA_REORDER', '1')
    e = Engine()
    try:
        coef_o = _resident(e, cells)
        assert e.perm is not None and not np.array_equal(e.perm, np.arange(len(e.perm)))
        np.testing.assert_array_equal(coef_o, coef)
        for (name, thr, edges), want in zip(sets, plain):
            got = _check_table(e, cells, coef, name + ', ordered', thr, edges, ['early', 'device'], orc)
            for a, b in zip(got, want):
                np.testing.assert_array_equal(a, b, err_msg=name)
    finally:
        e.close()
