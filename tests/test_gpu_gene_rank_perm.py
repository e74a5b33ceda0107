"""cna.tl.gene_rank_test / cna_x_columns, cna_gene_rank_corr_x, cna_gene_rank_corr_wide on the device (run with -m gpu on an
MI355X).

cna_x_columns is specified to the bit (float64, the samples ascending, the product rounded and then added): its output is
compared as bytes with the numpy loop of tests/test_gene_rank_perm_host.py.  The two rank entries return integers, and tie
terms that are integers below 2^53 on every shape here: assert_array_equal against the restatement of
tests/test_gene_rank_corr_host.py (checked there against scipy.stats.spearmanr) and, group of 16 columns by group, against
cna_gene_rank_corr itself under the call's kept set.  End to end, rho against scipy within RHO_TOL, the project's figure.

Shapes: the nine core genes on 3001 cells in the four stored forms (three sort chunks per long gene, two tiles of genes at
least under SMALL_WORK_BYTES: tests/test_gene_rank_corr_host.py proves both), 1 to 40 columns (one group, a full one, last
groups of 1 and 8 columns), X of 1, 3, 33 and 130 samples (3 and 33: the row stride is not the sample count), and the 3.1M
cells at which a sum passes 64 bits."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.stats

from test_gene_markers_host import FORMS, N_CORE, SMALL_WORK_BYTES, core_input, core_values
from test_gene_rank_corr_host import RHO_TOL, WIDE_CELLS, limbs, rank_corr_tiles, restated_rank_corr, wide_input
from test_gene_rank_perm_host import (COLUMN_COUNTS, COLUMN_SAMPLES, WIDE_COUNTS, X_ROWS, column_case, constant_row,
                                      restated_columns, wide_keys)
from test_gene_test_host import restated_bh
from test_gpu_gene_rank_corr import _equal, _same_bits

pytestmark = pytest.mark.gpu

_restated = {}


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()


def typed_values(form):
    Vg, _ = core_values()
    return Vg.astype(np.float32 if form.endswith('f32') else np.float64)


def restated(form, tag, V):
    """one restatement per stored type and column set: the sparse and the dense upload of one type hold the same values"""
    key = (form[-3:], tag)
    if key not in _restated:
        _restated[key] = restated_rank_corr(typed_values(form), V)
    return _restated[key]


# ------------------------------------------------------------------ the columns
@pytest.mark.parametrize('q', COLUMN_COUNTS)
@pytest.mark.parametrize('samples', COLUMN_SAMPLES)
def test_columns_are_the_numpy_loop_byte_for_byte(eng, samples, q):
    X, xrow, Z = column_case(samples, q)
    eng.ensure_expression(core_input('csr-f32'))
    eng.upload_x(X)
    gen = eng.x_generation()
    got = eng.x_columns(xrow, Z)
    want = restated_columns(X, xrow, Z)
    assert got.shape == (q, N_CORE) and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.broadcast_to(xrow < 0, got.shape))   # NaN exactly where xrow is -1
    assert got.tobytes() == want.tobytes()
    assert eng.x_columns(xrow, Z).tobytes() == got.tobytes()                     # a second run
    assert eng.x_generation() == gen                                             # X is read only
    assert np.array_equal(eng.x_full(), X)                                       # ... and as it was


# ------------------------------------------------------------------ the wide entry against the existing one and scipy
@pytest.mark.parametrize('q', WIDE_COUNTS)
@pytest.mark.parametrize('form', FORMS)
def test_wide_equals_the_restatement_and_the_existing_entry_group_by_group(eng, form, q):
    eng.ensure_expression(core_input(form))
    V = wide_keys(q)
    want = restated(form, ('wide', q), V)
    got = eng.gene_rank_corr_wide(V)
    assert got[0].shape == (q, 9) and got[3].shape == (q,)
    _equal('%s q=%d' % (form, q), got, want)
    kept = np.isfinite(V).all(axis=0)
    ok = ~want[4]
    assert got[4] == int(kept.sum()) and list(np.flatnonzero(got[5])) == [7]
    if q > 1:
        assert got[3][constant_row(q)] == float(got[4] ** 3 - got[4])            # the constant column
    # group by group: cna_gene_rank_corr on the group's columns with the call's kept set imposed
    for k0 in range(0, q, 16):
        Vg = np.where(kept[None, :], V[k0:k0 + 16], np.nan)
        one = eng.gene_rank_corr(Vg)
        np.testing.assert_array_equal(got[0][k0:k0 + 16][:, ok], one[0][:, ok])
        np.testing.assert_array_equal(got[1][k0:k0 + 16][:, ok], one[1][:, ok])
        np.testing.assert_array_equal(got[2][ok].view(np.int64), one[2][ok].view(np.int64))
        np.testing.assert_array_equal(got[3][k0:k0 + 16].view(np.int64), one[3].view(np.int64))
        assert one[4] == got[4] and np.array_equal(one[5], got[5])
    # two tiles of genes at least under the small budget (the per-entry buffer is refilled): the same bits; and on a rerun
    assert len(rank_corr_tiles(form, SMALL_WORK_BYTES)[0]) >= 2
    _same_bits(eng.gene_rank_corr_wide(V, SMALL_WORK_BYTES), got, ok)
    _same_bits(eng.gene_rank_corr_wide(V), got, ok)


def test_wide_rho_against_scipy(eng):
    from cna_amd.tools._gene_rank_corr import rank_corr_statistics
    form, q = 'dense-f64', 33
    eng.ensure_expression(core_input(form))
    V = wide_keys(q)
    rho = rank_corr_statistics(*eng.gene_rank_corr_wide(V))
    kept = np.isfinite(V).all(axis=0)
    Xd = typed_values(form)
    worst, seen = 0.0, 0
    for k in (0, 1, 15, 16, 18, 31, 32):
        for g in (1, 3, 4, 6, 8):
            want = scipy.stats.spearmanr(Xd[kept, g], V[k, kept]).statistic
            worst, seen = max(worst, abs(rho[k, g] - want)), seen + 1
    print('wide rho against scipy.stats.spearmanr on %d (column, gene) pairs: max |d rho| = %.3e' % (seen, worst))
    assert worst <= RHO_TOL
    assert np.isnan(rho[constant_row(q)]).all() and np.isnan(rho[:, [0, 2, 5, 7]]).all()


# ------------------------------------------------------------------ the X route
@pytest.mark.parametrize('integer', [False, True])
@pytest.mark.parametrize('samples,q', list(zip(COLUMN_SAMPLES, COLUMN_COUNTS)))
def test_x_route_equals_wide_on_the_restated_columns(eng, samples, q, integer):
    X, xrow, Z = column_case(samples, q, integer)
    V = restated_columns(X, xrow, Z)
    kept = xrow >= 0
    eng.upload_x(X)
    # the tie term scipy's ranking gives: rows 5 and 9 of X are equal, so no column is free of ties
    tie = np.array([float(sum(int(t) ** 3 - int(t) for t in np.unique(c[kept] + 0.0, return_counts=True)[1])) for c in V])
    assert (tie >= 6.0).all() and (integer or (tie == 6.0).all()) and (not integer or (tie > 1e5).all())
    for form in FORMS:
        eng.ensure_expression(core_input(form))
        got = eng.gene_rank_corr_x(xrow, Z)
        wide = eng.gene_rank_corr_wide(V)
        ok = ~wide[5]
        assert got[4] == X_ROWS == wide[4]
        _same_bits(got, wide, ok)
        np.testing.assert_array_equal(got[3], tie)
        _equal('%s x route' % form, got, restated(form, ('x', samples, q, integer), V))
        _same_bits(eng.gene_rank_corr_x(xrow, Z, SMALL_WORK_BYTES), got, ok)
        _same_bits(eng.gene_rank_corr_x(xrow, Z), got, ok)


def test_the_sum_passes_64_bits(eng):
    """3 100 000 cells, X one sample holding the key, Z = [[1], [-1]]: S = +-(m^3 - m) / 3 in both limbs"""
    Xe, key, S = wide_input()
    m = WIDE_CELLS
    assert S > 2 ** 63 - 1
    eng.ensure_expression(Xe)
    eng.upload_x(key[:, None])
    s_lo, s_hi, tie_gene, tie_key, got_m, nan = eng.gene_rank_corr_x(np.arange(m, dtype=np.int64), np.array([[1.0], [-1.0]]))
    want_lo, want_hi = limbs(np.array([[S, -S], [-S, S]], dtype=object))
    assert got_m == m and not nan.any() and tie_gene.tolist() == [0.0, 0.0] and tie_key.tolist() == [0.0, 0.0]
    np.testing.assert_array_equal(s_hi, want_hi)
    np.testing.assert_array_equal(s_lo, want_lo)
    assert s_hi.tolist() == [[0, -1], [-1, 0]]
    eng.drop_expression()


# ------------------------------------------------------------------ refusals, nothing written
def _raw(eng, which, q, xrow=None, Z=None, V=None, work_bytes=0, null=False, G=9, rows=48):
    """(status, untouched) of a raw call with pre-filled outputs; xrow / Z for the X entries, V for the wide one"""
    from cna_amd._ffi import ptr
    s_lo = np.full((rows, G), 77, dtype=np.uint64)
    s_hi = np.full((rows, G), -77, dtype=np.int64)
    tie_gene, tie_key = np.full(G, -77.0), np.full(rows, -77.0)
    m = np.full(1, -77, dtype=np.int64)
    nan = np.full(G, 77, dtype=np.uint8)
    out = np.full((rows, len(xrow) if xrow is not None else 1), -77.0)
    tail = [ptr(s_lo), ptr(s_hi), ptr(tie_gene), ptr(tie_key), m.ctypes.data_as(C.POINTER(C.c_int64)), None if null else ptr(nan)]
    if which == 'columns':
        rc = eng.lib.cna_x_columns(eng.h, ptr(xrow), len(xrow), ptr(Z), q, None if null else ptr(out))
    elif which == 'x':
        rc = eng.lib.cna_gene_rank_corr_x(eng.h, ptr(xrow), len(xrow), ptr(Z), q, work_bytes, *tail)
    else:
        rc = eng.lib.cna_gene_rank_corr_wide(eng.h, ptr(V), q, work_bytes, *tail)
    untouched = ((s_lo == 77).all() and (s_hi == -77).all() and (tie_gene == -77.0).all() and (tie_key == -77.0).all()
                 and m[0] == -77 and (nan == 77).all() and (out == -77.0).all())
    return rc, untouched, eng.lib.cna_last_error()


def test_bad_arguments_are_refused_and_nothing_is_written(eng):
    from cna_amd import _ffi
    X, xrow, Z = column_case(3, 40)
    xrow, Z = np.array(xrow), np.ascontiguousarray(np.tile(Z, (110, 1))[:4097])
    V = np.ascontiguousarray(np.tile(wide_keys(1), (4097, 1)))
    eng.ensure_expression(core_input('csr-f32'))
    eng.upload_x(X)
    for which in ('columns', 'x', 'wide'):
        for q in (0, 4097, -1):
            rc, untouched, msg = _raw(eng, which, q, xrow, Z, V)
            assert rc == -1 and untouched and b'1 <= q <= 4096' in msg, (which, q, msg)     # CNA_EINVAL
        rc, untouched, msg = _raw(eng, which, 3, xrow, Z, V, null=True)
        assert rc == -1 and untouched and b'null pointer' in msg, which
        if which != 'columns':
            rc, untouched, msg = _raw(eng, which, 3, xrow, Z, V, work_bytes=-5)
            assert rc == -1 and untouched and b'work_bytes' in msg, which
    free = np.flatnonzero(xrow < 0)
    took = np.flatnonzero(xrow >= 0)
    cases = {'too large': (free[0], X_ROWS, b'an xrow lies outside'), 'below -1': (free[1], -2, b'an xrow lies outside'),
             'twice': (free[2], xrow[took[40]], b'two cells name the same row of X')}
    for which in ('columns', 'x'):
        for name, (i, v, words) in cases.items():
            bad = xrow.copy()
            bad[i] = v
            rc, untouched, msg = _raw(eng, which, 17, bad, Z)
            assert rc == -1 and untouched and words in msg and msg.startswith(b'cna_'), (which, name, msg)
        rc, untouched, msg = _raw(eng, which, 17, xrow[:-1].copy(), Z)                      # another length than the matrix' cells
        assert rc == -1 and untouched and b'3000 entries' in msg, which
    # an inf in X: a formed value is not finite.  In a row no cell names it does no harm
    named = np.zeros(X_ROWS, dtype=bool)
    named[xrow[took]] = True
    assert named.all()
    Xi = np.array(X)
    Xi[xrow[took[7]], 1] = np.inf
    eng.upload_x(Xi)
    rc, untouched, msg = _raw(eng, 'x', 17, xrow, Z)
    assert rc == -1 and untouched and b'not finite' in msg
    Zi = Z[:17].copy()
    Zi[16, 2] = -np.inf                                                                     # ... or in Z, in the last group
    eng.upload_x(X)
    rc, untouched, msg = _raw(eng, 'x', 17, xrow, Zi)
    assert rc == -1 and untouched and b'not finite' in msg
    with pytest.raises(_ffi.CnaHipError, match='not finite'):
        eng.gene_rank_corr_x(xrow, Zi)
    with pytest.raises(ValueError):
        eng.gene_rank_corr_x(xrow, Z[:3, :2])
    with pytest.raises(ValueError):
        eng.gene_rank_corr_wide(V[:3, :-1])
    with pytest.raises(ValueError):
        eng.x_columns(xrow[:-1], Z[:3])
    # and the entries are as they were
    got = eng.gene_rank_corr_x(xrow, Z[:17])
    _same_bits(got, eng.gene_rank_corr_wide(restated_columns(X, xrow, Z[:17])), ~got[5])


def test_missing_state_is_an_estate_error(eng):
    from cna_amd._ffi import CnaHipError
    from cna_amd.engine import Engine
    X, xrow, Z = column_case(3, 16)
    xrow, V = np.array(xrow), np.array(wide_keys(16))
    eng.upload_x(X)
    eng.drop_expression()
    for which in ('columns', 'x', 'wide'):
        rc, untouched, msg = _raw(eng, which, 16, xrow, Z, V)
        assert rc == -4 and untouched and b'no expression matrix' in msg, which            # CNA_ESTATE
    other = Engine()
    try:
        other.ensure_expression(core_input('csr-f32'))
        for which in ('columns', 'x'):
            rc, untouched, msg = _raw(other, which, 16, xrow, Z)
            assert rc == -4 and untouched and b'X not available' in msg, which             # CNA_ESTATE: no X
        got = other.gene_rank_corr_wide(V)                                                  # the wide entry needs no X
        _equal('no X', got, restated('csr-f32', ('wide', 16), V))
    finally:
        other.close()


# ------------------------------------------------------------------ end to end
def _expression():
    from test_gpu_gene_test import expression
    E = expression(3000, 70, seed=70)
    return E


def _spearman_null(eng, E, kept, Z, genes):
    """{(g, p): scipy's rho of gene g with the null coefficient X z_p over the kept cells}: the columns restated from the
    working matrix as the engine holds it"""
    xrow = eng.x_row_of_cells()
    Xk = eng.x_full()                                                  # kept cells x samples, caller's order
    assert np.array_equal(np.flatnonzero(xrow >= 0), np.flatnonzero(kept)) and Xk.shape[0] == int(kept.sum())
    cols = restated_columns(Xk, np.arange(Xk.shape[0]), Z)
    return {(g, p): scipy.stats.spearmanr(E[kept, g], cols[p]).statistic for g in genes for p in range(len(Z))}


def test_end_to_end_on_the_qc_dataset(eng):
    import cna_amd as cna
    from cna_amd.tools._gene_null import null_phenotypes
    from test_gpu_gene_test import dataset
    data, y, batches, covs = dataset('qc')
    call = dict(nsteps=3, Nnull=40, seed=3)
    E = _expression()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d0 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'])
        p0 = cna.tl.association(d0, y, 'id', batches=batches, covs=covs, engine=eng, **call)
    kept = np.isfinite(d0.obs['coef'].values)
    assert (~kept).any()
    E[kept, 2] = 0.0                                                   # gene 2: non-zero only on cells the QC dropped
    E[:, 5] = 3.5                                                      # gene 5: constant
    assert (E[~kept, 2] != 0).any() and not E[:, 1].any()
    d = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        frame, null_rho = cna.tl.gene_rank_test(d, y, 'id', batches=batches, covs=covs, return_null=True, var_key_added='grt_',
                                                engine=eng, **call)
        assert (eng.x_row_of_cells() == -1).any() and np.array_equal(eng.x_row_of_cells() >= 0, kept)
        Zall = null_phenotypes(type(data)(data.obs[['id']].copy(), data.obsp['connectivities']), y, 'id', batches, covs, None, 'coef',
                               eng, dict(call), 'test')[1]
        want = _spearman_null(eng, E, kept, np.ascontiguousarray(Zall[:, 1:].T), (0, 3, 4, 17, 69))
        rc = cna.tl.gene_rank_corr(d, 'coef', engine=eng)
        cut, null_cut = cna.tl.gene_rank_test(d, y, 'id', batches=batches, covs=covs, return_null=True, n_perm=16, engine=eng, **call)
    assert list(frame.columns) == ['rho', 'null_mean', 'null_sd', 'z', 'p', 'q'] and null_rho.shape == (70, 40)
    assert frame.attrs['p'] == p0 and frame.attrs['n_null'] == 40 and frame.attrs['n_cells'] == int(kept.sum())
    for k in ('coef', 'coef_fdr'):
        assert d.obs[k].values.tobytes() == d0.obs[k].values.tobytes(), k
    assert np.array_equal(frame['rho'].values, rc['coef'].values, equal_nan=True) and frame.index.equals(rc.index)
    dead = np.zeros(70, dtype=bool)
    dead[[1, 2, 5]] = True
    assert np.isnan(frame.values[dead]).all() and np.isnan(null_rho[dead]).all()
    assert np.isfinite(frame.values[~dead]).all() and np.isfinite(null_rho[~dead]).all()
    worst = max(abs(null_rho[g, p] - v) for (g, p), v in want.items())
    print('end to end: null_rho against scipy.stats.spearmanr on %d pairs: max |d rho| = %.3e' % (len(want), worst))
    assert worst <= RHO_TOL
    rho = frame['rho'].values
    p = (1.0 + (np.abs(null_rho) >= np.abs(rho)[:, None]).sum(axis=1)) / 41.0
    p[dead] = np.nan
    assert np.array_equal(frame['p'].values, p, equal_nan=True)
    assert np.array_equal(frame['q'].values, restated_bh(p), equal_nan=True)
    assert np.array_equal(frame['null_mean'].values[~dead], null_rho[~dead].mean(axis=1))
    assert np.array_equal(d.var['grt_p'].values, frame['p'].values, equal_nan=True)
    # n_perm=16: the first 16 columns of the full call, bit for bit
    assert null_cut.shape == (70, 16) and cut.attrs['n_null'] == 16
    assert null_cut.tobytes() == np.ascontiguousarray(null_rho[:, :16]).tobytes()
    assert np.array_equal(cut['rho'].values, rho, equal_nan=True)


def test_end_to_end_on_the_two_call_path(eng):
    """one batch, a seed, nsteps given: the association is answered by the two-call path (tools/_fast.py)"""
    import cna_amd as cna
    from cna_amd.tools import _fast
    from cna_amd.tools._gene_null import null_phenotypes
    from test_gpu_gene_test import dataset
    data, y, batches, covs = dataset('24')
    E = _expression()
    call = dict(nsteps=3, Nnull=40, seed=3)
    d = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d0 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'])
        p0 = cna.tl.association(d0, y, 'id', engine=eng, **call)
        before = _fast.stats['taken']
        frame, null_rho = cna.tl.gene_rank_test(d, y, 'id', return_null=True, engine=eng, **call)
        assert _fast.stats['taken'] == before + 1
        Zall = null_phenotypes(type(data)(data.obs[['id']].copy(), data.obsp['connectivities']), y, 'id', None, None, None, 'coef',
                               eng, dict(call), 'test')[1]
        want = _spearman_null(eng, E, np.ones(3000, dtype=bool), np.ascontiguousarray(Zall[:, 1:].T), (0, 33, 69))
        rc = cna.tl.gene_rank_corr(d, 'coef', engine=eng)['coef'].values
    assert frame.attrs['p'] == p0 and frame.attrs['n_cells'] == 3000 and null_rho.shape == (70, 40)
    for k in ('coef', 'coef_fdr'):
        assert d.obs[k].values.tobytes() == d0.obs[k].values.tobytes(), k
    assert np.array_equal(frame['rho'].values, rc, equal_nan=True) and np.isnan(rc[1]) and np.isfinite(np.delete(rc, 1)).all()
    worst = max(abs(null_rho[g, p] - v) for (g, p), v in want.items())
    print('two-call path: null_rho against scipy.stats.spearmanr on %d pairs: max |d rho| = %.3e' % (len(want), worst))
    assert worst <= RHO_TOL
