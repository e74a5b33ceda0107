"""cna.tl.gene_test_strata end to end on the device (run with -m gpu on an MI355X), after the pattern of
tests/test_gpu_gene_test.py; the kernels alone are in tests/test_gpu_expr_cross_by.py.

The main case is tests/test_gene_test_strata_host.py:strata_case -- the 'qc' dataset (3 000 cells x 40 samples, 10 batches, 2
covariates, cells dropped by the QC), 70 genes, data.obs['cluster'] with NaN and a level of one cell, one gene zero inside one
cluster, Nnull=120, seed=3 -- in dense-f32 and csr.  r and null_r are compared with the oracle's materialised null restricted to
each level (oracle_routes there: _oracle_null's recipe of tests/test_gpu_gene_test.py, level by level), r also with
gene_corr_strata.

Tolerance.  Within a level the coefficient's variance is smaller than over all cells, so the centring of the sample-space
route cancels more than in gene_test.  The largest difference between that route on numpy sums and the materialised route on
this very case, measured on the CPU, is the first line of profiles/gene_test_strata_parity.txt (7.2e-15; the host test keeps
the record honest); the tolerance here is min(100 x that, 1e-8), as R_TOL is in tests/test_gpu_gene_test.py.  The device's own
figures are printed beside it and go to the file CNA_GENE_TEST_STRATA_GPU_OUT names, when it is set."""
import os
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from test_gene_test_strata_host import cpu_parity, oracle_routes, recorded_cpu_diff, restated_bh, strata_case

pytestmark = pytest.mark.gpu

CPU_DIFF = recorded_cpu_diff()                # profiles/gene_test_strata_parity.txt, first line
R_TOL = min(100 * CPU_DIFF, 1e-8)
_seen = {}


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()
    if os.environ.get('CNA_GENE_TEST_STRATA_GPU_OUT') and _seen:
        with open(os.environ['CNA_GENE_TEST_STRATA_GPU_OUT'], 'w') as f:
            for k in sorted(_seen):
                f.write('%-70s %.3e\n' % (k, _seen[k]))


def _note(key, value):
    _seen[key] = max(_seen.get(key, 0.0), float(value))
    print('%s = %.3e (CPU %.3e, tolerance %.3e)' % (key, value, CPU_DIFF, R_TOL))


def as_form(E, form):
    return np.ascontiguousarray(E, dtype=np.float32) if form == 'dense-f32' else sp.csr_matrix(E)


def fresh(data, X=None, cols=('id', 'cluster')):
    d = type(data)(data.obs[list(cols)].copy(), data.obsp['connectivities'], X=X)
    return d


def compare(tag, frame, null_r, want, levels):
    """frame / null_r of gene_test_strata against the materialised r_all [L, G, 1 + P]: the same entries finite, within R_TOL;
    p and q exactly as recomputed from the returned arrays"""
    seen = list(levels)
    got = np.stack([frame[lv].values.T for lv in seen])
    ok = np.isfinite(want[..., 0])
    assert np.array_equal(np.isfinite(got[:, 0]), ok) and np.array_equal(np.isfinite(null_r).all(axis=2), ok)
    assert np.isnan(null_r[~ok]).all() and np.isnan(got.transpose(0, 2, 1)[~ok]).all()
    d_r = float(np.max(np.abs(got[:, 0][ok] - want[..., 0][ok])))
    d_null = float(np.max(np.abs(null_r[ok] - want[..., 1:][ok])))
    _note('%s: max |r - materialised oracle|' % tag, d_r)
    _note('%s: max |null_r - materialised oracle|' % tag, d_null)
    assert d_r <= R_TOL and d_null <= R_TOL, (tag, d_r, d_null, R_TOL)
    P = null_r.shape[2]
    for i, lv in enumerate(seen):
        r = frame[(lv, 'r')].values
        p = (1.0 + (np.abs(null_r[i]) >= np.abs(r)[:, None]).sum(axis=1)) / (P + 1.0)
        p[~ok[i]] = np.nan
        assert np.array_equal(frame[(lv, 'p')].values, p, equal_nan=True), lv
        assert np.array_equal(frame[(lv, 'q')].values, restated_bh(p), equal_nan=True), lv
        if ok[i].any():
            assert np.array_equal(frame[(lv, 'null_mean')].values[ok[i]], null_r[i][ok[i]].mean(axis=1))
    return got, ok


@pytest.mark.parametrize('form', ['dense-f32', 'csr'])
def test_main_case_against_the_materialised_oracle(eng, form):
    import cna_amd as cna
    data, y, batches, covs, E, call = strata_case()
    cpu_d, levels, kept_ref, want, _, _, cells = cpu_parity()
    assert abs(cpu_d - CPU_DIFF) <= 3 * CPU_DIFF
    d = fresh(data, X=as_form(E, form))
    d0 = fresh(data, cols=('id',))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        p0 = cna.tl.association(d0, y, 'id', batches=batches, covs=covs, engine=eng, **call)
        frame, null_r = cna.tl.gene_test_strata(d, y, 'id', 'cluster', batches=batches, covs=covs, return_null=True,
                                                engine=eng, **call)
        rcs = cna.tl.gene_corr_strata(d, 'cluster', 'coef', engine=eng)
    L = len(levels)
    assert null_r.shape == (L, 70, 120) and null_r.dtype == np.float64 and (frame.dtypes == np.float64).all()
    assert list(frame.columns.get_level_values(0).unique()) == list(levels) == list(rcs.columns)
    assert list(frame.columns.get_level_values(1)[:6]) == ['r', 'null_mean', 'null_sd', 'z', 'p', 'q']
    # data.obs as a plain call leaves it; the kept cells are the oracle's
    for k in ('coef', 'coef_fdr'):
        assert d.obs[k].values.tobytes() == d0.obs[k].values.tobytes(), k
    assert np.array_equal(np.isfinite(d0.obs['coef'].values), kept_ref) and (~kept_ref).any()
    assert frame.attrs['p'] == p0 and frame.attrs['n_null'] == 120
    assert list(frame.attrs['n_cells'].index) == list(levels) and np.array_equal(frame.attrs['n_cells'].values, cells)
    got, ok = compare('main %s' % form, frame, null_r, want, levels)
    seen = list(levels)
    assert not ok[seen.index('solo')].any() and not ok[seen.index('c2'), 3] and not ok[:, 1].any() and ok[seen.index('c2'), 4]
    # r is gene_corr_strata's
    r2 = rcs.values.T
    assert np.array_equal(np.isfinite(r2), ok)
    d_r = float(np.max(np.abs(got[:, 0][ok] - r2[ok])))
    _note('main %s: max |r - gene_corr_strata|' % form, d_r)
    assert d_r <= R_TOL


def test_second_phenotype_launches_nothing_and_a_changed_clustering_launches_again(eng):
    import cna_amd as cna
    data, y, batches, covs, E, call = strata_case()
    d = fresh(data, X=as_form(E, 'csr'))
    y2 = pd.Series(np.random.RandomState(4).randn(len(y)), index=y.index)
    kw = dict(batches=batches, covs=covs, return_null=True, engine=eng, **call)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        cna.tl.gene_test_strata(d, y, 'id', 'cluster', **kw)
        n0 = eng.cross_by_launches
        passes = []
        real = eng.gene_corr_by
        eng.gene_corr_by = lambda *a, **k: passes.append(1) or real(*a, **k)
        try:
            f2, null2 = cna.tl.gene_test_strata(d, y2, 'id', 'cluster', **kw)
        finally:
            del eng.gene_corr_by
        assert eng.cross_by_launches == n0 and passes == []            # a second phenotype: sample-space algebra only
        eng._cross_by_memo = None
        f3, null3 = cna.tl.gene_test_strata(d, y2, 'id', 'cluster', **kw)
        assert eng.cross_by_launches == n0 + 1 and null3.tobytes() == null2.tobytes() and f3.equals(f2)
        big = list(f3.attrs['n_cells'].sort_values().index[-3:])         # three levels that keep cells
        lab = d.obs['cluster'].values.copy()
        lab[lab == big[0]] = big[1]                                     # a changed clustering: one level merged into another
        d.obs['merged'] = lab
        f4 = cna.tl.gene_test_strata(d, y2, 'id', 'merged', batches=batches, covs=covs, engine=eng, **call)
        assert eng.cross_by_launches == n0 + 2 and big[0] not in f4.columns.get_level_values(0)
        assert f4[big[2]].equals(f3[big[2]]) and not f4[big[1]].equals(f3[big[1]])
        assert f4.attrs['n_cells'][big[1]] == f3.attrs['n_cells'][big[0]] + f3.attrs['n_cells'][big[1]]
        eng.drop_expression()
        cna.tl.gene_test_strata(d, y2, 'id', 'merged', batches=batches, covs=covs, engine=eng, **call)
        assert eng.cross_by_launches == n0 + 3                          # dropped: uploaded and taken again


_plain = {}


def plain_case(N):
    """(data, y, E): 3 000 cells x N samples, one batch, no covariates; the generating clusters with NaN as stratification"""
    if N not in _plain:
        from cna_amd import synth
        data, meta = synth.make_dataset(3000, N, k=15, seed=N)
        lab = np.array(['c%d' % c for c in meta['cluster']], dtype=object)
        lab[7::31] = np.nan
        data.obs['cluster'] = lab
        rs = np.random.RandomState(N + 1)
        E = (rs.gamma(2.0, 1.0, (3000, 70)) * (rs.rand(3000, 70) < 0.6)).astype(np.float32).astype(np.float64)
        E[:, 1] = 0.0
        _plain[N] = (data, meta['y'], E)
    return _plain[N]


def test_on_the_two_call_path(eng):
    """One batch, a seed, nsteps given: the association behind gene_test_strata takes the two-call path (tools/_fast.py)."""
    import cna_amd as cna
    from cna_amd.tools import _fast
    data, y, E = plain_case(24)
    call = dict(nsteps=3, Nnull=120, seed=3)
    d = fresh(data, X=E)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d0 = fresh(data, cols=('id',))
        p0 = cna.tl.association(d0, y, 'id', engine=eng, **call)       # (a graph new to the device goes up by the general path)
        before = _fast.stats['taken']
        frame, null_r = cna.tl.gene_test_strata(d, y, 'id', 'cluster', return_null=True, engine=eng, **call)
        assert _fast.stats['taken'] == before + 1                      # gene_test_strata's association took that path
        assert frame.attrs['p'] == p0
        for k in ('coef', 'coef_fdr'):
            assert d.obs[k].values.tobytes() == d0.obs[k].values.tobytes(), k
        levels, kept, want, _, cells = oracle_routes(d, y, None, None, E, 'cluster', 120, **call)
    assert kept.all() and np.array_equal(frame.attrs['n_cells'].values, cells)
    compare('two-call path', frame, null_r, want, levels)


def test_without_the_local_test(eng):
    import cna_amd as cna
    data, y, E = plain_case(24)
    d1, d2 = fresh(data, X=E), fresh(data, X=E)
    call = dict(nsteps=3, Nnull=80, seed=4, engine=eng)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        f1, n1 = cna.tl.gene_test_strata(d1, y, 'id', 'cluster', return_null=True, local_test=False, **call)
        assert 'coef' in d1.obs and 'coef_fdr' not in d1.obs
        f2, n2 = cna.tl.gene_test_strata(d2, y, 'id', 'cluster', return_null=True, **call)
    ok = np.isfinite(n2).all(axis=2)
    assert n1.shape == n2.shape and np.array_equal(np.isfinite(n1).all(axis=2), ok) and ok.any()
    assert d1.obs['coef'].values.tobytes() == d2.obs['coef'].values.tobytes()
    assert np.max(np.abs(n1 - n2)[ok]) <= R_TOL and f1.attrs['p'] == f2.attrs['p']
    assert np.nanmax(np.abs(f1.values - f2.values)[:, ::6]) <= R_TOL


@pytest.mark.parametrize('form', ['dense-f32', 'csr'])
def test_at_130_samples(eng, form):
    """130 samples: three 64-sample blocks of k_gram_by in either form; dense-f32: five sample tiles of k_xcb_dense, the last of
    2; csr: one masked cna_expr_cross per level (k_xc_sparse with three accumulators per lane)."""
    import cna_amd as cna
    data, y, E = plain_case(130)
    call = dict(nsteps=3, Nnull=50, seed=9)
    d = fresh(data, X=as_form(E, form))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        frame, null_r = cna.tl.gene_test_strata(d, y, 'id', 'cluster', return_null=True, engine=eng, **call)
        levels, kept, want, _, cells = oracle_routes(d, y, None, None, E, 'cluster', 50, **call)
    assert np.array_equal(kept, np.isfinite(d.obs['coef'].values)) and null_r.shape[1:] == (70, 50)
    compare('130 samples %s' % form, frame, null_r, want, levels)


def test_seed_none_leaves_the_generator_where_a_plain_call_leaves_it(eng):
    import cna_amd as cna
    data, y, E = plain_case(24)
    d = fresh(data, X=E)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a, na = cna.tl.gene_test_strata(d, y, 'id', 'cluster', nsteps=3, Nnull=60, seed=5, return_null=True, engine=eng)
        np.random.seed(5)
        b, nb = cna.tl.gene_test_strata(d, y, 'id', 'cluster', nsteps=3, Nnull=60, return_null=True, engine=eng)
        after_test = np.random.get_state()
        np.random.seed(5)
        cna.tl.association(fresh(data, cols=('id',)), y, 'id', nsteps=3, Nnull=60, engine=eng)
        after_plain = np.random.get_state()
    assert a.equals(b) and na.tobytes() == nb.tobytes()
    assert after_test[0] == after_plain[0] and np.array_equal(after_test[1], after_plain[1]) and after_test[2:] == after_plain[2:]
