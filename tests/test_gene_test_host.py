"""cna.tl.gene_test on the CPU: argument checks and the sample-space algebra of its step 5 as pure functions.

`null_correlations` gets the null correlations of every gene from W = E^T X, rho, sx, sxx, m and Gamma = X^T X without ever
forming the cells x permutations matrix.  Here that matrix IS formed -- C = R^T Z / N, then np.corrcoef per gene and
column -- on random R (24 samples x 500 cells) and E (500 x 40), and the two are compared.  Both are float64 computations of
the same quantity with condition number ~1 (centred sums of O(1) terms over 500 cells), so they agree to a small multiple
of 500 * 2^-53 ~ 6e-14; the bound asserted is 1e-12.  The difference measured goes to the file CNA_GENE_TEST_PARITY_OUT
names, when it is set (profiles/r09_gene_test_parity.txt holds such a run's line), and the GPU test's tolerance is 100 x
that figure, never looser than 1e-8 (tests/test_gpu_gene_test.py)."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from cna_amd.tools._gene_test import benjamini_hochberg, null_correlations, permutation_stats

FACTORISED_BOUND = 1e-12


def materialised_null(R, E, Z):
    """genes x P: np.corrcoef of every gene's expression (E: cells x genes) with every null coefficient vector
    c_p = R^T z_p / N (R: samples x cells, Z: samples x P), the cells x P matrix formed."""
    C = R.T @ Z / R.shape[0]
    out = np.empty((E.shape[1], Z.shape[1]))
    for g in range(E.shape[1]):
        for p in range(Z.shape[1]):
            out[g, p] = np.corrcoef(E[:, g], C[:, p])[0, 1]
    return out


def factorised_null(R, E, Z):
    X = np.ascontiguousarray(R.T)                             # the working matrix: cells x samples
    return null_correlations(E.T @ X, X.sum(axis=0), E.sum(axis=0), (E * E).sum(axis=0), E.shape[0], X.T @ X, Z)


def restated_bh(p):
    """Benjamini-Hochberg in ten lines: the i-th smallest of n p-values times n / i, made monotone from the top."""
    p = np.asarray(p, dtype=float)
    q = np.full(len(p), np.nan)
    idx = [i for i in range(len(p)) if np.isfinite(p[i])]
    idx.sort(key=lambda i: p[i])
    running = 1.0
    for rank in range(len(idx), 0, -1):
        i = idx[rank - 1]
        running = min(running, p[i] * len(idx) / rank)
        q[i] = running
    return q


def test_factorised_equals_materialised():
    rs = np.random.RandomState(11)
    R = rs.randn(24, 500)
    E = rs.gamma(2.0, 1.0, (500, 40)) * (rs.rand(500, 40) < 0.6)
    Z = rs.randn(24, 30)
    Z = Z / Z.std(axis=0, ddof=1)
    got, want = factorised_null(R, E, Z), materialised_null(R, E, Z)
    diff = float(np.max(np.abs(got - want)))
    print('factorised against materialised, max |dr| = %.3e' % diff)
    out = os.environ.get('CNA_GENE_TEST_PARITY_OUT')
    if out:
        with open(out, 'w') as f:
            f.write('null_correlations against np.corrcoef on the materialised cells x P matrix (tests/test_gene_test_host.py; '
                    'R 24 x 500, E 500 x 40, 30 columns): max |dr| = %.3e (bound %.0e)\n' % (diff, FACTORISED_BOUND))
    assert diff <= FACTORISED_BOUND


def test_offsets_do_not_cancel():
    """Large means in E and in R: the centring (W - xbar rho^T, Gamma - rho rho^T / m) keeps the result at rounding level
    of the uncentred sums."""
    rs = np.random.RandomState(12)
    R = rs.randn(24, 500) + 3.0
    E = rs.rand(500, 7) + 50.0
    Z = rs.randn(24, 5)
    assert np.max(np.abs(factorised_null(R, E, Z) - materialised_null(R, E, Z))) <= 1e-9


def test_constant_gene_and_constant_coefficient_give_nan():
    rs = np.random.RandomState(13)
    R = rs.randn(10, 200)
    E = rs.rand(200, 4)
    E[:, 1] = 0.0
    E[:, 2] = 2.5
    Z = rs.randn(10, 3)
    Z[:, 2] = 0.0
    r = factorised_null(R, E, Z)
    assert np.isnan(r[1]).all() and np.isnan(r[:, 2]).all()
    assert np.isfinite(r[[0, 3]][:, :2]).all()


def test_p_and_q_follow_from_r_and_null_r_exactly():
    rs = np.random.RandomState(14)
    null_r = np.round(rs.uniform(-1, 1, (60, 99)), 2)          # ties with |r| on purpose
    r = np.round(rs.uniform(-1, 1, 60), 2)
    r[5] = np.nan
    null_r[5] = np.nan
    mean, sd, z, p, q = permutation_stats(r, null_r)
    for g in range(60):
        if g == 5:
            assert np.isnan(p[g]) and np.isnan(q[g]) and np.isnan(z[g])
            continue
        hits = sum(1 for v in null_r[g] if abs(v) >= abs(r[g]))
        assert p[g] == (1 + hits) / 100.0
        assert mean[g] == null_r[g].mean() and sd[g] == null_r[g].std(ddof=1)
        assert z[g] == (r[g] - mean[g]) / sd[g]
    assert np.array_equal(q, restated_bh(p), equal_nan=True)
    assert p[np.isfinite(p)].min() >= 1 / 100.0


def test_bh_against_the_restatement():
    rs = np.random.RandomState(15)
    for n in (1, 2, 17, 200):
        p = rs.rand(n)
        p[rs.rand(n) < 0.2] = np.nan
        p[:n // 3] = np.round(p[:n // 3], 1)                   # ties
        got, want = benjamini_hochberg(p), restated_bh(p)
        assert np.allclose(got, want, rtol=0, atol=0, equal_nan=True)
        ok = np.isfinite(p)
        assert (got[ok] >= p[ok]).all() and (got[ok] <= 1).all()
    assert np.isnan(benjamini_hochberg(np.array([np.nan, np.nan]))).all()
    assert benjamini_hochberg(np.array([0.01, 0.04, 0.03])).tolist() == [0.03, 0.04, 0.04]


# ------------------------------------------------------------------ argument errors: before anything runs
class _Refuses:
    """An engine nothing may be asked of."""
    nranks = 1

    def __getattr__(self, name):
        raise AssertionError('engine.%s used although the arguments are wrong' % name)


@pytest.fixture(scope='module')
def demo():
    from cna_amd import synth
    data, samplem = synth.make_demo_like(n_samples=20, n_genes=30, cells_per_sample=100, seed=3, keep_expression=True)
    return data, samplem


def _with_X(data, X):
    from cna_amd.synth import CellData
    return CellData(data.obs.copy(), data.obsp['connectivities'], X=X)


def test_bad_expression_raises_before_anything_runs(demo):
    import cna_amd as cna
    data, samplem = demo
    y = samplem.iloc[:, 0].astype(float)
    eng = _Refuses()
    n = len(data.obs)
    for bad, exc in ((data.X.astype(np.float16), TypeError), (data.X.astype(np.int32), TypeError),
                     (sp.coo_matrix(data.X), TypeError), (data.X.tolist(), TypeError),
                     (np.asfortranarray(data.X), TypeError), (data.X[:n - 1], ValueError), (data.X[:, 0], ValueError),
                     (None, ValueError)):
        with pytest.raises(exc):
            cna.tl.gene_test(_with_X(data, bad), y, 'id', engine=eng)
    with pytest.raises(KeyError):
        cna.tl.gene_test(data, y, 'id', layer='missing', engine=eng)
    assert 'coef' not in data.obs


def test_sharded_data_and_multi_rank_engines_are_refused(demo):
    import cna_amd as cna
    from cna_amd import dist
    data, samplem = demo
    y = samplem.iloc[:, 0].astype(float)
    part = dist.shard(data, rank=0, nranks=2)
    part.X = data.X[:len(part.obs)]
    with pytest.raises(NotImplementedError):
        cna.tl.gene_test(part, y, 'id', engine=_Refuses())
    two = _Refuses()
    two.__dict__['nranks'] = 2
    with pytest.raises(NotImplementedError):
        cna.tl.gene_test(data, y, 'id', engine=two)


def test_the_library_declares_the_entry_point():
    from cna_amd import _ffi
    assert 'cna_expr_cross' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'cna_expr_cross')
    assert 'cna_x_generation' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'cna_x_generation')


def test_x_row_of_cells_inverts_kept_to_user():
    """The map the engine hands cna_expr_cross: for every combination of device order and selection, X[xrow[i]] is the
    row kept_to_user() puts at cell i's place."""
    from cna_amd._order import CellOrder
    rs = np.random.RandomState(16)
    n = 50
    for perm in (None, rs.permutation(n).astype(np.int64)):
        for keep in (None, rs.rand(n) < 0.7):
            o = CellOrder()
            o.perm, o.n, o.row0, o.n_local, o.nranks = perm, n, 0, n, 1
            o._x_is_selection = True
            if keep is None:
                o._keep_dev, o.x_rows_total = None, n
            else:
                o.local_keep(keep)
                o.x_rows_total = int(keep.sum())
            xrow = o.x_row_of_cells()
            kept = np.ones(n, dtype=bool) if keep is None else keep
            assert xrow.dtype == np.int64 and (xrow[~kept] == -1).all()
            assert sorted(xrow[kept]) == list(range(int(kept.sum())))
            # device rows of X: the kept cells in device order
            dev_cells = np.arange(n) if perm is None else perm
            x_cells = dev_cells[kept[dev_cells]]                # caller's cell of every X row
            assert np.array_equal(x_cells[xrow[kept]], np.flatnonzero(kept))
    o = CellOrder()
    o.perm, o.n, o._x_is_selection, o.x_rows_total = rs.permutation(n), n, False, 7
    assert np.array_equal(o.x_row_of_cells(), np.arange(7))


# ------------------------------------------------------------------ the whole call on the numpy engine double
def _double():
    from fake_engine import FakeEngine
    from test_gene_corr_host import restated_gene_corr

    class CrossEngine(FakeEngine):
        """FakeEngine plus numpy restatements of the four engine calls gene_test adds to an association."""
        cross_launches = 0

        def ensure_expression(self, X):
            self.E = np.asarray(X, dtype=np.float64)

        def gram_held(self):
            return self.gram()

        def cross_extra(self):
            return self.__dict__.setdefault('_extra', {})

        def gene_corr(self, V):
            return restated_gene_corr(self.E, V)

        def expr_cross(self, content=None):
            from cna_amd._ffi import MAT_X
            self.cross_launches += 1
            xrow = self.x_row_of_cells()
            X = self.fetch_matrix(MAT_X)                       # rows in device order
            k = xrow >= 0
            EK, XK = self.E[k], X[xrow[k]]
            return EK.T @ XK, XK.sum(axis=0), EK.sum(axis=0), (EK * EK).sum(axis=0), int(k.sum())
    return CrossEngine(order='random')


def test_whole_call_against_the_materialised_oracle():
    """40 samples in 10 batches, 2 covariates, one population drawn from one batch's samples (the recipe of fixture
    c12_batchy_qc: with fewer than 8 batches no batch kurtosis can reach the QC's threshold of 6), a random device order:
    r equals gene_corr, null_r the np.corrcoef-like restatement on the oracle's namresid, M and draw."""
    import warnings
    import cna_amd as cna
    from cna_amd import synth
    from oracle import cna_oracle as orc
    data, meta = synth.make_dataset(3000, 40, k=15, seed=11, n_batches=10, n_covs=2, builder='cpu')
    cl, b = meta['cluster'], meta['batches'].values
    sid = np.asarray(data.obs['id']).copy()
    target = np.flatnonzero(cl == np.bincount(cl).argmax())
    sid[target] = np.random.RandomState(3).choice(np.flatnonzero(b == 0), size=len(target))
    data.obs['id'] = sid
    rs = np.random.RandomState(0)
    E = rs.gamma(2.0, 1.0, (3000, 20)) * (rs.rand(3000, 20) < 0.6)
    E[:, 1] = 0.0
    data.X = E
    eng = _double()
    call = dict(nsteps=3, Nnull=60, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        frame, null_r = cna.tl.gene_test(data, meta['y'], 'id', batches=meta['batches'], covs=meta['covs'], return_null=True,
                                         engine=eng, **call)
        rc = cna.tl.gene_corr(data, 'coef', engine=eng)['coef'].values
    ref = orc.association(data, meta['y'], 'id', batches=meta['batches'], covs=meta['covs'], mode='f64', **call)
    kept = ref['kept']
    assert 0 < (~kept).sum() < 3000 and eng.perm is not None and eng.cross_launches == 1
    Z = ref['M'].dot(ref['y_perm'][:, :60])
    Z = Z / Z.std(axis=0, ddof=1)
    Cn = ref['namresid'].dot(Z) / ref['namresid'].shape[1]
    Ec, Cc = E[kept] - E[kept].mean(axis=0), Cn - Cn.mean(axis=0)
    with np.errstate(all='ignore'):
        want = (Ec.T @ Cc) / np.sqrt(np.outer((Ec * Ec).sum(axis=0), (Cc * Cc).sum(axis=0)))
    ok = np.arange(20) != 1
    assert np.isnan(frame.values[1]).all() and np.isnan(null_r[1]).all() and np.isfinite(frame.values[ok]).all()
    assert np.max(np.abs(frame['r'].values[ok] - rc[ok])) <= 1e-12
    assert np.max(np.abs(null_r[ok] - want[ok])) <= 1e-12
    mean, sd, z, p, q = permutation_stats(frame['r'].values, null_r)
    assert np.array_equal(frame['p'].values, p, equal_nan=True) and np.array_equal(frame['q'].values, q, equal_nan=True)


def test_the_memo_carries_over_on_equal_content_only():
    """Engine.expr_cross's memo on a stand-in for the library: the same key serves the memo; a moved key (every
    association rebuilds X) serves it only under an equal, non-empty content word; other content, no content, or another
    upload of the expression matrix take the pass again; the extra dict goes with the memo."""
    import types
    from cna_amd.engine import Engine

    calls = []
    lib = types.SimpleNamespace(cna_expr_cross=lambda *a: (calls.append(1), 0)[1])
    e = types.SimpleNamespace(nranks=1, view_local=False, lib=lib, h=None, x_epoch=1, _cross_memo=None, cross_launches=0,
                              gen=1, uploads=1)
    e.expression_shape = lambda: dict(format='dense', uploads=e.uploads, n_genes=3)
    e.x_generation = lambda: e.gen
    e.matrix_shape = lambda which: (5, 2)
    e.x_row_of_cells = lambda: np.arange(5)
    cross = types.MethodType(Engine.expr_cross, e)
    extra = types.MethodType(Engine.cross_extra, e)
    a = cross(content=('A',))
    extra()['constant'] = 'kept'
    assert cross(content=('A',)) is a and cross() is a and e.cross_launches == 1
    e.x_epoch, e.gen = 2, 5                                    # a further association: X rebuilt
    assert cross(content=('A',)) is a and e.cross_launches == 1 and extra() == {'constant': 'kept'}
    e.x_epoch = 3
    b = cross(content=('B',))                                  # other covariates: other content
    assert b is not a and e.cross_launches == 2 and extra() == {}
    e.x_epoch = 4
    assert cross(content=None) is not b and e.cross_launches == 3      # nothing vouches for the rebuilt X
    e.gen = 6                                                  # X voided in place (no new epoch)
    cross(content=None)
    assert e.cross_launches == 4
    c = cross(content=('C',))
    assert e.cross_launches == 4                               # same key: the memo, whatever the content word
    e.uploads, e.x_epoch = 2, 5
    assert cross(content=('C',)) is not c and e.cross_launches == 5    # another expression matrix
    n = e.cross_launches
    cross(xrow=np.arange(5))                                   # an explicit map: neither read nor kept
    assert e.cross_launches == n + 1 and cross(content=('C',)) is not None and e.cross_launches == n + 1
