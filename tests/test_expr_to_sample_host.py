"""cna.ut.expr_to_sample on the CPU: the rows, the columns, the refusals and their order, against an engine double defined
here whose `expr_to_bins` is the numpy restatement of cna_expr_to_bins (what the GPU tests compare the device with)."""
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp


# ------------------------------------------------------------------ the restatement (the oracle of the issue)
def restated_bins(X, codes, n_bins, what):
    """(sums float64[n_bins, genes], counts int64[n_bins]): for every row b, X[codes == b].astype(float64).sum(axis=0)
    (what = 0) or (X > 0)[codes == b].sum(axis=0) (what = 1); codes == -1 marks cells that are left out.  The mean and
    the fraction of the definition are these over the counts."""
    Xd = np.asarray(X.toarray() if sp.issparse(X) else X)
    codes = np.asarray(codes)
    sums = np.zeros((n_bins, Xd.shape[1]))
    counts = np.zeros(n_bins, dtype=np.int64)
    for b in range(n_bins):
        w = codes == b
        counts[b] = int(w.sum())
        if counts[b]:
            sums[b] = Xd[w].astype(np.float64).sum(axis=0) if what == 0 else (Xd > 0)[w].sum(axis=0)
    return sums, counts


def restated_frame(X, codes, n_bins, aggregate):
    """The definition itself, with numpy's own mean: NaN for a row without cells."""
    Xd = np.asarray(X.toarray() if sp.issparse(X) else X)
    out = np.empty((n_bins, Xd.shape[1]))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for b in range(n_bins):
            w = np.asarray(codes) == b
            if aggregate == 'mean':
                out[b] = Xd[w].astype(np.float64).mean(axis=0)
            elif aggregate == 'sum':
                out[b] = Xd[w].astype(np.float64).sum(axis=0)
            else:
                out[b] = (Xd > 0)[w].mean(axis=0)
    return out


# ------------------------------------------------------------------ the double
class BinsEngine:
    """Records every call; the matrix 'goes up' by reference and the reduction is `restated_bins`."""
    nranks = 1

    def __init__(self, nranks=1):
        self.nranks = nranks
        self.calls = []
        self.resident = None

    def ensure_expression(self, X):
        self.calls.append('ensure_expression')
        self.resident = X
        return True

    def expr_to_bins(self, codes, n_bins, what):
        self.calls.append(('expr_to_bins', n_bins, what))
        assert self.resident is not None and codes.dtype == np.int32 and codes.shape == (self.resident.shape[0],)
        assert codes.min() >= -1 and codes.max() < n_bins
        return restated_bins(self.resident, codes, n_bins, what)


def _data(X, var_names=None, layers=None, **cols):
    from cna_amd.synth import CellData
    n = len(next(iter(cols.values())))
    obs = pd.DataFrame(cols, index=pd.Index(['c%d' % i for i in range(n)]))
    var = None if var_names is None else pd.DataFrame(index=pd.Index(var_names))
    return CellData(obs, None, X=X, var=var, layers=layers)


def _ids(kind, n=300, n_samples=7, seed=0):
    rs = np.random.RandomState(seed)
    raw = rs.permutation(np.r_[np.arange(n_samples), rs.randint(0, n_samples, n - n_samples)])
    if kind == 'int':
        return raw * 3 + 5
    names = np.array(['s%02d' % (n_samples - i) for i in range(n_samples)])
    if kind == 'str':
        return names[raw]
    return pd.Categorical(names[raw], categories=sorted(names) + ['never'])


def _X(n, g, seed=0, dtype=np.float32):
    return np.ascontiguousarray(np.random.RandomState(seed).randn(n, g).astype(dtype))


def _ets(*a, **k):
    import cna_amd as cna
    return cna.ut.expr_to_sample(*a, **k)


# ------------------------------------------------------------------ rows
@pytest.mark.parametrize('kind', ['int', 'str', 'cat'])
def test_index_is_the_one_obs_to_sample_returns(kind):
    import cna_amd as cna
    ids = _ids(kind)
    X = _X(300, 11)
    d = _data(X, id=ids, depth=np.arange(300.0))
    e = BinsEngine()
    out = _ets(d, 'id', engine=e)
    ref = cna.ut.obs_to_sample(d, 'depth', 'id')
    assert list(out.index) == list(ref.index) and len(out) == 7
    assert list(out.index) == list(pd.unique(pd.Series(ids)))
    codes = pd.factorize(pd.Series(ids))[0]
    np.testing.assert_array_equal(out.values, restated_frame(X, codes, 7, 'mean'))
    assert out.values.dtype == np.float64
    # the per-cell column aggregated by obs_to_sample and the same column as a "gene" agree row for row
    d2 = _data(np.ascontiguousarray(np.arange(300.0)[:, None]), id=ids, depth=np.arange(300.0))
    np.testing.assert_allclose(_ets(d2, 'id', engine=BinsEngine()).values[:, 0], ref['depth'].values, rtol=1e-13)


def test_groupby_gives_every_pair_sample_major():
    rs = np.random.RandomState(1)
    n = 400
    ids = _ids('str', n=n, n_samples=5, seed=1)
    lev = np.array(['b', 'a', 'c'])[rs.randint(0, 3, n)]
    first_sample, first_level = ids[0], 'c'
    lev[ids == first_sample] = np.where(lev[ids == first_sample] == first_level, 'a', lev[ids == first_sample])   # an empty pair
    X = _X(n, 6, seed=1)
    d = _data(X, id=ids, leiden=lev)
    for agg, empty in (('mean', np.nan), ('frac', np.nan), ('sum', 0.0)):
        with warnings.catch_warnings():
            warnings.simplefilter('error')                       # no numpy warning escapes
            out, counts = _ets(d, 'id', groupby='leiden', aggregate=agg, return_counts=True, engine=BinsEngine())
        samples, levels = list(pd.unique(ids)), list(pd.unique(lev))
        assert isinstance(out.index, pd.MultiIndex) and list(out.index.names) == ['id', 'leiden']
        assert list(out.index) == [(s, l) for s in samples for l in levels] and len(out) == 15
        assert counts.index.equals(out.index) and counts.dtype == np.int64
        assert counts[(first_sample, first_level)] == 0
        row = out.loc[(first_sample, first_level)].values
        assert np.isnan(row).all() if np.isnan(empty) else (row == 0).all()
        codes = pd.factorize(ids)[0] * 3 + pd.factorize(lev)[0]
        np.testing.assert_array_equal(out.values, restated_frame(X, codes, 15, agg))
        want = pd.Series(list(zip(ids, lev))).value_counts()
        for key, c in counts.items():
            assert c == want.get(key, 0)


def test_nan_ids_and_levels_are_left_out():
    n = 200
    ids = _ids('int', n=n, n_samples=4, seed=2).astype(float)
    lev = np.array(['x', 'y'], dtype=object)[np.arange(n) % 2]
    ids[[3, 50, 51]] = np.nan
    lev[[7, 50]] = None
    X = _X(n, 5, seed=2)
    d = _data(X, id=ids, leiden=lev)
    out, counts = _ets(d, 'id', return_counts=True, engine=BinsEngine())
    assert len(out) == 4 and not out.index.isna().any() and counts.sum() == n - 3
    want = pd.DataFrame(X.astype(np.float64)).groupby(ids).mean()
    np.testing.assert_allclose(out.values, want.loc[list(out.index)].values, rtol=1e-12, atol=1e-15)
    out2, counts2 = _ets(d, 'id', groupby='leiden', return_counts=True, engine=BinsEngine())
    assert len(out2) == 8 and counts2.sum() == n - 4
    want2 = pd.DataFrame(X.astype(np.float64)).groupby([ids, lev]).mean()
    np.testing.assert_allclose(out2.values, want2.loc[list(out2.index)].values, rtol=1e-12, atol=1e-15)


def test_return_counts_agrees_with_value_counts():
    ids = _ids('str', seed=3)
    d = _data(_X(300, 4), id=ids)
    out, counts = _ets(d, 'id', return_counts=True, engine=BinsEngine())
    vc = pd.Series(ids).value_counts()
    assert counts.dtype == np.int64 and counts.index.equals(out.index)
    np.testing.assert_array_equal(counts.values, vc.loc[list(counts.index)].values)


def test_aggregates_against_the_definition():
    ids = _ids('int', seed=4)
    X = _X(300, 9, seed=4)
    X[X < 0.3] = 0.0
    X[5, 2], X[9, 3] = np.nan, np.inf
    M = sp.csr_matrix(X)
    M.data[::5] = 0.0                                           # explicit zeros
    codes = pd.factorize(ids)[0]
    for mat in (X, M, M.tocsc()):
        d = _data(mat, id=ids)
        for agg in ('mean', 'sum', 'frac'):
            got = _ets(d, 'id', aggregate=agg, engine=BinsEngine()).values
            np.testing.assert_array_equal(got, restated_frame(mat, codes, 7, agg))
    got = _ets(_data(X, id=ids), 'id', aggregate='sum', engine=BinsEngine()).values
    assert np.isnan(got).sum() == 1 and np.isinf(got).sum() == 1
    assert np.isnan(got[codes[5], 2]) and np.isinf(got[codes[9], 3])


# ------------------------------------------------------------------ columns
def test_var_names_give_the_columns_and_a_wrong_length_falls_back():
    ids = _ids('int')
    X = _X(300, 3)
    out = _ets(_data(X, var_names=['g_a', 'g_b', 'g_c'], id=ids), 'id', engine=BinsEngine())
    assert list(out.columns) == ['g_a', 'g_b', 'g_c']
    out = _ets(_data(X, var_names=['g_a', 'g_b'], id=ids), 'id', engine=BinsEngine())
    assert out.columns.equals(pd.RangeIndex(3))
    out = _ets(_data(X, id=ids), 'id', engine=BinsEngine())
    assert out.columns.equals(pd.RangeIndex(3))


def test_layer_is_honoured():
    ids = _ids('int')
    X, L = _X(300, 3, seed=1), _X(300, 5, seed=2, dtype=np.float64)
    d = _data(X, layers={'counts': L}, id=ids)
    e = BinsEngine()
    out = _ets(d, 'id', layer='counts', engine=e)
    assert e.resident is L and out.shape == (7, 5)
    np.testing.assert_array_equal(out.values, restated_frame(L, pd.factorize(ids)[0], 7, 'mean'))
    with pytest.raises(KeyError):
        _ets(d, 'id', layer='nope', engine=e)


# ------------------------------------------------------------------ refusals, all before anything is uploaded
def test_only_mean_sum_and_frac_are_accepted():
    d = _data(_X(300, 3), id=_ids('int'))
    for agg in ('mean', 'sum', 'frac'):
        assert _ets(d, 'id', aggregate=agg, engine=BinsEngine()).shape == (7, 3)
    for agg in ('median', 'max', None, np.mean, 'Mean'):
        e = BinsEngine()
        with pytest.raises(ValueError, match='aggregate'):
            _ets(d, 'id', aggregate=agg, engine=e)
        assert e.calls == []


def test_every_refusal_comes_before_the_upload():
    n = 5000
    X = _X(n, 2)
    e = BinsEngine()
    with pytest.raises(ValueError, match=r'4097 samples x 1 levels'):
        _ets(_data(X, id=np.arange(n) % 4097), 'id', engine=e)
    with pytest.raises(ValueError, match=r'100 samples x 41 levels = 4100'):
        _ets(_data(X, id=np.arange(n) % 100, leiden=np.arange(n) % 41), 'id', groupby='leiden', engine=e)
    with pytest.raises(ValueError, match=r'0 samples x 1 levels'):
        _ets(_data(X, id=np.full(n, np.nan)), 'id', engine=e)
    with pytest.raises(KeyError):
        _ets(_data(X, id=np.arange(n) % 3), 'sample', engine=e)
    with pytest.raises(KeyError):
        _ets(_data(X, id=np.arange(n) % 3), 'id', groupby='leiden', engine=e)
    with pytest.raises(ValueError, match='data.X is missing'):
        _ets(_data(None, id=np.arange(n) % 3), 'id', engine=e)
    with pytest.raises(TypeError):
        _ets(_data(X.astype(np.int32), id=np.arange(n) % 3), 'id', engine=e)
    with pytest.raises(TypeError):
        _ets(_data(np.asfortranarray(X), id=np.arange(n) % 3), 'id', engine=e)
    with pytest.raises(ValueError, match='rows'):
        _ets(_data(X[:-1].copy(), id=np.arange(n) % 3), 'id', engine=e)
    with pytest.raises(TypeError):
        _ets(_data(sp.coo_matrix(X), id=np.arange(n) % 3), 'id', engine=e)
    assert e.calls == []
    out = _ets(_data(X, id=np.arange(n) % 4096), 'id', engine=e)          # the largest row count passes
    assert out.shape == (4096, 2) and e.calls == ['ensure_expression', ('expr_to_bins', 4096, 0)]


def test_a_shard_and_a_multi_rank_engine_are_refused():
    d = _data(_X(300, 3), id=_ids('int'))
    e = BinsEngine(nranks=2)
    with pytest.raises(NotImplementedError):
        _ets(d, 'id', engine=e)
    d.uns['cna_shard'] = {'row0': 0, 'n_global': 600}
    e1 = BinsEngine()
    with pytest.raises(NotImplementedError):
        _ets(d, 'id', engine=e1)
    assert e.calls == [] and e1.calls == []


def test_frac_uses_the_count_path_and_is_exported():
    import cna_amd as cna
    assert 'expr_to_sample' in cna.ut.__all__ and 'obs_to_sample' in cna.ut.__all__
    e = BinsEngine()
    _ets(_data(_X(300, 3), id=_ids('int')), 'id', aggregate='frac', engine=e)
    assert e.calls[-1] == ('expr_to_bins', 7, 1)
    from cna_amd import _ffi
    assert 'cna_expr_to_bins' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'cna_expr_to_bins')
