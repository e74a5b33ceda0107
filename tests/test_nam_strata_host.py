"""cna.tl.nam_strata on the CPU: the levels, the weights, the frames and the refusals of the host side, against the
engine double of tests/fake_engine.py with a `matrix_to_bins` defined here: the numpy restatement of cna_matrix_to_bins
over the double's NAM (what the GPU tests compare the device with)."""
import numpy as np
import pandas as pd
import pytest

from fake_engine import FakeEngine, MAT_NAM


# ------------------------------------------------------------------ the restatement (the oracle of the issue)
def restated_bins(M, codes, W, n_bins):
    """(sums float64[max(q, 1), n_bins, cols], n int64[max(q, 1), n_bins]) over the rows of M: row r contributes to weight
    column j when codes[r] >= 0 and W[j, r] is finite and not zero (W None: one column of ones); a row that does not
    contribute is not multiplied."""
    M = np.asarray(M, dtype=np.float64)
    codes = np.asarray(codes)
    W = np.ones((1, len(codes))) if W is None else np.asarray(W, dtype=np.float64)
    sums = np.zeros((len(W), n_bins, M.shape[1]))
    cnt = np.zeros((len(W), n_bins), dtype=np.int64)
    for j, w in enumerate(W):
        ok = (codes >= 0) & np.isfinite(w) & (w != 0)
        for b in range(n_bins):
            rows = np.flatnonzero(ok & (codes == b))
            cnt[j, b] = len(rows)
            if len(rows):
                sums[j, b] = (w[rows, None] * M[rows]).sum(axis=0)
    return sums, cnt


class BinsFake(FakeEngine):
    """FakeEngine plus matrix_to_bins over its NAM (device order inside, caller's order at the boundary)."""

    def __init__(self, order='random'):
        super().__init__(order=order)
        self.reuse_nam = True

    def matrix_to_bins(self, which, codes, W=None, n_bins=None):
        self.calls.append(('matrix_to_bins', which, None if W is None else W.shape[0], n_bins))
        assert which == MAT_NAM and codes.dtype == np.int32 and codes.shape == (self.n,)
        assert W is None or (W.dtype == np.float64 and W.shape[1] == self.n)
        assert codes.min() >= -1 and codes.max() < n_bins
        nam = self.cells_to_user(self.nam)
        if getattr(self, 'poison', None) is not None:
            nam = nam.copy()
            nam[self.poison] = np.nan
        return restated_bins(nam, codes, W, n_bins)

    def walks(self):
        return sum(1 for c in self.calls if c[0] == 'nam_step')


N_CELLS, N_SAMPLES = 500, 6


@pytest.fixture(scope='module')
def case():
    """One small dataset with its NAM (cells x samples, caller's order) from cna.tl.nam on the double."""
    import cna_amd as cna
    from cna_amd import synth
    data, _ = synth.make_dataset(N_CELLS, N_SAMPLES, k=10, seed=5, builder='cpu')
    rs = np.random.RandomState(0)
    lev = np.array(['c3', 'c1', 'c2', 'c0'])[rs.permutation(np.r_[np.arange(4), rs.randint(0, 4, N_CELLS - 4)])].astype(object)
    data.obs['leiden'] = lev
    data.obs['w1'] = rs.randn(N_CELLS)
    data.obs['w2'] = rs.rand(N_CELLS)
    data.obs['coef'] = rs.randn(N_CELLS) * 0.1
    data.obs['text'] = ['a'] * N_CELLS
    frame, keep = cna.tl.nam(data, 'id', nsteps=3, engine=BinsFake())
    assert keep.all()
    return data, frame.values.T.copy(), frame.index


def _ns(*a, **k):
    import cna_amd as cna
    return cna.tl.nam_strata(*a, nsteps=3, **k)


def _with(data, **cols):
    from cna_amd.synth import CellData
    obs = data.obs.copy()
    for k, v in cols.items():
        obs[k] = v
    return CellData(obs, data.obsp['connectivities'])


def _want(nam, lev, w=None, levels=None):
    """samples x levels by the definition, levels in order of first appearance (or as given)"""
    levels = list(pd.unique(pd.Series(lev).dropna())) if levels is None else levels
    w = np.ones(len(nam)) if w is None else np.asarray(w, dtype=np.float64)
    out = np.zeros((nam.shape[1], len(levels)))
    for b, L in enumerate(levels):
        rows = np.flatnonzero((np.asarray(lev, dtype=object) == L) & np.isfinite(w) & (w != 0))
        out[:, b] = (w[rows, None] * nam[rows]).sum(axis=0)
    return levels, out


def test_levels_in_order_of_first_appearance_rows_as_nam_and_rows_sum_to_one(case):
    data, nam, index = case
    got = _ns(data, 'leiden', 'id', engine=BinsFake())
    levels, want = _want(nam, data.obs['leiden'].values)
    assert list(got.columns) == levels and levels[0] == data.obs['leiden'].values[0] and got.columns.name == 'leiden'
    assert got.index.equals(index) and got.index.name == 'id'
    np.testing.assert_allclose(got.values, want, rtol=0, atol=1e-13)
    assert np.abs(got.values.sum(axis=1) - 1.0).max() <= 1e-12        # NAM rows sum to 1


def test_nan_levels_and_keep_leave_cells_out(case):
    data, nam, _ = case
    lev = data.obs['leiden'].values.copy()
    lev[::7] = None
    lev[3] = np.nan
    keep = np.random.RandomState(1).rand(N_CELLS) > 0.3
    d = _with(data, leiden=lev)
    got, counts = _ns(d, 'leiden', 'id', keep=keep, return_counts=True, engine=BinsFake())
    masked = np.where(keep, lev, None)
    levels = list(pd.unique(pd.Series(lev).dropna()))       # by the column itself: keep does not reorder the levels
    assert list(got.columns) == levels
    want = _want(nam, masked, levels=levels)[1]
    np.testing.assert_allclose(got.values, want, rtol=0, atol=1e-13)
    assert counts.dtypes.tolist() == [np.int64] and list(counts.columns) == ['n'] and counts.index.equals(got.columns)
    assert counts['n'].tolist() == [int(((masked == L) & keep).sum()) for L in levels]
    with pytest.raises(ValueError):
        _ns(d, 'leiden', 'id', keep=keep[:-1], engine=BinsFake())
    with pytest.raises(ValueError):
        _ns(d, 'leiden', 'id', keep=keep.astype(float), engine=BinsFake())


def test_weights_as_name_list_and_none_in_one_pass(case):
    data, nam, _ = case
    lev = data.obs['leiden'].values
    e = BinsFake()
    one = _ns(data, 'leiden', 'id', weights='w1', engine=e)
    assert isinstance(one, pd.DataFrame)
    np.testing.assert_allclose(one.values, _want(nam, lev, data.obs['w1'].values)[1], rtol=0, atol=1e-12)
    e = BinsFake()
    both, counts = _ns(data, 'leiden', 'id', weights=['w1', 'w2'], return_counts=True, engine=e)
    assert list(both) == ['w1', 'w2'] and list(counts.columns) == ['w1', 'w2']
    assert [c for c in e.calls if c[0] == 'matrix_to_bins'] == [('matrix_to_bins', MAT_NAM, 2, 4)]      # ONE device pass
    for k in ('w1', 'w2'):
        np.testing.assert_allclose(both[k].values, _want(nam, lev, data.obs[k].values)[1], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(both['w1'].values, one.values)
    lone = _ns(data, 'leiden', 'id', weights=['w2'], engine=BinsFake())
    assert isinstance(lone, dict) and list(lone) == ['w2']
    with pytest.raises(TypeError):
        _ns(data, 'leiden', 'id', weights='text', engine=BinsFake())
    with pytest.raises(KeyError):
        _ns(data, 'leiden', 'id', weights=['w1', 'absent'], engine=BinsFake())
    with pytest.raises(KeyError):
        _ns(data, 'absent', 'id', engine=BinsFake())


def test_nan_weight_leaves_the_cell_out_of_that_column_only(case):
    data, nam, _ = case
    lev = data.obs['leiden'].values
    w1 = data.obs['w1'].values.copy()
    w1[[2, 50, 51]] = [np.nan, np.inf, -np.inf]
    d = _with(data, w1=w1)
    both, counts = _ns(d, 'leiden', 'id', weights=['w1', 'w2'], return_counts=True, engine=BinsFake())
    assert np.isfinite(both['w1'].values).all()
    np.testing.assert_allclose(both['w1'].values, _want(nam, lev, w1)[1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(both['w2'].values, _want(nam, lev, data.obs['w2'].values)[1], rtol=0, atol=1e-12)
    levels = list(both['w1'].columns)
    assert counts['w2'].tolist() == [int((lev == L).sum()) for L in levels]
    assert counts['w1'].sum() == N_CELLS - 3 and counts['w2'].sum() == N_CELLS


def test_zero_weight_against_a_nan_entry_adds_nothing(case):
    data, nam, _ = case
    lev = data.obs['leiden'].values
    w = np.ones(N_CELLS)
    w[10] = 0.0
    e = BinsFake()
    e.poison = 10                                           # row 10 of the NAM is NaN
    got = _ns(_with(data, w1=w), 'leiden', 'id', weights='w1', engine=e)
    assert np.isfinite(got.values).all()
    np.testing.assert_allclose(got.values, _want(nam, lev, w)[1], rtol=0, atol=1e-13)
    e = BinsFake()
    e.poison = 10
    bad = _ns(data, 'leiden', 'id', engine=e)                 # without the zero the NaN reaches its own level, and only it
    assert np.isnan(bad[lev[10]].values).all() and np.isfinite(bad.drop(columns=[lev[10]]).values).all()


def test_sign_of_with_and_without_the_fdr_column(case):
    data, nam, _ = case
    lev = data.obs['leiden'].values
    coef = data.obs['coef'].values.copy()
    coef[::11] = np.nan
    fdr = np.random.RandomState(3).rand(N_CELLS) * 0.3
    fdr[5] = np.nan
    d0 = _with(data, coef=coef)
    r0, c0 = _ns(d0, 'leiden', 'id', sign_of='coef', return_counts=True, engine=BinsFake())
    assert list(r0) == ['pos', 'neg'] and list(c0.columns) == ['pos', 'neg']
    with np.errstate(invalid='ignore'):
        np.testing.assert_allclose(r0['pos'].values, _want(nam, lev, (coef > 0).astype(float))[1], rtol=0, atol=1e-13)
        np.testing.assert_allclose(r0['neg'].values, _want(nam, lev, (coef < 0).astype(float))[1], rtol=0, atol=1e-13)
        assert c0['pos'].sum() == int((coef > 0).sum()) and c0['neg'].sum() == int((coef < 0).sum())
    with pytest.raises(KeyError):
        _ns(d0, 'leiden', 'id', sign_of='coef', fdr_thresh=0.05, engine=BinsFake())
    with pytest.raises(KeyError):
        _ns(d0, 'leiden', 'id', sign_of='absent', engine=BinsFake())
    d1 = _with(data, coef=coef, coef_fdr=fdr)
    for thresh in (None, 0.05):
        t = 0.1 if thresh is None else thresh
        r1 = _ns(d1, 'leiden', 'id', sign_of='coef', fdr_thresh=thresh, engine=BinsFake())
        with np.errstate(invalid='ignore'):
            pos, neg = (coef > 0) & (fdr <= t), (coef < 0) & (fdr <= t)
        assert not pos[5] and not neg[5]                    # a NaN fdr fails
        np.testing.assert_allclose(r1['pos'].values, _want(nam, lev, pos.astype(float))[1], rtol=0, atol=1e-13)
        np.testing.assert_allclose(r1['neg'].values, _want(nam, lev, neg.astype(float))[1], rtol=0, atol=1e-13)


def test_refusals(case):
    data, _, _ = case
    with pytest.raises(ValueError):
        _ns(data, 'leiden', 'id', weights='w1', sign_of='coef', engine=BinsFake())
    with pytest.raises(ValueError):
        _ns(data, 'leiden', 'id', weights=['w1'] * 17, engine=BinsFake())
    with pytest.raises(ValueError):
        _ns(data, 'leiden', 'id', weights=[], engine=BinsFake())
    from cna_amd import synth
    many, _ = synth.make_dataset(1100, 3, k=5, seed=1, builder='cpu')
    many.obs['lev'] = np.arange(1100)
    e = BinsFake()
    with pytest.raises(ValueError):
        _ns(many, 'lev', 'id', engine=e)
    many.obs['lev'] = np.arange(1100) % 1024
    many.obs['w'] = 1.0
    with pytest.raises(ValueError):                          # 5 x 1024 sums do not fit one pass
        _ns(many, 'lev', 'id', weights=['w'] * 5, engine=e)
    assert e.walks() == 0                                    # refused before anything ran
    none = _with(data, leiden=np.full(N_CELLS, None, dtype=object))
    with pytest.raises(ValueError):
        _ns(none, 'leiden', 'id', engine=BinsFake())


def test_a_second_call_walks_nothing(case):
    data, _, _ = case
    e = BinsFake()
    first = _ns(data, 'leiden', 'id', engine=e)
    steps = e.walks()
    assert steps == 3
    second = _ns(data, 'leiden', 'id', weights='w2', engine=e)
    again = _ns(data, 'leiden', 'id', engine=e)
    assert e.walks() == steps and second.shape == first.shape
    np.testing.assert_array_equal(again.values, first.values)


def test_sharded_data_and_ranks_are_refused(case):
    data, _, _ = case
    from cna_amd.synth import CellData
    shard = CellData(data.obs, data.obsp['connectivities'])
    shard.uns['cna_shard'] = {'row0': 0, 'n_global': 2 * N_CELLS}
    with pytest.raises(NotImplementedError):
        _ns(shard, 'leiden', 'id', engine=BinsFake())
    e = BinsFake()
    e.nranks = 2
    with pytest.raises(NotImplementedError):
        _ns(data, 'leiden', 'id', engine=e)
