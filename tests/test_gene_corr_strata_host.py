"""cna.tl.gene_corr_strata on the CPU: the float64 numpy restatement of its semantics (what the GPU tests compare with),
the generator of the GPU tests' levels with the proof that their inputs are benign for raw moments, and the public call
against an engine double (GeneEngine of test_gene_corr_host.py with `gene_corr_by` backed by the restatement)."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from test_gene_corr_host import (GeneEngine, restated_gene_corr, dense_expression, sparse_expression, keys_for, demo, _frame)  # noqa: F401


# ------------------------------------------------------------------ the restatement
def _dense64(X):
    return np.asarray(X.toarray() if sp.issparse(X) else X, dtype=np.float64)


def restated_within(X, V, codes, n_levels):
    """The cluster-adjusted correlation, independently of the per-level sums, in two passes: the level means are subtracted
    from x and from v in float64, then one centred correlation over the cells that have a level and a finite v_j.  A level
    where the gene (the key) is constant -- minimum == maximum, decided exactly -- contributes exact zeros.  q x genes."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    Xd = _dense64(X)
    codes = np.asarray(codes)
    out = np.full((V.shape[0], Xd.shape[1]), np.nan)
    for j, v in enumerate(V):
        idx = np.flatnonzero((codes >= 0) & np.isfinite(v))
        if idx.size == 0:
            continue
        idx = idx[np.argsort(codes[idx], kind='stable')]
        c = codes[idx]
        starts = np.flatnonzero(np.r_[True, c[1:] != c[:-1]])
        cnt = np.diff(np.r_[starts, c.size])
        Xs, vs = Xd[idx], v[idx]
        xmean = np.add.reduceat(Xs, starts, axis=0) / cnt[:, None]
        vmean = np.add.reduceat(vs, starts) / cnt
        xc = Xs - np.repeat(xmean, cnt, axis=0)
        vc = vs - np.repeat(vmean, cnt)
        gene_live = np.minimum.reduceat(Xs, starts, axis=0) != np.maximum.reduceat(Xs, starts, axis=0)     # levels x genes
        key_live = np.minimum.reduceat(vs, starts) != np.maximum.reduceat(vs, starts)                      # levels
        xc[~np.repeat(gene_live, cnt, axis=0)] = 0.0
        vc[~np.repeat(key_live, cnt)] = 0.0
        cov, varx, varv = xc.T.dot(vc), (xc * xc).sum(axis=0), (vc * vc).sum()
        with np.errstate(all='ignore'):
            r = np.clip(cov / np.sqrt(varx * varv), -1.0, 1.0)
        r[~gene_live.any(axis=0)] = np.nan
        if not key_live.any():
            r[:] = np.nan
        out[j] = r
    return out


def restated_gene_corr_strata(X, V, codes, n_levels):
    """float64 restatement of cna_gene_corr_by: r[j, L] = restated_gene_corr(X, where(codes == L, V[j], nan)), the existing
    restatement level by level (taken on the level's own rows: restated_gene_corr reads no others), the within-level
    correlation by restated_within, n[j, L] = cells of level L with a finite V[j].  Returns (r q x levels x genes, within
    q x genes, n q x levels)."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    codes = np.asarray(codes)
    Xr = sp.csr_matrix(X) if sp.issparse(X) else X
    r = np.full((V.shape[0], n_levels, X.shape[1]), np.nan)
    n = np.zeros((V.shape[0], n_levels), dtype=np.int64)
    order = np.argsort(codes, kind='stable')
    bounds = np.searchsorted(codes[order], np.arange(n_levels + 1))
    for L in range(n_levels):
        rows = order[bounds[L]:bounds[L + 1]]
        if rows.size == 0:
            continue
        r[:, L] = restated_gene_corr(Xr[rows], V[:, rows])
        n[:, L] = np.isfinite(V[:, rows]).sum(axis=1)
    return r, restated_within(X, V, codes, n_levels), n


def strata_conditioning(X, V, codes):
    """max over (key, level, gene that is not constant there) of sum x^2 / sum (x - mean)^2 over the level's cells with a
    finite key: how much the raw-moment variance of cna_gene_corr_by loses."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    Xd = _dense64(X)
    codes = np.asarray(codes)
    worst = 0.0
    for w in np.unique(np.isfinite(V), axis=0):
        idx = np.flatnonzero((codes >= 0) & w)
        idx = idx[np.argsort(codes[idx], kind='stable')]
        c = codes[idx]
        starts = np.flatnonzero(np.r_[True, c[1:] != c[:-1]])
        cnt = np.diff(np.r_[starts, c.size])
        Xs = Xd[idx]
        mean = np.add.reduceat(Xs, starts, axis=0) / cnt[:, None]
        ss = np.add.reduceat(Xs * Xs, starts, axis=0)
        cs = np.add.reduceat((Xs - np.repeat(mean, cnt, axis=0)) ** 2, starts, axis=0)
        live = np.minimum.reduceat(Xs, starts, axis=0) != np.maximum.reduceat(Xs, starts, axis=0)
        if live.any():
            worst = max(worst, float((ss[live] / cs[live]).max()))
    return worst


# ------------------------------------------------------------------ the levels of the GPU cases
def levels_for(n, L, seed):
    """Codes of n cells in L levels for the GPU parity cases: a permutation modulo the level count (every level about
    n / L cells, in no order), 2 % of the cells without a level; from four levels on the last two are small: level L - 1 has
    exactly one cell, level L - 2 exactly two (the others share the rest)."""
    rs = np.random.RandomState(500 + seed)
    codes = (rs.permutation(n) % (L - 2 if L >= 4 else L)).astype(np.int32)
    codes[rs.rand(n) < 0.02] = -1
    if L >= 4:
        cells = rs.choice(n, 3, replace=False)
        codes[cells[0]] = L - 1
        codes[cells[1:]] = L - 2
    return codes


def with_benign_pair(X, codes, L):
    """X with the two cells of level L - 2 (levels_for, L >= 4) overwritten so that this level is benign for raw moments
    whatever the matrix held: two continuous values that happen to lie close would give a conditioning in the millions
    (2.0e6 was measured with random level sizes and no overwrite).  Dense: rows of 0.5 and 2.5; sparse: 1.0 at the even genes
    of one row, 3.0 at the genes divisible by 3 of the other.  Format, dtypes and index types are kept."""
    if L < 4:
        return X
    a, b = np.flatnonzero(np.asarray(codes) == L - 2)
    if not sp.issparse(X):
        X = X.copy()
        X[a], X[b] = 0.5, 2.5
        return X
    g = np.arange(X.shape[1])
    M = sp.lil_matrix(X)
    M[a], M[b] = np.where(g % 2 == 0, 1.0, 0.0), np.where(g % 3 == 0, 3.0, 0.0)
    M = sp.csr_matrix(M).astype(X.dtype)
    M.eliminate_zeros()
    M.sort_indices()
    M = M.asformat(X.format)
    M.indices, M.indptr = M.indices.astype(X.indices.dtype), M.indptr.astype(X.indptr.dtype)
    return M


N_ODD = 3001
# (cells, genes, levels, keys, masks) of the GPU parity cases (tests/test_gpu_gene_corr_strata.py)
PARITY_CASES = [(N_ODD, 70, 1, 1, 'none'), (N_ODD, 70, 2, 2, 'equal'), (N_ODD, 70, 17, 3, 'differ'), (N_ODD, 70, 64, 5, 'differ'),
                (N_ODD, 70, 16, 16, 'differ'), (N_ODD, 70, 33, 1, 'equal'), (20011, 70, 256, 2, 'differ'),
                (80021, 40, 1024, 4, 'differ'), (40013, 300, 7, 2, 'differ')]
CONDITIONING_CAP = 100.0


def parity_input(kind, n, g, L, q, masks, dtype=np.float64, fmt='csr', index_dtype=np.int32):
    """(X, V, codes) of a GPU parity case: dense_expression / sparse_expression and keys_for seeded with q, levels_for seeded
    with L, the pair of level L - 2 overwritten."""
    codes = levels_for(n, L, seed=L)
    if kind == 'dense':
        X = dense_expression(n, g, seed=q, dtype=dtype)
    else:
        X = sparse_expression(n, g, seed=q, dtype=dtype, fmt=fmt, index_dtype=index_dtype)
    return with_benign_pair(X, codes, L), keys_for(n, q, seed=q, masks=masks), codes


@pytest.mark.parametrize('n,g,L,q,masks', PARITY_CASES)
def test_gpu_parity_inputs_are_benign_for_raw_moments(n, g, L, q, masks):
    """The rule of test_parity_inputs_are_benign_for_raw_moments, level by level: for every GPU parity input the worst
    sum x^2 / sum (x - mean)^2 over (key, level, non-constant gene) stays under 100, so the 1e-10 bound of the GPU tests
    tests the kernels and not the formula.  Computed on the CPU across these cases: worst 24.8 (dense, L = 64); the
    80021-cell, 1024-level case 20.6 dense f32, 9.7 sparse.  A case that exceeds the cap gets a larger n, never a larger cap."""
    codes = levels_for(n, L, seed=L)
    assert codes.min() == -1 and codes.max() == L - 1 and 0.01 < (codes < 0).mean() < 0.03
    sizes = np.bincount(codes[codes >= 0], minlength=L)
    if L >= 4:
        assert sizes[L - 1] == 1 and sizes[L - 2] == 2 and sizes[:L - 2].min() >= 2
    for kind, dtype in (('dense', np.float32), ('dense', np.float64), ('sparse', np.float64)):
        X, V, _ = parity_input(kind, n, g, L, q, masks, dtype=dtype)
        worst = strata_conditioning(X, V, codes)
        print('%s %s n=%d L=%d q=%d %s: conditioning %.1f' % (kind, np.dtype(dtype).name, n, L, q, masks, worst))
        assert worst <= CONDITIONING_CAP, (kind, n, L, q, masks, worst)
        if kind == 'sparse':
            assert X.getnnz(axis=0)[0] >= n - 2 and X.getnnz(axis=0)[1] <= 5          # the skew genes stay


def test_nan_share_of_a_parity_case_is_small():
    X, V, codes = parity_input('sparse', 80021, 40, 1024, 4, 'differ')
    r, within, n = restated_gene_corr_strata(X, V, codes, 1024)
    assert np.isnan(r).mean() <= 0.15 and np.isfinite(within[:, 2:]).all()
    assert (n[:, 1023] <= 1).all() and np.isnan(r[:, 1023]).all()


# ------------------------------------------------------------------ checks on the restatement
def test_restatement_is_corrcoef_per_level_and_gene(demo):
    n = len(demo.obs)
    codes = levels_for(n, 6, seed=1)
    V = keys_for(n, 2, seed=4, masks='differ')
    V[0] = np.where(np.isfinite(V[0]), demo.obs['coef'].values, np.nan)
    X = with_benign_pair(demo.X, codes, 6)
    r, within, cnt = restated_gene_corr_strata(X, V, codes, 6)
    assert r.shape == (2, 6, X.shape[1]) and within.shape == (2, X.shape[1]) and cnt.shape == (2, 6)
    for j in range(2):
        for L in range(6):
            C = (codes == L) & np.isfinite(V[j])
            assert cnt[j, L] == C.sum()
            if C.sum() < 2:
                assert np.isnan(r[j, L]).all()
                continue
            want = np.corrcoef(V[j, C], X[C].astype(np.float64), rowvar=False)[0, 1:]
            np.testing.assert_allclose(r[j, L], want, rtol=0, atol=1e-12)
    assert np.isnan(r[:, 5]).all() and np.isfinite(r[:, :4]).all()
    # the literal definition: the whole matrix, the key masked to the level
    for L in range(6):
        np.testing.assert_array_equal(r[:, L], restated_gene_corr(X, np.where(codes == L, V, np.nan)))


def test_restatement_sparse_equals_dense():
    n, L = 1501, 9
    codes = levels_for(n, L, seed=3)
    M = with_benign_pair(sparse_expression(n, 40, seed=5), codes, L)
    M = sp.lil_matrix(M)
    M[:, 7] = 0.0                                  # all-zero gene
    M[np.flatnonzero(codes == 2), 8] = 2.5         # constant inside one level only
    M = sp.csr_matrix(M)
    M.eliminate_zeros()
    V = keys_for(n, 3, seed=5, masks='differ')
    V[2, codes == 4] = 1.25                        # a key that is constant inside one level
    a, b = restated_gene_corr_strata(M, V, codes, L), restated_gene_corr_strata(M.toarray(), V, codes, L)
    for x, y in zip(a[:2], b[:2]):
        np.testing.assert_array_equal(np.isnan(x), np.isnan(y))
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(a[2], b[2])
    r, within, _ = a
    assert np.isnan(r[:, :, 7]).all() and np.isnan(within[:, 7]).all()
    assert np.isnan(r[:, 2, 8]).all() and np.isfinite(r[:, 3, 8]).all() and np.isfinite(within[:, 8]).all()
    assert np.isnan(r[2, 4]).all() and np.isfinite(r[2, 3, 2:7]).all() and np.isfinite(within[2, 2:7]).all()


def test_a_single_level_with_every_cell_is_gene_corr():
    n = 1201
    X = dense_expression(n, 25, seed=2)
    V = keys_for(n, 3, seed=2, masks='differ')
    r, within, cnt = restated_gene_corr_strata(X, V, np.zeros(n, dtype=np.int32), 1)
    want = restated_gene_corr(X, V)
    np.testing.assert_array_equal(r[:, 0], want)
    np.testing.assert_allclose(within, want, rtol=0, atol=1e-12)       # one level: its mean is the mean
    np.testing.assert_array_equal(cnt[:, 0], np.isfinite(V).sum(axis=1))


def test_within_has_a_closed_form_on_two_levels():
    """gene 0 = level indicator * 5 + key: the indicator vanishes inside the levels, the within-level correlation is 1;
    gene 1 = the indicator alone: constant inside both levels, NaN; gene 2 = -key in level 0, a constant in level 1: -1 over
    level 0's share, sqrt(ssv_0 / (ssv_0 + ssv_1)) in size."""
    n = 400
    rs = np.random.RandomState(8)
    v = rs.randn(n)
    codes = (np.arange(n) % 2).astype(np.int32)
    codes[::37] = -1
    ind = (codes == 1).astype(np.float64)
    X = np.column_stack([5.0 * ind + v, ind, np.where(codes == 0, -v, 7.0)])
    r, within, _ = restated_gene_corr_strata(X, v, codes, 2)
    ss = [((v[codes == L] - v[codes == L].mean()) ** 2).sum() for L in (0, 1)]
    assert abs(within[0, 0] - 1.0) <= 1e-12 and np.isnan(within[0, 1])
    assert abs(within[0, 2] + np.sqrt(ss[0] / (ss[0] + ss[1]))) <= 1e-12
    np.testing.assert_allclose(r[0, :, 0], [1.0, 1.0], rtol=0, atol=1e-12)
    assert np.isnan(r[0, :, 1]).all() and abs(r[0, 0, 2] + 1.0) <= 1e-12 and np.isnan(r[0, 1, 2])
    # the global correlation does not see it: the indicator dominates gene 0
    assert restated_gene_corr(X, np.where(codes >= 0, v, np.nan))[0, 0] < 0.6


# ------------------------------------------------------------------ the double
class StrataEngine(GeneEngine):
    """GeneEngine (the real residency code, counted uploads) with the per-level reduction as numpy."""

    def gene_corr_by(self, V, codes, n_bins, want_within=True):
        assert self.resident is not None
        r, within, n = restated_gene_corr_strata(self.resident, V, codes, n_bins)
        return r, (within if want_within else None), n


@pytest.fixture()
def clustered(demo):
    n = len(demo.obs)
    d = _frame(n, X=demo.X, coef=demo.obs['coef'].values,
               other=np.where(np.arange(n) % 11 == 0, np.nan, demo.obs['coef'].values ** 2))
    d.var = pd.DataFrame(index=demo.var_names)
    lab = np.array(['c%d' % (i * 7 % 5) for i in range(n)], dtype=object)
    lab[3::50] = None
    d.obs['leiden'] = lab
    return d


def test_gene_corr_strata_through_the_public_call(clustered):
    import cna_amd as cna
    assert 'gene_corr_strata' in cna.tl.__all__
    d, eng = clustered, StrataEngine()
    codes, levels = pd.factorize(d.obs['leiden'])
    assert (codes < 0).sum() > 0 and list(levels) == list(pd.unique(d.obs['leiden'].dropna()))
    V = np.stack([d.obs['coef'].values, d.obs['other'].values])
    r, within, _ = restated_gene_corr_strata(d.X, V, codes, len(levels))
    out = cna.tl.gene_corr_strata(d, 'leiden', engine=eng)                    # a str key: the levels as columns
    assert isinstance(out, pd.DataFrame) and out.index.equals(d.var_names) and (out.dtypes == np.float64).all()
    assert list(out.columns) == list(levels) and out.columns.name == 'leiden' and not isinstance(out.columns, pd.MultiIndex)
    np.testing.assert_array_equal(out.values, r[0].T)
    for L, name in enumerate(levels):                                         # the NaN level is left out, the order is first appearance
        C = (d.obs['leiden'].values == name)
        want = np.corrcoef(V[0, C], d.X[C].astype(np.float64), rowvar=False)[0, 1:]
        np.testing.assert_allclose(out[name].values, want, rtol=0, atol=1e-12)
    out2, w2 = cna.tl.gene_corr_strata(d, 'leiden', ['coef', 'other'], return_within=True, engine=eng)
    assert isinstance(out2.columns, pd.MultiIndex) and list(out2.columns.names) == ['key', 'leiden']
    assert list(out2.columns) == [(k, name) for k in ('coef', 'other') for name in levels]               # key-major
    np.testing.assert_array_equal(out2['other'].values, r[1].T)
    np.testing.assert_array_equal(out2['coef'].values, out.values)
    assert list(w2.columns) == ['coef', 'other'] and w2.index.equals(d.var_names) and (w2.dtypes == np.float64).all()
    np.testing.assert_array_equal(w2.values, within.T)
    out3, w3 = cna.tl.gene_corr_strata(d, 'leiden', ['coef'], return_within=True, engine=eng)            # a list of one
    assert isinstance(out3.columns, pd.MultiIndex) and list(w3.columns) == ['coef']
    assert len(eng.uploads) == 1                                              # one upload across the calls
    assert cna.tl.gene_corr(d, 'coef', engine=eng).shape == (d.X.shape[1], 1) and len(eng.uploads) == 1   # shared with gene_corr
    # a layer, and data without var names
    d.layers['sq'] = np.ascontiguousarray(d.X.astype(np.float64) ** 2)
    out4 = cna.tl.gene_corr_strata(d, 'leiden', 'coef', layer='sq', engine=eng)
    np.testing.assert_array_equal(out4.values, restated_gene_corr_strata(d.layers['sq'], V[0], codes, len(levels))[0][0].T)
    d.var = None
    out5, w5 = cna.tl.gene_corr_strata(d, 'leiden', 'coef', return_within=True, engine=eng)
    assert isinstance(out5.index, pd.RangeIndex) and isinstance(w5.index, pd.RangeIndex) and len(out5) == d.X.shape[1]


def test_bad_arguments_raise_before_any_upload(clustered):
    import cna_amd as cna
    d, eng = clustered, StrataEngine()
    n = len(d.obs)
    with pytest.raises(KeyError, match='nope'):
        cna.tl.gene_corr_strata(d, 'leiden', ['coef', 'nope'], engine=eng)
    with pytest.raises(KeyError, match='louvain'):
        cna.tl.gene_corr_strata(d, 'louvain', engine=eng)
    cols = {'k%d' % j: np.arange(n, dtype=float) for j in range(17)}
    many = _frame(n, X=d.X, leiden=d.obs['leiden'].values, **cols)
    with pytest.raises(ValueError, match='16'):
        cna.tl.gene_corr_strata(many, 'leiden', list(cols), engine=eng)
    with pytest.raises(ValueError, match='0 levels'):
        cna.tl.gene_corr_strata(_frame(n, X=d.X, coef=np.zeros(n), leiden=np.full(n, np.nan)), 'leiden', engine=eng)
    ids = np.arange(n) % 1025
    with pytest.raises(ValueError, match='1025 levels'):
        cna.tl.gene_corr_strata(_frame(n, X=d.X, coef=np.zeros(n), leiden=ids), 'leiden', engine=eng)
    with pytest.raises(ValueError, match='4096'):                             # 5 keys x 1000 levels
        cna.tl.gene_corr_strata(_frame(n, X=d.X, leiden=np.arange(n) % 1000, **cols), 'leiden', list(cols)[:5], engine=eng)
    for bad in (d.X.astype(np.float16), sp.coo_matrix(d.X), np.asfortranarray(d.X)):
        with pytest.raises(TypeError):
            cna.tl.gene_corr_strata(_frame(n, X=bad, coef=np.zeros(n), leiden=ids % 3), 'leiden', engine=eng)
    with pytest.raises(ValueError, match='rows'):
        cna.tl.gene_corr_strata(_frame(n - 1, X=d.X, coef=np.zeros(n - 1), leiden=ids[1:] % 3), 'leiden', engine=eng)
    with pytest.raises(ValueError, match='data.X'):
        cna.tl.gene_corr_strata(_frame(n, coef=np.zeros(n), leiden=ids % 3), 'leiden', engine=eng)
    with pytest.raises(KeyError):
        cna.tl.gene_corr_strata(d, 'leiden', layer='missing', engine=eng)
    assert eng.uploads == []
    # the limits themselves pass: 1024 levels with 4 keys
    ok = _frame(n, X=d.X, leiden=np.arange(n) % 1024, **cols)
    assert cna.tl.gene_corr_strata(ok, 'leiden', list(cols)[:4], engine=eng).shape == (d.X.shape[1], 4096)


def test_sharded_data_and_multi_rank_engines_are_refused(demo):
    import cna_amd as cna
    from cna_amd import dist
    eng = StrataEngine()
    part = dist.shard(demo, rank=0, nranks=2)
    part.X = demo.X[:len(part.obs)]
    part.obs['coef'] = 1.0
    part.obs['leiden'] = 'a'
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.gene_corr_strata(part, 'leiden', engine=eng)
    whole = _frame(len(demo.obs), X=demo.X, coef=demo.obs['coef'].values, leiden=np.arange(len(demo.obs)) % 3)
    with pytest.raises(NotImplementedError, match='multi-rank'):
        cna.tl.gene_corr_strata(whole, 'leiden', engine=StrataEngine(nranks=2))
    assert eng.uploads == []
