"""cna.tl.gene_corr on the CPU: argument checks, the float64 numpy restatement of its semantics (what the GPU tests
compare with) and the residency bookkeeping, against an engine double defined here.

The double takes the REAL residency code of cna_amd.engine.Engine (ensure_expression, pin / unpin / drop, the quick key and
the content hash, which is host code of the library) and replaces only the two calls that need a device: the upload, which
it counts, and the reduction, which is `restated_gene_corr`."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from fake_engine import FakeEngine


# ------------------------------------------------------------------ the restatement
def restated_gene_corr(X, V):
    """float64 restatement of cna_gene_corr.  X: cells x genes, dense or scipy sparse; V: q x cells, non-finite = cell
    left out of that key.  Per key: mask, centred key, raw gene moments over the kept cells, constant genes and keys
    decided exactly (minimum == maximum) -> NaN.  Returns q x genes."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    sparse = sp.issparse(X)
    if sparse:
        X = sp.csr_matrix(X, dtype=np.float64, copy=True)
        X.sum_duplicates()
    else:
        X = np.asarray(X, dtype=np.float64)
    out = np.full((V.shape[0], X.shape[1]), np.nan)
    for j, v in enumerate(V):
        w = np.isfinite(v)
        n = int(w.sum())
        if n < 2 or v[w].min() == v[w].max():
            continue
        vc = v[w] - v[w].mean()
        Xw = X if w.all() else X[w]
        if sparse:
            sx = np.asarray(Xw.sum(axis=0)).ravel()
            sxx = np.asarray(Xw.multiply(Xw).sum(axis=0)).ravel()
            sxv = np.asarray(Xw.T.dot(vc)).ravel()
            mn = np.asarray(Xw.min(axis=0).todense()).ravel()
            mx = np.asarray(Xw.max(axis=0).todense()).ravel()
        else:
            sx, sxx, sxv = Xw.sum(axis=0), (Xw * Xw).sum(axis=0), Xw.T.dot(vc)
            mn, mx = Xw.min(axis=0), Xw.max(axis=0)
        mean = sx / n
        with np.errstate(all='ignore'):
            r = (sxv - mean * vc.sum()) / np.sqrt(sxx - sx * mean) / np.sqrt((vc * vc).sum())
            r = np.where(np.isnan(r), r, np.clip(r, -1.0, 1.0))
        r[mn == mx] = np.nan
        out[j] = r
    return out


def demo_line(v, X):
    """The reference's line (demo/demo.ipynb, "per-gene correlations to neighborhood coefficient"),
    np.corrcoef(v.reshape(1,-1), X, rowvar=False)[0,1:], literally where numpy still takes it: numpy 2 transposes a
    (1, n) first argument under rowvar=False and then refuses the shapes; the 1-D first argument is the same
    computation (row 0 = v, rows 1.. = the genes) on every numpy."""
    v = np.asarray(v)
    try:
        return np.corrcoef(v.reshape(1, -1), X, rowvar=False)[0, 1:]
    except ValueError:
        return np.corrcoef(v, X, rowvar=False)[0, 1:]


def conditioning(X):
    """max over the non-constant genes of sum x^2 / sum (x - mean)^2: how much the raw-moment variance loses."""
    Xd = np.asarray(X.toarray() if sp.issparse(X) else X, dtype=np.float64)
    ss = (Xd * Xd).sum(axis=0)
    cs = ((Xd - Xd.mean(axis=0)) ** 2).sum(axis=0)
    live = Xd.min(axis=0) != Xd.max(axis=0)
    return float((ss[live] / cs[live]).max())


def sparse_expression(n, g, density=0.05, seed=0, dtype=np.float64, fmt='csr', index_dtype=np.int32, skew=True):
    """Count-like sparse expression, benign for the raw-moment variance: every gene sits in its own random `density` of
    the cells with values 1 + Poisson(2) (sum x^2 / sum (x - mean)^2 is then about 1 / (1 - density) plus the spread's
    share, well under 100).  skew: gene 0 is present in every cell, gene 1 in exactly 3 cells."""
    rs = np.random.RandomState(seed)
    M = sp.random(n, g, density=density, format='csr', random_state=rs, data_rvs=lambda k: 1.0 + rs.poisson(2.0, k))
    M = sp.lil_matrix(M)
    if skew and g >= 2:
        M[:, 0] = (1.0 + rs.poisson(2.0, n)).reshape(-1, 1)
        M[:, 1] = 0.0
        M[rs.choice(n, 3, replace=False), 1] = [1.0, 2.0, 4.0]
    M = sp.csr_matrix(M).astype(dtype)
    M.eliminate_zeros()
    M.sort_indices()
    M = M.asformat(fmt)
    M.indices = M.indices.astype(index_dtype)
    M.indptr = M.indptr.astype(index_dtype)
    return M


def keys_for(n, q, seed=0, masks='none'):
    """q key columns (q x n): masks 'none' all finite, 'equal' the same 7 % of the cells NaN in every key, 'differ' each
    key its own."""
    rs = np.random.RandomState(100 + seed)
    V = rs.randn(q, n) * (1.0 + np.arange(q))[:, None] + np.arange(q)[:, None]
    if masks == 'equal':
        V[:, rs.rand(n) < 0.07] = np.nan
    elif masks == 'differ':
        for j in range(q):
            V[j, rs.rand(n) < 0.03 * (1 + j % 4)] = np.nan
    return V


# ------------------------------------------------------------------ the double
class GeneEngine(FakeEngine):
    """FakeEngine plus the expression residency of the real Engine; uploads are counted, the reduction is numpy."""

    def __init__(self, coll=None, nranks=None):
        super().__init__(coll=coll)
        from cna_amd import _ffi, _order
        self.lib = _ffi.load()
        self._host_threads = _order.usable_cpus(8)
        self._expr_key = self._expr_hash = self._expr_ref = self._expr_pinned = None
        self.uploads = []
        self.resident = None
        if nranks is not None:
            self.nranks = nranks


def _borrow():
    from cna_amd.engine import Engine
    for name in ('_quick_key', '_ident', '_buffers', '_hash', '_expr_arrays', '_expr_buffers', '_expr_ident', '_expr_quick_key',
                 '_expr_is_pinned', 'pin_expression', 'unpin_expression', 'ensure_expression'):
        setattr(GeneEngine, name, Engine.__dict__[name])

    def _upload_expression(self, X):
        self.uploads.append(X.shape)
        self.resident = X.copy()

    def drop_expression(self):
        self._expr_key = self._expr_hash = self._expr_ref = None
        self.resident = None

    def gene_corr(self, V):
        assert self.resident is not None
        return restated_gene_corr(self.resident, V)
    GeneEngine._upload_expression = _upload_expression
    GeneEngine.drop_expression = drop_expression
    GeneEngine.gene_corr = gene_corr


_borrow()


@pytest.fixture(scope='module')
def demo():
    from cna_amd import synth
    data, samplem = synth.make_demo_like(n_samples=20, n_genes=30, cells_per_sample=100, seed=3, keep_expression=True)
    rs = np.random.RandomState(0)
    data.obs['coef'] = data.X[:, :5].astype(np.float64).dot(rs.randn(5)) + rs.randn(len(data.obs))
    return data


def _frame(n, X=None, **cols):
    from cna_amd.synth import CellData
    obs = pd.DataFrame(cols, index=pd.Index(['c%d' % i for i in range(n)]))
    return CellData(obs, None, X=X)


# ------------------------------------------------------------------ semantics
def test_keep_expression_is_additive():
    from cna_amd import synth
    a, _ = synth.make_demo_like(n_samples=10, n_genes=12, cells_per_sample=40, seed=1)
    b, _ = synth.make_demo_like(n_samples=10, n_genes=12, cells_per_sample=40, seed=1, keep_expression=True)
    assert a.X is None and a.var is None and a.var_names is None and a.layers == {}
    assert b.X.shape == (400, 12) and b.X.dtype == np.float32 and list(b.var_names[:2]) == ['gene_0', 'gene_1']
    assert synth.graph_digest(a.obsp['connectivities']) == synth.graph_digest(b.obsp['connectivities'])
    assert a.obs.equals(b.obs)


def test_restatement_is_the_demo_line_when_every_cell_is_finite(demo):
    v = demo.obs['coef'].values
    want = demo_line(v, demo.X)
    got = restated_gene_corr(demo.X, v)[0]
    assert conditioning(demo.X) <= 5
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_restatement_with_left_out_cells_is_a_masked_corrcoef_per_gene(demo):
    V = keys_for(len(demo.obs), 3, seed=2, masks='differ')
    V[0] = demo.obs['coef'].values
    V[0, ::9] = np.nan
    got = restated_gene_corr(demo.X, V)
    for j in range(3):
        w = np.isfinite(V[j])
        assert 0 < (~w).sum() < len(w)
        for g in range(demo.X.shape[1]):
            want = np.corrcoef(V[j, w], demo.X[w, g].astype(np.float64))[0, 1]
            assert abs(got[j, g] - want) <= 1e-12, (j, g)


def test_restatement_sparse_equals_dense_and_marks_constants():
    M = sparse_expression(1501, 40, seed=5)
    M = sp.lil_matrix(M)
    M[:, 7] = 0.0             # all-zero gene
    M[:, 8] = 2.5             # constant non-zero gene
    M = sp.csr_matrix(M)
    M.eliminate_zeros()
    V = keys_for(1501, 4, seed=5, masks='differ')
    V[3] = 1.25               # constant key
    a, b = restated_gene_corr(M, V), restated_gene_corr(M.toarray(), V)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-12, equal_nan=True)
    assert np.isnan(a[:, 7]).all() and np.isnan(a[:, 8]).all() and np.isnan(a[3]).all()
    assert np.isfinite(a[:3, [0, 1, 2, 3]]).all()
    # fewer than two finite cells
    v = np.full(1501, np.nan)
    v[4] = 1.0
    assert np.isnan(restated_gene_corr(M, v)).all()


def test_single_nonzero_gene_has_a_closed_form():
    n = 500
    v = np.random.RandomState(3).randn(n)
    X = np.zeros((n, 2))
    X[123, 0] = 3.0
    X[:, 1] = v
    vc = v - v.mean()
    want = vc[123] / np.sqrt((vc * vc).sum() * (1 - 1 / n))
    got = restated_gene_corr(X, v)[0]
    assert abs(got[0] - want) <= 1e-13 and abs(got[1] - 1.0) <= 1e-13


PARITY_Q = [1, 2, 3, 5, 8, 16]      # key counts of the GPU parity cases; each also seeds its expression matrix and its keys


@pytest.mark.parametrize('seed', sorted(set([0, 1, 2] + PARITY_Q)))
def test_parity_inputs_are_benign_for_raw_moments(seed, demo):
    """The inputs the GPU tests use for parity: sum x^2 / sum (x - mean)^2 <= 100 for every non-constant gene, so that
    their 1e-10 bound tests the kernels and not the raw-moment formula.  For the key counts of PARITY_Q the matrices are
    the GPU cases' own (3001 x 70, seed = q), and the figure is taken again over the cells every key of every mask layout
    keeps -- the sums the kernels form."""
    assert conditioning(demo.X) <= 5
    for n, g in ((3001, 70), (1000, 33)):
        assert conditioning(sparse_expression(n, g, seed=seed)) <= 100
    assert conditioning(dense_expression(3001, 70, seed)) <= 100
    M = big_sparse_expression(2000, 400, per_row=20, seed=seed)
    assert conditioning(M) <= 100 and M.has_canonical_format
    if seed in PARITY_Q:
        q = seed
        Xs = (dense_expression(3001, 70, seed=q), dense_expression(3001, 70, seed=q, dtype=np.float32).astype(np.float64),
              sparse_expression(3001, 70, seed=q).toarray())
        for masks in ('none', 'equal', 'differ'):
            V = keys_for(3001, q, seed=q, masks=masks)
            assert V.shape == (q, 3001)
            kept = np.unique(np.isfinite(V), axis=0)
            assert len(kept) == (1 if masks != 'differ' or q == 1 else q) and (kept.sum(axis=1) > 2500).all()
            for w in kept:
                for X in Xs:
                    assert conditioning(X[w]) <= 100, (q, masks)
            # the keys themselves are centred before they are multiplied (k_key_stats, k_key_table): nothing to condition


def dense_expression(n, g, seed=0, dtype=np.float64):
    """Dense log-expression-like values: a gene-specific level in [0, 3] plus unit noise."""
    rs = np.random.RandomState(seed)
    return np.ascontiguousarray((rs.rand(g) * 3.0 + rs.randn(n, g)).astype(dtype))


def big_sparse_expression(n, g, per_row, seed=0, dtype=np.float32):
    """A CSR matrix with exactly per_row entries in every row, built without a sort (what the larger GPU case needs at
    200M entries): the genes are cut into per_row buckets of g / per_row, a row has one entry at a random place of each
    bucket; values 1 + Poisson(2).  Sorted indices, no duplicates; every gene is present in about per_row / g of the cells."""
    assert g % per_row == 0
    width = g // per_row
    rs = np.random.RandomState(seed)
    idx = (rs.randint(0, width, size=(n, per_row), dtype=np.int32) + (np.arange(per_row, dtype=np.int32) * width)[None, :])
    val = (1.0 + rs.poisson(2.0, size=n * per_row)).astype(dtype)
    M = sp.csr_matrix((val, idx.ravel(), np.arange(n + 1, dtype=np.int64) * per_row), shape=(n, g))
    M.has_sorted_indices = True
    M.has_canonical_format = True
    return M


# ------------------------------------------------------------------ arguments
def test_gene_corr_through_the_public_call(demo):
    import cna_amd as cna
    eng = GeneEngine()
    out = cna.tl.gene_corr(demo, 'coef', engine=eng)
    want = demo_line(demo.obs['coef'].values, demo.X)
    assert list(out.columns) == ['coef'] and out.index.equals(demo.var_names) and out['coef'].dtype == np.float64
    np.testing.assert_allclose(out['coef'].values, want, rtol=0, atol=1e-12)
    demo.obs['other'] = np.where(np.arange(len(demo.obs)) % 11 == 0, np.nan, demo.obs['coef'].values ** 2)
    out2 = cna.tl.gene_corr(demo, ['coef', 'other'], key_added='corr_', engine=eng)
    assert list(out2.columns) == ['coef', 'other'] and len(eng.uploads) == 1
    np.testing.assert_array_equal(demo.var['corr_other'].values, out2['other'].values)
    np.testing.assert_array_equal(demo.var['corr_coef'].values, out['coef'].values)
    # a layer, and data without var names
    demo.layers['sq'] = np.ascontiguousarray(demo.X.astype(np.float64) ** 2)
    out3 = cna.tl.gene_corr(demo, 'coef', layer='sq', engine=eng)
    np.testing.assert_allclose(out3['coef'].values, restated_gene_corr(demo.layers['sq'], demo.obs['coef'].values)[0],
                               rtol=0, atol=0)
    bare = _frame(len(demo.obs), X=demo.X, coef=demo.obs['coef'].values)
    out4 = cna.tl.gene_corr(bare, 'coef', key_added='r_', engine=eng)
    assert isinstance(out4.index, pd.RangeIndex) and list(bare.var.columns) == ['r_coef']


def test_bad_arguments_raise_before_any_upload(demo):
    import cna_amd as cna
    eng = GeneEngine()
    n = len(demo.obs)
    with pytest.raises(KeyError, match='nope'):
        cna.tl.gene_corr(demo, ['coef', 'nope'], engine=eng)
    many = _frame(n, X=demo.X, **{'k%d' % j: np.arange(n, dtype=float) for j in range(17)})
    with pytest.raises(ValueError, match='16'):
        cna.tl.gene_corr(many, ['k%d' % j for j in range(17)], engine=eng)
    assert cna.tl.gene_corr(many, ['k%d' % j for j in range(16)], engine=GeneEngine()).shape == (demo.X.shape[1], 16)
    with pytest.raises(ValueError):
        cna.tl.gene_corr(demo, [], engine=eng)
    with pytest.raises(ValueError, match='rows'):
        cna.tl.gene_corr(_frame(n - 1, X=demo.X, coef=np.zeros(n - 1)), 'coef', engine=eng)
    with pytest.raises(TypeError, match='C-contiguous'):
        cna.tl.gene_corr(_frame(n, X=np.asfortranarray(demo.X), coef=np.zeros(n)), 'coef', engine=eng)
    for bad in (demo.X.astype(np.float16), demo.X.astype(np.int32), sp.coo_matrix(demo.X), demo.X.tolist(),
                sp.csr_matrix(demo.X).astype(np.int64)):
        with pytest.raises(TypeError):
            cna.tl.gene_corr(_frame(n, X=bad, coef=np.zeros(n)), 'coef', engine=eng)
    with pytest.raises(ValueError, match='data.X'):
        cna.tl.gene_corr(_frame(n, coef=np.zeros(n)), 'coef', engine=eng)
    with pytest.raises(KeyError):
        cna.tl.gene_corr(demo, 'coef', layer='missing', engine=eng)
    assert eng.uploads == []


def test_sharded_data_and_multi_rank_engines_are_refused(demo):
    import cna_amd as cna
    from cna_amd import dist
    eng = GeneEngine()
    part = dist.shard(demo, rank=0, nranks=2)
    part.X = demo.X[:len(part.obs)]
    part.obs['coef'] = 1.0
    with pytest.raises(NotImplementedError):
        cna.tl.gene_corr(part, 'coef', engine=eng)
    with pytest.raises(NotImplementedError):
        cna.tl.gene_corr(demo, 'coef', engine=GeneEngine(nranks=2))
    assert eng.uploads == []


# ------------------------------------------------------------------ residency
@pytest.mark.parametrize('kind', ['dense', 'csr', 'csc'])
def test_residency_bookkeeping(kind):
    X = dense_expression(400, 20, seed=1) if kind == 'dense' else sparse_expression(400, 20, seed=1, fmt=kind)
    Y = X.copy()
    eng = GeneEngine()
    assert eng.ensure_expression(X) is True and eng.ensure_expression(X) is False and len(eng.uploads) == 1

    def edit(M):
        (M if kind == 'dense' else M.data)[...] *= 2.0
    edit(X)                                   # in place, not pinned: the content hash sees it
    assert eng.ensure_expression(X) is True and len(eng.uploads) == 2
    eng.pin_expression(X)
    assert eng.ensure_expression(X) is False
    (X if kind == 'dense' else X.data).reshape(-1)[X.size // 3 if kind == 'dense' else X.nnz // 3] += 1.0
    assert eng.ensure_expression(X) is False and len(eng.uploads) == 2     # pinned: the caller's promise stands in
    eng.unpin_expression()
    assert eng.ensure_expression(X) is True and len(eng.uploads) == 3
    assert eng.ensure_expression(Y) is True and len(eng.uploads) == 4      # another matrix replaces it
    assert eng.ensure_expression(Y) is False
    assert eng.ensure_expression(X) is True and len(eng.uploads) == 5
    eng.drop_expression()
    assert eng.resident is None
    assert eng.ensure_expression(X) is True and len(eng.uploads) == 6
    with pytest.raises(TypeError):
        eng.pin_expression([[1.0]])
