"""cna.tl.gene_nbhd_corr / cna.tl.nbhd_expr on the CPU: the numpy restatement of the definition (what the GPU tests compare
with), its check against independent routes, the argument checks and the assembly of the frames over a stub engine.

The definition: with one walk step P s = A.(s/c) + w*s/c, c = A.sum(0) + w, and e_g the gene's column in float64,
m_g = (P^nsteps e_g) / (P^nsteps 1) element-wise; a cell whose denominator is not a positive finite number is left out.
The restatement's walk is oracle.cna_oracle.diffuse(mode='f64').

Inputs (shared with tests/test_gpu_gene_nbhd.py), all from fixed seeds: synth.mixture_points(n, seed=SEED) with SEED = 11,
the fuzzy kNN graph of the cKDTree builder with k = 15, Poisson genes at about 23 % density whose rate follows a smooth
per-cell signal (numpy RandomState(SEED + 1))."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from oracle import cna_oracle as orc

SEED = 11
K = 15
N_CELLS = 3001          # not a multiple of 64, more rows than one slab of the moments pass


# ------------------------------------------------------------------ inputs
def smooth_signal(pts):
    """A per-cell signal that varies smoothly over the point cloud, standardised."""
    z = np.tanh(0.35 * pts[:, 0].astype(np.float64)) + 0.5 * np.sin(0.25 * pts[:, 1].astype(np.float64))
    return (z - z.mean()) / z.std()


def poisson_genes(signal, n_genes, seed=SEED + 1, dtype=np.float32):
    """cells x genes Poisson counts at about 23 % density: rate 0.26 exp(a_g * signal - a_g^2 / 2), |a_g| in [0.25, 0.75]."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(0.25, 0.75, n_genes) * rs.choice([-1.0, 1.0], n_genes)
    rate = 0.26 * np.exp(signal[:, None] * a[None, :] - 0.5 * a[None, :] ** 2)
    return rs.poisson(rate).astype(dtype)


def nbhd_inputs(n=N_CELLS, n_genes=40, graph_dtype=np.float32):
    """(graph CSR, signal, X dense float32 cells x genes)."""
    from cna_amd import synth
    pts, _ = synth.mixture_points(n, seed=SEED)
    A = synth.fuzzy_knn_graph(pts, k=K, dtype=graph_dtype, builder='cpu')
    signal = smooth_signal(pts)
    return A, signal, poisson_genes(signal, n_genes)


def awkward_graph(A, empty_row=5, hub_row=17, hub_entries=200, seed=SEED + 2):
    """The same graph with one empty row, one row of `hub_entries` entries and, in every third row, the stored entries in
    descending column order (no kNN builder emits any of the three)."""
    rs = np.random.RandomState(seed)
    A = sp.csr_matrix(A, copy=True)
    n = A.shape[0]
    rows = []
    for i in range(n):
        lo, hi = A.indptr[i], A.indptr[i + 1]
        idx, val = A.indices[lo:hi].copy(), A.data[lo:hi].copy()
        if i == empty_row:
            idx, val = idx[:0], val[:0]
        elif i == hub_row:
            extra = np.setdiff1d(rs.choice(n, 3 * hub_entries, replace=False), np.append(idx, i))[:hub_entries - len(idx)]
            idx = np.concatenate([idx, extra.astype(idx.dtype)])
            val = np.concatenate([val, rs.uniform(0.05, 1.0, len(extra)).astype(val.dtype)])
            assert len(idx) == hub_entries
        if i % 3 == 0:
            idx, val = idx[::-1].copy(), val[::-1].copy()
        rows.append((idx, val))
    indptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(A.indptr.dtype)
    out = sp.csr_matrix((np.concatenate([r[1] for r in rows]), np.concatenate([r[0] for r in rows]), indptr), shape=A.shape)
    assert not out.has_sorted_indices
    return out


def dense64(X):
    return np.asarray(X.toarray() if sp.issparse(X) else X, dtype=np.float64)


# ------------------------------------------------------------------ the restatement
def _walk_longdouble(A, s, nsteps, w):
    """The same walk in np.longdouble (scipy's products do not take the type): entries added with np.add.at."""
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    data = A.data.astype(np.longdouble)
    c = np.zeros(A.shape[0], dtype=np.longdouble)
    np.add.at(c, A.indices, data)
    c = c + np.longdouble(w)
    s = s.astype(np.longdouble)
    for _ in range(nsteps):
        t = s / c[:, None]
        new = np.longdouble(w) * t
        np.add.at(new, rows, data[:, None] * t[A.indices])
        s = new
    return s


def restated_parts(A, X, nsteps, w=1, dtype=np.float64):
    """(numerators cells x genes, denominator cells) of the definition."""
    E = dense64(X)
    ones = np.ones((E.shape[0], 1))
    if dtype == np.float64:
        return orc.diffuse(A, E, nsteps, w, mode='f64'), orc.diffuse(A, ones, nsteps, w, mode='f64')[:, 0]
    return _walk_longdouble(A, E, nsteps, w), _walk_longdouble(A, ones, nsteps, w)[:, 0]


def restated_nbhd_expr(A, X, nsteps, w=1, dtype=np.float64):
    num, den = restated_parts(A, X, nsteps, w, dtype)
    good = np.isfinite(den) & (den > 0)
    with np.errstate(all='ignore'):
        return np.where(good[:, None], num / den[:, None], np.nan)


def restated_gene_nbhd_corr(A, X, V, nsteps, w=1, dtype=np.float64, parts=None):
    """(r, mean, sd: q x genes; n_cells: q) of cna_gene_nbhd_corr: per key the cells where the key is finite and the
    denominator good; two-pass moments of m; NaN for a gene constant over all cells of the raw matrix (minimum == maximum),
    a constant key, fewer than two cells.  parts: restated_parts of the same arguments, when the caller has them."""
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    num, den = restated_parts(A, X, nsteps, w, dtype) if parts is None else parts
    good = np.isfinite(den) & (den > 0)
    with np.errstate(all='ignore'):
        m = np.where(good[:, None], num / den[:, None], np.nan)
    E = dense64(X)
    constant = E.min(axis=0) == E.max(axis=0)
    q, G = V.shape[0], E.shape[1]
    r, mean, sd = (np.full((q, G), np.nan) for _ in range(3))
    n_cells = np.zeros(q, dtype=np.int64)
    for j, v in enumerate(V):
        keep = np.isfinite(v) & good
        n = int(keep.sum())
        n_cells[j] = n
        if n == 0:
            continue
        mk = m[keep]
        vk = v[keep].astype(dtype)
        mu = mk.sum(axis=0) / n
        d = mk - mu
        s2 = (d * d).sum(axis=0)
        mean[j], sd[j] = mu, np.sqrt(s2 / n)
        if n < 2 or vk.min() == vk.max():
            continue
        vc = vk - vk.sum() / n
        with np.errstate(all='ignore'):
            rr = (d * vc[:, None]).sum(axis=0) / np.sqrt(s2) / np.sqrt((vc * vc).sum())
            rr = np.where(np.isnan(rr), rr, np.clip(rr, -1.0, 1.0)).astype(np.float64)
        rr[constant] = np.nan
        r[j] = rr
    return r, mean, sd, n_cells


def nbhd_keys(signal, q, masks='none', seed=SEED + 3):
    """q key columns (q x cells): the signal plus noise of growing size; masks 'none' all finite, 'equal' the same 7 % of the
    cells NaN in every key, 'differ' each key its own share."""
    rs = np.random.RandomState(seed + q)
    n = len(signal)
    V = signal[None, :] * (1.0 + 0.25 * np.arange(q))[:, None] + rs.randn(q, n) * (0.2 + 0.1 * np.arange(q))[:, None] + np.arange(q)[:, None]
    if masks == 'equal':
        V[:, rs.rand(n) < 0.07] = np.nan
    elif masks == 'differ':
        for j in range(q):
            V[j, rs.rand(n) < 0.03 * (1 + j % 4)] = np.nan
    return V


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope='module')
def inputs():
    A, signal, X = nbhd_inputs()
    A.sort_indices()
    return A, signal, X


@pytest.fixture(scope='module')
def m3(inputs):
    A, _, X = inputs
    m = restated_nbhd_expr(A, X, 3)
    m.setflags(write=False)
    return m


# ------------------------------------------------------------------ the restatement against independent routes
def test_adjoint_identity_of_the_numerators(inputs):
    """sum_i v_i (P^s e)_i = sum_j ((P^T)^s v)_j e_j, the right side with scipy's transposed product."""
    A, signal, X = inputs
    E = dense64(X)
    num, den = restated_parts(A, X, 3)
    A64 = sp.csr_matrix(A, dtype=np.float64)
    c = np.asarray(A64.sum(axis=0)).ravel() + 1.0
    for v in (signal, np.ones(len(signal)), np.random.RandomState(SEED).randn(len(signal))):
        u = v.copy()
        for _ in range(3):
            u = (A64.T.dot(u) + u) / c
        left, right = v.dot(num), u.dot(E)
        np.testing.assert_allclose(left, right, rtol=1e-11, atol=0)
        np.testing.assert_allclose(v.dot(den), u.sum(), rtol=1e-11)


def test_r_is_corrcoef_of_the_neighbourhood_means(inputs, m3):
    A, signal, X = inputs
    V = nbhd_keys(signal, 3, 'differ')
    r, mean, sd, n_cells = restated_gene_nbhd_corr(A, X, V, 3)
    for j, v in enumerate(V):
        keep = np.isfinite(v)
        assert n_cells[j] == keep.sum() < len(v)
        want = np.corrcoef(v[keep], m3[keep].T)[0, 1:]
        np.testing.assert_allclose(r[j], want, rtol=0, atol=1e-12)
        np.testing.assert_allclose(mean[j], m3[keep].mean(axis=0), rtol=1e-13)
        np.testing.assert_allclose(sd[j], m3[keep].std(axis=0), rtol=1e-12)


def test_restatement_is_precise_on_the_parity_inputs(inputs, m3):
    """float64 against np.longdouble to 1e-12, and the condition that makes it so: sd(m) >= 1e-3 |mean(m)| for every
    non-constant gene."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip('np.longdouble is float64 on this platform')
    A, signal, X = inputs
    V = nbhd_keys(signal, 5, 'differ')
    for nsteps in (1, 3):
        r, mean, sd, _ = restated_gene_nbhd_corr(A, X, V, nsteps)
        rl, meanl, sdl, _ = restated_gene_nbhd_corr(A, X, V, nsteps, dtype=np.longdouble)
        live = dense64(X).min(axis=0) != dense64(X).max(axis=0)
        ratio = float((sd[:, live] / np.abs(mean[:, live])).min())
        err = max(float(np.abs(r - rl.astype(np.float64)).max()), float(np.abs(mean / meanl.astype(np.float64) - 1).max()),
                  float(np.abs(sd / sdl.astype(np.float64) - 1).max()))
        print('nsteps=%d: min sd(m)/|mean(m)| = %.3e (needs >= 1e-3), max |f64 - longdouble| = %.3e (bound 1e-12)'
              % (nsteps, ratio, err))
        assert ratio >= 1e-3
        assert err <= 1e-12


def test_the_neighbourhood_means_carry_the_signal(inputs, m3):
    """What the tool is for: the same genes, signal and graph -- |r| against single cells is small, against the
    neighbourhood means it is not."""
    _, signal, X = inputs
    single = np.abs(np.corrcoef(signal, dense64(X).T)[0, 1:])
    nbhd = np.abs(np.corrcoef(signal, m3.T)[0, 1:])
    print('median |r|: single cells %.3f, neighbourhood means %.3f' % (np.median(single), np.median(nbhd)))
    assert np.median(single) < 0.3 and np.median(nbhd) > 0.6


def test_constant_genes_give_nan(inputs):
    A, signal, X = inputs
    X = X[:, :6].copy()
    X[:, 1], X[:, 2], X[:, 3] = 0.0, 2.0, 3.0
    r, mean, sd, _ = restated_gene_nbhd_corr(A, X, signal, 3)
    assert np.isnan(r[0, 1:4]).all() and np.isfinite(r[0, [0, 4, 5]]).all()
    m = restated_nbhd_expr(A, X, 3)
    assert (m[:, 2] == 2.0).all()                   # a power of two comes back exactly ...
    assert (m[:, 3] != 3.0).any()                   # ... 3.0 does not: the decision cannot be taken from m
    np.testing.assert_allclose(mean[0, 1:4], [0.0, 2.0, 3.0], rtol=1e-15)


def test_a_key_with_nan_cells(inputs, m3):
    A, signal, X = inputs
    v = signal.copy()
    v[::7] = np.nan
    r, _, _, n_cells = restated_gene_nbhd_corr(A, X, v, 3)
    keep = np.isfinite(v)
    assert n_cells[0] == keep.sum()
    np.testing.assert_allclose(r[0], np.corrcoef(v[keep], m3[keep].T)[0, 1:], atol=1e-12)


def test_a_cell_without_mass_is_left_out():
    """A negative self weight that cancels a column's sum: the quotient s/c is not finite there, and so is the
    denominator of every neighbourhood that reaches the cell."""
    A = sp.csr_matrix(np.array([[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 2.0], [0, 0, 2.0, 0]]))
    X = np.array([[1.0], [2.0], [3.0], [5.0]])
    with np.errstate(all='ignore'):
        m = restated_nbhd_expr(A, X, 1, w=-1)
        r, mean, sd, n_cells = restated_gene_nbhd_corr(A, X, np.arange(4.0), 1, w=-1)
    assert np.isnan(m[:2]).all() and np.isfinite(m[2:]).all()
    assert n_cells[0] == 2


# ------------------------------------------------------------------ the tool over a stub engine
class StubEngine:
    """Counts what the tool asks of an engine; the two reductions are the restatement."""
    nranks = 1

    def __init__(self, nranks=1):
        self.nranks = nranks
        self.calls = []
        self.A = self.X = None
        self._nam_sig = 'kept'

    def ensure_graph(self, A, shard=None, defer=False):
        self.calls.append('ensure_graph')
        new = self.A is not A
        self.A = A
        return new

    def colsums(self, w=1):
        self.calls.append(('colsums', w))
        self.w = w

    def ensure_expression(self, X):
        self.calls.append('ensure_expression')
        self.X = X

    def gene_nbhd_corr(self, V, nsteps):
        self.calls.append(('gene_nbhd_corr', nsteps))
        return restated_gene_nbhd_corr(self.A, self.X, V, nsteps, self.w)

    def nbhd_expr(self, genes, nsteps):
        self.calls.append(('nbhd_expr', nsteps))
        return restated_parts(self.A, dense64(self.X)[:, genes], nsteps, self.w)


@pytest.fixture()
def data(inputs):
    from cna_amd import synth
    A, signal, X = inputs
    G = X.shape[1]
    obs = pd.DataFrame({'coef': signal, 'other': -2.0 * signal + 1.0, 'label': ['a'] * len(signal)},
                       index=pd.Index(['cell_%d' % i for i in range(len(signal))], name='cell'))
    obs.loc[obs.index[::9], 'other'] = np.nan
    return synth.CellData(obs, A, X=X, var=pd.DataFrame(index=pd.Index(['gene_%d' % g for g in range(G)], name='gene')))


def test_exported():
    import cna_amd as cna
    assert 'gene_nbhd_corr' in cna.tl.__all__ and 'nbhd_expr' in cna.tl.__all__
    assert callable(cna.tl.gene_nbhd_corr) and callable(cna.tl.nbhd_expr)


def test_argument_checks_come_before_the_engine(data):
    import cna_amd as cna
    from cna_amd import synth
    e = StubEngine()
    with pytest.raises(TypeError, match='nsteps'):
        cna.tl.gene_nbhd_corr(data, 'coef', engine=e)
    with pytest.raises(TypeError, match='nsteps'):
        cna.tl.nbhd_expr(data, ['gene_0'], engine=e)
    for bad in (0, 16):
        with pytest.raises(ValueError, match='nsteps'):
            cna.tl.gene_nbhd_corr(data, 'coef', nsteps=bad, engine=e)
        with pytest.raises(ValueError, match='nsteps'):
            cna.tl.nbhd_expr(data, ['gene_0'], nsteps=bad, engine=e)
    with pytest.raises(TypeError, match='nsteps'):
        cna.tl.gene_nbhd_corr(data, 'coef', nsteps=2.0, engine=e)
    for k in range(17):
        data.obs['k%d' % k] = data.obs['coef'].values + k
    with pytest.raises(ValueError, match='at most 16'):
        cna.tl.gene_nbhd_corr(data, ['k%d' % k for k in range(17)], nsteps=3, engine=e)
    with pytest.raises(ValueError, match='at most 64'):
        cna.tl.nbhd_expr(data, list(range(40)) + list(range(25)), nsteps=3, engine=e)
    with pytest.raises(ValueError, match='at least one'):
        cna.tl.nbhd_expr(data, [], nsteps=3, engine=e)
    with pytest.raises(KeyError):
        cna.tl.nbhd_expr(data, ['gene_0', 'no_such_gene'], nsteps=3, engine=e)
    with pytest.raises(IndexError):
        cna.tl.nbhd_expr(data, [40], nsteps=3, engine=e)
    with pytest.raises(TypeError, match='not numeric'):
        cna.tl.gene_nbhd_corr(data, 'label', nsteps=3, engine=e)
    with pytest.raises(KeyError):
        cna.tl.gene_nbhd_corr(data, 'missing', nsteps=3, engine=e)
    short = synth.CellData(data.obs, data.obsp['connectivities'], X=data.X[:-1])
    with pytest.raises(ValueError, match='rows'):
        cna.tl.gene_nbhd_corr(short, 'coef', nsteps=3, engine=e)
    with pytest.raises(ValueError, match='rows'):
        cna.tl.nbhd_expr(short, [0], nsteps=3, engine=e)
    assert e.calls == []
    # sharded data and a multi-rank engine are refused, nothing uploaded
    data.uns['cna_shard'] = {'row0': 0, 'n_global': 2 * len(data.obs)}
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.gene_nbhd_corr(data, 'coef', nsteps=3, engine=e)
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.nbhd_expr(data, [0], nsteps=3, engine=e)
    del data.uns['cna_shard']
    e2 = StubEngine(nranks=2)
    with pytest.raises(NotImplementedError, match='multi-rank'):
        cna.tl.gene_nbhd_corr(data, 'coef', nsteps=3, engine=e2)
    assert e.calls == [] and e2.calls == []


def test_gene_nbhd_corr_frames(data, inputs):
    import cna_amd as cna
    A, signal, X = inputs
    e = StubEngine()
    out = cna.tl.gene_nbhd_corr(data, ['coef', 'other'], nsteps=3, key_added='nb_', engine=e)
    assert e.calls == ['ensure_graph', ('colsums', 1), 'ensure_expression', ('gene_nbhd_corr', 3)]
    assert e._nam_sig is None                      # (a graph the engine had not seen)
    V = np.stack([data.obs['coef'].values, data.obs['other'].values])
    r, mean, sd, n_cells = restated_gene_nbhd_corr(A, X, V, 3)
    assert out.index.equals(data.var_names) and list(out.columns) == ['coef', 'other']
    np.testing.assert_array_equal(out.values, r.T)
    assert out.attrs['nsteps'] == 3
    assert out.attrs['n_cells'] == {'coef': len(signal), 'other': int(np.isfinite(V[1]).sum())}
    for name, want in (('mean', mean), ('sd', sd)):
        f = out.attrs[name]
        assert f.index.equals(data.var_names) and list(f.columns) == ['coef', 'other']
        np.testing.assert_array_equal(f.values, want.T)
    np.testing.assert_array_equal(data.var['nb_coef'].values, out['coef'].values)
    np.testing.assert_array_equal(data.var['nb_other'].values, out['other'].values)
    assert np.median(np.abs(out['coef'].values)) > 0.6 and (np.sign(out['coef']) == -np.sign(out['other'])).all()
    # the engine's cached NAM is not dropped for a graph it holds already; another self weight reaches the column sums
    e._nam_sig = 'kept'
    one = cna.tl.gene_nbhd_corr(data, 'coef', nsteps=1, self_weight=2, engine=e)
    assert e._nam_sig == 'kept' and ('colsums', 2) in e.calls and list(one.columns) == ['coef']
    assert 'nb_coef' in data.var and one.attrs['nsteps'] == 1


def test_nbhd_expr_frames(data, inputs, m3):
    import cna_amd as cna
    A, signal, X = inputs
    e = StubEngine()
    out = cna.tl.nbhd_expr(data, ['gene_3', 7, 'gene_0'], nsteps=3, key_added='m_', engine=e)
    assert e.calls == ['ensure_graph', ('colsums', 1), 'ensure_expression', ('nbhd_expr', 3)]
    assert list(out.columns) == ['gene_3', 'gene_7', 'gene_0'] and out.index.equals(data.obs.index)
    np.testing.assert_array_equal(out.values, m3[:, [3, 7, 0]])
    for g in ('gene_3', 'gene_7', 'gene_0'):
        np.testing.assert_array_equal(data.obs['m_' + g].values, out[g].values)
    num, den = cna.tl.nbhd_expr(data, 'gene_3', nsteps=3, return_parts=True, engine=e)
    want_num, want_den = restated_parts(A, X[:, [3]], 3)
    np.testing.assert_array_equal(num.values, want_num)
    np.testing.assert_array_equal(den.values, want_den)
    assert list(num.columns) == ['gene_3'] and den.index.equals(data.obs.index)
    # without var_names: positions label the columns
    data.var = None
    out = cna.tl.nbhd_expr(data, [2, 5], nsteps=1, engine=e)
    assert list(out.columns) == [2, 5]
