"""cna.tl.gene_nbhd_corr / cna.tl.nbhd_expr on the device (run with -m gpu on an MI355X).

Shapes where the kernels can still go wrong, not the workload's: 3 001 cells (no multiple of 64, many slabs of the moments
passes), k = 15, one empty row, one row of 200 entries, rows stored in descending column order; 1, T - 1, T, T + 1 and
2 T + 3 genes for the tile width T = 64; 1 and 3 steps; 1, 5 and 16 keys with no, one shared and differing masks.

Bounds: the numerators and the denominator equal cna.tl.diffuse of the same columns bit for bit; r, mean and sd lie within
F64_TOL = 1e-10 of the float64 restatement of tests/test_gene_nbhd_host.py (the project's bound for the GPU against an f64
restatement, tests/test_gpu_gene_corr.py; absolute, on values of order 1 -- the counts are 0 to about 5), NaN in the same places.  The
inputs are the host file's (seeds there); test_restatement_is_precise_on_the_parity_inputs shows the restatement itself
good to 1e-12 on them."""
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from test_gene_nbhd_host import (N_CELLS, SEED, awkward_graph, dense64, nbhd_inputs, nbhd_keys, restated_gene_nbhd_corr,
                                 restated_parts)

pytestmark = pytest.mark.gpu

F64_TOL = 1e-10
T = 64
G_ALL = 2 * T + 3
GENES = [1, T - 1, T, T + 1, G_ALL]
CNA_EINVAL, CNA_ESTATE = -1, -4
FORMS = ['dense-f32', 'dense-f64', 'csr-f32', 'csc-f64']


# ------------------------------------------------------------------ inputs, made once
class Inputs:
    def __init__(self):
        A, self.signal, X = nbhd_inputs(N_CELLS, G_ALL)
        A = awkward_graph(A)
        self.graphs = {'f32': A, 'f64': sp.csr_matrix((A.data.astype(np.float64), A.indices, A.indptr), shape=A.shape)}
        X[:, 1], X[:, 2], X[:, 3] = 0.0, 2.0, 3.0            # constant genes
        X[:, 4] = 0.0
        X[100, 4] = 5.0                                       # one entry
        self.X = X
        self._forms, self._parts, self._data = {}, {}, {}

    def form(self, name, G=G_ALL):
        key = (name, G)
        if key not in self._forms:
            kind, dt = name.split('-')
            M = np.ascontiguousarray(self.X[:, :G].astype(np.float32 if dt == 'f32' else np.float64))
            if kind != 'dense':
                M = sp.csr_matrix(M) if kind == 'csr' else sp.csc_matrix(M)
                M.sort_indices()
            self._forms[key] = M
        return self._forms[key]

    def parts(self, graph, nsteps):
        key = (graph, nsteps)
        if key not in self._parts:
            num, den = restated_parts(self.graphs[graph], self.X, nsteps)
            num.setflags(write=False)
            den.setflags(write=False)
            self._parts[key] = (num, den)
        return self._parts[key]

    def data(self, graph, form, G=G_ALL):
        from cna_amd import synth
        key = (graph, form, G)
        if key not in self._data:
            obs = pd.DataFrame({'coef': self.signal}, index=pd.Index(['cell_%d' % i for i in range(N_CELLS)], name='cell'))
            var = pd.DataFrame(index=pd.Index(['gene_%d' % g for g in range(G)], name='gene'))
            self._data[key] = synth.CellData(obs, self.graphs[graph], X=self.form(form, G), var=var)
        return self._data[key]


@pytest.fixture(scope='module')
def inp():
    return Inputs()


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _fresh_order(eng, monkeypatch, reorder):
    monkeypatch.setenv('CNA_REORDER', '1' if reorder else '0')
    eng.drop_graph()


# ------------------------------------------------------------------ 1. bit for bit against the walk
@pytest.mark.parametrize('reorder', [True, False])
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('graph', ['f32', 'f64'])
def test_parts_equal_the_dense_walk_bit_for_bit(eng, inp, monkeypatch, graph, form, reorder):
    import cna_amd as cna
    _fresh_order(eng, monkeypatch, reorder)
    data = inp.data(graph, form)
    E = dense64(inp.X)
    rs = np.random.RandomState(SEED)
    for nsteps, m in ((1, 1), (3, T - 1), (3, T), (1, 5)):
        genes = rs.choice(G_ALL, m, replace=False)
        num, den = cna.tl.nbhd_expr(data, [int(g) for g in genes], nsteps=nsteps, return_parts=True, engine=eng)
        if reorder:
            assert eng.perm is not None and not np.array_equal(eng.perm, np.arange(N_CELLS))
        else:
            assert eng.perm is None
        want = cna.tl.diffuse(data, np.column_stack([E[:, genes], np.ones(N_CELLS)]), nsteps, engine=eng)
        np.testing.assert_array_equal(num.values, want[:, :m])
        np.testing.assert_array_equal(den.values, want[:, m])
        assert list(num.columns) == ['gene_%d' % g for g in genes]
        # and near the float64 restatement (the walk's own bound is far tighter; this catches a wrong column or cell order)
        rnum, rden = inp.parts(graph, nsteps)
        np.testing.assert_allclose(num.values, rnum[:, genes], rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(den.values, rden, rtol=1e-10)
    eng.drop_graph()


def test_another_self_weight_equals_the_walk_too(eng, inp):
    import cna_amd as cna
    data = inp.data('f32', 'csr-f32')
    num, den = cna.tl.nbhd_expr(data, [0, 7], nsteps=2, self_weight=2.5, return_parts=True, engine=eng)
    want = cna.tl.diffuse(data, np.column_stack([dense64(inp.X)[:, [0, 7]], np.ones(N_CELLS)]), 2, self_weight=2.5, engine=eng)
    np.testing.assert_array_equal(num.values, want[:, :2])
    np.testing.assert_array_equal(den.values, want[:, 2])
    eng.colsums(1)


def test_csr_and_csc_uploads_give_the_same_bits(eng, inp):
    import cna_amd as cna
    X = inp.form('csr-f32')
    out = []
    for M in (X, sp.csc_matrix(X)):
        data = inp.data('f32', 'csr-f32')
        data.X = M
        m = cna.tl.nbhd_expr(data, list(range(0, 64)), nsteps=3, engine=eng)
        r = cna.tl.gene_nbhd_corr(data, 'coef', nsteps=3, engine=eng)
        assert eng.expression_shape()['format'] == 'gene-major'
        out.append((m.values, r.values, r.attrs['mean'].values, r.attrs['sd'].values))
    data.X = X
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 2. r, mean, sd against the restatement
def _check(tag, got, want):
    """got: the frame of gene_nbhd_corr; want: (r, mean, sd, n_cells) of the restatement"""
    r, mean, sd, n_cells = want
    names = list(got.columns)
    assert [got.attrs['n_cells'][k] for k in names] == [int(v) for v in n_cells], tag
    for what, g, w in (('r', got.values, r.T), ('mean', got.attrs['mean'].values, mean.T), ('sd', got.attrs['sd'].values, sd.T)):
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg='%s %s' % (tag, what))
        err = float(np.nanmax(np.abs(g - w))) if np.isfinite(w).any() else 0.0
        print('%s %s: max error %.3e (bound %g)' % (tag, what, err, F64_TOL))
        assert err <= F64_TOL, (tag, what, err)


@pytest.mark.parametrize('q,masks', [(1, 'none'), (5, 'equal'), (16, 'differ')])
@pytest.mark.parametrize('nsteps', [1, 3])
@pytest.mark.parametrize('G', GENES)
def test_against_restatement(eng, inp, G, nsteps, q, masks):
    import cna_amd as cna
    form = FORMS[(GENES.index(G) + nsteps + q) % len(FORMS)]
    graph = 'f64' if (G + q) % 2 else 'f32'
    data = inp.data(graph, form, G)
    V = nbhd_keys(inp.signal, q, masks)
    keys = ['k%d' % j for j in range(q)]
    for j, k in enumerate(keys):
        data.obs[k] = V[j]
    got = cna.tl.gene_nbhd_corr(data, keys, nsteps=nsteps, engine=eng)
    num, den = inp.parts(graph, nsteps)
    want = restated_gene_nbhd_corr(inp.graphs[graph], inp.X[:, :G], V, nsteps, parts=(num[:, :G], den))
    assert got.shape == (G, q) and got.attrs['nsteps'] == nsteps
    _check('G=%d nsteps=%d q=%d %s %s %s' % (G, nsteps, q, masks, graph, form), got, want)
    if G > 4:
        assert np.isnan(got.values[1:4]).all() and np.isfinite(got.values[0]).all() and np.isfinite(got.values[4]).all()


def test_tiles_of_32_columns_give_the_same_bits(eng, inp, monkeypatch):
    """Two rows per wave: every column still adds its entries and its slabs in the same order."""
    import cna_amd as cna
    data = inp.data('f32', 'dense-f32')
    data.obs['other'] = np.where(np.arange(N_CELLS) % 11 == 0, np.nan, -inp.signal)
    out = []
    for tile in ('64', '32'):
        monkeypatch.setenv('CNA_NBHD_TILE', tile)
        r = cna.tl.gene_nbhd_corr(data, ['coef', 'other'], nsteps=3, engine=eng)
        out.append((r.values, r.attrs['mean'].values, r.attrs['sd'].values))
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 3. exact cases
@pytest.mark.parametrize('form', FORMS)
def test_constant_genes_and_one_entry(eng, inp, form):
    import cna_amd as cna
    data = inp.data('f32', form)
    out = cna.tl.gene_nbhd_corr(data, 'coef', nsteps=1, engine=eng)
    r, mean = out['coef'].values, out.attrs['mean']['coef'].values
    assert np.isnan(r[1:4]).all() and np.isfinite(np.delete(r, [1, 2, 3])).all()
    assert mean[1] == 0.0 and mean[2] == 2.0 and abs(mean[3] - 3.0) < 1e-14
    # gene 4 holds 5.0 in cell 100 alone: after one step its numerator is 5 (A[i, 100] + w [i == 100]) / c[100], one product
    A = inp.graphs['f32']
    c = eng.fetch_colsums()
    col = np.asarray(sp.csr_matrix((A.data.astype(np.float64), A.indices, A.indptr), shape=A.shape)[:, 100].todense()).ravel()
    col[100] += 1.0
    num, den = cna.tl.nbhd_expr(data, [4], nsteps=1, return_parts=True, engine=eng)
    np.testing.assert_array_equal(num.values[:, 0], col * (5.0 / c[100]))
    m = cna.tl.nbhd_expr(data, ['gene_4'], nsteps=1, engine=eng)['gene_4'].values
    np.testing.assert_array_equal(m, num.values[:, 0] / den.values)
    assert (m > 0).sum() == (col > 0).sum() and m[5] == 0.0                 # (the empty row keeps its own term only)


def test_repeatable(eng, inp):
    import cna_amd as cna
    data = inp.data('f64', 'csc-f64')
    data.obs['other'] = np.where(np.arange(N_CELLS) % 7 == 0, np.nan, inp.signal ** 2)

    def both():
        r = cna.tl.gene_nbhd_corr(data, ['coef', 'other'], nsteps=3, engine=eng)
        m = cna.tl.nbhd_expr(data, [0, 9, 130], nsteps=3, engine=eng)
        return r.values, r.attrs['mean'].values, r.attrs['sd'].values, m.values

    first, second = both(), both()
    eng.drop_expression()
    eng.drop_graph()
    third = both()
    for a, b, c in zip(first, second, third):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)


# ------------------------------------------------------------------ 4. the rest of the engine is left alone
def test_walk_state_nam_cache_pending_null_and_memory_are_left_alone():
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd.engine import Engine
    from test_gpu_gene_corr import _walk
    n, N = 20000, 30
    data, meta = synth.make_dataset(n, N, k=15, seed=0)
    rs = np.random.RandomState(SEED)
    data.X = rs.poisson(0.3, (n, 70)).astype(np.float32)
    e = Engine()
    e.reuse_nam = True
    try:
        kw = dict(nsteps=3, Nnull=200, seed=0, key_added='coef', engine=e, return_full=True)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            a1 = cna.tl.association(data, meta['y'], 'id', **kw).materialize()
            coef1, fdr1 = data.obs['coef'].values.copy(), data.obs['coef_fdr'].values.copy()
            e.prof_reset()
            e.prof_enable(True)
            r = cna.tl.gene_nbhd_corr(data, 'coef', nsteps=3, engine=e)
            m = cna.tl.nbhd_expr(data, [0, 1, 2], nsteps=3, engine=e)
            a2 = cna.tl.association(data, meta['y'], 'id', **kw).materialize()
            e.sync()
            e.prof_enable(False)
        prof = e.prof()
        assert not any(k.startswith('nam_') for k in prof), prof          # the cached NAM served: no walk step ran
        assert a1.p == a2.p and a1.k == a2.k
        np.testing.assert_array_equal(a1.ncorrs.values, a2.ncorrs.values)
        np.testing.assert_array_equal(a1.nam.values, a2.nam.values)
        np.testing.assert_array_equal(data.obs['coef'].values, coef1)
        np.testing.assert_array_equal(data.obs['coef_fdr'].values, fdr1)
        assert np.isfinite(r.values).all() and np.isfinite(m.values).all()
        # the work buffers go with the matrix
        e.drop_expression()
        base = e.device_bytes()
        r2 = cna.tl.gene_nbhd_corr(data, 'coef', nsteps=3, engine=e)
        cna.tl.nbhd_expr(data, [0, 1, 2], nsteps=3, engine=e)
        np.testing.assert_array_equal(r2.values, r.values)
        assert e.device_bytes() > base
        e.drop_expression()
        assert e.device_bytes() == base
        # between the launch and the fetch of a local-null pass
        P = 640
        y = rs.randn(N)
        y = (y - y.mean()) / y.std()
        Y = np.column_stack([y, rs.randn(N, P)])
        out, calls = [], []
        for insert in (False, True):
            e.null_local_discard()
            e.drop_graph()
            _walk(e, data, N)
            nz, maxabs = e.select_standardized(None, None, y=y)
            maxcorr = max(maxabs, 0.001)
            thr = np.arange(maxcorr / 4, maxcorr, maxcorr / 400)
            edges = thr ** 2 - 1e-8 - 1e-5 * thr ** 2
            e.condition(np.eye(N), Y)
            e.null_local_launch(1, P, edges, thr)
            if insert:
                e.ensure_expression(data.X)
                calls.append(e.gene_nbhd_corr(data.obs['coef'].values[None, :], 3)[0])
                calls.append(e.nbhd_expr([0, 1, 2], 3))
            out.append([np.asarray(f).copy() for f in e.null_local_fetch()])
        for a, b in zip(*out):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(calls[0][0], r['coef'].values)
        np.testing.assert_array_equal(calls[1][0] / calls[1][1][:, None], m.values)
    finally:
        e.close()


# ------------------------------------------------------------------ 5. refusals
def _raw_calls(e, n, G):
    from cna_amd._ffi import ptr
    V = np.zeros((1, n))
    outs = [np.full((1, G), 7.0) for _ in range(3)]
    cells = np.full(1, 7, dtype=np.int64)
    num, den = np.full((n, 1), 7.0), np.full(n, 7.0)
    genes = np.zeros(1, dtype=np.int32)
    rc1 = e.lib.cna_gene_nbhd_corr(e.h, ptr(V), 1, 3, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(cells), None)
    msg1 = e.lib.cna_last_error()
    rc2 = e.lib.cna_nbhd_expr(e.h, ptr(genes), 1, 3, ptr(num), ptr(den))
    msg2 = e.lib.cna_last_error()
    untouched = all((a == 7).all() for a in outs + [cells, num, den])
    return (rc1, msg1), (rc2, msg2), untouched


def test_refusals(inp):
    from cna_amd.engine import Engine
    from cna_amd._ffi import ptr
    A, X = inp.graphs['f32'], inp.form('dense-f32')
    n, G = X.shape
    e = Engine()
    try:
        def refused(code, word):
            a, b, untouched = _raw_calls(e, n, G)
            assert a[0] == code and b[0] == code, (a, b)
            assert word in a[1] and word in b[1], (a, b)
            assert untouched

        e.ensure_expression(X)
        refused(CNA_ESTATE, b'cna_graph_upload')                 # no graph
        e.ensure_graph(A)
        refused(CNA_ESTATE, b'cna_colsums')                      # no column sums
        e.colsums(1)
        e.drop_expression()
        refused(CNA_ESTATE, b'no expression matrix')
        e.ensure_expression(np.ascontiguousarray(X[:-1]))
        refused(CNA_EINVAL, b'cells')                            # cell counts that differ
        e.ensure_expression(X)
        # arguments out of range
        V = np.zeros((17, n))
        o = [np.full((17, G), 7.0) for _ in range(3)]
        cells = np.zeros(17, dtype=np.int64)
        for q, nsteps in ((0, 3), (17, 3), (1, 0), (1, 16)):
            assert e.lib.cna_gene_nbhd_corr(e.h, ptr(V), q, nsteps, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(cells), None) == CNA_EINVAL
        num, den = np.full((n, 65), 7.0), np.full(n, 7.0)
        for genes, nsteps in (([0] * 65, 3), ([], 3), ([G], 3), ([-1], 3), ([0], 0), ([0], 16)):
            g = np.asarray(genes, dtype=np.int32)
            assert e.lib.cna_nbhd_expr(e.h, ptr(g), len(genes), nsteps, ptr(num), ptr(den)) == CNA_EINVAL
        assert all((a == 7).all() for a in o + [num, den])
        r = e.gene_nbhd_corr(inp.signal[None, :], 1)[0]             # and the context still works
        assert np.isfinite(np.delete(r[0], [1, 2, 3])).all()
    finally:
        e.close()
    e = Engine(device=0, rank=0, nranks=1, unique_id=Engine.new_unique_id())
    try:
        e.ensure_graph(A)
        e.colsums(1)
        e.ensure_expression(X)
        a, b, untouched = _raw_calls(e, n, G)
        assert a[0] == CNA_ESTATE and b[0] == CNA_ESTATE and b'communicator' in a[1] and b'communicator' in b[1] and untouched
    finally:
        e.close()
