"""cna.tl.gene_corr on the device (run with -m gpu on an MI355X).

Bounds: 1e-5 absolute on r against the reference's own line (the project's rule for floats against the reference; |r| <= 1),
1e-10 absolute on r against the float64 numpy restatement of tests/test_gene_corr_host.py (GPU against an
f64 restatement).  Every parity input is benign for the raw-moment variance (test_parity_inputs_are_benign_for_raw_moments
checks sum x^2 / sum (x - mean)^2 <= 100 on the CPU), so the second bound tests the kernels and not the formula.
The observed maxima are written to the file CNA_GENE_CORR_PARITY_OUT names, when it is set (profiles/r07_gene_corr_parity.txt
is such a run's output)."""
import os
import time

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from test_gene_corr_host import (restated_gene_corr, demo_line, sparse_expression, dense_expression, big_sparse_expression,
                                 keys_for, PARITY_Q)

pytestmark = pytest.mark.gpu

REF_TOL = 1e-5      # floats against the reference (north_star)
F64_TOL = 1e-10     # GPU against an f64 restatement
_seen = {}


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()
    if os.environ.get('CNA_GENE_CORR_PARITY_OUT') and _seen:
        with open(os.environ['CNA_GENE_CORR_PARITY_OUT'], 'w') as f:
            f.write('max |r_gpu - r_restated| per case of tests/test_gpu_gene_corr.py (bound %g; demo line: %g)\n'
                    % (F64_TOL, REF_TOL))
            for k in sorted(_seen):
                f.write('%-58s %.3e\n' % (k, _seen[k]))
            f.write('%-58s %.3e\n' % ('maximum', max(_seen.values())))


def _check(name, got, want, tol=F64_TOL):
    got, want = np.asarray(got), np.asarray(want)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=name)
    err = float(np.nanmax(np.abs(got - want))) if np.isfinite(want).any() else 0.0
    _seen[name] = max(err, _seen.get(name, 0.0))
    print('%s: max |dr| = %.3e (bound %g)' % (name, err, tol))
    assert err <= tol, (name, err)


def _run(eng, X, V):
    eng.ensure_expression(X)
    return eng.gene_corr(V)


# ------------------------------------------------------------------ 1. the demo's line
def test_the_demo_line(eng):
    import cna_amd as cna
    from cna_amd import synth
    data, samplem = synth.make_demo_like(keep_expression=True)
    cna.tl.association(data, samplem['case'].astype(float), 'id', key_added='coef', Nnull=200, seed=0, engine=eng)
    out = cna.tl.gene_corr(data, 'coef', key_added='corr_', engine=eng)
    v = data.obs['coef'].values
    w = np.isfinite(v)
    assert w.sum() > 0.9 * len(v)
    want = demo_line(v[w], data.X[w])
    assert out.index.equals(data.var_names) and list(out.columns) == ['coef']
    _check('demo line', out['coef'].values, want, REF_TOL)
    _check('demo line vs restatement', out['coef'].values, restated_gene_corr(data.X, v)[0])
    np.testing.assert_array_equal(data.var['corr_coef'].values, out['coef'].values)
    assert np.abs(want).max() > 0.2          # the coefficient does pick out genes


# ------------------------------------------------------------------ 2. against the restatement
N_ODD = 3001      # prime-ish: a multiple of no slab, chunk or unroll size
# PARITY_Q = [1, 2, 3, 5, 8, 16] key columns: the kernels are instantiated for Q = 1, 2, 4, 8, 16 slots, so 2 runs Q = 2, 3 runs
# Q = 4 with one padded slot, 5 runs Q = 8 with three, 8 runs Q = 8 full -- each on the dense and the gene-major kernel, with
# one shared mask ('none', 'equal') and with one per key ('differ')


@pytest.mark.parametrize('masks', ['none', 'equal', 'differ'])
@pytest.mark.parametrize('q', PARITY_Q)
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_dense_against_restatement(eng, dtype, q, masks):
    X = dense_expression(N_ODD, 70, seed=q, dtype=dtype)
    V = keys_for(N_ODD, q, seed=q, masks=masks)
    _check('dense %s q=%d masks=%s' % (np.dtype(dtype).name, q, masks), _run(eng, X, V), restated_gene_corr(X, V))


@pytest.mark.parametrize('masks', ['none', 'equal', 'differ'])
@pytest.mark.parametrize('q', PARITY_Q)
@pytest.mark.parametrize('fmt,index_dtype,dtype', [('csr', np.int32, np.float32), ('csr', np.int64, np.float64),
                                                   ('csc', np.int32, np.float64), ('csc', np.int64, np.float32)])
def test_sparse_against_restatement(eng, fmt, index_dtype, dtype, q, masks):
    X = sparse_expression(N_ODD, 70, seed=q, dtype=dtype, fmt=fmt, index_dtype=index_dtype)
    assert X.indices.dtype == index_dtype and X.getnnz(axis=0)[0] == N_ODD and X.getnnz(axis=0)[1] == 3   # the skew case
    V = keys_for(N_ODD, q, seed=q, masks=masks)
    got = _run(eng, X, V)
    assert eng.expression_shape()['format'] == 'gene-major'
    _check('%s %s %s q=%d masks=%s' % (fmt, np.dtype(index_dtype).name, np.dtype(dtype).name, q, masks), got,
           restated_gene_corr(X, V))


def test_wide_dense_and_many_slabs(eng):
    """More genes than one gene block, cells over many slabs."""
    X = dense_expression(40013, 300, seed=4, dtype=np.float32)
    V = keys_for(40013, 8, seed=4, masks='equal')
    _check('dense f32 40013 x 300 q=8', _run(eng, X, V), restated_gene_corr(X, V))


# ------------------------------------------------------------------ 3. exactness
def test_constants_give_nan_exactly(eng):
    n = N_ODD
    X = dense_expression(n, 20, seed=9)
    X[:, 3] = 0.0
    X[:, 4] = 2.5                 # raw moments alone would give garbage here, not NaN
    X[:, 5] = 1e-3
    V = keys_for(n, 4, seed=9, masks='differ')
    V[2] = 0.75                   # a constant key
    X[np.isfinite(V[1]), 6] = 4.0     # constant over key 1's cells only
    X[~np.isfinite(V[1]), 6] = 5.0
    want = restated_gene_corr(X, V)
    assert np.isnan(want[:, [3, 4, 5]]).all() and np.isnan(want[2]).all() and np.isnan(want[1, 6]) and np.isfinite(want[0, 6])
    _check('constants dense', _run(eng, X, V), want)
    for fmt in ('csr', 'csc'):
        M = sp.csr_matrix(X).asformat(fmt)
        _check('constants %s' % fmt, _run(eng, M, V), want)
    few = np.full((1, n), np.nan)
    few[0, 17] = 1.0
    assert np.isnan(_run(eng, X, few)).all()


def test_single_nonzero_closed_form(eng):
    n = 5000
    v = np.random.RandomState(3).randn(n)
    vc = v - v.mean()
    want = vc[1234] / np.sqrt((vc * vc).sum() * (1 - 1 / n))
    M = sp.csr_matrix(([3.0, 1.0, 2.0], ([1234, 0, 1], [0, 1, 1])), shape=(n, 2))
    for X in (M, M.tocsc(), M.toarray()):
        got = _run(eng, X, v[None, :])
        assert abs(got[0, 0] - want) <= F64_TOL


def test_duplicates_and_explicit_zeros_behave_as_toarray(eng):
    rs = np.random.RandomState(12)
    n, g, k = 2000, 30, 9000
    rows, cols = rs.randint(0, n, k), rs.randint(0, g, k)
    vals = 1.0 + rs.poisson(2.0, k).astype(np.float64)
    vals[::7] = 0.0                                          # explicit zeros
    rows, cols, vals = np.r_[rows, rows[:500]], np.r_[cols, cols[:500]], np.r_[vals, vals[:500]]     # duplicates
    coo = sp.coo_matrix((vals, (rows, cols)), shape=(n, g))
    V = keys_for(n, 3, seed=12, masks='differ')
    for fmt in ('csr', 'csc'):
        order = np.lexsort((cols, rows)) if fmt == 'csr' else np.lexsort((rows, cols))
        major = (rows if fmt == 'csr' else cols)[order]
        indptr = np.r_[0, np.cumsum(np.bincount(major, minlength=n if fmt == 'csr' else g))]
        cls = sp.csr_matrix if fmt == 'csr' else sp.csc_matrix
        M = cls((vals[order], (cols if fmt == 'csr' else rows)[order].astype(np.int32), indptr.astype(np.int32)), shape=(n, g))
        assert not M.has_canonical_format and (M.data == 0).any()
        dense = np.ascontiguousarray(M.toarray())
        np.testing.assert_array_equal(dense, coo.toarray())
        nnz_before = M.nnz
        got = _run(eng, M, V)
        assert M.nnz == nnz_before                           # the caller's matrix stays as it is
        _check('duplicates + explicit zeros %s' % fmt, got, _run(eng, dense, V))
        _check('duplicates + explicit zeros %s vs restatement' % fmt, got, restated_gene_corr(dense, V))


@pytest.mark.parametrize('masks', ['none', 'differ'])
def test_csr_and_csc_uploads_give_the_same_bits(eng, masks):
    X = sparse_expression(N_ODD, 70, seed=21, dtype=np.float32, fmt='csr')
    V = keys_for(N_ODD, 3, seed=21, masks=masks)
    a = _run(eng, X, V)
    b = _run(eng, X.tocsc(), V)
    X64 = X.copy()
    X64.indices, X64.indptr = X64.indices.astype(np.int64), X64.indptr.astype(np.int64)
    c = _run(eng, X64, V)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)


# ------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize('kind', ['dense', 'csr'])
def test_reproducible_across_calls_and_uploads(eng, kind, monkeypatch):
    X = dense_expression(20011, 130, seed=2, dtype=np.float32) if kind == 'dense' else \
        sparse_expression(20011, 130, seed=2, dtype=np.float32, skew=True)
    V = keys_for(20011, 5, seed=2, masks='differ')
    a = _run(eng, X, V)
    b = eng.gene_corr(V)
    eng.drop_expression()
    assert eng.expression_shape()['format'] == 'none'
    c = _run(eng, X, V)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)
    from cna_amd.engine import Engine
    monkeypatch.setenv('CNA_REORDER', '0')
    e = Engine(device=0)
    try:
        np.testing.assert_array_equal(a, _run(e, X, V))
    finally:
        e.close()


# ------------------------------------------------------------------ 5. independence from the rest of the library
def _walk(eng, data, n_samples, nsteps=3):
    from cna_amd.tools._nam import sample_codes
    eng.ensure_graph(data.obsp['connectivities'])
    eng.colsums(1)
    codes, labels = sample_codes(data.obs['id'])
    eng.set_samples(codes, n_samples, np.bincount(codes, minlength=n_samples).astype(float))
    eng.nam_steps(nsteps)


def test_between_launch_and_fetch_of_a_local_null(eng):
    """gene_corr between cna_null_local_launch and cna_null_local_fetch: the pending pass returns what it returns without the
    call in between, bit for bit, and the correlations are right."""
    from cna_amd import synth
    N, P = 50, 640
    data, meta = synth.make_dataset(20000, N, k=15, seed=21)
    rs = np.random.RandomState(4)
    y = rs.randn(N)
    y = (y - y.mean()) / y.std()
    Y = np.column_stack([y, rs.randn(N, P)])
    X = dense_expression(20000, 64, seed=6, dtype=np.float32)
    V = keys_for(20000, 2, seed=6, masks='equal')
    want = restated_gene_corr(X, V)
    out = []
    for insert in (False, True):
        eng.null_local_discard()
        eng.drop_graph()
        _walk(eng, data, N)
        nz, maxabs = eng.select_standardized(None, None, y=y)
        maxcorr = max(maxabs, 0.001)
        thr = np.arange(maxcorr / 4, maxcorr, maxcorr / 400)
        edges = thr ** 2 - 1e-8 - 1e-5 * thr ** 2
        eng.condition(np.eye(N), Y)
        eng.null_local_launch(1, P, edges, thr)
        r = _run(eng, X, V) if insert else None
        fetched = eng.null_local_fetch()
        out.append([np.asarray(f).copy() for f in fetched])
        if insert:
            _check('between launch and fetch', r, want)
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


def test_association_is_untouched_by_gene_corr_calls(eng):
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd.engine import Engine
    data, meta = synth.make_dataset(3000, 24, k=15, seed=2)
    kw = dict(nsteps=3, Nnull=200, seed=5)
    X = sparse_expression(3000, 40, seed=8)
    V = keys_for(3000, 3, seed=8)
    e = Engine(device=0)
    try:
        _check('fresh engine, no graph', _run(e, X, V), restated_gene_corr(X, V))     # an engine that never saw a graph
        res = cna.tl.association(data, meta['y'], 'id', engine=e, return_full=True, **kw)
        want = (res.p, int(res.k), data.obs['coef'].values.copy(), data.obs['coef_fdr'].values.copy())
    finally:
        e.close()
    eng.ensure_expression(X)
    res = cna.tl.association(data, meta['y'], 'id', engine=eng, return_full=True, **kw)
    r = eng.gene_corr(V)
    res2 = cna.tl.association(data, meta['y'], 'id', engine=eng, return_full=True, **kw)
    for got in (res, res2):
        assert (got.p, int(got.k)) == want[:2]
    np.testing.assert_array_equal(data.obs['coef'].values, want[2])
    np.testing.assert_array_equal(data.obs['coef_fdr'].values, want[3])
    _check('after an association', r, restated_gene_corr(X, V))


# ------------------------------------------------------------------ 6. residency
def test_residency_on_the_device(eng):
    eng.unpin_expression()
    eng.drop_expression()
    base = eng.device_bytes()
    X = dense_expression(50000, 100, seed=3, dtype=np.float32)
    V = keys_for(50000, 2, seed=3)
    up0 = eng.expression_shape()['uploads']
    a = _run(eng, X, V)
    assert eng.device_bytes() - base >= X.nbytes
    info = eng.expression_shape()
    assert (info['n_cells'], info['n_genes'], info['format'], info['f64'], info['uploads']) == (50000, 100, 'dense', False, up0 + 1)
    _run(eng, X, V)
    assert eng.expression_shape()['uploads'] == up0 + 1              # same object, same content
    eng.pin_expression(X)
    X[123, 45] += 1.0                                                # pinned: not looked at again
    b = _run(eng, X, V)
    assert eng.expression_shape()['uploads'] == up0 + 1
    np.testing.assert_array_equal(a, b)
    eng.unpin_expression()
    c = _run(eng, X, V)                                              # the edit is seen and goes up
    assert eng.expression_shape()['uploads'] == up0 + 2 and not np.array_equal(a[:, 45], c[:, 45])
    M = sparse_expression(3001, 40, seed=1)
    _run(eng, M, keys_for(3001, 1))                                  # another matrix replaces it
    info = eng.expression_shape()
    assert (info['n_cells'], info['format'], info['nnz'], info['uploads']) == (3001, 'gene-major', M.nnz, up0 + 3)
    assert eng.device_bytes() - base < X.nbytes
    eng.drop_expression()
    assert eng.device_bytes() == base and eng.expression_shape()['format'] == 'none'
    from cna_amd._ffi import CnaHipError
    with pytest.raises(CnaHipError, match='no expression matrix'):
        eng.gene_corr(V)


def test_bad_sparse_structure_is_refused_and_leaves_nothing_resident(eng):
    from cna_amd._ffi import CnaHipError
    M = sparse_expression(3001, 40, seed=1)
    bad = M.copy()
    bad.indices[5] = 40                                              # a gene that does not exist
    with pytest.raises(CnaHipError, match='outside'):
        eng._upload_expression(bad)
    assert eng.expression_shape()['format'] == 'none'


# ------------------------------------------------------------------ 7. one larger case
def test_larger_case(eng):
    """200k cells: 2 000 genes dense float32 (1.6 GB) and 20 000 genes CSR at 5 % density (200M entries, 1.6 GB), q = 4
    against the restatement.  Measured on an MI355X: 30 s for the whole case inside the GPU suite (335 s in all), nearly all
    of it the host generating the inputs and numpy / scipy restating them; errors in profiles/r07_gene_corr_parity.txt."""
    n = 200000
    t0 = time.time()
    V = keys_for(n, 4, seed=30, masks='equal')
    X = dense_expression(n, 2000, seed=30, dtype=np.float32)
    t1 = time.time()
    got = _run(eng, X, V)
    t2 = time.time()
    _check('larger dense f32 200000 x 2000 q=4', got, restated_gene_corr(X, V))
    del X
    M = big_sparse_expression(n, 20000, per_row=1000, seed=31, dtype=np.float32)
    assert M.nnz == 200000000
    t3 = time.time()
    got = _run(eng, M, V)
    t4 = time.time()
    _check('larger csr f32 200000 x 20000 5% q=4', got, restated_gene_corr(M, V))
    eng.drop_expression()
    print('larger case: dense upload + call %.2f s, csr upload + call %.2f s, all %.1f s' % (t2 - t1, t4 - t3, time.time() - t0))
