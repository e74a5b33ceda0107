"""cna.ut.expr_to_sample / cna_expr_to_bins on the device (run with -m gpu on an MI355X).

Exactness: with integer-valued X (counts 0..9) every sum is exactly representable, so sums, counts of x > 0 and cell counts
equal the numpy restatement of tests/test_expr_to_sample_host.py bit for bit, in every storage form.
Rounding: with real-valued X, per (bin, gene) |got - want| <= (m - 1) * 2**-52 * sum|x| for the sums (m = the bin's cells),
the worst case for two float64 summations of the same m terms in any order; the same over m for the means.  The largest
observed ratio to that bound goes to the file CNA_PSEUDOBULK_PARITY_OUT names, when it is set
(profiles/r08_pseudobulk_parity.txt is such a run's output)."""
import os
import re

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from test_expr_to_sample_host import restated_bins

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_seen = {}


def _constant(name):
    src = open(os.path.join(ROOT, 'cna_amd', 'csrc', 'genes.hip')).read()
    return int(re.search(r'constexpr int64_t %s = (\d+);' % name, src).group(1))


DENSE_CHUNK = _constant('PB_DENSE_CHUNK')      # cells of a bin per workgroup of the dense kernel
LIST_CHUNK = 1024                              # build_chunks: the shortest chunk of a gene's list
assert 2 * max(DENSE_CHUNK, LIST_CHUNK) + 37 <= 20000
N_LONG = 2 * max(DENSE_CHUNK, LIST_CHUNK) + 37           # more than two chunks, a multiple of nothing
CELLS = [1, 63, 64, 65, 1000, N_LONG]
GENES = [1, 63, 64, 65, 130]
BINS = [1, 2, 50, 4096]
FORMS = ['dense-f32', 'dense-f64', 'csr-i32', 'csr-i64', 'csc-i32', 'csc-i64']


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()
    if os.environ.get('CNA_PSEUDOBULK_PARITY_OUT') and _seen:
        with open(os.environ['CNA_PSEUDOBULK_PARITY_OUT'], 'w') as f:
            f.write('largest |got - want| / ((m - 1) 2^-52 sum|x|) per case of tests/test_gpu_expr_to_sample.py (bound 1)\n')
            for k in sorted(_seen):
                f.write('%-58s %.3e\n' % (k, _seen[k]))
            f.write('%-58s %.3e\n' % ('maximum', max(_seen.values())))


def counts_matrix(n, g, seed):
    """Integer-valued expression 0..9 as CSR float64, about half of it absent, some explicit zeros, gene 1 empty, gene 0
    present in every cell (its list is the longest: n entries)."""
    rs = np.random.RandomState(seed)
    D = rs.randint(0, 10, (n, g)).astype(np.float64) * (rs.rand(n, g) < 0.5)
    D[:, 0] = rs.randint(1, 10, n)
    if g >= 2:
        D[:, 1] = 0.0
    M = sp.csr_matrix(D)
    M.data[rs.rand(M.nnz) < 0.1] = 0.0          # explicit zeros stay stored
    M.sort_indices()
    return M


def as_form(M, form):
    kind, t = form.split('-')
    if kind == 'dense':
        return np.ascontiguousarray(M.toarray().astype(np.float32 if t == 'f32' else np.float64))
    X = M.asformat(kind).astype(np.float32 if t == 'i32' else np.float64)
    idt = np.int32 if t == 'i32' else np.int64
    X.indices, X.indptr = X.indices.astype(idt), X.indptr.astype(idt)
    return X


def codes_for(n, n_bins, seed, layout='mixed'):
    rs = np.random.RandomState(seed)
    if layout == 'one':
        return np.full(n, n_bins - 1, dtype=np.int32)
    c = rs.randint(0, n_bins, n).astype(np.int32)
    if n_bins >= 2:
        c[c == n_bins // 2] = 0                 # a bin without cells
    c[rs.rand(n) < 0.1] = -1                    # cells that are left out
    return c


def _bins(eng, X, codes, n_bins, what):
    eng.ensure_expression(X)
    return eng.expr_to_bins(codes, n_bins, what)


def _exact(eng, X, ref, codes, n_bins, tag):
    for what in (0, 1):
        got, cnt = _bins(eng, X, codes, n_bins, what)
        want, wcnt = restated_bins(ref, codes, n_bins, what)
        np.testing.assert_array_equal(cnt, wcnt, err_msg=tag)
        np.testing.assert_array_equal(got, want, err_msg='%s what=%d' % (tag, what))


# ------------------------------------------------------------------ 1. exactness over every shape and form
@pytest.mark.parametrize('form', FORMS)
def test_exact_on_integer_valued_input(eng, form):
    k = 0
    cases = [(n, g, BINS[(i + j) % 4]) for i, n in enumerate(CELLS) for j, g in enumerate(GENES)]
    cases += [(n, g, b) for (n, g) in ((1000, 65), (N_LONG, 130)) for b in BINS]
    for n, g, b in cases:
        k += 1
        M = counts_matrix(n, g, seed=k)
        X = as_form(M, form)
        _exact(eng, X, M, codes_for(n, b, seed=k), b, '%s %d x %d bins %d' % (form, n, g, b))
    assert (M.data == 0).any() and M.getnnz(axis=0)[1] == 0 and M.getnnz(axis=0)[0] == N_LONG > 2 * LIST_CHUNK


@pytest.mark.parametrize('form', FORMS)
def test_every_cell_in_one_bin(eng, form):
    """The most conflicts for the gene-major kernel, the longest cell list for the dense one."""
    M = counts_matrix(N_LONG, 65, seed=7)
    X = as_form(M, form)
    for b in (1, 50, 4096):
        _exact(eng, X, M, codes_for(N_LONG, b, 0, layout='one'), b, '%s one bin of %d' % (form, b))
    two = (np.arange(N_LONG) % 2).astype(np.int32)          # two bins alternating: 32 lanes of every batch per bin
    _exact(eng, X, M, two, 2, '%s two bins alternating' % form)


def test_refusals_leave_the_matrix_usable(eng):
    from cna_amd._ffi import CnaHipError
    M = counts_matrix(1000, 65, seed=3)
    for X in (as_form(M, 'csr-i32'), as_form(M, 'dense-f32')):
        good = codes_for(1000, 50, seed=3)
        want = _bins(eng, X, good, 50, 0)
        with pytest.raises(CnaHipError, match='4096'):
            eng.expr_to_bins(np.zeros(1000, np.int32), 4097, 0)
        with pytest.raises(CnaHipError, match='4096'):
            eng.expr_to_bins(np.zeros(1000, np.int32), 0, 0)
        with pytest.raises(CnaHipError, match='what'):
            eng.expr_to_bins(good, 50, 2)
        for wrong in (50, -2, 2 ** 31 - 1):
            bad = good.copy()
            bad[777] = wrong                                     # a code equal to n_bins, below -1, far outside
            with pytest.raises(CnaHipError, match='outside'):
                eng.expr_to_bins(bad, 50, 0)
        with pytest.raises(ValueError):
            eng.expr_to_bins(good[:-1], 50, 0)
        got = eng.expr_to_bins(good, 50, 0)                      # a following valid call still works
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[0], restated_bins(M, good, 50, 0)[0])
        full = eng.expr_to_bins(np.arange(1000, dtype=np.int32) % 4096, 4096, 0)       # the largest bin count passes
        assert full[1].sum() == 1000


def test_second_gene_tile_of_the_gene_major_kernel(eng):
    """4096 bins leave pb_sparse 8192 chunks per gene tile; 418 genes present in each of 20 517 cells are 8778 chunks of 1024
    entries: two tiles, an empty gene closing the first (tests/test_expr_tiles_host.py builds the input and asserts that).
    Integer-valued, so sums, counts of x > 0 and cell counts equal the restatement bit for bit."""
    from test_expr_tiles_host import bins_tile_case, assert_bins_tile_case, BINS_BINS
    M, codes = bins_tile_case()
    assert_bins_tile_case(M)
    D = M.toarray()
    want, wcnt = restated_bins(D, codes, BINS_BINS, 0)
    # restated_bins(.., what=1) compares the whole matrix with 0 once per bin; the same figure from the comparison made once
    want_pos = restated_bins((D > 0).astype(np.float64), codes, BINS_BINS, 0)[0]
    assert (wcnt == 0).any() and (want_pos != want).any()
    for form in ('csr-i32', 'csc-i64'):
        X = as_form(M, form)
        assert X.nnz == M.nnz                                        # the stored zeros stay stored
        for what, ref in ((0, want), (1, want_pos)):
            got, cnt = _bins(eng, X, codes, BINS_BINS, what)
            np.testing.assert_array_equal(cnt, wcnt, err_msg=form)
            np.testing.assert_array_equal(got, ref, err_msg='%s what=%d' % (form, what))
    eng.drop_expression()


# ------------------------------------------------------------------ 2. rounding
def _real(n, g, seed, dtype):
    rs = np.random.RandomState(seed)
    return np.ascontiguousarray((rs.randn(n, g) * (1.0 + 3.0 * rs.rand(g)) + rs.randn(g)).astype(dtype))


@pytest.mark.parametrize('form', ['dense-f32', 'dense-f64', 'csr-i64', 'csc-i32'])
def test_rounding_bound_on_real_valued_input(eng, form):
    worst = 0.0
    for n, g, b in ((N_LONG, 130, 1), (N_LONG, 65, 2), (N_LONG, 64, 50), (1000, 63, 4096), (19997, 130, 7)):
        D = _real(n, g, seed=n + b, dtype=np.float32 if form.endswith('32') else np.float64)
        if not form.startswith('dense'):
            D[np.random.RandomState(b).rand(n, g) < 0.6] = 0.0
            D[:, 0] = np.abs(D[:, 0]) + 1.0
        M = sp.csr_matrix(D)
        X = D if form.startswith('dense') else as_form(M, form).astype(D.dtype)
        codes = codes_for(n, b, seed=b)
        got, cnt = _bins(eng, X, codes, b, 0)
        want, wcnt = restated_bins(D, codes, b, 0)
        np.testing.assert_array_equal(cnt, wcnt)
        absum = restated_bins(np.abs(D), codes, b, 0)[0]
        bound = np.maximum(cnt - 1, 0)[:, None] * 2.0 ** -52 * absum
        err = np.abs(got - want)
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
        name = 'sum %s %d x %d bins %d' % (form, n, g, b)
        _seen[name] = ratio
        print('%s: largest |got - want| / bound = %.3e' % (name, ratio))
        assert (err <= bound).all(), name
        m = np.maximum(cnt, 1)[:, None].astype(np.float64)
        assert (np.abs(got / m - want / m) <= bound / m).all(), 'mean ' + name
        worst = max(worst, ratio)
    assert worst <= 1.0


# ------------------------------------------------------------------ 3. determinism
def test_same_bits_again_and_across_forms(eng):
    n, g, b = N_LONG, 130, 50
    D = _real(n, g, seed=5, dtype=np.float32)
    D[np.random.RandomState(5).rand(n, g) < 0.5] = 0.0
    D[:, 0] = 1.0 + np.abs(D[:, 0])
    M = sp.csr_matrix(D)
    codes = codes_for(n, b, seed=5)
    csr = as_form(M, 'csr-i32').astype(np.float32)
    a = _bins(eng, csr, codes, b, 0)[0]
    np.testing.assert_array_equal(a, eng.expr_to_bins(codes, b, 0)[0])             # a second call
    eng.drop_expression()
    np.testing.assert_array_equal(a, _bins(eng, csr, codes, b, 0)[0])              # a second upload
    for form in ('csc-i32', 'csc-i64', 'csr-i64'):
        np.testing.assert_array_equal(a, _bins(eng, as_form(M, form).astype(np.float32), codes, b, 0)[0], err_msg=form)
    d = _bins(eng, D, codes, b, 0)[0]
    np.testing.assert_array_equal(d, eng.expr_to_bins(codes, b, 0)[0])
    Mi = counts_matrix(n, g, seed=6)                                               # integer-valued: CSR == dense, bit for bit
    np.testing.assert_array_equal(_bins(eng, as_form(Mi, 'csr-i32'), codes, b, 0)[0],
                                  _bins(eng, as_form(Mi, 'dense-f32'), codes, b, 0)[0])


def test_nan_and_inf_touch_only_their_own_bin_and_gene(eng):
    n, g, b = 1000, 65, 50
    M = counts_matrix(n, g, seed=8)
    codes = codes_for(n, b, seed=8)
    codes[[10, 20, 30]] = [3, 4, -1]
    D = M.toarray()
    D[10, 5], D[20, 64], D[30, 7] = np.nan, np.inf, np.nan        # the third sits in a cell that is left out
    for X in (np.ascontiguousarray(D.astype(np.float32)), sp.csr_matrix(D), sp.csc_matrix(D)):
        got = _bins(eng, X, codes, b, 0)[0]
        want = restated_bins(D, codes, b, 0)[0]
        np.testing.assert_array_equal(got, want)
        assert np.isnan(got).sum() == 1 and np.isnan(got[3, 5]) and np.isinf(got).sum() == 1 and got[4, 64] == np.inf
        np.testing.assert_array_equal(_bins(eng, X, codes, b, 1)[0], restated_bins(D, codes, b, 1)[0])


# ------------------------------------------------------------------ 4. independence from the rest of the library
def test_on_a_context_that_never_saw_a_graph(eng):
    from cna_amd.engine import Engine
    M = counts_matrix(1000, 63, seed=9)
    codes = codes_for(1000, 50, seed=9)
    e = Engine(device=0)
    try:
        for form in ('dense-f64', 'csr-i32'):
            _exact(e, as_form(M, form), M, codes, 50, 'fresh engine ' + form)
    finally:
        e.close()


def test_between_launch_and_fetch_of_a_local_null(eng):
    """expr_to_bins between cna_null_local_launch and cna_null_local_fetch: the pending pass returns what it returns
    without the call in between, bit for bit, and the sums are right."""
    from cna_amd import synth
    from test_gpu_gene_corr import _walk
    N, P = 50, 640
    data, meta = synth.make_dataset(20000, N, k=15, seed=21)
    rs = np.random.RandomState(4)
    y = rs.randn(N)
    y = (y - y.mean()) / y.std()
    Y = np.column_stack([y, rs.randn(N, P)])
    M = counts_matrix(20000, 64, seed=6)
    X = as_form(M, 'dense-f32')
    codes = codes_for(20000, N, seed=6)
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
        if insert:
            _exact(eng, X, M, codes, N, 'between launch and fetch')
        fetched = eng.null_local_fetch()
        out.append([np.asarray(f).copy() for f in fetched])
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 5. residency
def test_residency_uploads_and_drop(eng):
    import cna_amd as cna
    from cna_amd._ffi import CnaHipError
    from cna_amd.synth import CellData
    eng.unpin_expression()
    eng.drop_expression()
    base = eng.device_bytes()
    n = 5000
    M = counts_matrix(n, 65, seed=11)
    X = as_form(M, 'dense-f32')
    obs = pd.DataFrame({'id': np.arange(n) % 13, 'coef': np.random.RandomState(0).randn(n)})
    d = CellData(obs, None, X=X)
    up0 = eng.expression_shape()['uploads']
    a = cna.ut.expr_to_sample(d, 'id', engine=eng)
    assert eng.expression_shape()['uploads'] == up0 + 1 and eng.device_bytes() - base >= X.nbytes
    b = cna.ut.expr_to_sample(d, 'id', aggregate='sum', engine=eng)               # resident: not uploaded again
    cna.tl.gene_corr(d, 'coef', engine=eng)                                        # nor by the other user of the matrix
    assert eng.expression_shape()['uploads'] == up0 + 1
    eng.pin_expression(X)
    cna.ut.expr_to_sample(d, 'id', aggregate='frac', engine=eng)                   # pinned: not looked at again
    assert eng.expression_shape()['uploads'] == up0 + 1
    eng.unpin_expression()
    np.testing.assert_array_equal(b.values, restated_bins(M, obs['id'].values, 13, 0)[0])
    np.testing.assert_array_equal(a.values, b.values / restated_bins(M, obs['id'].values, 13, 0)[1][:, None])
    eng.drop_expression()
    assert eng.device_bytes() == base and eng.expression_shape()['format'] == 'none'
    with pytest.raises(CnaHipError, match='no expression matrix'):
        eng.expr_to_bins(np.zeros(n, np.int32), 13, 0)


# ------------------------------------------------------------------ 6. end to end
def test_end_to_end_on_the_demo_like_dataset(eng):
    import cna_amd as cna
    from cna_amd import synth
    d, samplem = synth.make_demo_like(keep_expression=True)
    d.obs['id'] = np.random.RandomState(1).permutation(d.obs['id'].values)         # first appearance != sorted
    out, counts = cna.ut.expr_to_sample(d, 'id', return_counts=True, engine=eng)
    first = d.obs['id'].unique()
    X64 = d.X.astype(np.float64)
    want = pd.DataFrame(X64).groupby(d.obs['id'].values).mean().reindex(first)
    assert list(out.index) == list(first) and out.columns.equals(d.var_names)
    d.obs['depth'] = X64.sum(axis=1)
    assert out.index.equals(cna.ut.obs_to_sample(d, 'depth', 'id').index)
    absum = pd.DataFrame(np.abs(X64)).groupby(d.obs['id'].values).sum().reindex(first).values
    m = counts.values[:, None]
    bound = (m - 1) * 2.0 ** -52 * absum / m
    ratio = float((np.abs(out.values - want.values) / bound).max())
    _seen['mean demo-like 10000 x 50 bins 50'] = ratio
    assert (np.abs(out.values - want.values) <= bound).all()
    # per sample and cluster: the population read off the two halves of the genes, as a clustering would find it
    G = d.X.shape[1]
    lo, hi = d.X[:, :G // 2].mean(axis=1), d.X[:, G // 2:].mean(axis=1)
    d.obs['leiden'] = np.where(hi > lo, 'B', np.where(lo > 1.2, 'C', 'A'))
    both, cnt2 = cna.ut.expr_to_sample(d, 'id', groupby='leiden', return_counts=True, engine=eng)
    sm = cna.ut.obs_to_sample(d, 'depth', 'id')
    assert both.index.levels[0].dtype == sm.index.dtype
    assert list(both.index.get_level_values(0)[::3]) == list(sm.index) and len(both) == 3 * len(sm)
    assert list(both.index.get_level_values(1)[:3]) == list(d.obs['leiden'].unique())
    want2 = pd.DataFrame(X64).groupby([d.obs['id'].values, d.obs['leiden'].values]).mean().reindex(both.index)
    absum2 = pd.DataFrame(np.abs(X64)).groupby([d.obs['id'].values, d.obs['leiden'].values]).sum().reindex(both.index).values
    m2 = np.maximum(cnt2.values, 1)[:, None]
    bound2 = (m2 - 1) * 2.0 ** -52 * absum2 / m2
    ok = cnt2.values > 0
    assert ok.sum() >= 2 * len(sm)
    assert (np.abs(both.values[ok] - want2.values[ok]) <= bound2[ok]).all()
    assert np.isnan(both.values[~ok]).all()
    assert cnt2.groupby(level=0, sort=False).sum().tolist() == counts.tolist()
