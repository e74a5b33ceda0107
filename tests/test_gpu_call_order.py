"""State the library keeps between two calls (run with -m gpu on an MI355X).

A local-null pass lives from cna_null_local_launch to cna_null_local_fetch.  Should its integer kernel give up (a recheck
queue overflow, forced here through CNA_I8_QCAP), the fetch reruns it on the f64 kernel -- on the X, the conditioned
phenotypes and the exact cuts the launch saw.  The contract (csrc/common.h: NO_NULL_PENDING): an entry point that would
rewrite X or carve the scratch those cuts live in refuses with CNA_ESTATE while a pass is pending, changes nothing, and
the fetch returns the f64 kernel's integers.  Also here: the FDR column the helper thread copies while a given-up pass is
collected, and the Gram matrix queued with a selection that turns out to have cells of zero variance.

State derived from X, the walk or the cells holds only as long as what it was derived from (csrc/c_api.hip: void_x,
void_walk, void_cells; every producer of X goes through x_begin / x_commit).  The kept projection (cna_project_keep) and
the Gram matrix refuse to be fetched once X has been rewritten, the walk restarted or the graph replaced; the
coefficients of an analysis do not outlive its walk.  A walk with a selection hint while a pass is pending leaves X to
that pass: the hint does not arm, the step writes the NAM, and the next selection is the separate pass of a walk without
the hint, bit for bit (the by-product agrees with that pass to rounding, not bit for bit)."""
import threading

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N, P = 50, 640


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    return get_engine()


def _walk(eng, data, n_samples, nsteps=3):
    """The NAM of `data` (cells x samples) resident on the engine."""
    from cna_amd.tools._nam import sample_codes
    eng.ensure_graph(data.obsp['connectivities'])
    eng.colsums(1)
    codes, labels = sample_codes(data.obs['id'])
    assert len(labels) == n_samples
    eng.set_samples(codes, n_samples, np.bincount(codes, minlength=n_samples).astype(float))
    eng.nam_steps(nsteps)
    return codes


@pytest.fixture(scope='module')
def resident():
    """20 000 cells x 50 samples: X = the standardised NAM (select_standardized with y), thresholds and edges of the
    reference's formula (_association.py:268-271), the phenotype and 640 permutations to condition."""
    from cna_amd import synth
    data, meta = synth.make_dataset(20000, N, k=15, seed=21)
    rs = np.random.RandomState(4)
    y = rs.randn(N)
    y = (y - y.mean()) / y.std()
    Y = np.column_stack([y, rs.randn(N, P)])
    thr = edges = None

    def setup(eng):
        nonlocal thr, edges
        eng.null_local_discard()
        codes = _walk(eng, data, N)
        nz, maxabs = eng.select_standardized(None, None, y=y)
        assert nz == 0
        if thr is None:
            maxcorr = max(maxabs, 0.001)
            thr = np.arange(maxcorr / 4, maxcorr, maxcorr / 400)
            z2 = thr ** 2
            edges = z2 - 1e-8 - 1e-5 * z2
        eng.condition(np.eye(N), Y)
        return codes, thr, edges
    return dict(setup=setup, Y=Y, y=y, data=data)


@pytest.fixture(scope='module')
def reference(eng, resident):
    """What every fetch must return: the f64 kernel's per-permutation tails on the resident columns 1 .. P, summed; the
    observed counts; and a plain numpy recount of the same quantity that agrees up to the outputs within 1e-9 relative
    of a cut."""
    from cna_amd import _ffi
    codes, thr, edges = resident['setup'](eng)
    tails = eng.null_local_resident(1, P, edges)              # want_tails: the f64 kernel
    sums = tails.sum(axis=0)
    ranks, numdet = eng.obs_counts(edges, thr)
    X = eng.fetch_matrix(_ffi.MAT_X)
    Y = resident['Y']
    Zc = Y / Y.std(axis=0, ddof=1)
    z2 = (X.dot(Zc[:, 1:]) / N) ** 2
    for t, e in enumerate(edges):
        near = np.abs(z2 - e) <= 1e-9 * e
        want = int(np.count_nonzero(z2 >= e))
        assert abs(int(sums[t]) - want) <= int(np.count_nonzero(near)), t
    assert (np.diff(sums) <= 0).all() and sums[0] > sums[-1]
    return dict(sums=sums, ranks=ranks, numdet=numdet, codes=codes)


@pytest.fixture(scope='module')
def fresh_association():
    """A small association on an engine nobody else has used: what the shared engine must return after each case."""
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd.engine import Engine
    data, meta = synth.make_dataset(3000, 24, k=15, seed=2)
    kw = dict(nsteps=3, Nnull=200, seed=5)
    e = Engine()
    try:
        res = cna.tl.association(data, meta['y'], 'id', engine=e, return_full=True, **kw)
        want = (res.p, int(res.k), res.fdrs.values.copy(), data.obs['coef'].values.copy(), data.obs['coef_fdr'].values.copy())
    finally:
        e.close()
    return data, meta, kw, want


def _insert(eng, what, codes, thr, edges):
    """The call made between launch and fetch."""
    from cna_amd import _ffi
    rs = np.random.RandomState(9)
    T = len(thr)
    if what == 'ncorrs':
        eng.ncorrs(rs.randn(N))
    elif what == 'obs_counts':
        t2 = thr * 0.7
        eng.obs_counts(t2 ** 2 - 1e-8 - 1e-5 * t2 ** 2, t2)
    elif what == 'percell':
        eng.percell(thr, np.linspace(1.0, 0.01, T))
    elif what == 'zero_variance':
        eng.zero_variance(None)
    elif what == 'batch_kurtosis':
        eng.batch_kurtosis(_ffi.MAT_X, np.arange(N, dtype=np.int32) % 3, 3)
    elif what == 'resid_lowrank':
        Cm = np.ones((N, 1)) / np.sqrt(N)
        eng.resid_lowrank(Cm, Cm.T.copy(), center=True, standardize=True)
    elif what == 'select':
        eng.select(None, None)
    else:
        assert what == 'nothing'


INSERTED = ['nothing', 'ncorrs', 'obs_counts', 'percell', 'zero_variance', 'batch_kurtosis', 'resid_lowrank', 'select']


@pytest.mark.parametrize('split', ['one_shot', 'prepared'])
@pytest.mark.parametrize('give_up', [False, True])
@pytest.mark.parametrize('what', INSERTED)
def test_calls_between_launch_and_fetch(eng, resident, reference, fresh_association, monkeypatch, what, give_up, split):
    """The inserted call fails with CNA_ESTATE and changes nothing; the fetch returns the f64 kernel's integers, whether
    the integer pass stood or gave up (then the rerun really ran: fallback); the next analysis on the engine is a fresh
    engine's."""
    import warnings
    import cna_amd as cna
    from cna_amd import _ffi
    codes, thr, edges = resident['setup'](eng)
    if give_up:
        monkeypatch.setenv('CNA_I8_QCAP', '8')
    else:
        monkeypatch.delenv('CNA_I8_QCAP', raising=False)
    if split == 'prepared':
        eng.null_local_prepare(P, edges, thr)
        eng.null_local_launch(1, P, None)
    else:
        eng.null_local_launch(1, P, edges, thr)
    if what == 'nothing':
        _insert(eng, what, codes, thr, edges)
    else:
        with pytest.raises(_ffi.CnaHipError, match=r'status -4\).*still pending'):
            _insert(eng, what, codes, thr, edges)
    sums, ranks, numdet = eng.null_local_fetch()
    monkeypatch.delenv('CNA_I8_QCAP', raising=False)
    used, rechecked, fallback = eng.null_local_i8_stats()
    assert used and fallback == give_up
    np.testing.assert_array_equal(sums, reference['sums'])
    np.testing.assert_array_equal(ranks, reference['ranks'])
    np.testing.assert_array_equal(numdet, reference['numdet'])
    # nothing pending any more: the refused call now goes through
    _insert(eng, what, codes, thr, edges)
    data, meta, kw, want = fresh_association
    for key in ('coef', 'coef_fdr'):
        if key in data.obs:
            del data.obs[key]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = cna.tl.association(data, meta['y'], 'id', engine=eng, return_full=True, **kw)
    got = (res.p, int(res.k), res.fdrs.values, data.obs['coef'].values, data.obs['coef_fdr'].values)
    assert got[0] == want[0] and got[1] == want[1]
    for a, b in zip(got[2:], want[2:]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('give_up', [False, True])
def test_helper_thread_fdr_copy_while_the_main_thread_fetches(eng, resident, reference, monkeypatch, give_up):
    """percell_fdr_copy_early on a second thread while this one collects a pass (given up or not): it copies nothing
    (done == 0), or exactly the column percell() returns after the fetch -- never the void table of a given-up pass."""
    codes, thr, edges = resident['setup'](eng)
    if give_up:
        monkeypatch.setenv('CNA_I8_QCAP', '8')
    else:
        monkeypatch.delenv('CNA_I8_QCAP', raising=False)
    assert eng.percell_coef_launch()
    eng.null_local_prepare(P, edges, thr)
    eng.null_local_launch(1, P, None)
    dst = np.full(eng.n, -1.0)
    done = []
    th = threading.Thread(target=lambda: done.append(eng.percell_fdr_copy_early(dst)))
    th.start()
    try:
        sums, ranks, numdet = eng.null_local_fetch()
    finally:
        th.join()
    monkeypatch.delenv('CNA_I8_QCAP', raising=False)
    assert eng.null_local_i8_stats()[2] == give_up
    np.testing.assert_array_equal(sums, reference['sums'])
    with np.errstate(all='ignore'):
        runmin = np.fmin.accumulate(sums / ranks / P)
    coef, fdr = eng.percell(thr, runmin)
    fdr = fdr.copy()
    assert np.isfinite(fdr).all()
    if done[0]:
        np.testing.assert_array_equal(dst, fdr)
    else:
        assert (dst == -1.0).all()
    if give_up:
        assert not eng.percell_fdr_copied_early()


def test_pass_with_thresholds_and_tails(eng, resident):
    """cna_null_local_launch with thresholds AND want_tails (no Engine method asks for both): the observed counts then
    sit behind the P x T tails in the pinned result block.  One fetch with all four outputs returns the f64 kernel's
    tails, their column sums and the observed counts of cna_obs_counts, integer for integer."""
    from cna_amd._ffi import check, ptr
    codes, thr, edges = resident['setup'](eng)
    T = len(edges)
    want_tails = eng.null_local_resident(1, P, edges)
    want_ranks, want_numdet = eng.obs_counts(edges, thr)
    check(eng.lib.cna_null_local_launch(eng.h, 1, P, ptr(edges), T, 1, ptr(thr)), 'cna_null_local_launch')
    tails = np.full((P, T), -1, dtype=np.int64)
    sums, ranks, numdet = (np.full(T, -1, dtype=np.int64) for _ in range(3))
    check(eng.lib.cna_null_local_fetch(eng.h, ptr(tails), ptr(sums), ptr(ranks), ptr(numdet)), 'cna_null_local_fetch')
    np.testing.assert_array_equal(tails, want_tails)
    np.testing.assert_array_equal(sums, want_tails.sum(axis=0))
    np.testing.assert_array_equal(ranks, want_ranks)
    np.testing.assert_array_equal(numdet, want_numdet)


def _with_zero_variance_cells(n_samples, seed):
    """A dataset of n_samples samples plus a far-away blob of 25 cells that all belong to one more sample: over the first
    n_samples samples (colmap) the blob's NAM rows are zero -- cells of zero variance."""
    from cna_amd import synth
    data, meta = synth.make_dataset(4000, n_samples, k=15, seed=seed)
    A = sp.csr_matrix(data.obsp['connectivities'])
    n, n_iso = A.shape[0], 25
    rs = np.random.RandomState(seed)
    B = sp.random(n_iso, n_iso, density=0.6, random_state=rs, format='csr', dtype=np.float64)
    B = B + B.T
    B.setdiag(0)
    B.eliminate_zeros()
    B.data = np.clip(B.data, 0.05, 1.0)
    A2 = sp.block_diag([A, B.astype(A.dtype)], format='csr')
    A2.sort_indices()
    obs = pd.DataFrame({'id': np.concatenate([data.obs['id'].values, np.repeat(n_samples, n_iso)])},
                       index=pd.Index(['cell_%d' % i for i in range(n + n_iso)], name='cell'))
    d2 = type('D', (), {'obs': obs, 'obsp': {'connectivities': A2}, 'uns': {}})()
    return d2, n_iso


@pytest.mark.parametrize('n_samples', [50, 130, 200])
def test_gram_queued_with_zero_variance_cells_is_dropped(eng, n_samples):
    """select_standardized with y queues the Gram kernels before it knows the zero-variance count: with such cells the
    matrix is void and cna_gram_fetch refuses (CNA_ESTATE) instead of returning it.  The general path's re-selection
    without those cells then gets X^T X of its own X."""
    from cna_amd import _ffi
    eng.null_local_discard()
    d2, n_iso = _with_zero_variance_cells(n_samples, seed=n_samples)
    _walk(eng, d2, n_samples + 1)
    colmap = np.arange(n_samples, dtype=np.int32)
    y = np.random.RandomState(n_samples).randn(n_samples)
    y = (y - y.mean()) / y.std()
    nz, _ = eng.select_standardized(None, colmap, y=y, fuse_null=100)
    assert nz == n_iso
    assert not eng._fused['gram']
    G = np.full((n_samples, n_samples), -1.0)
    assert eng.lib.cna_gram_fetch(eng.h, G.ctypes.data) == -4     # CNA_ESTATE: no N x N array
    assert (G == -1.0).all()
    zero_var, nz2 = eng.zero_variance(colmap)
    assert nz2 == n_iso and zero_var.sum() == n_iso
    assert eng.select_standardized(~zero_var, colmap) == 0
    eng.gram_launch()
    G = eng.gram_fetch()
    X = eng.fetch_matrix(_ffi.MAT_X)
    assert X.shape == (d2.obs.shape[0] - n_iso, n_samples)
    want = X.T @ X
    np.testing.assert_array_equal(G, G.T)
    np.testing.assert_allclose(G, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


NS = 30


@pytest.fixture(scope='module')
def small():
    """Two small datasets of NS samples (the second one: another graph) and a standardised phenotype."""
    from cna_amd import synth
    data, _ = synth.make_dataset(4000, NS, k=15, seed=7)
    other, _ = synth.make_dataset(3000, NS, k=15, seed=8)
    y = np.random.RandomState(7).randn(NS)
    return data, other, (y - y.mean()) / y.std()


def _x_standardized(eng, data):
    """The shared engine with the 3-step NAM of `data` resident and X = its standardised selection; returns the codes."""
    eng.null_local_discard()
    codes = _walk(eng, data, NS)
    assert eng.select_standardized(None, None) == 0
    return codes


def _rewrite(eng, what, small, codes):
    """One call that replaces X (or the walk, or the graph X was derived from)."""
    from cna_amd import _ffi
    data, other, y = small
    rs = np.random.RandomState(3)
    nx, Nx = eng.matrix_shape(_ffi.MAT_X)
    Cm = np.ones((Nx, 1)) / np.sqrt(Nx)
    batches = np.arange(Nx, dtype=np.int32) % 3
    if what == 'select':
        eng.select(None, None)
    elif what == 'select_checked':
        assert eng.select_checked(None, None) == 0
    elif what == 'select_standardized':
        assert eng.select_standardized(None, None) == 0
    elif what == 'select_resid_bk':
        assert eng.select_resid_bk(Cm, Cm.T.copy(), y, batches, 3) is not None
    elif what == 'upload_x':
        eng.upload_x(rs.randn(nx, Nx))
    elif what == 'resid_apply':
        eng.resid_apply(np.eye(Nx) - Cm @ Cm.T, True)
    elif what == 'resid_lowrank':
        eng.resid_lowrank(Cm, Cm.T.copy(), center=True, standardize=True)
    elif what == 'resid_lowrank_bk':
        eng.resid_lowrank_bk(Cm, Cm.T.copy(), y, batches, 3)
    elif what == 'standardize':
        eng.standardize(center=True)
    elif what == 'restart':
        assert eng.lib.cna_restart_nam(eng.h) == 0
    elif what == 'set_samples':
        eng.set_samples(codes, NS, np.bincount(codes, minlength=NS).astype(float))
    else:
        assert what == 'graph'
        eng.ensure_graph(other.obsp['connectivities'])


@pytest.mark.parametrize('what', ['select', 'upload_x', 'resid_lowrank', 'standardize', 'restart', 'graph'])
def test_kept_projection_is_void_after(eng, small, what):
    """cna_project_keep, then a new X, walk or graph: cna_fetch_rows(CNA_MAT_PROJ) refuses (CNA_ESTATE) and leaves
    `out` untouched instead of returning the rows of the old X."""
    from cna_amd import _ffi
    codes = _x_standardized(eng, small[0])
    X = eng.fetch_matrix(_ffi.MAT_X)
    W = np.random.RandomState(5).randn(NS, 3)
    eng.project_keep(W)
    np.testing.assert_allclose(eng.fetch_rows(_ffi.MAT_PROJ), X @ W, rtol=1e-12, atol=1e-12 * np.abs(X @ W).max())
    _rewrite(eng, what, small, codes)
    out = np.full((X.shape[0], 3), -1.0)
    assert eng.lib.cna_fetch_rows(eng.h, _ffi.MAT_PROJ, None, 0, None, 0, out.ctypes.data, 0) == -4
    assert (out == -1.0).all()


@pytest.mark.parametrize('what', ['select', 'select_checked', 'select_standardized', 'select_resid_bk', 'upload_x',
                                  'resid_apply', 'resid_lowrank', 'resid_lowrank_bk', 'standardize'])
def test_gram_matrix_is_void_after_x_is_rewritten(eng, small, what):
    """cna_gram_launch, then a rewrite of X: cna_gram_fetch refuses (CNA_ESTATE) instead of returning X^T X of the old
    X; a fresh cna_gram_launch gives X^T X of the current X."""
    from cna_amd import _ffi
    codes = _x_standardized(eng, small[0])
    assert eng.lib.cna_gram_launch(eng.h) == 0
    G = np.full((NS, NS), -1.0)
    assert eng.lib.cna_gram_fetch(eng.h, G.ctypes.data) == 0
    _rewrite(eng, what, small, codes)
    G = np.full((NS, NS), -1.0)
    assert eng.lib.cna_gram_fetch(eng.h, G.ctypes.data) == -4
    assert (G == -1.0).all()
    assert eng.lib.cna_gram_launch(eng.h) == 0
    assert eng.lib.cna_gram_fetch(eng.h, G.ctypes.data) == 0
    X = eng.fetch_matrix(_ffi.MAT_X)
    want = X.T @ X
    np.testing.assert_array_equal(G, G.T)
    np.testing.assert_allclose(G, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize('what', ['restart', 'set_samples'])
def test_coefficients_do_not_outlive_the_walk(eng, small, what):
    """select_standardized with y, then a new walk begins: the coefficients of the old one are not served
    (cna_percell_coef_launch raises CNA_ESTATE) and X is no longer the resident walk's (cna_x_identity = 0)."""
    from cna_amd import _ffi
    data, other, y = small
    eng.null_local_discard()
    codes = _walk(eng, data, NS)
    nz, _ = eng.select_standardized(None, None, y=y)
    assert nz == 0 and eng.x_identity_resident()
    assert eng.percell_coef_launch()
    eng.percell_coef_wait()
    _rewrite(eng, what, small, codes)
    with pytest.raises(_ffi.CnaHipError, match=r'status -4\)'):
        eng.percell_coef_launch()
    assert not eng.x_identity_resident()


def test_early_coefficient_column_does_not_outlive_its_coefficients(eng, small):
    """select_standardized with y, the early coefficient column launched and collected, then cna_ncorrs with another
    phenotype on the same X: the pinned column holds the coefficients of the old y, and cna_percell_coef_wait refuses
    (CNA_ESTATE) instead of serving it (csrc/c_api.hip: void_coef)."""
    from cna_amd import _ffi
    data, other, y = small
    eng.null_local_discard()
    _walk(eng, data, NS)
    nz, _ = eng.select_standardized(None, None, y=y)
    assert nz == 0
    assert eng.percell_coef_launch()
    eng.percell_coef_wait()
    y2 = np.random.RandomState(11).randn(NS)
    eng.ncorrs((y2 - y2.mean()) / y2.std())
    with pytest.raises(_ffi.CnaHipError, match=r'status -4\)'):
        eng.percell_coef_wait()


NW, PW = 96, 256          # more than 64 samples: the walk's last step can leave the selection by-product (t_ld > 64)


@pytest.fixture(scope='module')
def wide(eng):
    """10 000 cells x NW samples: X = the standardised 3-step NAM with y, Zc conditioned; what a pass on it must return
    (the f64 kernel's tail sums and the observed counts), and X4 = the separate selection pass over a 4-step walk."""
    from cna_amd import _ffi, synth
    data, _ = synth.make_dataset(10000, NW, k=15, seed=31)
    rs = np.random.RandomState(6)
    y = rs.randn(NW)
    y = (y - y.mean()) / y.std()
    Y = np.column_stack([y, rs.randn(NW, PW)])
    eng.null_local_discard()
    codes = _walk(eng, data, NW)
    eng.set_samples(codes, NW, np.bincount(codes, minlength=NW).astype(float))
    eng.nam_steps(4)
    assert eng.select_standardized(None, None, y=y)[0] == 0
    X4 = eng.fetch_matrix(_ffi.MAT_X)
    thr = edges = None

    def setup(eng):
        nonlocal thr, edges
        eng.null_local_discard()
        codes = _walk(eng, data, NW)
        nz, maxabs = eng.select_standardized(None, None, y=y)
        assert nz == 0
        if thr is None:
            maxcorr = max(maxabs, 0.001)
            thr = np.arange(maxcorr / 4, maxcorr, maxcorr / 400)
            z2 = thr ** 2
            edges = z2 - 1e-8 - 1e-5 * z2
        eng.condition(np.eye(NW), Y)
        return codes, thr, edges
    codes, thr, edges = setup(eng)
    sums = eng.null_local_resident(1, PW, edges).sum(axis=0)       # want_tails: the f64 kernel
    ranks, numdet = eng.obs_counts(edges, thr)
    return dict(setup=setup, y=y, X4=X4, sums=sums, ranks=ranks, numdet=numdet)


@pytest.mark.parametrize('give_up', [False, True])
def test_walk_with_a_selection_hint_while_a_pass_is_pending(eng, wide, monkeypatch, give_up):
    """A pass is pending (its integer kernel kept or given up) when a walk of another length with a selection hint runs:
    the hint does not arm, so the fetch -- a given-up pass reruns in f64 on X -- returns the f64 kernel's sums of the
    launch's X; the next selection is then the separate pass, as after the same walk without a hint."""
    from cna_amd import _ffi
    codes, thr, edges = wide['setup'](eng)
    if give_up:
        monkeypatch.setenv('CNA_I8_QCAP', '8')
    else:
        monkeypatch.delenv('CNA_I8_QCAP', raising=False)
    eng.null_local_launch(1, PW, edges, thr)
    eng.set_samples(codes, NW, np.bincount(codes, minlength=NW).astype(float))
    eng.nam_select_hint(wide['y'])
    eng.nam_steps(4)
    sums, ranks, numdet = eng.null_local_fetch()
    monkeypatch.delenv('CNA_I8_QCAP', raising=False)
    used, rechecked, fallback = eng.null_local_i8_stats()
    assert used and fallback == give_up
    np.testing.assert_array_equal(sums, wide['sums'])
    np.testing.assert_array_equal(ranks, wide['ranks'])
    np.testing.assert_array_equal(numdet, wide['numdet'])
    assert eng.select_standardized(None, None, y=wide['y'])[0] == 0
    np.testing.assert_array_equal(eng.fetch_matrix(_ffi.MAT_X), wide['X4'])
