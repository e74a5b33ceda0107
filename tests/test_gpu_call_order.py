"""State the library keeps between two calls (run with -m gpu on an MI355X).

A local-null pass lives from cna_null_local_launch to cna_null_local_fetch.  Should its integer kernel give up (a recheck
queue overflow, forced here through CNA_I8_QCAP), the fetch reruns it on the f64 kernel -- on the X, the conditioned
phenotypes and the exact cuts the launch saw.  The contract (csrc/c_api.hip: NO_NULL_PENDING): an entry point that would
rewrite X or carve the scratch those cuts live in refuses with CNA_ESTATE while a pass is pending, changes nothing, and
the fetch returns the f64 kernel's integers.  Also here: the FDR column the helper thread copies while a given-up pass is
collected, and the Gram matrix queued with a selection that turns out to have cells of zero variance."""
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
