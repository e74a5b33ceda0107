"""cna.tl.gene_rank_test on the CPU: the numpy restatement of cna_x_columns (what the GPU tests compare the device with, byte
for byte), the inputs of the GPU tests, and the public call against an engine double -- tests/fake_engine.py with
`gene_rank_corr` and `gene_rank_corr_x` backed by the restatement of tests/test_gene_rank_corr_host.py, as `_double()` of
tests/test_gene_test_host.py backs `expr_cross` -- checked against scipy.stats.spearmanr on the oracle's residualised NAM and
null draw.  RHO_TOL is the project's figure for rho against scipy (tests/test_gene_rank_corr_host.py)."""
import functools
import os
import re
import warnings

import numpy as np
import pytest
import scipy.stats

from test_gene_markers_host import N_CORE, ROOT
from test_gene_rank_corr_host import RHO_TOL, as_engine, core_keys, restated_rank_corr
from test_gene_test_host import restated_bh


# ------------------------------------------------------------------ the restatement of cna_x_columns
def restated_columns(X, xrow, Z):
    """float64 [q, cells]: out[j, i] = sum over the samples, ascending, of X[xrow[i], s] * Z[j, s], each product rounded and
    then added to the running sum; NaN where xrow[i] == -1.  The loop of the header, whose bits the device must give."""
    X, Z = np.asarray(X, dtype=np.float64), np.atleast_2d(np.asarray(Z, dtype=np.float64))
    xrow = np.asarray(xrow)
    keep = xrow >= 0
    rows = xrow[keep]
    out = np.full((Z.shape[0], len(xrow)), np.nan)
    for j in range(Z.shape[0]):
        acc = np.zeros(len(rows))
        for s in range(X.shape[1]):
            acc = acc + X[rows, s] * Z[j, s]
        out[j, keep] = acc
    return out


# ------------------------------------------------------------------ the GPU tests' inputs
X_ROWS = 2700                       # rows of the uploaded X: nine cells in ten of the 3001 have one
COLUMN_SAMPLES = [1, 3, 33, 130]    # 3 and 33: the row stride of X is not the sample count
COLUMN_COUNTS = [1, 16, 17, 40]     # one column, a full group, last groups of 1 and of 8 columns
WIDE_COUNTS = [1, 16, 17, 33, 40]


@functools.lru_cache(maxsize=None)
def column_case(samples, q, integer=False):
    """(X float64 [2700, samples], xrow int64 [3001], Z float64 [q, samples]): xrow a permutation of the rows of X on 2700 of
    the 3001 cells and -1 elsewhere.  integer: small integers on both sides, so that the formed columns tie heavily.  Rows 5
    and 9 of X hold the same values: their two cells tie in every column."""
    rs = np.random.RandomState(1000 * samples + q + (7 if integer else 0))
    if integer:
        X = rs.randint(-2, 3, (X_ROWS, samples)).astype(np.float64)
        Z = rs.randint(-2, 3, (q, samples)).astype(np.float64)
        Z[Z.any(axis=1) == 0, 0] = 1.0                                           # no column of zeros only
    else:
        X = rs.randn(X_ROWS, samples) * (1.0 + rs.rand(samples)) + rs.randn(samples)
        Z = rs.randn(q, samples)
    X[9] = X[5]
    xrow = np.full(N_CORE, -1, dtype=np.int64)
    xrow[np.sort(rs.permutation(N_CORE)[:X_ROWS])] = rs.permutation(X_ROWS)
    for a in (X, xrow, Z):
        a.setflags(write=False)
    return X, xrow, Z


def constant_row(q):
    return q // 2 if q <= 16 else q // 2 + 1


@functools.lru_cache(maxsize=None)
def wide_keys(q):
    """float64 [q, 3001]: core_keys(16) tiled to q rows and perturbed.  Rows from 16 on are the negation of their row (ties
    kept, order reversed) or their row plus noise; row 16 equals row 0 (q > 16), row q - 2 equals row 0 (4 <= q <= 16); row
    constant_row(q) is constant on its finite cells (q > 1); three cells that every other row keeps are NaN in row q - 1 alone -- a
    column of the last group: the kept set is one per call, not one per group."""
    rs = np.random.RandomState(500 + q)
    base = core_keys(16)
    V = np.array(base[np.arange(q) % 16])
    for k in range(17, q):
        V[k] = -V[k] if k % 2 else V[k] + rs.randn(N_CORE) * 0.25
    if 4 <= q <= 16:
        V[q - 2] = V[0]
    if q > 1:
        V[constant_row(q)] = np.where(np.isfinite(V[constant_row(q)]), 4.0, np.nan)
    everywhere = np.flatnonzero(np.isfinite(V).all(axis=0))
    V[q - 1, everywhere[[150, 1200, 2500]]] = np.nan
    V = np.ascontiguousarray(V)
    V.setflags(write=False)
    return V


def test_restated_columns_are_the_matrix_product_and_keep_the_order_of_the_sum():
    X, xrow, Z = column_case(33, 17)
    out = restated_columns(X, xrow, Z)
    keep = xrow >= 0
    assert out.shape == (17, N_CORE) and int(keep.sum()) == X_ROWS and sorted(xrow[keep]) == list(range(X_ROWS))
    assert np.isnan(out[:, ~keep]).all() and np.isfinite(out[:, keep]).all()
    want = X[xrow[keep]] @ Z.T
    assert np.max(np.abs(out[:, keep].T - want)) <= 33 * 2.0 ** -52 * np.max(np.abs(X)) * np.max(np.abs(Z)) * 33
    # the order matters to the last bit somewhere: the restatement is not just any matrix product
    rev = restated_columns(X[:, ::-1], xrow, Z[:, ::-1])
    assert rev.tobytes() != out.tobytes() and np.allclose(rev[:, keep], out[:, keep], rtol=0, atol=1e-12)
    # integer inputs: exact whatever the order, and heavy ties
    Xi, xi, Zi = column_case(3, 16, True)
    outi = restated_columns(Xi, xi, Zi)
    assert np.array_equal(outi[:, xi >= 0].T, Xi[xi[xi >= 0]] @ Zi.T)
    assert all(len(np.unique(c[xi >= 0])) < 30 for c in outi) and all(np.ptp(c[xi >= 0]) > 0 for c in outi)


def test_the_inputs_reach_what_they_are_meant_to_reach():
    for q in WIDE_COUNTS:
        V = wide_keys(q)
        assert V.shape == (q, N_CORE)
        kept = np.isfinite(V).all(axis=0)
        without_last = np.isfinite(V[:q - 1]).all(axis=0) if q > 1 else np.isfinite(core_keys(16)[0])
        assert int(without_last.sum()) - int(kept.sum()) == 3                     # the last row alone drops three cells
        if q > 1:
            assert np.ptp(V[constant_row(q)][kept]) == 0.0 and constant_row(q) not in (0, 1, 16, q - 2, q - 1)
            assert len(np.unique(V[1][kept])) < 10                                # heavy ties
        if q > 16:
            assert np.array_equal(V[16][kept], V[0][kept]) and (q - 1) // 16 >= 1    # (q = 17: row 16 is the last one)
        elif q >= 4:
            assert np.array_equal(V[q - 2], V[0], equal_nan=True)
    for n in COLUMN_SAMPLES:
        X, xrow, Z = column_case(n, 16)
        assert X.shape == (X_ROWS, n) and Z.shape == (16, n) and (xrow == -1).sum() == N_CORE - X_ROWS
        assert np.array_equal(X[5], X[9])


# ------------------------------------------------------------------ the whole call on the numpy engine double
def _double(**kw):
    from fake_engine import FakeEngine
    from cna_amd._ffi import MAT_X

    class RankEngine(FakeEngine):
        """FakeEngine plus numpy restatements of the engine calls gene_rank_test adds to an association."""
        m_shift = 0

        def ensure_expression(self, X):
            self.E = np.asarray(X)

        def gene_rank_corr(self, V, work_bytes=0):
            return as_engine(restated_rank_corr(self.E, V))

        def gene_rank_corr_x(self, xrow, Z, work_bytes=0):
            self.Z_seen = np.array(Z)
            V = restated_columns(self.fetch_matrix(MAT_X), xrow, Z)        # rows of X in device order: what xrow names
            out = as_engine(restated_rank_corr(self.E, V))
            return out[:4] + (out[4] + self.m_shift,) + out[5:]
    return RankEngine(order='random', **kw)


@functools.lru_cache(maxsize=None)
def _qc_case():
    """40 samples in 10 batches, 2 covariates, one population drawn from one batch's samples: the QC drops cells (the recipe of
    tests/test_gene_test_host.py).  20 genes: gene 1 all zero, gene 2 non-zero only where no cell is kept, gene 3 with a NaN."""
    from cna_amd import synth
    from oracle import cna_oracle as orc
    data, meta = synth.make_dataset(3000, 40, k=15, seed=11, n_batches=10, n_covs=2, builder='cpu')
    cl, b = meta['cluster'], meta['batches'].values
    sid = np.asarray(data.obs['id']).copy()
    target = np.flatnonzero(cl == np.bincount(cl).argmax())
    sid[target] = np.random.RandomState(3).choice(np.flatnonzero(b == 0), size=len(target))
    data.obs['id'] = sid
    call = dict(nsteps=3, Nnull=60, seed=3)
    ref = orc.association(data, meta['y'], 'id', batches=meta['batches'], covs=meta['covs'], mode='f64', **call)
    kept = ref['kept']
    rs = np.random.RandomState(0)
    E = rs.gamma(2.0, 1.0, (3000, 20)) * (rs.rand(3000, 20) < 0.6)
    E[:, 1] = 0.0
    E[kept, 2] = 0.0
    E[np.flatnonzero(kept)[17], 3] = np.nan
    assert 0 < (~kept).sum() < 3000 and (E[~kept, 2] != 0).any()
    return data, meta, call, ref, E


def _run(eng, **kw):
    import cna_amd as cna
    data, meta, call, ref, E = _qc_case()
    d = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = cna.tl.gene_rank_test(d, meta['y'], 'id', batches=meta['batches'], covs=meta['covs'], engine=eng, **call, **kw)
    return d, out


def test_whole_call_against_spearmanr_on_the_oracle():
    import cna_amd as cna
    data, meta, call, ref, E = _qc_case()
    eng = _double()
    d, (frame, null_rho) = _run(eng, return_null=True, var_key_added='grt_')
    kept = ref['kept']
    assert eng.perm is not None and (eng.x_row_of_cells()[~kept] == -1).all()
    assert list(frame.columns) == ['rho', 'null_mean', 'null_sd', 'z', 'p', 'q'] and null_rho.shape == (20, 60)
    assert frame.attrs['n_null'] == 60 and frame.attrs['n_cells'] == int(kept.sum()) and frame.attrs['p'] == ref['p']
    # rho: the restated gene_rank_corr on the stored coefficient, and the public call's, bit for bit
    from cna_amd.tools._gene_rank_corr import rank_corr_statistics
    coef = d.obs['coef'].values
    assert np.array_equal(np.isfinite(coef), kept)
    want_rho = rank_corr_statistics(*as_engine(restated_rank_corr(E, coef[None, :])))[0]
    assert np.array_equal(frame['rho'].values, want_rho, equal_nan=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        assert np.array_equal(frame['rho'].values, cna.tl.gene_rank_corr(d, 'coef', engine=eng)['coef'].values, equal_nan=True)
    # constant over the kept cells (1, 2) and a NaN in a kept cell (3): NaN everywhere
    dead = np.zeros(20, dtype=bool)
    dead[[1, 2, 3]] = True
    assert np.isnan(frame.values[dead]).all() and np.isnan(null_rho[dead]).all()
    assert np.isfinite(frame.values[~dead]).all() and np.isfinite(null_rho[~dead]).all()
    # every null rho against scipy on the materialised null coefficients of the oracle
    Z = ref['M'].dot(ref['y_perm'][:, :60])
    Z = Z / Z.std(axis=0, ddof=1)
    assert eng.Z_seen.shape == (60, 40) and np.max(np.abs(eng.Z_seen.T - Z)) <= 1e-12
    Cn = ref['namresid'].dot(Z)                                        # kept cells x P
    worst = 0.0
    for g in np.flatnonzero(~dead):
        for p in range(60):
            want = scipy.stats.spearmanr(E[kept, g], Cn[:, p]).statistic
            worst = max(worst, abs(null_rho[g, p] - want))
    print('null_rho against scipy.stats.spearmanr: max |d rho| = %.3e (bound %.0e)' % (worst, RHO_TOL))
    assert worst <= RHO_TOL
    # p, q and null_mean exactly from the returned arrays
    rho = frame['rho'].values
    p = (1.0 + (np.abs(null_rho) >= np.abs(rho)[:, None]).sum(axis=1)) / 61.0
    p[dead] = np.nan
    assert np.array_equal(frame['p'].values, p, equal_nan=True)
    assert np.array_equal(frame['q'].values, restated_bh(p), equal_nan=True)
    assert np.array_equal(frame['null_mean'].values[~dead], null_rho[~dead].mean(axis=1))
    assert np.array_equal(frame['null_sd'].values[~dead], null_rho[~dead].std(axis=1, ddof=1))
    for k in ('rho', 'p', 'q'):
        assert np.array_equal(d.var['grt_' + k].values, frame[k].values, equal_nan=True)
    assert frame.index.equals(cna.tl.gene_rank_corr(d, 'coef', engine=eng).index)


def test_n_perm_cuts_the_columns_and_bad_values_are_refused():
    full_d, (full, null_full) = _run(_double(), return_null=True)
    eng = _double()
    d, (cut, null_cut) = _run(eng, return_null=True, n_perm=16)
    assert null_cut.shape == (20, 16) and cut.attrs['n_null'] == 16 and eng.Z_seen.shape == (16, 40)
    assert null_cut.tobytes() == np.ascontiguousarray(null_full[:, :16]).tobytes()
    assert np.array_equal(cut['rho'].values, full['rho'].values, equal_nan=True)
    ok = np.isfinite(cut['rho'].values)
    p = (1.0 + (np.abs(null_cut) >= np.abs(cut['rho'].values)[:, None]).sum(axis=1)) / 17.0
    assert np.array_equal(cut['p'].values[ok], p[ok])
    _, more = _run(_double(), n_perm=np.int64(5000))                   # more than there are: all of them
    assert more.attrs['n_null'] == 60
    for bad, exc in ((0, ValueError), (-3, ValueError), (2.5, TypeError), ('7', TypeError), (True, TypeError)):
        refuses = _double()
        with pytest.raises(exc, match='n_perm'):
            _run(refuses, n_perm=bad)
        assert not hasattr(refuses, 'E')                               # before anything ran


def test_the_m_mismatch_raises_and_names_both_numbers():
    _, _, _, ref, _ = _qc_case()
    eng = _double()
    eng.m_shift = 2
    m = int(ref['kept'].sum())
    with pytest.raises(RuntimeError, match=r'%d cells.*%d' % (m, m + 2)):
        _run(eng)


def test_refusals():
    import cna_amd as cna
    from cna_amd import dist
    from test_gene_test_host import _Refuses
    data, meta, call, ref, E = _qc_case()
    d = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E)
    part = dist.shard(d, rank=0, nranks=2)
    part.X = E[:len(part.obs)]
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.gene_rank_test(part, meta['y'], 'id', engine=_Refuses())
    two = _Refuses()
    two.__dict__['nranks'] = 2
    with pytest.raises(NotImplementedError, match='multi-rank'):
        cna.tl.gene_rank_test(d, meta['y'], 'id', engine=two)
    with pytest.raises(TypeError, match='return_full'):
        cna.tl.gene_rank_test(d, meta['y'], 'id', engine=_Refuses(), return_full=True)
    with pytest.raises(ValueError, match='data.X'):
        cna.tl.gene_rank_test(type(data)(data.obs[['id']].copy(), data.obsp['connectivities']), meta['y'], 'id', engine=_Refuses())
    assert 'coef' not in d.obs


def test_the_generator_is_left_as_a_plain_association_leaves_it():
    import cna_amd as cna
    data, meta, call, ref, E = _qc_case()
    unseeded = dict(call)
    del unseeded['seed']
    d = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        np.random.seed(5)
        a = cna.tl.gene_rank_test(d, meta['y'], 'id', batches=meta['batches'], covs=meta['covs'], engine=_double(), n_perm=4,
                                  **unseeded)
        after_test = np.random.get_state()
        d0 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'])
        np.random.seed(5)
        p0 = cna.tl.association(d0, meta['y'], 'id', batches=meta['batches'], covs=meta['covs'], engine=_double(), **unseeded)
        after_plain = np.random.get_state()
        seeded = cna.tl.gene_rank_test(d, meta['y'], 'id', batches=meta['batches'], covs=meta['covs'], engine=_double(), n_perm=4,
                                       seed=5, **unseeded)
    assert after_test[0] == after_plain[0] and np.array_equal(after_test[1], after_plain[1]) and after_test[2:] == after_plain[2:]
    assert a.attrs['p'] == p0 and a.equals(seeded)
    for k in ('coef', 'coef_fdr'):
        assert d.obs[k].values.tobytes() == d0.obs[k].values.tobytes(), k


# ------------------------------------------------------------------ the library's side
def test_the_three_entries_are_declared():
    import cna_amd as cna
    from cna_amd import _ffi
    from cna_amd.engine import Engine
    text = open(os.path.join(ROOT, 'include', 'cna_hip.h')).read()
    lib = _ffi.load()
    for name in ('cna_x_columns', 'cna_gene_rank_corr_x', 'cna_gene_rank_corr_wide'):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert re.search(r'\bint\s+%s\(cna_ctx\* ctx' % name, text), name
    block = text[text.index("Spearman's rho under the permuted phenotypes"):text.index('int  cna_x_columns(')]
    assert '_association.py:94-99' in block                            # the reference citation of the compute entries
    for name in ('x_columns', 'gene_rank_corr_x', 'gene_rank_corr_wide'):
        assert callable(getattr(Engine, name))
    assert 'gene_rank_test' in cna.tl.__all__ and callable(cna.tl.gene_rank_test)
    make = open(os.path.join(ROOT, 'cna_amd', 'csrc', 'Makefile')).read()
    assert 'expr_rankperm.hip' in make and re.search(r'^[^#\n]*expr_rankperm\.o[^\n]*: rank_sort\.h', make, flags=re.M)
    src = open(os.path.join(ROOT, 'cna_amd', 'csrc', 'expr_rankperm.hip')).read()
    assert '#pragma clang fp contract(off)' in src and 'rankcorr_keys(' in src and 'k_rc_mask<true>' in src
    # shared, not copied: one definition of each in the csrc tree
    tree = ''.join(open(os.path.join(ROOT, 'cna_amd', 'csrc', f)).read() for f in sorted(os.listdir(os.path.join(ROOT, 'cna_amd', 'csrc')))
                   if f.endswith(('.hip', '.h')))
    assert tree.count('void k_rc_mask(') == 1 and tree.count('struct alignas(4 * W) BRow') == 1
    assert tree.count('\nint rankcorr_keys(') == 2 and tree.count('void with_width(') == 1     # declared once, defined once


def test_engine_entries_refuse_a_sharded_engine():
    from cna_amd.engine import Engine
    import types
    e = types.SimpleNamespace(nranks=2, view_local=False)
    for name, args in (('x_columns', (np.zeros(3, dtype=np.int64), np.zeros((1, 2)))),
                       ('gene_rank_corr_x', (np.zeros(3, dtype=np.int64), np.zeros((1, 2)))),
                       ('gene_rank_corr_wide', (np.zeros((1, 3)),))):
        e._x_columns_args = types.MethodType(Engine._x_columns_args, e)
        with pytest.raises(NotImplementedError):
            types.MethodType(getattr(Engine, name), e)(*args)
    e.nranks, e.view_local = 1, True
    with pytest.raises(NotImplementedError):
        types.MethodType(Engine.gene_rank_corr_wide, e)(np.zeros((1, 3)))
