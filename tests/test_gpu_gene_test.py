"""cna.tl.gene_test / cna_expr_cross on the device (run with -m gpu on an MI355X).

Shapes: 3000 cells; 24 and 33 samples (33 is no multiple of 4 and crosses the dense kernel's tile of 32 samples); 70 and 130
genes (130 crosses a wave and leaves a ragged one); 3000 cells are 23 slabs of the dense kernel and, for the dense-ish
lists used here, several chunks of 1024 entries per gene.  One dataset has 5 batches and covariates ('b5'); with 5 batches no
batch kurtosis can reach the QC's threshold of 6 (five values have a kurtosis of at most 3.25), so the dataset on which the
QC drops cells and xrow holds -1 ('qc') has 10 batches, as fixture c12_batchy_qc itself has: 40 samples, covariates, one
population's cells all from the samples of one batch.  The default cell reorder is on (perm is not the identity), one case
runs with CNA_REORDER=0.

Bounds.  W, rho, sx, sxx against numpy in np.longdouble: |got - want| <= 2 (m - 1) 2^-52 sum_i |terms|, the bound of two
fixed-order float64 sums of the same m terms (tests/test_gpu_expr_to_sample.py uses the same form; the factor 2 covers the
rounding of each product, which the FMA does not even commit).  Integer-valued inputs: bit-exact.  End to end: r against
gene_corr and null_r against the materialised oracle within 100 x the CPU difference of tests/test_gene_test_host.py
(4.441e-16, profiles/r09_gene_test_parity.txt), never looser than 1e-8.  The largest figures seen go to the file
CNA_GENE_TEST_GPU_OUT names, when it is set.

The sample axis and the host loops (profiles/r10_gene_cross_wide_parity.txt).  cna_expr_cross branches on the number of
samples: k_xc_sparse<T, P> holds P = 1, 2, 4, 8, 16 accumulators per lane for up to 64, 128, 256, 512, 1024 samples, k_xc_dense
takes tiles of 32 samples (the last one ragged or full), k_xc_rho keeps four accumulators per thread (samples t, t + 256, ...),
and the row stride of X differs from the sample count where that is no multiple of 4.  WIDE_N walks both sides of each of
these at 2200 cells -- gene 0 present in every cell: chunks of 1024, 1024 and 152 entries, the last batch ragged; 17 slabs of
the dense kernel -- through an explicit xrow (a permutation of the rows of a shorter X, a tenth of the cells -1): integer-
valued inputs bit for bit at every count, real-valued ones against np.longdouble under the bound above at 65, 200 and 1024.
Beside them: NaN and Inf stay in their own gene (and out of every sum when their cell has no row in X), a second gene tile
of xc_sparse (tests/test_expr_tiles_host.py builds the input and proves its reach), k_xc_check's verdicts and k_xc_rho where
1.1 million cells take the grid-stride loop and 1024 blocks, and one end-to-end call at 130 samples."""
import ctypes as C
import os
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

CPU_DIFF = 4.441e-16                          # profiles/r09_gene_test_parity.txt, first line
R_TOL = min(100 * CPU_DIFF, 1e-8)
FORMS = ['dense-f32', 'dense-f64', 'csr', 'csc']
_seen = {}


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()
    if os.environ.get('CNA_GENE_TEST_GPU_OUT') and _seen:
        with open(os.environ['CNA_GENE_TEST_GPU_OUT'], 'w') as f:
            for k in sorted(_seen):
                f.write('%-70s %.3e\n' % (k, _seen[k]))


def _note(key, value):
    _seen[key] = max(_seen.get(key, 0.0), float(value))
    print('%s = %.3e' % (key, value))


def expression(n, g, seed, integer=False):
    """cells x genes float64, about 60 % present; gene 1 all zero."""
    rs = np.random.RandomState(seed)
    E = (rs.randint(0, 10, (n, g)).astype(np.float64) if integer else rs.gamma(2.0, 1.0, (n, g))) * (rs.rand(n, g) < 0.6)
    E[:, 1] = 0.0
    return E


def as_form(E, form):
    if form == 'dense-f32':
        return np.ascontiguousarray(E, dtype=np.float32)
    if form == 'dense-f64':
        return np.ascontiguousarray(E)
    return sp.csr_matrix(E) if form == 'csr' else sp.csc_matrix(E)


_cases = {}


def dataset(kind):
    """(data, y, batches, covs) of '24', '33' (plain), 'b5' (24 samples, 5 batches, 2 covariates) and 'qc' (40 samples, 10
    batches, 2 covariates, cells dropped by the QC)."""
    if kind not in _cases:
        from cna_amd import synth
        if kind == 'b5':
            data, meta = synth.make_dataset(3000, 24, k=15, seed=7, n_batches=5, n_covs=2)
        elif kind == 'qc':
            data, meta = synth.make_dataset(3000, 40, k=15, seed=11, n_batches=10, n_covs=2, builder='cpu')
            # one population's cells all from batch-0 samples: their neighbourhoods fail the batch-kurtosis QC (the recipe of
            # fixture c12_batchy_qc)
            cl, b = meta['cluster'], meta['batches'].values
            sid = np.asarray(data.obs['id']).copy()
            target = np.flatnonzero(cl == np.bincount(cl).argmax())
            sid[target] = np.random.RandomState(3).choice(np.flatnonzero(b == 0), size=len(target))
            data.obs['id'] = sid
        else:
            data, meta = synth.make_dataset(3000, int(kind), k=15, seed=int(kind))
        _cases[kind] = (data, meta['y'], meta['batches'], meta['covs'])
    return _cases[kind]


def analysed(eng, kind, **kw):
    import cna_amd as cna
    data, y, batches, covs = dataset(kind)
    call = dict(nsteps=3, Nnull=50, seed=1)
    call.update(kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = cna.tl.association(data, y, 'id', batches=batches, covs=covs, return_full=True, engine=eng, **call)
    return data, res


def reference_sums(EK, XK):
    """[(name, want, sum of |terms|)] of W, rho, sx, sxx in np.longdouble: EK the cells that take part x genes, XK their rows
    of X."""
    EK, XL = EK.astype(np.longdouble), XK.astype(np.longdouble)
    return [('W', EK.T @ XL, np.abs(EK).T @ np.abs(XL)), ('rho', XL.sum(axis=0), np.abs(XL).sum(axis=0)),
            ('sx', EK.sum(axis=0), np.abs(EK).sum(axis=0)), ('sxx', (EK * EK).sum(axis=0), (EK * EK).sum(axis=0))]


def check_against(tag, ref, m, out):
    """out[:4] against reference_sums' figures: |got - want| <= 2 (m - 1) 2^-52 sum |terms|."""
    u = 2.0 * (m - 1) * 2.0 ** -52
    for (name, want, mag), got in zip(ref, out[:4]):
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        bound = (u * mag).astype(np.float64)
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        _note('%s %s: max |err| / bound' % (tag, name), ratio)
        assert ratio <= 1.0, (tag, name, ratio)


def check_sums(tag, eng, E_used, kept, out):
    """out = engine.expr_cross() against longdouble numpy on E_used (the values the device holds, cells x genes)."""
    X = eng.x_full()                                                   # kept cells x samples, caller's order
    m = out[4]
    assert X.shape[0] == int(kept.sum()) and m == X.shape[0]
    check_against(tag, reference_sums(E_used[kept], X), m, out)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('kind,genes', [('24', 70), ('33', 130), ('b5', 70), ('qc', 130)])
def test_cross_against_longdouble(eng, kind, genes, form):
    data, res = analysed(eng, kind)
    kept = np.asarray(res.kept, dtype=bool)
    assert eng.perm is not None and not np.array_equal(eng.perm, np.arange(len(kept)))
    if kind == 'qc':
        assert 0 < (~kept).sum() < len(kept)                          # xrow holds -1
        assert (eng.x_row_of_cells()[~kept] == -1).all()
    E = expression(3000, genes, seed=genes)
    Ef = as_form(E, form)
    eng.ensure_expression(Ef)
    out = eng.expr_cross()
    check_sums('%s G=%d %s' % (kind, genes, form), eng, np.asarray(Ef.todense()) if sp.issparse(Ef) else Ef.astype(np.float64),
               kept, out)


def test_cross_without_reorder(eng, monkeypatch):
    monkeypatch.setenv('CNA_REORDER', '0')
    from cna_amd import synth
    import cna_amd as cna
    data, meta = synth.make_dataset(3000, 24, k=15, seed=91)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = cna.tl.association(data, meta['y'], 'id', nsteps=3, Nnull=50, seed=1, return_full=True, engine=eng)
    assert eng.perm is None
    E = expression(3000, 70, seed=5)
    eng.ensure_expression(E)
    check_sums('no reorder', eng, E, np.asarray(res.kept, dtype=bool), eng.expr_cross())


def _integer_case(eng, N, G):
    rs = np.random.RandomState(N)
    X = rs.randint(-3, 4, (3000, N)).astype(np.float64)
    E = expression(3000, G, seed=G, integer=True)
    eng.upload_x(X)
    return X, E


@pytest.mark.parametrize('N,G', [(24, 70), (33, 130)])
def test_integer_inputs_are_bit_exact_in_every_form_and_on_a_rerun(eng, N, G):
    X, E = _integer_case(eng, N, G)
    want = (E.T @ X, X.sum(axis=0), E.sum(axis=0), (E * E).sum(axis=0))
    got = {}
    for form in FORMS:
        eng.ensure_expression(as_form(E, form))
        out = eng.expr_cross()
        assert out[4] == 3000
        for a, b in zip(out[:4], want):
            assert np.array_equal(a, b), form
        eng._cross_memo = None
        again = eng.expr_cross()
        for a, b in zip(out[:4], again[:4]):
            assert a.tobytes() == b.tobytes(), form
        got[form] = out


@pytest.mark.parametrize('kind,genes', [('33', 130), ('qc', 70)])
def test_same_bits_on_a_rerun_and_from_csr_and_csc(eng, kind, genes):
    analysed(eng, kind)
    E = expression(3000, genes, seed=genes + 1)
    outs = {}
    for form in ('csr', 'csc', 'dense-f64'):
        eng.ensure_expression(as_form(E, form))
        a = eng.expr_cross()
        eng._cross_memo = None
        b = eng.expr_cross()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])) and a[4] == b[4], form
        outs[form] = a
    assert all(x.tobytes() == y.tobytes() for x, y in zip(outs['csr'][:4], outs['csc'][:4]))


def _raw_cross(eng, xrow, G, N):
    from cna_amd._ffi import ptr
    bufs = [np.full((G, N), 7.5), np.full(N, 7.5), np.full(G, 7.5), np.full(G, 7.5)]
    m = C.c_int64(-5)
    xrow = np.ascontiguousarray(xrow, dtype=np.int64)
    rc = eng.lib.cna_expr_cross(eng.h, ptr(xrow), len(xrow), ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), C.byref(m))
    return rc, bufs, m.value


def test_bad_xrow_is_refused_with_nothing_written(eng):
    X, E = _integer_case(eng, 24, 70)
    eng.ensure_expression(E)
    good = np.arange(3000, dtype=np.int64)
    cases = {'too large': (2999, 3000), 'below -1': (5, -2), 'twice': (17, 16)}
    for name, (i, v) in cases.items():
        xrow = good.copy()
        xrow[i] = v
        rc, bufs, m = _raw_cross(eng, xrow, 70, 24)
        assert rc == -1, name                                         # CNA_EINVAL
        assert all((b == 7.5).all() for b in bufs) and m == -5, name
    rc, bufs, m = _raw_cross(eng, good[:-1], 70, 24)                   # another length than the matrix' cells
    assert rc == -1 and all((b == 7.5).all() for b in bufs)
    xrow = good.copy()
    xrow[::3] = -1                                                     # -1 is fine, also many of them
    rc, bufs, m = _raw_cross(eng, xrow, 70, 24)
    assert rc == 0 and m == 2000
    keep = xrow >= 0
    assert np.array_equal(bufs[0], E[keep].T @ X[keep]) and np.array_equal(bufs[1], X[keep].sum(axis=0))


def test_missing_state_is_an_estate_error(eng):
    from cna_amd._ffi import CnaHipError
    from cna_amd.engine import Engine
    X, E = _integer_case(eng, 24, 70)
    eng.drop_expression()
    rc, _, _ = _raw_cross(eng, np.arange(3000), 70, 24)
    assert rc == -4                                                    # CNA_ESTATE: no expression matrix
    with pytest.raises(CnaHipError, match='no expression matrix'):
        eng.expr_cross()
    other = Engine()
    try:
        other.ensure_expression(E)
        rc, bufs, _ = _raw_cross(other, np.arange(3000), 70, 24)
        assert rc == -4 and (bufs[0] == 7.5).all()                     # CNA_ESTATE: no X
        with pytest.raises(CnaHipError, match='X not available'):
            other.expr_cross()
    finally:
        other.close()


def _oracle_null(data, y, batches, covs, E, P, **call):
    from oracle import cna_oracle as orc
    ref = orc.association(data, y, 'id', batches=batches, covs=covs, mode='f64', **call)
    kept = ref['kept']
    Z = ref['M'].dot(ref['y_perm'][:, :P])
    Z = Z / Z.std(axis=0, ddof=1)
    Cn = ref['namresid'].dot(Z) / ref['namresid'].shape[1]             # kept cells x P, materialised
    EK = E[kept]
    Ec = EK - EK.mean(axis=0)
    Cc = Cn - Cn.mean(axis=0)
    with np.errstate(all='ignore'):
        r = (Ec.T @ Cc) / np.sqrt(np.outer((Ec * Ec).sum(axis=0), (Cc * Cc).sum(axis=0)))
    return r, kept


def test_end_to_end_with_seed_3(eng):
    import cna_amd as cna
    from test_gene_test_host import restated_bh
    data, y, batches, covs = dataset('qc')
    call = dict(nsteps=3, Nnull=120, seed=3)
    E = expression(3000, 70, seed=70)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = data.obs.copy()
        d0 = type(data)(plain, data.obsp['connectivities'])
        p0 = cna.tl.association(d0, y, 'id', batches=batches, covs=covs, engine=eng, **call)
        kept0 = np.isfinite(d0.obs['coef'].values)
    assert (~kept0).any()
    E[kept0, 2] = 0.0                                                  # gene 2: non-zero only on cells the QC dropped
    assert (E[~kept0, 2] != 0).any()
    data.X = E
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        frame, null_r = cna.tl.gene_test(data, y, 'id', batches=batches, covs=covs, return_null=True, var_key_added='gt_',
                                         engine=eng, **call)
        rc = cna.tl.gene_corr(data, 'coef', engine=eng)['coef'].values
    assert list(frame.columns) == ['r', 'null_mean', 'null_sd', 'z', 'p', 'q'] and null_r.shape == (70, 120)
    # data.obs as a plain call leaves it
    for k in ('coef', 'coef_fdr'):
        assert data.obs[k].values.tobytes() == d0.obs[k].values.tobytes(), k
    # the constant genes
    for g in (1, 2):
        assert np.isnan(frame[['r', 'p', 'q']].values[g]).all() and np.isnan(null_r[g]).all()
    ok = np.ones(70, dtype=bool)
    ok[[1, 2]] = False
    assert np.isfinite(frame.values[ok]).all() and np.isnan(rc[~ok]).all()
    d_r = float(np.max(np.abs(frame['r'].values[ok] - rc[ok])))
    want, kept_ref = _oracle_null(data, y, batches, covs, E, 120, **call)
    assert np.array_equal(kept_ref, kept0)
    d_null = float(np.max(np.abs(null_r[ok] - want[ok])))
    _note('end to end: max |r - gene_corr|', d_r)
    _note('end to end: max |null_r - materialised oracle|', d_null)
    assert d_r <= R_TOL and d_null <= R_TOL, (d_r, d_null, R_TOL)
    # p and q exactly as recomputed from the returned arrays
    r = frame['r'].values
    p = (1.0 + (np.abs(null_r) >= np.abs(r)[:, None]).sum(axis=1)) / 121.0
    p[~ok] = np.nan
    assert np.array_equal(frame['p'].values, p, equal_nan=True)
    assert np.array_equal(frame['q'].values, restated_bh(p), equal_nan=True)
    assert np.array_equal(frame['null_mean'].values[ok], null_r[ok].mean(axis=1))
    assert np.array_equal(data.var['gt_p'].values, frame['p'].values, equal_nan=True)
    # the scalar p of gene_test's association is the plain call's, bit for bit
    assert frame.attrs['p'] == p0 and frame.attrs['n_null'] == 120


def test_global_rng_and_seed_none(eng):
    import cna_amd as cna
    data, y, batches, covs = dataset('24')
    data.X = expression(3000, 70, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a, na = cna.tl.gene_test(data, y, 'id', nsteps=3, Nnull=60, seed=5, return_null=True, engine=eng)
        np.random.seed(5)
        b, nb = cna.tl.gene_test(data, y, 'id', nsteps=3, Nnull=60, return_null=True, engine=eng)
        after_test = np.random.get_state()
        np.random.seed(5)
        cna.tl.association(data, y, 'id', nsteps=3, Nnull=60, engine=eng)
        after_plain = np.random.get_state()
    assert a.equals(b) and na.tobytes() == nb.tobytes()
    assert after_test[0] == after_plain[0] and np.array_equal(after_test[1], after_plain[1]) and after_test[2:] == after_plain[2:]


def test_nnull_caps_and_warning(eng):
    import cna_amd as cna
    data, y, batches, covs = dataset('24')
    data.X = expression(3000, 70, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, big = cna.tl.gene_test(data, y, 'id', nsteps=3, Nnull=1500, seed=2, return_null=True, engine=eng)
    assert big.shape == (70, 1000)
    with pytest.warns(UserWarning, match='smallest p-value 50 permutations'):
        _, small = cna.tl.gene_test(data, y, 'id', nsteps=3, Nnull=50, seed=2, return_null=True, engine=eng)
    assert small.shape == (70, 50)


def test_memo(eng):
    import cna_amd as cna
    data, y, batches, covs = dataset('qc')
    data.X = expression(3000, 70, seed=8)
    y2 = pd.Series(np.random.RandomState(4).randn(len(y)), index=y.index)
    call = dict(nsteps=3, Nnull=60, seed=2, engine=eng)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        cna.tl.gene_test(data, y, 'id', batches=batches, covs=covs, **call)
        n0 = eng.cross_launches
        passes = []
        real_gene_corr = eng.gene_corr
        eng.gene_corr = lambda V: passes.append(1) or real_gene_corr(V)
        try:
            f2, null2 = cna.tl.gene_test(data, y2, 'id', batches=batches, covs=covs, return_null=True, **call)
        finally:
            del eng.gene_corr
        assert eng.cross_launches == n0                                # a second phenotype on the same covariates
        assert passes == []                                            # ... passes over the expression matrix for nothing
        # ... and what the memo served is what a fresh pass gives
        eng._cross_memo = None
        f3, null3 = cna.tl.gene_test(data, y2, 'id', batches=batches, covs=covs, return_null=True, **call)
        assert eng.cross_launches == n0 + 1 and null3.tobytes() == null2.tobytes() and f3.equals(f2)
        cna.tl.gene_test(data, y2, 'id', batches=batches, covs=covs.iloc[:, :1], **call)
        assert eng.cross_launches == n0 + 2                            # other covariates: another X
        eng.drop_expression()
        base = eng.device_bytes()
        cna.tl.gene_test(data, y2, 'id', batches=batches, covs=covs.iloc[:, :1], **call)
        assert eng.cross_launches == n0 + 3                            # dropped: uploaded and taken again
        eng.drop_expression()
        assert eng.device_bytes() == base


def test_cross_between_launch_and_fetch(eng):
    """Both only read X: the cross on the expression stream between the launch and the fetch of a local-null pass leaves
    both results as they are without it."""
    data, res = analysed(eng, '33')
    E = expression(3000, 130, seed=12)
    eng.ensure_expression(E)
    rs = np.random.RandomState(0)
    Y = rs.randn(33, 41)
    eng.condition(np.eye(33), Y)
    _, maxabs = eng.ncorrs(Y[:, 0] / Y[:, 0].std())
    thr = np.arange(maxabs / 4, maxabs, maxabs / 400)
    edges = thr ** 2 - 1e-8 - 1e-5 * thr ** 2

    def null_pass(between):
        eng.null_local_launch(1, 40, edges, thr)
        mid = between() if between else None
        return [np.array(a) for a in eng.null_local_fetch()], mid
    alone, _ = null_pass(None)
    eng._cross_memo = None
    cross_alone = eng.expr_cross()
    eng._cross_memo = None
    mixed, cross_mid = null_pass(eng.expr_cross)
    assert all(np.array_equal(a, b) for a, b in zip(alone, mixed))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cross_alone[:4], cross_mid[:4]))


def test_end_to_end_on_the_two_call_path(eng):
    """The common call -- one batch, a seed, nsteps given -- is answered by the two-call path (tools/_fast.py), whose Gram
    matrix is the one cna_assoc_finish left: r against gene_corr and null_r against the materialised oracle there too."""
    import cna_amd as cna
    from cna_amd.tools import _fast
    data, y, batches, covs = dataset('24')
    E = expression(3000, 70, seed=21)
    data.X = E
    call = dict(nsteps=3, Nnull=120, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d0 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'])
        p0 = cna.tl.association(d0, y, 'id', engine=eng, **call)
        before = _fast.stats['taken']
        frame, null_r = cna.tl.gene_test(data, y, 'id', return_null=True, engine=eng, **call)
        rc = cna.tl.gene_corr(data, 'coef', engine=eng)['coef'].values
    assert _fast.stats['taken'] == before + 1                          # gene_test's association took that path
    assert frame.attrs['p'] == p0
    for k in ('coef', 'coef_fdr'):
        assert data.obs[k].values.tobytes() == d0.obs[k].values.tobytes(), k
    want, kept_ref = _oracle_null(data, y, None, None, E, 120, **call)
    assert kept_ref.all()
    ok = np.arange(70) != 1
    d_r = float(np.max(np.abs(frame['r'].values[ok] - rc[ok])))
    d_null = float(np.max(np.abs(null_r[ok] - want[ok])))
    _note('two-call path: max |r - gene_corr|', d_r)
    _note('two-call path: max |null_r - materialised oracle|', d_null)
    assert d_r <= R_TOL and d_null <= R_TOL, (d_r, d_null, R_TOL)


def test_without_the_local_test(eng):
    """local_test=False: the association writes the coefficient column and no FDR column (a plain call raises at that point,
    as upstream does); gene_test returns its frame, from a Gram matrix it had to find without the local test's schedule."""
    import cna_amd as cna
    data, y, batches, covs = dataset('33')
    d1 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=expression(3000, 70, seed=22))
    d2 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=d1.X)
    call = dict(nsteps=3, Nnull=80, seed=4, engine=eng)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        f1, n1 = cna.tl.gene_test(d1, y, 'id', return_null=True, local_test=False, **call)
        assert 'coef' in d1.obs and 'coef_fdr' not in d1.obs
        f2, n2 = cna.tl.gene_test(d2, y, 'id', return_null=True, **call)
        with pytest.raises(AttributeError):
            cna.tl.association(d1, y, 'id', local_test=False, **call)          # the plain call keeps upstream's end
    assert n1.shape == (70, 80) and np.isfinite(f1.values[np.arange(70) != 1]).all()
    assert d1.obs['coef'].values.tobytes() == d2.obs['coef'].values.tobytes()
    assert np.max(np.abs(n1 - n2)[np.arange(70) != 1]) <= R_TOL and np.max(np.abs(f1['r'] - f2['r']).values[np.arange(70) != 1]) <= R_TOL
    assert f1.attrs['p'] == f2.attrs['p']


# ------------------------------------------------------------------ the sample axis: every P of k_xc_sparse, 2 to 32 dense tiles
WIDE_N = [64, 65, 100, 128, 129, 200, 256, 257, 512, 513, 1024]
WIDE_CELLS = 2200


def wide_case(N, G, integer, seed=0):
    """(E, X, xrow): E as expression() makes it, but gene 0 present in every cell (gene 1 stays empty) and, real-valued,
    rounded to float32 so that the four forms hold the same values; X with fewer rows than there are cells; xrow a random
    permutation of X's rows on nine cells in ten, -1 on the others."""
    n = WIDE_CELLS
    rs = np.random.RandomState(1000 * N + G + seed)
    E = expression(n, G, seed=N + G + seed, integer=integer)
    E[:, 0] = rs.randint(1, 10, n) if integer else 0.5 + rs.gamma(2.0, 1.0, n)
    if not integer:
        E = E.astype(np.float32).astype(np.float64)
    took = rs.rand(n) < 0.9
    nx = int(took.sum())
    X = rs.randint(-3, 4, (nx, N)).astype(np.float64) if integer else rs.randn(nx, N) * (1.0 + rs.rand(N)) + rs.randn(N)
    xrow = np.full(n, -1, dtype=np.int64)
    xrow[took] = rs.permutation(nx)
    assert nx < n and (E[:, 0] != 0).all() and not E[:, 1].any()
    return E, X, xrow


def _integer_want(E, X, xrow):
    keep = xrow >= 0
    EK, XK = E[keep], X[xrow[keep]]
    return (EK.T @ XK, XK.sum(axis=0), EK.sum(axis=0), (EK * EK).sum(axis=0)), int(keep.sum())


@pytest.mark.parametrize('G', [70, 130])
@pytest.mark.parametrize('N', WIDE_N)
def test_wide_integer_inputs_are_bit_exact_in_every_form_and_on_a_rerun(eng, N, G):
    """Every partial sum is an integer far below 2^53 (at most 2200 x 9 x 3), so float64 numpy is exact in any order."""
    E, X, xrow = wide_case(N, G, integer=True)
    want, m = _integer_want(E, X, xrow)
    eng.upload_x(X)
    for form in FORMS:
        eng.ensure_expression(as_form(E, form))
        out = eng.expr_cross(xrow=xrow)
        assert out[4] == m and out[0].shape == (G, N) and out[1].shape == (N,)
        for name, a, b in zip(('W', 'rho', 'sx', 'sxx'), out[:4], want):
            assert np.array_equal(a, b), (form, name)
        eng._cross_memo = None
        again = eng.expr_cross(xrow=xrow)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out[:4], again[:4])) and again[4] == m, form


@pytest.mark.parametrize('N', [65, 200, 1024])
def test_wide_real_inputs_against_longdouble(eng, N):
    G = 70
    E, X, xrow = wide_case(N, G, integer=False)
    keep = xrow >= 0
    ref = reference_sums(E[keep], X[xrow[keep]])                     # once: the four forms hold the same float32 values
    eng.upload_x(X)
    outs = {}
    for form in FORMS:
        Ef = as_form(E, form)
        assert np.array_equal(np.asarray(Ef.todense()) if sp.issparse(Ef) else Ef.astype(np.float64), E)
        eng.ensure_expression(Ef)
        outs[form] = eng.expr_cross(xrow=xrow)
        assert outs[form][4] == int(keep.sum())
        check_against('wide N=%d G=%d %s' % (N, G, form), ref, outs[form][4], outs[form])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs['csr'][:4], outs['csc'][:4]))


# ------------------------------------------------------------------ NaN and Inf stay where they are
@pytest.mark.parametrize('form', ['dense-f32', 'dense-f64', 'csr', 'csc'])
@pytest.mark.parametrize('N', [33, 200])
def test_nan_and_inf_touch_only_their_own_gene(eng, N, form):
    G = 70
    E, X, xrow = wide_case(N, G, integer=True, seed=7)
    took, left = np.flatnonzero(xrow >= 0), np.flatnonzero(xrow < 0)
    eng.upload_x(X)

    def run(M):
        eng.ensure_expression(as_form(M, form))
        return eng.expr_cross(xrow=xrow)
    clean = run(E)
    want, m = _integer_want(E, X, xrow)
    assert all(np.array_equal(a, b) for a, b in zip(clean[:4], want))
    # in cells that take part: the first, one in the second chunk of gene 0's list, the last; the genes 0 (three chunks), 9 and
    # 64 (the second gene block of the dense kernel)
    hit = {0: (took[len(took) // 2], np.nan), 9: (took[0], np.inf), 64: (took[-1], -np.inf)}
    assert took[len(took) // 2] > 1024
    D = E.copy()
    for g, (cell, v) in hit.items():
        D[cell, g] = v
    got = run(D)
    bad = np.zeros(G, dtype=bool)
    bad[list(hit)] = True
    assert got[4] == m and got[1].tobytes() == clean[1].tobytes()                     # rho
    for a, b in zip((got[0], got[2], got[3]), (clean[0], clean[2], clean[3])):
        assert not np.isfinite(a[bad]).any()
        assert a[~bad].tobytes() == b[~bad].tobytes()
    assert np.isnan(got[2][0]) and got[2][9] == np.inf and got[2][64] == -np.inf and got[3][64] == np.inf
    # in cells without a row in X: never read into a sum
    D = E.copy()
    D[left[0], 0], D[left[len(left) // 2], 9], D[left[-1], 64], D[left[1], 1] = np.nan, np.inf, -np.inf, np.nan
    got = run(D)
    assert got[4] == m and all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], clean[:4]))


# ------------------------------------------------------------------ more than one gene tile
def test_second_gene_tile_of_the_gene_major_cross(eng):
    """33 100 genes of one chunk each against 1024 samples: xc_sparse goes over the genes in two tiles (the first full to its
    last chunk, an empty gene closing it; tests/test_expr_tiles_host.py asserts that).  Integer-valued, against
    scipy.sparse @ dense in float64, bit for bit.  W takes 271 MB on each side."""
    from test_expr_tiles_host import cross_tile_case, assert_cross_tile_case, cross_reference
    E, X, xrow = cross_tile_case()
    assert_cross_tile_case(E)
    want = cross_reference(E, X, xrow)
    eng.upload_x(X)
    eng.ensure_expression(E)
    assert eng.expression_shape()['format'] == 'gene-major'
    got = eng.expr_cross(xrow=xrow)
    eng.drop_expression()
    assert got[4] == want[4]
    for name, a, b in zip(('W', 'rho', 'sx', 'sxx'), got[:4], want[:4]):
        assert np.array_equal(a, b), name


# ------------------------------------------------------------------ k_xc_check and k_xc_rho beyond one thread per cell
LONG_CELLS = 1100000               # k_xc_check: 4096 blocks x 256 threads = 1 048 576 cells before the grid-stride loop starts
LONG_GRID = 4096 * 256


def long_case():
    """(E, X, xrow, took): 1.1M cells x 3 genes CSC with about 5000 integer entries, a third of them in cells that take part;
    X 500 x 33; xrow -1 but for 500 cells spread over the whole range (the first, the last, 120 beyond cell 1 048 576)."""
    if 'long' not in _cases:
        rs = np.random.RandomState(77)
        n = LONG_CELLS
        inner = rs.choice(np.arange(1, LONG_GRID), 379, replace=False)
        outer = rs.choice(np.arange(LONG_GRID, n - 1), 119, replace=False)
        took = np.sort(np.r_[0, inner, outer, n - 1])
        xrow = np.full(n, -1, dtype=np.int64)
        xrow[took] = rs.permutation(500)
        X = rs.randint(-3, 4, (500, 33)).astype(np.float64)
        cols = []
        for g in range(3):
            cells = np.unique(np.r_[rs.choice(took, 300, replace=False), rs.randint(0, n, 1400)])
            cols.append(sp.csc_matrix((rs.randint(1, 10, len(cells)).astype(np.float64), (cells, np.zeros(len(cells), dtype=int))),
                                      shape=(n, 1)))
        E = sp.hstack(cols, format='csc')
        assert len(took) == 500 and (took >= LONG_GRID).sum() >= 100 and 4500 < E.nnz < 5500
        _cases['long'] = (E, X, xrow, took)
    return _cases['long']


def test_long_cell_axis_valid_map(eng):
    E, X, xrow, took = long_case()
    EK, XK = E.tocsr()[took], X[xrow[took]]
    want = (np.asarray(EK.T @ XK), XK.sum(axis=0), np.asarray(EK.sum(axis=0)).ravel(), np.asarray(EK.multiply(EK).sum(axis=0)).ravel())
    assert np.abs(want[0]).sum() > 0
    eng.upload_x(X)
    one = np.ascontiguousarray(E[:, [0]].toarray(), dtype=np.float32)           # dense, one gene: 4.4 MB, 2045 slabs of 538 cells
    for tag, M, sel in (('csc', E, slice(None)), ('dense-f32 one gene', one, slice(0, 1))):
        eng.ensure_expression(M)
        got = eng.expr_cross(xrow=xrow)
        assert got[4] == 500, tag
        assert np.array_equal(got[0], want[0][sel]) and np.array_equal(got[1], want[1]), tag
        assert np.array_equal(got[2], want[2][sel]) and np.array_equal(got[3], want[3][sel]), tag


def test_long_cell_axis_refusals(eng):
    """The verdicts of k_xc_check where a cell is reached by the grid-stride loop: refused before anything is written."""
    E, X, xrow, took = long_case()
    eng.upload_x(X)
    eng.ensure_expression(E)
    n = LONG_CELLS
    low, high = took[took < LONG_GRID][5], took[took >= LONG_GRID][5]
    free = np.flatnonzero(xrow[n - 1000:] < 0)[[3, -3]] + n - 1000                 # two cells of the last 1000 without a row
    cases = {'twice': (high, xrow[low], 'two cells name the same row of X'),
             'too large': (free[0], 500, 'an xrow lies outside'),
             'far too large': (free[1], 2 ** 40, 'an xrow lies outside'),
             'below -1': (free[1], -2, 'an xrow lies outside')}
    for name, (i, v, msg) in cases.items():
        bad = xrow.copy()
        bad[i] = v
        assert i >= LONG_GRID, name
        rc, bufs, m = _raw_cross(eng, bad, 3, 33)
        assert rc == -1, name                                          # CNA_EINVAL
        assert msg in eng.lib.cna_last_error().decode(), name
        assert all((b == 7.5).all() for b in bufs) and m == -5, name
    rc, bufs, m = _raw_cross(eng, xrow, 3, 33)                         # the map itself passes, through the same entry
    assert rc == 0 and m == 500


# ------------------------------------------------------------------ end to end at a wide sample axis
@pytest.mark.parametrize('form', ['dense-f32', 'csr'])
def test_end_to_end_at_130_samples(eng, form):
    """130 samples: k_xc_sparse<T, 4> / five dense tiles (the last of 2) inside the whole call.  r against gene_corr, null_r
    against the materialised oracle, within R_TOL (the CPU difference of the restatement at 130 samples is in
    profiles/r10_gene_cross_wide_parity.txt)."""
    import cna_amd as cna
    if 'wide' not in _cases:
        from cna_amd import synth
        data, meta = synth.make_dataset(3000, 130, k=15, seed=130)
        _cases['wide'] = (data, meta['y'])
    data, y = _cases['wide']
    E = expression(3000, 70, seed=131).astype(np.float32).astype(np.float64)
    d = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=as_form(E, form))
    call = dict(nsteps=3, Nnull=50, seed=9)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        frame, null_r = cna.tl.gene_test(d, y, 'id', return_null=True, engine=eng, **call)
        rc = cna.tl.gene_corr(d, 'coef', engine=eng)['coef'].values
    assert null_r.shape == (70, 50) and eng.expr_cross()[0].shape == (70, 130)
    want, kept_ref = _oracle_null(d, y, None, None, E, 50, **call)
    assert np.array_equal(kept_ref, np.isfinite(d.obs['coef'].values))
    ok = np.arange(70) != 1
    assert np.isnan(frame['r'].values[1]) and np.isfinite(frame.values[ok]).all()
    d_r = float(np.max(np.abs(frame['r'].values[ok] - rc[ok])))
    d_null = float(np.max(np.abs(null_r[ok] - want[ok])))
    _note('130 samples %s: max |r - gene_corr|' % form, d_r)
    _note('130 samples %s: max |null_r - materialised oracle|' % form, d_null)
    assert d_r <= R_TOL and d_null <= R_TOL, (d_r, d_null, R_TOL)
