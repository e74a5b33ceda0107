"""cna.tl.gene_test_strata on the CPU: the sample-space algebra per level against the materialised null, the frame, the
arguments -- and the case and the two routes that tests/test_gpu_gene_test_strata.py runs on the device.

The algebra.  For a level l with kept cells C_l the null coefficient of permutation p on those cells is c_p = X_l z_p / N.
`level_statistics` sees only the sums W_l = E_l^T X_l, rho_l, sx_l, sxx_l, m_l, Gamma_l = X_l^T X_l (formed in numpy here) and
must give, per level, what np.corrcoef gives on the materialised cells x permutations matrix restricted to C_l.

The parity figure.  Within a level the coefficient's variance is smaller than over all cells, so the centring of the
sample-space route cancels more than in gene_test (4.4e-16 there).  `cpu_parity()` measures, on the very case of the GPU test
(the 'qc' dataset: 3 000 cells x 40 samples, 70 genes, a clustering with NaN, Nnull=120, seed=3), the largest difference
between the sample-space route on numpy sums and the materialised route: the first line of
profiles/gene_test_strata_parity.txt, which the GPU test reads for its tolerance.  Here it must stay below 1e-10: the
centred sums lose about eps x m x (mean / sd)^2 of a level's coefficient, 2.2e-16 x 3 000 x 100 at the very worst."""
import os
import warnings

import numpy as np
import pandas as pd
import pytest

from cna_amd.tools._gene_test import benjamini_hochberg, permutation_stats
from cna_amd.tools._gene_test_strata import STATISTICS, level_statistics, strata_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_FILE = os.path.join(ROOT, 'profiles', 'gene_test_strata_parity.txt')
CPU_BOUND = 1e-10


# ------------------------------------------------------------------ the two routes, in numpy
def level_sums(E, X, codes, L):
    """(W, rho, sx, sxx, m, Gamma) per level from E (cells x genes) and X (the same cells x samples), codes -1 = left out"""
    G, N = E.shape[1], X.shape[1]
    W, rho, sx, sxx = np.zeros((L, G, N)), np.zeros((L, N)), np.zeros((L, G)), np.zeros((L, G))
    m, Gam = np.zeros(L, dtype=np.int64), np.zeros((L, N, N))
    for l in range(L):
        EK, XK = E[codes == l], X[codes == l]
        W[l], rho[l], sx[l], sxx[l], m[l], Gam[l] = EK.T @ XK, XK.sum(axis=0), EK.sum(axis=0), (EK * EK).sum(axis=0), len(EK), XK.T @ XK
    return W, rho, sx, sxx, m, Gam


def level_constant(E, codes, L):
    """constant[l, g]: gene g does not vary on the cells of level l (minimum == maximum; a level without cells counts)"""
    out = np.ones((L, E.shape[1]), dtype=bool)
    for l in range(L):
        EK = E[codes == l]
        if len(EK):
            out[l] = EK.min(axis=0) == EK.max(axis=0)
    return out


def materialised_by_level(E, X, codes, L, Zall):
    """r_all[l, g, p] = np.corrcoef of gene g with the coefficient X z_p / N over the cells of level l, the cells x
    permutations matrix formed; NaN for a level with fewer than two cells, a constant gene or a constant coefficient."""
    Cn = X @ Zall / X.shape[1]
    out = np.full((L, E.shape[1], Zall.shape[1]), np.nan)
    for l in range(L):
        EK, CK = E[codes == l], Cn[codes == l]
        if len(EK) < 2:
            continue
        live = EK.min(axis=0) != EK.max(axis=0)
        with np.errstate(all='ignore'):
            full = np.corrcoef(EK[:, live], CK, rowvar=False)
        out[l][live] = full[:int(live.sum()), int(live.sum()):]
    return out


def restated_bh(p):
    """Benjamini-Hochberg over the finite entries, written out: q_i = min over j with p_j >= p_i of p_j n / rank_j, <= 1"""
    p = np.asarray(p, dtype=np.float64)
    q = np.full(p.shape, np.nan)
    ok = np.flatnonzero(np.isfinite(p))
    n = len(ok)
    order = ok[np.argsort(p[ok], kind='stable')]
    for i, gi in enumerate(order):
        q[gi] = min(1.0, min(p[order[j]] * n / (j + 1) for j in range(i, n)))
    return q


# ------------------------------------------------------------------ the algebra on one small case
def small_case():
    """5 levels, 24 samples, 40 genes, 30 permutations on 400 cells: level 3 keeps one cell, level 4 none, gene 7 is constant
    (and not zero) inside level 1; the coefficient has an offset per level, as a cluster's has."""
    rs = np.random.RandomState(5)
    n, N, G, P, L = 400, 24, 40, 30, 5
    codes = rs.choice([0, 1, 2], n, p=[0.6, 0.25, 0.15]).astype(np.int32)
    codes[rs.rand(n) < 0.05] = -1
    codes[17] = 3
    X = rs.randn(n, N) + 0.5 * rs.randn(3, N)[np.maximum(codes, 0) % 3]
    E = rs.gamma(2.0, 1.0, (n, G)) * (rs.rand(n, G) < 0.6)
    E[codes == 1, 7] = 2.5
    Zall = rs.randn(N, P + 1)
    Zall = Zall / Zall.std(axis=0, ddof=1)
    return E, X, codes, L, Zall


def test_sample_space_route_equals_materialised_route_per_level():
    E, X, codes, L, Zall = small_case()
    sums = level_sums(E, X, codes, L)
    assert list(sums[4][3:]) == [1, 0] and (sums[4][:3] > 20).all()
    constant = level_constant(E, codes, L)
    assert constant[1, 7] and constant[:3].sum() == 1
    table, null_r = level_statistics(sums, Zall, constant)
    want = materialised_by_level(E, X, codes, L, Zall)
    assert table.shape == (5, 6, 40) and null_r.shape == (5, 40, 30)
    # the NaN levels and the constant gene
    assert np.isnan(table[3:]).all() and np.isnan(null_r[3:]).all()
    assert np.isnan(table[1, :, 7]).all() and np.isnan(null_r[1, 7]).all()
    ok = ~constant
    ok[3:] = False
    assert np.isfinite(table[:, 0][ok]).all() and np.isfinite(want[..., 0][ok]).all()
    d = max(float(np.max(np.abs(table[:, 0][ok] - want[..., 0][ok]))), float(np.max(np.abs(null_r[ok] - want[..., 1:][ok]))))
    print('5 levels x 24 samples x 40 genes x 30 permutations: max |sample space - materialised| = %.3e' % d)
    assert d <= 1e-12
    # the statistics follow from r and null_r exactly, level by level; q is BH inside the level
    for l in range(3):
        mean, sd, z, p, q = permutation_stats(table[l, 0], null_r[l])
        for k, a in enumerate((mean, sd, z, p, q)):
            assert np.array_equal(table[l, k + 1], a, equal_nan=True)
        hits = (np.abs(null_r[l]) >= np.abs(table[l, 0])[:, None]).sum(axis=1)
        pw = np.where(np.isfinite(table[l, 0]), (1.0 + hits) / 31.0, np.nan)
        assert np.array_equal(table[l, 4], pw, equal_nan=True)
        assert np.array_equal(table[l, 5], restated_bh(pw), equal_nan=True)
    assert np.isfinite(table[1, 5]).sum() == 39 and np.isfinite(table[0, 5]).sum() == 40


def test_frame_layout():
    E, X, codes, L, Zall = small_case()
    table, _ = level_statistics(level_sums(E, X, codes, L), Zall, level_constant(E, codes, L))
    levels = pd.Index(['b', 'a', 'z', 'solo', 'none'])
    frame = strata_frame(table, levels, 'leiden', pd.Index(['g%d' % i for i in range(40)], name='gene'))
    assert frame.shape == (40, 30) and (frame.dtypes == np.float64).all()
    assert frame.columns.names == ['leiden', 'statistic']
    assert list(frame.columns) == [(lv, st) for lv in levels for st in STATISTICS]            # level-major
    assert STATISTICS == ['r', 'null_mean', 'null_sd', 'z', 'p', 'q']
    for i, lv in enumerate(levels):
        assert np.array_equal(frame[lv].values, table[i].T, equal_nan=True)
    assert frame['solo'].isna().all().all() and frame['none'].isna().all().all()


# ------------------------------------------------------------------ the case of the GPU test
_case = {}


def strata_case():
    """(data, y, batches, covs, E, call): the 'qc' dataset of tests/test_gpu_gene_test.py (3 000 cells x 40 samples, 10
    batches, 2 covariates, one population's cells all from the samples of one batch, which the QC drops) with 70 genes and
    data.obs['cluster']: the generating clusters as strings, NaN on one cell in 29, one cell a level of its own; gene 3 is
    zero inside cluster 'c2'."""
    if not _case:
        from cna_amd import synth
        data, meta = synth.make_dataset(3000, 40, k=15, seed=11, n_batches=10, n_covs=2, builder='cpu')
        cl, b = meta['cluster'], meta['batches'].values
        sid = np.asarray(data.obs['id']).copy()
        target = np.flatnonzero(cl == np.bincount(cl).argmax())
        sid[target] = np.random.RandomState(3).choice(np.flatnonzero(b == 0), size=len(target))
        data.obs['id'] = sid
        lab = np.array(['c%d' % c for c in cl], dtype=object)
        lab[5::29] = np.nan
        lab[1234] = 'solo'
        data.obs['cluster'] = lab
        rs = np.random.RandomState(70)
        E = rs.gamma(2.0, 1.0, (3000, 70)) * (rs.rand(3000, 70) < 0.6)
        E[:, 1] = 0.0
        E[lab == 'c2', 3] = 0.0
        E = E.astype(np.float32).astype(np.float64)               # a float32 upload holds the same values
        _case['v'] = (data, meta['y'], meta['batches'], meta['covs'], E, dict(nsteps=3, Nnull=120, seed=3))
    return _case['v']


def oracle_routes(data, y, batches, covs, E, strat, P, **call):
    """The oracle's association, then both routes restricted to each level of data.obs[strat]: (levels, kept,
    materialised r_all [L, G, 1 + P], sample-space (table, null_r), cells per level).  _oracle_null's recipe
    (tests/test_gpu_gene_test.py), level by level; the observed column is the standardised phenotype."""
    from oracle import cna_oracle as orc
    ref = orc.association(data, y, 'id', batches=batches, covs=covs, mode='f64', **call)
    kept = np.asarray(ref['kept'], dtype=bool)
    codes, levels = pd.factorize(data.obs[strat])
    L = len(levels)
    Z = ref['M'].dot(ref['y_perm'][:, :P])
    Z = Z / Z.std(axis=0, ddof=1)
    ys = np.asarray(y.reindex(ref['sample_labels']).values, dtype=np.float64)
    ys = (ys - ys.mean()) / ys.std()
    Zall = np.column_stack([ys, Z])
    R = np.asarray(ref['namresid'], dtype=np.float64)             # kept cells x samples
    EK, ck = E[kept], codes[kept]
    want = materialised_by_level(EK, R, ck, L, Zall)
    got = level_statistics(level_sums(EK, R, ck, L), Zall, level_constant(EK, ck, L))
    return levels, kept, want, got, np.bincount(ck[ck >= 0], minlength=L)


def cpu_parity():
    if 'parity' not in _case:
        data, y, batches, covs, E, call = strata_case()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            levels, kept, want, (table, null_r), cells = oracle_routes(data, y, batches, covs, E, 'cluster', 120, **call)
        ok = np.isfinite(want[..., 0])
        assert np.array_equal(ok, np.isfinite(table[:, 0]))
        d = max(float(np.max(np.abs(table[:, 0][ok] - want[..., 0][ok]))), float(np.max(np.abs(null_r[ok] - want[..., 1:][ok]))))
        _case['parity'] = (d, levels, kept, want, table, null_r, cells)
    return _case['parity']


def recorded_cpu_diff():
    """the figure in the first line of profiles/gene_test_strata_parity.txt"""
    import re
    first = open(PARITY_FILE).readline()
    return float(re.search(r'max \|dr\| = ([0-9.e+-]+)', first).group(1))


def test_cpu_parity_of_the_gpu_case_and_its_record():
    d, levels, kept, want, table, null_r, cells = cpu_parity()
    print('qc case, %d levels: max |sample space - materialised| = %.3e' % (len(levels), d))
    assert 0 < (~kept).sum() < 3000 and len(levels) >= 10 and levels[-1] != 'solo' and 'solo' in list(levels)
    solo = list(levels).index('solo')
    assert cells[solo] <= 1 and np.isnan(table[solo]).all()
    c2 = list(levels).index('c2')
    assert np.isnan(table[c2, 0, 3]) and np.isnan(table[:, 0, 1]).all() and np.isfinite(table[c2, 0, 4])
    assert d <= CPU_BOUND
    # the record the GPU test takes its tolerance from is this figure (a BLAS that adds in another order moves its last digits)
    assert d / 4 <= recorded_cpu_diff() <= 4 * d, (recorded_cpu_diff(), d)


# ------------------------------------------------------------------ the whole call on a numpy engine
def _stub():
    from fake_engine import FakeEngine
    from test_gene_corr_strata_host import restated_gene_corr_strata

    class StrataStub(FakeEngine):
        """FakeEngine plus numpy restatements of the engine calls gene_test_strata adds to an association."""
        cross_by_launches = 0

        def ensure_expression(self, X):
            self.E = np.asarray(X, dtype=np.float64)

        def gram_held(self):
            return self.gram()

        def cross_by_extra(self):
            return self.__dict__.setdefault('_extra', {})

        def gene_corr_by(self, V, codes, n_bins, want_within=True):
            r, within, n = restated_gene_corr_strata(self.E, V, codes, n_bins)
            return r, (within if want_within else None), n

        # ... and of the calls gene_test adds, for the comparison of the two tools
        cross_launches = 0

        def cross_extra(self):
            return self.__dict__.setdefault('_extra1', {})

        def gene_corr(self, V):
            from test_gene_corr_host import restated_gene_corr
            return restated_gene_corr(self.E, V)

        def expr_cross(self, content=None):
            from cna_amd._ffi import MAT_X
            self.cross_launches += 1
            xrow = self.x_row_of_cells()
            X = self.fetch_matrix(MAT_X)
            k = xrow >= 0
            EK, XK = self.E[k], X[xrow[k]]
            return EK.T @ XK, XK.sum(axis=0), EK.sum(axis=0), (EK * EK).sum(axis=0), int(k.sum())

        def expr_cross_by(self, codes, n_bins, bins=None, content=None, xrow=None):
            from cna_amd._ffi import MAT_X
            self.cross_by_launches += 1
            xrow = self.x_row_of_cells()
            X = self.fetch_matrix(MAT_X)                       # rows in device order
            k = xrow >= 0
            return level_sums(self.E[k], X[xrow[k]], np.asarray(codes)[k], n_bins)
    return StrataStub(order='random')


@pytest.fixture(scope='module')
def whole():
    import cna_amd as cna
    data, y, batches, covs, E, call = strata_case()
    data.X = E
    data.var = pd.DataFrame(index=pd.Index(['gene%d' % g for g in range(70)]))
    eng = _stub()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        frame, null_r = cna.tl.gene_test_strata(data, y, 'id', 'cluster', batches=batches, covs=covs, return_null=True,
                                                engine=eng, **call)
        plain = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'])
        p0 = cna.tl.association(plain, y, 'id', batches=batches, covs=covs, engine=_stub(), **call)
    return data, frame, null_r, plain, p0, eng


def test_whole_call_against_the_materialised_oracle(whole):
    data, frame, null_r, plain, p0, eng = whole
    d, levels, kept, want, table, nr, cells = cpu_parity()
    L = len(levels)
    assert 'gene_test_strata' in __import__('cna_amd').tl.__all__
    assert eng.cross_by_launches == 1 and eng.perm is not None
    # levels in order of first appearance, NaN left out; level-major columns; the gene index
    seen = list(dict.fromkeys(v for v in data.obs['cluster'] if isinstance(v, str)))
    assert list(frame.columns.levels[0].reindex(frame.columns.get_level_values(0).unique())[0]) == seen == list(levels)
    assert list(frame.columns) == [(lv, st) for lv in seen for st in STATISTICS] and frame.columns.names == ['cluster', 'statistic']
    assert list(frame.index) == list(data.var_names) and (frame.dtypes == np.float64).all()
    assert null_r.shape == (L, 70, 120) and null_r.dtype == np.float64
    # attrs
    assert frame.attrs['p'] == p0 and frame.attrs['n_null'] == 120
    assert list(frame.attrs['n_cells'].index) == seen and np.array_equal(frame.attrs['n_cells'].values, cells)
    # data.obs as a plain call leaves it
    for k in ('coef', 'coef_fdr'):
        assert data.obs[k].values.tobytes() == plain.obs[k].values.tobytes(), k
    got = np.stack([frame[lv].values.T for lv in seen])                       # L x 6 x genes
    ok = np.isfinite(want[..., 0])
    assert np.array_equal(np.isfinite(got[:, 0]), ok)
    assert np.isnan(got[seen.index('solo')]).all() and np.isnan(got[seen.index('c2'), :, 3]).all()
    assert np.max(np.abs(got[:, 0][ok] - want[..., 0][ok])) <= CPU_BOUND
    assert np.max(np.abs(null_r[ok] - want[..., 1:][ok])) <= CPU_BOUND
    # BH per level, from the frame's own p
    for i, lv in enumerate(seen):
        assert np.array_equal(frame[(lv, 'q')].values, benjamini_hochberg(frame[(lv, 'p')].values), equal_nan=True)
        assert np.array_equal(frame[(lv, 'q')].values, restated_bh(frame[(lv, 'p')].values), equal_nan=True)


def test_one_level_of_all_cells_is_gene_test(whole):
    """gene_test_strata takes gene_test's steps up to the cells (the association under _tolerate.no_fdr, the re-draw of the
    null phenotypes, Zall) from tools/_gene_null.py, as gene_test does; what differs is the engine's sums.  With every cell in one level the
    two tools must return the same r, the same null, the same p and q, write the same columns and leave numpy's generator
    in the same place -- with a seed and without."""
    import cna_amd as cna
    data, y, batches, covs, E, call = strata_case()
    for seed in (3, None):
        kw = dict(batches=batches, covs=covs, return_null=True, nsteps=3, Nnull=60, seed=seed)
        d1 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E)
        d2 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E)
        d2.obs['all'] = 'every cell'
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            np.random.seed(11)
            f1, n1 = cna.tl.gene_test(d1, y, 'id', engine=_stub(), **kw)
            after1 = np.random.get_state()
            np.random.seed(11)
            f2, n2 = cna.tl.gene_test_strata(d2, y, 'id', 'all', engine=_stub(), **kw)
            after2 = np.random.get_state()
        assert after1[0] == after2[0] and np.array_equal(after1[1], after2[1]) and after1[2:] == after2[2:]
        for k in ('coef', 'coef_fdr'):
            assert d1.obs[k].values.tobytes() == d2.obs[k].values.tobytes(), k
        g2 = f2['every cell']
        ok = np.isfinite(f1['r'].values)
        assert np.array_equal(np.isfinite(g2['r'].values), ok) and ok.sum() == 69 and n2.shape == (1,) + n1.shape
        # the same phenotypes, the same null: what is left is the rounding of the sums (the stubs' Gram matrices are formed
        # in different orders), far below the spacing 1 / 61 of the p-values
        assert np.allclose(n2[0], n1, rtol=0, atol=1e-12, equal_nan=True)
        for c in STATISTICS:
            assert np.allclose(g2[c].values, f1[c].values, rtol=0, atol=1e-9, equal_nan=True), c
        assert f1.attrs['p'] == f2.attrs['p'] and f1.attrs['n_null'] == f2.attrs['n_null'] == 60


# ------------------------------------------------------------------ argument errors: before anything runs
class _Refuses:
    """An engine nothing may be asked of."""
    nranks = 1

    def __getattr__(self, name):
        raise AssertionError('engine.%s used although the arguments are wrong' % name)


def test_argument_errors_come_before_anything_runs():
    import cna_amd as cna
    from cna_amd import dist, synth
    data, samplem = synth.make_demo_like(n_samples=20, n_genes=30, cells_per_sample=100, seed=3, keep_expression=True)
    y = samplem.iloc[:, 0].astype(float)
    n = len(data.obs)
    data.obs['leiden'] = np.array(['c%d' % (i % 4) for i in range(n)], dtype=object)
    eng = _Refuses()
    with pytest.raises(KeyError):
        cna.tl.gene_test_strata(data, y, 'id', 'missing', engine=eng)
    with pytest.raises(KeyError):
        cna.tl.gene_test_strata(data, y, 'id', 'leiden', layer='missing', engine=eng)
    data.obs['many'] = np.arange(n) % 1025
    with pytest.raises(ValueError, match='1025 levels'):
        cna.tl.gene_test_strata(data, y, 'id', 'many', engine=eng)
    data.obs['none'] = np.full(n, np.nan)
    with pytest.raises(ValueError, match='0 levels'):
        cna.tl.gene_test_strata(data, y, 'id', 'none', engine=eng)
    for name in ('return_full', ):
        with pytest.raises(TypeError):
            cna.tl.gene_test_strata(data, y, 'id', 'leiden', engine=eng, **{name: True})
    part = dist.shard(data, rank=0, nranks=2)
    part.X = data.X[:len(part.obs)]
    with pytest.raises(NotImplementedError, match='sharded data or a multi-rank engine'):
        cna.tl.gene_test_strata(part, y, 'id', 'leiden', engine=eng)
    two = _Refuses()
    two.__dict__['nranks'] = 2
    with pytest.raises(NotImplementedError):
        cna.tl.gene_test_strata(data, y, 'id', 'leiden', engine=two)
    assert 'coef' not in data.obs


def test_the_library_declares_the_entry_points():
    from cna_amd import _ffi
    for name in ('cna_expr_cross_by', 'cna_gram_by'):
        assert name in _ffi.SIGNATURES and hasattr(_ffi.load(), name)


def test_the_memo_of_expr_cross_by():
    """Engine.expr_cross_by's memo on a stand-in for the library: the same key and codes serve the memo; a moved key serves
    it only under an equal, non-empty content word; other codes, other content, another upload or a dropped matrix take the
    passes again; the extra dict goes with the memo; a result beyond the host budget is taken in groups and not kept."""
    import types
    from cna_amd.engine import Engine
    calls = {'cross': [], 'gram': [], 'rho': []}
    e = types.SimpleNamespace(nranks=1, view_local=False, h=None, x_epoch=1, _cross_by_memo=None, cross_by_launches=0, gen=1,
                              uploads=1, x_rows_total=6, CROSS_BY_HOST_BYTES=Engine.CROSS_BY_HOST_BYTES)
    e.expression_shape = lambda: dict(format='dense', uploads=e.uploads, n_genes=3)
    e.x_generation = lambda: e.gen
    e.matrix_shape = lambda which: (6, 2)
    e.x_row_of_cells = lambda: np.arange(6)

    def raw(xrow, codes, n_bins, bin0=0, nb=None):
        calls['cross'].append((n_bins, bin0, nb))
        return np.zeros((nb, 3, 2)), np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros(nb, dtype=np.int64)

    def gram(xrow, codes, n_bins):
        calls['gram'].append(n_bins)
        return np.zeros((n_bins, 2, 2)), np.zeros(n_bins, dtype=np.int64)

    def rows_to_bins(which, codes, W, n_bins):
        calls['rho'].append(n_bins)
        return np.zeros((1, n_bins, 2)), np.zeros((1, n_bins), dtype=np.int64)
    e.expr_cross_by_raw, e.gram_by, e.matrix_rows_to_bins = raw, gram, rows_to_bins
    by = types.MethodType(Engine.expr_cross_by, e)
    extra = types.MethodType(Engine.cross_by_extra, e)
    codes = np.array([0, 1, 2, 2, -1, 0], dtype=np.int32)
    a = by(codes, 3, content=('A',))
    extra()['constant'] = 'kept'
    assert [x.shape for x in a] == [(3, 3, 2), (3, 2), (3, 3), (3, 3), (3,), (3, 2, 2)]
    assert by(codes, 3, content=('A',)) is a and by(codes, 3) is a and e.cross_by_launches == 1
    assert [x.shape[0] for x in by(codes, 3, bins=[2, 0])] == [2] * 6 and e.cross_by_launches == 1
    e.x_epoch, e.gen = 2, 5                                    # a further association: X rebuilt
    assert by(codes, 3, content=('A',)) is a and e.cross_by_launches == 1 and extra() == {'constant': 'kept'}
    other = codes.copy()
    other[0] = 1
    b = by(other, 3, content=('A',))                           # another clustering
    assert b is not a and e.cross_by_launches == 2 and extra() == {}
    assert by(other, 4, content=('A',)) is not b and e.cross_by_launches == 3          # ... or another number of levels
    e.x_epoch = 3
    by(other, 4, content=('B',))                               # other covariates: other content
    assert e.cross_by_launches == 4
    e.x_epoch = 4
    by(other, 4, content=None)                                 # nothing vouches for the rebuilt X
    assert e.cross_by_launches == 5
    e.uploads = 2                                              # another expression matrix
    by(other, 4, content=None)
    assert e.cross_by_launches == 6
    by(other, 4, xrow=np.arange(6))                            # an explicit map: neither read nor written
    assert e.cross_by_launches == 7 and by(other, 4) is not None and e.cross_by_launches == 7
    # beyond the host budget: groups of levels, the requested ones only, no memo
    e.CROSS_BY_HOST_BYTES = 8 * 3 * 2 * 2                      # two levels of W (and six of Gamma) per group
    for k in calls:
        del calls[k][:]
    out = by(codes, 3)
    assert calls['cross'] == [(3, 0, 2), (3, 2, 1)] and calls['gram'] == [3] and e._cross_by_memo is None
    assert [x.shape[0] for x in out] == [3] * 6
    out = by(codes, 3, bins=[2])
    assert calls['cross'][-1] == (1, 0, 1) and [x.shape[0] for x in out] == [1] * 6 and extra() == {}
