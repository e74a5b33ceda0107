"""cna.tl.gene_rank_test_strata on the CPU: the numpy / scipy restatement of cna_gene_rank_corr_x_by (the restatement of
cna_gene_rank_corr_by on the restated columns of cna_x_columns, the codes masked by xrow >= 0: what the GPU tests compare the
device with, integer for integer), its check against scipy.stats.spearmanr per (level, column, gene), the proofs, without a
device, that the GPU tests' inputs reach what they are meant to reach, and the public call against an engine double on the
oracle's residualised NAM and null draw.  RHO_TOL is the project's figure for rho against scipy
(tests/test_gene_rank_corr_host.py)."""
import functools
import os
import re
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.stats

from test_gene_markers_host import (FORMS, N_CORE, ROOT, RUN_ON_CUT, RUN_OVER_CUTS, SMALL_WORK_BYTES, core_codes, core_input,
                                    core_values, ranksum_constant, sort_chunks)
from test_gene_rank_corr_host import RHO_TOL, rank_corr_tiles, restated_rank_corr
from test_gene_rank_corr_strata_host import as_engine_by, assert_levels_match_scipy, many_codes, restated_rank_corr_by
from test_gene_rank_perm_host import COLUMN_COUNTS, COLUMN_SAMPLES, X_ROWS, _qc_case, column_case, restated_columns
from test_gene_test_host import restated_bh

PERM_LEVELS = 9
# what the levels of perm_strata_codes() are for
BIG_A, BIG_B, ALL_LOST, TOP_A, TOP_B, ONE, TWO, LOSES, EMPTY = range(PERM_LEVELS)
CASES = [(s, q, integer) for integer in (False, True) for s, q in zip(COLUMN_SAMPLES, COLUMN_COUNTS)]


# ------------------------------------------------------------------ the restatement
def restated_rank_corr_x_by(X, V, xrow, codes, L):
    """(S object[L, q, G], tie_gene float64[L, G], tie_key float64[L, q], m int64[L], nan bool[G]) of cna_gene_rank_corr_x_by for
    the expression matrix X and the columns V = restated_columns(working matrix, xrow, Z): restated_rank_corr_by on them, a
    cell keeping its level only where it has a row."""
    return restated_rank_corr_by(X, V, np.where(np.asarray(xrow) >= 0, np.asarray(codes), -1), L)


# ------------------------------------------------------------------ the GPU tests' inputs
@functools.lru_cache(maxsize=None)
def case_columns(samples, q, integer=False):
    V = restated_columns(*column_case(samples, q, integer))
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def perm_strata_codes(samples, q, integer=False):
    """int32 [3001] for the nine core genes and column_case(samples, q, integer), whose kept cells are those with xrow >= 0:
      BIG_A     exactly RUN_ON_CUT of the kept cells where gene 4 is -1.0 and none where it is -2.0: in the level's own
                positions gene 4's run of -1.0 is [0, 256) and ends on a cut of the unit, another value behind it
      BIG_B     the kept cells where gene 4 is -2.0 and the other kept cells with -1.0: the same tie run of the gene, split
                between the two levels, spans two cuts here; and 40 cells without a row
      (the other cells are dealt between the two by their index)
      ALL_LOST  two cells without a row: cells but no kept cell
      TOP_A, TOP_B   8 and 6 kept cells that hold one value in column 0 (integer: its most frequent value; else any cells):
                the last entry of one level and the first of the next tie in that column
      ONE, TWO  one and two kept cells
      LOSES     twelve kept cells and three without a row
      EMPTY     no cell at all
    The cell of gene 8's NaN and the cells that core_codes() leaves out among gene 4's stored entries are in no level."""
    Vg, Sg = core_values()
    X, xrow, Z = column_case(samples, q, integer)
    col0 = case_columns(samples, q, integer)[0]
    kept = xrow >= 0
    left = core_codes() < 0
    usable = kept & ~(left & Sg[:, 4])
    usable[np.flatnonzero(np.isnan(Vg[:, 8]))] = False
    codes = np.full(N_CORE, -1, dtype=np.int32)
    codes[usable] = np.where(np.arange(N_CORE)[usable] % 2 == 0, BIG_A, BIG_B)
    minus1 = np.flatnonzero(usable & Sg[:, 4] & (Vg[:, 4] == -1.0))
    assert len(minus1) > 2 * RUN_ON_CUT
    codes[minus1[:RUN_ON_CUT]] = BIG_A
    codes[minus1[RUN_ON_CUT:]] = BIG_B
    codes[usable & Sg[:, 4] & (Vg[:, 4] == -2.0)] = BIG_B
    free = usable & ~Sg[:, 4]                              # the small levels: no stored entry of gene 4
    if integer:
        values, counts = np.unique(col0[free], return_counts=True)
        top = np.flatnonzero(free & (col0 == values[np.argmax(counts)]))
    else:
        top = np.flatnonzero(free)
    assert len(top) >= 14
    codes[top[:8]] = TOP_A
    codes[top[8:14]] = TOP_B
    other = np.setdiff1d(np.flatnonzero(free), top[:14])
    codes[other[0]] = ONE
    codes[other[[1, 200]]] = TWO
    codes[other[300:312]] = LOSES
    lost = np.flatnonzero(~kept & ~left)
    codes[lost[:2]] = ALL_LOST
    codes[lost[2:5]] = LOSES
    codes[lost[5:45]] = BIG_B
    codes.setflags(write=False)
    return codes


def kept_levels(samples, q, integer=False):
    """int [3001]: the level of a kept cell, -1 for the others"""
    return np.where(column_case(samples, q, integer)[1] >= 0, perm_strata_codes(samples, q, integer), -1)


@functools.lru_cache(maxsize=None)
def perm_strata_reference(form, samples, q, integer=False):
    """One restatement per stored type and case: the sparse and the dense upload of one type hold the same values."""
    Vg, _ = core_values()
    out = restated_rank_corr_x_by(Vg.astype(np.float32 if form.endswith('f32') else np.float64), case_columns(samples, q, integer),
                                  column_case(samples, q, integer)[1], perm_strata_codes(samples, q, integer), PERM_LEVELS)
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize('samples,q,integer', [(3, 16, False), (33, 17, True)])
def test_restatement_is_spearmanr_inside_every_level(samples, q, integer):
    X, xrow, Z = column_case(samples, q, integer)
    V, codes = case_columns(samples, q, integer), perm_strata_codes(samples, q, integer)
    ref = perm_strata_reference('dense-f32', samples, q, integer)
    kept = kept_levels(samples, q, integer)
    assert ref[0].shape == (PERM_LEVELS, q, 9) and list(ref[3]) == [int((kept == l).sum()) for l in range(PERM_LEVELS)]
    assert set(np.flatnonzero(ref[4])) <= {7}
    # V is NaN exactly where xrow is -1: the mask by xrow and the finite columns name the same cells
    assert np.array_equal(np.isfinite(V).all(axis=0), xrow >= 0)
    assert assert_levels_match_scipy(ref, core_input('dense-f32'), V, np.where(xrow >= 0, codes, -1), PERM_LEVELS) > 10 * q
    assert (ref[0][ALL_LOST] == 0).all() and (ref[0][EMPTY] == 0).all() and (ref[0][ONE] == 0).all()


def test_level_equals_the_masked_whole_call_and_the_group_of_sixteen():
    """the two identities the device is held to: level l is cna_gene_rank_corr_x with xrow set to -1 outside the level, and a
    group of 16 columns is cna_gene_rank_corr_by on those columns"""
    samples, q, integer = 33, 17, True
    X, xrow, Z = column_case(samples, q, integer)
    E, codes = core_input('dense-f32'), perm_strata_codes(samples, q, integer)
    ref = perm_strata_reference('dense-f32', samples, q, integer)
    ok = ~ref[4]
    for l in range(PERM_LEVELS):
        masked = np.where(codes == l, xrow, -1)
        S, tie_gene, tie_key, m, nan = restated_rank_corr(E, restated_columns(X, masked, Z))
        assert m == ref[3][l] and (S[:, ok] == ref[0][l][:, ok]).all()
        np.testing.assert_array_equal(tie_gene[ok], ref[1][l][ok])
        np.testing.assert_array_equal(tie_key, ref[2][l])
    V = case_columns(samples, q, integer)
    for k0 in range(0, q, 16):
        S, tie_gene, tie_key, m, nan = restated_rank_corr_by(E, V[k0:k0 + 16], codes, PERM_LEVELS)
        assert (S[:, :, ok] == ref[0][:, k0:k0 + 16][:, :, ok]).all() and np.array_equal(m, ref[3])
        np.testing.assert_array_equal(tie_key, ref[2][:, k0:k0 + 16])


# ------------------------------------------------------------------ proofs about the GPU inputs
def _runs(col):
    heads = np.flatnonzero(np.r_[True, col[1:] != col[:-1]])
    return {float(col[h]): (int(h), int(e)) for h, e in zip(heads, np.r_[heads[1:], len(col)])}


@pytest.mark.parametrize('samples,q,integer', CASES)
def test_the_codes_reach_the_small_levels_and_the_lost_cells(samples, q, integer):
    Vg, Sg = core_values()
    X, xrow, Z = column_case(samples, q, integer)
    codes, kept = perm_strata_codes(samples, q, integer), kept_levels(samples, q, integer)
    size = [int((kept == l).sum()) for l in range(PERM_LEVELS)]
    assert int((xrow >= 0).sum()) == X_ROWS
    assert (size[ALL_LOST], size[EMPTY], size[ONE], size[TWO]) == (0, 0, 1, 2)
    assert int((codes == EMPTY).sum()) == 0                                    # a level with 0 cells
    assert int((codes == ALL_LOST).sum()) == 2 and (xrow[codes == ALL_LOST] == -1).all()    # cells, every one without a row
    assert int((codes == LOSES).sum()) == 15 and size[LOSES] == 12             # a level that loses some cells to xrow
    assert int((codes == BIG_B).sum()) == size[BIG_B] + 40
    assert (size[TOP_A], size[TOP_B]) == (8, 6) and TOP_B == TOP_A + 1
    # (gene, level) pairs without a stored entry: gene 0 everywhere, gene 4 in every small level
    assert not Sg[:, 0].any() and Sg[kept == BIG_A, 4].any() and Sg[kept == BIG_B, 4].any()
    for l in (TOP_A, TOP_B, ONE, TWO, LOSES):
        assert not Sg[kept == l, 4].any()
    # the whole-gene guard: gene 8's NaN lies in no level; gene 7's does where its cell has a row
    assert (kept[np.isnan(Vg[:, 8])] == -1).all()
    cell7 = int(np.flatnonzero(np.isnan(Vg[:, 7]))[0])
    flagged = perm_strata_reference('dense-f32', samples, q, integer)[4]
    assert list(np.flatnonzero(flagged)) == ([7] if kept[cell7] >= 0 else [])


def test_the_known_flagged_gene():
    """gene 7 is flagged in most cases, so the guard is exercised; where its cell has no row, no gene is"""
    Vg, _ = core_values()
    cell7 = int(np.flatnonzero(np.isnan(Vg[:, 7]))[0])
    hits = [column_case(*c)[1][cell7] >= 0 for c in CASES]
    assert sum(hits) >= len(CASES) // 2


@pytest.mark.parametrize('samples,q', list(zip(COLUMN_SAMPLES, COLUMN_COUNTS)))
def test_a_tie_run_of_a_column_spans_the_boundary_of_two_levels(samples, q):
    """integer columns: level-major and sorted inside a level, the last entry of TOP_A and the first of TOP_B hold the same
    value in column 0, and that value has more cells than the two levels: a run that must end where the level does"""
    kept = kept_levels(samples, q, True)
    col0 = case_columns(samples, q, True)[0]
    a, b = col0[kept == TOP_A], col0[kept == TOP_B]
    assert np.ptp(a) == 0 and np.ptp(b) == 0 and a.max() == b.min()
    assert int((col0[kept >= 0] == a[0]).sum()) > len(a) + len(b)
    if q > 1:                                                                  # and a column that is not constant there
        assert any(np.ptp(c[kept == TOP_A]) > 0 for c in case_columns(samples, q, True)[1:])
    # the genes: gene 2 (every cell, constant) ties across every boundary; gene 3's small integers are not constant in BIG_A
    Vg, Sg = core_values()
    assert Sg[:, 2].all() and np.ptp(Vg[:, 2]) == 0 and np.ptp(Vg[kept == BIG_A, 3]) > 0


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('samples,q,integer', CASES)
def test_two_big_levels_split_a_tie_run_of_a_gene_on_a_cut_of_the_unit(form, samples, q, integer):
    """k_rp_rank walks the sub-segment of (gene 4, level) RS_UNIT at a time from the level's first entry.  Gene 4's run of
    -1.0 (RUN_OVER_CUTS cells of core_values()) is split between BIG_A and BIG_B: in BIG_A's positions it is [0, unit), ends
    exactly on a cut and has another value behind it; in BIG_B's it begins behind the run of -2.0 and spans two cuts."""
    unit = ranksum_constant('RS_UNIT')
    assert RUN_ON_CUT == unit and RUN_OVER_CUTS > 2 * unit
    Vg, Sg = core_values()
    kept = kept_levels(samples, q, integer)
    dtype = np.float32 if form.endswith('f32') else np.float64
    lists = {}
    for level in (BIG_A, BIG_B):
        use = (kept == level) if form.startswith('dense') else (kept == level) & Sg[:, 4]
        lists[level] = np.sort(Vg[use, 4].astype(dtype))
    runs = _runs(lists[BIG_A])
    assert min(runs) == -1.0 and runs[-1.0] == (0, unit) and len(lists[BIG_A]) > unit
    runs = _runs(lists[BIG_B])
    lo, hi = runs[-1.0]
    assert min(runs) == -2.0 and runs[-2.0] == (0, lo) and 0 < lo < unit and hi < len(lists[BIG_B])
    assert len([c for c in range(unit, len(lists[BIG_B]), unit) if lo < c < hi]) >= 2
    assert int((kept == BIG_A).sum()) > 2 * unit and int((kept == BIG_B).sum()) > 2 * unit


def test_the_level_limit_input():
    codes = many_codes(255)
    X, xrow, Z = column_case(3, 16)
    ref = restated_rank_corr_x_by(core_input('dense-f32'), case_columns(3, 16), xrow, codes, 255)
    assert (ref[3] == 0).any() and (ref[3] > 20).any() and ref[3][254] > 0 and ref[3].sum() < X_ROWS
    assert assert_levels_match_scipy(ref, core_input('dense-f32'), case_columns(3, 16), np.where(xrow >= 0, codes, -1), 255) > 255


@pytest.mark.parametrize('form', FORMS)
def test_the_small_budget_cuts_two_tiles_and_the_sort_three_chunks(form):
    tiles, limit, length, cols = rank_corr_tiles(form, SMALL_WORK_BYTES)
    assert len(tiles) >= 2 and cols == 1                   # of genes; and a group of 16 columns goes one column per tile
    chunks, _ = sort_chunks(form)
    assert chunks[1] >= 3 and chunks[2] >= 3
    dense = ranksum_constant('RS_DENSE_CHUNK')
    assert -(-N_CORE // dense) >= 3 and N_CORE % dense != 0                    # a column: a segment of n entries in such chunks


# ------------------------------------------------------------------ the whole call on the numpy engine double
def _double(**kw):
    from fake_engine import FakeEngine
    from cna_amd._ffi import MAT_X

    class StrataRankEngine(FakeEngine):
        """FakeEngine plus numpy restatements of the engine calls gene_rank_test_strata adds to an association."""
        m_shift = None

        def ensure_expression(self, X):
            self.E = np.asarray(X)

        def gene_rank_corr_by(self, V, codes, n_levels, work_bytes=0):
            return as_engine_by(restated_rank_corr_by(self.E, V, codes, n_levels))

        def gene_rank_corr_x_by(self, xrow, Z, codes, n_levels, work_bytes=0):
            self.Z_seen = np.array(Z)
            V = restated_columns(self.fetch_matrix(MAT_X), xrow, Z)        # rows of X in device order: what xrow names
            out = as_engine_by(restated_rank_corr_x_by(self.E, V, xrow, codes, n_levels))
            m = np.array(out[4])
            if self.m_shift is not None:
                m[self.m_shift] += 2
            return out[:4] + (m,) + out[5:]
    return StrataRankEngine(order='random', **kw)


def _labels(n):
    """a clustering of the 3000 cells: three levels in order of first appearance, one of three cells (one of them in no
    kept set if the QC dropped it), one of one cell, some cells in none"""
    rs = np.random.RandomState(23)
    lab = np.array(['c1', 'c0'], dtype=object)[rs.choice(2, size=n, p=[0.35, 0.65])]
    lab[rs.rand(n) < 0.05] = None
    lab[[10, 20, 30]] = 'tiny'
    lab[40] = 'single'
    return lab


def _data():
    data, meta, call, ref, E = _qc_case()
    d = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E)
    d.obs['cluster'] = _labels(len(d.obs))
    return d


def _run(eng, **kw):
    import cna_amd as cna
    data, meta, call, ref, E = _qc_case()
    d = _data()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = cna.tl.gene_rank_test_strata(d, meta['y'], 'id', 'cluster', batches=meta['batches'], covs=meta['covs'], engine=eng,
                                           **call, **kw)
    return d, out


def test_whole_call_against_spearmanr_on_the_oracle():
    import cna_amd as cna
    data, meta, call, ref, E = _qc_case()
    eng = _double()
    d, (frame, null_rho) = _run(eng, return_null=True)
    kept = ref['kept']
    lab = d.obs['cluster'].values
    levels = [v for v in pd.unique(lab) if v is not None and v == v]
    assert set(levels) == {'c0', 'c1', 'tiny', 'single'} and len(levels) == 4
    stats = ['rho', 'null_mean', 'null_sd', 'z', 'p', 'q']
    assert isinstance(frame.columns, pd.MultiIndex) and frame.columns.names == ['cluster', 'statistic']
    assert list(frame.columns) == [(lev, s) for lev in levels for s in stats]                # level-major
    assert frame.shape == (20, 24) and (frame.dtypes == np.float64).all() and null_rho.shape == (4, 20, 60)
    assert null_rho.dtype == np.float64
    n_cells = frame.attrs['n_cells']
    assert frame.attrs['n_null'] == 60 and frame.attrs['p'] == ref['p']
    assert isinstance(n_cells, pd.Series) and n_cells.dtype == np.int64 and list(n_cells.index) == levels
    assert n_cells.index.name == 'cluster'
    assert [int(n_cells[lev]) for lev in levels] == [int((kept & (lab == lev)).sum()) for lev in levels]
    assert int(n_cells['single']) <= 1 and int(n_cells['tiny']) <= 3 and int(n_cells['c0']) > 1000
    # rho: gene_rank_corr_strata on the stored coefficient, bit for bit
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        plain = cna.tl.gene_rank_corr_strata(d, 'cluster', 'coef', engine=eng)
    assert frame.index.equals(plain.index)
    coef = d.obs['coef'].values
    assert np.array_equal(np.isfinite(coef), kept)
    Z = ref['M'].dot(ref['y_perm'][:, :60])
    Z = Z / Z.std(axis=0, ddof=1)
    assert eng.Z_seen.shape == (60, 40) and np.max(np.abs(eng.Z_seen.T - Z)) <= 1e-12
    Cn = np.full((3000, 60), np.nan)
    Cn[kept] = ref['namresid'].dot(Z)                                  # the null coefficients of the oracle, per cell
    worst_rho = worst_null = 0.0
    for l, lev in enumerate(levels):
        cells = kept & (lab == lev)
        rho = frame[(lev, 'rho')].values
        assert rho.tobytes() == plain[lev].values.tobytes()
        nulls = null_rho[l]
        if cells.sum() < 2:                                            # a level with fewer than two kept cells: NaN throughout
            assert np.isnan(frame[lev].values).all() and np.isnan(nulls).all()
            continue
        # NaN rules: constant on the level's kept cells (genes 1 and 2 everywhere), a NaN in a kept cell of any level (3)
        Ec = E[cells]
        with np.errstate(invalid='ignore'):
            dead = (np.ptp(Ec, axis=0) == 0) | np.isnan(np.ptp(Ec, axis=0))
        dead[3] = True
        assert dead[[1, 2, 3]].all()
        assert np.isnan(frame[lev].values[dead]).all() and np.isnan(nulls[dead]).all()
        assert np.isfinite(rho[~dead]).all() and np.isfinite(nulls[~dead]).all()
        for g in np.flatnonzero(~dead):
            worst_rho = max(worst_rho, abs(rho[g] - scipy.stats.spearmanr(Ec[:, g], coef[cells]).statistic))
            for p in range(60):
                worst_null = max(worst_null, abs(nulls[g, p] - scipy.stats.spearmanr(Ec[:, g], Cn[cells, p]).statistic))
        # p, q and the null moments exactly from the returned arrays: a direct count, Benjamini-Hochberg inside the level
        p = (1.0 + (np.abs(nulls) >= np.abs(rho)[:, None]).sum(axis=1)) / 61.0
        p[dead] = np.nan
        assert np.array_equal(frame[(lev, 'p')].values, p, equal_nan=True)
        assert np.array_equal(frame[(lev, 'q')].values, restated_bh(p), equal_nan=True)
        assert np.array_equal(frame[(lev, 'null_mean')].values[~dead], nulls[~dead].mean(axis=1))
        assert np.array_equal(frame[(lev, 'null_sd')].values[~dead], nulls[~dead].std(axis=1, ddof=1))
        with np.errstate(all='ignore'):
            z = (rho - nulls.mean(axis=1)) / nulls.std(axis=1, ddof=1)
        ok = ~dead & np.isfinite(z)
        assert np.allclose(frame[(lev, 'z')].values[ok], z[ok], rtol=1e-12, atol=0)
    print('rho and null_rho against scipy.stats.spearmanr: max |d rho| = %.3e, %.3e (bound %.0e)' % (worst_rho, worst_null, RHO_TOL))
    assert worst_rho <= RHO_TOL and worst_null <= RHO_TOL
    # the small level is ranked on its own cells: three of them at most, and rho is one of the few values that allows
    if int(n_cells['tiny']) >= 2:
        r = frame[('tiny', 'rho')].values
        assert set(np.round(r[np.isfinite(r)], 12)) <= {-1.0, -0.866025403784, -0.5, 0.0, 0.5, 0.866025403784, 1.0}


def test_without_return_null_the_frame_is_the_same():
    _, (frame, _) = _run(_double(), return_null=True)
    _, alone = _run(_double())
    assert isinstance(alone, pd.DataFrame) and alone.equals(frame) and alone.attrs['n_null'] == 60


def test_n_perm_cuts_the_columns_and_bad_values_are_refused():
    _, (full, null_full) = _run(_double(), return_null=True)
    eng = _double()
    d, (cut, null_cut) = _run(eng, return_null=True, n_perm=16)
    assert null_cut.shape == (4, 20, 16) and cut.attrs['n_null'] == 16 and eng.Z_seen.shape == (16, 40)
    assert null_cut.tobytes() == np.ascontiguousarray(null_full[:, :, :16]).tobytes()
    for lev in ('c0', 'c1', 'tiny'):
        rho = cut[(lev, 'rho')].values
        assert np.array_equal(rho, full[(lev, 'rho')].values, equal_nan=True)
        l = list(cut.attrs['n_cells'].index).index(lev)
        ok = np.isfinite(rho)
        p = (1.0 + (np.abs(null_cut[l]) >= np.abs(rho)[:, None]).sum(axis=1)) / 17.0
        assert np.array_equal(cut[(lev, 'p')].values[ok], p[ok])
    _, more = _run(_double(), n_perm=np.int64(5000))                   # more than there are: all of them
    assert more.attrs['n_null'] == 60
    for bad, exc in ((0, ValueError), (-3, ValueError), (2.5, TypeError), ('7', TypeError), (True, TypeError)):
        refuses = _double()
        with pytest.raises(exc, match='gene_rank_test_strata: n_perm'):
            _run(refuses, n_perm=bad)
        assert not hasattr(refuses, 'E')                               # before anything ran


def test_the_m_mismatch_raises_and_names_both_numbers():
    _, _, _, ref, _ = _qc_case()
    lab = _labels(3000)
    eng = _double()
    eng.m_shift = 1                                                    # the second level in order of first appearance
    levels = [v for v in pd.unique(lab) if v is not None]
    m = int((ref['kept'] & (lab == levels[1])).sum())
    with pytest.raises(RuntimeError, match=r'%s.*%d cells.*%d' % (levels[1], m, m + 2)):
        _run(eng)


def test_refusals():
    import cna_amd as cna
    from cna_amd import dist
    from test_gene_test_host import _Refuses
    data, meta, call, ref, E = _qc_case()
    d = _data()
    part = dist.shard(d, rank=0, nranks=2)
    part.X = E[:len(part.obs)]
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.gene_rank_test_strata(part, meta['y'], 'id', 'cluster', engine=_Refuses())
    two = _Refuses()
    two.__dict__['nranks'] = 2
    with pytest.raises(NotImplementedError, match='multi-rank'):
        cna.tl.gene_rank_test_strata(d, meta['y'], 'id', 'cluster', engine=two)
    with pytest.raises(KeyError, match='nope'):                        # an unknown stratification
        cna.tl.gene_rank_test_strata(d, meta['y'], 'id', 'nope', engine=_Refuses())
    d.obs['fine'] = np.arange(len(d.obs)) % 256
    with pytest.raises(ValueError, match='255'):                       # 256 levels
        cna.tl.gene_rank_test_strata(d, meta['y'], 'id', 'fine', engine=_Refuses())
    with pytest.raises(TypeError, match='return_full'):
        cna.tl.gene_rank_test_strata(d, meta['y'], 'id', 'cluster', engine=_Refuses(), return_full=True)
    bare = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'])
    bare.obs['cluster'] = d.obs['cluster'].values
    with pytest.raises(ValueError, match='data.X'):
        cna.tl.gene_rank_test_strata(bare, meta['y'], 'id', 'cluster', engine=_Refuses())
    assert 'coef' not in d.obs


def test_strata_frame_keeps_its_default_statistics():
    from cna_amd.tools._gene_test_strata import STATISTICS, strata_frame
    table = np.arange(2 * 6 * 3, dtype=np.float64).reshape(2, 6, 3)
    index = pd.Index(['a', 'b', 'c'])
    old = strata_frame(table, ['x', 'y'], 'leiden', index)
    assert list(old.columns) == [(lev, s) for lev in ('x', 'y') for s in STATISTICS] and STATISTICS[0] == 'r'
    new = strata_frame(table, ['x', 'y'], 'leiden', index, statistics=['rho'] + STATISTICS[1:])
    assert list(new.columns.get_level_values(1)[:6]) == ['rho', 'null_mean', 'null_sd', 'z', 'p', 'q']
    assert np.array_equal(new.values, old.values) and new[('y', 'rho')].tolist() == [18.0, 19.0, 20.0]


# ------------------------------------------------------------------ the library's side
def test_the_entry_is_declared_and_the_kernel_names_are_unchanged():
    import cna_amd as cna
    from cna_amd import _ffi
    from cna_amd import engine as engine_module
    from cna_amd.engine import Engine
    text = open(os.path.join(ROOT, 'include', 'cna_hip.h')).read()
    lib = _ffi.load()
    name = 'cna_gene_rank_corr_x_by'
    assert name in _ffi.SIGNATURES and hasattr(lib, name) and lib.cna_abi_version() == 1
    assert re.search(r'\bint\s+%s\(cna_ctx\* ctx' % name, text)
    assert callable(Engine.gene_rank_corr_x_by) and engine_module.RANK_X_BY_HOST_BYTES == 1 << 30
    assert 'gene_rank_test_strata' in cna.tl.__all__ and callable(cna.tl.gene_rank_test_strata)
    assert _ffi.KERNELS[-1] == 'ranksum_pairs' and _ffi.KERNELS_RANK_CORR == ['rankcorr_keys', 'rankcorr_corr']
    names = [lib.cna_kernel_name(k).decode() for k in range(len(_ffi.KERNELS) + len(_ffi.KERNELS_RANK_CORR))]
    assert names == _ffi.KERNELS + _ffi.KERNELS_RANK_CORR and lib.cna_kernel_name(len(names)) == b'?'
    # shared, not copied: the two sources of a workgroup's list are defined once, in the header both files include
    csrc = os.path.join(ROOT, 'cna_amd', 'csrc')
    tree = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h'))}
    for struct in ('struct WholeGene {', 'struct GeneLevel {'):
        assert [f for f, src in tree.items() if struct in src] == ['rank_corr.h'], struct
    src = tree['expr_rankperm.hip']
    assert 'k_rp_codes_by' in src and 'GeneLevel{' in src and 'WholeGene{' in src and 'sort_count(' in src


def test_the_engine_chunks_whole_groups_of_sixteen(monkeypatch):
    """Engine.gene_rank_corr_x_by on a stand-in library: the columns go in chunks of whole groups of 16 under the cap, every
    chunk with the same xrow and codes, and the chunks are put back in order"""
    import types
    from cna_amd import engine as engine_module
    from cna_amd.engine import Engine
    calls = []

    class Lib:
        def cna_gene_rank_corr_x_by(self, h, xrow, n, Z, q, codes, L, work_bytes, s_lo, s_hi, tie_gene, tie_key, m, nan):
            calls.append((n, q, L, work_bytes))
            return 0

    G, n, L = 5, 7, 3
    e = types.SimpleNamespace(nranks=1, view_local=False, lib=Lib(), h=None,
                              expression_shape=lambda: {'format': 'csc', 'n_cells': n, 'n_genes': G},
                              matrix_shape=lambda which: (n, 2))
    e._x_columns_args = types.MethodType(Engine._x_columns_args, e)
    call = types.MethodType(Engine.gene_rank_corr_x_by, e)
    xrow, codes = np.arange(n), np.zeros(n, dtype=np.int32)
    out = call(xrow, np.zeros((40, 2)), codes, L)
    assert calls == [(n, 40, L, 0)] and out[0].shape == (L, 40, G) and out[3].shape == (L, 40) and out[4].shape == (L,)
    del calls[:]
    monkeypatch.setattr(engine_module, 'RANK_X_BY_HOST_BYTES', 16 * 16 * L * G)                       # one group per call
    call(xrow, np.zeros((40, 2)), codes, L, work_bytes=9)
    assert calls == [(n, 16, L, 9), (n, 16, L, 9), (n, 8, L, 9)]
    del calls[:]
    monkeypatch.setattr(engine_module, 'RANK_X_BY_HOST_BYTES', 2 * 16 * 16 * L * G + 5)               # two groups per call
    call(xrow, np.zeros((40, 2)), codes, L)
    assert calls == [(n, 32, L, 0), (n, 8, L, 0)]
    del calls[:]
    monkeypatch.setattr(engine_module, 'RANK_X_BY_HOST_BYTES', 1)                                  # below one group: one group at least
    call(xrow, np.zeros((17, 2)), codes, L)
    assert calls == [(n, 16, L, 0), (n, 1, L, 0)]
    with pytest.raises(ValueError):
        call(xrow, np.zeros((3, 2)), codes[:-1], L)
    e.nranks = 2
    with pytest.raises(NotImplementedError):
        call(xrow, np.zeros((3, 2)), codes, L)
