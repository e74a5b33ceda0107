"""cna.tl.gene_rank_corr_strata on the CPU: the numpy / scipy restatement of cna_gene_rank_corr_by (per level, the restatement
of cna_gene_rank_corr on the level's cells: what the GPU tests compare the device with, integer for integer), its check
against scipy.stats.spearmanr per (level, key, gene) on the GPU tests' own inputs, the public call against an engine double,
and the proofs, without a device, that those inputs reach what they are meant to reach: inside ONE level a tie run of a gene
and of a key that ends on a cut of the kernels' unit and one that spans two, a value shared by the last entry of a level and
the first of the next, a (gene, level) without a stored entry, levels of 0, 1 and 2 kept cells, a level that loses cells to a
non-finite key, two tiles of genes under the small budget and three sort chunks.  The constants of csrc/rank_sort.h and
csrc/expr_rankcorr.hip are read from the source."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import scipy.stats

from test_gene_corr_host import GeneEngine, _frame
from test_gene_markers_host import (FORMS, N_CORE, RUN_ON_CUT, RUN_OVER_CUTS, SMALL_WORK_BYTES, _dense, core_codes, core_input,
                                    core_values, markers_input, ranksum_constant, sort_chunks)
from test_gene_rank_corr_host import (KEY_RUN_ON_CUT, KEY_RUN_OVER_CUTS, RHO_TOL, assert_matches_scipy, core_keys, core_kept,
                                      end_to_end_keys, limbs, rank_corr_tiles, restated_rank_corr, spearman_table)

STRATA_LEVELS = 9
# what the levels of strata_codes() are for
BIG, REST, ALL_LOST, TOP_A, TOP_B, ONE, TWO, LOSES, EMPTY = range(STRATA_LEVELS)


# ------------------------------------------------------------------ the restatement
def restated_rank_corr_by(X, V, codes, L):
    """(S object[L, q, G], tie_gene float64[L, G], tie_key float64[L, q], m int64[L], nan bool[G]) of cna_gene_rank_corr_by:
    restated_rank_corr on the cells of every level.  A gene flagged in any level is flagged: callers compare the others."""
    Xd = _dense(X)
    V = np.atleast_2d(np.asarray(V, dtype=np.float64))
    codes = np.asarray(codes)
    q, G = V.shape[0], Xd.shape[1]
    S = np.zeros((L, q, G), dtype=object)
    tie_gene, tie_key, m, nan = np.zeros((L, G)), np.zeros((L, q)), np.zeros(L, dtype=np.int64), np.zeros(G, dtype=bool)
    for l in range(L):
        cells = np.flatnonzero(codes == l)
        S[l], tie_gene[l], tie_key[l], m[l], flagged = restated_rank_corr(Xd[cells], V[:, cells])
        nan |= flagged
    return S, tie_gene, tie_key, m, nan


def as_engine_by(restated):
    """the restatement in the shape Engine.gene_rank_corr_by returns"""
    S, tie_gene, tie_key, m, nan = restated
    lo, hi = zip(*[limbs(S[l]) for l in range(S.shape[0])])
    return np.stack(lo), np.stack(hi), tie_gene, tie_key, m, nan


# ------------------------------------------------------------------ the GPU tests' inputs
@functools.lru_cache(maxsize=None)
def strata_codes():
    """int32 [3001] for the nine core genes and core_keys(): nine levels whose kept cells (every key finite) are
      BIG       every kept cell that gene 4 stores, and every one where key 1 is -3.0 or -1.0: the tie runs that meet the cuts
                of the unit lie inside this one level, in its own positions
      REST      the other kept cells, and 40 cells whose keys are all NaN
      ALL_LOST  two cells where key 0 is not finite: cells but no kept cell
      TOP_A, TOP_B   40 and 30 cells where key 1 is 7.0, its largest value: the last entry of one and the first of the next tie
      ONE, TWO  one and two kept cells
      LOSES     twelve kept cells and the three other cells where key 0 is not finite
      EMPTY     no cell at all
    the cells with core_codes() < 0 are left out by their code, but for those 40."""
    Vg, Sg = core_values()
    V = core_keys()
    kept = core_kept()
    codes = np.full(N_CORE, -1, dtype=np.int32)
    big = kept & (Sg[:, 4] | (V[1] <= -1.0))
    codes[big] = BIG
    rest = np.flatnonzero(kept & ~big)
    top = rest[V[1, rest] == 7.0]
    assert len(top) >= 70
    codes[rest] = REST
    codes[top[:40]] = TOP_A
    codes[top[40:70]] = TOP_B
    other = rest[V[1, rest] != 7.0]
    codes[other[0]] = ONE
    codes[other[[1, 200]]] = TWO
    codes[other[300:312]] = LOSES
    own = np.flatnonzero((core_codes() >= 0) & ~np.isfinite(V[0]))
    assert len(own) == 5
    codes[own[:2]] = ALL_LOST
    codes[own[2:]] = LOSES
    codes[np.flatnonzero(core_codes() < 0)[:40]] = REST
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def strata_reference(form, q=3):
    """One restatement per stored type and key count: the sparse and the dense upload of one type hold the same values."""
    Vg, _ = core_values()
    out = restated_rank_corr_by(Vg.astype(np.float32 if form.endswith('f32') else np.float64), core_keys(q), strata_codes(),
                                STRATA_LEVELS)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def strata_kept():
    """int [3001]: the level of a kept cell, -1 for the others"""
    return np.where(core_kept(), strata_codes(), -1)


def many_codes(L):
    """3001 cells in L levels of unequal size, some empty"""
    rs = np.random.RandomState(41)
    codes = (rs.randint(0, L, size=N_CORE) * rs.randint(1, 4, size=N_CORE) % L).astype(np.int32)
    codes[rs.rand(N_CORE) < 0.03] = -1
    codes[codes == 5] = 6
    return codes


def strata_labels(n):
    """a clustering of markers_input()'s 600 cells: three levels, one of three cells, some cells in none"""
    rs = np.random.RandomState(17)
    lab = np.array(['c0', 'c1'], dtype=object)[rs.choice(2, size=n, p=[0.6, 0.4])]
    lab[rs.rand(n) < 0.05] = None
    lab[[10, 20, 30]] = 'tiny'
    return lab


# ------------------------------------------------------------------ the restatement against scipy
def assert_levels_match_scipy(ref, Xd, V, codes, L):
    """per level: rank_corr_statistics on the level's integers against scipy.stats.spearmanr on the level's cells"""
    from cna_amd.tools._gene_rank_corr import rank_corr_statistics
    S, tie_gene, tie_key, m, _ = ref
    checked = 0
    for l in range(L):
        cells = np.flatnonzero(codes == l)
        table = spearman_table(np.asarray(Xd)[cells], V[:, cells])
        flagged = np.isnan(np.asarray(Xd, dtype=np.float64)[cells][np.isfinite(V[:, cells]).all(axis=0)]).any(axis=0)
        level = (S[l], tie_gene[l], tie_key[l], int(m[l]), flagged)
        if table:
            assert_matches_scipy(level, table)
            checked += len(table)
        else:
            lo, hi = limbs(S[l])
            assert np.isnan(rank_corr_statistics(lo, hi, tie_gene[l], tie_key[l], int(m[l]), flagged)).all()
    return checked


@pytest.mark.parametrize('form', ['dense-f32', 'dense-f64'])
def test_restatement_is_spearmanr_inside_every_level_of_the_core_input(form):
    ref = strata_reference(form)
    codes, V = strata_codes(), core_keys()
    kept = strata_kept()
    assert list(ref[3]) == [int((kept == l).sum()) for l in range(STRATA_LEVELS)] and list(np.flatnonzero(ref[4])) == [7]
    assert assert_levels_match_scipy(ref, core_input(form), V, codes, STRATA_LEVELS) > 40
    # a level is ranked on its own: its m, and S of an increasing transform (gene 1 and key 2) is the level's (m^3 - m) / 3
    for l in (BIG, REST, TOP_A, LOSES, TWO):
        m = int(ref[3][l])
        assert ref[0][l, 2, 1] == (m ** 3 - m) // 3 and ref[1][l, 1] == 0.0 and ref[2][l, 2] == 0.0
    assert ref[0][ONE, 2, 1] == 0 and (ref[0][ALL_LOST] == 0).all() and (ref[0][EMPTY] == 0).all()


def test_restatement_on_the_other_inputs():
    for q in (1, 16):
        ref = strata_reference('dense-f64', q)
        assert ref[0].shape == (STRATA_LEVELS, q, 9) and list(ref[3]) == list(strata_reference('dense-f64')[3])
        assert assert_levels_match_scipy(ref, core_input('dense-f64'), core_keys(q), strata_codes(), STRATA_LEVELS) > 10 * q
    codes = many_codes(255)
    ref = restated_rank_corr_by(core_input('dense-f32'), core_keys(), codes, 255)
    assert (ref[3] == 0).any() and (ref[3] > 20).any() and ref[3][254] > 0
    assert assert_levels_match_scipy(ref, core_input('dense-f32'), core_keys(), codes, 255) > 255
    d = markers_input()
    coef, score = end_to_end_keys(len(d.obs))
    lab = strata_labels(len(d.obs))
    codes = np.array([{'c0': 0, 'c1': 1, 'tiny': 2}.get(v, -1) for v in lab])
    ref = restated_rank_corr_by(d.X, np.stack([coef, score]), codes, 3)
    assert ref[3][2] <= 3 and ref[3][0] > 100
    assert assert_levels_match_scipy(ref, d.X, np.stack([coef, score]), codes, 3) >= 24


def test_level_equals_the_masked_whole_call():
    """the identity the device is held to: level l is cna_gene_rank_corr with the keys set to NaN outside level l"""
    X, V, codes = core_input('dense-f32'), core_keys(), strata_codes()
    ref = strata_reference('dense-f32')
    for l in range(STRATA_LEVELS):
        S, tie_gene, tie_key, m, nan = restated_rank_corr(X, np.where(codes == l, V, np.nan))
        ok = ~nan
        assert m == ref[3][l] and (S[:, ok] == ref[0][l][:, ok]).all()
        np.testing.assert_array_equal(tie_gene[ok], ref[1][l][ok])
        np.testing.assert_array_equal(tie_key, ref[2][l])


# ------------------------------------------------------------------ proofs about the GPU inputs
def _runs(col):
    heads = np.flatnonzero(np.r_[True, col[1:] != col[:-1]])
    return {float(col[h]): (int(h), int(e)) for h, e in zip(heads, np.r_[heads[1:], len(col)])}


@pytest.mark.parametrize('form', FORMS)
def test_tie_runs_inside_one_level_meet_the_cuts_of_the_unit(form):
    """k_rc_corr walks the sub-segment of (gene 4, BIG) and k_rc_keyrank ranks key 1 inside BIG, RS_UNIT at a time from the
    level's first entry: in those positions the run of the smallest value ends exactly on a cut with another value behind
    it, and the run of -1.0 spans two cuts."""
    unit = ranksum_constant('RS_UNIT')
    Vg, Sg = core_values()
    level = strata_kept() == BIG
    assert RUN_ON_CUT == KEY_RUN_ON_CUT == unit and min(RUN_OVER_CUTS, KEY_RUN_OVER_CUTS) > 2 * unit
    use = level if form.startswith('dense') else level & Sg[:, 4]
    col = np.sort(Vg[use, 4].astype(np.float32 if form.endswith('f32') else np.float64))
    key = np.sort(core_keys()[1][level] + 0.0)
    assert len(col) > 2 * unit and len(key) > 2 * unit
    for runs, n in ((_runs(col), len(col)), (_runs(key), len(key))):
        lo, hi = runs[min(runs)]
        assert lo == 0 and hi == unit and hi < n
        lo, hi = runs[-1.0]
        assert lo == unit and len([c for c in range(unit, n, unit) if lo < c < hi]) >= 2
    # BIG is the first level, but not the whole list: the same walk from a later start is the levels behind it
    assert int((strata_kept() == REST).sum()) > 2 * unit


def test_a_value_is_shared_across_the_boundary_of_two_levels():
    """level-major and sorted inside a level: the last entry of TOP_A and the first of TOP_B hold the same value, in gene 2
    (every cell, constant) and in key 1 (its largest value): a run that must break where the level does"""
    Vg, Sg = core_values()
    kept = strata_kept()
    a, b = kept == TOP_A, kept == TOP_B
    assert a.sum() == 40 and b.sum() == 30 and TOP_B == TOP_A + 1
    assert Sg[:, 2].all() and Vg[a, 2].max() == Vg[b, 2].min()
    key = core_keys()[1]
    assert key[a].max() == key[b].min() == 7.0
    # and a gene that is not constant there: gene 3's small integers
    assert Vg[a, 3].max() > Vg[a, 3].min() and Vg[kept == BIG, 3].max() == 3.0 and Vg[kept == REST, 3].max() == 3.0


def test_small_levels_lost_cells_and_empty_sub_segments():
    Vg, Sg = core_values()
    codes, kept = strata_codes(), strata_kept()
    size = [int((kept == l).sum()) for l in range(STRATA_LEVELS)]
    assert (size[ALL_LOST], size[EMPTY], size[ONE], size[TWO]) == (0, 0, 1, 2)
    assert int((codes == ALL_LOST).sum()) == 2 and int((codes == EMPTY).sum()) == 0
    assert int((codes == LOSES).sum()) == 15 and size[LOSES] == 12         # a level that loses cells to a non-finite key
    assert int((codes == REST).sum()) == size[REST] + 40
    # sparse (gene, level) pairs without a stored entry: gene 0 everywhere, gene 4 outside BIG, gene 5 (its one entry left out)
    assert not Sg[:, 0].any() and not Sg[kept == REST, 4].any() and not Sg[kept >= 0, 5].any() and Sg[:, 5].sum() == 1
    assert Sg[kept == BIG, 4].sum() > 0


@pytest.mark.parametrize('form', FORMS)
def test_the_small_budget_cuts_two_tiles_and_the_sort_three_chunks(form):
    tiles, limit, length, cols = rank_corr_tiles(form, SMALL_WORK_BYTES)
    assert len(tiles) >= 2 and cols == 1
    if form.startswith('cs'):
        assert tiles[0] == (0, 1) and length[0] == 0        # a tile without an entry: no pass runs, every level is empty
    chunks, _ = sort_chunks(form)
    assert chunks[1] >= 3 and chunks[2] >= 3
    dense = ranksum_constant('RS_DENSE_CHUNK')
    assert -(-N_CORE // dense) >= 3 and N_CORE % dense != 0                  # a key: a segment of n entries in such chunks


# ------------------------------------------------------------------ the public call
class StrataRankEngine(GeneEngine):
    """GeneEngine (the real residency code, counted uploads) with the device call as numpy."""

    def gene_rank_corr_by(self, V, codes, n_levels, work_bytes=0):
        assert self.resident is not None
        return as_engine_by(restated_rank_corr_by(self.resident, V, codes, n_levels))


def _strata_data():
    d = markers_input()
    n = len(d.obs)
    d.obs['coef'], d.obs['score'] = end_to_end_keys(n)
    d.obs['cluster'] = strata_labels(n)
    d.var = pd.DataFrame(index=pd.Index(['g%d' % i for i in range(6)]))
    return d


def check_against_spearmanr(d, frame, keys, columns_of):
    """every column of the frame against scipy on the level's kept cells; -> the (key, level) pairs checked"""
    lab = d.obs['cluster'].values
    kept = np.all([np.isfinite(d.obs[k].values) for k in keys], axis=0)
    Xd = d.X.astype(np.float64)
    levels = [v for v in pd.unique(lab) if v is not None and v == v]
    assert list(frame.attrs['n_cells'].index) == levels
    for lev in levels:
        cells = kept & (lab == lev)
        assert frame.attrs['n_cells'][lev] == int(cells.sum())
        for k in keys:
            col = frame[columns_of(k, lev)].values
            for g in range(6):
                x, v = Xd[cells, g], d.obs[k].values[cells]
                if cells.sum() < 2 or np.ptp(x) == 0 or np.ptp(v) == 0:
                    assert np.isnan(col[g])
                else:
                    want = scipy.stats.spearmanr(x, v).statistic
                    print('%s %s gene %d: rho %.12f scipy %.12f' % (k, lev, g, col[g], want))
                    assert abs(col[g] - want) <= RHO_TOL
    return levels


def test_gene_rank_corr_strata_through_the_public_call():
    import cna_amd as cna
    assert 'gene_rank_corr_strata' in cna.tl.__all__
    d, eng = _strata_data(), StrataRankEngine()
    one = cna.tl.gene_rank_corr_strata(d, 'cluster', engine=eng)              # keys='coef'
    assert isinstance(one, pd.DataFrame) and one.shape == (6, 3) and (one.dtypes == np.float64).all()
    assert one.index.equals(d.var_names) and one.columns.name == 'cluster' and not isinstance(one.columns, pd.MultiIndex)
    levels = check_against_spearmanr(d, one, ['coef'], lambda k, lev: lev)
    assert list(one.columns) == levels and 'tiny' in levels
    n_cells = one.attrs['n_cells']
    assert isinstance(n_cells, pd.Series) and n_cells.dtype == np.int64 and n_cells.index.name == 'cluster'
    both = cna.tl.gene_rank_corr_strata(d, 'cluster', ['coef', 'score'], engine=eng)
    assert both.shape == (6, 6) and isinstance(both.columns, pd.MultiIndex) and both.columns.names == ['key', 'cluster']
    assert list(both.columns) == [(k, lev) for k in ('coef', 'score') for lev in levels]     # key-major
    check_against_spearmanr(d, both, ['coef', 'score'], lambda k, lev: (k, lev))
    assert (both.attrs['n_cells'].values <= n_cells.values).all() and both.attrs['n_cells'].sum() == n_cells.sum() - 1
    # a list of one key is a list
    assert list(cna.tl.gene_rank_corr_strata(d, 'cluster', ['coef'], engine=eng).columns) == [('coef', lev) for lev in levels]
    # invariant to monotone normalisations of the matrix and of a key
    d.layers['log'] = np.ascontiguousarray(np.log1p(d.X - d.X.min()) * 3.0)
    d.obs['cube'] = d.obs['coef'].values ** 3
    logged = cna.tl.gene_rank_corr_strata(d, 'cluster', ['cube', 'score'], layer='log', engine=eng)
    np.testing.assert_array_equal(logged['cube'].values, both['coef'].values)
    np.testing.assert_array_equal(logged['score'].values, both['score'].values)
    assert len(eng.uploads) == 2                                              # X once, the layer once
    bare = _frame(len(d.obs), X=d.X, coef=d.obs['coef'].values, cluster=d.obs['cluster'].values)
    out = cna.tl.gene_rank_corr_strata(bare, 'cluster', 'coef', engine=eng)
    assert isinstance(out.index, pd.RangeIndex)
    np.testing.assert_array_equal(out.values, one.values)


def test_nan_rules():
    import cna_amd as cna
    Vg, _ = core_values()
    V = core_keys()
    names = ['l%d' % c if c >= 0 else None for c in strata_codes()]
    d = _frame(N_CORE, X=np.ascontiguousarray(Vg), k0=V[0], k1=V[1], k2=V[2], level=np.array(names, dtype=object))
    out = cna.tl.gene_rank_corr_strata(d, 'level', ['k0', 'k1', 'k2'], engine=StrataRankEngine())
    order = [int(v[1:]) for v in pd.unique(np.array([v for v in names if v is not None], dtype=object))]
    assert sorted(order) == [l for l in range(STRATA_LEVELS) if l != EMPTY] and out.shape == (9, 3 * 8)
    m = out.attrs['n_cells']
    kept = strata_kept()
    assert [int(m['l%d' % l]) for l in order] == [int((kept == l).sum()) for l in order]
    for k in ('k0', 'k1', 'k2'):
        for l in (ALL_LOST, ONE):
            assert np.isnan(out[(k, 'l%d' % l)].values).all()               # m_l < 2
        assert np.isnan(out[(k, 'l%d' % BIG)].values[[0, 2, 5, 7]]).all()   # constant on the level; the flagged gene
        assert np.isfinite(out[(k, 'l%d' % BIG)].values[[1, 3, 4, 6, 8]]).all()
        for l in order:
            assert np.isnan(out[(k, 'l%d' % l)].values[7])                  # flagged once, NaN in every level
        assert np.isnan(out[(k, 'l%d' % REST)].values[4])                   # a sparse gene without an entry in the level
    for l in (TOP_A, TOP_B):
        assert np.isnan(out[('k1', 'l%d' % l)].values).all()                # a key that is constant on the level
        assert np.isfinite(out[('k0', 'l%d' % l)].values[[1, 3]]).all()
    assert out[('k2', 'l%d' % REST)].iloc[1] == 1.0 and out[('k2', 'l%d' % TWO)].iloc[1] == 1.0


def test_bad_arguments_and_refusals():
    import cna_amd as cna
    from cna_amd import dist, synth
    d, eng = _strata_data(), StrataRankEngine()
    n = len(d.obs)
    d.obs['coef'] = np.arange(n, dtype=float)
    with pytest.raises(KeyError, match='nope'):
        cna.tl.gene_rank_corr_strata(d, 'nope', engine=eng)
    with pytest.raises(KeyError, match='nope'):
        cna.tl.gene_rank_corr_strata(d, 'cluster', ['coef', 'nope'], engine=eng)
    many = _frame(n, X=d.X, cluster=d.obs['cluster'].values, **{'k%d' % j: np.arange(n, dtype=float) * (j + 1) for j in range(17)})
    with pytest.raises(ValueError, match='16'):
        cna.tl.gene_rank_corr_strata(many, 'cluster', ['k%d' % j for j in range(17)], engine=eng)
    with pytest.raises(ValueError):
        cna.tl.gene_rank_corr_strata(d, 'cluster', [], engine=eng)
    d.obs['fine'] = np.arange(n) % 256
    with pytest.raises(ValueError, match='255'):
        cna.tl.gene_rank_corr_strata(d, 'fine', engine=eng)
    with pytest.raises(TypeError, match='not numeric'):
        cna.tl.gene_rank_corr_strata(d, 'cluster', 'pop', engine=eng)
    with pytest.raises(ValueError, match='data.X'):
        cna.tl.gene_rank_corr_strata(_frame(n, coef=np.zeros(n), cluster=d.obs['cluster'].values), 'cluster', engine=eng)
    with pytest.raises(KeyError):
        cna.tl.gene_rank_corr_strata(d, 'cluster', layer='missing', engine=eng)
    with pytest.raises(TypeError):
        cna.tl.gene_rank_corr_strata(_frame(n, X=d.X.astype(np.int32), coef=np.zeros(n), cluster=d.obs['cluster'].values),
                                     'cluster', engine=eng)
    with pytest.raises(NotImplementedError, match='multi-rank'):
        cna.tl.gene_rank_corr_strata(d, 'cluster', engine=StrataRankEngine(nranks=2))
    data, _ = synth.make_demo_like(n_samples=20, n_genes=30, cells_per_sample=100, seed=3, keep_expression=True)
    part = dist.shard(data, rank=0, nranks=2)
    part.X = data.X[:len(part.obs)]
    part.obs['coef'] = 1.0
    part.obs['cluster'] = 'a'
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.gene_rank_corr_strata(part, 'cluster', engine=eng)
    assert eng.uploads == []
    d.obs['fine'] = np.arange(n) % 255
    assert cna.tl.gene_rank_corr_strata(d, 'fine', engine=eng).shape == (6, 255)
    assert cna.tl.gene_rank_corr_strata(many, 'cluster', ['k%d' % j for j in range(16)], engine=eng).shape == (6, 48)


def test_entry_is_declared_and_the_kernel_names_are_unchanged():
    from cna_amd import _ffi
    lib = _ffi.load()
    assert 'cna_gene_rank_corr_by' in _ffi.SIGNATURES and hasattr(lib, 'cna_gene_rank_corr_by') and lib.cna_abi_version() == 1
    assert _ffi.KERNELS[-1] == 'ranksum_pairs'
    assert _ffi.KERNELS_RANK_CORR == ['rankcorr_keys', 'rankcorr_corr']
    names = [lib.cna_kernel_name(k).decode() for k in range(len(_ffi.KERNELS) + len(_ffi.KERNELS_RANK_CORR))]
    assert names == _ffi.KERNELS + _ffi.KERNELS_RANK_CORR and lib.cna_kernel_name(len(names)) == b'?'
    from cna_amd.engine import Engine
    assert callable(Engine.gene_rank_corr_by)
    assert ranksum_constant('RC_MAX_LEVELS') == 255
    from cna_amd.tools import _gene_rank_corr
    assert _gene_rank_corr.MAX_LEVELS == 255
