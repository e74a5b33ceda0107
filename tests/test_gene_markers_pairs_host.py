"""cna.tl.gene_markers_pairs on the CPU: the numpy restatement of cna_gene_ranksum_pairs (what the GPU tests compare the
device with, integer for integer), its check against scipy.stats.rankdata / mannwhitneyu on the GPU tests' own inputs and
against the restatement of cna_gene_ranksum_by on recoded codes, the public call against an engine double, its refusals, and
the proof that the GPU inputs still put a tie run on a cut of the kernel's unit and one across two cuts for the levels of a
tested pair.  The inputs are those of tests/test_gene_markers_host.py."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.stats

from test_gene_corr_host import _frame
from test_gene_markers_host import (CORE_LEVELS, N_CORE, P_RTOL, Z_MAX, MarkersEngine, _dense, core_codes, core_values,
                                    markers_input, ranksum_constant, restated_ranksum)

RANK_COLS = ['auc', 'u', 'z', 'p', 'q']
PAIR_STATISTICS = RANK_COLS + ['mean_in', 'mean_vs', 'frac_in', 'frac_vs']
CORE_PAIRS = [(a, b) for a in range(CORE_LEVELS) for b in range(CORE_LEVELS) if a != b]     # 12 ordered; level 3 is empty


# ------------------------------------------------------------------ the restatement
def restated_pairs(X, codes, L, pairs):
    """(u2 int64[P, G], tie float64[P, G], n int64[L], nan bool[G]) of cna_gene_ranksum_pairs: per gene the tie groups of
    the kept column (np.unique on the stored type's values), the groups x levels count matrix c and C = the counts strictly
    below, then 2 U_ab = sum c[a] (2 C[b] + c[b]) and tie_ab = sum t (t^2 - 1), t = c[a] + c[b], in int64 integers.  A gene
    with a NaN in a kept cell is flagged and its numbers are 0, as in restated_ranksum."""
    Xd = _dense(X)
    codes = np.asarray(codes)
    kept = codes >= 0
    lev = codes[kept]
    G, P = Xd.shape[1], len(pairs)
    u2 = np.zeros((P, G), dtype=np.int64)
    tie = np.zeros((P, G))
    nan = np.zeros(G, dtype=bool)
    n = np.bincount(lev, minlength=L).astype(np.int64)
    assert n.sum() < 2 ** 21
    for g in range(G):
        col = Xd[kept, g].astype(np.float64)            # exact from float32: the order and the ties of the stored type
        if np.isnan(col).any():
            nan[g] = True
            continue
        if col.size == 0:
            continue
        _, inv = np.unique(col, return_inverse=True)
        c = np.zeros((int(inv.max()) + 1, L), dtype=np.int64)
        np.add.at(c, (inv.ravel(), lev), 1)
        C = np.cumsum(c, axis=0) - c
        U = c.T @ (2 * C + c)                           # [a, b]; every sum is far below 2^63 at m < 2^21 cells
        T = np.zeros((L, L), dtype=np.int64)
        for a in range(L):
            t = c[:, [a]] + c
            T[a] = (t * (t * t - 1)).sum(axis=0)
        for k, (a, b) in enumerate(pairs):
            u2[k, g] = U[a, b]
            tie[k, g] = float(int(T[a, b]))
    return u2, tie, n, nan


@functools.lru_cache(maxsize=None)
def core_pairs_reference(f64):
    V, _ = core_values()
    out = restated_pairs(V.astype(np.float64 if f64 else np.float32), core_codes(), CORE_LEVELS, CORE_PAIRS)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize('f64', [False, True])
def test_restatement_is_rankdata_and_mannwhitneyu_on_the_core_input(f64):
    V, _ = core_values()
    Xd = V.astype(np.float64 if f64 else np.float32).astype(np.float64)
    codes = core_codes()
    u2, tie, n, nan = core_pairs_reference(f64)
    assert list(np.flatnonzero(nan)) == [7] and n[3] == 0 and (n[:3] > 0).all()
    checked = 0
    for k, (a, b) in enumerate(CORE_PAIRS):
        na, nb = int(n[a]), int(n[b])
        for g in range(9):
            if g == 7:
                continue
            xa, xb = Xd[codes == a, g], Xd[codes == b, g]
            both = np.r_[xa, xb]
            r2 = np.rint(2.0 * scipy.stats.rankdata(both)).astype(np.int64) if both.size else np.zeros(0, dtype=np.int64)
            assert u2[k, g] == int(r2[:na].sum()) - na * (na + 1), (a, b, g)
            t = np.unique(both, return_counts=True)[1]
            assert tie[k, g] == float(sum(int(v) ** 3 - int(v) for v in t)), (a, b, g)
            if na and nb:
                res = scipy.stats.mannwhitneyu(xa, xb, use_continuity=False, method='asymptotic')
                assert u2[k, g] / 2.0 == res.statistic, (a, b, g)
                checked += 1
            else:
                assert u2[k, g] == 0
        back = CORE_PAIRS.index((b, a))
        ok = np.arange(9) != 7
        np.testing.assert_array_equal(u2[k, ok] + u2[back, ok], 2 * na * nb)
    assert checked == 6 * 8


@pytest.mark.parametrize('f64', [False, True])
def test_restatement_is_the_existing_one_on_recoded_codes(f64):
    """what the parent commit offers for one pair: a -> 0, b -> 1, the rest -> -1, one cna_gene_ranksum_by"""
    V, _ = core_values()
    X = V.astype(np.float64 if f64 else np.float32)
    codes = core_codes()
    u2, tie, n, nan = core_pairs_reference(f64)
    ok = ~nan
    for k, (a, b) in enumerate(CORE_PAIRS):
        two = np.where(codes == a, 0, np.where(codes == b, 1, -1)).astype(np.int32)
        rank2, tie1, n1, nan1 = restated_ranksum(X, two, 2)
        assert list(n1) == [n[a], n[b]]
        np.testing.assert_array_equal(rank2[0][ok] - n[a] * (n[a] + 1), u2[k][ok])
        np.testing.assert_array_equal(tie1[ok], tie[k][ok])


# ------------------------------------------------------------------ the public call
class PairsEngine(MarkersEngine):
    """MarkersEngine with `gene_ranksum_pairs` backed by the restatement; records what the tool asked for"""

    def gene_ranksum_pairs(self, codes, n_levels, pairs, work_bytes=0):
        assert self.resident is not None
        pairs = np.asarray(pairs)
        assert pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2
        assert np.asarray(codes).max() < n_levels
        self.asked = (np.array(codes), n_levels, pairs.copy())
        return restated_pairs(self.resident, codes, n_levels, [tuple(p) for p in pairs.tolist()])


def _check_pair_columns(out, d, level, versus):
    lab = d.obs['pop'].astype(object).values
    Xd = d.X.astype(np.float64)
    ins, vs = lab == level, lab == versus
    na, nb = int(ins.sum()), int(vs.sum())
    m = na + nb
    from cna_amd.tools._gene_test import benjamini_hochberg
    col = {s: out[(level, versus, s)].values for s in RANK_COLS}
    for g in range(Xd.shape[1]):
        x, y = Xd[ins, g], Xd[vs, g]
        res = scipy.stats.mannwhitneyu(x, y, use_continuity=False, method='asymptotic')
        t = np.unique(np.r_[x, y], return_counts=True)[1].astype(np.float64)
        sd = np.sqrt(na * nb / 12.0 * ((m + 1) - (t ** 3 - t).sum() / (m * (m - 1.0))))
        z = (res.statistic - na * nb / 2.0) / sd
        got = {s: col[s][g] for s in RANK_COLS}
        assert got['u'] == res.statistic
        assert got['auc'] == res.statistic / (na * nb)
        assert abs(z) < Z_MAX and abs(got['z'] - z) <= 1e-10
        assert abs(got['p'] - res.pvalue) <= P_RTOL * res.pvalue
    np.testing.assert_array_equal(out[(level, versus, 'q')].values, benjamini_hochberg(out[(level, versus, 'p')].values))
    np.testing.assert_allclose(out[(level, versus, 'mean_in')].values, Xd[ins].mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(out[(level, versus, 'mean_vs')].values, Xd[vs].mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(out[(level, versus, 'frac_in')].values, (Xd[ins] > 0).mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(out[(level, versus, 'frac_vs')].values, (Xd[vs] > 0).mean(axis=0), rtol=1e-12)


def test_gene_markers_pairs_through_the_public_call():
    import cna_amd as cna
    assert 'gene_markers_pairs' in cna.tl.__all__
    d, eng = markers_input(), PairsEngine()
    d.var = pd.DataFrame(index=pd.Index(['g%d' % i for i in range(6)]))
    levels = list(pd.unique(d.obs['pop'].dropna()))                           # first appearance
    assert sorted(levels) == ['neg1', 'pos1', 'pos2']
    lab = d.obs['pop'].astype(object).values
    # pairs=: the order given; (b, a) beside (a, b)
    asked = [('pos1', 'neg1'), ('neg1', 'pos1'), ('pos2', 'neg1')]
    out = cna.tl.gene_markers_pairs(d, 'pop', pairs=asked, engine=eng)
    assert isinstance(out, pd.DataFrame) and out.shape == (6, 27) and (out.dtypes == np.float64).all()
    assert out.index.equals(d.var_names) and list(out.columns.names) == ['pop', 'versus', 'statistic']
    assert list(out.columns) == [(a, b, s) for a, b in asked for s in PAIR_STATISTICS]
    assert list(out.attrs['n_cells'].index) == levels and out.attrs['n_cells'].index.name == 'pop'
    assert list(out.attrs['n_cells'].values) == [int((lab == l).sum()) for l in levels]
    for a, b in asked:
        _check_pair_columns(out, d, a, b)
    np.testing.assert_array_equal(out[('pos1', 'neg1', 'auc')].values + out[('neg1', 'pos1', 'auc')].values, 1.0)
    assert out[('pos1', 'neg1', 'z')].iloc[0] > 5 and out[('pos1', 'neg1', 'auc')].iloc[0] > 0.6      # the planted marker
    # only the named levels are kept: two of three here, recoded to 0, 1, everything else left out
    two = cna.tl.gene_markers_pairs(d, 'pop', pairs=[('neg1', 'pos2')], engine=eng)
    codes, L, idx = eng.asked
    kept2 = [l for l in levels if l in ('neg1', 'pos2')]
    assert L == 2 and idx.tolist() == [[kept2.index('neg1'), kept2.index('pos2')]]
    np.testing.assert_array_equal(codes, [kept2.index(l) if l in kept2 else -1 for l in lab])
    assert list(two.attrs['n_cells'].index) == kept2 and two.shape == (6, 9)
    _check_pair_columns(two, d, 'neg1', 'pos2')
    # reference=: every other level against it, in order of first appearance
    ref = cna.tl.gene_markers_pairs(d, 'pop', reference='neg1', engine=eng)
    want = [(l, 'neg1') for l in levels if l != 'neg1']
    assert list(ref.columns) == [(a, b, s) for a, b in want for s in PAIR_STATISTICS]
    for a, b in want:
        _check_pair_columns(ref, d, a, b)
    # the default: every unordered pair, in order of first appearance
    every = cna.tl.gene_markers_pairs(d, 'pop', engine=eng)
    want = [(levels[i], levels[j]) for i in range(3) for j in range(i + 1, 3)]
    assert list(every.columns) == [(a, b, s) for a, b in want for s in PAIR_STATISTICS] and every.shape == (6, 27)
    for a, b in want:
        _check_pair_columns(every, d, a, b)
    # without the tie correction T = 0; the tie-free gene does not move
    plain = cna.tl.gene_markers_pairs(d, 'pop', pairs=asked, tie_correct=False, engine=eng)
    for a, b in asked:
        na, nb = float((lab == a).sum()), float((lab == b).sum())
        z0 = (out[(a, b, 'u')].values - na * nb / 2) / np.sqrt(na * nb * (na + nb + 1) / 12)
        np.testing.assert_allclose(plain[(a, b, 'z')].values, z0, rtol=1e-13)
        assert (np.abs(plain[(a, b, 'z')].values[:5]) < np.abs(out[(a, b, 'z')].values[:5])).all()
        assert abs(plain[(a, b, 'z')].iloc[5] - out[(a, b, 'z')].iloc[5]) <= 1e-12 * abs(out[(a, b, 'z')].iloc[5])
        np.testing.assert_array_equal(plain[(a, b, 'u')].values, out[(a, b, 'u')].values)
    assert len(eng.uploads) == 1
    d.var = None
    assert isinstance(cna.tl.gene_markers_pairs(d, 'pop', reference='neg1', engine=eng).index, pd.RangeIndex)


def test_pair_statistics_keep_the_level_frame():
    """ranksum_statistics kept its signature and its results: a level against the rest of two levels is the pair"""
    from cna_amd.tools._gene_markers import pair_statistics, ranksum_statistics
    V, _ = core_values()
    codes = core_codes()
    two = np.where(codes == 0, 0, np.where(codes == 2, 1, -1)).astype(np.int32)
    by = ranksum_statistics(*restated_ranksum(V, two, 2))
    u2, tie, n, nan = restated_pairs(V, two, 2, [(0, 1), (1, 0)])
    pr = pair_statistics(u2, tie, n, nan, [(0, 1), (1, 0)])
    assert by.shape == pr.shape == (2, 5, 9)
    np.testing.assert_array_equal(by, pr)


def test_nan_rules():
    import cna_amd as cna
    V, _ = core_values()
    codes = core_codes()
    lev = np.array(['a', 'b', 'c'], dtype=object)[np.maximum(codes, 0)]
    lev[codes < 0] = None
    d = _frame(N_CORE, X=np.ascontiguousarray(V), lev=lev)
    out = cna.tl.gene_markers_pairs(d, 'lev', engine=PairsEngine())
    assert out.shape == (9, 27)
    for a, b in (('a', 'b'), ('a', 'c'), ('b', 'c')):
        for s in RANK_COLS:
            col = out[(a, b, s)].values
            assert np.isnan(col[[0, 2, 5, 7]]).all(), (a, b, s)               # constant over the two levels; a kept NaN
            assert np.isfinite(col[[1, 3, 4, 6, 8]]).all(), (a, b, s)         # a NaN in a left-out cell does no harm
        assert np.isfinite(out[(a, b, 'mean_in')].values[[0, 1, 2, 3, 4, 5, 8]]).all()
    # the NaN of gene 7 sits in one cell of one level: the gene is flagged for every pair, also the pair without that level
    holder = lev[np.flatnonzero(codes >= 0)[7]]
    others = tuple(l for l in ('a', 'b', 'c') if l != holder)
    assert np.isnan(out[others + ('u',)].iloc[7])
    # ... while a call that leaves that level out ranks the gene
    alone = cna.tl.gene_markers_pairs(d, 'lev', pairs=[others], engine=PairsEngine())
    assert np.isfinite(alone[others + ('u',)].iloc[7])
    # an empty level through the statistics directly
    from cna_amd.tools._gene_markers import pair_statistics
    st = pair_statistics(*core_pairs_reference(True), CORE_PAIRS)
    assert st.shape == (12, 5, 9)
    for k, (a, b) in enumerate(CORE_PAIRS):
        assert np.isnan(st[k]).all() if 3 in (a, b) else np.isfinite(st[k][:, 1]).all()


def test_bad_arguments_and_refusals():
    import cna_amd as cna
    from cna_amd import dist, synth
    d, eng = markers_input(), PairsEngine()
    with pytest.raises(KeyError, match='louvain'):
        cna.tl.gene_markers_pairs(d, 'louvain', engine=eng)
    with pytest.raises(ValueError, match='not both'):
        cna.tl.gene_markers_pairs(d, 'pop', pairs=[('pos1', 'neg1')], reference='neg1', engine=eng)
    with pytest.raises(ValueError, match='no level'):
        cna.tl.gene_markers_pairs(d, 'pop', pairs=[('pos1', 'neg9')], engine=eng)
    with pytest.raises(ValueError, match='no level'):
        cna.tl.gene_markers_pairs(d, 'pop', reference='neg9', engine=eng)
    with pytest.raises(ValueError, match='with itself'):
        cna.tl.gene_markers_pairs(d, 'pop', pairs=[('pos1', 'neg1'), ('pos2', 'pos2')], engine=eng)
    with pytest.raises(ValueError, match='twice'):
        cna.tl.gene_markers_pairs(d, 'pop', pairs=[('pos1', 'neg1'), ('pos2', 'neg1'), ('pos1', 'neg1')], engine=eng)
    with pytest.raises(ValueError, match='no pair'):
        cna.tl.gene_markers_pairs(d, 'pop', pairs=[], engine=eng)
    with pytest.raises(KeyError):
        cna.tl.gene_markers_pairs(d, 'pop', layer='missing', engine=eng)
    # the limits: 64 levels taking part, 2016 pairs; a column with more levels is fine when the pairs name few
    wide = np.ascontiguousarray(np.arange(2200, dtype=np.float32).reshape(1100, 2) % 7)
    d65 = _frame(1100, X=wide, lev=np.arange(1100) % 65)
    with pytest.raises(ValueError, match='65 levels take part, at most 64'):
        cna.tl.gene_markers_pairs(d65, 'lev', engine=eng)
    with pytest.raises(ValueError, match='65 levels take part, at most 64'):
        cna.tl.gene_markers_pairs(d65, 'lev', reference=0, engine=eng)
    ordered = [(a, b) for a in range(64) for b in range(64) if a != b]
    with pytest.raises(ValueError, match='2017 pairs, at most 2016'):
        cna.tl.gene_markers_pairs(d65, 'lev', pairs=ordered[:2017], engine=eng)
    with pytest.raises(NotImplementedError, match='multi-rank'):
        cna.tl.gene_markers_pairs(d, 'pop', engine=PairsEngine(nranks=2))
    data, _ = synth.make_demo_like(n_samples=20, n_genes=30, cells_per_sample=100, seed=3, keep_expression=True)
    part = dist.shard(data, rank=0, nranks=2)
    part.X = data.X[:len(part.obs)]
    part.obs['lev'] = np.where(np.arange(len(part.obs)) % 2, 'a', 'b')
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.gene_markers_pairs(part, 'lev', engine=eng)
    assert eng.uploads == []
    assert cna.tl.gene_markers_pairs(d65, 'lev', pairs=ordered[:2016], engine=eng).shape == (2, 2016 * 9)
    assert cna.tl.gene_markers_pairs(d65, 'lev', pairs=[(64, 3), (3, 1)], engine=eng).shape == (2, 18)
    assert eng.asked[1] == 3 and eng.asked[2].tolist() == [[2, 1], [1, 0]]


def test_entry_is_declared():
    from cna_amd import _ffi
    assert 'cna_gene_ranksum_pairs' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'cna_gene_ranksum_pairs')
    assert _ffi.KERNELS[-1] == 'ranksum_pairs' and _ffi.load().cna_abi_version() == 1
    from cna_amd.engine import Engine
    assert callable(Engine.gene_ranksum_pairs)


# ------------------------------------------------------------------ what the GPU inputs reach
@pytest.mark.parametrize('form', ['csr-f32', 'csc-f64', 'dense-f32', 'dense-f64'])
def test_tie_runs_of_a_tested_pair_meet_the_cuts_of_the_unit(form):
    """k_rs_pairs takes the sorted kept entries of a gene RS_UNIT at a time, over ALL levels (the sort is shared).  Gene 4:
    the run of -2.0 ends exactly on a cut with another value behind it -- its group is closed by the unit's last thread;
    the run of -1.0 spans two cuts -- its start counts are carried twice.  Both runs hold cells of the levels 0, 1 and 2,
    so every tested pair of those reads them."""
    unit = ranksum_constant('RS_UNIT')
    V, S = core_values()
    codes = core_codes()
    kept = codes >= 0
    use = kept if form.startswith('dense') else kept & S[:, 4]
    order = np.argsort(V[use, 4].astype(np.float32 if form.endswith('f32') else np.float64), kind='stable')
    col, lev = V[use, 4][order], codes[use][order]
    heads = np.flatnonzero(np.r_[True, col[1:] != col[:-1]])
    ends = np.r_[heads[1:], len(col)]
    runs = {float(col[h]): (int(h), int(e)) for h, e in zip(heads, ends)}
    lo, hi = runs[-2.0]
    assert lo == 0 and hi % unit == 0 and hi < len(col) and hi - lo > 1
    assert set(lev[lo:hi]) == {0, 1, 2}
    lo, hi = runs[-1.0]
    assert len([c for c in range(unit, len(col), unit) if lo < c < hi]) >= 2
    assert set(lev[lo:hi]) == {0, 1, 2}
    assert all((a, b) in CORE_PAIRS for a in range(3) for b in range(3) if a != b)
