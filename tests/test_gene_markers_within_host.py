"""cna.tl.gene_markers_within on the CPU: the numpy / scipy restatement of cna_gene_ranksum_within (what the GPU tests compare
the device with: integers for equality, the two weighted float64 sums bit for bit), an independent computation from
scipy.stats.mannwhitneyu per block, the public call against an engine double (MarkersEngine of test_gene_markers_host.py
with `gene_ranksum_within` backed by the restatement), the confounded example that is the reason for the tool, and the
figures of the GPU tests' fixtures: their kept cells, their largest tie term, the one-block case."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.stats

from test_gene_corr_host import _frame
from test_gene_markers_host import (FORMS, N_CORE, MarkersEngine, _dense, core_codes, core_input, core_reference, core_values,
                                    markers_input, ranksum_constant, restated_ranksum)
from test_gene_rank_corr_host import RHO_TOL
from test_gene_rank_corr_strata_host import STRATA_LEVELS, BIG, ONE, TWO, ALL_LOST, EMPTY, many_codes, strata_kept, strata_labels

WITHIN_STATISTICS = ['auc', 'z', 'p', 'q', 'blocks']


# ------------------------------------------------------------------ the restatement
def restated_within(X, codes, L, blocks, B, w_num, w_tie):
    """(d2 int64[L, G], num float64[L, G], tiew float64[L, G], live int32[L, G], n int64[B, L], nan bool[G]) of
    cna_gene_ranksum_within.  Per block scipy's midranks of the block's kept rows, doubled; D in Python integers; the tie term
    from np.unique's counts in Python integers, asserted below 2^53: every partial sum of the device's doubles is then an
    integer a double holds, which is why its T_gs, and with it the sequential fold below -- a product and a sum, each
    rounded once, blocks in order, empty ones included -- can be asked for bit for bit.  A gene with a NaN in a kept cell
    is flagged and its numbers are 0 (the device leaves them unspecified: callers compare the other genes)."""
    Xd = _dense(X)
    codes, blocks = np.asarray(codes), np.asarray(blocks)
    w_num = np.asarray(w_num, dtype=np.float64)
    w_tie = np.asarray(w_tie, dtype=np.float64).reshape(B, L)
    kept = (codes >= 0) & (blocks >= 0)
    G = Xd.shape[1]
    n = np.bincount(blocks[kept].astype(np.int64) * L + codes[kept], minlength=B * L).reshape(B, L).astype(np.int64)
    rows = [np.flatnonzero(kept & (blocks == s)) for s in range(B)]
    d2 = np.zeros((L, G), dtype=object)
    num, tiew = np.zeros((L, G)), np.zeros((L, G))
    live = np.zeros((L, G), dtype=np.int32)
    nan = np.zeros(G, dtype=bool)
    for g in range(G):
        if np.isnan(Xd[kept, g].astype(np.float64)).any():
            nan[g] = True
            continue
        for s in range(B):
            col = Xd[rows[s], g].astype(np.float64)          # exact from float32: the order and the ties of the stored type
            ns = len(col)
            D, T = [0] * L, 0
            if ns:
                r2 = np.rint(2.0 * scipy.stats.rankdata(col, method='average'))
                R2 = np.rint(np.bincount(codes[rows[s]], weights=r2, minlength=L)).astype(np.int64)      # sums < 2^53: exact
                D = [int(R2[l]) - int(n[s, l]) * (ns + 1) for l in range(L)]
                t = np.unique(col, return_counts=True)[1]
                T = sum(int(v) ** 3 - int(v) for v in t)
                assert T < 2 ** 53
                live[:, g] += ((n[s] > 0) & (n[s] < ns) & (len(t) > 1)).astype(np.int32)
            for l in range(L):
                d2[l, g] += D[l]
            Df = np.array([float(v) for v in D])
            num[:, g] = num[:, g] + w_num[s] * Df
            tiew[:, g] = tiew[:, g] + w_tie[s] * float(T)
    assert all(abs(int(v)) < 2 ** 63 for v in d2.ravel())
    return d2.astype(np.int64), num, tiew, live, n, nan


def largest_tie_term(X, codes, blocks, B):
    Xd = _dense(X)
    kept = (np.asarray(codes) >= 0) & (np.asarray(blocks) >= 0)
    best = 0
    for g in range(Xd.shape[1]):
        for s in range(B):
            col = Xd[kept & (blocks == s), g].astype(np.float64)
            if len(col) and not np.isnan(col).any():
                best = max(best, sum(int(v) ** 3 - int(v) for v in np.unique(col, return_counts=True)[1]))
    return best


# ------------------------------------------------------------------ the GPU tests' inputs
def counts_of(codes, L, blocks, B):
    kept = (codes >= 0) & (blocks >= 0)
    return np.bincount(blocks[kept].astype(np.int64) * L + codes[kept], minlength=B * L).reshape(B, L).astype(np.int64)


def weight_tables(codes, L, blocks, B, which):
    """(w_num [B], w_tie [B, L]): 've' van Elteren's, from the product's own function of the counts; 'any' an arbitrary
    finite table with negative entries; 'ones' all 1"""
    if which == 've':
        from cna_amd.tools._gene_markers import within_weights
        a, c, _, _ = within_weights(counts_of(codes, L, blocks, B))
        return np.ascontiguousarray(a), np.ascontiguousarray(c)
    if which == 'ones':
        return np.ones(B), np.ones((B, L))
    rs = np.random.RandomState(29)
    return rs.randn(B) * 3.0, np.ascontiguousarray(rs.randn(B, L) * np.exp(rs.randn(B, L)))


def within_codes(which='core'):
    """(level codes, L, block codes, B) of the GPU tests' cases on the 3001 core cells"""
    if which == 'core':
        return core_codes(), 4, strata_kept().astype(np.int32), STRATA_LEVELS
    if which == '1024':
        return core_codes('1024'), 1024, strata_kept().astype(np.int32), STRATA_LEVELS
    if which == '255':
        return core_codes(), 4, many_codes(255), 255
    assert which == 'one'
    return core_codes(), 4, np.zeros(N_CORE, dtype=np.int32), 1


@functools.lru_cache(maxsize=None)
def within_reference(form, which='core', weights='ve'):
    """One restatement per stored type, code set and weight table: the sparse and the dense upload of one type hold the same
    values."""
    V, _ = core_values()
    codes, L, blocks, B = within_codes(which)
    out = restated_within(V.astype(np.float32 if form.endswith('f32') else np.float64), codes, L, blocks, B,
                          *weight_tables(codes, L, blocks, B, weights))
    for a in out:
        a.setflags(write=False)
    return out


def test_figures_of_the_gpu_fixtures():
    codes, L, blocks, B = within_codes()
    assert int(((codes >= 0) & (blocks >= 0)).sum()) == 2844 and B == 9 and L == 4
    n = counts_of(codes, L, blocks, B)
    sizes = n.sum(axis=1)
    assert sizes[ONE] == 1 and sizes[TWO] == 2 and sizes[ALL_LOST] == 0 and sizes[EMPTY] == 0        # tiny and empty blocks
    assert (n[:, 3] == 0).all() and ((n[:, :3] == 0) & (sizes > 0)[:, None]).any()                     # a level absent in a block
    for form in ('dense-f32', 'dense-f64'):
        assert largest_tie_term(core_input(form), codes, blocks, B) == 7055790714
    _, S = core_values()
    assert not S[blocks == BIG + 1, 4].any() and S[blocks == BIG, 4].any()        # a sparse gene without an entry in a block
    ref = within_reference('dense-f64')
    assert list(np.flatnonzero(ref[5])) == [7] and ref[3].max() >= 5 and (ref[3][3] == 0).all()
    assert len(set(ref[1].ravel())) == 16 and (ref[2] >= 0).all()       # 3 levels x 5 genes that vary: 15 sums, and 0.0


@pytest.mark.parametrize('form', ['dense-f32', 'dense-f64'])
def test_one_block_is_the_pooled_rank_sum(form):
    """one block of all kept cells, weights 1: D = rank2 - n_l (m + 1) and the tie term of cna_gene_ranksum_by"""
    d2, num, tiew, live, n, nan = within_reference(form, 'one', 'ones')
    rank2, tie, nl, flagged = core_reference(form)
    m = int(nl.sum())
    ok = ~flagged
    np.testing.assert_array_equal(nan, flagged)
    np.testing.assert_array_equal(n[0], nl)
    np.testing.assert_array_equal(d2[:, ok], (rank2 - (nl * (m + 1))[:, None])[:, ok])
    np.testing.assert_array_equal(num[:, ok], d2[:, ok].astype(np.float64))
    np.testing.assert_array_equal(tiew[:, ok], np.broadcast_to(tie, tiew.shape)[:, ok])
    constant = tie == float(m ** 3 - m)
    np.testing.assert_array_equal(live[:3][:, ok], np.broadcast_to(~constant, (3, 9))[:, ok].astype(np.int32))
    # and through the statistics: with weights 'sum' the one block is the pooled test
    from cna_amd.tools._gene_markers import ranksum_statistics, within_statistics, within_weights
    pooled = ranksum_statistics(rank2, tie, nl, flagged)
    a, c, _, _ = within_weights(n, 'sum')
    assert a.tolist() == [1.0]
    V, _ = core_values()
    codes, L, blocks, B = within_codes('one')
    summed = restated_within(V.astype(np.float32 if form.endswith('f32') else np.float64), codes, L, blocks, B, a, c)
    np.testing.assert_array_equal(summed[0], d2)
    mine = within_statistics(*summed, weights='sum')
    np.testing.assert_array_equal(np.isnan(mine[:, 1]), np.isnan(pooled[:, 2]))
    alive = ~np.isnan(pooled[:, 2])
    assert alive.sum() == 15 and np.abs(mine[:, 1][alive] - pooled[:, 2][alive]).max() <= RHO_TOL        # z
    assert np.abs(mine[:, 0][alive] - pooled[:, 0][alive]).max() <= RHO_TOL                              # auc


def test_sum_of_the_single_blocks_is_the_whole():
    """what the GPU test asks of the device, on the restatement: a block alone (the others left out) as a 1-block call.  The
    integer sum of the single blocks' d2 is the whole call's; a single block's num is w_s D_s rounded once, so folding them
    in block order gives the whole call's num bit for bit"""
    V, _ = core_values()
    codes, L, blocks, B = within_codes()
    w_num, w_tie = weight_tables(codes, L, blocks, B, 've')
    whole = within_reference('dense-f64')
    total = np.zeros((L, 9), dtype=np.int64)
    num, tiew = np.zeros((L, 9)), np.zeros((L, 9))
    for s in range(B):
        only = np.where(blocks == s, 0, -1).astype(np.int32)
        one = restated_within(V, codes, L, only, 1, w_num[s:s + 1], w_tie[s:s + 1])
        np.testing.assert_array_equal(one[4][0], whole[4][s])
        total += one[0]
        num = num + one[1]
        tiew = tiew + one[2]
    ok = ~whole[5]
    np.testing.assert_array_equal(total[:, ok], whole[0][:, ok])
    np.testing.assert_array_equal(num[:, ok].view(np.int64), np.ascontiguousarray(whole[1][:, ok]).view(np.int64))
    np.testing.assert_array_equal(tiew[:, ok].view(np.int64), np.ascontiguousarray(whole[2][:, ok]).view(np.int64))


# ------------------------------------------------------------------ an independent computation, block by block
def van_elteren_table(Xd, codes, L, blocks, B, weights='van_elteren', tie_correct=True):
    """{(level, gene): (auc, z, blocks)} from scipy.stats.mannwhitneyu(x_in, x_rest, use_continuity=False,
    method='asymptotic') inside every block that holds the level and other cells; the variance of a block's U with the tie
    correction, n1 n2 / 12 ((n + 1) - sum(t^3 - t) / (n (n - 1))), is the textbook's.  None where no block can tell."""
    Xd = np.asarray(Xd, dtype=np.float64)
    out = {}
    for l in range(L):
        for g in range(Xd.shape[1]):
            top = var = centred = pairs = 0.0
            used = 0
            bad = False
            for s in range(B):
                cells = (blocks == s) & (codes >= 0)
                x, y = Xd[cells & (codes == l), g], Xd[cells & (codes != l), g]
                if np.isnan(x).any() or np.isnan(y).any():
                    bad = True
                if len(x) == 0 or len(y) == 0 or bad:
                    continue
                n1, n2, ns = len(x), len(y), len(x) + len(y)
                a = 1.0 / (ns + 1.0) if weights == 'van_elteren' else 1.0
                u = scipy.stats.mannwhitneyu(x, y, use_continuity=False, method='asymptotic').statistic
                t = np.unique(np.r_[x, y], return_counts=True)[1].astype(np.float64)
                T = (t ** 3 - t).sum() if tie_correct else 0.0
                top += a * (u - n1 * n2 / 2.0)
                var += a * a * n1 * n2 / 12.0 * ((ns + 1.0) - T / (ns * (ns - 1.0)))
                centred += u - n1 * n2 / 2.0
                pairs += n1 * n2
                used += len(t) > 1
            out[(l, g)] = None if bad or pairs == 0 or used == 0 else (0.5 + centred / pairs, top / np.sqrt(var), used)
    return out


def assert_frame_matches(frame, levels, table, G):
    checked = 0
    for b, lev in enumerate(levels):
        for g in range(G):
            got, want = frame[lev].iloc[g], table[(b, g)]
            if want is None:
                assert np.isnan(got[['auc', 'z', 'p', 'q']].values).all(), (lev, g)
                continue
            print('%s gene %d: auc %.12f / %.12f  z %.12f / %.12f  blocks %d' % (lev, g, got['auc'], want[0], got['z'], want[1],
                                                                                   got['blocks']))
            assert abs(got['auc'] - want[0]) <= RHO_TOL and abs(got['z'] - want[1]) <= RHO_TOL and got['blocks'] == want[2]
            assert abs(got['p'] - scipy.stats.norm.sf(abs(want[1])) * 2) <= 1e-6 * got['p'] + 1e-300
            checked += 1
    return checked


# ------------------------------------------------------------------ the public call
class WithinEngine(MarkersEngine):
    """MarkersEngine (the real residency code, counted uploads, the pooled calls as numpy) with the new device call as numpy."""

    def gene_ranksum_within(self, codes, n_levels, blocks, n_blocks, w_num, w_tie, work_bytes=0):
        assert self.resident is not None
        self.last = restated_within(self.resident, codes, n_levels, blocks, n_blocks, w_num, w_tie)
        return self.last


def _within_data():
    d = markers_input()
    d.obs['sample'] = strata_labels(len(d.obs))
    d.var = pd.DataFrame(index=pd.Index(['g%d' % i for i in range(6)]))
    return d


def _factor(col):
    codes, levels = pd.factorize(np.asarray(col, dtype=object))
    return codes.astype(np.int32), list(levels)


def test_gene_markers_within_through_the_public_call():
    import cna_amd as cna
    from cna_amd.tools._gene_test import benjamini_hochberg
    assert 'gene_markers_within' in cna.tl.__all__
    d, eng = _within_data(), WithinEngine()
    out = cna.tl.gene_markers_within(d, 'pop', 'sample', engine=eng)
    codes, levels = _factor(d.obs['pop'])
    blocks, samples = _factor(d.obs['sample'])
    assert sorted(levels) == ['neg1', 'pos1', 'pos2'] and sorted(samples) == ['c0', 'c1', 'tiny']
    assert isinstance(out, pd.DataFrame) and out.shape == (6, 15) and (out.dtypes == np.float64).all()
    assert out.index.equals(d.var_names) and list(out.columns.names) == ['pop', 'statistic']
    assert list(out.columns) == [(l, s) for l in levels for s in WITHIN_STATISTICS]             # level-major
    kept = (codes >= 0) & (blocks >= 0)
    assert 0 < (codes < 0).sum() and 0 < (blocks < 0).sum() and kept.sum() < min((codes >= 0).sum(), (blocks >= 0).sum())
    n_cells, counts = out.attrs['n_cells'], out.attrs['counts']
    assert isinstance(n_cells, pd.Series) and n_cells.index.name == 'pop' and list(n_cells.index) == levels
    assert list(n_cells.values) == [int((kept & (codes == b)).sum()) for b in range(3)]         # NaN in either column: left out
    assert isinstance(counts, pd.DataFrame) and counts.index.name == 'sample' and list(counts.index) == samples
    assert list(counts.columns) == levels and counts.values.sum() == kept.sum() and counts.values.dtype == np.int64
    np.testing.assert_array_equal(counts.values, counts_of(codes, 3, blocks, 3))
    np.testing.assert_array_equal(eng.last[4], counts.values)
    assert assert_frame_matches(out, levels, van_elteren_table(d.X, codes, 3, blocks, 3), 6) == 18
    for l in levels:
        np.testing.assert_array_equal(out[(l, 'q')].values, benjamini_hochberg(out[(l, 'p')].values))   # q inside the level
    assert out[('pos1', 'z')].iloc[0] > 5 and out[('pos1', 'auc')].iloc[0] > 0.6                  # the planted marker
    # the weights and the tie correction
    plain = cna.tl.gene_markers_within(d, 'pop', 'sample', weights='sum', engine=eng)
    assert assert_frame_matches(plain, levels, van_elteren_table(d.X, codes, 3, blocks, 3, weights='sum'), 6) == 18
    np.testing.assert_array_equal(plain.xs('auc', axis=1, level=1).values, out.xs('auc', axis=1, level=1).values)
    assert not np.array_equal(plain.xs('z', axis=1, level=1).values, out.xs('z', axis=1, level=1).values)
    loose = cna.tl.gene_markers_within(d, 'pop', 'sample', tie_correct=False, engine=eng)
    assert assert_frame_matches(loose, levels, van_elteren_table(d.X, codes, 3, blocks, 3, tie_correct=False), 6) == 18
    for l in levels:
        assert (np.abs(loose[(l, 'z')].values[:5]) < np.abs(out[(l, 'z')].values[:5])).all()
        assert abs(loose[(l, 'z')].iloc[5] - out[(l, 'z')].iloc[5]) <= 1e-12 * abs(out[(l, 'z')].iloc[5])   # the tie-free gene
    with pytest.raises(ValueError, match='weights'):
        cna.tl.gene_markers_within(d, 'pop', 'sample', weights='size', engine=eng)
    assert len(eng.uploads) == 1
    d.var = None
    assert isinstance(cna.tl.gene_markers_within(d, 'pop', 'sample', engine=eng).index, pd.RangeIndex)


def test_the_core_input_against_mannwhitneyu_per_block():
    """the GPU tests' nine genes in their nine blocks through the statistics: every (level, gene) against scipy"""
    from cna_amd.tools._gene_markers import within_statistics
    codes, L, blocks, B = within_codes()
    for weights in ('van_elteren', 'sum'):
        from cna_amd.tools._gene_markers import within_weights
        a, c, _, _ = within_weights(counts_of(codes, L, blocks, B), weights)
        V, _ = core_values()
        d2, num, tiew, live, n, nan = restated_within(V, codes, L, blocks, B, a, c)
        st = within_statistics(d2, num, tiew, live, n, nan, weights=weights)
        table = van_elteren_table(V, codes, L, blocks, B, weights=weights)
        checked = 0
        for (l, g), want in table.items():
            if want is None:
                assert np.isnan(st[l, :4, g]).all(), (l, g)
            else:
                assert abs(st[l, 0, g] - want[0]) <= RHO_TOL and abs(st[l, 1, g] - want[1]) <= RHO_TOL and st[l, 4, g] == want[2]
                checked += 1
        assert checked == 15 and np.isnan(st[3, :4]).all() and np.isnan(st[:, :4, [0, 2, 5, 7]]).all()


def test_nan_rules():
    import cna_amd as cna
    rs = np.random.RandomState(3)
    n = 240
    block = np.array(['s%d' % (i % 3) for i in range(n)], dtype=object)
    level = np.array(['a', 'b'], dtype=object)[rs.randint(0, 2, size=n)]
    level[:12] = 'ghost'                                   # every cell of this level has no block: an empty level
    block[:12] = None
    level[12:40] = 'solo'                                  # a level that is a whole block wherever it occurs
    block[12:40] = 'own'
    X = rs.poisson(2.0, size=(n, 5)).astype(np.float64)
    X[:, 1] = np.where(block == 's0', 4.0, np.where(block == 's1', 9.0, -1.0))        # constant inside every block
    X[block == 'own', 2] = 3.0                                                         # constant only where nothing can tell
    X[50, 3] = np.nan                                                                  # a kept NaN
    X[3, 4] = np.nan                                                                   # a NaN in a left-out cell
    out = cna.tl.gene_markers_within(_frame(n, X=X, level=level, block=block), 'level', 'block', engine=WithinEngine())
    rank_cols = ['auc', 'z', 'p', 'q']
    assert list(out.attrs['n_cells'].index)[:2] == ['ghost', 'solo'] and sorted(out.attrs['n_cells'].index[2:]) == ['a', 'b']
    assert out.attrs['n_cells']['ghost'] == 0
    assert out.attrs['n_cells']['solo'] == 28 and list(out.attrs['counts'].index) == ['own', 's1', 's2', 's0']   # first appearance
    for lev in ('ghost', 'solo'):
        assert np.isnan(out[lev][rank_cols].values).all() and (out[(lev, 'blocks')].values == 0).all()
    for lev in ('a', 'b'):
        assert np.isnan(out[lev][rank_cols].values[[1, 3]]).all()                     # constant in every block; flagged
        assert np.isfinite(out[lev][rank_cols].values[[0, 2, 4]]).all()
        assert out[(lev, 'blocks')].iloc[1] == 0 and list(out[(lev, 'blocks')].values[[0, 2, 4]]) == [3, 3, 3]
    # two levels share every block: d2 of one is minus the other's, the aucs sum to 1 (each rounded once, at 0.5: 2^-53 each)
    np.testing.assert_allclose(out[('a', 'auc')].values[[0, 2, 4]] + out[('b', 'auc')].values[[0, 2, 4]], 1.0, rtol=0, atol=2.0 ** -51)


def test_a_shift_between_blocks_is_no_marker():
    """400 cells, two blocks, one population: in block 0 (values 1000 + j) every tie group holds four cells of it and one of
    the rest, in block 1 (values j) one and four.  Pooled, the population's cells are the high ones: auc 0.8; inside each
    block twice the centred rank sum is exactly 0."""
    import cna_amd as cna
    j = np.repeat(np.arange(40), 5)
    X = np.r_[1000.0 + j, 0.0 + j][:, None]
    pop = np.r_[np.tile(['pop', 'pop', 'pop', 'pop', 'rest'], 40), np.tile(['pop', 'rest', 'rest', 'rest', 'rest'], 40)]
    block = np.repeat(['donor0', 'donor1'], 200)
    d, eng = _frame(400, X=np.ascontiguousarray(X), pop=pop.astype(object), donor=block.astype(object)), WithinEngine()
    pooled = cna.tl.gene_markers(d, 'pop', engine=eng)
    res = scipy.stats.mannwhitneyu(X[pop == 'pop', 0], X[pop == 'rest', 0], use_continuity=False, method='asymptotic')
    assert abs(pooled[('pop', 'auc')].iloc[0] - 0.8) <= 1e-12 and res.pvalue < 1e-24 and pooled[('pop', 'p')].iloc[0] < 1e-24
    for weights in ('van_elteren', 'sum'):
        out = cna.tl.gene_markers_within(d, 'pop', 'donor', weights=weights, engine=eng)
        assert (eng.last[0] == 0).all() and (eng.last[1] == 0.0).all() and (eng.last[3] == 2).all()
        for lev in ('pop', 'rest'):
            assert out[(lev, 'auc')].iloc[0] == 0.5 and out[(lev, 'z')].iloc[0] == 0.0 and out[(lev, 'p')].iloc[0] == 1.0
            assert out[(lev, 'blocks')].iloc[0] == 2


def test_one_block_with_sum_weights_is_gene_markers():
    import cna_amd as cna
    d, eng = markers_input(), WithinEngine()
    d.obs['all'] = 'everything'
    pooled = cna.tl.gene_markers(d, 'pop', engine=eng)
    out = cna.tl.gene_markers_within(d, 'pop', 'all', weights='sum', engine=eng)
    for lev in ('pos1', 'neg1', 'pos2'):
        for s in ('z', 'auc'):
            assert np.abs(out[(lev, s)].values - pooled[(lev, s)].values).max() <= RHO_TOL
        np.testing.assert_allclose(out[(lev, 'p')].values, pooled[(lev, 'p')].values, rtol=1e-6)
        assert (out[(lev, 'blocks')].values == 1).all()


def test_bad_arguments_and_refusals():
    import cna_amd as cna
    from cna_amd import dist, synth
    d, eng = _within_data(), WithinEngine()
    n = len(d.obs)
    with pytest.raises(KeyError, match='louvain'):
        cna.tl.gene_markers_within(d, 'louvain', 'sample', engine=eng)
    with pytest.raises(KeyError, match='donor'):
        cna.tl.gene_markers_within(d, 'pop', 'donor', engine=eng)
    d.obs['fine'] = np.arange(n) % 256
    with pytest.raises(ValueError, match='255'):
        cna.tl.gene_markers_within(d, 'pop', 'fine', engine=eng)
    with pytest.raises(ValueError, match='0 levels'):
        cna.tl.gene_markers_within(_frame(n, X=d.X, pop=d.obs['pop'].values, sample=np.full(n, np.nan)), 'pop', 'sample', engine=eng)
    with pytest.raises(KeyError):
        cna.tl.gene_markers_within(d, 'pop', 'sample', layer='missing', engine=eng)
    with pytest.raises(NotImplementedError, match='multi-rank'):
        cna.tl.gene_markers_within(d, 'pop', 'sample', engine=WithinEngine(nranks=2))
    data, _ = synth.make_demo_like(n_samples=20, n_genes=30, cells_per_sample=100, seed=3, keep_expression=True)
    part = dist.shard(data, rank=0, nranks=2)
    part.X = data.X[:len(part.obs)]
    part.obs['lev'] = 'a'
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.gene_markers_within(part, 'lev', 'id', engine=eng)
    assert eng.uploads == []
    d.obs['fine'] = np.arange(n) % 255
    out = cna.tl.gene_markers_within(d, 'pop', 'fine', engine=eng)
    assert out.shape == (6, 15) and out.attrs['counts'].shape == (255, 3)


def test_entry_is_declared_and_the_kernel_ids_have_not_moved():
    from cna_amd import _ffi
    from cna_amd.engine import Engine
    from cna_amd.tools import _gene_markers
    lib = _ffi.load()
    assert 'cna_gene_ranksum_within' in _ffi.SIGNATURES and hasattr(lib, 'cna_gene_ranksum_within') and lib.cna_abi_version() == 1
    assert callable(Engine.gene_ranksum_within)
    assert ranksum_constant('RW_MAX_BLOCKS') == 255 == _gene_markers.MAX_BLOCKS and ranksum_constant('RS_MAX_LEVELS') == 1024
    names = _ffi.KERNELS + _ffi.KERNELS_RANK_CORR
    assert [lib.cna_kernel_name(k).decode() for k in range(len(names))] == names
