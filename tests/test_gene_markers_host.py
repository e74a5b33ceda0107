"""cna.tl.gene_markers on the CPU: the numpy / scipy restatement of cna_gene_ranksum_by (what the GPU tests compare the device
with, integer for integer), its check against scipy.stats.mannwhitneyu on the GPU tests' own inputs, the public call against
an engine double (GeneEngine of test_gene_corr_host.py with `gene_ranksum_by` backed by the restatement), and the proofs,
without a device, that the GPU inputs reach what they are meant to reach: three sort chunks per long gene, two tiles of
genes under the small budget, a tie run that ends on a cut of the rank kernel's unit and one that spans two cuts.  The
constants of csrc/rank_sort.h (the sort and the walk), csrc/expr_ranksum.hip and csrc/expr_rankcorr.hip are read from the
source, so a change there fails these proofs instead of leaving a path untested."""
import functools
import os
import re

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import scipy.stats

from test_gene_corr_host import GeneEngine, _frame
from test_expr_tiles_host import chunk_length

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATISTICS = ['auc', 'u', 'z', 'p', 'q', 'mean_in', 'mean_rest', 'frac_in', 'frac_rest']
Z_MAX = 30.0            # |z| of every checked (gene, level): the project's 1e-10 on z then moves p by z^2 1e-10 <= 9e-8
P_RTOL = 1e-6           # ... relative, with a factor 10 of margin


def ranksum_source(*files):
    return ''.join(open(os.path.join(ROOT, 'cna_amd', 'csrc', f)).read() for f in files)


def ranksum_constant(name):
    src = ranksum_source('rank_sort.h', 'expr_ranksum.hip', 'expr_rankcorr.hip')
    m = re.search(r'constexpr (?:int|int64_t) %s = (\d+)(?:ll)?(?: << (\d+))?;' % name, src)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


# ------------------------------------------------------------------ the restatement
def _dense(X):
    return np.asarray(X.toarray() if sp.issparse(X) else X)


def restated_ranksum(X, codes, L):
    """(rank2 int64[L, G], tie float64[G], n int64[L], nan bool[G]) of cna_gene_ranksum_by: scipy's midranks of the kept rows
    of every gene, doubled; the tie term from np.unique's counts in exact integers.  A gene with a NaN in a kept cell is
    flagged and its numbers are 0 (the device leaves them unspecified: callers compare the other genes)."""
    Xd = _dense(X)
    codes = np.asarray(codes)
    kept = codes >= 0
    c = codes[kept]
    G = Xd.shape[1]
    rank2 = np.zeros((L, G), dtype=np.int64)
    tie = np.zeros(G)
    nan = np.zeros(G, dtype=bool)
    n = np.bincount(c, minlength=L).astype(np.int64)
    for g in range(G):
        col = Xd[kept, g].astype(np.float64)            # exact from float32: the order and the ties of the stored type
        if np.isnan(col).any():
            nan[g] = True
            continue
        if col.size == 0:
            continue
        r2 = np.rint(2.0 * scipy.stats.rankdata(col, method='average'))
        rank2[:, g] = np.rint(np.bincount(c, weights=r2, minlength=L)).astype(np.int64)      # sums < 2^53: exact
        t = np.unique(col, return_counts=True)[1]
        tie[g] = float(sum(int(v) ** 3 - int(v) for v in t))
    return rank2, tie, n, nan


def restated_bins(X, codes, L, what):
    Xd = _dense(X).astype(np.float64)
    if what == 1:
        Xd = (Xd > 0).astype(np.float64)
    codes = np.asarray(codes)
    sums = np.zeros((L, Xd.shape[1]))
    with np.errstate(invalid='ignore'):                # inf - inf inside a gene is that gene's own affair
        for b in range(L):
            sums[b] = Xd[codes == b].sum(axis=0)
    return sums, np.bincount(codes[codes >= 0], minlength=L).astype(np.int64)


# ------------------------------------------------------------------ the GPU tests' inputs
N_CORE = 3001
CORE_LEVELS = 4         # 0, 1, 2 and a level without cells
RUN_ON_CUT = 256        # gene 4: kept cells with -2.0, the smallest value: positions [0, 256) of the sorted list
RUN_OVER_CUTS = 700     # gene 4: kept cells with -1.0: positions [256, 956)
SMALL_WORK_BYTES = 40000
FORMS = ['csr-f32', 'csc-f64', 'dense-f32', 'dense-f64']


def core_codes(which='core'):
    rs = np.random.RandomState(11)
    codes = rs.choice(3, size=N_CORE, p=[0.5, 0.3, 0.2]).astype(np.int32)
    codes[rs.rand(N_CORE) < 0.05] = -1
    if which == 'one':
        return np.where(codes >= 0, 0, -1).astype(np.int32)
    if which == '1024':
        return np.where(codes >= 0, np.arange(N_CORE) * 7 % 1024, -1).astype(np.int32)
    return codes


@functools.lru_cache(maxsize=None)
def core_values():
    """(values float64 [3001, 9], stored bool [3001, 9]): the nine genes of tests/test_gpu_gene_markers.py.  `stored` says
    which entries a sparse upload stores (explicit zeros among them); a dense upload holds `values` as it is."""
    n = N_CORE
    rs = np.random.RandomState(5)
    codes = core_codes()
    kept = np.flatnonzero(codes >= 0)
    left = np.flatnonzero(codes < 0)
    V = np.zeros((n, 9))
    S = np.zeros((n, 9), dtype=bool)
    # 0: no stored entry
    # 1: every cell, all distinct: three chunks, the last one ragged
    V[:, 1] = (rs.permutation(n) + 1) * 0.5
    S[:, 1] = True
    # 2: every cell, constant: one run across every cut
    V[:, 2] = 2.5
    S[:, 2] = True
    # 3: small integers with explicit stored zeros, a stored -0.0, implicit zeros
    at = rs.rand(n) < 0.4
    V[at, 3] = rs.randint(0, 4, size=int(at.sum()))
    S[at, 3] = True
    V[kept[:3], 3] = -0.0
    S[kept[:3], 3] = True
    # 4: negatives and positives around the implicit zero group, ties shared across the levels; a run that ends on a cut of
    # the rank kernel's unit and one that spans two
    order = rs.permutation(kept)
    a, b = RUN_ON_CUT, RUN_ON_CUT + RUN_OVER_CUTS
    V[order[:a], 4] = -2.0
    V[order[a:b], 4] = -1.0
    V[order[b:b + 300], 4] = 1.0
    V[order[b + 300:b + 500], 4] = 3.0
    S[order[:b + 500], 4] = True
    V[left[:20], 4] = np.tile([-1.0, 1.0, -5.0, 9.0], 5)      # left-out cells: no part of any rank
    S[left[:20], 4] = True
    # 5: a single stored entry whose cell is left out
    V[left[-1], 5] = 7.0
    S[left[-1], 5] = True
    # 6: +-inf, denormals (of float32 and of float64), neighbours one ulp apart, pairs that collide in float32
    one = np.float32(1.0)
    up1 = np.nextafter(one, np.float32(2.0))
    up2 = np.nextafter(up1, np.float32(2.0))
    d32 = float(np.float32(1.4e-45))
    vals = [np.inf, -np.inf, np.inf, -np.inf, d32, 2 * d32, -d32, d32, 5e-324, -5e-324, 1.0, float(up1), float(up2), float(up1),
            1.0 + 2.0 ** -40, 1.0 + 2.0 ** -41, 3.0, 3.0 + 2.0 ** -30, -3.0, -3.0 - 2.0 ** -30, 1e38, -1e38, 0.0, -0.0]
    cells = rs.permutation(kept)[:2 * len(vals)]
    V[cells, 6] = np.r_[vals, vals]
    S[cells, 6] = True
    # 7: a NaN in a kept cell
    at = rs.rand(n) < 0.3
    V[at, 7] = rs.randint(1, 5, size=int(at.sum()))
    S[at, 7] = True
    V[kept[7], 7] = np.nan
    S[kept[7], 7] = True
    # 8: a NaN only in a left-out cell
    at = rs.rand(n) < 0.3
    V[at, 8] = rs.randint(1, 5, size=int(at.sum())) * (1 - 2 * (rs.rand(int(at.sum())) < 0.3))
    S[at, 8] = True
    V[left[3], 8] = np.nan
    S[left[3], 8] = True
    V.setflags(write=False)
    S.setflags(write=False)
    return V, S


def sparse_of(V, S, fmt, dtype, index_dtype):
    """the stored entries of (V, S) as a canonical CSR / CSC matrix; explicit zeros and -0.0 stay stored"""
    r, c = np.nonzero(S)
    M = sp.csr_matrix((V[r, c].astype(dtype), (r, c)), shape=V.shape)         # row-major order of (r, c): no duplicates to sum
    assert M.nnz == int(S.sum())
    M = M.asformat(fmt)
    M.sort_indices()
    M.indices = M.indices.astype(index_dtype)
    M.indptr = M.indptr.astype(index_dtype)
    assert M.nnz == int(S.sum()) and M.dtype == dtype
    return M


def core_input(form):
    V, S = core_values()
    if form == 'csr-f32':
        return sparse_of(V, S, 'csr', np.float32, np.int32)
    if form == 'csc-f64':
        return sparse_of(V, S, 'csc', np.float64, np.int64)
    return np.ascontiguousarray(V.astype(np.float32 if form == 'dense-f32' else np.float64))


@functools.lru_cache(maxsize=None)
def core_reference(form, which='core'):
    """One restatement per stored type and code set: the sparse and the dense upload of one type hold the same values."""
    V, _ = core_values()
    L = {'core': CORE_LEVELS, 'one': 1, '1024': 1024}[which]
    out = restated_ranksum(V.astype(np.float32 if form.endswith('f32') else np.float64), core_codes(which), L)
    for a in out:
        a.setflags(write=False)
    return out


MID = (200001, 48, 32)


@functools.lru_cache(maxsize=None)
def mid_input():
    """200 001 x 48, sparse 5 %, small counts (many ties), 32 levels of unequal size; float32 CSR"""
    n, G, L = MID
    rs = np.random.RandomState(23)
    X = sp.random(n, G, density=0.05, format='csr', dtype=np.float32, random_state=rs,
                  data_rvs=lambda k: rs.geometric(0.3, size=k).astype(np.float32))
    X.sort_indices()
    w = np.arange(1, L + 1, dtype=np.float64) ** 2
    codes = rs.choice(L, size=n, p=w / w.sum()).astype(np.int32)
    codes[rs.rand(n) < 0.03] = -1
    return X, codes


def markers_input():
    """600 x 6 with a coef_populations-like categorical column ('pos1', 'neg1', 'pos2', NaN for the cells in none)"""
    rs = np.random.RandomState(2)
    n = 600
    lab = np.array(['pos1', 'neg1', 'pos2'], dtype=object)[rs.choice(3, size=n, p=[0.5, 0.3, 0.2])]
    lab[rs.rand(n) < 0.1] = None
    X = rs.poisson(1.0, size=(n, 6)).astype(np.float32)
    X[:, 0] += (lab == 'pos1') * rs.poisson(1.0, size=n)                     # a marker, |z| far below Z_MAX at this size
    X[:, 5] = rs.randn(n).astype(np.float32)                                 # no ties, negatives
    d = _frame(n, X=np.ascontiguousarray(X), pop=pd.Categorical(lab, categories=['pos1', 'pos2', 'neg1']))
    return d


def mannwhitney_table(Xd, codes, L, genes=None, levels=None):
    """{(level, gene): (U, z, p)} of scipy.stats.mannwhitneyu(x_in, x_rest, use_continuity=False, method='asymptotic'); z is
    recovered from scipy's own arithmetic (it returns U and p only)."""
    Xd = np.asarray(Xd, dtype=np.float64)
    out = {}
    kept = codes >= 0
    for b in (range(L) if levels is None else levels):
        for g in (range(Xd.shape[1]) if genes is None else genes):
            x, y = Xd[codes == b, g], Xd[kept & (codes != b), g]
            if len(x) == 0 or len(y) == 0 or np.isnan(x).any() or np.isnan(y).any() or np.ptp(np.r_[x, y]) == 0:
                continue
            res = scipy.stats.mannwhitneyu(x, y, use_continuity=False, method='asymptotic')
            out[(b, g)] = (float(res.statistic), float(res.pvalue))
    return out


def assert_matches_scipy(rank2, tie, n, nan, table):
    """U exact; z within Z_MAX (asserted) and checked through p to P_RTOL"""
    from cna_amd.tools._gene_markers import ranksum_statistics
    stats = ranksum_statistics(rank2, tie, n, nan)
    assert table
    for (b, g), (u, p) in table.items():
        assert stats[b, 1, g] == u, (b, g)
        assert abs(stats[b, 2, g]) <= Z_MAX, (b, g, stats[b, 2, g])
        assert abs(stats[b, 3, g] - p) <= P_RTOL * p, (b, g, stats[b, 3, g], p)
    return stats


# ------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize('form', ['dense-f32', 'dense-f64'])
def test_restatement_is_mannwhitneyu_on_the_core_input(form):
    codes = core_codes()
    rank2, tie, n, nan = core_reference(form)
    assert list(n) == [int((codes == b).sum()) for b in range(3)] + [0] and list(np.flatnonzero(nan)) == [7]
    table = mannwhitney_table(core_input(form), codes, CORE_LEVELS)
    assert {g for _, g in table} == {1, 3, 4, 6, 8} and {b for b, _ in table} == {0, 1, 2}
    assert_matches_scipy(rank2, tie, n, nan, table)
    m = int(n.sum())
    np.testing.assert_array_equal(rank2[:, 2], n * (m + 1))                  # the constant gene: every cell has the midrank
    np.testing.assert_array_equal(rank2[:, 0], n * (m + 1))
    np.testing.assert_array_equal(rank2[:, 5], n * (m + 1))                  # its only entry is left out
    assert tie[0] == tie[2] == tie[5] == float(m ** 3 - m)
    assert rank2[:, [0, 1, 2, 3, 4, 5, 6, 8]].sum(axis=0).tolist() == [m * (m + 1)] * 8       # all ranks: 2 (1 + ... + m)
    assert tie[1] == 0.0


def test_float32_collisions_tie_only_in_float32():
    t32, t64 = core_reference('dense-f32')[1], core_reference('dense-f64')[1]
    assert t32[6] > t64[6] > 0 and np.array_equal(np.delete(t32, 6), np.delete(t64, 6))
    assert not np.array_equal(core_reference('dense-f32')[0][:, 6], core_reference('dense-f64')[0][:, 6])


def test_restatement_is_mannwhitneyu_on_the_other_inputs():
    X, codes = mid_input()
    L = MID[2]
    assert len(set(np.bincount(codes[codes >= 0], minlength=L))) > L // 2 and (codes < 0).sum() > 0
    genes, levels = [0, 17, 47], [0, 31]
    sub = X[:, genes].toarray()
    rank2, tie, n, nan = restated_ranksum(sub, codes, L)
    table = mannwhitney_table(sub, codes, L, levels=levels)
    assert len(table) == 6
    assert_matches_scipy(rank2, tie, n, nan, table)
    d = markers_input()
    pcodes, plevels = pd.factorize(d.obs['pop'])
    out = restated_ranksum(d.X, pcodes, len(plevels))
    assert_matches_scipy(*out, mannwhitney_table(d.X, pcodes, len(plevels)))
    for which, Lw in (('one', 1), ('1024', 1024)):
        rank2, tie, n, nan = core_reference('dense-f64', which)
        assert rank2.shape == (Lw, 9) and n.sum() == (core_codes() >= 0).sum()
        np.testing.assert_array_equal(tie, core_reference('dense-f64')[1])


# ------------------------------------------------------------------ proofs about the GPU inputs
def sort_chunks(form):
    """Chunks of every gene in the radix sort: build_chunks' pieces of the stored lists, RS_DENSE_CHUNK cells of the dense form"""
    X = core_input(form)
    if sp.issparse(X):
        return -(-np.diff(sp.csc_matrix(X).indptr).astype(np.int64) // chunk_length(int(X.nnz))), chunk_length(int(X.nnz))
    length = ranksum_constant('RS_DENSE_CHUNK')
    return np.full(X.shape[1], -(-X.shape[0] // length)), length


@pytest.mark.parametrize('form', FORMS)
def test_long_genes_span_three_sort_chunks_the_last_one_ragged(form):
    chunks, length = sort_chunks(form)
    assert chunks[1] >= 3 and chunks[2] >= 3 and N_CORE % length != 0
    if form.startswith('cs'):
        assert chunks[0] == 0 and chunks[5] == 1


def ranksum_tiles(form, work_bytes, X=None):
    """ranksum_run: tiles of whole genes whose entries fit work_bytes / (2 * (key bytes + 2)), one gene at least; of the core
    input in that form, or of the matrix X of that form"""
    X = core_input(form) if X is None else X
    key = 4 if form.endswith('f32') else 8
    limit = max(1, (work_bytes or ranksum_constant('RS_WORK_BYTES')) // (2 * (key + 2)))
    length = np.diff(sp.csc_matrix(X).indptr) if sp.issparse(X) else np.full(X.shape[1], X.shape[0])
    seg = np.r_[0, np.cumsum(length)]
    tiles, g0, G = [], 0, len(length)
    while g0 < G:
        g1 = g0 + 1
        while g1 < G and seg[g1 + 1] - seg[g0] <= limit:
            g1 += 1
        tiles.append((g0, g1))
        g0 = g1
    return tiles, limit, length


@pytest.mark.parametrize('form', FORMS)
def test_the_small_budget_cuts_at_least_two_tiles(form):
    tiles, limit, length = ranksum_tiles(form, SMALL_WORK_BYTES)
    assert len(tiles) >= 2 and tiles[0][0] == 0 and tiles[-1][1] == 9
    assert len(ranksum_tiles(form, 0)[0]) == 1
    if form.endswith('f64'):
        assert length[1] > limit                       # a gene that alone exceeds the budget: still one tile


@pytest.mark.parametrize('form', FORMS)
def test_tie_runs_meet_the_cuts_of_the_rank_unit(form):
    """The rank kernel takes the sorted kept entries of a gene RS_UNIT at a time.  Gene 4: the run of -2.0 ends exactly on a
    cut with another value behind it, the run of -1.0 spans two cuts; gene 2 is one run across every cut."""
    unit = ranksum_constant('RS_UNIT')
    V, S = core_values()
    kept = core_codes() >= 0
    use = kept if form.startswith('dense') else kept & S[:, 4]
    col = np.sort(V[use, 4].astype(np.float32 if form.endswith('f32') else np.float64))
    heads = np.flatnonzero(np.r_[True, col[1:] != col[:-1]])
    ends = np.r_[heads[1:], len(col)]
    runs = {float(col[h]): (int(h), int(e)) for h, e in zip(heads, ends)}
    lo, hi = runs[-2.0]
    assert lo == 0 and hi % unit == 0 and hi < len(col) and hi - lo > 1
    lo, hi = runs[-1.0]
    assert len([c for c in range(unit, len(col), unit) if lo < c < hi]) >= 2
    assert int(kept.sum()) > 3 * unit and S[:, 2].all()


# ------------------------------------------------------------------ the public call
class MarkersEngine(GeneEngine):
    """GeneEngine (the real residency code, counted uploads) with the device calls as numpy."""

    def gene_ranksum_by(self, codes, n_levels, work_bytes=0):
        assert self.resident is not None
        return restated_ranksum(self.resident, codes, n_levels)

    def expr_to_bins(self, codes, n_bins, what):
        assert self.resident is not None
        return restated_bins(self.resident, codes, n_bins, what)


def test_gene_markers_through_the_public_call():
    import cna_amd as cna
    assert 'gene_markers' in cna.tl.__all__
    d, eng = markers_input(), MarkersEngine()
    d.var = pd.DataFrame(index=pd.Index(['g%d' % i for i in range(6)]))
    out = cna.tl.gene_markers(d, 'pop', engine=eng)
    levels = list(pd.unique(d.obs['pop'].dropna()))                           # first appearance, not the category order
    assert sorted(levels) == ['neg1', 'pos1', 'pos2'] and levels != ['pos1', 'pos2', 'neg1']
    assert isinstance(out, pd.DataFrame) and out.shape == (6, 27) and (out.dtypes == np.float64).all()
    assert out.index.equals(d.var_names) and list(out.columns.names) == ['pop', 'statistic']
    assert list(out.columns) == [(l, s) for l in levels for s in STATISTICS]  # level-major
    codes = pd.factorize(d.obs['pop'])[0]
    Xd = d.X.astype(np.float64)
    for b, l in enumerate(levels):
        ins, rest = codes == b, (codes >= 0) & (codes != b)
        for g in range(6):
            res = scipy.stats.mannwhitneyu(Xd[ins, g], Xd[rest, g], use_continuity=False, method='asymptotic')
            assert out[(l, 'u')].iloc[g] == res.statistic
            assert abs(out[(l, 'auc')].iloc[g] - res.statistic / (ins.sum() * rest.sum())) <= 1e-12
            assert abs(out[(l, 'z')].iloc[g]) <= Z_MAX
            assert abs(out[(l, 'p')].iloc[g] - res.pvalue) <= P_RTOL * res.pvalue
        from cna_amd.tools._gene_test import benjamini_hochberg
        np.testing.assert_array_equal(out[(l, 'q')].values, benjamini_hochberg(out[(l, 'p')].values))   # q inside the level
        np.testing.assert_allclose(out[(l, 'mean_in')].values, Xd[ins].mean(axis=0), rtol=1e-12)
        np.testing.assert_allclose(out[(l, 'mean_rest')].values, Xd[rest].mean(axis=0), rtol=1e-12)
        np.testing.assert_allclose(out[(l, 'frac_in')].values, (Xd[ins] > 0).mean(axis=0), rtol=1e-12)
        np.testing.assert_allclose(out[(l, 'frac_rest')].values, (Xd[rest] > 0).mean(axis=0), rtol=1e-12)
    assert out[('pos1', 'z')].iloc[0] > 5 and out[('pos1', 'auc')].iloc[0] > 0.6      # the planted marker
    assert list(out.attrs['n_cells'].values) == [int((codes == b).sum()) for b in range(3)]
    # without the tie correction: the plain variance m (m + 1) ... / 12; the tie-free gene does not move
    plain = cna.tl.gene_markers(d, 'pop', tie_correct=False, engine=eng)
    n, m = out.attrs['n_cells'].values.astype(float), float((codes >= 0).sum())
    for b, l in enumerate(levels):
        want = (out[(l, 'u')].values - n[b] * (m - n[b]) / 2) / np.sqrt(n[b] * (m - n[b]) * (m + 1) / 12)
        np.testing.assert_allclose(plain[(l, 'z')].values, want, rtol=1e-13)
        assert (np.abs(plain[(l, 'z')].values[:5]) < np.abs(out[(l, 'z')].values[:5])).all()
        assert abs(plain[(l, 'z')].iloc[5] - out[(l, 'z')].iloc[5]) <= 1e-12 * abs(out[(l, 'z')].iloc[5])
        np.testing.assert_array_equal(plain[(l, 'u')].values, out[(l, 'u')].values)
    assert len(eng.uploads) == 1
    d.var = None
    assert isinstance(cna.tl.gene_markers(d, 'pop', engine=eng).index, pd.RangeIndex)


def test_nan_rules():
    import cna_amd as cna
    V, _ = core_values()
    rank_cols = ['auc', 'u', 'z', 'p', 'q']
    d = _frame(N_CORE, X=np.ascontiguousarray(V), lev=np.where(core_codes() >= 0, core_codes(), np.nan))
    out = cna.tl.gene_markers(d, 'lev', engine=MarkersEngine())
    assert out.shape == (9, 27)
    for l in out.columns.levels[0]:
        for s in rank_cols:
            col = out[(l, s)].values
            assert np.isnan(col[[0, 2, 5, 7]]).all(), (l, s)                  # constant over the kept cells; a kept NaN
            assert np.isfinite(col[[1, 3, 4, 6, 8]]).all(), (l, s)            # a NaN in a left-out cell does no harm
        assert np.isfinite(out[(l, 'mean_in')].values[[0, 1, 2, 3, 4, 5, 8]]).all()
    # one level holds every kept cell: every rank statistic is NaN, the means of the level are not
    one = _frame(N_CORE, X=np.ascontiguousarray(V), lev=np.where(core_codes() >= 0, 'all', None))
    out1 = cna.tl.gene_markers(one, 'lev', engine=MarkersEngine())
    assert out1.shape == (9, 9) and np.isnan(out1[[('all', s) for s in rank_cols]].values).all()
    assert np.isfinite(out1[('all', 'mean_in')].values[:6]).all()
    # an empty level (a code the engine is asked for and no cell has) through the statistics directly
    from cna_amd.tools._gene_markers import ranksum_statistics
    st = ranksum_statistics(*core_reference('dense-f64'))
    assert st.shape == (4, 5, 9) and np.isnan(st[3]).all() and np.isfinite(st[:3, :, 1]).all()


def test_bad_arguments_and_refusals():
    import cna_amd as cna
    from cna_amd import dist, synth
    d, eng = markers_input(), MarkersEngine()
    n = len(d.obs)
    wide = np.ascontiguousarray(np.arange(2200, dtype=np.float32).reshape(1100, 2) % 7)
    with pytest.raises(KeyError, match='louvain'):
        cna.tl.gene_markers(d, 'louvain', engine=eng)
    with pytest.raises(ValueError, match='1025 levels'):
        cna.tl.gene_markers(_frame(1100, X=wide, lev=np.arange(1100) % 1025), 'lev', engine=eng)
    with pytest.raises(ValueError, match='0 levels'):
        cna.tl.gene_markers(_frame(n, X=d.X, lev=np.full(n, np.nan)), 'lev', engine=eng)
    with pytest.raises(KeyError):
        cna.tl.gene_markers(d, 'pop', layer='missing', engine=eng)
    with pytest.raises(NotImplementedError, match='multi-rank'):
        cna.tl.gene_markers(d, 'pop', engine=MarkersEngine(nranks=2))
    data, _ = synth.make_demo_like(n_samples=20, n_genes=30, cells_per_sample=100, seed=3, keep_expression=True)
    part = dist.shard(data, rank=0, nranks=2)
    part.X = data.X[:len(part.obs)]
    part.obs['lev'] = 'a'
    with pytest.raises(NotImplementedError, match='sharded'):
        cna.tl.gene_markers(part, 'lev', engine=eng)
    assert eng.uploads == []
    assert cna.tl.gene_markers(_frame(1100, X=wide, lev=np.arange(1100) % 1024), 'lev', engine=eng).shape == (2, 1024 * 9)


def test_entry_is_declared():
    from cna_amd import _ffi
    assert 'cna_gene_ranksum_by' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'cna_gene_ranksum_by')
    from cna_amd.engine import Engine
    assert callable(Engine.gene_ranksum_by)
