"""``cna.tl.gene_markers``: exact Wilcoxon rank-sum marker genes of every level of a clustering, on the device.

``cna.tl.coef_populations`` ends on a categorical column (``'pos1'``, ``'neg1'``, ...), ``cna.tl.coef_strata`` takes a
``leiden`` column; the first question of either is *what are these cells?* -- which genes mark each level against all other
cells.  The standard answer is the Mann-Whitney U of ``scanpy.tl.rank_genes_groups(method='wilcoxon')``, which ranks the
matrix gene by gene on the host.  Here the resident expression matrix is ranked once per gene over all kept cells on the
device (csrc/expr_ranksum.hip, ``cna_gene_ranksum_by``: a segmented radix sort, the implicit zeros of a sparse matrix one
tie group placed by arithmetic); a level's rank sum is the sum of those ranks over its cells, so one ranking serves every
level.  The device returns integers; this module is the host side only: the codes, the argument checks, the float64
arithmetic from those integers and the frame.
"""
import numpy as np
import pandas as pd
from scipy.special import erfc

from ..engine import get_engine
from ._gene_test import benjamini_hochberg
from ._genes import expression_of, gene_index
from ._nam import refuse_sharded
from ._strata import levels_of

STATISTICS = ['auc', 'u', 'z', 'p', 'q', 'mean_in', 'mean_rest', 'frac_in', 'frac_rest']


def _mannwhitney_block(u, na, nb, tie, dead, tie_correct):
    """float64[5, genes]: auc, u, z, p, q of the U statistics `u` of na cells against nb (floats that hold integers), `tie`
    the tie term over their union; NaN where `dead`.  The one statement of the float64 arithmetic of both frames."""
    m = na + nb
    pairs = na * nb
    T = tie if tie_correct else 0.0
    with np.errstate(all='ignore'):
        sd = np.sqrt(pairs / 12.0 * ((m + 1.0) - T / (m * (m - 1.0))))
        z = (u - pairs / 2.0) / sd
    p = erfc(np.abs(z) / np.sqrt(2.0))
    block = np.stack([u / pairs, u, z, p, p])
    block[:, dead] = np.nan
    block[4] = benjamini_hochberg(block[3])
    return block


def ranksum_statistics(rank2, tie, n, nan, tie_correct=True):
    """-> float64[levels, 5, genes]: auc, u, z, p, q from the integers of ``Engine.gene_ranksum_by``.  With m the kept
    cells and n_b those of level b: U = rank2 / 2 - n_b (n_b + 1) / 2, auc = U / (n_b (m - n_b)), z = (U - n_b (m - n_b) / 2)
    / sqrt(n_b (m - n_b) / 12 * ((m + 1) - T / (m (m - 1)))) with T = tie (0 without the correction), no continuity
    correction; p two-sided normal; q Benjamini-Hochberg over the genes of each level.  NaN for a level that is empty or holds
    every kept cell, for a gene that is constant over the kept cells and for a gene flagged `nan`."""
    rank2 = np.asarray(rank2, dtype=np.int64)
    n = np.asarray(n, dtype=np.int64)
    tie = np.asarray(tie, dtype=np.float64)
    L, G = rank2.shape
    m = float(n.sum())
    out = np.full((L, 5, G), np.nan)
    # one tie group holds every kept cell: the gene is constant (t^3 - t is exact here or far above the comparison's reach)
    dead = np.asarray(nan, dtype=bool) | (tie >= m * (m * m - 1.0)) | (m < 2)
    for b in range(L):
        nb = float(n[b])
        if nb == 0 or nb == m:
            continue
        u = rank2[b].astype(np.float64) / 2.0 - nb * (nb + 1.0) / 2.0
        out[b] = _mannwhitney_block(u, nb, m - nb, tie, dead, tie_correct)
    return out


def pair_statistics(u2, tie, n, nan, pairs, tie_correct=True):
    """-> float64[pairs, 5, genes]: auc, u, z, p, q from the integers of ``Engine.gene_ranksum_pairs``.  For the pair (a, b)
    with n_a, n_b cells and m = n_a + n_b: U = u2 / 2, auc = U / (n_a n_b), z = (U - n_a n_b / 2) / sqrt(n_a n_b / 12 *
    ((m + 1) - T / (m (m - 1)))) with T = tie (0 without the correction), no continuity correction; p two-sided normal; q
    Benjamini-Hochberg over the genes of the pair.  NaN where either level is empty, where the gene is constant over the
    cells of the two levels (tie >= m (m^2 - 1)) and for a gene flagged `nan`."""
    u2 = np.asarray(u2, dtype=np.int64)
    tie = np.asarray(tie, dtype=np.float64)
    n = np.asarray(n, dtype=np.int64)
    nan = np.asarray(nan, dtype=bool)
    out = np.full((len(pairs), 5, u2.shape[1]), np.nan)
    for k, (a, b) in enumerate(pairs):
        na, nb = float(n[a]), float(n[b])
        if na == 0 or nb == 0:
            continue
        m = na + nb
        dead = nan | (tie[k] >= m * (m * m - 1.0))
        out[k] = _mannwhitney_block(u2[k].astype(np.float64) / 2.0, na, nb, tie[k], dead, tie_correct)
    return out


def gene_markers(data, stratification, layer=None, tie_correct=True, engine=None):
    """Marker genes of each distinct value of ``data.obs[stratification]`` against all other cells that have a level: per
    gene and level ``scipy.stats.mannwhitneyu(x_in, x_rest, use_continuity=False, method='asymptotic')``, implicit zeros of
    a sparse matrix included, ranked exactly (midranks, float64 matrices on all 64 bits).  Levels in order of first
    appearance; cells whose level is NaN / None are left out of both sides; at most 1024 levels.

    The matrix is ``data.X`` or ``data.layers[layer]``, resident on the device and shared with ``gene_corr`` and the other
    gene tools.

    Returns a float64 DataFrame indexed by ``data.var_names`` (a ``RangeIndex`` when there are none) with a column
    MultiIndex ``(level, statistic)``, level-major, the statistics ``auc`` (U over the number of pairs: the probability that
    a cell of the level exceeds one of the rest, ties half), ``u``, ``z`` (normal approximation with the tie correction
    unless ``tie_correct=False``, no continuity correction), ``p`` (two-sided), ``q`` (Benjamini-Hochberg over the genes of
    the level), then ``mean_in, mean_rest`` and ``frac_in, frac_rest`` (the fraction of cells with x > 0) of the level and
    of the other kept cells.  ``auc, u, z, p, q`` are NaN for a level that is empty or holds every kept cell, for a gene that
    is constant over the kept cells and for a gene with a NaN in a kept cell.  ``frame.attrs['n_cells']``: a Series level ->
    cells.

    Not here: one level against another (``gene_markers_pairs``), exact small-sample p-values, log fold changes, sharded data."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_markers', 'the ranking runs over all cells of a gene: the rows of other ranks are elsewhere')
    codes, levels = levels_of(data.obs, stratification, 'gene_markers')
    L = len(levels)
    X = expression_of(data, layer, 'gene_markers')
    engine.ensure_expression(X)
    rank2, tie, n, nan = engine.gene_ranksum_by(codes, L)
    n = np.asarray(n, dtype=np.int64)
    table = np.full((L, len(STATISTICS), X.shape[1]), np.nan)
    table[:, :5] = ranksum_statistics(rank2, tie, n, nan, tie_correct=bool(tie_correct))
    m = n.sum()
    for k, what in ((5, 0), (7, 1)):                       # sums of x, then cells with x > 0; the rest = the total - the level
        sums, _ = engine.expr_to_bins(codes, L, what)
        sums = np.asarray(sums, dtype=np.float64)
        with np.errstate(all='ignore'):
            table[:, k] = sums / n[:, None]
            table[:, k + 1] = (sums.sum(axis=0)[None, :] - sums) / (m - n)[:, None]
    level_index = pd.Index(levels, name=stratification)
    columns = pd.MultiIndex.from_product([level_index, STATISTICS], names=[stratification, 'statistic'])
    out = pd.DataFrame(np.ascontiguousarray(table.reshape(L * len(STATISTICS), -1).T), index=gene_index(data, X.shape[1]),
                       columns=columns)
    out.attrs['n_cells'] = pd.Series(n, index=level_index)
    return out


PAIR_STATISTICS = ['auc', 'u', 'z', 'p', 'q', 'mean_in', 'mean_vs', 'frac_in', 'frac_vs']
MAX_PAIR_LEVELS = 64            # levels that take part in one call (csrc/expr_ranksum.hip: the accumulators live in LDS)
MAX_PAIRS = 2016                # ... and its pairs: every unordered pair of 64 levels


def _chosen_pairs(levels, pairs, reference, stratification):
    """[(index of level, index of versus)] into `levels`, from the caller's labels"""
    index = {l: i for i, l in enumerate(levels)}

    def find(label):
        if label not in index:
            raise ValueError('gene_markers_pairs: %r is no level of data.obs[%r]' % (label, stratification))
        return index[label]

    if pairs is not None and reference is not None:
        raise ValueError('gene_markers_pairs: give `pairs` or `reference`, not both')
    if reference is not None:
        ref = find(reference)
        chosen = [(i, ref) for i in range(len(levels)) if i != ref]
    elif pairs is not None:
        chosen = []
        for pair in pairs:
            if len(pair) != 2:
                raise ValueError('gene_markers_pairs: a pair is (level, versus), not %r' % (pair,))
            chosen.append((find(pair[0]), find(pair[1])))
    else:
        chosen = [(i, j) for i in range(len(levels)) for j in range(i + 1, len(levels))]
    if not chosen:
        raise ValueError('gene_markers_pairs: no pair to compare (an empty list, or a single level)')
    for a, b in chosen:
        if a == b:
            raise ValueError('gene_markers_pairs: the pair (%r, %r) compares a level with itself' % (levels[a], levels[b]))
    if len(set(chosen)) != len(chosen):
        raise ValueError('gene_markers_pairs: a pair is given twice')
    return chosen


def gene_markers_pairs(data, stratification, pairs=None, reference=None, layer=None, tie_correct=True, engine=None):
    """One level of ``data.obs[stratification]`` against another: per gene and pair ``(level, versus)``
    ``scipy.stats.mannwhitneyu(x_level, x_versus, use_continuity=False, method='asymptotic')``, implicit zeros of a sparse
    matrix included, ranked exactly -- what separates ``'pos1'`` from ``'neg1'``, where ``gene_markers`` says what each is
    against all other cells.  The order within the cells of two levels is their order within all cells, so the one ranking
    of ``gene_markers`` (a segmented radix sort on the device) serves every pair of the call
    (``cna_gene_ranksum_pairs``): 31 pairs take one sort, not 31.

    ``pairs``: a list of ``(level, versus)`` labels; or ``reference='neg1'``: every other level against that one (scanpy's
    ``rank_genes_groups(reference=...)``); with neither, every unordered pair of levels, in order of first appearance.
    Only the levels named in some pair take part: at most 64 of them and at most 2016 pairs in one call (the column itself
    may hold more levels).  A pair ``(b, a)`` may stand beside ``(a, b)``; an unknown label, a level against itself, a pair
    given twice and an empty list are refused.

    Returns a float64 DataFrame indexed like ``gene_markers``' with a column MultiIndex ``(level, versus, statistic)`` in
    pair order, the statistics ``auc`` (U over n_level * n_versus: the probability that a cell of the level exceeds one of
    the other, ties half), ``u``, ``z`` (normal approximation with the tie correction over the two levels' cells unless
    ``tie_correct=False``, no continuity correction), ``p`` (two-sided), ``q`` (Benjamini-Hochberg over the genes of the
    pair), then ``mean_in, mean_vs`` and ``frac_in, frac_vs`` (the fraction of cells with x > 0) of the two levels.
    ``auc, u, z, p, q`` are NaN where either level is empty, where the gene is constant over the cells of the two levels,
    and for a gene with a NaN in ANY cell of ANY level that takes part: such a gene is flagged for every pair of the call,
    also for the pairs whose own cells hold no NaN.  ``frame.attrs['n_cells']``: a Series level -> cells over the levels that
    take part.

    Measured (``profiles/kbench_gene_markers_pairs.txt``, 2 000 genes, 32 levels, float32): 1M cells at 5 % density take
    7.9 to 8.2 ms for 1, 31 or 496 pairs with all 32 levels taking part (the kernel behind the sort 3.8 ms of it), where one
    ``gene_ranksum_by`` per pair on recoded codes takes 4.3, 134 and 2 148 ms.  The kernel counts every level that takes
    part whatever the pairs, so ONE pair among 32 levels that take part is slower than that one recoded call: 1.8x on the
    sparse counts (1.7x at 200k cells), 3.7x on 200k dense cells of distinct floats, 5.8x on dense floats in tie runs of
    three.  There is no switch.  This function hands over only the levels its pairs name, and one pair with its two
    levels ties the recoded call (4.4 against 4.4 ms; 19.8 against 19.9 ms dense).

    Not here: exact small-sample p-values, log fold changes, sharded data, more than 64 levels in one call."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_markers_pairs',
                   'the ranking runs over all cells of a gene: the rows of other ranks are elsewhere')
    codes, levels = levels_of(data.obs, stratification, 'gene_markers_pairs', max_levels=np.iinfo(np.int32).max)
    levels = list(levels)
    chosen = _chosen_pairs(levels, pairs, reference, stratification)
    part = sorted({i for pair in chosen for i in pair})                       # the levels that take part, first appearance
    if len(part) > MAX_PAIR_LEVELS:
        raise ValueError('gene_markers_pairs: %d levels take part, at most %d can in one call' % (len(part), MAX_PAIR_LEVELS))
    if len(chosen) > MAX_PAIRS:
        raise ValueError('gene_markers_pairs: %d pairs, at most %d can go in one call' % (len(chosen), MAX_PAIRS))
    recode = np.full(len(levels) + 1, -1, dtype=np.int32)                     # the last entry: code -1 stays -1
    recode[part] = np.arange(len(part), dtype=np.int32)
    codes = np.ascontiguousarray(recode[codes])
    idx = np.ascontiguousarray([(recode[a], recode[b]) for a, b in chosen], dtype=np.int32)
    La, P = len(part), len(chosen)
    X = expression_of(data, layer, 'gene_markers_pairs')
    engine.ensure_expression(X)
    u2, tie, n, nan = engine.gene_ranksum_pairs(codes, La, idx)
    n = np.asarray(n, dtype=np.int64)
    table = np.full((P, len(PAIR_STATISTICS), X.shape[1]), np.nan)
    table[:, :5] = pair_statistics(u2, tie, n, nan, idx, tie_correct=bool(tie_correct))
    for k, what in ((5, 0), (7, 1)):                       # sums of x, then cells with x > 0
        sums, _ = engine.expr_to_bins(codes, La, what)
        with np.errstate(all='ignore'):
            means = np.asarray(sums, dtype=np.float64) / n[:, None]
        table[:, k] = means[idx[:, 0]]
        table[:, k + 1] = means[idx[:, 1]]
    columns = pd.MultiIndex.from_tuples([(levels[a], levels[b], s) for a, b in chosen for s in PAIR_STATISTICS],
                                        names=[stratification, 'versus', 'statistic'])
    out = pd.DataFrame(np.ascontiguousarray(table.reshape(P * len(PAIR_STATISTICS), -1).T), index=gene_index(data, X.shape[1]),
                       columns=columns)
    out.attrs['n_cells'] = pd.Series(n, index=pd.Index([levels[i] for i in part], name=stratification))
    return out
