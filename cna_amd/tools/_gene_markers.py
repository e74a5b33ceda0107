"""``cna.tl.gene_markers``: exact Wilcoxon rank-sum marker genes of every level of a clustering, on the device.

``cna.tl.coef_populations`` ends on a categorical column (``'pos1'``, ``'neg1'``, ...), ``cna.tl.coef_strata`` takes a
``leiden`` column; the first question of either is *what are these cells?* -- which genes mark each level against all other
cells.  The standard answer is the Mann-Whitney U of ``scanpy.tl.rank_genes_groups(method='wilcoxon')``, which ranks the
matrix gene by gene on the host.  Here the resident expression matrix is ranked once per gene over all kept cells on the
device (csrc/expr_ranksum.hip, ``cna_gene_ranksum_by``: a segmented radix sort, the implicit zeros of a sparse matrix one
tie group placed by arithmetic); a level's rank sum is the sum of those ranks over its cells, so one ranking serves every
level.  The device returns integers; this module is the host side only: the codes, the argument checks, the float64
arithmetic from those integers and the frame.

``cna.tl.gene_markers_pairs`` compares one level with another from the same ranking; ``cna.tl.gene_markers_within`` ranks
inside every block of a second column (the sample, the batch) and combines the blocks: the stratified test, for levels that
are unevenly spread over the samples (``cna_gene_ranksum_within``: one more pass of the sort on the block).
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


WITHIN_STATISTICS = ['auc', 'z', 'p', 'q', 'blocks']
WITHIN_WEIGHTS = ('van_elteren', 'sum')
MAX_BLOCKS = 255                # cna_gene_ranksum_within: the block is one digit of the sort, 255 stands for a left-out entry


def within_weights(n, weights='van_elteren'):
    """From n int64[blocks, levels], the kept cells n_sl, and n_s their sum over the levels -> (a float64[blocks]: the weight
    of a block's centred rank sums, 1 / (n_s + 1) for 'van_elteren' and 1 for 'sum'; c float64[blocks, levels]: the weight of
    a block's tie term in the level's variance, a_s^2 n_sl (n_s - n_sl) / (12 n_s (n_s - 1)), exactly 0.0 where n_sl is 0 or
    n_s; V0 float64[levels] = sum_s a_s^2 n_sl (n_s - n_sl) (n_s + 1) / 12, the variance without ties; pairs float64[levels]
    = sum_s n_sl (n_s - n_sl), the (level, rest) pairs of cells inside a block)."""
    if weights not in WITHIN_WEIGHTS:
        raise ValueError('gene_markers_within: weights must be one of %s, not %r' % (', '.join(map(repr, WITHIN_WEIGHTS)), weights))
    n = np.asarray(n, dtype=np.float64)
    ns = n.sum(axis=1)
    a = 1.0 / (ns + 1.0) if weights == 'van_elteren' else np.ones(len(ns))
    cross = n * (ns[:, None] - n)                                             # 0 where the level is absent or the whole block
    with np.errstate(all='ignore'):
        c = a[:, None] ** 2 * cross / (12.0 * ns * (ns - 1.0))[:, None]
    c[cross == 0] = 0.0                                                       # (n_s = 0 and n_s = 1 among them: 0 / 0)
    V0 = (a[:, None] ** 2 * cross * (ns[:, None] + 1.0) / 12.0).sum(axis=0)
    return a, np.ascontiguousarray(c), V0, cross.sum(axis=0)


def within_statistics(d2, num, tiew, live, n, nan, weights='van_elteren', tie_correct=True):
    """-> float64[levels, 5, genes]: auc, z, p, q, blocks from the numbers of ``Engine.gene_ranksum_within`` called with
    ``within_weights(n, weights)``.  Per level l and gene: auc = 0.5 + d2 / (2 pairs_l), the share of the (level, rest) pairs
    of cells inside one block in which the level's cell is higher, ties half; z = (num / 2) / sqrt(V0_l - tiew) with tiew
    taken as 0 without the tie correction, no continuity correction; p two-sided normal; q Benjamini-Hochberg over the
    genes of the level; blocks = live.  All but blocks are NaN where pairs_l = 0 (in every block the level is absent or
    alone), where live = 0 (the gene is constant in every block that could tell) and for a gene flagged `nan`."""
    d2 = np.asarray(d2, dtype=np.int64)
    num = np.asarray(num, dtype=np.float64)
    tiew = np.asarray(tiew, dtype=np.float64)
    live = np.asarray(live)
    _, _, V0, pairs = within_weights(n, weights)
    L, G = d2.shape
    out = np.full((L, 5, G), np.nan)
    out[:, 4] = live
    for b in range(L):
        if pairs[b] == 0:
            continue
        dead = np.asarray(nan, dtype=bool) | (live[b] == 0)
        with np.errstate(all='ignore'):
            z = (num[b] / 2.0) / np.sqrt(V0[b] - (tiew[b] if tie_correct else 0.0))
        p = erfc(np.abs(z) / np.sqrt(2.0))
        block = np.stack([0.5 + d2[b].astype(np.float64) / (2.0 * pairs[b]), z, p, p])
        block[:, dead] = np.nan
        block[3] = benjamini_hochberg(block[2])
        out[b, :4] = block
    return out


def gene_markers_within(data, stratification, within, weights='van_elteren', layer=None, tie_correct=True, engine=None):
    """Marker genes of each distinct value of ``data.obs[stratification]`` against the other cells OF THE SAME BLOCK of
    ``data.obs[within]`` (the sample, the donor, the batch): the stratified Wilcoxon rank-sum test, van Elteren's test.  The
    cells are ranked inside each block, the level is compared with the rest inside each block, and the blocks are combined:
    with R_sl the level's rank sum inside block s, n_s the block's cells and n_sl the level's among them,
    z = sum_s a_s (R_sl - n_sl (n_s + 1) / 2) / sqrt(sum_s a_s^2 Var_s), Var_s the rank sum's variance inside the block with
    its tie correction, and a_s = 1 / (n_s + 1) (``weights='van_elteren'``, the locally most powerful choice when the shift
    is the same in every block) or a_s = 1 (``weights='sum'``: the blocks' U statistics added up, large blocks dominate).

    Prefer it over ``gene_markers`` whenever the levels are unevenly spread over samples or batches -- the populations of
    ``coef_populations`` are, by construction: an association with a sample-level phenotype means over-representation in
    some samples.  ``gene_markers`` pools all cells into one ranking, so a gene whose baseline differs between donors or
    batches (ambient RNA, a batch shift, a genotype) comes out as a marker of the population although it separates the
    population's cells from their neighbours in no single sample; here such a gene has auc 0.5 and z 0.  A block in which a
    level is absent, or holds every cell, says nothing about that level and drops out of its sums.

    Levels and blocks in order of first appearance; a cell with NaN / None in either column is left out; at most 1024 levels
    and 255 blocks.  The matrix is ``data.X`` or ``data.layers[layer]``, resident on the device and shared with the other
    gene tools; every gene is sorted once, by value and then by block (``cna_gene_ranksum_within``), whatever the number of
    blocks, and the implicit zeros of a sparse matrix take part.

    Returns a float64 DataFrame indexed by ``data.var_names`` (a ``RangeIndex`` when there are none) with a column
    MultiIndex ``(level, statistic)``, level-major, the statistics ``auc`` (the share of the (level's cell, other cell) pairs
    inside one block in which the level's cell is higher, ties half: 0.5 + the summed centred U over the number of such
    pairs, whatever the weights), ``z`` (normal approximation, tie-corrected unless ``tie_correct=False``, no continuity
    correction), ``p`` (two-sided), ``q`` (Benjamini-Hochberg over the genes of the level) and ``blocks`` (the blocks that
    hold the level and other cells and in which the gene is not constant).  ``auc, z, p, q`` are NaN for a level without
    such a pair in any block, for a gene with ``blocks`` = 0 and for a gene with a NaN in a kept cell.
    ``frame.attrs['n_cells']``: a Series level -> kept cells; ``frame.attrs['counts']``: the blocks x levels frame of kept
    cells.

    Measured (``profiles/kbench_gene_markers_within.txt``, 2 000 genes, 32 levels, float32): 1M cells at 5 % density take
    11.2 ms in 50 blocks and 13.7 ms in 200, where the pooled ``gene_ranksum_by`` call takes 5.7 ms and one such call per
    block on masked codes 215.8 ms at 50 blocks; 200k dense cells 68.7 and 78.3 ms against 52.9 and 749.2 ms.

    Not here: means and fractions (``gene_markers`` has them), more than 255 blocks (coarsen samples to batches), one level
    against another inside the blocks, exact small-sample p-values (the normal approximation needs the combined blocks to
    be large, not each one), sharded data."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_markers_within',
                   'the ranking runs over all cells of a block: the rows of other ranks are elsewhere')
    if weights not in WITHIN_WEIGHTS:
        raise ValueError('gene_markers_within: weights must be one of %s, not %r' % (', '.join(map(repr, WITHIN_WEIGHTS)), weights))
    codes, levels = levels_of(data.obs, stratification, 'gene_markers_within')
    blocks, block_levels = levels_of(data.obs, within, 'gene_markers_within', max_levels=MAX_BLOCKS)
    L, B = len(levels), len(block_levels)
    kept = (codes >= 0) & (blocks >= 0)
    counts = np.bincount(blocks[kept].astype(np.int64) * L + codes[kept], minlength=B * L).reshape(B, L).astype(np.int64)
    a, c, _, _ = within_weights(counts, weights)
    X = expression_of(data, layer, 'gene_markers_within')
    engine.ensure_expression(X)
    d2, num, tiew, live, n, nan = engine.gene_ranksum_within(codes, L, blocks, B, a, c)
    assert np.array_equal(np.asarray(n, dtype=np.int64), counts), 'gene_markers_within: the device counted other cells than the host'
    table = within_statistics(d2, num, tiew, live, counts, nan, weights=weights, tie_correct=bool(tie_correct))
    level_index = pd.Index(levels, name=stratification)
    columns = pd.MultiIndex.from_product([level_index, WITHIN_STATISTICS], names=[stratification, 'statistic'])
    out = pd.DataFrame(np.ascontiguousarray(table.reshape(L * len(WITHIN_STATISTICS), -1).T), index=gene_index(data, X.shape[1]),
                       columns=columns)
    out.attrs['n_cells'] = pd.Series(counts.sum(axis=0), index=level_index)
    out.attrs['counts'] = pd.DataFrame(counts, index=pd.Index(block_levels, name=within), columns=level_index)
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
