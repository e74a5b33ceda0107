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
        pairs = nb * (m - nb)
        u = rank2[b].astype(np.float64) / 2.0 - nb * (nb + 1.0) / 2.0
        T = tie if tie_correct else 0.0
        with np.errstate(all='ignore'):
            sd = np.sqrt(pairs / 12.0 * ((m + 1.0) - T / (m * (m - 1.0))))
            z = (u - pairs / 2.0) / sd
        p = erfc(np.abs(z) / np.sqrt(2.0))
        block = np.stack([u / pairs, u, z, p])
        block[:, dead] = np.nan
        out[b, :4] = block
        out[b, 4] = benjamini_hochberg(block[3])
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

    Not here: level-against-level comparisons, exact small-sample p-values, log fold changes, sharded data."""
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
