"""``cna.tl.gene_rank_test_strata``: permutation p-values for Spearman's rank correlation of every gene with the
neighbourhood coefficient inside every level of a clustering.

``cna.tl.gene_rank_corr_strata`` gives an exact Spearman rho per gene and level, and no measure of significance; inside a
cluster -- few cells, a smooth coefficient -- a rho of 0.1-0.3 is common under a permuted phenotype too, so it cannot be
read without a null.  The null is ``gene_rank_test``'s (the association's own conditional permutations, reference
_association.py:80-83, 94-99; ``c_p = X z_p`` per cell), ranked inside the level: every ``c_p`` is formed once, ranked
inside every level and correlated with every gene's ranks there, all levels from one sort of the expression matrix
(``Engine.gene_rank_corr_x_by``: csrc/expr_rankperm.hip).  This module is the host side: the association and its null
phenotypes (tools/_gene_null.py), ``rank_corr_statistics`` on each level's integers and ``permutation_stats`` per level.

(The module is not called ``_gene_rank_test_strata.py``: see the note at the top of tools/_gene_null.py.)
"""
import numpy as np
import pandas as pd

from ..engine import get_engine
from ._gene_null import null_phenotypes, warn_smallest_p
from ._gene_rank_corr import MAX_LEVELS, rank_corr_statistics
from ._gene_rank_perm import checked_n_perm
from ._gene_test import permutation_stats
from ._gene_test_strata import strata_frame
from ._genes import expression_of, gene_index, key_columns
from ._nam import refuse_sharded
from ._strata import levels_of

STATISTICS = ['rho', 'null_mean', 'null_sd', 'z', 'p', 'q']


def gene_rank_test_strata(data, y, sid_name, stratification, batches=None, covs=None, donorids=None, layer=None,
                          key_added='coef', n_perm=None, return_null=False, engine=None, **kwargs):
    """``gene_rank_test`` inside each distinct value of ``data.obs[stratification]``: the association
    (``data.obs[key_added]`` and ``data.obs[key_added + '_fdr']`` are written as a plain call writes them;
    ``local_test=False`` is allowed) and, for every gene and every level, Spearman's rho of the gene with the neighbourhood
    coefficient over the level's kept cells -- ``gene_rank_corr_strata(data, stratification, key_added)``, bit for bit --
    together with the same rho under the P = min(1000, Nnull) permuted phenotypes the association drew (same ``seed`` /
    same state of numpy's global generator, which is left where the association left it).

    ``n_perm`` (an integer >= 1): use the first ``n_perm`` null phenotypes only; the cost is linear in P, as in
    ``gene_rank_test``, and the integers the device returns take 16 x levels x P x genes bytes on the host (taken in
    chunks of permutations within 1 GiB).  The expression matrix is sorted once per chunk, whatever the number of levels.

    Levels in order of first appearance; cells whose level is NaN / None are in no level; at most 255 levels.  Returns a
    float64 DataFrame indexed like ``gene_rank_corr``'s with a column MultiIndex ``(level, statistic)``, level-major, the
    statistics ``rho, null_mean, null_sd, z, p, q`` as in ``gene_rank_test``; ``q`` is Benjamini-Hochberg inside each level
    over the genes with a finite p.  ``frame.attrs``: ``p`` the association's global p-value, ``n_null`` = P, ``n_cells`` a
    Series level -> kept cells of the level.  NaN rules are ``gene_rank_corr_strata``'s (a gene that is constant on the
    level's kept cells; a gene with a NaN in a kept cell of any level, in every level), and a level with fewer than two
    kept cells is NaN throughout.  ``return_null=True``: ``(frame, null_rho)`` with null_rho float64 [levels, genes, P];
    without it the float64 null of one level is dropped before the next is formed.

    The kept cells of rho are the level's cells where the stored coefficient is finite, those of the null the level's
    cells with a row in X: the same cells, and a RuntimeError if the two calls ever disagree on a level's number.

    Not here: more than 255 levels, Kendall's tau, sharded data."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_rank_test_strata',
                   'the ranking runs over all cells of a level: the rows of other ranks are elsewhere')
    n_perm = checked_n_perm(n_perm, 'gene_rank_test_strata')
    if stratification not in data.obs:
        raise KeyError(stratification)
    codes, levels = levels_of(data.obs, stratification, 'gene_rank_test_strata', max_levels=MAX_LEVELS)
    L = len(levels)
    X = expression_of(data, layer, 'gene_rank_test_strata')
    res, Zall, P = null_phenotypes(data, y, sid_name, batches, covs, donorids, key_added, engine, kwargs, 'gene_rank_test_strata')
    if n_perm is not None:
        P = min(P, n_perm)

    engine.ensure_expression(X)
    # gene_rank_corr_strata's call
    s_lo, s_hi, tie_gene, tie_key, m, nan = engine.gene_rank_corr_by(key_columns(data.obs, key_added)[1], codes, L)
    Z = np.ascontiguousarray(Zall[:, 1:1 + P].T)                # P x samples: one row per null coefficient
    n_lo, n_hi, n_tie_gene, n_tie_key, n_m, n_nan = engine.gene_rank_corr_x_by(engine.x_row_of_cells(), Z, codes, L)
    m, n_m = np.asarray(m, dtype=np.int64), np.asarray(n_m, dtype=np.int64)
    if not np.array_equal(m, n_m):
        l = int(np.flatnonzero(m != n_m)[0])
        raise RuntimeError('gene_rank_test_strata: in level %r the stored coefficient is finite in %d cells, the working matrix X '
                           'has a row for %d: the observed and the null correlations would rank different cells'
                           % (levels[l], int(m[l]), int(n_m[l])))

    G = X.shape[1]
    table = np.full((L, len(STATISTICS), G), np.nan)
    null_all = np.full((L, G, P), np.nan) if return_null else None
    for l in range(L):
        if m[l] < 2:
            continue
        table[l, 0] = rank_corr_statistics(s_lo[l], s_hi[l], tie_gene[l], tie_key[l], int(m[l]), nan)[0]
        null_rho = np.ascontiguousarray(rank_corr_statistics(n_lo[l], n_hi[l], n_tie_gene[l], n_tie_key[l], int(m[l]), n_nan).T)
        table[l, 1:] = permutation_stats(table[l, 0], null_rho)
        if return_null:
            null_all[l] = null_rho

    warn_smallest_p(P, G)
    level_index = pd.Index(levels, name=stratification)
    out = strata_frame(table, levels, stratification, gene_index(data, G), statistics=STATISTICS)
    out.attrs['p'] = res.p                                     # the association's global p-value, as a plain call returns it
    out.attrs['n_null'] = P
    out.attrs['n_cells'] = pd.Series(m, index=level_index)
    return (out, null_all) if return_null else out
