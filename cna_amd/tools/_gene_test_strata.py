"""``cna.tl.gene_test_strata``: permutation p-values for the per-gene correlations inside every level of a clustering.

``cna.tl.gene_corr_strata`` answers the question the violins of ``cna.tl.coef_strata`` raise (the reference's
``cna.pl.violinplot(d, 'leiden', key='coef')``, plotting/_strat.py:21-29) -- which genes separate the expanded from the
depleted cells of one cluster -- with a Pearson r per gene and level, and no measure of significance.  A cluster has far fewer
cells than the dataset, its coefficient a narrow range, smoothed over the same kNN graph as everything else: within-cluster
r values of 0.1-0.3 appear for hundreds of genes under a permuted phenotype as well.  The null is ``gene_test``'s (reference
_association.py:80-83, 94-99: ``c_p = R^T z_p / N``), restricted to the level's kept cells C_l; every cell-sized sum is
linear or quadratic in ``z_p`` there too (tools/_gene_test.py), over the level's rows of X only::

    sum_{i in C_l} x_ig c_p[i] = (W_l[g] . z_p) / N         W_l     = E_{C_l}^T X_{C_l}    (cna_expr_cross_by)
    sum_{i in C_l} c_p[i]      = (rho_l . z_p) / N          rho_l   = column sums of X_{C_l}  (cna_matrix_to_bins)
    sum_{i in C_l} c_p[i]^2    = z_p^T Gamma_l z_p / N^2    Gamma_l = X_{C_l}^T X_{C_l}    (cna_gram_by)

so ``gene_test``'s own steps serve here (tools/_gene_null.py: ``null_phenotypes``, ``content_signature``,
``constant_genes``) and ``null_correlations`` runs once per level, unchanged.  None of the sums depends on y: the engine keeps them
(``Engine.expr_cross_by``) and a further phenotype on the same covariates and clustering costs sample-space algebra only.
This module is the host side.
"""
import numpy as np
import pandas as pd

from ..engine import get_engine
from ._gene_null import constant_genes, content_signature, null_phenotypes, warn_smallest_p
from ._gene_test import null_correlations, permutation_stats
from ._genes import expression_of, gene_index
from ._nam import refuse_sharded
from ._strata import levels_of

STATISTICS = ['r', 'null_mean', 'null_sd', 'z', 'p', 'q']


def level_statistics(sums, Zall, constant):
    """-> (table float64[levels, 6, genes] in the order of STATISTICS, null_r float64[levels, genes, P]) from the per-level
    sums (W, rho, sx, sxx, m, Gamma) of ``Engine.expr_cross_by``, the phenotypes Zall (samples x (1 + P), the observed one
    first) and the mask constant[level, gene] of the genes that do not vary on a level's kept cells.  A level with fewer
    than two kept cells is NaN throughout; q is Benjamini-Hochberg inside each level."""
    W, rho, sx, sxx, m, Gamma = sums
    L, G = np.asarray(sx).shape
    P = Zall.shape[1] - 1
    table = np.full((L, len(STATISTICS), G), np.nan)
    null_r = np.full((L, G, P), np.nan)
    for l in range(L):
        if m[l] < 2:
            continue
        r_all = null_correlations(W[l], rho[l], sx[l], sxx[l], m[l], Gamma[l], Zall)
        r_all[np.asarray(constant[l], dtype=bool)] = np.nan
        null_r[l] = r_all[:, 1:]
        table[l, 0] = r_all[:, 0]
        table[l, 1:] = permutation_stats(table[l, 0], null_r[l])
    return table, null_r


def strata_frame(table, levels, stratification, gindex, statistics=STATISTICS):
    """genes x MultiIndex (level, statistic), level-major; `statistics` names the table's second axis"""
    L, S, G = table.shape
    columns = pd.MultiIndex.from_product([pd.Index(levels, name=stratification), list(statistics)],
                                         names=[stratification, 'statistic'])
    return pd.DataFrame(np.ascontiguousarray(table.reshape(L * S, G).T), index=gindex, columns=columns)


def gene_test_strata(data, y, sid_name, stratification, batches=None, covs=None, donorids=None, layer=None,
                     key_added='coef', return_null=False, engine=None, **kwargs):
    """``gene_test`` inside each distinct value of ``data.obs[stratification]``: the association (``data.obs[key_added]``
    and ``data.obs[key_added + '_fdr']`` are written as a plain call writes them; ``local_test=False`` is allowed) and,
    for every gene and every level, the correlation r of the gene with the neighbourhood coefficient over the level's
    kept cells -- ``gene_corr_strata(data, stratification, key_added)`` -- together with the same correlation under the
    P' = min(1000, Nnull) permuted phenotypes the association drew (same ``seed`` / same state of numpy's global
    generator, which is left where the association left it).

    Levels in order of first appearance; cells whose level is NaN / None are left out; at most 1024
    levels.  Returns a float64 DataFrame indexed like ``gene_corr``'s with a column MultiIndex ``(level, statistic)``,
    level-major, the statistics ``r, null_mean, null_sd, z, p, q`` as in ``gene_test``; ``q`` is Benjamini-Hochberg inside
    each level over the genes with a finite p.  ``frame.attrs``: ``p`` the association's global p-value, ``n_null`` = P',
    ``n_cells`` a Series level -> cells of the level with a row in X.  A gene that is constant on a level's kept cells
    (decided exactly, minimum == maximum) is NaN there; a level with fewer than two kept cells is NaN throughout.
    ``return_null=True``: ``(frame, null_r)`` with null_r float64 [levels, genes, P'].

    The passes over the cells depend on the covariates, the batches and the clustering, not on y: the engine keeps
    their results, and a further phenotype costs sample-space algebra only.  When the per-level sums of all levels do
    not fit 1 GiB they are taken in groups of levels and not kept (``Engine.expr_cross_by``)."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_test_strata', 'the per-level sums add over row blocks: one all-reduce away')
    codes, levels = levels_of(data.obs, stratification, 'gene_test_strata')
    L = len(levels)
    X = expression_of(data, layer, 'gene_test_strata')
    res, Zall, P = null_phenotypes(data, y, sid_name, batches, covs, donorids, key_added, engine, kwargs, 'gene_test_strata')

    engine.ensure_expression(X)
    content = content_signature(engine, res, engine.gram_held())
    sums = engine.expr_cross_by(codes, L, content=content)
    # per level (gene_corr_by, as gene_corr_strata decides them): the mask depends on the clustering too, as the sums do
    constant = constant_genes(np.asarray(res.kept, dtype=bool), engine.cross_by_extra(),
                              lambda V: engine.gene_corr_by(V, codes, L, want_within=False)[0][0])
    table, null_r = level_statistics(sums, Zall, constant)

    warn_smallest_p(P, X.shape[1])
    out = strata_frame(table, levels, stratification, gene_index(data, X.shape[1]))
    out.attrs['p'] = res.p                                     # the association's global p-value, as a plain call returns it
    out.attrs['n_null'] = P
    out.attrs['n_cells'] = pd.Series(np.asarray(sums[4], dtype=np.int64), index=pd.Index(levels, name=stratification))
    return (out, null_r) if return_null else out
