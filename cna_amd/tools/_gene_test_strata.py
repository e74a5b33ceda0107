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

so ``null_correlations`` runs once per level, unchanged.  None of the sums depends on y: the engine keeps them
(``Engine.expr_cross_by``) and a further phenotype on the same covariates and clustering costs sample-space algebra only.
This module is the host side.
"""
import warnings

import numpy as np
import pandas as pd

from ..engine import get_engine
from . import _association as _assoc
from ._association import association, _draw_null
from ._gene_test import MAX_NULL, _digest, _expression, null_correlations, permutation_stats
from ._nam import shard_of

MAX_LEVELS = 1024
STATISTICS = ['r', 'null_mean', 'null_sd', 'z', 'p', 'q']


# ------------------------------------------------------------------ gene_test's pieces, as functions
def null_phenotypes(data, y, sid_name, batches, covs, donorids, key_added, engine, kwargs, who):
    """gene_test's steps up to the cells as one function (tools/_gene_test.py holds them inline, unchanged): the
    association (its FDR column optional: ``_tolerate.no_fdr``), then the null phenotypes it used -- the same draw again, numpy's generator put back afterwards.
    -> (res, Zall, P): the full result, samples x (1 + P) with the standardised observed phenotype first and the P =
    min(1000, Nnull) conditioned, standardised null phenotypes behind it."""
    for name in ('return_full', 'engine'):
        if name in kwargs:
            raise TypeError("%s() got an unexpected keyword argument '%s'" % (who, name))
    seed = kwargs.get('seed')
    Nnull = kwargs.get('Nnull', 1000)
    state0 = np.random.get_state() if seed is None else None
    _assoc._tolerate.no_fdr = True
    try:
        res = association(data, y, sid_name, batches=batches, covs=covs, donorids=donorids, key_added=key_added,
                          return_full=True, engine=engine, **kwargs)
    finally:
        _assoc._tolerate.no_fdr = False

    # the null phenotypes this association used: the same draw again, numpy's generator put back afterwards
    index = res.M.index
    yv = np.asarray(y.reindex(index).values, dtype=np.float64)
    bv = np.ones(len(index)) if batches is None else batches.reindex(index).values
    dv = None if donorids is None else donorids.reindex(index).values
    state1 = np.random.get_state()
    try:
        if state0 is not None:
            np.random.set_state(state0)
        y_std, y_null = _draw_null(yv, bv, dv, Nnull=Nnull, force_permute_all=kwargs.get('force_permute_all', False), seed=seed)
    finally:
        np.random.set_state(state1)
    P = min(MAX_NULL, int(Nnull))
    Mv = np.asarray(res.M, dtype=np.float64)
    Z = Mv @ np.asarray(y_null, dtype=np.float64)[:, :P]
    Z = Z / Z.std(axis=0, ddof=1)                              # _association.py:96-97 (pandas' std: ddof=1)
    # the observed phenotype: standardised, not residualised (_association.py:77) -- so that r is gene_corr's
    return res, np.column_stack([np.asarray(y_std, dtype=np.float64), Z]), P


def content_signature(engine, res, Gamma):
    """What this X was made from, for the engine's memos of the cell-sized sums: every association rebuilds X, so the
    engine's own key moves with every call; an equal signature of the NAM, the kept cells, the samples, the projector
    (covariates, batches, ridge) and the Gram matrix' bits says the rebuilt X is the same one.  No signature of the NAM:
    None, no carry-over."""
    if getattr(engine, '_nam_sig', None) is None:
        return None
    kept = np.asarray(res.kept, dtype=bool)
    return (repr(engine._nam_sig), len(kept), None if kept.all() else _digest(kept), tuple(map(str, res.M.index)),
            _digest(np.asarray(res.M, dtype=np.float64)), _digest(Gamma))


def warn_smallest_p(P, G):
    if 1.0 / (P + 1) > 0.05 / G:
        warnings.warn(('the smallest p-value {} permutations can give, {:.3g}, is above 0.05 / {} genes. ' +
                       'Consider increasing Nnull').format(P, 1.0 / (P + 1), G))


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


def strata_frame(table, levels, stratification, gindex):
    """genes x MultiIndex (level, statistic), level-major"""
    L, S, G = table.shape
    columns = pd.MultiIndex.from_product([pd.Index(levels, name=stratification), STATISTICS],
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

    Levels in order of first appearance (``pd.factorize``); cells whose level is NaN / None are left out; at most 1024
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
    if shard_of(data) is not None or int(getattr(engine, 'nranks', 1)) > 1:
        raise NotImplementedError('gene_test_strata does not take sharded data or a multi-rank engine yet (the per-level '
                                  'sums add over row blocks: one all-reduce away).')
    obs = data.obs
    if stratification not in obs:
        raise KeyError(stratification)
    codes, levels = pd.factorize(obs[stratification])           # first appearance; NaN / None -> -1
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError('gene_test_strata: data.obs[%r] has %d levels, must lie in [1, %d]'
                         % (stratification, len(levels), MAX_LEVELS))
    codes = np.ascontiguousarray(codes, dtype=np.int32)
    L = len(levels)
    X = _expression(data, layer)
    res, Zall, P = null_phenotypes(data, y, sid_name, batches, covs, donorids, key_added, engine, kwargs, 'gene_test_strata')

    engine.ensure_expression(X)
    content = content_signature(engine, res, engine.gram_held())
    sums = engine.expr_cross_by(codes, L, content=content)
    # constant genes, decided as gene_corr_strata decides them (exactly: minimum == maximum over the level's kept cells) --
    # by gene_corr_by itself, against a column that is finite on the kept cells and varies there.  They depend on E, the
    # kept cells and the clustering only, so the mask is kept beside the sums
    extra = engine.cross_by_extra()
    constant = extra.get('constant')
    if constant is None:
        kept = np.asarray(res.kept, dtype=bool)
        probe = np.where(kept, np.arange(len(kept), dtype=np.float64), np.nan)
        constant = np.isnan(engine.gene_corr_by(probe[None, :], codes, L, want_within=False)[0][0])
        extra['constant'] = constant
    table, null_r = level_statistics(sums, Zall, constant)

    G = X.shape[1]
    warn_smallest_p(P, G)
    gindex = getattr(data, 'var_names', None)
    if gindex is None or len(gindex) != G:
        gindex = pd.RangeIndex(G)
    out = strata_frame(table, levels, stratification, gindex)
    out.attrs['p'] = res.p                                     # the association's global p-value, as a plain call returns it
    out.attrs['n_null'] = P
    out.attrs['n_cells'] = pd.Series(np.asarray(sums[4], dtype=np.int64), index=pd.Index(levels, name=stratification))
    return (out, null_r) if return_null else out
