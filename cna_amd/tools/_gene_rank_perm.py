"""``cna.tl.gene_rank_test``: permutation p-values for Spearman's rank correlation of every gene with the neighbourhood
coefficient.

``cna.tl.gene_rank_corr`` gives an exact Spearman rho per gene against the coefficient ``association`` stored.  Whether a
rho is more than a permuted phenotype would give is ``cna.tl.gene_test``'s question, asked of ranks: the null is the
association's own conditional permutations of the phenotype (reference _association.py:80-83, 94-99), and the null
coefficient of permutation p is ``c_p = X z_p`` per cell (_association.py:99, up to the factor 1 / N that no rank sees) with
X the residualised NAM -- the working matrix on the device.  ``gene_test`` never forms a ``c_p``: every sum a Pearson r
needs is linear or quadratic in ``z_p``.  Ranks are not, so here every ``c_p`` is formed, ranked over the kept cells and
correlated with every gene's ranks -- on the device, from one sort of the expression matrix for all permutations
(``Engine.gene_rank_corr_x``: csrc/expr_rankperm.hip).  This module is the host side: the association and its null
phenotypes (tools/_gene_null.py), the one float64 line from the device's integers (``rank_corr_statistics``) and the
permutation statistics (``permutation_stats`` of tools/_gene_test.py).

(The module is not called ``_gene_rank_test.py``: see the note at the top of tools/_gene_null.py.)
"""
import operator

import numpy as np
import pandas as pd

from ..engine import get_engine
from ._gene_null import null_phenotypes, warn_smallest_p
from ._gene_rank_corr import rank_corr_statistics
from ._gene_test import permutation_stats
from ._genes import expression_of, gene_index, key_columns
from ._nam import refuse_sharded


def checked_n_perm(n_perm, who):
    """None, or n_perm as an int >= 1 (``gene_rank_test`` and ``gene_rank_test_strata``: the cost is linear in it)"""
    if n_perm is None:
        return None
    try:
        n_perm = operator.index(None if isinstance(n_perm, (bool, np.bool_)) else n_perm)
    except TypeError:
        raise TypeError('%s: n_perm must be an integer >= 1 or None, got %r' % (who, n_perm)) from None
    if n_perm < 1:
        raise ValueError('%s: n_perm must be an integer >= 1 or None, got %r' % (who, n_perm))
    return n_perm


def gene_rank_test(data, y, sid_name, batches=None, covs=None, donorids=None, layer=None, key_added='coef', var_key_added=None,
                   n_perm=None, return_null=False, engine=None, **kwargs):
    """``association(data, y, sid_name, batches, covs, donorids, key_added=key_added, **kwargs)`` and, for every gene of
    ``data.X`` (or ``data.layers[layer]``; the matrices ``gene_rank_corr`` takes), Spearman's rho of its expression with the
    neighbourhood coefficient together with the same rho under the P = min(1000, Nnull) permuted phenotypes the
    association drew (same ``seed`` / same state of numpy's global generator, which is left where the association left
    it).  ``data.obs[key_added]`` and ``data.obs[key_added + '_fdr']`` are written as the association writes them;
    ``local_test=False`` is allowed (the FDR column is then not written).

    ``n_perm`` (an integer >= 1): use the first ``n_perm`` null phenotypes only.  Unlike ``gene_test``, whose null costs
    sample-space algebra, the cost here is LINEAR in P: every null coefficient is a per-cell column that is formed, ranked
    (one radix sort of the cells) and correlated with every gene's ranks, and its ranks stay on the device until the call
    ends, 4 bytes per cell and permutation.  The expression matrix itself is sorted once, whatever P is.

    Returns a DataFrame indexed like ``gene_rank_corr``'s: ``rho`` (equal to ``gene_rank_corr(data, key_added)``, bit for
    bit), ``null_mean``, ``null_sd``, ``z`` = (rho - null_mean) / null_sd, ``p`` = (1 + #{|rho_p| >= |rho|}) / (P + 1),
    two-sided, ``q`` = Benjamini-Hochberg over the genes with a finite p.  ``frame.attrs['p']`` is the association's
    global p-value, ``attrs['n_null']`` is P and ``attrs['n_cells']`` the number of kept cells.  NaN rules are
    ``gene_rank_corr``'s: a gene that is constant over the kept cells, or has a NaN in a kept cell, is NaN in every column.
    ``return_null=True``: ``(frame, null_rho)`` with null_rho genes x P float64.  ``var_key_added='grt_'`` also writes
    ``data.var['grt_rho']``, ``['grt_p']``, ``['grt_q']``.  ``association``'s other keywords (ks, nsteps, Nnull, seed,
    force_permute_all, ...) pass through.

    The kept cells of rho are those where the stored coefficient is finite, the kept cells of the null those with a row in
    X: the same cells, and a RuntimeError if the two calls ever disagree on their number.

    Inside the levels of a clustering: ``gene_rank_test_strata``.  Not here: sharded data, Kendall's tau."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_rank_test', 'the ranking runs over all cells of a gene: the rows of other ranks are elsewhere')
    n_perm = checked_n_perm(n_perm, 'gene_rank_test')
    X = expression_of(data, layer, 'gene_rank_test')
    res, Zall, P = null_phenotypes(data, y, sid_name, batches, covs, donorids, key_added, engine, kwargs, 'gene_rank_test')
    if n_perm is not None:
        P = min(P, n_perm)

    engine.ensure_expression(X)
    s_lo, s_hi, tie_gene, tie_key, m, nan = engine.gene_rank_corr(key_columns(data.obs, key_added)[1])   # gene_rank_corr's call
    rho = np.ascontiguousarray(rank_corr_statistics(s_lo, s_hi, tie_gene, tie_key, m, nan)[0])
    Z = np.ascontiguousarray(Zall[:, 1:1 + P].T)                # P x samples: one row per null coefficient
    n_lo, n_hi, n_tie_gene, n_tie_key, n_m, n_nan = engine.gene_rank_corr_x(engine.x_row_of_cells(), Z)
    if int(n_m) != int(m):
        raise RuntimeError('gene_rank_test: the stored coefficient is finite in %d cells, the working matrix X has a row for %d: '
                           'the observed and the null correlations would rank different cells' % (int(m), int(n_m)))
    null_rho = np.ascontiguousarray(rank_corr_statistics(n_lo, n_hi, n_tie_gene, n_tie_key, n_m, n_nan).T)
    mean, sd, z, p, q = permutation_stats(rho, null_rho)

    warn_smallest_p(P, X.shape[1])
    gindex = gene_index(data, X.shape[1])
    out = pd.DataFrame({'rho': rho, 'null_mean': mean, 'null_sd': sd, 'z': z, 'p': p, 'q': q}, index=gindex,
                       columns=['rho', 'null_mean', 'null_sd', 'z', 'p', 'q'])
    out.attrs['p'] = res.p                                     # the association's global p-value, as a plain call returns it
    out.attrs['n_null'] = P
    out.attrs['n_cells'] = int(m)
    if var_key_added is not None:
        if getattr(data, 'var', None) is None:
            data.var = pd.DataFrame(index=gindex)
        for k in ('rho', 'p', 'q'):
            data.var['%s%s' % (var_key_added, k)] = out[k].values
    return (out, null_rho) if return_null else out
