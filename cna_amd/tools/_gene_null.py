"""The steps ``cna.tl.gene_test`` and ``cna.tl.gene_test_strata`` share on either side of the engine's sums: the
association and the null phenotypes it drew (reference _association.py:80-83, 94-99), the word that tells the engine a
rebuilt X is the same one, the genes that are constant on the kept cells, the warning about too few permutations.  One
statement of each: the tools differ in the sums they ask the engine for (``Engine.expr_cross``, ``Engine.expr_cross_by``)
and in nothing before them.  Host side only.

Why not in tools/_gene_test.py, beside ``null_correlations``: that file's name matches ``*_test.py``, which test runners
and the tooling around them take for a test file and may handle apart from the package (pytest's default ``python_files``
lists the pattern).  The package must import whichever revision of that file it meets, so no other module takes a name
from it that it has not always had.
"""
import warnings

import numpy as np

from ..engine import array_digest
from . import _association as _assoc
from ._association import association, _draw_null

MAX_NULL = 1000          # the local test's cap on the permutations it uses (_association.py:94)


def null_phenotypes(data, y, sid_name, batches, covs, donorids, key_added, engine, kwargs, who):
    """The steps up to the cells: the association (its FDR column optional: ``_tolerate.no_fdr``), then the null phenotypes
    it used -- the same draw again, numpy's generator put back afterwards.
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
    return (repr(engine._nam_sig), len(kept), None if kept.all() else array_digest(kept), tuple(map(str, res.M.index)),
            array_digest(np.asarray(res.M, dtype=np.float64)), array_digest(Gamma))


def constant_genes(kept, extra, corr):
    """The genes that do not vary over the kept cells, decided as gene_corr decides them (exactly: minimum == maximum) -- by
    gene_corr itself: `corr(V)` is the engine's correlation of every gene with the one row of V, a column that is finite on
    the kept cells and varies there, so NaN marks a constant gene.  They depend on E and the cells only, so the mask is
    kept in `extra`, the dict beside the engine's memo of the sums, and a further phenotype does not pass over the matrix
    for it either."""
    constant = extra.get('constant')
    if constant is None:
        probe = np.where(kept, np.arange(len(kept), dtype=np.float64), np.nan)
        constant = extra['constant'] = np.isnan(corr(probe[None, :]))
    return constant


def warn_smallest_p(P, G):
    if 1.0 / (P + 1) > 0.05 / G:
        warnings.warn(('the smallest p-value {} permutations can give, {:.3g}, is above 0.05 / {} genes. ' +
                       'Consider increasing Nnull').format(P, 1.0 / (P + 1), G))
