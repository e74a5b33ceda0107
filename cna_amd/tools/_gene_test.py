"""``cna.tl.gene_test``: permutation p-values for the per-gene correlations to the neighbourhood coefficient.

``cna.tl.gene_corr`` gives a Pearson r per gene against the coefficient ``association`` stored (demo/demo.ipynb,
"per-gene correlations to neighborhood coefficient").  Whether an r is more than a permuted phenotype would give is a
question about the samples, not about the cells, and the package has the null for it already: the conditional
permutations of the phenotype behind the local test (reference _association.py:80-83, 94-99).  The null coefficient of
permutation p is ``c_p = R^T z_p / N`` (_association.py:99; the observed one is _association.py:77) with R the
residualised NAM -- the working matrix X on the device -- and every cell-sized sum a correlation with ``c_p`` needs is
linear or quadratic in ``z_p``::

    sum_i x_ig c_p[i] = (W_g . z_p) / N        W   = E_K^T X   genes x samples   (cna_expr_cross, csrc/expr_cross.hip)
    sum_i c_p[i]      = (rho . z_p) / N        rho = column sums of X
    sum_i c_p[i]^2    = z_p^T Gamma z_p / N^2  Gamma = X^T X                     (the association's Gram matrix)

W depends on the dataset, the covariates and the batches, not on the phenotype: one pass over the cells, kept by the
engine (``Engine.expr_cross``), and the observed r and every null r of every gene are sample-space algebra, genes x
samples by samples x permutations.  The cells x permutations matrix is never formed.  This module is the host side.
"""
import warnings

import numpy as np
import pandas as pd

from ..engine import get_engine
from . import _association as _assoc
from ._association import association, _draw_null
from ._genes import check_expression
from ._nam import shard_of

MAX_NULL = 1000          # the local test's cap on the permutations it uses (_association.py:94)


def null_correlations(W, rho, sx, sxx, m, Gamma, Z):
    """r[g, p] = Pearson correlation over the m cells of gene g with the coefficient X z_p / N of column p of Z
    (samples x P), from the sample-space sums alone: W = E^T X (genes x samples), rho = column sums of X, sx / sxx =
    per-gene sums of x and x^2, Gamma = X^T X.  Centred first, against cancellation; float64 throughout.  A gene
    without variance in these sums, or a column whose coefficient has none, gives NaN (gene_test decides the constant
    genes exactly, with gene_corr's rule, on top of this)."""
    W, rho, Gamma, Z = (np.asarray(a, dtype=np.float64) for a in (W, rho, Gamma, Z))
    sx, sxx = np.asarray(sx, dtype=np.float64), np.asarray(sxx, dtype=np.float64)
    m = float(m)
    Wc = W - np.outer(sx / m, rho)
    Gc = Gamma - np.outer(rho, rho) / m
    num = Wc @ Z                                              # genes x P
    vc = np.einsum('sp,sp->p', Z, Gc @ Z)                     # P
    vx = sxx - sx * sx / m                                    # genes
    with np.errstate(all='ignore'):
        den = np.sqrt(vx[:, None] * vc[None, :])
        r = num / den
        r[~(den > 0)] = np.nan
    return np.clip(r, -1.0, 1.0)


def benjamini_hochberg(p):
    """Benjamini-Hochberg q-values over the finite entries of p (NaN stays NaN)."""
    p = np.asarray(p, dtype=np.float64)
    q = np.full(p.shape, np.nan)
    ok = np.flatnonzero(np.isfinite(p))
    if len(ok):
        order = ok[np.argsort(p[ok], kind='stable')]
        scaled = p[order] * len(ok) / np.arange(1, len(ok) + 1)
        q[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return q


def permutation_stats(r, null_r):
    """-> null_mean, null_sd (ddof=1), z, p, q of the observed r (genes) against null_r (genes x P); p is two-sided,
    (1 + #{|null| >= |r|}) / (P + 1); NaN wherever r is."""
    r = np.asarray(r, dtype=np.float64)
    null_r = np.asarray(null_r, dtype=np.float64)
    P = null_r.shape[1]
    with np.errstate(all='ignore'):
        mean = null_r.mean(axis=1) if P else np.full(len(r), np.nan)
        sd = null_r.std(axis=1, ddof=1) if P > 1 else np.full(len(r), np.nan)
        z = (r - mean) / sd
        hits = (np.abs(null_r) >= np.abs(r)[:, None]).sum(axis=1)
    p = (1.0 + hits) / (P + 1.0)
    p[~np.isfinite(r)] = np.nan
    return mean, sd, z, p, benjamini_hochberg(p)


def _expression(data, layer):
    if layer is None:
        X = getattr(data, 'X', None)
        if X is None:
            raise ValueError('data.X is missing: gene_test needs the expression matrix')
    else:
        layers = getattr(data, 'layers', None)
        if layers is None or layer not in layers:
            raise KeyError(layer)
        X = layers[layer]
    return check_expression(X, len(data.obs))


def _digest(a):
    import hashlib
    a = np.ascontiguousarray(a)
    return hashlib.blake2b(a.view(np.uint8).reshape(-1), digest_size=16).hexdigest()


def gene_test(data, y, sid_name, batches=None, covs=None, donorids=None, layer=None, key_added='coef', var_key_added=None,
              return_null=False, engine=None, **kwargs):
    """``association(data, y, sid_name, batches, covs, donorids, key_added=key_added, **kwargs)`` and, for every gene of
    ``data.X`` (or ``data.layers[layer]``; the matrices ``gene_corr`` takes), the correlation r of its expression with
    the neighbourhood coefficient together with the same correlation under the P' = min(1000, Nnull) permuted
    phenotypes the association drew (same ``seed`` / same state of numpy's global generator, which is left where the
    association left it).  ``data.obs[key_added]`` and ``data.obs[key_added + '_fdr']`` are written as the association
    writes them; ``local_test=False`` is allowed (the FDR column is then not written).

    Returns a DataFrame indexed like ``gene_corr``'s: ``r`` (equal to ``gene_corr(data, key_added)``), ``null_mean``,
    ``null_sd``, ``z`` = (r - null_mean) / null_sd, ``p`` = (1 + #{|r_p| >= |r|}) / (P' + 1), ``q`` = Benjamini-Hochberg
    over the genes with a finite p; ``frame.attrs['p']`` is the association's global p-value.  A gene that is constant
    over the kept cells gives NaN, as in ``gene_corr``.
    ``return_null=True``: ``(frame, null_r)`` with null_r genes x P' float64.  ``var_key_added='gt_'`` also writes
    ``data.var['gt_r']``, ``['gt_p']``, ``['gt_q']``.  ``association``'s other keywords (ks, nsteps, Nnull, seed,
    force_permute_all, ...) pass through.

    The one pass over the cells (W = E^T X) depends on the covariates and batches, not on y: the engine keeps it, and a
    further phenotype on the same covariates costs sample-space algebra only."""
    engine = engine or get_engine()
    if shard_of(data) is not None or int(getattr(engine, 'nranks', 1)) > 1:
        raise NotImplementedError('gene_test does not take sharded data or a multi-rank engine yet (the per-gene sums '
                                  'add over row blocks: one all-reduce away).')
    X = _expression(data, layer)
    for name in ('return_full', 'engine'):
        if name in kwargs:
            raise TypeError("gene_test() got an unexpected keyword argument '%s'" % name)
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
    Zall = np.column_stack([np.asarray(y_std, dtype=np.float64), Z])

    engine.ensure_expression(X)
    Gamma = engine.gram_held()
    kept = np.asarray(res.kept, dtype=bool)
    # What this X was made from, for the engine's memo of W: every association rebuilds X, so the engine's own key moves
    # with every call; an equal signature of the NAM, the kept cells, the samples, the projector (covariates, batches,
    # ridge) and the Gram matrix' bits says the rebuilt X is the same one.  No signature of the NAM: no carry-over.
    content = None
    if getattr(engine, '_nam_sig', None) is not None:
        content = (repr(engine._nam_sig), len(kept), None if kept.all() else _digest(kept), tuple(map(str, index)),
                   _digest(Mv), _digest(Gamma))
    W, rho, sx, sxx, m = engine.expr_cross(content=content)
    r_all = null_correlations(W, rho, sx, sxx, m, Gamma, Zall)
    # constant genes, decided as gene_corr decides them (exactly: minimum == maximum over the kept cells) -- by gene_corr
    # itself, against a column that is finite on the kept cells and varies there.  They depend on E and the kept cells
    # only, so the mask is kept beside W and a further phenotype does not pass over the matrix for it either
    extra = engine.cross_extra()
    constant = extra.get('constant')
    if constant is None:
        probe = np.where(kept, np.arange(len(kept), dtype=np.float64), np.nan)
        constant = np.isnan(engine.gene_corr(probe[None, :])[0])
        extra['constant'] = constant
    r_all[constant] = np.nan
    r, null_r = np.ascontiguousarray(r_all[:, 0]), np.ascontiguousarray(r_all[:, 1:])
    mean, sd, z, p, q = permutation_stats(r, null_r)

    G = X.shape[1]
    if 1.0 / (P + 1) > 0.05 / G:
        warnings.warn(('the smallest p-value {} permutations can give, {:.3g}, is above 0.05 / {} genes. ' +
                       'Consider increasing Nnull').format(P, 1.0 / (P + 1), G))
    gindex = getattr(data, 'var_names', None)
    if gindex is None or len(gindex) != G:
        gindex = pd.RangeIndex(G)
    out = pd.DataFrame({'r': r, 'null_mean': mean, 'null_sd': sd, 'z': z, 'p': p, 'q': q}, index=gindex,
                       columns=['r', 'null_mean', 'null_sd', 'z', 'p', 'q'])
    out.attrs['p'] = res.p                                     # the association's global p-value, as a plain call returns it
    out.attrs['n_null'] = P
    if var_key_added is not None:
        if getattr(data, 'var', None) is None:
            data.var = pd.DataFrame(index=gindex)
        for k in ('r', 'p', 'q'):
            data.var['%s%s' % (var_key_added, k)] = out[k].values
    return (out, null_r) if return_null else out
