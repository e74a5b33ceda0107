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
samples by samples x permutations.  The cells x permutations matrix is never formed.  This module is the host side; the steps
``cna.tl.gene_test_strata`` takes as well are in tools/_gene_null.py.
"""
import numpy as np
import pandas as pd

from ..engine import get_engine
from ._gene_null import constant_genes, content_signature, null_phenotypes, warn_smallest_p
from ._genes import expression_of, gene_index
from ._nam import refuse_sharded


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
    refuse_sharded(data, engine, 'gene_test', 'the per-gene sums add over row blocks: one all-reduce away')
    X = expression_of(data, layer, 'gene_test')
    res, Zall, P = null_phenotypes(data, y, sid_name, batches, covs, donorids, key_added, engine, kwargs, 'gene_test')

    engine.ensure_expression(X)
    Gamma = engine.gram_held()
    W, rho, sx, sxx, m = engine.expr_cross(content=content_signature(engine, res, Gamma))
    r_all = null_correlations(W, rho, sx, sxx, m, Gamma, Zall)
    constant = constant_genes(np.asarray(res.kept, dtype=bool), engine.cross_extra(), lambda V: engine.gene_corr(V)[0])
    r_all[constant] = np.nan
    r, null_r = np.ascontiguousarray(r_all[:, 0]), np.ascontiguousarray(r_all[:, 1:])
    mean, sd, z, p, q = permutation_stats(r, null_r)

    warn_smallest_p(P, X.shape[1])
    gindex = gene_index(data, X.shape[1])
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
