"""``cna.tl.gene_nbhd_corr`` and ``cna.tl.nbhd_expr``: the expression of a neighbourhood.

The association's result is a number per *neighbourhood*: neighbourhood ``i`` is the soft set of cells that the
``nsteps``-step random walk anchored at cell ``i`` reaches, and the NAM is the abundance of every sample in those sets.
``gene_corr`` and its relatives correlate that number with the expression of the anchor cell alone, which is zero-inflated
and noisy.  The quantity in the coefficient's own unit is the mean of the gene over the neighbourhood's cells, with the
weights the NAM uses.  With one walk step ``P s = A.(s/c) + w*s/c``, ``c = A.sum(0) + w`` (reference _nam.py:28-33), and
``e_g`` the gene's column in float64::

    m_g = (P^nsteps e_g) / (P^nsteps 1)          element-wise

The numerator is what the NAM would hold if the gene were a sample; the denominator is the membership mass of the
neighbourhood.  A cell whose denominator is not a positive finite number is left out of every sum; its ``m`` is NaN.
The walk runs on the device over tiles of gene columns (csrc/expr_nbhd.hip), bit for bit as ``cna.tl.diffuse`` would walk
the same columns, and leaves the walk's state and the cached NAM of the engine alone.  This module is the host side only:
argument checks and the frames.

Not built: permutation p-values, rank statistics of ``m``, strata, ``nsteps=None``, sharded data.
"""
import numbers

import numpy as np
import pandas as pd

from ..engine import get_engine
from ._genes import expression_of, gene_index, key_columns
from ._nam import _prepare_graph, refuse_sharded

MAX_STEPS = 15
MAX_GENES = 64
_REQUIRED = object()
_REMEDY = 'the walk over gene columns needs the halo exchange of the sharded walk'


def _check_nsteps(nsteps, who):
    if nsteps is _REQUIRED:
        raise TypeError('%s needs nsteps: pass what the association used' % who)
    if isinstance(nsteps, bool) or not isinstance(nsteps, numbers.Integral):
        raise TypeError('%s: nsteps must be an int, got %r' % (who, nsteps))
    if not 1 <= int(nsteps) <= MAX_STEPS:
        raise ValueError('%s: nsteps must lie in [1, %d], got %d' % (who, MAX_STEPS, int(nsteps)))
    return int(nsteps)


def _gene_positions(genes, index):
    """Positions of 1 to 64 genes given by name (entries of `index`) or integer position; (labels, int32 positions)."""
    if isinstance(genes, (str, numbers.Integral)):
        genes = [genes]
    genes = list(genes)
    if not genes:
        raise ValueError('nbhd_expr needs at least one gene')
    if len(genes) > MAX_GENES:
        raise ValueError('nbhd_expr takes at most %d genes per call, got %d' % (MAX_GENES, len(genes)))
    pos, labels = [], []
    for g in genes:
        if isinstance(g, numbers.Integral) and not isinstance(g, bool):
            if not 0 <= int(g) < len(index):
                raise IndexError('gene position %d outside [0, %d)' % (int(g), len(index)))
            pos.append(int(g))
        else:
            where = index.get_indexer([g])[0]
            if where < 0:
                raise KeyError(g)
            pos.append(int(where))
        labels.append(index[pos[-1]])
    return labels, np.asarray(pos, dtype=np.int32)


def _make_resident(engine, data, X, self_weight):
    _prepare_graph(engine, data, self_weight)
    engine.ensure_expression(X)


def gene_nbhd_corr(data, keys='coef', nsteps=_REQUIRED, self_weight=1, layer=None, key_added=None, engine=None):
    """Pearson correlation of the neighbourhood-mean expression ``m_g`` of every gene (module docstring) with one or
    several columns of ``data.obs`` (1 to 16 float columns, usually the coefficient that
    ``association(..., key_added='coef')`` stored), over the cells where the column is finite and the neighbourhood has
    mass -- each column its own set.

    ``nsteps`` (required, an int in [1, 15]): pass what the association used, so that the neighbourhoods are the ones its
    coefficient belongs to; ``self_weight`` likewise.  The matrix is ``data.X`` or ``data.layers[layer]`` as for
    ``gene_corr``; the graph is ``data.obsp['connectivities']``.  Both stay on the device between calls, and the NAM the
    engine caches for the association survives.

    NaN where numpy's 0/0 gives NaN (a constant column, fewer than two cells) and for a gene that is constant over all
    cells of the raw matrix (decided exactly, implicit zeros counted).

    Returns a DataFrame, genes x keys.  ``attrs['n_cells']``: cells per key (dict); ``attrs['nsteps']``;
    ``attrs['mean']`` and ``attrs['sd']``: genes x keys frames of the mean and the population sd of ``m_g`` over the
    key's cells.  ``key_added`` (a prefix) also writes ``data.var[key_added + key]``."""
    nsteps = _check_nsteps(nsteps, 'gene_nbhd_corr')
    names, V = key_columns(data.obs, keys)
    X = expression_of(data, layer, 'gene_nbhd_corr')
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_nbhd_corr', _REMEDY)
    _make_resident(engine, data, X, self_weight)
    r, mean, sd, n_cells = engine.gene_nbhd_corr(V, nsteps)
    index = gene_index(data, X.shape[1])

    def frame(a):
        return pd.DataFrame({k: a[j] for j, k in enumerate(names)}, index=index, columns=names)

    out = frame(r)
    out.attrs['n_cells'] = {k: int(n_cells[j]) for j, k in enumerate(names)}
    out.attrs['nsteps'] = nsteps
    out.attrs['mean'] = frame(mean)
    out.attrs['sd'] = frame(sd)
    if key_added is not None:
        if getattr(data, 'var', None) is None:
            data.var = pd.DataFrame(index=index)
        for k in names:
            data.var['%s%s' % (key_added, k)] = out[k].values
    return out


def nbhd_expr(data, genes, nsteps=_REQUIRED, self_weight=1, layer=None, key_added=None, return_parts=False, engine=None):
    """The neighbourhood-mean expression ``m_g`` (module docstring) of 1 to 64 genes -- names in ``data.var_names`` or
    integer positions -- as a cells x genes float64 DataFrame in the caller's cell order: the smoothed marker to put on
    the embedding.  NaN for a cell whose neighbourhood has no mass.

    ``nsteps`` (required, an int in [1, 15]): pass what the association used.  ``key_added`` (a prefix) also writes the
    columns into ``data.obs``, where ``coef_raster`` and the ``*_strata`` tools take them.  ``return_parts=True`` returns
    ``(numerator, denominator)`` -- a cells x genes frame and a Series -- instead of their quotient: bit for bit what
    ``cna.tl.diffuse`` returns for the genes' columns and for a column of ones."""
    nsteps = _check_nsteps(nsteps, 'nbhd_expr')
    X = expression_of(data, layer, 'nbhd_expr')
    labels, pos = _gene_positions(genes, gene_index(data, X.shape[1]))
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'nbhd_expr', _REMEDY)
    _make_resident(engine, data, X, self_weight)
    num, den = engine.nbhd_expr(pos, nsteps)
    num = pd.DataFrame(num, index=data.obs.index, columns=labels)
    den = pd.Series(den, index=data.obs.index, name='mass')
    if return_parts:
        return num, den
    good = np.isfinite(den.values) & (den.values > 0)
    with np.errstate(all='ignore'):
        m = np.where(good[:, None], num.values / den.values[:, None], np.nan)
    out = pd.DataFrame(m, index=data.obs.index, columns=labels)
    if key_added is not None:
        for g in labels:
            data.obs['%s%s' % (key_added, g)] = out[g].values
    return out
