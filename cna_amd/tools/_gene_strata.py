"""``cna.tl.gene_corr_strata``: per-gene correlation to per-cell columns inside every level of a clustering, on the device.

``cna.tl.coef_strata`` (the numbers behind the reference's ``cna.pl.violinplot(d, 'leiden', key='coef')``,
plotting/_strat.py:21-29) shows a cluster whose violin spans both signs; the next question is which genes separate its
expanded cells from its depleted ones.  The global line of the reference's workflow (demo/demo.ipynb, "per-gene correlations
to neighborhood coefficient") cannot say: across all cells it is dominated by the cluster markers.  Here one pass over the
resident expression matrix, with the cell's level as the accumulator index, gives the correlation inside every level and
one cluster-adjusted number per gene (csrc/expr_corr_by.hip, ``cna_gene_corr_by``).  This module is the host side only: the
codes, the argument checks and the frames.
"""
import numpy as np
import pandas as pd

from ..engine import get_engine
from ._genes import check_expression, key_columns
from ._nam import shard_of

MAX_LEVELS = 1024
MAX_ROWS = 4096         # keys x levels, the row cap of cna.ut.expr_to_sample


def gene_corr_strata(data, stratification, keys='coef', layer=None, return_within=False, engine=None):
    """Pearson correlation of every gene with one or several columns of ``data.obs`` (1 to 16 float columns, as in
    ``gene_corr``) inside each distinct value of ``data.obs[stratification]`` (levels in order of first appearance, as
    ``coef_strata`` orders its rows): per key and level over the level's cells where the column is finite,
    ``np.corrcoef(v[C], X[C], rowvar=False)[0, 1:]``, implicit zeros of a sparse matrix included.  Cells whose level is
    NaN / None are left out.  NaN where a level has fewer than two such cells, or where the column or the gene is constant
    on them.

    The matrix is ``data.X`` or ``data.layers[layer]``, resident on the device and shared with ``gene_corr``,
    ``gene_test`` and ``cna.ut.expr_to_sample``.

    Returns a float64 DataFrame indexed by ``data.var_names`` (a ``RangeIndex`` when there are none); its columns are the
    levels (an Index named after the stratification) for a ``str`` key, a MultiIndex ``(key, level)``, key-major, for a
    list of keys.  ``return_within=True`` returns ``(frame, within)``: ``within`` (genes x keys) is the cluster-adjusted
    correlation, that of ``x - level mean`` with ``v - level mean`` over the cells that have a level and a finite value
    -- NaN when the gene, or the column, is constant inside every level.

    At most 1024 levels, and keys x levels <= 4096."""
    engine = engine or get_engine()
    if shard_of(data) is not None or int(getattr(engine, 'nranks', 1)) > 1:
        raise NotImplementedError('gene_corr_strata does not take sharded data or a multi-rank engine yet (the per-level '
                                  'sums add over row blocks: one all-reduce away).')
    obs = data.obs
    if stratification not in obs:
        raise KeyError(stratification)
    names, V = key_columns(obs, keys)
    codes, levels = pd.factorize(obs[stratification])           # first appearance; NaN / None -> -1
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError('gene_corr_strata: data.obs[%r] has %d levels, must lie in [1, %d]'
                         % (stratification, len(levels), MAX_LEVELS))
    if len(names) * len(levels) > MAX_ROWS:
        raise ValueError('gene_corr_strata: %d keys x %d levels exceed %d rows; pass fewer keys per call'
                         % (len(names), len(levels), MAX_ROWS))
    if layer is None:
        X = getattr(data, 'X', None)
        if X is None:
            raise ValueError('data.X is missing: gene_corr_strata needs the expression matrix')
    else:
        layers = getattr(data, 'layers', None)
        if layers is None or layer not in layers:
            raise KeyError(layer)
        X = layers[layer]
    X = check_expression(X, len(obs))
    engine.ensure_expression(X)
    r, within, _ = engine.gene_corr_by(V, np.asarray(codes, dtype=np.int32), len(levels), want_within=bool(return_within))
    index = getattr(data, 'var_names', None)
    if index is None or len(index) != X.shape[1]:
        index = pd.RangeIndex(X.shape[1])
    level_index = pd.Index(levels, name=stratification)
    r = np.asarray(r, dtype=np.float64)
    if isinstance(keys, str):
        frame = pd.DataFrame(r[0].T, index=index, columns=level_index)
    else:
        columns = pd.MultiIndex.from_product([names, level_index], names=['key', stratification])
        frame = pd.DataFrame(r.reshape(len(names) * len(levels), -1).T, index=index, columns=columns)
    if not return_within:
        return frame
    return frame, pd.DataFrame(np.asarray(within, dtype=np.float64).T, index=index, columns=names)
