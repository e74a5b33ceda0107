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
from ._genes import expression_of, gene_index, key_columns
from ._nam import refuse_sharded
from ._strata import levels_of

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
    refuse_sharded(data, engine, 'gene_corr_strata', 'the per-level sums add over row blocks: one all-reduce away')
    obs = data.obs
    if stratification not in obs:
        raise KeyError(stratification)
    names, V = key_columns(obs, keys)
    codes, levels = levels_of(obs, stratification, 'gene_corr_strata')
    if len(names) * len(levels) > MAX_ROWS:
        raise ValueError('gene_corr_strata: %d keys x %d levels exceed %d rows; pass fewer keys per call'
                         % (len(names), len(levels), MAX_ROWS))
    X = expression_of(data, layer, 'gene_corr_strata')
    engine.ensure_expression(X)
    r, within, _ = engine.gene_corr_by(V, codes, len(levels), want_within=bool(return_within))
    index = gene_index(data, X.shape[1])
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
