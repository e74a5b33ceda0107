"""``cna.ut.expr_to_sample``: the sample-level expression matrix ("pseudobulk"), on the device.

``obs_to_sample`` (reference utils/multisample.py:4-11) turns per-cell columns of ``data.obs`` into one row per sample;
this is the same aggregation for ``data.X``, so that mean expression per sample (or per sample and cluster) sits beside
``y``, ``covs``, ``res.yresid`` and ``res.namresid_sampleXpc`` row for row.  The expression matrix is the one
``cna.tl.gene_corr`` keeps resident (``Engine.ensure_expression``); a call is one pass over it (csrc/expr_bins.hip,
``cna_expr_to_bins``).  This module is the host side only: the codes, the argument checks and the frame.
"""
import numpy as np
import pandas as pd

from ..engine import get_engine
from ..tools._genes import expression_of, gene_index
from ..tools._nam import first_appearance, refuse_sharded

MAX_ROWS = 4096
AGGREGATES = ('mean', 'sum', 'frac')


def expr_to_sample(data, sid_name, layer=None, aggregate='mean', groupby=None, return_counts=False, engine=None):
    """One row per sample id (in order of first appearance, the index ``obs_to_sample`` returns), one column per gene:
    the ``aggregate`` of ``data.X`` (or ``data.layers[layer]``) over that sample's cells, float64.

    ``aggregate``: ``'mean'`` (default), ``'sum'``, or ``'frac'``, the fraction of the cells with ``x > 0`` (an explicit zero
    of a sparse matrix does not count).  ``groupby`` names a second column of ``data.obs`` (a clustering, say): one row per
    (sample, level) pair as a two-level MultiIndex, sample-major, both in order of first appearance, every pair present.
    Cells whose sample id or level is NaN / None are left out, as pandas' groupby drops them.  A row without cells is NaN for
    ``'mean'`` and ``'frac'`` and 0 for ``'sum'``; NaN / inf inside the matrix reach their own (row, gene) only.  At most
    4096 rows.

    The matrix is a C-contiguous float32 / float64 array or a scipy CSR / CSC matrix and stays on the device between calls,
    shared with ``cna.tl.gene_corr``.  ``return_counts=True`` returns ``(frame, counts)``, ``counts`` an int64 Series of
    the cells per row on the same index."""
    if aggregate not in AGGREGATES:
        raise ValueError("aggregate must be one of 'mean', 'sum', 'frac', got %r" % (aggregate,))
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'expr_to_sample', 'the per-row sums add over row blocks: one all-reduce away')
    obs = data.obs
    for k in (sid_name, groupby):
        if k is not None and k not in obs:
            raise KeyError(k)
    scode, samples = first_appearance(obs[sid_name])
    if groupby is None:
        codes, n_levels = scode, 1
        index = samples
    else:
        lcode, levels = first_appearance(obs[groupby])
        n_levels = len(levels)
        codes = np.where((scode < 0) | (lcode < 0), -1, scode * n_levels + lcode)
        index = pd.MultiIndex.from_product([samples, levels], names=[sid_name, groupby])
    n_rows = len(samples) * n_levels
    if not 1 <= n_rows <= MAX_ROWS:
        raise ValueError('expr_to_sample: %d samples x %d levels = %d rows, must lie in [1, %d]'
                         % (len(samples), n_levels, n_rows, MAX_ROWS))
    X = expression_of(data, layer, 'expr_to_sample')
    engine.ensure_expression(X)
    sums, counts = engine.expr_to_bins(codes.astype(np.int32), n_rows, 1 if aggregate == 'frac' else 0)
    if aggregate != 'sum':
        with np.errstate(invalid='ignore', divide='ignore'):
            sums = sums / np.asarray(counts, dtype=np.float64)[:, None]
    frame = pd.DataFrame(sums, index=index, columns=gene_index(data, X.shape[1]))
    if return_counts:
        return frame, pd.Series(np.asarray(counts, dtype=np.int64), index=index)
    return frame
