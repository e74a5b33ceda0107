"""``cna.tl.gene_corr``: per-gene correlation to per-cell columns, on the device.

The reference's workflow reads the result of ``cna.tl.association`` like this (demo/demo.ipynb, "per-gene
correlations to neighborhood coefficient")::

    d.var['corr_case'] = np.corrcoef(d.obs.male_coef.values.reshape(1,-1), d.X, rowvar=False)[0,1:]

which builds a (genes + 1) x (genes + 1) matrix to read one row of it, does not take a sparse ``X`` and turns all-NaN as
soon as the QC dropped one cell.  Here the expression matrix goes to the device once (``Engine.ensure_expression``) and
every call is one pass over it (csrc/genes.hip, csrc/expr_corr.hip).  This module is the host side only: argument checks and the frame.
"""
import numpy as np
import pandas as pd
import scipy.sparse as sp

from ..engine import get_engine
from ._nam import refuse_sharded

MAX_KEYS = 16


def check_expression(X, n_obs):
    """The expression matrix as the engine takes it, or TypeError / ValueError -- before anything is uploaded."""
    if isinstance(X, np.ndarray):
        if X.ndim != 2:
            raise ValueError('the expression matrix must be 2-D (cells x genes), got %d-D' % X.ndim)
        if X.dtype not in (np.float32, np.float64):
            raise TypeError('the expression matrix must be float32 or float64, got %s' % X.dtype)
        if not X.flags['C_CONTIGUOUS']:
            raise TypeError('a dense expression matrix must be C-contiguous (cells x genes, one row per cell)')
    elif sp.issparse(X):
        if X.format not in ('csr', 'csc'):
            raise TypeError('a sparse expression matrix must be CSR or CSC, got %s' % X.format)
        if X.data.dtype not in (np.float32, np.float64):
            raise TypeError('the expression values must be float32 or float64, got %s' % X.data.dtype)
        if X.indices.dtype not in (np.int32, np.int64) or X.indptr.dtype not in (np.int32, np.int64):
            raise TypeError('the expression matrix needs int32 or int64 indices')
    else:
        raise TypeError('the expression matrix must be a numpy.ndarray or a scipy CSR / CSC matrix, got %s'
                        % type(X).__name__)
    if X.shape[0] != n_obs:
        raise ValueError('the expression matrix has %d rows, data.obs has %d cells' % (X.shape[0], n_obs))
    if X.shape[0] < 1 or X.shape[1] < 1 or X.shape[0] >= 2 ** 31 or X.shape[1] >= 2 ** 31:
        raise ValueError('cells and genes must lie in [1, 2^31), got %d x %d' % X.shape)
    return X


def expression_of(data, layer, who):
    """``data.X``, or ``data.layers[layer]``, checked (check_expression); ValueError / KeyError when it is not there."""
    if layer is None:
        X = getattr(data, 'X', None)
        if X is None:
            raise ValueError('data.X is missing: %s needs the expression matrix' % who)
    else:
        layers = getattr(data, 'layers', None)
        if layers is None or layer not in layers:
            raise KeyError(layer)
        X = layers[layer]
    return check_expression(X, len(data.obs))


def gene_index(data, n_genes):
    """``data.var_names`` when there are n_genes of them, else a RangeIndex."""
    index = getattr(data, 'var_names', None)
    return pd.RangeIndex(n_genes) if index is None or len(index) != n_genes else index


def numeric_column(obs, k):
    """data.obs[k] as contiguous float64, or TypeError."""
    try:
        return np.ascontiguousarray(np.asarray(obs[k].values, dtype=np.float64))
    except (TypeError, ValueError):
        raise TypeError('data.obs[%r] is not numeric' % (k,)) from None


def key_columns(obs, keys):
    """(names, q x cells float64) of the requested columns of data.obs."""
    names = [keys] if isinstance(keys, str) else list(keys)
    if not names:
        raise ValueError('gene_corr needs at least one key')
    if len(names) > MAX_KEYS:
        raise ValueError('gene_corr takes at most %d keys per call, got %d' % (MAX_KEYS, len(names)))
    cols = []
    for k in names:
        if k not in obs:
            raise KeyError(k)
        cols.append(numeric_column(obs, k))
    return names, np.ascontiguousarray(np.stack(cols))


def gene_corr(data, keys='coef', layer=None, key_added=None, engine=None):
    """Pearson correlation of every gene with one or several columns of ``data.obs`` (the neighbourhood coefficient
    that ``association(..., key_added='coef')`` stored, several phenotypes' coefficients, NAM PC loadings: 1 to 16
    float columns), over the cells where the column is finite -- each column its own set; NaN marks the cells the
    association did not keep.  Where every cell is finite this is
    ``np.corrcoef(v, X, rowvar=False)[0, 1:]``.

    The matrix is ``data.X`` or ``data.layers[layer]``, cells x genes: a C-contiguous float32 / float64 array or a scipy
    CSR / CSC matrix.  It stays on the device between calls (``engine.pin_expression`` skips the content hash,
    ``engine.drop_expression`` frees it).  A gene that is constant over a column's cells, and a constant column, give
    NaN, as numpy does.

    Returns a DataFrame (index ``data.var_names`` when there are any), one float64 column per key; ``key_added``
    (a prefix) also writes ``data.var[key_added + key]``."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_corr', 'the per-gene sums add over row blocks: one all-reduce away')
    names, V = key_columns(data.obs, keys)
    X = expression_of(data, layer, 'gene_corr')
    engine.ensure_expression(X)
    r = engine.gene_corr(V)
    index = gene_index(data, X.shape[1])
    out = pd.DataFrame({k: r[j] for j, k in enumerate(names)}, index=index, columns=names)
    if key_added is not None:
        if getattr(data, 'var', None) is None:
            data.var = pd.DataFrame(index=index)
        for k in names:
            data.var['%s%s' % (key_added, k)] = out[k].values
    return out
