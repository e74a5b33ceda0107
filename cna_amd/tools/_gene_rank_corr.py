"""``cna.tl.gene_rank_corr``: Spearman's rank correlation of every gene with per-cell columns, exactly, on the device.

``cna.tl.gene_corr`` is the demo's ``np.corrcoef``: a Pearson r.  Expression is zero-inflated counts, the neighbourhood
coefficient is heavy-tailed, a handful of cells can carry an r, and the answer moves with ``log1p``, scaling and every other
monotone normalisation that may or may not have been applied to ``X``.  The rank correlation is invariant to all of that.
The host route is ``scipy.stats.rankdata`` per gene; here the segmented radix sort of ``gene_markers``
(csrc/expr_ranksum.hip) ranks every gene of the resident matrix over the kept cells with the cell as the entry's payload,
the columns are ranked by the same passes, and one kernel per gene forms the sum of products of the centred, doubled ranks
in integers (``cna_gene_rank_corr``).  This module is the host side only: the argument checks, the one float64 line from
those integers and the frame.
"""
import numpy as np
import pandas as pd

from ..engine import get_engine
from ._genes import expression_of, gene_index, key_columns
from ._nam import refuse_sharded
from ._strata import levels_of

MAX_LEVELS = 255        # cna_gene_rank_corr_by: the level is one digit of the sort, 255 stands for a left-out entry


def wide_to_float(s_lo, s_hi):
    """float64 of the 128-bit two's complement integers {low 64 bits, the limb above}: exact where the value fits 64 bits
    and is below 2^53 in absolute value, else rounded once per limb (relative error below 2^-51: there |S| >= 2^63)."""
    lo = np.ascontiguousarray(s_lo, dtype=np.uint64)
    hi = np.asarray(s_hi, dtype=np.int64)
    signed = lo.view(np.int64)
    fits = hi == (signed >> 63)                           # the high limb is the sign of the low one
    return np.where(fits, signed.astype(np.float64), hi.astype(np.float64) * 2.0 ** 64 + lo.astype(np.float64))


def rank_corr_statistics(s_lo, s_hi, tie_gene, tie_key, m, nan):
    """-> float64[keys, genes]: Spearman's rho from the integers of ``Engine.gene_rank_corr``.  With r the midrank over the m
    kept cells, a = 2 r_gene - (m + 1) and b = 2 r_key - (m + 1): S = sum a b (s_lo, s_hi: 128-bit two's complement),
    sum a^2 = (m^3 - m - T_gene) / 3 with T = sum over the tie groups of t^3 - t, the same for the key, so

        rho = 3 S / sqrt((m^3 - m - T_gene) (m^3 - m - T_key))

    NaN for a gene that is constant over the kept cells (T_gene = m^3 - m), a constant key, m < 2 and a gene flagged `nan`.
    The one statement of this arithmetic."""
    S = wide_to_float(s_lo, s_hi)
    tie_gene = np.asarray(tie_gene, dtype=np.float64)
    tie_key = np.asarray(tie_key, dtype=np.float64)
    m = float(m)
    full = m * (m * m - 1.0)
    dead = np.asarray(nan, dtype=bool)[None, :] | (tie_gene >= full)[None, :] | (tie_key >= full)[:, None] | (m < 2)
    with np.errstate(all='ignore'):
        rho = 3.0 * S / np.sqrt((full - tie_gene)[None, :] * (full - tie_key)[:, None])
    rho = np.clip(rho, -1.0, 1.0)                         # (3 S and the root round separately: 1 + 2^-52 is not a correlation)
    rho[dead] = np.nan
    return rho


def gene_rank_corr(data, keys='coef', layer=None, key_added=None, engine=None):
    """Spearman's rank correlation of every gene with one or several numeric columns of ``data.obs`` (1 to 16: the
    neighbourhood coefficient that ``association(..., key_added='coef')`` stored, several phenotypes' coefficients, NAM PC
    loadings), exact: unlike ``gene_corr``'s Pearson r it does not change with ``log1p``, scaling or any other monotone
    normalisation of the matrix or of a column, and no handful of cells carries it.

    Kept cells: those where EVERY key of the call is finite -- one set per call, unlike ``gene_corr``'s set per key,
    because a gene's ranks depend on the set; a non-finite value in a key means "cell left out".  ``m`` is their number,
    ``frame.attrs['n_cells']``.

    Ranks: genes and keys are both ranked over the kept cells with midranks.  A gene is ranked on the stored type's bits
    (``-0.0`` = ``+0.0`` = a stored zero = the implicit zeros of a sparse matrix, ``+-inf`` ordinary values, a float64
    matrix on all 64 bits); a key as float64 on all 64 bits with ``-0.0`` = ``+0.0``.

    NaN results: a gene that is constant over the kept cells, a constant key, ``m < 2``, and a gene with a NaN in a kept
    cell.  Where nothing is NaN the result is ``scipy.stats.spearmanr(x_g[kept], v_k[kept]).statistic``.

    The matrix is ``data.X`` or ``data.layers[layer]``, cells x genes: a C-contiguous float32 / float64 array or a scipy
    CSR / CSC matrix, resident on the device and shared with ``gene_corr`` and the other gene tools.  The device returns
    integers (the sum of products of the centred, doubled ranks on 128 bits, the tie terms); rho is one float64 line on
    the host (``rank_corr_statistics``).

    Returns a float64 DataFrame (index ``data.var_names`` when there are any), one column per key; ``key_added`` (a
    prefix) also writes ``data.var[key_added + key]``.

    Not here: p-values (cells are not independent, so the t approximation would be anti-conservative: the answer to that
    is a permutation null, ``gene_rank_test`` for this rho as ``gene_test`` is for r), Kendall's tau, gene-gene
    rank correlations, a kept set per key, more than 16 keys per call, sharded data."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_rank_corr', 'the ranking runs over all cells of a gene: the rows of other ranks are elsewhere')
    names, V = key_columns(data.obs, keys)
    X = expression_of(data, layer, 'gene_rank_corr')
    engine.ensure_expression(X)
    s_lo, s_hi, tie_gene, tie_key, m, nan = engine.gene_rank_corr(V)
    rho = rank_corr_statistics(s_lo, s_hi, tie_gene, tie_key, m, nan)
    index = gene_index(data, X.shape[1])
    out = pd.DataFrame({k: rho[j] for j, k in enumerate(names)}, index=index, columns=names)
    out.attrs['n_cells'] = int(m)
    if key_added is not None:
        if getattr(data, 'var', None) is None:
            data.var = pd.DataFrame(index=index)
        for k in names:
            data.var['%s%s' % (key_added, k)] = out[k].values
    return out


def gene_rank_corr_strata(data, stratification, keys='coef', layer=None, engine=None):
    """Spearman's rank correlation of every gene with one or several numeric columns of ``data.obs`` (1 to 16, as in
    ``gene_rank_corr``) inside each distinct value of ``data.obs[stratification]`` (levels in order of first appearance, as
    ``gene_corr_strata`` orders them): which genes separate the expanded from the depleted cells inside a cluster, or
    inside a ``coef_populations`` population.  A cluster has few cells, its counts are zero-inflated and its coefficient is
    smooth, so a handful of cells easily carries ``gene_corr_strata``'s Pearson r, and that r moves with whatever
    normalisation ``X`` went through; the rank version does neither.

    Kept cells: ``C_l``, the cells of level ``l`` where EVERY key of the call is finite -- ``gene_rank_corr``'s one kept set
    per call, intersected with the level; cells whose level is NaN / None are in no level.  ``m_l`` is their number,
    ``frame.attrs['n_cells']`` (a Series indexed by level).

    Ranks: genes and keys are both ranked with midranks over ``C_l``, under ``gene_rank_corr``'s rules (``-0.0`` = ``+0.0``
    = a stored zero = an implicit zero, float64 on all 64 bits, ``+-inf`` ordinary values of a gene).

    NaN results: a gene that is constant on ``C_l`` (a sparse gene with no stored entry in the level among them), a key
    that is constant on ``C_l``, ``m_l < 2``; and a gene with a NaN in a kept cell of ANY level, in every level -- a guard
    on the whole gene, as in ``gene_rank_corr``, not what scipy would say level by level.  Where nothing is NaN the result
    is ``scipy.stats.spearmanr(x_g[C_l], v_k[C_l]).statistic``.

    The matrix is ``data.X`` or ``data.layers[layer]``, resident on the device and shared with the other gene tools.  All
    levels come from one sort of the matrix (``cna_gene_rank_corr_by``: one more radix pass on the level behind the value
    passes), as integers; rho is ``rank_corr_statistics`` on each level's integers.

    Returns a float64 DataFrame indexed by ``data.var_names`` (a ``RangeIndex`` when there are none); its columns are the
    levels (an Index named after the stratification) for a ``str`` key, a MultiIndex ``(key, level)``, key-major, for a
    list of keys.

    p-values: ``gene_rank_test_strata``, a permutation null per level.  Not here: a pooled "within" coefficient across the levels (ranks inside different
    levels do not pool the way ``gene_corr_strata``'s centred sums do), more than 255 levels or 16 keys per call, sharded
    data."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'gene_rank_corr_strata',
                   'the ranking runs over all cells of a level: the rows of other ranks are elsewhere')
    obs = data.obs
    if stratification not in obs:
        raise KeyError(stratification)
    names, V = key_columns(obs, keys)
    codes, levels = levels_of(obs, stratification, 'gene_rank_corr_strata', max_levels=MAX_LEVELS)
    X = expression_of(data, layer, 'gene_rank_corr_strata')
    engine.ensure_expression(X)
    s_lo, s_hi, tie_gene, tie_key, m, nan = engine.gene_rank_corr_by(V, codes, len(levels))
    rho = np.stack([rank_corr_statistics(s_lo[l], s_hi[l], tie_gene[l], tie_key[l], int(m[l]), nan)
                    for l in range(len(levels))], axis=1)                     # [key, level, gene]
    index = gene_index(data, X.shape[1])
    level_index = pd.Index(levels, name=stratification)
    if isinstance(keys, str):
        frame = pd.DataFrame(rho[0].T, index=index, columns=level_index)
    else:
        columns = pd.MultiIndex.from_product([names, level_index], names=['key', stratification])
        frame = pd.DataFrame(rho.reshape(len(names) * len(levels), -1).T, index=index, columns=columns)
    frame.attrs['n_cells'] = pd.Series(np.asarray(m, dtype=np.int64), index=level_index)
    return frame
