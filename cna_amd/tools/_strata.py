"""``cna.tl.coef_strata``: the neighbourhood coefficient by cluster, on the device.

The reference's workflow looks at the result of ``cna.tl.association`` per cluster (demo/demo.ipynb)::

    sc.tl.leiden(d)
    cna.pl.violinplot(d, 'leiden', key='coef')

``cna.pl.violinplot`` (plotting/_strat.py:21-29) hands ``data.obs[key]`` of every level to ``Axes.violinplot``, whose
kernel density (``matplotlib.cbook.violin_stats`` with ``mlab.GaussianKDE``) is a Python loop over cell-sized numpy
temporaries, turns all-NaN as soon as the QC dropped one cell of a cluster, and leaves the numbers in a figure.  Here the
three per-cell columns go to the device and come back as one row per level plus, on request, the dicts ``Axes.violin``
draws (csrc/strata.hip, ``cna_coef_strata``).  Drawing itself stays with matplotlib.  This module is the host side only:
the codes, the argument checks, the frame and the dicts.
"""
import math
from numbers import Number

import numpy as np
import pandas as pd

from ..engine import get_engine
from ._genes import numeric_column
from ._nam import first_appearance, refuse_sharded

MAX_LEVELS = 1024
MAX_POINTS = 1024
FDR_THRESH = 0.1        # plotting/_umap.py:10, umap_ncorr's default


def levels_of(obs, stratification, who, max_levels=MAX_LEVELS):
    """(int32 code per cell, the levels) of ``data.obs[stratification]``: levels in order of first appearance, NaN / None
    -> code -1.  KeyError without the column; ValueError, under `who`'s name, unless there are 1 to max_levels levels."""
    if stratification not in obs:
        raise KeyError(stratification)
    codes, levels = first_appearance(obs[stratification])
    if not 1 <= len(levels) <= max_levels:
        raise ValueError('%s: data.obs[%r] has %d levels, must lie in [1, %d]'
                         % (who, stratification, len(levels), max_levels))
    return np.ascontiguousarray(codes, dtype=np.int32), levels


def _bandwidth(bw_method):
    """(kind, value) of mlab.GaussianKDE's bw_method."""
    if bw_method is None or (isinstance(bw_method, str) and bw_method == 'scott'):
        return 'scott', 0.0
    if isinstance(bw_method, str) and bw_method == 'silverman':
        return 'silverman', 0.0
    if isinstance(bw_method, Number) and not isinstance(bw_method, bool):
        f = float(bw_method)
        if not (f > 0.0 and math.isfinite(f)):
            raise ValueError('bw_method as a number must be positive and finite, got %r' % (bw_method,))
        return 'constant', f
    if callable(bw_method):
        raise TypeError('bw_method as a callable is not taken: there is no GaussianKDE object per level to hand it; '
                        "use 'scott', 'silverman' or a positive float")
    raise ValueError("bw_method should be None, 'scott', 'silverman' or a positive float, got %r" % (bw_method,))


def coef_strata(data, stratification, key='coef', fdr_thresh=None, points=100, bw_method=None, return_violin=False,
                engine=None):
    """One row per distinct value of ``data.obs[stratification]`` (in order of first appearance, as
    ``cna.pl.violinplot`` orders its violins): the distribution of ``data.obs[key]`` over that level's cells.

    Cells whose level is NaN / None are left out; cells whose ``data.obs[key]`` is not finite (NaN marks the cells the
    association did not keep) count in ``n`` only.  Columns: ``n``, ``n_kept`` (int64), ``mean``, ``sd`` (ddof = 1),
    ``min``, ``median``, ``max`` (float64; NaN where undefined: ``sd`` below two kept cells, the rest without any).  When
    ``data.obs`` has ``key + '_fdr'`` (``association(..., key_added=key)`` writes it) also ``n_pos`` / ``n_neg``, the kept
    cells with ``fdr <= fdr_thresh`` (default 0.1 as ``cna.pl.umap_ncorr``; a NaN fdr fails) and a positive / negative
    coefficient, and ``frac_pos`` / ``frac_neg``, those over ``n_kept``.

    ``return_violin=True`` returns ``(frame, violin)``: one dict per level with ``n_kept >= 1``, in row order, with the keys
    ``Axes.violin`` reads (``coords``, ``vals``, ``mean``, ``median``, ``min``, ``max``, ``quantiles``), the density as
    ``Axes.violinplot`` computes it on ``points`` grid points: ``mlab.GaussianKDE`` with ``bw_method`` ``None`` /
    ``'scott'``, ``'silverman'`` or a positive float, and all ones for a level whose kept values are all equal::

        ax.violin(violin, positions=np.flatnonzero(frame.n_kept.values > 0), widths=0.9,
                  showmeans=False, showextrema=False, showmedians=False)

    At most 1024 levels and 1024 points."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'coef_strata', 'the per-level sums add over row blocks, the median and the density need '
                                                'every block: a gather away')
    obs = data.obs
    for k in (stratification, key):
        if k not in obs:
            raise KeyError(k)
    fkey = '%s_fdr' % (key,)
    has_fdr = fkey in obs
    if not has_fdr and fdr_thresh is not None:
        raise KeyError(fkey)
    v = numeric_column(obs, key)
    fdr = numeric_column(obs, fkey) if has_fdr else None
    thresh = FDR_THRESH if fdr_thresh is None else float(fdr_thresh)
    if isinstance(points, bool) or int(points) != points or not 1 <= int(points) <= MAX_POINTS:
        raise ValueError('points must be an integer in [1, %d], got %r' % (MAX_POINTS, points))
    points = int(points)
    bw_kind, bw_value = _bandwidth(bw_method)
    codes, levels = levels_of(obs, stratification, 'coef_strata')
    r = engine.coef_strata(v, fdr, codes, len(levels), thresh, points, bw_kind, bw_value)
    kept = np.asarray(r['n_kept'], dtype=np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        sd = np.where(kept >= 2, np.sqrt(np.asarray(r['ssd']) / (kept - 1.0)), np.nan)
        cols = {'n': np.asarray(r['n'], dtype=np.int64), 'n_kept': kept}
        for k in ('mean', 'sd', 'min', 'median', 'max'):
            cols[k] = sd if k == 'sd' else np.where(kept >= 1, np.asarray(r[k], dtype=np.float64), np.nan)
        if has_fdr:
            for k in ('n_pos', 'n_neg'):
                cols[k] = np.asarray(r[k], dtype=np.int64)
            cols['frac_pos'] = cols['n_pos'] / kept.astype(np.float64)
            cols['frac_neg'] = cols['n_neg'] / kept.astype(np.float64)
    frame = pd.DataFrame(cols, index=pd.Index(levels, name=stratification), columns=list(cols))
    if not return_violin:
        return frame
    violin = []
    for b in np.flatnonzero(kept >= 1):
        lo, hi = float(cols['min'][b]), float(cols['max'][b])
        violin.append({'coords': np.linspace(lo, hi, points), 'vals': np.array(r['vals'][b], dtype=np.float64),
                       'mean': float(cols['mean'][b]), 'median': float(cols['median'][b]), 'min': lo, 'max': hi,
                       'quantiles': np.empty(0)})
    return frame, violin
