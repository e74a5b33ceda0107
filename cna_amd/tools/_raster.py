"""``cna.tl.coef_raster``: the neighbourhood coefficient on the embedding, as images, on the device.

The first thing the reference's workflow does with the result of ``cna.tl.association`` is a picture
(demo/demo.ipynb 1.2, 1.3)::

    cna.pl.umap_ncorr(d, key='case_coef')

``cna.pl.umap_ncorr`` (plotting/_umap.py:6-36) draws every cell in grey and on top of them the cells with
``coef_fdr <= 0.1`` coloured by coefficient: two matplotlib scatters of all cells through scanpy, which sorts the points by
value so that the highest lies on top, and the numbers stay in the figure.  Section 3.2.1 draws NAM-PC loadings the same
way (``sc.pl.umap(d, color='NAMPC1', cmap='seismic')``).  Here the cells are reduced to pixels on the device
(csrc/raster.hip, ``cna_coef_raster``) and come back as arrays for ``Axes.imshow``.  Drawing, colour maps and the alpha
blending of overlapping markers stay with matplotlib.  This module is the host side only: the columns, the argument
checks, the mean and the dict.
"""
import math

import numpy as np

from ..engine import get_engine
from ._genes import numeric_column
from ._nam import refuse_sharded
from ._strata import FDR_THRESH

MAX_KEYS = 16
MAX_SIDE = 4096
MAX_PIXELS = 2 ** 22
MAX_RADIUS = 16


def _int_in(name, value, lo, hi):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError('coef_raster: %s must be an integer in [%d, %d], got %r' % (name, lo, hi, value))
    return int(value)


def _coordinates(data, basis, components, n):
    """cells x 2 float64 (float32 widens exactly) from data.obsm[basis][:, components] or an array-like of two columns."""
    if isinstance(basis, str):
        obsm = getattr(data, 'obsm', None)
        if obsm is None or basis not in obsm:
            raise KeyError(basis)
        a = np.asarray(obsm[basis])
        comps = tuple(components)
        if len(comps) != 2 or a.ndim != 2 or not all(isinstance(c, (int, np.integer)) and 0 <= c < a.shape[1] for c in comps):
            raise ValueError('coef_raster: components must name two columns of data.obsm[%r] of shape %s, got %r'
                             % (basis, a.shape, components))
        a = a[:, list(comps)]
    else:
        a = np.asarray(basis)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError('coef_raster: basis as an array must have shape (cells, 2), got %s' % (a.shape,))
    if a.shape[0] != n:
        raise ValueError('coef_raster: %d coordinates for %d cells' % (a.shape[0], n))
    try:
        return np.ascontiguousarray(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError('coef_raster: the coordinates are not numeric') from None


def coef_raster(data, key='coef', basis='X_umap', shape=512, extent=None, fdr_thresh=None, radius=0, components=(0, 1),
                engine=None):
    """The numbers behind ``cna.pl.umap_ncorr(data, key=key)``, per pixel of a ``shape`` grid over ``data.obsm[basis]``::

        img = cna.tl.coef_raster(data, key='coef', basis='X_umap', shape=512)
        ax.imshow(img['n'] > 0, extent=img['extent'], origin='lower', cmap='Greys', alpha=.3)      # the grey layer
        ax.imshow(img['top'][0], extent=img['extent'], origin='lower', cmap='seismic',
                  vmin=-img['absmax'][0], vmax=img['absmax'][0])                                    # what umap_ncorr shows

    ``key``: one column of ``data.obs`` or a list of 1 to 16; all keys share one pass over the coordinates.  A cell PASSES
    for key k when ``obs[k]`` is finite and either ``obs[k + '_fdr'] <= fdr_thresh`` (default 0.1 as ``umap_ncorr``; a NaN
    fdr fails) or ``obs`` has no such column (``NAMPC1``: every cell with a value passes).  ``fdr_thresh`` given while a
    key has no fdr column raises ``KeyError``.  ``basis``: a key of ``data.obsm`` with the two columns ``components``, or an
    array-like (cells, 2).  ``shape``: an int or ``(height, width)``, each side in [1, 4096] and keys x height x width at
    most 2**22.  ``extent``: ``(x0, x1, y0, y1)``, finite and increasing, or ``None``: the min and max over the cells whose
    coordinates are both finite (an axis without width is widened by 0.5 either side; ``ValueError`` without any such
    cell).  ``radius``: an int in [0, 16], the footprint of a marker in pixels.

    Returns a dict; the arrays are ``[iy, ix]``, row 0 at ``y0`` (``origin='lower'``): ``extent`` (4-tuple, ``imshow``'s
    order), ``n`` int64[H, W] the cells with finite coordinates inside the extent whatever their value, ``n_outside`` those
    outside, ``keys``, and stacked per key ``[q, H, W]``: ``n_pass`` (int64), ``sum`` (0 where nothing passes), ``mean``
    (``sum / n_pass``, NaN where nothing passes), ``top`` / ``bottom`` the largest / smallest passing value (NaN where
    nothing passes; ``top`` is what scanpy's ``sort_order=True`` leaves visible), and ``absmax`` float64[q],
    ``np.abs(c).max()`` over the passing cells inside the extent (NaN when none passes).  With ``radius = r > 0`` ``top``
    and ``bottom`` are dilated by the disc ``dx**2 + dy**2 <= r**2`` (max / min over the disc, empty pixels ignored) and
    ``covered`` bool[H, W] is ``n > 0`` dilated the same way; counts, ``sum`` and ``mean`` stay per pixel.

    A cell on ``x1`` or ``y1`` belongs to the last pixel; counts, extremes and the extent are exact, sums take a fixed
    order: two runs give the same bits."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'coef_raster', 'counts, sums and extremes fold over row blocks: a follow-up')
    obs = data.obs
    keys = [key] if isinstance(key, str) else list(key)
    if not 1 <= len(keys) <= MAX_KEYS:
        raise ValueError('coef_raster takes 1 to %d keys per call, got %d' % (MAX_KEYS, len(keys)))
    for k in keys:
        if k not in obs:
            raise KeyError(k)
    has_fdr = np.array(['%s_fdr' % (k,) in obs for k in keys], dtype=np.int32)
    if fdr_thresh is not None and not has_fdr.all():
        raise KeyError('%s_fdr' % (keys[int(np.flatnonzero(has_fdr == 0)[0])],))
    thresh = FDR_THRESH if fdr_thresh is None else float(fdr_thresh)
    if isinstance(shape, (tuple, list)):
        if len(shape) != 2:
            raise ValueError('coef_raster: shape must be an int or (height, width), got %r' % (shape,))
        height, width = shape
    else:
        height = width = shape
    height, width = _int_in('height', height, 1, MAX_SIDE), _int_in('width', width, 1, MAX_SIDE)
    if len(keys) * height * width > MAX_PIXELS:
        raise ValueError('coef_raster: keys x height x width = %d x %d x %d exceeds 2**22' % (len(keys), height, width))
    radius = _int_in('radius', radius, 0, MAX_RADIUS)
    if extent is not None:
        extent = tuple(float(e) for e in extent)
        if len(extent) != 4 or not all(math.isfinite(e) for e in extent) or not (extent[1] > extent[0] and extent[3] > extent[2]):
            raise ValueError('coef_raster: extent must be (x0, x1, y0, y1), finite with x1 > x0 and y1 > y0, got %r' % (extent,))
    xy = _coordinates(data, basis, components, len(obs))
    V = np.ascontiguousarray(np.stack([numeric_column(obs, k) for k in keys]))
    FDR = None
    if has_fdr.any():
        FDR = np.zeros_like(V)
        for j, k in enumerate(keys):
            if has_fdr[j]:
                FDR[j] = numeric_column(obs, '%s_fdr' % (k,))
    r = engine.coef_raster(xy, V, FDR, has_fdr, thresh, extent, width, height, radius)
    n_pass = np.asarray(r['n_pass'], dtype=np.int64)
    total = np.asarray(r['sum'], dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(n_pass > 0, total / n_pass, np.nan)
    out = {'extent': tuple(float(e) for e in r['extent']), 'n': np.asarray(r['n'], dtype=np.int64),
           'n_outside': int(r['n_outside']), 'n_pass': n_pass, 'sum': total, 'mean': mean,
           'top': np.asarray(r['top'], dtype=np.float64), 'bottom': np.asarray(r['bottom'], dtype=np.float64),
           'absmax': np.asarray(r['absmax'], dtype=np.float64), 'keys': keys}
    if radius > 0:
        out['covered'] = np.asarray(r['covered'], dtype=bool)
    return out
