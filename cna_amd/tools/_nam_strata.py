"""``cna.tl.nam_strata``: the NAM mass of every sample in every cluster, on the device.

The reference's demo ends on "working directly with the NAM" (demo/demo.ipynb, section 3.2), and every analysis ends on a
plot of the phenotype against the abundance of the associated population in each sample.  Both are sums over the cell axis
of the cells x samples NAM (_nam.py:73), aggregated the way utils/multisample.py:4-11 aggregates per-cell columns:

- how much of sample s lies in cluster L: the sum of NAM[i, s] over the cells i of L, the diffused version of the cluster
  proportions;
- how much of sample s lies in the expanded / depleted neighbourhoods: the same sum with the per-cell coefficient, or a mask
  of the cells that pass the FDR, as weights.

The route through ``cna.tl.nam`` takes the whole NAM to the host and groups it there; here it is read once where it is and
levels x samples come back (csrc/nam_bins.hip, ``cna_matrix_to_bins``).  This module is the host side only: the codes, the
weights, the argument checks and the frames.
"""
import numpy as np
import pandas as pd

from .._ffi import MAT_NAM
from ..engine import get_engine
from ._genes import numeric_column
from ._nam import _nam_device, refuse_sharded, sample_codes_cached
from ._strata import FDR_THRESH, levels_of

MAX_WEIGHTS = 16
MAX_SUMS = 4096         # weight columns x levels of one device pass


def signed_passes(obs, key, fdr_thresh=None):
    """(expanded, depleted), one bool per cell: ``obs[key]`` finite and > 0 / < 0, and ``obs[key + '_fdr'] <= fdr_thresh``
    (default 0.1; a NaN fdr fails) where ``obs`` has that column.  KeyError without ``key``, and for ``fdr_thresh`` without the
    fdr column.  The rule of ``nam_strata(sign_of=...)`` and of ``coef_populations``."""
    if key not in obs:
        raise KeyError(key)
    fkey = '%s_fdr' % (key,)
    has_fdr = fkey in obs
    if not has_fdr and fdr_thresh is not None:
        raise KeyError(fkey)
    v = numeric_column(obs, key)
    with np.errstate(invalid='ignore'):
        passes = np.isfinite(v)
        if has_fdr:
            passes &= numeric_column(obs, fkey) <= (FDR_THRESH if fdr_thresh is None else float(fdr_thresh))
        return passes & (v > 0), passes & (v < 0)


def nam_strata(data, stratification, sid_name, weights=None, sign_of=None, fdr_thresh=None, keep=None,
               return_counts=False, nsteps=None, self_weight=1, engine=None):
    """Samples x levels of ``data.obs[stratification]``: the sum of the NAM over the cells of every level.

    The NAM is the one ``cna.tl.nam(data, sid_name, nsteps=nsteps, self_weight=self_weight)`` walks; one that the device
    already holds for these inputs (after ``cna.tl.association`` on the same data, say) is reused and no diffusion runs.
    Rows are the samples in the order of ``cna.tl.nam``'s frame, the index named ``sid_name``; columns are the levels in
    order of first appearance (as ``cna.tl.coef_strata``), NaN / None levels left out, at most 1024.  With every cell in a
    level and no weights every row sums to 1, as the rows of the NAM do.

    ``keep``: bool per cell (``cna.tl.nam``'s second result); False leaves the cell out.
    ``weights``: None, the name of a numeric column of ``data.obs`` (the sums are weighted by it; the result is still one
    frame), or a list of 1 to 16 names: a dict name -> frame from ONE pass over the NAM.  A cell whose weight is zero, NaN or
    infinite is left out of that column only.
    ``sign_of='coef'`` (not together with ``weights``) returns ``{'pos': frame, 'neg': frame}``: the NAM mass of every
    sample in the expanded / depleted neighbourhoods of every level -- weight 1 on the cells with a finite coefficient
    > 0 / < 0, which must also have ``fdr <= fdr_thresh`` (default 0.1; a NaN fdr fails) when ``data.obs`` has
    ``sign_of + '_fdr'``.  ``fdr_thresh`` without that column is a KeyError.
    ``return_counts=True`` returns ``(result, counts)``: a frame levels x (one column per result frame) of the contributing
    cells, int64."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'nam_strata', 'the per-level sums add over row blocks: an all-reduce away')
    obs = data.obs
    for k in (stratification, sid_name):
        if k not in obs:
            raise KeyError(k)
    if weights is not None and sign_of is not None:
        raise ValueError('nam_strata: give weights or sign_of, not both')
    if fdr_thresh is not None and sign_of is None:
        raise ValueError('nam_strata: fdr_thresh goes with sign_of')
    n = len(obs)
    single = weights is None or isinstance(weights, str)
    names, W = None, None
    if sign_of is not None:
        W = np.stack(signed_passes(obs, sign_of, fdr_thresh)).astype(np.float64)
        names, single = ['pos', 'neg'], False
    elif weights is not None:
        names = [weights] if isinstance(weights, str) else list(weights)
        if not 1 <= len(names) <= MAX_WEIGHTS:
            raise ValueError('nam_strata: %d weight columns, must lie in [1, %d]' % (len(names), MAX_WEIGHTS))
        for k in names:
            if k not in obs:
                raise KeyError(k)
        W = np.stack([numeric_column(obs, k) for k in names])
    if keep is not None:
        keep = np.asarray(keep)
        if keep.dtype != bool or keep.shape != (n,):
            raise ValueError('nam_strata: keep must be one bool per cell')
    codes, levels = levels_of(obs, stratification, 'nam_strata')
    q = 1 if W is None else len(W)
    if q * len(levels) > MAX_SUMS:
        raise ValueError('nam_strata: %d weight columns x %d levels, at most %d sums in one pass' % (q, len(levels), MAX_SUMS))
    if keep is not None:
        codes = np.where(keep, codes, np.int32(-1)).astype(np.int32)
    labels, _ = _nam_device(engine, data, sid_name, nsteps=nsteps, self_weight=self_weight,
                            codes_labels=sample_codes_cached(obs[sid_name]))
    sums, cnt = engine.matrix_to_bins(MAT_NAM, codes, W, n_bins=len(levels))
    samples = pd.Index(labels, name=sid_name)
    cols = pd.Index(levels, name=stratification)
    frames = [pd.DataFrame(np.ascontiguousarray(sums[j].T), index=samples, columns=cols) for j in range(q)]
    result = frames[0] if single else dict(zip(names, frames))
    if not return_counts:
        return result
    counts = pd.DataFrame(np.asarray(cnt, dtype=np.int64).T, index=cols,
                          columns=['n'] if names is None else list(names))
    return result, counts
