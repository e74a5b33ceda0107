"""What cna.tl.association does once the device has answered (reference _association.py:55-129, :223-237), for both
call paths -- the general one (tools/_association.py) and the two-call one (tools/_fast.py): the verdict with its two
warnings, the result namespace, the two data.obs columns as the call found them.  The paths differ in
how they schedule the device; what they make of its answers is written here, once."""
import warnings

import numpy as np
import pandas as pd

from ._nam import _defer_pcs

# everything but the three cells x samples frames is materialised for return_full=True, like upstream
FULL_FIELDS = ('ncorrs', 'fdrs', 'namresid_sampleXpc', 'namresid_svs', 'namresid_varexp', 'yresid', 'beta')


def _rule_cells(data, engine):
    shard = getattr(data, 'uns', {}).get('cna_shard') if hasattr(data, 'uns') else None
    if shard:
        return -(-int(shard['n_global']) // max(1, int(getattr(engine, 'nranks', 1))))
    return len(data.obs)


def holds_last_step(data, engine, nsteps, nsamples, min_cells):
    """The walk's last step is held back so that it can take the selection pass along: the part of that rule both
    paths share, so that they run the same kernels (each adds its own conditions; _nam._nam_device keeps a guard).
    ``min_cells``: _association._DEFER_LAST_CELLS."""
    return nsteps >= 3 and nsamples > 64 and _rule_cells(data, engine) >= min_cells


def kept_pcs(N, max_frac_pcs, ks):
    """The reference's npcs (_association.py:207), as it writes it: raises for a tuple ks, or an ndarray of more than two."""
    return min(N, max([10] + [int(max_frac_pcs * N)] + [ks if ks is not None else []][0]))


def verdict(best, pv, r2v, ks, Nnull):
    """-> k, p, r2, pfinal, nullminps, nullr2s from the global F-tests of the observed phenotype (entry 0) and the
    permutations (_association.py:55-62, :84-88), with the reference's two warnings."""
    if (best < 0).any():
        raise ValueError('All-NaN slice encountered')        # np.nanargmin in _minp_stats
    k, p, r2 = ks[best[0]], pv[0], r2v[0]
    if k == max(ks):
        warnings.warn(('data supported use of {} NAM PCs, which is the maximum considered. ' +
                       'Consider allowing more PCs by using the "ks" argument.').format(k))
    nullminps, nullr2s = pv[1:], r2v[1:]
    hits = (nullminps <= p + 1e-8).sum()
    pfinal = (hits + 1) / (Nnull + 1)
    if hits == 0:
        warnings.warn('global association p-value attained minimal possible value. ' +
                      'Consider increasing Nnull')
    return k, p, r2, pfinal, nullminps, nullr2s


def sample_fields(res, pcs, Uk, Mv, y_std, index, ks, npcs, n_cells, verdict, fdrs, fdr_5p_t, fdr_10p_t):
    """The chosen model (_association.py:69-74) and every sample-sized field of the result.  ``Uk``: the leading
    eigenvectors the F-tests ran on; ``pcs``: GramPCs -- what shows the PC signs (U, beta) comes from LAPACK's SVD of G
    like upstream's (_nam.py:105, _association.py:70-72) and is built only when somebody reads it.  ``index``: the
    analysed samples; ``n_cells``: a callable (all ranks' cells); ``verdict``: what verdict() returned; ``fdrs``:
    (thresholds, fdr, num_detected), or None without the local test."""
    k, _, r2, pfinal, nullminps, nullr2s = verdict
    ycond_v = Mv.dot(y_std)
    ycond_v = ycond_v / ycond_v.std(ddof=1)
    beta_k = Uk[:, :k].T.dot(ycond_v)                   # up to the sign of every PC
    yhat = Uk[:, :k].dot(beta_k)                         # sign free
    r2_perpc = (beta_k / np.sqrt(ycond_v.dot(ycond_v))) ** 2
    nU = len(pcs)

    def names():
        return ['PC' + str(i) for i in range(1, nU + 1)]
    res._defer('namresid_sampleXpc', lambda: pd.DataFrame(pcs.U, index=index, columns=names()))
    res._defer('namresid_svs', lambda: pd.Series(pcs.svs, index=names())[:npcs])
    res._defer('namresid_varexp', lambda: pd.Series(pcs.svs, index=names()) / nU / n_cells())
    res._defer('yresid', lambda: pd.Series(ycond_v, index=index))
    res._defer('beta', lambda: pcs.U[:, :k].T.dot(ycond_v))
    if fdrs is None:
        res.fdrs = None
    else:
        thresholds, fdr_vals, num_detected = fdrs
        res._defer('fdrs', lambda: pd.DataFrame({'threshold': thresholds, 'fdr': fdr_vals, 'num_detected': num_detected}))
    res.__dict__.update({'p': pfinal, 'nullminps': nullminps, 'k': k, 'fdr_5p_t': fdr_5p_t, 'fdr_10p_t': fdr_10p_t,
                         'yresid_hat': yhat, 'ks': ks, 'r2': r2, 'r2_perpc': r2_perpc, 'nullr2_mean': nullr2s.mean(),
                         'nullr2_std': nullr2s.std()})


def cell_fields(res, engine, pcs, kept, colmap, sample_index, cell_index, nam_epoch, coef_kept):
    """The cells-sized fields: fetched from the device (nam, namresid_nbhdXpc) or built from the stored column
    (``coef_kept``: the values data.obs holds) when they are read."""
    _defer_pcs(res, engine, pcs, cell_index)
    res.kept = kept

    def fetch_nam():
        if engine.nam_epoch != nam_epoch:
            raise RuntimeError('res.nam lives on the GPU and a later cna_amd call has replaced it; '
                               'read it (or call res.materialize()) before running the next analysis')
        return pd.DataFrame(engine.nam_full(keep=kept, cols=colmap, transposed=True), index=sample_index,
                            columns=cell_index(), copy=False)
    res._defer('nam', fetch_nam)
    res._defer('ncorrs', lambda: pd.Series(coef_kept if kept.all() else coef_kept[kept], index=cell_index()))


class ObsSnapshot:
    """Columns of data.obs as a call found them.  The call sets ``written`` when it first writes one; restore() then
    puts every column back as it was (one that was not there is deleted), once."""

    def __init__(self, obs, *keys):
        self._obs = obs
        self._prev = {key: obs[key] if key in obs else None for key in keys}
        self.written = False

    def had(self, key):
        return self._prev[key] is not None

    def put_back(self, key):
        if self._prev[key] is not None:
            self._obs[key] = self._prev[key]
        elif key in self._obs:
            del self._obs[key]

    def restore(self):
        if self.written:
            self.written = False
            for key in self._prev:
                self.put_back(key)
