"""cna.tl.nam_strata and Engine.matrix_to_bins on the device's own NAM and X (run with -m gpu on an MI355X): the mapping
from the caller's cells to the matrix' rows, the lazy NAM, and an X that is a selection.

The bound, per entry of a result: |got - want| <= (m + 2) 2^-52 sum |w x| over the m contributing cells -- each side is a
float64 sum of the same m products in some order (at most m - 1 roundings of partial sums that never exceed sum |w x| in
magnitude, 2^-53 each, on either side), and each product is rounded once (numpy) or not at all (the device's fused
multiply-add).  Counts are exact."""
import warnings

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
N_CELLS, N_SAMPLES = 3000, 70          # above 64 samples: the deferred last step and its by-product can occur


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    keep = e.reuse_nam
    e.reuse_nam = True
    yield e
    e.reuse_nam = keep
    e.drop_expression()


@pytest.fixture(scope='module')
def case():
    from cna_amd import synth
    data, meta = synth.make_dataset(N_CELLS, N_SAMPLES, k=15, seed=70)
    rs = np.random.RandomState(1)
    lev = np.array(['L%02d' % i for i in range(12)], dtype=object)[rs.randint(0, 12, N_CELLS)]
    lev[rs.rand(N_CELLS) < 0.05] = None
    data.obs['lev'] = lev
    data.obs['w1'] = rs.randn(N_CELLS)
    w2 = rs.rand(N_CELLS)
    w2[rs.rand(N_CELLS) < 0.2] = 0.0
    w2[7] = np.nan
    data.obs['w2'] = w2
    return data, meta, rs.rand(N_CELLS) > 0.25


def host_sums(M, codes, W, n_bins):
    """(sums, sum of |terms|, contributing cells) over the rows of M (cells x columns, caller's order) in numpy"""
    W = np.ones((1, len(codes))) if W is None else np.asarray(W, dtype=np.float64)
    sums = np.zeros((len(W), n_bins, M.shape[1]))
    mag = np.zeros_like(sums)
    cnt = np.zeros((len(W), n_bins), dtype=np.int64)
    for j, w in enumerate(W):
        ok = (codes >= 0) & np.isfinite(w) & (w != 0)
        for b in range(n_bins):
            rows = np.flatnonzero(ok & (codes == b))
            cnt[j, b] = len(rows)
            if len(rows):
                terms = w[rows, None] * M[rows]
                sums[j, b], mag[j, b] = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    return sums, mag, cnt


def worst_ratio(got, want, mag, cnt):
    bound = (cnt[:, :, None] + 2) * EPS * mag
    err = np.abs(got - want)
    assert (err[bound == 0] == 0).all()
    return float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0))


def _codes(data, keep=None):
    codes, levels = pd.factorize(data.obs['lev'])
    codes = codes.astype(np.int32)
    if keep is not None:
        codes[~keep] = -1
    return codes, list(levels)


def test_cells_are_mapped_to_the_device_order(eng, case):
    import cna_amd as cna
    data, _, keep = case
    res, counts = cna.tl.nam_strata(data, 'lev', 'id', weights=['w1', 'w2'], keep=keep, return_counts=True, nsteps=3, engine=eng)
    plain, plain_n = cna.tl.nam_strata(data, 'lev', 'id', keep=keep, return_counts=True, nsteps=3, engine=eng)
    assert eng.perm is not None and not np.array_equal(eng.perm, np.arange(N_CELLS))       # the device cell order is active
    nam = eng.nam_full()
    assert nam.shape == (N_CELLS, N_SAMPLES)
    codes, levels = _codes(data, keep)
    W = np.stack([data.obs['w1'].values, data.obs['w2'].values])
    want, mag, cnt = host_sums(nam, codes, W, len(levels))
    got = np.stack([res[k].values.T for k in ('w1', 'w2')])
    assert list(res['w1'].columns) == levels and list(res['w1'].index) == sorted(set(data.obs['id']))
    np.testing.assert_array_equal(counts.values.T, cnt)
    assert cnt[1].sum() < cnt[0].sum()                       # the zero and NaN weights of w2 left cells out of it alone
    r1 = worst_ratio(got, want, mag, cnt)
    want0, mag0, cnt0 = host_sums(nam, codes, None, len(levels))
    np.testing.assert_array_equal(plain_n.values.T, cnt0)
    r0 = worst_ratio(plain.values.T[None], want0, mag0, cnt0)
    print('nam_strata against numpy over nam_full(): largest |err| / bound %.3g (weighted), %.3g (plain)' % (r1, r0))
    assert r1 <= 1.0 and r0 <= 1.0
    everyone = cna.tl.nam_strata(data, 'id', 'id', nsteps=3, engine=eng)      # every cell in a level: NAM rows sum to 1
    assert np.abs(everyone.values.sum(axis=1) - 1.0).max() <= 1e-12


def test_a_lazy_nam_is_produced_and_nothing_is_disturbed(eng, monkeypatch):
    """An association on a graph that is new to the device, on the schedule of large inputs: its last walk step may leave
    the selection pass's results instead of the NAM (cna_nam_select_hint), which is then one more run of that step away."""
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd.tools import _association as A
    monkeypatch.setattr(A, '_DEFER_LAST_CELLS', 0)
    data, meta = synth.make_dataset(N_CELLS, N_SAMPLES, k=15, seed=71)
    rs = np.random.RandomState(4)
    data.obs['lev'] = np.array(['L%02d' % i for i in range(9)], dtype=object)[rs.randint(0, 9, N_CELLS)]
    kw = dict(nsteps=3, Nnull=100, seed=1, engine=eng)
    eng.prof_reset()
    eng.prof_enable(True)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            p1 = cna.tl.association(data, meta['y'], 'id', **kw)
        eng.sync()
        before = eng.prof()
        lazy = 'select' not in before                          # the last step did the selection pass: no NAM was written
        assert lazy
        epoch = eng.nam_epoch
        res, counts = cna.tl.nam_strata(data, 'lev', 'id', sign_of='coef', return_counts=True, nsteps=3, engine=eng)
        after = eng.prof()
    finally:
        eng.prof_enable(False)
    assert eng.nam_epoch == epoch                              # no new walk ...
    steps = [after.get(k, (0, 0))[1] - before.get(k, (0, 0))[1] for k in ('nam_first', 'nam_step', 'nam_step_sparse')]
    assert steps == [0, 1 if lazy else 0, 0], (lazy, steps)    # ... only the last step once more where the NAM was lazy
    assert after['matrix_bins_sum'][1] == 1 and after['matrix_bins_sort'][1] == 1
    coef, fdr = data.obs['coef'].values, data.obs['coef_fdr'].values
    with np.errstate(invalid='ignore'):
        W = np.stack([np.isfinite(coef) & (coef > 0) & (fdr <= 0.1), np.isfinite(coef) & (coef < 0) & (fdr <= 0.1)]).astype(float)
    codes, levels = _codes(data)
    want, mag, cnt = host_sums(eng.nam_full(), codes, W, len(levels))
    assert eng.nam_epoch == epoch
    np.testing.assert_array_equal(counts.values.T, cnt)
    ratio = worst_ratio(np.stack([res['pos'].values.T, res['neg'].values.T]), want, mag, cnt)
    print('sign_of after an association (NAM lazy: %s): %d / %d cells pass, largest |err| / bound %.3g'
          % (lazy, cnt[0].sum(), cnt[1].sum(), ratio))
    assert ratio <= 1.0
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        p2 = cna.tl.association(data, meta['y'], 'id', **kw)
    assert p2 == p1


def test_a_selected_x_takes_the_kept_cells_only(eng):
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd._ffi import MAT_X
    data, meta = synth.make_dataset(3000, 40, k=15, seed=11, n_batches=10, n_covs=2, builder='cpu')
    # one population's cells all from batch-0 samples: their neighbourhoods fail the batch-kurtosis QC
    cl, b = meta['cluster'], meta['batches'].values
    sid = np.asarray(data.obs['id']).copy()
    target = np.flatnonzero(cl == np.bincount(cl).argmax())
    sid[target] = np.random.RandomState(3).choice(np.flatnonzero(b == 0), size=len(target))
    data.obs['id'] = sid
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = cna.tl.association(data, meta['y'], 'id', batches=meta['batches'], covs=meta['covs'], return_full=True,
                                 nsteps=3, Nnull=50, seed=1, engine=eng)
    kept = np.asarray(res.kept, dtype=bool)
    assert 0 < (~kept).sum() < len(kept) and eng.perm is not None
    rs = np.random.RandomState(2)
    codes = rs.randint(-1, 9, len(kept)).astype(np.int32)
    W = rs.randn(3, len(kept))
    W[rs.rand(3, len(kept)) < 0.2] = 0.0
    X = eng.x_full()                                           # kept cells x samples, caller's order
    assert X.shape[0] == kept.sum()
    for weights in (W, None):
        got, n = eng.matrix_to_bins(MAT_X, codes, weights, n_bins=9)
        want, mag, cnt = host_sums(X, codes[kept], None if weights is None else weights[:, kept], 9)
        np.testing.assert_array_equal(n, cnt)                  # a dropped cell contributes nothing
        ratio = worst_ratio(got, want, mag, cnt)
        print('X after a selection that dropped %d cells, q = %d: largest |err| / bound %.3g'
              % ((~kept).sum(), 0 if weights is None else 3, ratio))
        assert ratio <= 1.0
