"""More than sixteen batches, on the CPU: the inputs of tests/test_gpu_batches_wide.py, their reference, and the proofs that
file relies on.

Sixteen batches is where the device's dispatch changes (csrc/rows.hip: BK_FAST; csrc/rows16.hip:launch_rowpass16): from
seventeen on, the batch kurtosis is k_batch_kurtosis and the ridge pass takes the LDS branch of k_resid_lowrank.  Here:

* kurtosis_longdouble -- _batch_kurtosis (_nam.py:78-82) stated in np.longdouble, the reference of every kurtosis
  comparison on the device (the f64 oracle rounds like the kernels and is itself held to it below);
* wide_input / kurt_case / ridge_case / nam_codes / wide_dataset -- the inputs;
* the oracle against kurtosis_longdouble on every one of those inputs at 1e-11 relative (worst seen: 1.3e-12), so that the
  device's bars of 1e-9 / 1e-8 test the kernels and not the conditioning of the inputs;
* the LDS budget of the factored ridge pass as the host states it against the kernel's own need, shape by shape;
* association() end to end through the CPU double of the engine with 20 and with 60 batches: the kept mask built on the host
  after a non-zero count of the device's QC, the optimistic first ridge taken back (plan.reselect) and a schedule of several
  ridges.
"""
import functools
import warnings
from argparse import Namespace

import numpy as np
import pandas as pd
import pytest

from fake_engine import FakeEngine
from helpers import relerr, fdr_rows
from oracle import cna_oracle as orc
from test_gpu_select_layouts import _x_ld

LONGDOUBLE_TOL = 1e-11          # f64 oracle against the longdouble statement, on these inputs
EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------------ reference
def kurtosis_longdouble(X, codes, nb):
    """_batch_kurtosis (_nam.py:78-82) in np.longdouble: per row, m4 / m2^2 (Pearson) over the means of the nb batches; a
    code of -1 is a sample of no batch; NaN where a batch is empty, and where scipy's kurtosis gives NaN (the batch means
    agree to rounding: m2 <= (eps mean)^2).  Returns float64."""
    X = np.asarray(X, dtype=np.longdouble)
    codes = np.asarray(codes)
    means = np.full((X.shape[0], nb), np.nan, dtype=np.longdouble)
    for b in range(nb):
        cols = np.flatnonzero(codes == b)
        if len(cols):
            means[:, b] = X[:, cols].sum(axis=1) / np.longdouble(len(cols))
    mean = means.mean(axis=1)
    d2 = (means - mean[:, None]) ** 2
    m2, m4 = d2.mean(axis=1), (d2 * d2).mean(axis=1)
    with np.errstate(all='ignore'):
        k = np.where(m2 <= (np.longdouble(EPS) * mean) ** 2, np.nan, m4 / (m2 * m2))
    return np.asarray(k, dtype=np.float64)


# --------------------------------------------------------------------------------------------------------- inputs
def uneven_codes(rs, N, nb):
    """A batch code per sample: every batch present, sizes uneven (the samples beyond one per batch crowd into the low
    codes), single-sample batches whenever N < 2 nb, and the order permuted, so that the batches are not runs of samples."""
    assert nb <= N
    codes = np.empty(N, dtype=np.int32)
    codes[:nb] = np.arange(nb)
    codes[nb:] = (nb * rs.rand(N - nb) ** 2).astype(np.int32)
    return codes[rs.permutation(N)]


def wide_input(n, N, nb, seed):
    """(X, codes): rows of rand / N, every seventh shifted by +1.0 -- a common offset a million times the spread of the batch
    means, the case where their deviations cancel -- and uneven_codes."""
    rs = np.random.RandomState(seed)
    X = rs.rand(n, N) / N
    X[::7] += 1.0
    return X, uneven_codes(rs, N, nb)


def with_unassigned(codes, seed, count=5):
    """`count` samples in no batch (code -1): taken from batches that keep another sample while there are such -- with one
    sample per batch (N = nb) their batches are left empty."""
    codes = codes.copy()
    sizes = np.bincount(codes)
    order = np.random.RandomState(seed).permutation(len(codes))
    for spare in (True, False):
        for s in order:
            if count and codes[s] >= 0 and (sizes[codes[s]] > 1 or not spare):
                sizes[codes[s]] -= 1
                codes[s] = -1
                count -= 1
    assert count == 0
    return codes


CONSTANT_ROWS = ((3, 0.375), (100, 1.0), (255, 2.0 ** -20))    # sums of equal such terms are exact: equal batch means


def with_constant_rows(X):
    X = X.copy()
    for row, v in CONSTANT_ROWS:
        X[row] = v
    return X


# (n, N, nb, variation) of test_gpu_batches_wide.py (a); 'rowpass16=0' is the same input under CNA_ROWPASS16=0
KURT_CASES = [(301, 20, 17, None), (301, 20, 17, 'constant'),
              (301, 64, 64, None), (301, 65, 65, None), (301, 65, 65, 'unassigned'),
              (257, 130, 128, None), (257, 130, 128, 'constant'),
              (257, 200, 129, None), (257, 200, 129, 'unassigned+empty'),
              (130, 260, 192, None), (130, 300, 193, None), (130, 300, 193, 'unassigned'),
              (100, 520, 256, None), (64, 1024, 256, None),
              (301, 100, 16, None), (301, 300, 16, None), (301, 100, 16, 'rowpass16=0')]
EMPTY_BATCH = 70


@functools.lru_cache(maxsize=None)
def kurt_case(n, N, nb, variation):
    """(X, codes, longdouble kurtosis) of one case of KURT_CASES; computed once, not to be written to."""
    X, codes = wide_input(n, N, nb, seed=n + N + nb)
    variation = variation or ''
    if 'unassigned' in variation:
        codes = with_unassigned(codes, seed=N)
    if 'empty' in variation:
        codes = np.where(codes == EMPTY_BATCH, -1, codes).astype(np.int32)
    if 'constant' in variation:
        X = with_constant_rows(X)
    ref = kurtosis_longdouble(X, codes, nb)
    for a in (X, codes, ref):
        a.setflags(write=False)
    return X, codes, ref


# (n, N, r, nb) of test_gpu_batches_wide.py (c)
RIDGE_CASES = [(1000, 100, 3, 17), (777, 64, 21, 20), (513, 130, 5, 65), (300, 260, 4, 129), (200, 520, 2, 40),
               (301, 300, 25, 24), (301, 124, 64, 60)]
RIDGE_FOLDED = RIDGE_CASES[:3]                   # ... run once more with their batches folded into sixteen
RIDGE_PAST_BUDGET = [(301, 126, 64, 60), (301, 128, 64, 60)]


def fold16(codes):
    return (np.asarray(codes) % 16).astype(np.int32)


@functools.lru_cache(maxsize=None)
def ridge_case(n, N, r, nb):
    """The inputs of one ridge pass, as tests/test_gpu_parity.py::test_sixteen_rows_per_wave_passes_vs_numpy builds them
    (uneven batches in place of its random ones), and numpy's results: a Namespace of X, Cm, W, y, codes, resid (centred and
    residualised, before the division), Xs (after it) and maxabs (max |coefficient|).  Computed once, not to be written to."""
    rs = np.random.RandomState(n + 3 * N + r)
    X = rs.randn(n, N) * rs.rand(1, N) + rs.randn(n, 1)
    codes = uneven_codes(rs, N, nb)
    y = rs.randn(N)
    Cm = rs.randn(N, r)
    Cm = Cm - Cm.mean(axis=0)
    W = np.linalg.solve(Cm.T.dot(Cm) + 0.3 * N * np.eye(r), Cm.T)
    Xc = X - X.mean(axis=1, keepdims=True)
    resid = Xc - Xc.dot(W.T).dot(Cm.T)
    Xs = resid / resid.std(axis=1, ddof=1)[:, None]
    maxabs = float(np.abs((Xs * y[None, :]).sum(axis=1) / N).max())
    for a in (X, codes, y, Cm, W, resid, Xs):
        a.setflags(write=False)
    return Namespace(X=X, Cm=Cm, W=W, y=y, codes=codes, resid=resid, Xs=Xs, maxabs=maxabs)


# (N, nb) of test_gpu_batches_wide.py (b): the NAM of synth.make_dataset(3001, N, k=15, seed=21) after three steps
NAM_CELLS = 3001
NAM_CASES = [(100, 20), (100, 70), (300, 20), (300, 70)]


def nam_codes(N, nb):
    return uneven_codes(np.random.RandomState(N + nb), N, nb)


# (n, N, batches, covariates, seed) of test_gpu_batches_wide.py (d); the seeds were picked with the oracle so that no
# cell's QC kurtosis is within 1e-9 of its threshold (test_end_to_end_inputs_have_no_qc_tie) and the QC drops cells where
# the table says so
E2E_CASES = [(3000, 100, 20, 1, 3100), (2000, 300, 40, 0, 2300), (3000, 128, 60, 4, 3128), (2500, 500, 13, 3, 3000)]
E2E_KW = dict(nsteps=3, Nnull=130, seed=5)
QC_TIE = 1e-9


@functools.lru_cache(maxsize=None)
def wide_dataset(n, N, nb, n_covs, seed):
    """(data, meta) of synth.make_dataset on the CPU-built graph (the same on every machine), with an uneven `batches` Series
    of nb levels over the samples."""
    from cna_amd import synth
    data, meta = synth.make_dataset(n, N, k=15, seed=seed, n_covs=n_covs, builder='cpu')
    codes = uneven_codes(np.random.RandomState(seed + 1), N, nb)
    meta['batches'] = pd.Series(codes.astype(np.int64), index=meta['y'].index)
    return data, meta


@functools.lru_cache(maxsize=None)
def e2e_reference(n, N, nb, n_covs, seed):
    data, meta = wide_dataset(n, N, nb, n_covs, seed)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return orc.association(data, meta['y'], 'id', covs=meta['covs'], batches=meta['batches'], mode='f64', **E2E_KW)


@functools.lru_cache(maxsize=None)
def qc_margin(n, N, nb, n_covs, seed):
    """min over the cells of |kurtosis - threshold| / threshold of the oracle's QC (_nam.py:94-96) on wide_dataset."""
    data, meta = wide_dataset(n, N, nb, n_covs, seed)
    nm = orc.nam(data, 'id', batches=None, nsteps=E2E_KW['nsteps'], mode='f64')
    b = meta['batches'].reindex(nm['labels']).values          # (a sample without cells is not part of the NAM)
    levels = np.unique(b)
    kurt = orc.batch_kurtosis(nm['nam'], np.searchsorted(levels, b), len(levels))
    assert not np.isnan(kurt).any()
    thr = max(6, 2 * np.median(kurt))
    return float(np.abs(kurt - thr).min() / thr)


def assert_matches_oracle(res, data, ref):
    """The assertions and bars of tests/test_gpu_parity.py::test_association_wide_sample_axis_vs_oracle."""
    from helpers import sign_align
    assert int(res.k) == ref['k'] and res.p == ref['p'] and np.array_equal(res.kept, ref['kept'])
    assert relerr(res.nam.values.T, ref['nam']) < 1e-13
    assert relerr(res.namresid.values.T, ref['namresid']) < 1e-9
    assert relerr(res.ncorrs.values, ref['ncorrs']) < 1e-9
    assert relerr(res.namresid_svs.values, ref['svs']) < 1e-9
    np.testing.assert_allclose(res.nullminps, ref['nullminps'], rtol=1e-7)
    T = fdr_rows(res.fdrs, ref['fdrs'], ref['ncorrs'])
    assert np.array_equal(res.fdrs.num_detected.values[:T], ref['fdrs']['num_detected'][:T])
    np.testing.assert_allclose(res.fdrs.fdr.values[:T], ref['fdrs']['fdr'][:T], rtol=1e-8, atol=1e-13)
    np.testing.assert_allclose(data.obs['coef_fdr'].values, ref['obs_coef_fdr'], rtol=1e-8, atol=1e-13)
    V, Vref = sign_align(res.namresid_nbhdXpc.values, ref['V'], int(res.k))
    assert relerr(V, Vref) < 1e-6


# ------------------------------------------------------------------------------------------------ the inputs, checked
def _assert_oracle_is_benign(name, X, codes, nb, ref=None):
    ref = kurtosis_longdouble(X, codes, nb) if ref is None else ref
    with np.errstate(all='ignore'):
        got = orc.batch_kurtosis(np.asarray(X), np.asarray(codes), nb)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=name)
    ok = ~np.isnan(ref)
    err = float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]))) if ok.any() else 0.0
    print('%s: oracle against longdouble %.2e (bound %g)' % (name, err, LONGDOUBLE_TOL))
    assert err <= LONGDOUBLE_TOL, (name, err)
    return err


@pytest.mark.parametrize('n,N,nb,variation', KURT_CASES)
def test_kurtosis_inputs_are_what_they_claim(n, N, nb, variation):
    variation = variation or ''
    X, codes, ref = kurt_case(n, N, nb, variation)
    base = wide_input(n, N, nb, n + N + nb)[1]
    sizes = np.bincount(base, minlength=nb)
    assert base.min() == 0 and (sizes > 0).all()                               # every batch present
    assert N == nb or sizes.max() > sizes.min()                                 # uneven
    assert N >= 2 * nb or (sizes == 1).any()                                    # single-sample batches
    assert (np.diff(base) < 0).any()                                            # not grouped
    unassigned = (5 if 'unassigned' in variation else 0) + (int(sizes[EMPTY_BATCH]) if 'empty' in variation else 0)
    assert (codes < 0).sum() == unassigned and (codes[codes >= 0] == base[codes >= 0]).all()
    left = np.bincount(codes[codes >= 0], minlength=nb)
    if 'empty' in variation:
        assert left[EMPTY_BATCH] == 0
    if (left == 0).any():
        assert np.isnan(ref).all() and ('empty' in variation or N == nb)
    elif 'constant' in variation:
        rows = [r for r, _ in CONSTANT_ROWS]
        assert np.isnan(ref[rows]).all() and np.isnan(ref).sum() == len(rows)
    else:
        assert not np.isnan(ref).any()


@pytest.mark.parametrize('n,N,nb,variation', KURT_CASES)
def test_oracle_agrees_with_longdouble_on_the_kurtosis_inputs(n, N, nb, variation):
    X, codes, ref = kurt_case(n, N, nb, variation)
    _assert_oracle_is_benign('kurtosis %s' % ((n, N, nb, variation),), X, codes, nb, ref)


@pytest.mark.parametrize('n,N,r,nb', RIDGE_CASES)
def test_oracle_agrees_with_longdouble_on_the_residualised_rows(n, N, r, nb):
    c = ridge_case(n, N, r, nb)
    _assert_oracle_is_benign('ridge %s' % ((n, N, r, nb),), c.resid, c.codes, nb)
    if (n, N, r, nb) in RIDGE_FOLDED:
        _assert_oracle_is_benign('ridge %s folded' % ((n, N, r, nb),), c.resid, fold16(c.codes), 16)


@pytest.mark.parametrize('N,nb', NAM_CASES)
def test_oracle_agrees_with_longdouble_on_the_nam(N, nb):
    """(the device's NAM equals the f64 oracle's bit for bit: tests/test_gpu_parity.py)"""
    from cna_amd import synth
    data, _ = synth.make_dataset(NAM_CELLS, N, k=15, seed=21, builder='cpu')
    nm = orc.nam(data, 'id', batches=None, nsteps=3, mode='f64')
    assert nm['nam'].shape[1] == N
    _assert_oracle_is_benign('nam %s' % ((N, nb),), nm['nam'], nam_codes(N, nb), nb)


# ------------------------------------------------------------------------------------------------ the LDS budget
def _kernel_lds(r, N, bk):
    """csrc/rows.hip:launch_resid_lowrank's dynamic LDS in bytes, restated: W and C^T, and with the batch kurtosis a row of X
    per wave."""
    return 8 * (2 * r * N + (4 * _x_ld(N) if bk else 0))


@pytest.mark.parametrize('bk', [True, False])
def test_factored_ridge_pass_is_admitted_only_within_the_kernels_lds(bk):
    """_resid_run takes engine.resid_lowrank_bk (bk) / engine.resid_lowrank where _lowrank_ok says so; the library refuses
    either beyond 128 KB of LDS -- after it has voided X -- so the predicate must hold exactly where the kernel's need fits."""
    from cna_amd.tools import _nam
    engine = Namespace(resid_lowrank=None, resid_lowrank_bk=None)
    plan = Namespace(r=0, N=0)
    bad = []
    for N in range(2, 1025):
        for r in range(1, 273):
            plan.r, plan.N = r, N
            admitted = _nam._lowrank_ok(engine, plan, bk=True) if bk else _nam._lowrank_ok(engine, plan)
            if bool(admitted) != (_kernel_lds(r, N, bk) <= 131072):
                bad.append((N, r))
    assert not bad, (len(bad), bad[:8])
    plan.r, plan.N = 0, 100
    assert not _nam._lowrank_ok(engine, plan)
    assert not _nam._lowrank_ok(Namespace(), Namespace(r=3, N=100))          # (an engine without the factored pass)


@pytest.mark.parametrize('N,r,fits', [(124, 64, True), (126, 64, False), (128, 64, False), (500, 16, False), (400, 20, False),
                                      (1000, 8, False), (300, 25, True)])
def test_lds_budget_at_the_shapes_that_were_refused(N, r, fits):
    """2 r N doubles fit 128 KB at every one of these; with the kurtosis's row buffers some do not.  Those take the ridge
    by ridge route (resid_lowrank without the kurtosis, which fits, then batch_kurtosis)."""
    from cna_amd.tools import _nam
    engine = Namespace(resid_lowrank=None)
    assert _nam._lowrank_ok(engine, Namespace(r=r, N=N))
    assert _nam._lowrank_ok(engine, Namespace(r=r, N=N), bk=True) == fits
    assert (_kernel_lds(r, N, True) <= 131072) == fits


# ------------------------------------------------------------------------------------- end to end on the CPU double
class DeviceLikeEngine(FakeEngine):
    """The CPU double with the entry points of the device engine that decide which route tools/_nam.py takes: the QC
    decided "on the device" (stat_qc), the selection that counts zero-variance rows, and the factored ridge passes --
    refusing, as the library does, a pass whose LDS need is beyond 128 KB."""

    def stat_qc(self):
        self.calls.append(('stat_qc',))
        med = self.stat_median()
        thr = max(6, 2 * med)
        with np.errstate(invalid='ignore'):
            return med, thr, int(np.count_nonzero(~(self.stat < thr)))

    def select_checked(self, keep_global, colmap):
        self.calls.append(('select_checked',))
        self.select(keep_global, colmap)
        with np.errstate(all='ignore'):
            return int((self.X.std(axis=1, ddof=1) == 0).sum())

    def _lowrank(self, Cmat, W, center, bk):
        r, N = np.shape(Cmat)[1], self.X.shape[1]
        if _kernel_lds(r, N, bk) > 131072:
            self.X = None                                   # (the library has voided X by then)
            raise RuntimeError('cna_resid_lowrank: r x N too large for LDS')
        if center:
            self.X = self.X - self.X.mean(axis=1, keepdims=True)
        if r:
            self.X = self.X - self.X.dot(np.asarray(W).T).dot(np.asarray(Cmat).T)

    def resid_lowrank(self, Cmat, W, center=True, standardize=False, y=None):
        self.calls.append(('resid_lowrank', np.shape(Cmat)[1]))
        self._lowrank(Cmat, W, center, False)
        if standardize:
            self.standardize(center=False)
        return self.ncorrs(y)[1] if y is not None else None

    def resid_lowrank_bk(self, Cmat, W, y, batch_codes, n_batches):
        self.calls.append(('resid_lowrank_bk', np.shape(Cmat)[1]))
        self._lowrank(Cmat, W, True, True)
        self.batch_kurtosis(1, batch_codes, n_batches)
        med = self.stat_median()
        self.standardize(center=False)
        return self.ncorrs(y)[1], med


def _run_double(case):
    import cna_amd as cna
    data, meta = wide_dataset(*case)
    eng = DeviceLikeEngine()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = cna.tl.association(data, meta['y'], 'id', covs=meta['covs'], batches=meta['batches'], return_full=True,
                                 engine=eng, **E2E_KW)
    return res, data, eng, e2e_reference(*case)


HOST_CASES = [(1500, 100, 20, 1, 1600), (1500, 100, 50, 1, 1600), (1500, 128, 60, 4, 1628)]


@pytest.mark.parametrize('case', HOST_CASES)
def test_association_with_many_batches_on_the_cpu_double(case):
    """20 batches (the schedule ends at its first ridge), 50 batches (it does not: the optimistic pass is taken back and eight
    ridges are walked) and 60 uneven batches with 4 covariates on 128 samples (r = 64: the factors alone fill the 128 KB, so
    the pass with the kurtosis is past the budget and the schedule runs ridge by ridge from the start), against the f64
    oracle."""
    res, data, eng, ref = _run_double(case)
    assert_matches_oracle(res, data, ref)
    names = [c[0] for c in eng.calls]
    assert 'stat_qc' in names
    n, N, nb, n_covs, _ = case
    if _kernel_lds(nb + n_covs, N, True) > 131072:
        assert 'resid_lowrank_bk' not in names and names.count('resid_lowrank') == len(ref['ridge_log']) + 1
    else:
        assert names.count('resid_lowrank_bk') == 1
        if len(ref['ridge_log']) > 1:           # the optimistic first ridge was taken back and the schedule walked
            assert names.count('select_checked') == 2 and names.count('resid_lowrank') == len(ref['ridge_log']) + 1


def test_cpu_double_cases_cover_the_host_logic():
    """Between them the cases above drop cells in the QC (the kept mask is then built on the host) and go past the first
    ridge."""
    refs = [e2e_reference(*case) for case in HOST_CASES]
    assert any(0 < r['kept'].sum() < len(r['kept']) for r in refs)
    assert any(len(r['ridge_log']) > 1 for r in refs)


@pytest.mark.parametrize('case', E2E_CASES)
def test_end_to_end_inputs_have_no_qc_tie(case):
    """No cell of the device's end-to-end cases has a QC kurtosis within 1e-9 of the threshold: a cell the device keeps
    and the oracle drops (or the reverse) is then an error of the kernel, not a tie."""
    assert qc_margin(*case) > QC_TIE


def test_one_end_to_end_input_drops_cells():
    """(the oracle's NAM walk only: its full association on these inputs is the device test's work)"""
    dropped = []
    for case in E2E_CASES:
        data, meta = wide_dataset(*case)
        nm = orc.nam(data, 'id', batches=meta['batches'], nsteps=E2E_KW['nsteps'], mode='f64')
        dropped.append(int((~nm['keep']).sum()))
    assert any(0 < d < case[0] for d, case in zip(dropped, E2E_CASES)), dropped
