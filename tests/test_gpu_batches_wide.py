"""Batch kurtosis and the ridge pass beyond sixteen batches (run with -m gpu on an MI355X).

Sixteen is where the dispatch changes (csrc/rows.hip: BK_FAST; csrc/rows16.hip:launch_rowpass16 takes nb <= 16 only): from
seventeen batches on the batch kurtosis is k_batch_kurtosis -- a row staged in LDS, lane b + 64 q sums batch b -- and the
ridge pass takes the LDS branch of k_resid_lowrank.  Inputs and reference come from tests/test_batches_wide_host.py, which
proves on the CPU that the f64 oracle is within 1e-11 of the np.longdouble statement on every one of them: EVERY kurtosis
below is compared with that statement, never with another device route alone.

Bounds, the project's own for the same quantities: batch kurtosis of a given matrix 1e-9 relative with equal NaN patterns
(test_gpu_parity.py::test_dense_row_kernels_vs_numpy); for the ridge pass X after the division 1e-11, the kurtosis of the
residualised rows 1e-8, max |coefficient| 1e-10 (test_sixteen_rows_per_wave_passes_vs_numpy); medians exactly np.median of
the fetched vector; end to end the bars of test_association_wide_sample_axis_vs_oracle.  The observed maxima are written to
the file CNA_BATCHES_WIDE_PARITY_OUT names, when it is set (profiles/r13_batches_wide_parity.txt is such a run's output)."""
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import relerr
from test_batches_wide_host import (kurtosis_longdouble, kurt_case, ridge_case, fold16, nam_codes, wide_dataset, e2e_reference,
                                    qc_margin, assert_matches_oracle, KURT_CASES, RIDGE_CASES, RIDGE_FOLDED,
                                    RIDGE_PAST_BUDGET, NAM_CELLS, NAM_CASES, E2E_CASES, E2E_KW, QC_TIE, CONSTANT_ROWS)

pytestmark = pytest.mark.gpu

KURT_TOL = 1e-9         # batch kurtosis of a matrix as it is
RIDGE_X_TOL = 1e-11     # X after the ridge pass and the division by the std
RIDGE_KURT_TOL = 1e-8   # batch kurtosis of the residualised rows
RIDGE_COEF_TOL = 1e-10  # max |coefficient|
_seen = {}


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    yield get_engine()
    if os.environ.get('CNA_BATCHES_WIDE_PARITY_OUT') and _seen:
        with open(os.environ['CNA_BATCHES_WIDE_PARITY_OUT'], 'w') as f:
            f.write('max relative |gpu - reference| per case of tests/test_gpu_batches_wide.py; the kurtosis against np.longdouble\n')
            for k in sorted(_seen):
                f.write('%-74s %.3e  (bound %g)\n' % ((k,) + _seen[k]))
            for tol in sorted({b for _, b in _seen.values()}):
                f.write('%-74s %.3e  (bound %g)\n' % ('maximum', max(e for e, b in _seen.values() if b == tol), tol))


def _note(name, err, tol):
    _seen[name] = (max(err, _seen.get(name, (0.0, tol))[0]), tol)
    print('%s: %.3e (bound %g)' % (name, err, tol))


def _check_kurtosis(name, got, ref, tol):
    """Equal NaN patterns and max |got - ref| / |ref| <= tol over the rest."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=name)
    ok = ~np.isnan(ref)
    err = float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]))) if ok.any() else 0.0
    _note(name, err, tol)
    assert err <= tol, (name, err)


def _same_median(med, vec):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = np.median(vec)
    return med == want or (np.isnan(med) and np.isnan(want))


def _sized_for(eng, n):
    eng.ensure_graph(sp.identity(n, format='csr', dtype=np.float32))      # (the per-cell buffers are sized by the graph)


# ------------------------------------------------------------------------------------ (a) the batch kurtosis alone
def _kurtosis_of(eng, X, codes, nb):
    from cna_amd import _ffi
    _sized_for(eng, len(X))
    eng.upload_x(X)
    eng.batch_kurtosis(_ffi.MAT_X, codes, nb)
    return eng.x_stat().copy(), eng.stat_median()


@pytest.mark.parametrize('n,N,nb,variation', KURT_CASES)
def test_batch_kurtosis_of_a_matrix_vs_longdouble(eng, monkeypatch, n, N, nb, variation):
    """(301, 20, 17): the first count past the register path, most batches of one sample, a last workgroup with one live
    wave; 64 / 65, 128 / 129, 192 / 193 batches: the last lane of a batch slot and the first batch of the next; 256 batches:
    the limit, at 520 and at 1024 samples (32 KB of LDS per workgroup); 16 batches: the near side of the boundary, through
    rowpass16 (100 samples), k_batch_kurtosis_fast<8> (300) and <2> (100 under CNA_ROWPASS16=0).  Variations: samples in no
    batch, a batch left empty (every row NaN, the median too), constant rows (NaN on both sides)."""
    X, codes, ref = kurt_case(n, N, nb, variation)
    if variation == 'rowpass16=0':
        monkeypatch.setenv('CNA_ROWPASS16', '0')
    got, med = _kurtosis_of(eng, X, codes, nb)
    _check_kurtosis('a kurtosis %s' % ((n, N, nb, variation),), got, ref, KURT_TOL)
    assert _same_median(med, got), (med, np.median(got))
    if variation and 'constant' in variation:
        assert np.isnan(got[[r for r, _ in CONSTANT_ROWS]]).all()
    if variation and 'empty' in variation:
        assert np.isnan(got).all() and np.isnan(med)


def test_more_than_256_batches_are_refused_and_leave_the_engine_whole(eng):
    from cna_amd import _ffi
    X, codes, ref = kurt_case(301, 20, 17, None)
    before, med_before = _kurtosis_of(eng, X, codes, 17)
    rs = np.random.RandomState(257)
    wide = rs.rand(64, 300)
    eng.upload_x(wide)
    many = (np.arange(300) % 257).astype(np.int32)
    with pytest.raises(_ffi.CnaHipError, match='256 batches'):
        eng.batch_kurtosis(_ffi.MAT_X, many, 257)
    after, med_after = _kurtosis_of(eng, X, codes, 17)
    np.testing.assert_array_equal(before, after)
    assert med_before == med_after
    _check_kurtosis('a kurtosis (301, 20, 17) after a refusal', after, ref, KURT_TOL)


# ------------------------------------------------------------------------------------ (b) the batch kurtosis of the NAM
def _walk(eng, data, nsteps=3):
    """The NAM of `data` resident on the engine; returns its number of samples."""
    from cna_amd.tools._nam import sample_codes
    eng.null_local_discard()
    eng.ensure_graph(data.obsp['connectivities'])
    eng.colsums(1)
    codes, labels = sample_codes(data.obs['id'])
    Ns = len(labels)
    eng.set_samples(codes, Ns, np.bincount(codes, minlength=Ns).astype(float))
    eng.nam_steps(nsteps)
    return Ns


@pytest.mark.parametrize('N', sorted({N for N, _ in NAM_CASES}))
def test_batch_kurtosis_of_the_nam_and_its_qc_vs_longdouble(eng, N):
    """cna_batch_kurtosis(CNA_MAT_NAM) on the NAM of a walk (its own row stride, every cell) against the longdouble
    statement on the NAM fetched from the engine -- only the kernel is under test -- and cna_stat_qc's median, threshold
    and count of failing cells against the fetched kurtosis."""
    from cna_amd import _ffi, synth
    data, _ = synth.make_dataset(NAM_CELLS, N, k=15, seed=21)
    Ns = _walk(eng, data)
    assert Ns == N
    nam = eng.fetch_matrix(_ffi.MAT_NAM)                        # (device order, as cell_stat(.., nam_space=False))
    assert nam.shape == (NAM_CELLS, N)
    for nb in sorted(b for M, b in NAM_CASES if M == N):
        codes = nam_codes(N, nb)
        eng.batch_kurtosis(_ffi.MAT_NAM, codes, nb)
        got = eng.cell_stat(eng.n, nam_space=False).copy()
        _check_kurtosis('b NAM kurtosis %s' % ((NAM_CELLS, N, nb),), got, kurtosis_longdouble(nam, codes, nb), KURT_TOL)
        assert _same_median(eng.stat_median(), got)
        med, thr, dropped = eng.stat_qc()
        assert med == np.median(got) and thr == max(6, 2 * med)
        assert dropped == np.count_nonzero(~(got < thr))
        print('b NAM qc %s: median %.4f threshold %.4f dropped %d' % ((N, nb), med, thr, dropped))


# ------------------------------------------------------------------------------------ (c) the ridge pass with its kurtosis
def _ridge_pass(eng, c, codes, nb):
    from cna_amd import _ffi
    eng.upload_x(c.X)
    maxabs, med = eng.resid_lowrank_bk(c.Cm, c.W, c.y, codes, nb)
    return eng.fetch_matrix(_ffi.MAT_X), eng.x_stat().copy(), med, maxabs


def _check_ridge_pass(name, c, codes, nb, out):
    got, bk, med, maxabs = out
    err = relerr(got, c.Xs)
    _note('c X %s' % name, err, RIDGE_X_TOL)
    assert err < RIDGE_X_TOL
    _check_kurtosis('c kurtosis %s' % name, bk, kurtosis_longdouble(c.resid, codes, nb), RIDGE_KURT_TOL)
    assert _same_median(med, bk), (med, np.median(bk))
    err = abs(maxabs - c.maxabs) / c.maxabs
    _note('c max |coefficient| %s' % name, err, RIDGE_COEF_TOL)
    assert maxabs == pytest.approx(c.maxabs, rel=RIDGE_COEF_TOL)


@pytest.mark.parametrize('n,N,r,nb', RIDGE_CASES)
def test_ridge_pass_with_its_kurtosis_vs_numpy_and_longdouble(eng, n, N, r, nb):
    """k_resid_lowrank's LDS branch: (1000, 100, 3, 17) two rows per wave taking turns on one LDS row, NQ = 2; (777, 64, 21,
    20) r > 16, NQ = 1; (513, 130, 5, 65) the second batch slot, NQ = 3; (300, 260, 4, 129) the third, NQ = 8 and one row per
    wave; (200, 520, 2, 40) NQ = 16; (301, 300, 25, 24) 129 600 B of dynamic LDS; (301, 124, 64, 60) 130 944 B, the largest
    request that fits.  The first three once more with their batches folded into sixteen: the register branch of the same
    kernel (rowpass16 below 129 samples and rank 17) on the same rows, held to the same reference."""
    c = ridge_case(n, N, r, nb)
    _sized_for(eng, n)
    _check_ridge_pass('%s' % ((n, N, r, nb),), c, c.codes, nb, _ridge_pass(eng, c, c.codes, nb))
    if (n, N, r, nb) in RIDGE_FOLDED:
        folded = fold16(c.codes)
        _check_ridge_pass('%s folded to 16' % ((n, N, r, nb),), c, folded, 16, _ridge_pass(eng, c, folded, 16))


@pytest.mark.parametrize('n,N,r,nb', RIDGE_PAST_BUDGET)
def test_ridge_pass_past_the_lds_budget_is_refused_and_leaves_the_engine_whole(eng, n, N, r, nb):
    """133 120 B and 135 168 B of LDS: the library refuses both ("r x N too large for LDS", after it has voided X), which is
    why tools/_nam.py:_lowrank_ok keeps such a pass from being asked for -- with the predicate that left the row buffers
    out, the (3000, 128) and (2500, 500) calls of test_association_with_many_batches_vs_oracle raised this CnaHipError.
    Should the library come to take such a pass, it must be right; after a refusal the next upload computes what it
    computed before, bit for bit."""
    from cna_amd import _ffi
    small = ridge_case(*RIDGE_CASES[0])
    _sized_for(eng, max(n, RIDGE_CASES[0][0]))
    before = _ridge_pass(eng, small, small.codes, RIDGE_CASES[0][3])
    c = ridge_case(n, N, r, nb)
    try:
        out = _ridge_pass(eng, c, c.codes, nb)
    except Exception as e:                                  # noqa: BLE001
        assert isinstance(e, _ffi.CnaHipError) and 'too large for LDS' in str(e), repr(e)
    else:
        _check_ridge_pass('%s' % ((n, N, r, nb),), c, c.codes, nb, out)
    after = _ridge_pass(eng, small, small.codes, RIDGE_CASES[0][3])
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------ (d) end to end
REDO_CASE = (1500, 100, 50, 1, 1600)     # its schedule goes past the first ridge within the LDS budget: plan.reselect


@pytest.mark.parametrize('case', E2E_CASES + [REDO_CASE])
def test_association_with_many_batches_vs_oracle(eng, case):
    """(3000, 100) with 20 batches and a covariate: the LDS branch in a real call; (2000, 300) with 40: wide rows; (3000,
    128) with 60 batches and 4 covariates: r = 64, the factors alone fill the 128 KB, so the pass that carries the kurtosis is
    past the budget (the library refused it: CnaHipError) and a schedule of eight ridges is walked; (2500, 500) with 13
    batches and 3 covariates: the same budget with the register branch; (1500, 100) with 50: the optimistic first ridge taken
    back.  Every one drops cells in the QC; none has a cell within 1e-9 of the threshold (a flipped cell is an error)."""
    import cna_amd as cna
    assert qc_margin(*case) > QC_TIE
    data, meta = wide_dataset(*case)
    ref = e2e_reference(*case)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = cna.tl.association(data, meta['y'], 'id', covs=meta['covs'], batches=meta['batches'], return_full=True,
                                 engine=eng, **E2E_KW)
    assert_matches_oracle(res, data, ref)
    assert 0 < res.kept.sum() < len(res.kept)
    if case == REDO_CASE or case[2:4] == (60, 4):
        assert len(ref['ridge_log']) > 1
