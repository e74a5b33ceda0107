"""The global F-test kernels (csrc/stats.hip) on inputs with ONE right answer (run with -m gpu on an MI355X).

tests/global_exact.py: integer columns with a power-of-two standard deviation, U a signed permutation or Hadamard blocks,
M the identity or block centring -- Zc, the projections, ssered, fit and ssefull are then exact on the device in any
order, F and r2 are three float64 operations each, and p is mpmath's.  kidx, r2 and every edge value are compared with
array_equal, p at the project's rtol of 1e-9 (test_gpu_parity.py::test_global_test_matches_scipy).  Everything goes
through Engine.upload_x / condition / global_test.

a. sample counts 3 ... 1023 of every residue mod 4 and mod 16 and 4 ... 1024, each with 1 ... 257 columns; k lists;
   both U, both M, r in {0, 3}, a column mean that is not zero;
b. the conventions of f_sf and k_gt_min: ssefull == 0, fit == 0, no degrees of freedom, constant / NaN / inf columns,
   ties -- at columns 0, 15, 16 and P - 1 between ordinary neighbours;
c. the F tail: d1 1 ... 100 x d2 1 ... 1020, both sides of incbet's branch point, p from 1 - 1e-6 to the bottom of the
   double range; the table and the worst relative error are printed;
d. state: a large P before a small one, two tests in a row, a launch on top of a pending one, a test without a
   condition."""
import mpmath
import numpy as np
import pytest

import global_exact as ge

pytestmark = pytest.mark.gpu

RTOL = 1e-9


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    return get_engine()


def _x(N):
    """Any 64 x N matrix: it only defines the sample axis."""
    return ((np.arange(64 * N).reshape(64, N) * 7) % 11 - 5.0)


def _start(eng, N):
    eng.null_local_discard()
    eng.global_test_discard()
    eng.upload_x(_x(N))


def _check(got, ref, what):
    kidx, p, r2 = got
    assert np.array_equal(kidx, ref[0]), what + ': kidx'
    assert np.array_equal(r2, ref[2], equal_nan=True), what + ': r2'
    exact = ~((ref[1] > 0) & (ref[1] < 1))                      # 0, 1 and NaN have no tolerance
    assert np.array_equal(p[exact], ref[1][exact], equal_nan=True), what + ': p at the edges'
    np.testing.assert_allclose(p[~exact], ref[1][~exact], rtol=RTOL, atol=0, err_msg=what + ': p')


def _run(eng, c, P=None):
    P = c['Y'].shape[1] if P is None else P
    eng.condition(c['M'], np.ascontiguousarray(c['Y'][:, :P]))
    return eng.global_test(c['U'], c['ks'], c['r'])


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize('N', ge.SWEEP_ODD + ge.SWEEP_EVEN)
def test_sample_axis_and_tile_remainders(eng, N):
    """Every N with P = 1 (one wave), 15 ... 17, 63 ... 65 (one workgroup of four 16-column tiles, one more) and 257:
    the N step the sample axis of both MFMA kernels through every remainder mod 4 and both sides of one and of several
    16-row tiles.  U, M and r rotate over the N (global_exact.sweep_setup)."""
    c = ge.sweep_case(N)
    _start(eng, N)
    for P in ge.SWEEP_P:
        _check(_run(eng, c, P), [v[:P] for v in c['ref']], 'N=%d P=%d %s block=%s r=%d ks=%s'
               % (N, P, c['ukind'], c['block'], c['r'], c['ks']))


@pytest.mark.parametrize('N,ks,r', [(65, [1], 0), (65, [15], 0), (65, [16], 3), (65, [17], 0), (65, [33], 3),
                                    (129, [33, 5, 17, 5, 1], 0), (64, [2, 1], 3), (19, [17], 0), (65, [63], 0),
                                    (65, [60, 1], 3), (1023, [1021], 0), (1024, [1022, 3], 0)])
def test_k_lists(eng, N, ks, r):
    """One k; kmax on both sides of one and two 16-row tiles of the projection; lists that are not increasing and
    repeat a k; kmax = N - 2 (one degree of freedom left) and N - 2 - r."""
    c = ge.case(N, 17, 'hadamard', False, r, ks)
    _start(eng, N)
    _check(_run(eng, c), c['ref'], 'N=%d ks=%s r=%d' % (N, ks, r))


@pytest.mark.parametrize('N', [19, 65, 256])
@pytest.mark.parametrize('ukind', ['perm', 'hadamard'])
@pytest.mark.parametrize('block', [False, True])
@pytest.mark.parametrize('r', [0, 3])
def test_both_u_and_both_m(eng, N, ukind, block, r):
    c = ge.case(N, 33, ukind, block, r, [3, 1, 12])
    _start(eng, N)
    _check(_run(eng, c), c['ref'], 'N=%d %s block=%s r=%d' % (N, ukind, block, r))


@pytest.mark.parametrize('N', [13, 64, 257])
def test_a_column_mean_that_is_not_zero(eng, N):
    """k_cond_scale subtracts the mean for the standard deviation only: Zc keeps it, and so do ssered and the fit."""
    c = ge.case(N, 20, 'hadamard', False, 0, [1, 4, 9], shift=True)
    assert len(set(c['Z'].sum(axis=0))) > 2
    _start(eng, N)
    _check(_run(eng, c), c['ref'], 'N=%d shifted' % N)


# ------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize('order', [0, 1])
def test_edge_conventions_between_ordinary_columns(eng, order):
    """A column inside the span of the first k PCs (ssefull == 0: p = 0, r2 = 1), one with no weight on them (fit == 0:
    p = 1, r2 = 0), a constant one, a zero one, one with a NaN, with +inf, with -inf (all -1, nan, nan), at columns 0,
    15, 16, P - 1 and beside them; both k tie at p = 0 / p = 1 and the FIRST of the list wins, whichever it is.  The
    ordinary columns between them are exact as ever: a NaN column disturbs no neighbour."""
    e = ge.edge_case()
    ks = [e['K1'], 2 * e['K1']][::-1 if order else 1]
    ref = ge.reference(e['Z'], e['U'], ks, 0)
    for col, name in e['spots'].items():
        want = {'inside': (0, 0.0, 1.0), 'outside': (0, 1.0, 0.0)}.get(name, (-1, ge.NAN, ge.NAN))
        assert ge.same((ref[0][col], ref[1][col], ref[2][col]), want)
    assert set(e['spots']) >= {0, 15, 16, e['Y'].shape[1] - 1}
    _start(eng, e['N'])
    eng.condition(e['M'], e['Y'])
    got = eng.global_test(e['U'], ks, 0)
    _check(got, ref, 'edges, ks=%s' % ks)
    assert np.isfinite(got[1]).sum() == e['Y'].shape[1] - 6


@pytest.mark.parametrize('ks,valid', [([9, 8], True), ([8, 9, 12], True), ([9, 10], False), ([12], False)])
def test_k_without_degrees_of_freedom(eng, ks, valid):
    """N = 13, r = 3: k = 8 leaves one degree of freedom, k >= 9 none (p is NaN there).  A valid k beside an invalid one
    wins wherever it stands; with every k invalid every column is (-1, nan, nan)."""
    c = ge.case(13, 17, 'perm', False, 3, ks)
    assert (c['ref'][0] == (ks.index(8) if valid else -1)).all() and np.isnan(c['ref'][1]).all() != valid
    _start(eng, 13)
    _check(_run(eng, c), c['ref'], 'ks=%s' % ks)


# ------------------------------------------------------------------------------------------------ c
def test_f_tail_against_mpmath(eng):
    """(d1, d2, F) from exact columns: d1 in 1, 2, 3, 16, 17, 100; d2 in 1, 2, 3, 10, 100, 500 and 922 ... 1020; x on
    both sides of incbet's branch point; p from 1 - 1e-6 down to 1e-800.  rtol 1e-9 wherever p_ref >= 1e-290 (that
    includes front = exp(...) well below 1e-280); below, 0 <= p <= 1e-289 and finite."""
    rows, bad = [], []
    for g in ge.tail_table():
        N, k = g['N'], g['k']
        _start(eng, N)
        eng.condition(np.eye(N), g['Z'])
        kidx, p, _ = eng.global_test(g['U'], [k], g['r'])
        for f, pr, pm, pd in zip(g['F'], g['p'], g['p_mp'], p):
            if pr >= 1e-290:
                err = abs(float((mpmath.mpf(float(pd)) - pm) / pm)) if np.isfinite(pd) else np.inf
                ok = err <= RTOL
            else:
                err = np.nan
                ok = bool(np.isfinite(pd) and 0.0 <= pd <= 1e-289)
            rows.append((k, g['d2'], float(f), mpmath.nstr(pm, 8), float(pd), err))
            if not ok:
                bad.append(rows[-1])
        assert (kidx == 0).all()
    print('\n  d1    d2            F             p_ref              p_device   rel.err')
    for k, d2, f, pm, pd, err in sorted(rows):
        print('%4d %5d %12.6g %17s %21.14e  %8.2e' % (k, d2, f, pm, pd, err))
    print('\n  d2   points   smallest p compared at rtol   worst rel.err')
    for d2 in sorted({r[1] for r in rows}):
        sel = [r for r in rows if r[1] == d2]
        errs = [r[5] for r in sel if r[5] == r[5]]
        print('%5d %7d %26.3e %14.2e' % (d2, len(sel), min(r[4] for r in sel if r[5] == r[5]), max(errs)))
    worst = max((r[5], r) for r in rows if r[5] == r[5])
    print('\nworst relative error of p on the device: %.3g at (d1, d2, F, p_ref) = %s' % (worst[0], worst[1][:4]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ d
def test_large_p_then_small_p_equals_a_fresh_engine(eng):
    """condition with P = 1000, then 5, then 70 on ONE engine (c->gt is carved as M | Y by the condition and as
    U | ks | results | scratch by the test; Zc keeps its allocation and is re-zeroed): each result equals a fresh
    engine's array for array, and the reference."""
    from cna_amd.engine import Engine
    N = 65
    _start(eng, N)
    for P in (1000, 5, 70):
        c = ge.case(N, P, 'hadamard', True, 3, [2, 7, 21])
        got = _run(eng, c)
        fresh = Engine()
        try:
            fresh.upload_x(_x(N))
            want = _run(fresh, c)
        finally:
            fresh.close()
        assert ge.same(got, want), P
        _check(got, c['ref'], 'P=%d after a larger one' % P)


def test_twice_in_a_row_and_a_launch_on_top_of_a_pending_one(eng):
    from cna_amd._ffi import CnaHipError
    N = 63
    c = ge.case(N, 40, 'perm', False, 0, [1, 5, 17])
    _start(eng, N)
    eng.condition(c['M'], c['Y'])
    one = eng.global_test(c['U'], c['ks'], 0)
    two = eng.global_test(c['U'], c['ks'], 0)
    assert ge.same(one, two)
    _check(one, c['ref'], 'first of two')
    other = ge.reference(c['Z'], c['U'], [3], 3)
    eng.global_test_launch(c['U'], c['ks'], 0)
    with pytest.raises(CnaHipError, match='still pending'):
        eng.global_test_launch(c['U'], [3], 3)
    _check(eng.global_test_fetch(), c['ref'], 'the fetch after a refused launch')
    with pytest.raises(CnaHipError, match='no global test pending'):
        eng.global_test_fetch()
    _check(eng.global_test(c['U'], [3], 3), other, 'the test after the refusals')


def test_without_a_condition_it_is_refused(eng):
    from cna_amd._ffi import CnaHipError
    from cna_amd.engine import Engine
    N = 19
    c = ge.case(N, 17, 'hadamard', False, 0, [2, 5])
    e = Engine()
    try:
        e.upload_x(_x(N))
        with pytest.raises(CnaHipError, match='needs cna_condition_phenotypes'):
            e.global_test(c['U'], c['ks'], 0)
        with pytest.raises(CnaHipError, match='needs cna_condition_phenotypes'):
            e.global_test_launch(c['U'], c['ks'], 0)
        _check(_run(e, c), c['ref'], 'the first condition after a refusal')
        e.upload_x(_x(N + 1))                             # another sample axis: the resident Zc is of the old one
        with pytest.raises(CnaHipError, match='needs cna_condition_phenotypes'):
            e.global_test(c['U'], c['ks'], 0)
        e.upload_x(_x(N))
        _check(_run(e, c), c['ref'], 'conditioned again')
    finally:
        e.close()
