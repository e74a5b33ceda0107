"""The exact-grid inputs and their brute-force counts (tests/exact_grid.py), checked on the CPU for every shape that
tests/test_gpu_local_exact.py runs on the device -- so that a failure there is never the test's own arithmetic.

What makes the reference exact: the products are integers times 2^-8 (compared here with the int64 product and with the
sum taken in the opposite order), and the test on z^2 = (a / N)^2 against (d / N)^2 is the test a >= d on those integers.
What makes it sharp: at least 50 outputs of every case sit ON a cut; one ulp up moves exactly those, one ulp down none."""
import numpy as np
import pytest

import exact_grid as eg
from fake_engine import FakeEngine

CASES = ([('null', s) for s in eg.NULL_SHAPES] + [('T', T) for T in eg.T_EDGES] + [('P', P) for P in eg.P_EDGES])


def _case(kind, arg):
    if kind == 'null':
        return eg.null_case(*arg)
    return eg.edge_case(eg.EDGE_P_FOR_T, arg) if kind == 'T' else eg.edge_case(arg, 300)


def _int_counts(a, d):
    """#{i : a[i, p] >= d[t]} counted on the integers a / 2^-8 and d / 2^-8."""
    gg = eg.G * eg.G
    ai, di = np.rint(a / gg).astype(np.int64), np.rint(d / gg).astype(np.int64)
    assert np.array_equal(ai * gg, a) and np.array_equal(di * gg, d)
    ai = np.sort(ai, axis=0)
    return np.array([ai.shape[0] - np.searchsorted(ai[:, p], di, side='left') for p in range(ai.shape[1])])


@pytest.mark.parametrize('kind,arg', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_products_are_exact_and_the_cuts_are_tied(kind, arg):
    from oracle import cna_oracle as orc
    c = _case(kind, arg)
    X, Yc, D, d, edges, N = c['X'], c['Yc'], c['D'], c['d'], c['edges'], c['N']
    g = eg.G
    Xi, Yi = np.rint(X / g).astype(np.int64), np.rint(Yc / g).astype(np.int64)
    assert np.array_equal(Xi * g, X) and np.array_equal(Yi * g, Yc) and np.abs(X).max() <= 4 and np.abs(Yc).max() <= 4
    np.testing.assert_array_equal(D, Xi.dot(Yi) * (g * g))
    np.testing.assert_array_equal(D, X[:, ::-1].dot(Yc[::-1]))
    assert np.abs(D).max() < 2.0 ** 15 and (np.diff(d) > 0).all() and d[0] > 0
    # (z2 >= e) == (a >= d) for every output and every t: both sides depend on the output through a alone
    a = np.abs(D)
    u = np.unique(a)
    z2 = (u / N) ** 2
    np.testing.assert_array_equal(z2[:, None] >= edges[None, :], u[:, None] >= d[None, :])
    ties = eg.tie_count(a, d)
    assert ties == c['ties'] and ties >= 50, ties
    want = eg.brute_tails(X, Yc, N, edges)
    np.testing.assert_array_equal(want, _int_counts(a, d))
    up = eg.brute_tails(X, Yc, N, np.nextafter(edges, np.inf))
    assert int(want.sum()) - int(up.sum()) == ties
    np.testing.assert_array_equal(eg.brute_tails(X, Yc, N, np.nextafter(edges, -np.inf)), want)
    # the reference's own edges, the oracle's count
    thr = d / N
    np.testing.assert_array_equal(eg.brute_tails(X, Yc, N, eg.reference_edges(thr)), orc.tail_counts(thr, D / N))
    # the irregular set of the GPU test: every edge is an attained value
    pick, irr = eg.irregular_edges(np.random.RandomState(5), D, N, 120)
    assert (np.diff(pick) > 0).all() and np.isin(pick, a).all()
    got = eg.brute_tails(X, Yc, N, irr)
    np.testing.assert_array_equal(got, _int_counts(a, pick))


def test_grid_matrix_options():
    rs = np.random.RandomState(3)
    M = eg.grid_matrix(rs, 200, 30, zero_rows=4, dup_rows=5, single_row=True)
    assert int((np.abs(M).sum(axis=1) == 0).sum()) == 4
    assert int((np.count_nonzero(M, axis=1) == 1).sum()) == 1
    assert 200 - len(np.unique(M, axis=0)) == 3 + 5           # four zero rows count once, five repeats
    plain = eg.grid_matrix(np.random.RandomState(3), 200, 30)
    assert int((plain != M).any(axis=1).sum()) <= 10
    with pytest.raises(ValueError):
        eg.grid_matrix(rs, 6, 3, zero_rows=4)


def test_observed_counts_reference():
    o = eg.obs_case()
    X, y, nc, N = o['X'], o['y'], o['nc'], o['N']
    g = eg.G
    Di = np.rint(X / g).astype(np.int64).dot(np.rint(y / g).astype(np.int64))
    np.testing.assert_array_equal(nc, Di * (g * g) / N)
    np.testing.assert_array_equal(nc, X[:, ::-1].dot(y[::-1]) / N)
    fe = FakeEngine()
    fe.nc = nc
    for name, thr in o['sets'].items():
        assert (np.diff(thr) >= 0).all(), name
        ties = eg.obs_ties(nc, thr)
        if len(thr) > 3:
            assert ties >= 50, (name, ties)
        for edges in (thr ** 2, eg.reference_edges(thr)):
            ranks, numdet = eg.brute_obs(nc, edges, thr)
            r2, n2 = fe.obs_counts(edges, thr)
            np.testing.assert_array_equal(ranks, r2)
            np.testing.assert_array_equal(numdet, n2)
        # inclusive against strict: on edges = thr^2 the two counts differ by at least the cells ON the threshold
        ranks, numdet = eg.brute_obs(nc, thr ** 2, thr)
        on = np.array([(np.abs(nc) == t).sum() for t in thr])
        assert (ranks - numdet >= on).all() and int(on.sum()) >= ties
    assert o['sets']['duplicate_first'][0] == o['sets']['duplicate_first'][1]
    assert eg.brute_obs(nc, o['sets']['above_max'] ** 2, o['sets']['above_max'])[0][-2:].tolist() == [0, 0]
