"""The helpers of tests/global_exact.py, pinned on the CPU before tests/test_gpu_global_exact.py trusts them.

- the builder serves every N the device tests name (none had to be replaced) and every N from 3 to 200, proves each
  column in Fractions, and raises where it cannot: N = 2, N = 4 in pairs, a column whose variance is no power of four;
- on the exact inputs the host restatement cna_amd.tools._stats.minp_stats gives the reference's kidx and r2 bit for
  bit and a p (scipy's fdtrc) within 1e-9 of mpmath's;
- betacf / incbet / f_sf of stats.hip restated in Python doubles, over the F-tail grid, against mpmath: the worst
  relative error and the largest iteration count are printed (the yardstick for the device's figure) and the count
  stays below the kernel's cap of 500;
- the F-tail grid covers what it is for: every d1 and d2, both sides of incbet's branch point within a factor 1.5,
  p from 1 - 1e-5 up down to below 1e-280;
- model(), the five kernels in numpy, agrees with the reference, and each one-line slip it knows makes a device case
  fail -- except dropping f_sf's `f == inf` line, which changes nothing: x = d2 / (d2 + d1 inf) is 0 and incbet(., ., 0)
  is 0 already."""
import math

import mpmath
import numpy as np
import pytest

import global_exact as ge


def test_the_builder_serves_every_sample_count_of_the_device_tests():
    """Every N of sections (a) has an exact column of each family claimed for it, as Y = scale (z + offsets) for both
    M; no N had to be replaced by a neighbour."""
    for N in ge.SWEEP_ODD + ge.SWEEP_EVEN:
        fam = ge.kinds(N)
        assert fam, N
        for kind in fam:
            z = ge.exact_vector(N, kind)
            assert len(z) == N and z.sum() == 0 and ge.check_exact(z) >= 0
        c = ge.columns(N, 30)
        assert np.array_equal(c['M'].dot(c['Y']), c['Z'] * c['scale'])
        assert len({tuple(c['Z'][:, p]) for p in range(min(N, ge.PERIOD))}) > min(N, ge.PERIOD) // 2
        if ge.sweep_setup(N)[1]:
            c = ge.columns(N, 30, block=True)
            assert np.array_equal(c['M'].dot(c['Y']), c['Z'] * c['scale'])
            assert not np.array_equal(c['Y'], c['Z'] * c['scale'])       # the offsets are there for M to remove
            assert np.abs(c['M']).min() > 0 or N > 4
    assert {ge.sweep_setup(N)[0] for N in ge.SWEEP_ODD} == {'hadamard', 'perm'}
    assert {ge.sweep_setup(N)[1:3] for N in ge.SWEEP_ODD + ge.SWEEP_EVEN} == {(False, 0), (True, 0), (False, 3), (True, 3)}


def test_the_builder_serves_every_n_from_3_to_200_and_raises_where_it_cannot():
    for N in range(3, 201):
        assert ge.check_exact(ge.exact_vector(N)) >= 0
    with pytest.raises(ValueError):
        ge.exact_vector(2)
    with pytest.raises(ValueError):
        ge.columns(2, 3)
    with pytest.raises(ValueError):
        ge.columns(4, 3, block=True)                    # (3, -1, -1, -1) is the only family of N = 4: not in pairs
    with pytest.raises(ValueError):
        ge.exact_vector(6, 'ones')
    with pytest.raises(ValueError):
        ge.exact_vector(8, 'pow4')
    with pytest.raises(ValueError):
        ge.check_exact(np.array([1, -1, 1, -1]))        # variance 4/3
    with pytest.raises(ValueError):
        ge.check_exact(np.array([1, 1, -1]))            # mean 1/3
    with pytest.raises(ValueError):
        ge.check_exact(np.array([1.5, -1.5, 0]))
    assert ge.check_exact(np.array([3, -3, 1, -1, 0, 0])) == 1
    assert ge.check_exact(np.array([8, -8, 1, -1, 1, -1, 1, -1] + [0] * 127)) == 0      # N = 135, F = 1440 at k = 2


def test_the_exact_u_are_orthonormal_and_on_the_grid():
    for N in (3, 6, 16, 19, 65, 257, 1023, 1024):
        H, Pm = ge.hadamard_u(N), ge.perm_u(N, first=(2, 0))
        for U in (H, Pm):
            assert np.array_equal(U.T.dot(U), np.eye(N))
        assert Pm[2, 0] == 1 and abs(Pm[0, 1]) == 1 and (np.abs(Pm).sum(axis=0) == 1).all()
        if N in (16, 1024):
            assert (np.abs(H) == 1 / math.sqrt(N)).all()
        if N >= 16:
            assert (np.count_nonzero(H[:, :4], axis=0) >= 4).any()


def test_the_example_of_the_issue():
    """J = 3, one pair of +-8, three pairs of +-1, N = 135: F = 1440 at k = 2, p = 2.2565845e-90."""
    z = np.array([8, -8, 1, -1, 1, -1, 1, -1] + [0] * 127, dtype=float)[:, None]
    F, p, r2 = ge.ftest_terms(z, ge.perm_u(135, first=(0, 1)), [2], 0)
    assert F[0, 0] == 1440.0 and r2[0, 0] == 1.0 - 6.0 / 134.0
    assert abs(p[0, 0] / 2.2565845e-90 - 1) < 1e-7
    import scipy.special as sc
    assert abs(sc.fdtrc(2, 132, 1440.0) / p[0, 0] - 1) < 1e-9


def test_the_edge_conventions_of_the_reference():
    assert math.isnan(ge.f_sf_mp(1.0, 2, 0)[0]) and math.isnan(ge.f_sf_mp(1.0, 2, -3)[0])
    assert math.isnan(ge.f_sf_mp(ge.NAN, 2, 5)[0])
    assert ge.f_sf_mp(0.0, 2, 5)[0] == 1.0 and ge.f_sf_mp(-1.0, 2, 5)[0] == 1.0
    assert ge.f_sf_mp(math.inf, 2, 5)[0] == 0.0
    e = ge.edge_case()
    K1 = e['K1']
    kidx, p, r2 = ge.reference(e['Z'], e['U'], [K1, 2 * K1], 0)
    for c, name in e['spots'].items():
        want = {'inside': (0, 0.0, 1.0), 'outside': (0, 1.0, 0.0)}.get(name, (-1, ge.NAN, ge.NAN))
        assert ge.same((kidx[c], p[c], r2[c]), want), (c, name)
    plain = [c for c in range(e['Z'].shape[1]) if c not in e['spots']]
    assert (kidx[plain] >= 0).all() and ((p[plain] > 0) & (p[plain] < 1)).all()


@pytest.mark.parametrize('N', [3, 5, 6, 13, 16, 19, 65, 129, 256, 1023])
def test_minp_stats_matches_the_reference_on_exact_inputs(N):
    """kidx and r2 bit for bit, p (scipy's fdtrc) within 1e-9 of mpmath's."""
    from cna_amd.tools._stats import minp_stats
    c = ge.sweep_case(N)
    kidx, p, r2 = minp_stats(c['Y'], c['M'], c['U'], np.asarray(c['ks']), c['r'])
    kr, pr, r2r = c['ref']
    assert np.array_equal(kidx, kr) and np.array_equal(r2, r2r)
    np.testing.assert_allclose(p, pr, rtol=1e-9, atol=0)
    assert len(set(r2r)) >= (min(N, ge.PERIOD) // 3 if N >= 13 else 2)          # the columns are not copies of one another


def _tail_points():
    for g in ge.tail_table():
        for f, p, pm in zip(g['F'], g['p'], g['p_mp']):
            yield g['k'], g['d2'], float(f), float(p), pm


def test_the_tail_grid_covers_what_it_is_for():
    pts = list(_tail_points())
    assert {d1 for d1, *_ in pts} == set(ge.TAIL_D1) and {min(d2, 1020) for _, d2, *_ in pts} >= set(ge.TAIL_D2)
    ratio = np.array([(d2 / (d2 + d1 * f)) / ge.branch_x(d1, d2) for d1, d2, f, _, _ in pts])
    assert ((ratio < 1) & (ratio * ge.BRANCH_FACTOR >= 1)).sum() >= 10
    assert ((ratio >= 1) & (ratio <= ge.BRANCH_FACTOR)).sum() >= 10
    logp = np.array([float(mpmath.log10(pm)) for *_, pm in pts])
    assert max(p for *_, p, _ in pts) >= 1 - 1e-5 and logp.min() < -300
    assert ((logp < -280) & (logp >= -290)).any() and ((logp < -290) & (logp > -308)).any()
    assert ((logp < -100) & (logp > -280)).sum() >= 10
    assert len(pts) <= 600


def test_the_formula_in_python_doubles_against_mpmath(capsys):
    """What the continued fraction of stats.hip can do in float64 with the host's lgamma / exp: printed, and the
    iteration count stays below the cap of 500.  The relative error is asserted at the device test's own 1e-9 wherever
    the reference is at least 1e-290."""
    worst, worst_at, most = 0.0, None, 0
    for d1, d2, f, p, pm in _tail_points():
        v, it = ge.f_sf_double(f, float(d1), float(d2))
        most = max(most, it)
        if p >= 1e-290:
            err = abs(float((mpmath.mpf(v) - pm) / pm))
            if err > worst:
                worst, worst_at = err, (d1, d2, f, p)
        else:
            assert 0.0 <= v <= 1e-289
    with capsys.disabled():
        print('\nf_sf in Python doubles over the F-tail grid: worst relative error %.3g at (d1, d2, F, p) = %s; '
              'most iterations %d' % (worst, worst_at, most))
    assert most < 500
    assert worst <= 1e-9


SMALL = [(13, 17, 'perm', False, 0, [1, 3]), (19, 17, 'hadamard', True, 3, [2, 5, 1]), (16, 5, 'hadamard', False, 0, [14]),
         (6, 3, 'perm', False, 0, [1, 4])]


def _agree(got, ref):
    return (np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2], equal_nan=True)
            and np.allclose(got[1], ref[1], rtol=1e-9, atol=0, equal_nan=True))


def test_the_model_of_the_kernels_and_the_slips_it_knows():
    """model() with no slip passes the device tests' assertions on small cases of (a), the edges of (b) and a slice of
    the tail (c); every slip fails at least one of them -- bar `no_inf`, which is no change of behaviour."""
    cases = []
    for N, P, uk, block, r, ks in SMALL:
        c = ge.case(N, P, uk, block, r, ks)
        cases.append((c['M'], c['Y'], c['U'], ks, r, c['ref']))
    e = ge.edge_case()
    for ks in ([e['K1'], 2 * e['K1']], [2 * e['K1'], e['K1']]):
        cases.append((e['M'], e['Y'], e['U'], ks, 0, ge.reference(e['Z'], e['U'], ks, 0)))
    for g in ge.tail_table()[::7]:
        keep = g['p'] >= 1e-290
        if keep.any():
            Z = g['Z'][:, keep]
            cases.append((np.eye(g['N']), Z, g['U'], [g['k']], g['r'], ge.reference(Z, g['U'], [g['k']], g['r'])))
    for M, Y, U, ks, r, ref in cases:
        assert _agree(ge.model(M, Y, U, ks, r), ref)
    for mutant in ge.MUTANTS:
        caught = sum(not _agree(ge.model(M, Y, U, ks, r, mutant), ref) for M, Y, U, ks, r, ref in cases)
        assert (caught == 0) if mutant == 'no_inf' else (caught > 0), (mutant, caught)
