"""The inputs of tests/test_gpu_order_stats.py, checked without a GPU: every builder of tests/order_stats.py has the
property its name claims (asserted on the integer keys), the numpy restatement of the radix select equals np.median on
every case and count, and each of six deliberate mistakes in that select is caught by at least one case -- a list of
cases that a wrong select passes would not be worth running on the device."""
import numpy as np
import pytest

import order_stats as osx
from order_stats import U

SMALL = [n for n in osx.SIZES if n <= 4097]


@pytest.fixture(scope='module')
def all_cases():
    return {n: osx.cases(n) for n in osx.SIZES}


def test_key_and_inverse():
    v = np.array([-np.inf, -1.7e308, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.7e308, np.inf])
    k = osx.order_key(v)
    assert (np.diff(k.astype(object)) > 0).all()                      # strictly ascending, -0.0 below +0.0
    assert k[0] == osx.KEY_MIN - U(1) and k[-1] == osx.KEY_MAX + U(1)
    assert k[4] == osx.KEY_NEG_ZERO and k[5] == osx.KEY_POS_ZERO
    np.testing.assert_array_equal(osx.key_value(k).view(U), v.view(U))
    fmax = np.finfo(np.float64).max
    assert osx.order_key(np.array([-fmax, fmax])).tolist() == [osx.KEY_MIN, osx.KEY_MAX]
    rb = osx.random_bits(5000, np.random.RandomState(1))
    np.testing.assert_array_equal(osx.key_value(osx.order_key(rb)).view(U), rb.view(U))
    order = np.argsort(osx.order_key(rb), kind='stable')
    assert (np.diff(rb[order]) >= 0).all()                             # the key order is the order of the values


def test_sizes_and_lengths():
    assert osx.SIZES == [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 70001]
    cap = lambda n: min(max((n + 1023) // 1024, 1), 1024)             # launch_auto_median's grid
    assert (osx.N_CAP + 1023) // 1024 == 1025 and cap(osx.N_CAP) == 1024 and (osx.N_CAP - 1 + 1023) // 1024 == 1024
    assert cap(1024) == 1 and cap(1025) == 2
    c = osx.st_chunk()
    assert osx.strata_lengths() == [1, 2, 3, c - 1, c, c + 1, 2 * c + 1] and c >= 4    # ([1, 2, 3, 511, 512, 513, 1025] today)


def test_every_case_has_the_requested_length_and_a_name_of_its_own(all_cases):
    for n, cs in all_cases.items():
        names = [name for name, _ in cs]
        assert len(set(names)) == len(names)
        for name, v in cs:
            assert v.dtype == np.float64 and v.shape == (n,), (name, n)
        assert ('split_at(3)' in names) == (n % 2 == 0)
        for want in ('digit(0, 0)', 'digit(7, 255)', 'zeros', 'denormals', 'all_equal', 'two_values even', 'two_values 60/40',
                     'adjacent', 'random_bits', 'infinities half', 'infinities minority', 'huge', 'nan_first', 'nan_last',
                     'nan_middle', 'all_nan', 'kurtosis_like'):
            assert want in names
    again = osx.cases(256)
    for (a, v), (b, w) in zip(all_cases[256], again):
        assert a == b
        np.testing.assert_array_equal(v.view(U), w.view(U))           # the same bits on every call


def test_splits_part_the_middle_keys_at_the_named_pass(all_cases):
    seen = set()
    for n, cs in all_cases.items():
        for name, v in cs:
            if not name.startswith('split_at'):
                continue
            p = int(name[9])
            kl, ku = osx.middle_keys(v)
            assert np.isfinite(v).all() and kl < ku and osx.first_split(kl, ku) == p, (name, n)
            if name.endswith('sign'):
                assert kl < osx.KEY_NEG_ZERO + U(1) <= ku                # a negative below a positive value
            if name.endswith('exp'):
                assert (kl >> U(63)) == (ku >> U(63))
            seen.add(name)
    assert len(seen) == 9


def test_digits_of_the_middle_key(all_cases):
    fmax = np.finfo(np.float64).max
    for n, cs in all_cases.items():
        for name, v in cs:
            if not name.startswith('digit'):
                continue
            p, d = (int(x) for x in name[6:-1].split(', '))
            kl, ku = osx.middle_keys(v)
            assert np.isfinite(v).all(), (name, n)
            assert osx.key_byte(kl, p) == d and osx.key_byte(ku, p) == d, (name, n)
            assert osx.first_split(kl, ku) > p or kl == ku
            if n >= 255:                                              # the other elements reach the neighbouring bins too
                assert len(np.unique(osx.order_key(v))) > n // 2
            if p == 0 and d == 255:
                assert (osx.key_value(np.array([kl, ku])) >= 2.0 ** 1009).all()
            if p == 0 and d == 0:
                x = osx.key_value(np.array([kl, ku]))
                assert (x <= -2.0 ** 1009).all() and (x >= -fmax).all()


def test_the_other_builders(all_cases):
    for n, cs in all_cases.items():
        c = dict(cs)
        z = c['zeros']
        assert (z == 0).all()
        if n >= 2:
            assert np.signbit(z).any() and not np.signbit(z).all()
        dn = c['denormals']
        assert (np.abs(dn) <= 1e-310).all() and (np.abs(dn[dn != 0]) >= 5e-324).all()
        if n >= 255:
            assert (dn < 0).any() and (dn > 0).any() and (np.abs(dn) == 5e-324).any() and np.abs(dn).max() > 1e-312
        assert len(np.unique(c['all_equal'])) == 1 and np.isfinite(c['all_equal']).all()
        for name, share in (('two_values even', 0.5), ('two_values 60/40', 0.6)):
            vals, counts = np.unique(c[name], return_counts=True)
            if n >= 2:
                assert len(vals) == 2 and counts[0] == (n // 2 if share == 0.5 else min(int(np.ceil(0.6 * n)), n - 1)), (name, n)
        if n % 2 == 0:
            a, b = np.unique(c['two_values even'])
            assert osx.np_median(c['two_values even']) not in (a, b)  # the mean of two different values
        ad = np.unique(c['adjacent'])
        assert len(ad) == min(n, 2) and (n < 2 or ad[1] == np.nextafter(ad[0], np.inf))
        assert not np.isnan(c['random_bits']).any()
        if n >= 255:
            rb = osx.order_key(c['random_bits'])
            assert len(np.unique(osx.key_byte(rb, 0))) > 100 and (c['random_bits'] < 0).any()
        ih = c['infinities half']
        assert np.isinf(ih).all() and (ih < 0).sum() == n // 2
        if n % 2 == 0:
            assert np.isnan(osx.np_median(ih))
        im = c['infinities minority']
        if n >= 255:
            assert 0 < np.isinf(im).sum() < n // 2 and np.isfinite(osx.np_median(im))
        h = c['huge']
        assert (np.abs(h) >= 1.7e308).all() and np.isfinite(h).all()
        if n >= 255:
            assert (h < 0).any() and osx.np_median(h) >= 1.7e308
        if n % 2 == 0:
            assert osx.np_median(h) == np.inf                         # lo + hi overflows, in numpy as on the device
        for where, at in (('first', 0), ('last', n - 1), ('middle', n // 2)):
            w = c['nan_' + where]
            assert np.flatnonzero(np.isnan(w)).tolist() == [at]
        assert np.isnan(c['all_nan']).all()
        kl = c['kurtosis_like']
        assert (kl > -2).all() and (kl < 40).all()


def test_qc_cases():
    for n in osx.QC_SIZES + [256]:
        cs = osx.qc_cases(n)
        assert [name for name, _ in cs] == ['median below 3, entries 6.0', 'median exactly 3', 'median above 3, entries 2 median',
                                           'NaN median', 'nobody fails']
        for name, v in cs:
            assert v.shape == (n,)
            med, thr, cnt = osx.qc_expected(v)
            if name == 'median below 3, entries 6.0':
                assert med == 2.25 and thr == 6.0 and (v == 6.0).any()
            elif name == 'median exactly 3':
                assert med == 3.0 and thr == 6.0 and (v == 6.0).any()
            elif name.startswith('median above 3'):
                assert med == 3.7 and thr == 7.4 and (v == thr).any()
                assert (v == np.nextafter(thr, 0.0)).any() and (v == np.nextafter(thr, 8.0)).any()
            elif name == 'NaN median':
                assert np.isnan(med) and thr == 6.0 and (v == 6.0).any() and np.isnan(v).any()
                assert cnt == np.isnan(v).sum() + (v >= 6.0).sum()     # NaN fails the comparison
            else:
                assert cnt == 0 and thr == 6.0
            if name != 'nobody fails':
                assert thr in v                                       # strictness decides: `<` and `<=` give different counts
                assert cnt == np.count_nonzero(~(v < thr)) != np.count_nonzero(~(v <= thr))
                assert 0 < cnt < n
    assert osx.py_threshold(float('nan')) == 6 and osx.py_threshold(np.float64('nan')) == 6
    assert osx.py_threshold(-np.inf) == 6 and osx.py_threshold(np.inf) == np.inf


def test_restated_select_equals_numpy_on_every_case(all_cases):
    for n, cs in all_cases.items():
        for name, v in cs:
            got, want = osx.radix_median(v), osx.np_median(v)
            assert osx.same(got, want), (name, n, got, want)
    for n in osx.QC_SIZES:
        for name, v in osx.qc_cases(n):
            assert osx.same(osx.radix_median(v), osx.np_median(v)), (name, n)
    assert np.isnan(osx.radix_median(np.zeros(0)))


def test_every_fault_is_caught(all_cases):
    """For each deliberate mistake at least one case gives radix_median(v, fault) != np.median(v); the early last bin
    and the missing bit flip by a structured case, not by random bits alone."""
    caught = {f: set() for f in osx.FAULTS}
    for n in SMALL:
        for name, v in all_cases[n]:
            want = osx.np_median(v)
            for f in osx.FAULTS:
                if not osx.same(osx.radix_median(v, f), want):
                    caught[f].add(name)
    for f in osx.FAULTS:
        print(f, len(caught[f]), sorted(caught[f])[:6])
        assert caught[f], f
    assert caught['last_bin_early'] - {'random_bits'} and caught['no_sign_flip'] - {'random_bits'}
    # and by the cases made for them
    assert {'digit(%d, 255)' % p for p in range(8)} <= caught['last_bin_early']
    assert {'split_at(0) sign', 'digit(0, 0)', 'denormals'} <= caught['no_sign_flip']
    assert {'split_at(%d)' % p for p in range(1, 7)} <= caught['shared_prefix']
    assert {'nan_first', 'nan_last', 'nan_middle'} <= caught['nan_in_bin0']
    assert {'two_values even', 'split_at(5)', 'adjacent'} <= caught['same_rank']
    assert {'kurtosis_like', 'digit(4, 254)'} <= caught['rank_not_reduced']


def test_strata_layout_and_expectation():
    rs = np.random.RandomState(3)
    segs = [np.array([1.0, 3.0, 2.0]), np.zeros(0), np.array([np.nan, -4.0, np.inf, 5.0]), np.array([7.0])]
    v, codes, n_bins = osx.strata_layout(segs, rs)
    assert n_bins == 4 and (codes == -1).sum() >= 3 and len(v) == len(codes) == 8 + (codes == -1).sum()
    want = osx.strata_expected(v, codes, n_bins)
    assert want['n_kept'].tolist() == [3, 0, 2, 1]
    np.testing.assert_array_equal(want['median'], [2.0, np.nan, 0.5, 7.0])
    np.testing.assert_array_equal(want['min'], [1.0, np.nan, -4.0, 7.0])
    np.testing.assert_array_equal(want['max'], [3.0, np.nan, 5.0, 7.0])
