"""The exact order statistics on the device against np.median, on vectors chosen bit by bit (run with -m gpu on an
MI355X; the inputs and what they are made for: tests/order_stats.py, checked in tests/test_order_stats_host.py).

  rows.hip    k_digit_hist2 + k_auto_pick (launch_auto_median): cna_stat_median, cna_stat_qc, the walk's stop rule
  walk.hip    stat_select over k_digit_hist: cna_stat_median under CNA_MEDIAN_HOST=1
  rows.hip    k_qc_count: the cells failing `kurtosis < max(6, 2 median)`
  strata.hip  k_st_hist + k_st_pick: the median column of cna_coef_strata, every bin at once

cna_load_cell_stat puts the vector where the kurtosis kernels leave theirs.  Every comparison is exact: a median is
np.median's, both NaN or equal as floats (a zero may carry either sign); counts are integers."""
import numpy as np
import pytest
import scipy.sparse as sp

import order_stats as osx

pytestmark = pytest.mark.gpu

U = np.uint64
EINVAL, ESTATE = -1, -4                                  # include/cna_hip.h


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.wait_reorder()
    e.drop_graph()
    e.drop_expression()


_RINGS = {}


def ring(n):
    """n cells, one edge per row: it only sizes the statistic's buffer."""
    if n not in _RINGS:
        i = np.arange(n)
        _RINGS[n] = sp.csr_matrix((np.ones(n, dtype=np.float32), (i, (i + 1) % n)), shape=(n, n))
    return _RINGS[n]


def assert_median(got, v, tag):
    want = osx.np_median(v)
    assert osx.same(got, want), '%s: %r, numpy %r' % (tag, got, want)


# ------------------------------------------------------------------ 1. the median of the NAM-space statistic
@pytest.mark.parametrize('n', osx.SIZES)
def test_median_of_every_case(eng, monkeypatch, n):
    """cna_stat_median on the device (default) and with the digit choice on the host (CNA_MEDIAN_HOST=1), every case of
    order_stats.cases at this count; what cna_fetch_cell_stat hands back is what was loaded, bit for bit."""
    cs = osx.cases(n)
    assert len(cs) >= 47
    eng.ensure_graph(ring(n))
    for name, v in cs:
        eng.load_cell_stat(v)
        back = eng.cells_to_device(eng.cell_stat(n))
        np.testing.assert_array_equal(back.view(U), v.view(U), err_msg=name)
        monkeypatch.delenv('CNA_MEDIAN_HOST', raising=False)
        assert_median(eng.stat_median(), v, '%s, %d cells, device' % (name, n))
        monkeypatch.setenv('CNA_MEDIAN_HOST', '1')
        assert_median(eng.stat_median(), v, '%s, %d cells, host-driven' % (name, n))
        monkeypatch.delenv('CNA_MEDIAN_HOST')
        assert_median(eng.stat_qc()[0], v, '%s, %d cells, cna_stat_qc' % (name, n))


def test_median_at_the_workgroup_cap(eng, monkeypatch):
    """N_CAP values: the first count at which launch_auto_median and launch_digit_hist take 1024 workgroups for what would
    be 1025, so that the first thread's stride reaches a fifth value.  N_CAP is odd and a split needs an even count:
    split_at(3) runs at N_CAP + 1 (a second upload; it asks for 1025 workgroups as well)."""
    monkeypatch.setenv('CNA_REORDER', '0')             # (a ring gains nothing from a device cell order: seconds of host work here)

    def both(v, tag):
        eng.load_cell_stat(v)
        monkeypatch.delenv('CNA_MEDIAN_HOST', raising=False)
        assert_median(eng.stat_median(), v, tag + ' at the cap, device')
        monkeypatch.setenv('CNA_MEDIAN_HOST', '1')
        assert_median(eng.stat_median(), v, tag + ' at the cap, host-driven')
        monkeypatch.delenv('CNA_MEDIAN_HOST')
        np.testing.assert_array_equal(eng.cells_to_device(eng.cell_stat(len(v))).view(U), v.view(U))

    n = osx.N_CAP
    eng.ensure_graph(ring(n))
    both(osx.random_bits(n, np.random.RandomState(100)), 'random_bits')
    v = osx.with_nan(n, np.random.RandomState(101), 'last')
    assert np.isnan(v[-1]) and np.isnan(v).sum() == 1   # the one NaN is the value only the fifth pass of a stride reads
    both(v, 'nan_last')
    v[-1] = 1e300                                       # ... and so is the largest value (the median moves if it is missed)
    both(v[::-1].copy(), 'largest value first')
    both(v, 'largest value last')
    eng.ensure_graph(ring(n + 1))
    v = osx.split_at(3, n + 1, np.random.RandomState(102))
    assert osx.first_split(*osx.middle_keys(v)) == 3
    both(v, 'split_at(3)')


def test_loader_refusals(eng):
    from cna_amd._ffi import CnaHipError, check
    from cna_amd.engine import Engine
    v = osx.kurtosis_like(257, np.random.RandomState(0))
    eng.ensure_graph(ring(257))
    eng.load_cell_stat(v)
    for bad in (v[:-1], np.concatenate([v, v[:1]])):
        with pytest.raises(CnaHipError, match=r'status %d\): .*n_global' % EINVAL):
            eng.load_cell_stat(bad)
    with pytest.raises(CnaHipError, match=r'status %d\): .*null pointer' % EINVAL):
        check(eng.lib.cna_load_cell_stat(eng.h, None, 257), 'cna_load_cell_stat')
    with pytest.raises(ValueError):
        eng.load_cell_stat(np.zeros((257, 1)))
    assert_median(eng.stat_median(), v, 'after the refusals')                      # the statistic is untouched
    e = Engine(device=0)
    try:
        with pytest.raises(CnaHipError, match=r'status %d\): .*cna_graph_upload' % ESTATE):
            e.load_cell_stat(v)
    finally:
        e.close()


# ------------------------------------------------------------------ 2. the QC decision
@pytest.mark.parametrize('n', osx.QC_SIZES)
def test_qc_median_threshold_and_count(eng, n):
    """cna_stat_qc: np.median, max(6, 2 median) with Python's max, and exactly the entries that are not < threshold --
    where the threshold equals entries of the vector, lies one double beside others, or the median is NaN."""
    eng.ensure_graph(ring(n))
    for name, v in osx.qc_cases(n):
        eng.load_cell_stat(v)
        med, thr, cnt = eng.stat_qc()
        w_med, w_thr, w_cnt = osx.qc_expected(v)
        tag = '%s, %d cells' % (name, n)
        assert osx.same(med, w_med), (tag, med, w_med)
        assert thr == w_thr, (tag, thr, w_thr)
        assert cnt == w_cnt, (tag, cnt, w_cnt)
        med2, thr2, cnt2 = eng.stat_qc()                                           # the count starts from zero every time
        assert (osx.same(med2, med), thr2, cnt2) == (True, thr, cnt), tag
    for name, v in osx.cases(n):                                                   # and on the medians' own cases
        eng.load_cell_stat(v)
        med, thr, cnt = eng.stat_qc()
        w_med, w_thr, w_cnt = osx.qc_expected(v)
        assert osx.same(med, w_med) and thr == w_thr and cnt == w_cnt, (name, n, (med, thr, cnt), (w_med, w_thr, w_cnt))


# ------------------------------------------------------------------ 3. the walk's medians
@pytest.mark.parametrize('n,N,seed', [(30000, 40, 3), (50001, 24, 5)])
def test_walk_medians_and_stop_rule_against_numpy(eng, monkeypatch, n, N, seed):
    """The datasets of test_walk_with_the_stop_rule_on_the_device (several workgroups add into one histogram), this time
    against numpy: cna_nam_auto's medians equal np.median of the kurtosis fetched after every step of a step-by-step
    walk, and its step count is the rule of _nam.py:64-68 applied in Python to those numpy medians."""
    from cna_amd import synth
    from cna_amd.tools._nam import sample_codes
    monkeypatch.setenv('CNA_AUTO_HOST', '0')
    monkeypatch.delenv('CNA_MEDIAN_HOST', raising=False)
    data, meta = synth.make_dataset(n, N, k=15, seed=seed)
    codes, labels = sample_codes(data.obs['id'])
    counts = np.bincount(codes, minlength=len(labels)).astype(float)
    eng.ensure_graph(data.obsp['connectivities'])
    eng.colsums(1)
    maxn = 15
    eng.set_samples(codes, len(labels), counts)
    taken, med = eng.nam_auto(maxn)
    eng.set_samples(codes, len(labels), counts)
    want, steps, prev = [], None, np.inf
    for i in range(maxn):
        eng.nam_step(True, True, True)
        v = eng.cell_stat(n)
        m = osx.np_median(v)
        assert_median(eng.stat_median(), v, 'step %d' % (i + 1))
        want.append(m)
        if prev - m < 3 and i + 1 >= 3:
            steps = i + 1
            break
        prev = m
    steps = maxn if steps is None else steps
    print('%d cells: %d steps, numpy medians %r' % (n, steps, want))
    assert taken == steps
    assert np.isnan(med[0]) and len(med) == taken       # (the rule never reads the first step's median: not computed)
    np.testing.assert_array_equal(med[1:], want[1:])
    assert not np.isnan(want).any() and 3 <= taken <= maxn


# ------------------------------------------------------------------ 4. the per-bin select of cna_coef_strata
def _strata(eng, segments, seed, tag):
    v, codes, n_bins = osx.strata_layout(segments, np.random.RandomState(seed))
    got = eng.coef_strata(v, None, codes, n_bins, 0.1, 2)
    want = osx.strata_expected(v, codes, n_bins)
    np.testing.assert_array_equal(want['n_kept'], [np.isfinite(s).sum() for s in segments])
    np.testing.assert_array_equal(got['n_kept'], want['n_kept'], err_msg=tag + ' n_kept')
    for k in ('min', 'max', 'median'):                  # assert_array_equal: NaN equals NaN, -0.0 equals 0.0
        bad = np.flatnonzero(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))))
        assert bad.size == 0, '%s %s: bins %r, got %r, numpy %r' % (tag, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
    return got, want


def _segments(seeds, limit=None):
    """[(name, vector)]: every finite case at every segment length, one bin each; after every seventh an empty bin or one
    that holds only values that are dropped."""
    out = []
    for seed in seeds:
        for m in osx.strata_lengths():
            for name, v in osx.finite_cases(m, seed):
                out.append(('%s x %d' % (name, m), v))
                if len(out) % 14 == 7:
                    out.append(('empty', np.zeros(0)))
                if len(out) % 14 == 0:
                    out.append(('nothing kept', np.array([np.nan, np.inf, -np.inf])))
    return out if limit is None else out[:limit]


def test_per_bin_median_several_hundred_bins(eng):
    segs = _segments([0])
    assert 300 <= len(segs) <= 1024
    names = [s[0] for s in segs]
    c = osx.st_chunk()
    assert {'empty', 'nothing kept', 'split_at(5) x %d' % c, 'digit(7, 255) x %d' % (2 * c + 1)} <= set(names)
    _strata(eng, [s[1] for s in segs], 11, '%d bins' % len(segs))


def test_per_bin_median_at_the_bin_limit(eng):
    segs = _segments([1, 2, 3, 4], limit=1024)
    assert len(segs) == 1024
    got, want = _strata(eng, [s[1] for s in segs], 12, '1024 bins')
    assert (want['n_kept'] == 0).sum() >= 100 and want['n_kept'].max() == 2 * osx.st_chunk() + 1


def test_per_bin_median_every_bin_over_three_chunks(eng):
    """All split_at(p) and digit(p, d) cases in bins of three chunks: their histograms are summed across workgroups.
    (The splits need an even count: one value more than the digits' 2 ST_CHUNK + 1.)"""
    m = 2 * osx.st_chunk() + 1
    segs = []
    for seed in (5, 6):
        segs += [v for name, v in osx.cases(m, seed) if name.startswith('digit')]
        segs += [v for name, v in osx.cases(m + 1, seed) if name.startswith('split_at')]
    assert len(segs) == 2 * (8 * len(osx.DIGITS) + 9)
    got, want = _strata(eng, segs, 13, 'three chunks')
    assert want['n_kept'].min() == m
