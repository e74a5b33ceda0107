"""cna_matrix_to_bins on inputs where it has ONE right answer (run with -m gpu on an MI355X): the kernel through
engine.upload_x and CNA_MAT_X, no graph needed.

Matrix entries are integers in [-1024, 1024], weights integers in [-256, 256] with zeros, at most 2^20 rows: every product
and every partial sum is an integer below 2^38, so the float64 sums are exact in any order (and with or without a fused
product) and are compared BIT FOR BIT with int64 numpy.  The shapes sit where the kernel branches (NB_CHUNK and NB_UNROLL
are read from the source): a bin's KEPT rows -- those with one contributing weight -- number 1, unroll - 1, unroll,
unroll + 1, chunk - 1, chunk, chunk + 1 and 2 chunk + 37, beside rows of the same bin that no weight column takes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = -1, -4


def _constant(name):
    src = open(os.path.join(ROOT, 'cna_amd', 'csrc', 'nam_bins.hip')).read()
    return int(re.search(r'constexpr (?:int64_t|int) %s = (\d+);' % name, src).group(1))


CHUNK, UNROLL = _constant('NB_CHUNK'), _constant('NB_UNROLL')
SIZES = [1, UNROLL - 1, UNROLL, UNROLL + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 37]
COLS = [1, 63, 64, 65, 200, 256, 257, 1024]
QS = [0, 1, 2, 15, 16]


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.drop_expression()


def build(N, q, n_bins, seed, layout='mixed'):
    """(M float64 rows x N, codes int32, W float64 q x rows or None)."""
    rs = np.random.RandomState(seed)
    codes, must = [], []
    if layout == 'mixed':                       # bins 0 .. 7: the special sizes; one bin empty; 10 % left out
        assert n_bins >= 10
        for b, size in enumerate(SIZES):
            codes += [b] * size
            must += [True] * size
            codes += [b] * 3                    # rows of the bin that no weight takes (they count when q = 0)
            must += [False] * 3
        rest = rs.randint(8, n_bins, 3 * (n_bins - 8))
        rest[rest == n_bins // 2] = 8           # a bin without rows
        codes += list(rest)
        must += [True] * len(rest)
        n_out = len(codes) // 9
        codes += [-1] * n_out
        must += [True] * n_out
    else:
        n = 2 * CHUNK + 37
        c = rs.randint(0, n_bins, n)
        if layout == 'few':
            if n_bins >= 2:
                c[c == 0] = n_bins - 1          # a bin without rows
            c[rs.rand(n) < 0.1] = -1
        elif layout == 'none':
            c[:] = -1
        elif layout == 'last':
            c[:] = n_bins - 1
        codes, must = list(c), [True] * n
    order = rs.permutation(len(codes))
    codes = np.asarray(codes, dtype=np.int32)[order]
    must = np.asarray(must)[order]
    n = len(codes)
    assert n <= 2 ** 20
    M = rs.randint(-1024, 1025, (n, N)).astype(np.float64)
    if q == 0:
        return M, codes, None
    W = rs.randint(-256, 257, (q, n))
    W[rs.rand(q, n) < 0.3] = 0
    W[0, must & (W[0] == 0)] = 7                # kept whatever the other columns say
    W[:, ~must] = 0
    return M, codes, W.astype(np.float64)


def exact(M, codes, W, n_bins):
    """int64 numpy: the sums and the contributing rows"""
    Mi = M.astype(np.int64)
    Wf = np.ones((1, len(codes))) if W is None else W
    sums = np.zeros((len(Wf), n_bins, M.shape[1]), dtype=np.int64)
    cnt = np.zeros((len(Wf), n_bins), dtype=np.int64)
    for j, w in enumerate(Wf):
        ok = np.flatnonzero((codes >= 0) & np.isfinite(w) & (w != 0))
        np.add.at(sums[j], codes[ok], w[ok].astype(np.int64)[:, None] * Mi[ok])
        np.add.at(cnt[j], codes[ok], 1)
    assert np.abs(sums).max(initial=0) < 2 ** 53
    return sums, cnt


def _upload(eng, M):
    eng.null_local_discard()
    eng.upload_x(M)


def _check(eng, M, codes, W, n_bins, what):
    from cna_amd._ffi import MAT_X
    _upload(eng, M)
    sums, cnt = eng.matrix_to_bins(MAT_X, codes, W, n_bins=n_bins)
    want, want_n = exact(M, codes, W, n_bins)
    assert sums.dtype == np.float64 and cnt.dtype == np.int64 and sums.shape == want.shape and cnt.shape == want_n.shape
    np.testing.assert_array_equal(cnt, want_n, err_msg=what + ': contributing rows')
    np.testing.assert_array_equal(sums, want.astype(np.float64), err_msg=what)
    return sums, cnt


@pytest.mark.parametrize('q', QS)
@pytest.mark.parametrize('N', COLS)
def test_every_width_and_every_chunk_boundary(eng, N, q):
    """50 bins: eight hold exactly the special numbers of kept rows, one is empty, a ninth of the codes is -1."""
    M, codes, W = build(N, q, 50, seed=1000 * N + q)
    sums, cnt = _check(eng, M, codes, W, 50, '%d columns, q = %d' % (N, q))
    assert (cnt[0, :8] == (np.asarray(SIZES) + (3 if q == 0 else 0))).all() and (cnt[:, 25] == 0).all()
    assert not sums[:, 25].any()


@pytest.mark.parametrize('n_bins,q,layout', [(1, 0, 'few'), (1, 16, 'few'), (2, 0, 'few'), (2, 15, 'few'), (1024, 0, 'mixed'),
                                             (1024, 1, 'mixed'), (1024, 4, 'mixed'), (50, 2, 'none'), (50, 0, 'none'),
                                             (50, 15, 'last'), (1024, 2, 'last'), (2, 0, 'last')])
def test_bins_from_one_to_the_cap(eng, n_bins, q, layout):
    """1, 2 and 1024 bins (4 x 1024 is the cap on the sums of one pass); every code -1: all zeros; every row in the last bin."""
    M, codes, W = build(65, q, n_bins, seed=n_bins + q, layout=layout)
    sums, cnt = _check(eng, M, codes, W, n_bins, '%d bins, q = %d, %s' % (n_bins, q, layout))
    if layout == 'none':
        assert not sums.any() and not cnt.any()
    if layout == 'last':
        assert not sums[:, :-1].any() and not cnt[:, :-1].any() and cnt[0, -1] == len(codes)


def test_weights_that_are_not_finite_leave_the_row_out_of_their_column_only(eng):
    M, codes, W = build(65, 2, 50, seed=5)
    rows = np.flatnonzero(codes >= 0)[:6]
    W[0, rows[0]], W[0, rows[1]], W[0, rows[2]] = np.nan, np.inf, -np.inf
    W[1, rows[:3]] = [3, -2, 5]
    W[1, rows[3]], W[0, rows[3]] = np.nan, 4
    sums, cnt = _check(eng, M, codes, W, 50, 'NaN and inf weights')
    assert np.isfinite(sums).all()
    clean = W.copy()
    clean[~np.isfinite(clean)] = 0
    np.testing.assert_array_equal(cnt, exact(M, codes, clean, 50)[1])


def test_nan_and_inf_in_the_matrix_reach_their_own_sum_only(eng):
    """NaN, +inf and -inf in rows that contribute to column 0 only, to both columns, to none (weight 0 everywhere) and in a
    row with code -1: the first two appear in exactly their (j, bin, column), the last two nowhere."""
    from cna_amd._ffi import MAT_X
    N, q, n_bins = 65, 2, 50
    M, codes, W = build(N, q, n_bins, seed=9)
    live = np.flatnonzero(codes >= 8)
    r_a, r_b, r_c, r_d = live[0], live[1], live[2], live[3]
    bins = codes[[r_a, r_b, r_c, r_d]]
    assert len(set(bins)) >= 1
    W[:, r_a] = [5, 0]                           # column 0 only
    W[:, r_b] = [-3, 2]                          # both (the negative weight turns +inf into -inf)
    W[:, r_c] = [1, 1]
    W[:, r_d] = [0, 0]                           # contributes to nothing
    out = np.flatnonzero(codes == -1)[0]
    special = [(r_a, 3, np.nan), (r_b, 10, np.inf), (r_c, 64, -np.inf), (r_d, 5, np.nan), (out, 7, np.inf)]
    plain = M.copy()
    for r, s, v in special:
        M[r, s] = v
        plain[r, s] = 0
    _upload(eng, M)
    sums, cnt = eng.matrix_to_bins(MAT_X, codes, W, n_bins=n_bins)
    want, want_n = exact(plain, codes, W, n_bins)
    want = want.astype(np.float64)
    touched = np.zeros(want.shape, dtype=bool)
    for r, s, v in special[:3]:
        for j in range(q):
            if W[j, r] != 0:
                want[j, codes[r], s] = np.nan if np.isnan(v) else v * np.sign(W[j, r])
                touched[j, codes[r], s] = True
    assert touched.sum() == 5
    np.testing.assert_array_equal(cnt, want_n)
    np.testing.assert_array_equal(sums, want)                      # (NaN == NaN here, inf by sign)
    assert (~np.isfinite(sums) == touched).all()


def _raw(eng, which, codes, W, q, n_rows, n_bins, n_cols):
    """The entry itself on buffers that hold a sentinel: (status, sums, n)."""
    from cna_amd._ffi import ptr
    sums = np.full((max(q, 1), max(n_bins, 1), n_cols), -77.0)
    cnt = np.full((max(q, 1), max(n_bins, 1)), -77, dtype=np.int64)
    rc = eng.lib.cna_matrix_to_bins(eng.h, which, ptr(codes), ptr(W), q, n_rows, n_bins, ptr(sums), ptr(cnt))
    return rc, sums, cnt


def test_refusals_write_nothing(eng):
    from cna_amd._ffi import MAT_X
    M, codes, W = build(65, 2, 50, seed=11)
    n = len(codes)
    _upload(eng, M)
    for bad in (50, -2):
        c = codes.copy()
        c[n // 2] = bad
        rc, sums, cnt = _raw(eng, MAT_X, c, W, 2, n, 50, 65)
        assert rc == EINVAL and (sums == -77.0).all() and (cnt == -77).all(), bad
    W17 = np.ones((17, n))
    for what, args in [('q = 17', (codes, W17, 17, n, 50)), ('1025 bins', (codes, None, 0, n, 1025)),
                       ('5 x 1024 sums', (codes, W17[:5], 5, n, 1024)), ('rows', (codes, W, 2, n - 1, 50)),
                       ('which', None)]:
        if args is None:
            rc, sums, cnt = _raw(eng, 2, codes, W, 2, n, 50, 65)
        else:
            rc, sums, cnt = _raw(eng, MAT_X, *args, 65)
        assert rc == EINVAL and (sums == -77.0).all() and (cnt == -77).all(), what
    with pytest.raises(ValueError):
        eng.matrix_to_bins(MAT_X, codes[:-1], W[:, :-1], n_bins=50)       # before the library is called
    with pytest.raises(ValueError):
        eng.matrix_to_bins(MAT_X, codes, W[:, :-1], n_bins=50)
    sums, _ = eng.matrix_to_bins(MAT_X, codes, W, n_bins=50)               # and the entry still works afterwards
    np.testing.assert_array_equal(sums, exact(M, codes, W, 50)[0].astype(np.float64))


def test_no_matrix_is_a_state_error():
    from cna_amd._ffi import MAT_NAM, MAT_X
    from cna_amd.engine import Engine
    e = Engine()
    try:
        codes = np.zeros(10, dtype=np.int32)
        for which in (MAT_X, MAT_NAM):
            rc, sums, cnt = _raw(e, which, codes, None, 0, 10, 1, 4)
            assert rc == ESTATE and (sums == -77.0).all() and (cnt == -77).all()
    finally:
        e.close()


def test_two_runs_give_the_same_bits(eng):
    """Real-valued entries and weights, where the order of a sum shows: the order is fixed."""
    from cna_amd._ffi import MAT_X
    rs = np.random.RandomState(3)
    n, N, q, n_bins = 4 * CHUNK + 5, 200, 3, 7
    M = rs.randn(n, N) * np.exp(rs.randn(n, 1) * 3)
    codes = rs.randint(-1, n_bins, n).astype(np.int32)
    W = rs.randn(q, n)
    W[rs.rand(q, n) < 0.2] = 0
    _upload(eng, M)
    a = eng.matrix_to_bins(MAT_X, codes, W, n_bins=n_bins)
    b = eng.matrix_to_bins(MAT_X, codes, W, n_bins=n_bins)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    want = np.stack([[(W[j, (codes == L) & (W[j] != 0), None] * M[(codes == L) & (W[j] != 0)]).sum(axis=0) for L in range(n_bins)]
                     for j in range(q)])
    scale = np.stack([[np.abs(W[j, codes == L, None] * M[codes == L]).sum(axis=0) for L in range(n_bins)] for j in range(q)])
    assert (np.abs(a[0] - want) <= (n + 2) * 2.0 ** -52 * scale).all()
