"""The counting sort by code that cna_expr_to_bins and cna_coef_strata share (csrc/expr.h: k_sort_count, k_sort_fill), on the
device (run with -m gpu on an MI355X).

1. More than one batch per block.  A block of the sort holds round_up(ceil(n / 1024), 64) cells and its wave takes them 64
   at a time, carrying the bins' cursors from one batch to the next behind two barriers.  Up to 65 536 cells every block is
   one batch, so the inputs of the two entries' own test files (19 997 cells at most) never run the carry.  N_CARRY cells
   give blocks of 192: three batches, the last block ragged.
   Integer-valued expression: sums and counts equal the numpy restatement bit for bit -- a lost, doubled or misplaced cell
   shows.  Real-valued float32 expression, dense form: the sums equal, bit for bit, the restatement of what k_pb_dense and
   k_pb_finish_dense add: per bin the cells in ascending index in chunks of PB_DENSE_CHUNK, each chunk added one cell
   after another in float64, the chunk totals added one after another -- a reordered cell shows.
   cna_coef_strata: counts, min, max and median exact; mean, ssd and densities within the bounds of
   tests/test_gpu_coef_strata.py where its density tolerance holds (groups of at most 4 133 kept cells: the 50-bin case).
2. The two callers keep their own buffers: a call of the one between two calls of the other, in either order and also when
   it is refused, changes no bit of what each returns alone."""
import numpy as np
import pytest

from test_expr_to_sample_host import restated_bins
from test_coef_strata_host import restated_strata
from test_gpu_expr_to_sample import DENSE_CHUNK, as_form, codes_for, counts_matrix
from test_gpu_coef_strata import _compare, _run, columns_for

pytestmark = pytest.mark.gpu

N_CARRY = 2 * 65536 + 37
ROWS_PER_BLOCK = -(-(-(-N_CARRY // 1024)) // 64) * 64
assert ROWS_PER_BLOCK == 192 and N_CARRY % ROWS_PER_BLOCK not in (0, 64, 128)   # three batches, the last block ragged
EXACT = ('n', 'n_kept', 'n_pos', 'n_neg', 'min', 'max', 'median')


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    e.unpin_expression()
    yield e
    e.drop_expression()


def carry_codes(n_bins):
    if n_bins == 2:
        return (np.arange(N_CARRY) % 2).astype(np.int32)      # two bins alternating: 32 lanes of every batch per bin
    if n_bins == 1:
        return np.zeros(N_CARRY, dtype=np.int32)              # every cell
    codes = codes_for(N_CARRY, n_bins, seed=n_bins)           # mixed, cells left out, a bin without cells
    assert (codes == -1).any() and (np.bincount(codes[codes >= 0], minlength=n_bins) == 0).any()
    return codes


# ------------------------------------------------------------------ 1. the carry from batch to batch
@pytest.mark.parametrize('form', ['dense-f32', 'csr-i32'])
def test_bins_exact_with_three_batches_per_block(eng, form):
    M = counts_matrix(N_CARRY, 3, seed=31)
    X = as_form(M, form)
    eng.ensure_expression(X)
    D = M.toarray()
    for n_bins in (2, 50, 1):
        codes = carry_codes(n_bins)
        for what in (0, 1):
            got, cnt = eng.expr_to_bins(codes, n_bins, what)
            want, wcnt = restated_bins(D, codes, n_bins, what)
            np.testing.assert_array_equal(cnt, wcnt, err_msg='%s %d bins' % (form, n_bins))
            np.testing.assert_array_equal(got, want, err_msg='%s %d bins what=%d' % (form, n_bins, what))


def restated_dense_order(D, codes, n_bins):
    """What k_pb_dense + k_pb_finish_dense add, in their order."""
    out = np.zeros((n_bins, D.shape[1]))
    for b in range(n_bins):
        cells = np.flatnonzero(codes == b)                     # ascending
        total = np.zeros(D.shape[1])
        for lo in range(0, len(cells), DENSE_CHUNK):
            total = total + np.cumsum(D[cells[lo:lo + DENSE_CHUNK]].astype(np.float64), axis=0)[-1]
        out[b] = total
    return out


@pytest.mark.parametrize('n_bins', [2, 50])
def test_bins_order_inside_a_bin_across_the_carry(eng, n_bins):
    rs = np.random.RandomState(n_bins)
    # float32 values over 60 binary orders of magnitude: their float64 sums round, so the order of the additions shows (values
    # of one magnitude would not do: 24-bit terms add exactly in float64)
    D = np.ascontiguousarray((rs.randn(N_CARRY, 3) * 2.0 ** rs.randint(-30, 31, (N_CARRY, 3))).astype(np.float32))
    codes = carry_codes(n_bins)
    eng.ensure_expression(D)
    got, cnt = eng.expr_to_bins(codes, n_bins, 0)
    want = restated_dense_order(D, codes, n_bins)
    assert cnt[cnt > 0].min() > DENSE_CHUNK                    # every bin that has cells has more than one chunk
    # the order is told apart: numpy's own (pairwise) sum of the same cells differs from the ordered one in every column
    assert (restated_bins(D, codes, n_bins, 0)[0] != want)[cnt > 0].any(axis=0).all()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('n_bins', [2, 50])
def test_strata_with_three_batches_per_block(eng, n_bins):
    v, fdr, codes = columns_for(N_CARRY, n_bins, seed=40 + n_bins, outlier=True)
    assert np.isinf(v).sum() == 2 and np.isnan(v).any() and (codes == -1).any()
    got = _run(eng, v, fdr, codes, n_bins, 100, None)
    want = restated_strata(v, fdr, codes, n_bins, 0.1, 100, None)
    if n_bins == 50:
        # the density tolerance is derived for groups of at most 4 133 kept cells: bin 0, which took the emptied bin's cells
        # too, is past that and keeps the other comparisons only
        big = want['n_kept'] > 4096 + 37
        assert big.tolist() == [True] + [False] * 49 and (want['n_kept'][1:] > 0).sum() == 48
        seen = dict(got, vals=np.where(big[:, None], want['vals'], got['vals']))
        _compare(seen, want, v, codes, n_bins, '%d cells %d bins' % (N_CARRY, n_bins))
    else:
        for k in EXACT:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    again = _run(eng, v, fdr, codes, n_bins, 100, None)
    for k in got:
        np.testing.assert_array_equal(got[k], again[k], err_msg='second call: ' + k)


# ------------------------------------------------------------------ 2. the two callers do not see each other
def test_bins_and_strata_do_not_see_each_other(eng):
    from cna_amd._ffi import CnaHipError
    M = counts_matrix(1000, 130, seed=51)
    rs = np.random.RandomState(51)
    M.data = M.data * rs.rand(M.nnz)                           # real-valued: a changed order would show
    X = as_form(M, 'csr-i32')
    bcodes = codes_for(1000, 50, seed=51)
    v, fdr, scodes = columns_for(4133, 7, seed=52)

    def bins():
        eng.ensure_expression(X)
        return eng.expr_to_bins(bcodes, 50, 0)

    def strata():
        return _run(eng, v, fdr, scodes, 7, 100, None)

    def refused_bins():
        bad = bcodes.copy()
        bad[777] = 50                                          # a code equal to n_bins
        with pytest.raises(CnaHipError, match='outside'):
            eng.expr_to_bins(bad, 50, 0)

    def refused_strata():
        bad = scodes.copy()
        bad[777] = 7
        with pytest.raises(CnaHipError, match='outside'):
            _run(eng, v, fdr, bad, 7, 100, None)

    def same_bins(got, tag):
        np.testing.assert_array_equal(got[0], bins_alone[0], err_msg=tag)
        np.testing.assert_array_equal(got[1], bins_alone[1], err_msg=tag)

    def same_strata(got, tag):
        for k in strata_alone:
            np.testing.assert_array_equal(got[k], strata_alone[k], err_msg='%s %s' % (tag, k))

    eng.drop_expression()
    bins_alone = bins()
    eng.drop_expression()                                      # frees every work buffer of either
    strata_alone = strata()
    eng.drop_expression()
    np.testing.assert_array_equal(bins_alone[1], restated_bins(M, bcodes, 50, 0)[1])
    np.testing.assert_array_equal(strata_alone['n_kept'], restated_strata(v, fdr, scodes, 7, 0.1, 100, None)['n_kept'])

    same_bins(bins(), 'bins first')
    same_strata(strata(), 'strata after bins')
    same_bins(bins(), 'bins after strata')
    eng.drop_expression()
    same_strata(strata(), 'strata first')
    same_bins(bins(), 'bins after strata')
    same_strata(strata(), 'strata after bins')
    refused_bins()
    same_strata(strata(), 'strata after refused bins')
    same_bins(bins(), 'bins before refused strata')
    refused_strata()
    same_bins(bins(), 'bins after refused strata')
