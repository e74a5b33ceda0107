"""cna.tl.gene_markers_within / cna_gene_ranksum_within on the device (run with -m gpu on an MI355X).

The device returns integers (the summed D, the blocks that can tell, the kept cells per block and level, the NaN flags) and
two float64 sums folded over the blocks in a stated order with every product and sum rounded once, from tie terms that are
integers below 2^53 on every shape here (the largest: 7 055 790 714): the integers are compared with assert_array_equal and
the float64 sums BIT FOR BIT against the numpy / scipy restatement of tests/test_gene_markers_within_host.py, which that
file checks against scipy.stats.mannwhitneyu per block on these same inputs.  The inputs are the nine core genes in four
forms with the nine blocks of tests/test_gene_rank_corr_strata_host.py: in one block gene 4's tie runs on and across the cuts
of the walk's unit, two blocks that share a value across their boundary, blocks of 1 and 2 kept cells, two empty blocks,
blocks in which a level is absent, a sparse gene without a stored entry in a block."""
import numpy as np
import pytest

from test_gene_markers_host import FORMS, N_CORE, SMALL_WORK_BYTES, core_codes, core_input, core_values, sparse_of, markers_input
from test_gene_rank_corr_host import RHO_TOL, rank_corr_tiles
from test_gene_rank_corr_strata_host import STRATA_LEVELS, strata_labels
from test_gene_markers_within_host import (assert_frame_matches, van_elteren_table, weight_tables, within_codes, within_reference,
                                           _factor)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _equal(name, got, want):
    """d2, num, tiew, live, n, nan against the restatement: integers equal, the float64 sums bit for bit; the numbers of a
    flagged gene are unspecified"""
    ok = ~want[5]
    np.testing.assert_array_equal(got[5], want[5], err_msg=name + ' nan')
    np.testing.assert_array_equal(got[4], want[4], err_msg=name + ' n')
    np.testing.assert_array_equal(got[0][:, ok], want[0][:, ok], err_msg=name + ' d2')
    np.testing.assert_array_equal(got[3][:, ok], want[3][:, ok], err_msg=name + ' live')
    np.testing.assert_array_equal(_bits(got[1][:, ok]), _bits(want[1][:, ok]), err_msg=name + ' num')
    np.testing.assert_array_equal(_bits(got[2][:, ok]), _bits(want[2][:, ok]), err_msg=name + ' tiew')
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[2].dtype == np.float64
    assert got[3].dtype == np.int32 and got[4].dtype == np.int64 and got[5].dtype == bool
    assert got[0].shape == want[0].shape and got[4].shape == want[4].shape


def _same_bits(a, b, ok=slice(None)):
    np.testing.assert_array_equal(a[0][:, ok], b[0][:, ok])
    np.testing.assert_array_equal(_bits(a[1][:, ok]), _bits(b[1][:, ok]))
    np.testing.assert_array_equal(_bits(a[2][:, ok]), _bits(b[2][:, ok]))
    np.testing.assert_array_equal(a[3][:, ok], b[3][:, ok])
    np.testing.assert_array_equal(a[4], b[4])
    np.testing.assert_array_equal(a[5], b[5])


def _run(eng, which='core', weights='ve', work_bytes=0):
    codes, L, blocks, B = within_codes(which)
    return eng.gene_ranksum_within(codes, L, blocks, B, *weight_tables(codes, L, blocks, B, weights), work_bytes=work_bytes)


# ------------------------------------------------------------------ the nine genes, four forms, nine blocks
@pytest.mark.parametrize('form', FORMS)
def test_core_case_equals_the_restatement(eng, form):
    eng.ensure_expression(core_input(form))
    got = _run(eng)
    want = within_reference(form)
    _equal(form, got, want)
    assert list(np.flatnonzero(got[5])) == [7]                               # the kept NaN; the left-out one sets nothing
    _equal(form + ' arbitrary weights', _run(eng, weights='any'), within_reference(form, 'core', 'any'))
    assert (weight_tables(*within_codes(), 'any')[0] < 0).any() and (weight_tables(*within_codes(), 'any')[1] < 0).any()
    # the same bits on a second run and under the small budget, which cuts two tiles of genes at least
    assert len(rank_corr_tiles(form, SMALL_WORK_BYTES)[0]) >= 2 and len(rank_corr_tiles(form, 0)[0]) == 1   # {key, cell} entries
    ok = ~want[5]
    _same_bits(_run(eng), got, ok)
    _same_bits(_run(eng, work_bytes=SMALL_WORK_BYTES), got, ok)


@pytest.mark.parametrize('form', FORMS)
def test_one_block_of_all_kept_cells_is_the_pooled_call(eng, form):
    eng.ensure_expression(core_input(form))
    codes = core_codes()
    rank2, tie, n, nan = eng.gene_ranksum_by(codes, 4)
    d2, num, tiew, live, nw, nanw = _run(eng, 'one', 'ones')
    m = int(n.sum())
    ok = ~nan
    np.testing.assert_array_equal(nanw, nan)
    np.testing.assert_array_equal(nw[0], n)
    np.testing.assert_array_equal(d2[:, ok], (rank2 - (n * (m + 1))[:, None])[:, ok])
    np.testing.assert_array_equal(_bits(tiew[:, ok]), _bits(np.broadcast_to(tie, tiew.shape)[:, ok]))
    np.testing.assert_array_equal(_bits(num[:, ok]), _bits(d2[:, ok].astype(np.float64)))
    _equal(form + ' one block', (d2, num, tiew, live, nw, nanw), within_reference(form, 'one', 'ones'))


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_every_block_alone_and_their_sum(eng, form):
    """the call with the blocks set to -1 outside block s is the 1-block call on those cells; the integer sum of these
    single-block d2 is the full call's"""
    eng.ensure_expression(core_input(form))
    codes, L, blocks, B = within_codes()
    w_num, w_tie = weight_tables(codes, L, blocks, B, 'any')
    full = eng.gene_ranksum_within(codes, L, blocks, B, np.ones(B), np.ones((B, L)))
    ok = ~full[5]
    total = np.zeros_like(full[0])
    for s in range(B):
        masked = eng.gene_ranksum_within(codes, L, np.where(blocks == s, blocks, -1).astype(np.int32), B, w_num, w_tie)
        alone = eng.gene_ranksum_within(codes, L, np.where(blocks == s, 0, -1).astype(np.int32), 1, w_num[s:s + 1], w_tie[s:s + 1])
        good = ok & ~masked[5]
        np.testing.assert_array_equal(masked[5], alone[5])
        np.testing.assert_array_equal(masked[0][:, good], alone[0][:, good])
        np.testing.assert_array_equal(_bits(masked[1][:, good]), _bits(alone[1][:, good]))
        np.testing.assert_array_equal(_bits(masked[2][:, good]), _bits(alone[2][:, good]))
        np.testing.assert_array_equal(masked[3][:, good], alone[3][:, good])
        np.testing.assert_array_equal(masked[4][s], alone[4][0])
        assert masked[4].sum() == alone[4].sum() == full[4][s].sum()
        total += np.where(ok[None, :], alone[0], 0)
    np.testing.assert_array_equal(total[:, ok], full[0][:, ok])


@pytest.mark.parametrize('form', ['csc-f64', 'dense-f32'])
def test_255_blocks(eng, form):
    eng.ensure_expression(core_input(form))
    got = _run(eng, '255')
    _equal(form + ' 255 blocks', got, within_reference(form, '255'))
    assert got[4].shape == (255, 4) and got[4][254].sum() > 0 and (got[4].sum(axis=1) == 0).any()


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_1024_levels_in_nine_blocks(eng, form):
    eng.ensure_expression(core_input(form))
    got = _run(eng, '1024')
    _equal(form + ' 1024 levels', got, within_reference(form, '1024'))
    assert got[0].shape == (1024, 9) and got[4][:, 1023].sum() > 0 and got[0][1023].any()


def test_uploads_of_one_matrix_agree(eng):
    """CSR and CSC of one matrix: the same bits; its dense upload too"""
    V, S = core_values()
    out = {}
    for fmt, idx in (('csr', np.int32), ('csc', np.int64)):
        eng.ensure_expression(sparse_of(V, S, fmt, np.float64, idx))
        out[fmt] = _run(eng)
    ok = ~out['csr'][5]
    _same_bits(out['csr'], out['csc'], ok)
    eng.ensure_expression(np.ascontiguousarray(V))
    _same_bits(_run(eng), out['csr'], ok)


# ------------------------------------------------------------------ refusals and residency
def test_refusals_write_nothing(eng):
    from cna_amd import _ffi
    eng.ensure_expression(core_input('csr-f32'))
    codes, L, blocks, B = within_codes()
    w_num, w_tie = weight_tables(codes, L, blocks, B, 've')

    def call(n_bins=L, n_blocks=B, the_codes=codes, the_blocks=blocks, num=w_num, tie=w_tie, work_bytes=0, drop=None):
        out = [np.full((1025, 9), -77, dtype=np.int64), np.full((1025, 9), -77.0), np.full((1025, 9), -77.0),
               np.full((1025, 9), -77, dtype=np.int32), np.full((256, 1025), -77, dtype=np.int64), np.full(9, 77, dtype=np.uint8)]
        ptrs = [_ffi.ptr(a) for a in out]
        if drop is not None:
            ptrs[drop] = None
        rc = eng.lib.cna_gene_ranksum_within(eng.h, _ffi.ptr(the_codes), n_bins, _ffi.ptr(the_blocks), n_blocks, _ffi.ptr(num),
                                             _ffi.ptr(tie), work_bytes, *ptrs)
        assert (out[0] == -77).all() and (out[1] == -77.0).all() and (out[2] == -77.0).all() and (out[3] == -77).all()
        assert (out[4] == -77).all() and (out[5] == 77).all()
        return rc, eng.lib.cna_last_error()

    wide_num, wide_tie = np.ones(256), np.ones((256, 1025))
    for n_blocks in (0, 256):
        rc, msg = call(n_blocks=n_blocks, num=wide_num, tie=wide_tie)
        assert rc == -1 and b'1 <= n_blocks <= 255' in msg                   # CNA_EINVAL
    for n_bins in (0, 1025):
        rc, msg = call(n_bins=n_bins, num=wide_num, tie=wide_tie)
        assert rc == -1 and b'1 <= n_bins <= 1024' in msg
    wrong = blocks.copy()
    wrong[N_CORE - 1] = B
    rc, msg = call(the_blocks=wrong)
    assert rc == -1 and b'a block code lies outside [-1, n_blocks)' in msg
    wrong = codes.copy()
    wrong[N_CORE // 2] = L
    rc, msg = call(the_codes=wrong)
    assert rc == -1 and b'a level code lies outside [-1, n_bins)' in msg
    for which in ('num', 'tie'):
        bad_num, bad_tie = w_num.copy(), w_tie.copy()
        (bad_num if which == 'num' else bad_tie).flat[-1] = np.nan
        rc, msg = call(num=bad_num, tie=bad_tie)
        assert rc == -1 and b'a weight is not finite' in msg
    rc, msg = call(work_bytes=-5)
    assert rc == -1 and b'work_bytes' in msg
    rc, msg = call(drop=3)
    assert rc == -1 and b'null pointer' in msg
    with pytest.raises(_ffi.CnaHipError, match='n_blocks <= 255'):
        eng.gene_ranksum_within(codes, L, blocks, 256, wide_num, wide_tie[:, :L])
    with pytest.raises(ValueError):
        eng.gene_ranksum_within(codes[:-1], L, blocks, B, w_num, w_tie)
    with pytest.raises(ValueError):
        eng.gene_ranksum_within(codes, L, blocks, B, w_num[:-1], w_tie)
    _equal('after the refusals', _run(eng), within_reference('csr-f32'))


def test_no_resident_matrix_is_refused_and_drop_frees_the_buffers(eng):
    from cna_amd import _ffi
    eng.unpin_expression()
    eng.drop_expression()
    base = eng.device_bytes()
    out = [np.zeros((1, 1), dtype=np.int64), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1), dtype=np.int32),
           np.zeros((1, 1), dtype=np.int64), np.zeros(1, dtype=np.uint8)]
    zeros = np.zeros(10, dtype=np.int32)
    rc = eng.lib.cna_gene_ranksum_within(eng.h, _ffi.ptr(zeros), 1, _ffi.ptr(zeros), 1, _ffi.ptr(np.ones(1)), _ffi.ptr(np.ones(1)),
                                         0, *[_ffi.ptr(a) for a in out])
    assert rc == -4 and b'no expression matrix' in eng.lib.cna_last_error()  # CNA_ESTATE
    for form in ('dense-f64', 'csr-f32'):
        eng.ensure_expression(core_input(form))
        _run(eng)
        assert eng.device_bytes() > base
        eng.drop_expression()                       # the work buffers go with the matrix
        assert eng.device_bytes() == base


def test_between_launch_and_fetch_of_a_local_null(eng):
    """the call between cna_null_local_launch and cna_null_local_fetch: the pending pass returns what it returns without the
    call in between, bit for bit, and the call's own numbers are the restatement's"""
    from cna_amd import synth
    from test_gpu_gene_corr import _walk
    N, P = 50, 640
    data, meta = synth.make_dataset(20000, N, k=15, seed=21)
    rs = np.random.RandomState(4)
    y = rs.randn(N)
    y = (y - y.mean()) / y.std()
    Y = np.column_stack([y, rs.randn(N, P)])
    out = []
    for insert in (False, True):
        eng.null_local_discard()
        eng.drop_graph()
        _walk(eng, data, N)
        nz, maxabs = eng.select_standardized(None, None, y=y)
        maxcorr = max(maxabs, 0.001)
        thr = np.arange(maxcorr / 4, maxcorr, maxcorr / 400)
        edges = thr ** 2 - 1e-8 - 1e-5 * thr ** 2
        eng.condition(np.eye(N), Y)
        eng.null_local_launch(1, P, edges, thr)
        if insert:
            eng.ensure_expression(core_input('csr-f32'))
            _equal('between launch and fetch', _run(eng), within_reference('csr-f32'))
        fetched = eng.null_local_fetch()
        out.append([np.asarray(f).copy() for f in fetched])
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)
    eng.drop_graph()


# ------------------------------------------------------------------ end to end
def test_gene_markers_within_against_mannwhitneyu_per_block(eng):
    import cna_amd as cna
    d = markers_input()
    d.obs['sample'] = strata_labels(len(d.obs))
    out = cna.tl.gene_markers_within(d, 'pop', 'sample', engine=eng)
    codes, levels = _factor(d.obs['pop'])
    blocks, samples = _factor(d.obs['sample'])
    assert out.shape == (6, 15) and list(out.columns.get_level_values(0)[::5]) == levels
    kept = (codes >= 0) & (blocks >= 0)
    np.testing.assert_array_equal(out.attrs['counts'].values,
                                  np.bincount(blocks[kept] * 3 + codes[kept], minlength=9).reshape(3, 3))     # the integers: exact
    assert list(out.attrs['n_cells'].values) == [int((kept & (codes == b)).sum()) for b in range(3)]
    assert assert_frame_matches(out, levels, van_elteren_table(d.X, codes, 3, blocks, 3), 6) == 18       # auc, z within RHO_TOL
    assert RHO_TOL == 1e-10
