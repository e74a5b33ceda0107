"""cna.tl.gene_rank_corr_strata / cna_gene_rank_corr_by on the device (run with -m gpu on an MI355X).

The device returns integers per level (S on 128 bits in two limbs, the kept cells, the NaN flags) and tie terms that are
integers below 2^53 on every shape here, so everything is compared with assert_array_equal against the numpy / scipy
restatement of tests/test_gene_rank_corr_strata_host.py, which that file checks against scipy.stats.spearmanr per level on
these same inputs.  It also proves what the inputs reach: inside one level tie runs on and across the cuts of the kernels'
unit, a value shared across the boundary of two levels, levels of 0, 1 and 2 kept cells, a tile of genes without an entry
and two tiles at least under SMALL_WORK_BYTES, three sort chunks per long gene and per key."""
import numpy as np
import pytest
import scipy.stats

from test_gene_markers_host import (FORMS, CORE_LEVELS, N_CORE, SMALL_WORK_BYTES, core_codes, core_input, core_reference,
                                    core_values, sparse_of, markers_input)
from test_gene_rank_corr_host import (RHO_TOL, WIDE_CELLS, as_engine, core_keys, core_rank_reference, end_to_end_keys, limbs,
                                      wide_input)
from test_gene_rank_corr_strata_host import (STRATA_LEVELS, as_engine_by, many_codes, restated_rank_corr_by, strata_codes,
                                             strata_labels, strata_reference)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()


def _equal(name, got, restated):
    """s_lo, s_hi, tie_gene, tie_key, m, nan against the restatement; the numbers of a flagged gene are unspecified"""
    want = as_engine_by(restated)
    ok = ~want[5]
    np.testing.assert_array_equal(got[4], want[4], err_msg=name + ' m')
    np.testing.assert_array_equal(got[5], want[5], err_msg=name + ' nan')
    np.testing.assert_array_equal(got[0][:, :, ok], want[0][:, :, ok], err_msg=name + ' s_lo')
    np.testing.assert_array_equal(got[1][:, :, ok], want[1][:, :, ok], err_msg=name + ' s_hi')
    np.testing.assert_array_equal(got[2][:, ok], want[2][:, ok], err_msg=name + ' tie_gene')
    np.testing.assert_array_equal(got[3], want[3], err_msg=name + ' tie_key')
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int64 and got[2].dtype == np.float64
    assert got[3].dtype == np.float64 and got[4].dtype == np.int64 and got[5].dtype == bool
    assert got[0].shape == want[0].shape and got[2].shape == want[2].shape and got[3].shape == want[3].shape


def _same_bits(a, b, ok=slice(None)):
    np.testing.assert_array_equal(a[0][:, :, ok], b[0][:, :, ok])
    np.testing.assert_array_equal(a[1][:, :, ok], b[1][:, :, ok])
    np.testing.assert_array_equal(a[2][:, ok].view(np.int64), b[2][:, ok].view(np.int64))
    np.testing.assert_array_equal(a[3].view(np.int64), b[3].view(np.int64))
    np.testing.assert_array_equal(a[4], b[4])
    np.testing.assert_array_equal(a[5], b[5])


def _level_equals_whole(by, l, whole, ok):
    """level l of the new entry against what cna_gene_rank_corr returned: limbs, both tie terms and m"""
    np.testing.assert_array_equal(by[0][l][:, ok], whole[0][:, ok])
    np.testing.assert_array_equal(by[1][l][:, ok], whole[1][:, ok])
    np.testing.assert_array_equal(by[2][l][ok].view(np.int64), whole[2][ok].view(np.int64))
    np.testing.assert_array_equal(by[3][l].view(np.int64), whole[3].view(np.int64))
    assert int(by[4][l]) == whole[4]


# ------------------------------------------------------------------ the nine genes, four forms
@pytest.mark.parametrize('form', FORMS)
def test_core_case_equals_the_restatement(eng, form):
    eng.ensure_expression(core_input(form))
    V, codes = core_keys(), strata_codes()
    got = eng.gene_rank_corr_by(V, codes, STRATA_LEVELS)
    want = strata_reference(form)
    _equal(form, got, want)
    ok = ~want[4]
    assert list(np.flatnonzero(got[5])) == [7]                               # the kept NaN; the left-out one sets nothing
    # under the small budget (two tiles of genes at least, one column at a time) the same bits; and on a second run
    _same_bits(eng.gene_rank_corr_by(V, codes, STRATA_LEVELS, SMALL_WORK_BYTES), got, ok)
    _same_bits(eng.gene_rank_corr_by(V, codes, STRATA_LEVELS), got, ok)


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_level_equals_the_whole_call_on_masked_keys(eng, form):
    eng.ensure_expression(core_input(form))
    V, codes = core_keys(), strata_codes()
    by = eng.gene_rank_corr_by(V, codes, STRATA_LEVELS)
    ok = ~by[5]
    for l in range(STRATA_LEVELS):
        _level_equals_whole(by, l, eng.gene_rank_corr(np.where(codes == l, V, np.nan)), ok)


@pytest.mark.parametrize('form', FORMS)
def test_one_level_of_all_cells_is_the_whole_call_bit_for_bit(eng, form):
    eng.ensure_expression(core_input(form))
    V = core_keys()
    whole = eng.gene_rank_corr(V)
    by = eng.gene_rank_corr_by(V, np.zeros(N_CORE, dtype=np.int32), 1)
    _level_equals_whole(by, 0, whole, slice(None))
    np.testing.assert_array_equal(by[5], whole[5])
    for a in (whole, (by[0][0], by[1][0], by[2][0], by[3][0], int(by[4][0]), by[5])):    # and both are the restatement
        want = as_engine(core_rank_reference(form))
        np.testing.assert_array_equal(a[0][:, ~want[5]], want[0][:, ~want[5]])
        np.testing.assert_array_equal(a[3], want[3])


@pytest.mark.parametrize('q', [1, 16])
@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_one_key_and_sixteen_keys(eng, form, q):
    eng.ensure_expression(core_input(form))
    got = eng.gene_rank_corr_by(core_keys(q), strata_codes(), STRATA_LEVELS)
    assert got[0].shape == (STRATA_LEVELS, q, 9)
    _equal('%s q=%d' % (form, q), got, strata_reference(form, q))
    _same_bits(eng.gene_rank_corr_by(core_keys(q), strata_codes(), STRATA_LEVELS, SMALL_WORK_BYTES), got, ~got[5])


@pytest.mark.parametrize('form', FORMS)
def test_tiles_of_several_keys_and_a_shorter_last_one(eng, form):
    """Five keys under 160 000 bytes: an entry of a key's segment costs 24 bytes, so 6666 entries fit and the keys of 3001
    cells go two, two and one to a tile -- the second and third tiles begin at key 2 and key 4, where the key's index, its
    first chunk, its first entry and its rows of the level pass' scan all matter.  The same budget cuts the dense genes into
    tiles of two (float64) or three (float32).  The same bits as under the default budget, where all keys are one tile."""
    assert 160000 // 24 // N_CORE == 2
    eng.ensure_expression(core_input(form))
    V, codes = core_keys(5), strata_codes()
    got = eng.gene_rank_corr_by(V, codes, STRATA_LEVELS)
    _equal('%s q=5' % form, got, strata_reference(form, 5))
    _same_bits(eng.gene_rank_corr_by(V, codes, STRATA_LEVELS, 160000), got, ~got[5])


@pytest.mark.parametrize('form', ['csc-f64', 'dense-f32'])
def test_255_levels(eng, form):
    eng.ensure_expression(core_input(form))
    codes = many_codes(255)
    got = eng.gene_rank_corr_by(core_keys(), codes, 255)
    Vg, _ = core_values()
    _equal(form, got, restated_rank_corr_by(Vg.astype(np.float32 if form.endswith('f32') else np.float64), core_keys(), codes, 255))
    assert got[4][254] > 0 and (got[4] == 0).any()


def test_bad_counts_are_refused_and_nothing_is_written(eng):
    from cna_amd import _ffi
    eng.ensure_expression(core_input('csr-f32'))
    V = np.ascontiguousarray(np.tile(core_keys(1), (17, 1)))
    codes = np.zeros(N_CORE, dtype=np.int32)

    def call(q, n_bins, work_bytes=0, the_codes=codes, drop=None):
        out = [np.full((2, 17, 9), 77, dtype=np.uint64), np.full((2, 17, 9), -77, dtype=np.int64), np.full((2, 9), -77.0),
               np.full((2, 17), -77.0), np.full(2, -77, dtype=np.int64), np.full(9, 77, dtype=np.uint8)]
        ptrs = [_ffi.ptr(a) for a in out]
        if drop is not None:
            ptrs[drop] = None
        rc = eng.lib.cna_gene_rank_corr_by(eng.h, _ffi.ptr(V), q, _ffi.ptr(the_codes), n_bins, work_bytes, *ptrs)
        assert (out[0] == 77).all() and (out[1] == -77).all() and (out[2] == -77.0).all() and (out[3] == -77.0).all()
        assert (out[4] == -77).all() and (out[5] == 77).all()
        return rc, eng.lib.cna_last_error()

    for q in (17, 0, -1):
        rc, msg = call(q, 1)
        assert rc == -1 and b'1 <= q <= 16' in msg                             # CNA_EINVAL
    for n_bins in (256, 0, -3):
        rc, msg = call(1, n_bins)
        assert rc == -1 and b'1 <= n_bins <= 255' in msg
    rc, msg = call(1, 1, work_bytes=-5)
    assert rc == -1 and b'work_bytes' in msg
    rc, msg = call(1, 1, drop=5)
    assert rc == -1 and b'null pointer' in msg
    for bad in (1, -2):
        wrong = codes.copy()
        wrong[N_CORE - 1] = bad
        rc, msg = call(1, 1, the_codes=wrong)
        assert rc == -1 and b'a code lies outside [-1, n_bins)' in msg
    with pytest.raises(_ffi.CnaHipError, match='1 <= q <= 16'):
        eng.gene_rank_corr_by(V, codes, 1)
    with pytest.raises(_ffi.CnaHipError, match='n_bins <= 255'):
        eng.gene_rank_corr_by(core_keys(), codes, 256)
    with pytest.raises(ValueError):
        eng.gene_rank_corr_by(core_keys()[:, :-1], codes, 1)
    with pytest.raises(ValueError):
        eng.gene_rank_corr_by(core_keys(), codes[:-1], 1)
    _equal('after the refusals', eng.gene_rank_corr_by(core_keys(), strata_codes(), STRATA_LEVELS), strata_reference('csr-f32'))


def test_uploads_of_one_matrix_agree(eng):
    """CSR and CSC of one matrix: the same bits; its dense upload: equal integers"""
    Vg, S = core_values()
    V, codes = core_keys(), strata_codes()
    out = {}
    for fmt, idx in (('csr', np.int32), ('csc', np.int64)):
        eng.ensure_expression(sparse_of(Vg, S, fmt, np.float64, idx))
        out[fmt] = eng.gene_rank_corr_by(V, codes, STRATA_LEVELS)
    ok = ~out['csr'][5]
    _same_bits(out['csr'], out['csc'], ok)
    eng.ensure_expression(np.ascontiguousarray(Vg))
    _same_bits(eng.gene_rank_corr_by(V, codes, STRATA_LEVELS), out['csr'], ok)


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_marker_rank_and_strata_calls_share_their_buffers(eng, form):
    """2-byte levels and 4-byte cells ride in the same buffers, and the new entry's odd pass count leaves its lists in the
    other one of each pair: each call finds them sized and filled for itself whatever ran before"""
    from test_gpu_gene_markers import _equal as markers_equal, _same_bits as markers_same_bits
    from test_gpu_gene_rank_corr import _equal as rank_equal, _same_bits as rank_same_bits
    eng.drop_expression()                                                    # fresh buffers: the first call sizes them
    eng.ensure_expression(core_input(form))
    codes, V, levels = core_codes(), core_keys(), strata_codes()
    marks = eng.gene_ranksum_by(codes, CORE_LEVELS)
    ranks = eng.gene_rank_corr(V)
    strata = eng.gene_rank_corr_by(V, levels, STRATA_LEVELS)
    marks2 = eng.gene_ranksum_by(codes, CORE_LEVELS)
    ranks2 = eng.gene_rank_corr(V)
    strata2 = eng.gene_rank_corr_by(V, levels, STRATA_LEVELS)
    markers_equal(form, marks, core_reference(form))
    markers_same_bits(marks, marks2, ~marks[3])
    rank_equal(form, ranks, core_rank_reference(form))
    rank_same_bits(ranks, ranks2, ~ranks[5])
    _equal(form, strata, strata_reference(form))
    _same_bits(strata, strata2, ~strata[5])
    # and the new entry first, from fresh buffers
    eng.drop_expression()
    eng.ensure_expression(core_input(form))
    _same_bits(eng.gene_rank_corr_by(V, levels, STRATA_LEVELS), strata, ~strata[5])
    rank_same_bits(eng.gene_rank_corr(V), ranks, ~ranks[5])
    markers_same_bits(eng.gene_ranksum_by(codes, CORE_LEVELS), marks, ~marks[3])


def test_the_sum_passes_64_bits_inside_one_level(eng):
    """3 100 000 cells in levels of 3 050 000 and 50 000: genes and key monotone in each other with distinct values, so
    S_l = +-(m_l^3 - m_l) / 3 in closed form per level; the large level's passes a signed 64-bit sum, the small one's not"""
    X, key, _ = wide_input()
    sizes = [3050000, 50000]
    assert sum(sizes) == WIDE_CELLS
    codes = np.zeros(WIDE_CELLS, dtype=np.int32)
    codes[np.random.RandomState(3).permutation(WIDE_CELLS)[:sizes[1]]] = 1
    S = [(m ** 3 - m) // 3 for m in sizes]
    assert S[0] > 2 ** 63 - 1 and S[1] <= 2 ** 63 - 1
    eng.ensure_expression(X)
    s_lo, s_hi, tie_gene, tie_key, m, nan = eng.gene_rank_corr_by(key[None, :], codes, 2)
    assert m.tolist() == sizes and not nan.any() and not tie_gene.any() and not tie_key.any()
    for l in range(2):
        want_lo, want_hi = limbs(np.array([[S[l], -S[l]]], dtype=object))
        np.testing.assert_array_equal(s_hi[l], want_hi)
        np.testing.assert_array_equal(s_lo[l], want_lo)
    assert s_hi.tolist() == [[[0, -1]], [[0, -1]]]
    eng.drop_expression()


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f32'])
def test_no_kept_cell_in_any_level(eng, form):
    from cna_amd.tools._gene_rank_corr import rank_corr_statistics
    eng.ensure_expression(core_input(form))
    got = eng.gene_rank_corr_by(np.full((2, N_CORE), np.nan), strata_codes(), STRATA_LEVELS)
    assert not got[4].any() and not got[0].any() and not got[1].any() and not got[2].any() and not got[3].any()
    assert np.isnan(rank_corr_statistics(got[0][0], got[1][0], got[2][0], got[3][0], 0, got[5])).all()


# ------------------------------------------------------------------ residency
def test_no_resident_matrix_is_refused_and_drop_frees_the_buffers(eng):
    from cna_amd import _ffi
    eng.unpin_expression()
    eng.drop_expression()
    base = eng.device_bytes()
    out = [np.zeros((1, 1, 1), dtype=np.uint64), np.zeros((1, 1, 1), dtype=np.int64), np.zeros((1, 1)), np.zeros((1, 1)),
           np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint8)]
    V, codes = np.zeros((1, 10)), np.zeros(10, dtype=np.int32)
    rc = eng.lib.cna_gene_rank_corr_by(eng.h, _ffi.ptr(V), 1, _ffi.ptr(codes), 1, 0, *[_ffi.ptr(a) for a in out])
    assert rc == -4 and b'no expression matrix' in eng.lib.cna_last_error()  # CNA_ESTATE
    for form in ('dense-f64', 'csr-f32'):
        eng.ensure_expression(core_input(form))
        eng.gene_rank_corr_by(core_keys(), strata_codes(), STRATA_LEVELS)
        assert eng.device_bytes() > base
        eng.drop_expression()                       # the work buffers go with the matrix
        assert eng.device_bytes() == base


# ------------------------------------------------------------------ end to end
def test_gene_rank_corr_strata_against_spearmanr(eng):
    import cna_amd as cna
    d = markers_input()
    d.obs['coef'], d.obs['score'] = end_to_end_keys(len(d.obs))
    d.obs['cluster'] = strata_labels(len(d.obs))
    out = cna.tl.gene_rank_corr_strata(d, 'cluster', ['coef', 'score'], engine=eng)
    kept = np.isfinite(d.obs['coef'].values) & np.isfinite(d.obs['score'].values)
    levels = ['c0', 'c1', 'tiny']
    assert out.shape == (6, 6) and sorted(out.attrs['n_cells'].index) == levels
    Xd = d.X.astype(np.float64)
    checked = 0
    for lev in levels:
        cells = kept & (d.obs['cluster'].values == lev)
        assert out.attrs['n_cells'][lev] == int(cells.sum())
        for k in ('coef', 'score'):
            for g in range(6):
                x, v = Xd[cells, g], d.obs[k].values[cells]
                if np.ptp(x) == 0 or np.ptp(v) == 0:
                    assert np.isnan(out[(k, lev)].iloc[g])
                    continue
                want = scipy.stats.spearmanr(x, v).statistic
                print('%s %s gene %d: rho %.12f scipy %.12f' % (k, lev, g, out[(k, lev)].iloc[g], want))
                assert abs(out[(k, lev)].iloc[g] - want) <= RHO_TOL
                checked += 1
    assert checked >= 24
