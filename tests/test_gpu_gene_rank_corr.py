"""cna.tl.gene_rank_corr / cna_gene_rank_corr on the device (run with -m gpu on an MI355X).

The device returns integers (S on 128 bits in two limbs, the kept cells, the NaN flags) and tie terms that are integers below
2^53 on every shape here, so everything is compared with assert_array_equal against the numpy / scipy restatement of
tests/test_gene_rank_corr_host.py, which that file checks against scipy.stats.spearmanr on these same inputs.  It also proves
what the inputs reach: three sort chunks per long gene and per key, two tiles of genes and one per key under SMALL_WORK_BYTES,
tie runs on and across the cuts of the kernels' unit, a sum beyond 64 bits."""
import numpy as np
import pytest
import scipy.stats

from test_gene_markers_host import (FORMS, CORE_LEVELS, N_CORE, SMALL_WORK_BYTES, core_codes, core_input, core_reference,
                                    core_values, sparse_of, markers_input)
from test_gene_rank_corr_host import (RHO_TOL, WIDE_CELLS, as_engine, core_keys, core_rank_reference, end_to_end_keys, limbs,
                                      wide_input)

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
    want = as_engine(restated)
    ok = ~want[5]
    assert got[4] == want[4], name + ' m'
    np.testing.assert_array_equal(got[5], want[5], err_msg=name + ' nan')
    np.testing.assert_array_equal(got[0][:, ok], want[0][:, ok], err_msg=name + ' s_lo')
    np.testing.assert_array_equal(got[1][:, ok], want[1][:, ok], err_msg=name + ' s_hi')
    np.testing.assert_array_equal(got[2][ok], want[2][ok], err_msg=name + ' tie_gene')
    np.testing.assert_array_equal(got[3], want[3], err_msg=name + ' tie_key')
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int64 and got[2].dtype == np.float64
    assert got[3].dtype == np.float64 and isinstance(got[4], int) and got[5].dtype == bool


def _same_bits(a, b, ok=slice(None)):
    np.testing.assert_array_equal(a[0][:, ok], b[0][:, ok])
    np.testing.assert_array_equal(a[1][:, ok], b[1][:, ok])
    np.testing.assert_array_equal(a[2][ok].view(np.int64), b[2][ok].view(np.int64))
    np.testing.assert_array_equal(a[3].view(np.int64), b[3].view(np.int64))
    assert a[4] == b[4]
    np.testing.assert_array_equal(a[5], b[5])


# ------------------------------------------------------------------ the nine genes, four forms
@pytest.mark.parametrize('form', FORMS)
def test_core_case_equals_the_restatement(eng, form):
    eng.ensure_expression(core_input(form))
    V = core_keys()
    got = eng.gene_rank_corr(V)
    want = core_rank_reference(form)
    _equal(form, got, want)
    m, ok = want[3], ~want[4]
    assert m == int((core_codes() >= 0).sum()) - 5                            # the intersection over the keys
    assert int(got[0][2, 1]) == (m ** 3 - m) // 3 and got[1][2, 1] == 0      # an increasing transform of gene 1
    assert got[2][1] == 0.0 and got[3][2] == 0.0
    assert got[2][2] == float(m ** 3 - m) and (got[0][:, 2] == 0).all() and (got[1][:, 2] == 0).all()    # the constant gene
    assert list(np.flatnonzero(got[5])) == [7]                               # the kept NaN; the left-out one sets nothing
    from cna_amd.tools._gene_rank_corr import rank_corr_statistics
    rho = rank_corr_statistics(*got)
    assert np.isnan(rho[:, [0, 2, 5, 7]]).all() and np.isfinite(rho[:, [1, 3, 4, 6, 8]]).all() and rho[2, 1] == 1.0
    # under the small budget (two tiles of genes at least, one column at a time) the same bits; and on a second run
    _same_bits(eng.gene_rank_corr(V, SMALL_WORK_BYTES), got, ok)
    _same_bits(eng.gene_rank_corr(V), got, ok)


@pytest.mark.parametrize('q', [1, 16])
@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_one_key_and_sixteen_keys(eng, form, q):
    eng.ensure_expression(core_input(form))
    got = eng.gene_rank_corr(core_keys(q))
    assert got[0].shape == (q, 9)
    _equal('%s q=%d' % (form, q), got, core_rank_reference(form, q))
    _same_bits(eng.gene_rank_corr(core_keys(q), SMALL_WORK_BYTES), got, ~got[5])


@pytest.mark.parametrize('form', FORMS)
def test_tiles_of_several_keys_and_a_shorter_last_one(eng, form):
    """Five keys under 160 000 bytes: an entry of a key's segment costs 24 bytes, so 6666 entries fit and the keys of 3001
    cells go two, two and one to a tile -- the second and third tiles begin at key 2 and key 4, where the key's index, its
    first chunk and its first entry all matter.  The same budget cuts the dense genes into tiles of two (float64) or three
    (float32).  The same bits as under the default budget, where all keys are one tile."""
    assert 160000 // 24 // N_CORE == 2
    eng.ensure_expression(core_input(form))
    V = core_keys(5)
    got = eng.gene_rank_corr(V)
    _equal('%s q=5' % form, got, core_rank_reference(form, 5))
    _same_bits(eng.gene_rank_corr(V, 160000), got, ~got[5])


def test_key_counts_outside_1_to_16_are_refused_and_nothing_is_written(eng):
    from cna_amd import _ffi
    eng.ensure_expression(core_input('csr-f32'))
    V = np.ascontiguousarray(np.tile(core_keys(1), (17, 1)))
    for q in (17, 0, -1):
        s_lo = np.full((17, 9), 77, dtype=np.uint64)
        s_hi = np.full((17, 9), -77, dtype=np.int64)
        tie_gene, tie_key = np.full(9, -77.0), np.full(17, -77.0)
        m = np.full(1, -77, dtype=np.int64)
        nan = np.full(9, 77, dtype=np.uint8)
        rc = eng.lib.cna_gene_rank_corr(eng.h, _ffi.ptr(V), q, 0, _ffi.ptr(s_lo), _ffi.ptr(s_hi), _ffi.ptr(tie_gene),
                                        _ffi.ptr(tie_key), m.ctypes.data_as(_ffi.c_i64p), _ffi.ptr(nan))
        assert rc == -1 and b'1 <= q <= 16' in eng.lib.cna_last_error()      # CNA_EINVAL
        assert (s_lo == 77).all() and (s_hi == -77).all() and (tie_gene == -77.0).all() and (tie_key == -77.0).all()
        assert m[0] == -77 and (nan == 77).all()
    m = np.zeros(1, dtype=np.int64)
    out = [np.zeros((1, 9), dtype=np.uint64), np.zeros((1, 9), dtype=np.int64), np.zeros(9), np.zeros(1)]
    nan = np.zeros(9, dtype=np.uint8)
    rc = eng.lib.cna_gene_rank_corr(eng.h, _ffi.ptr(V), 1, -5, *[_ffi.ptr(a) for a in out], m.ctypes.data_as(_ffi.c_i64p),
                                    _ffi.ptr(nan))
    assert rc == -1 and b'work_bytes' in eng.lib.cna_last_error()
    rc = eng.lib.cna_gene_rank_corr(eng.h, _ffi.ptr(V), 1, 0, *[_ffi.ptr(a) for a in out], m.ctypes.data_as(_ffi.c_i64p), None)
    assert rc == -1 and b'null pointer' in eng.lib.cna_last_error()
    with pytest.raises(_ffi.CnaHipError, match='1 <= q <= 16'):
        eng.gene_rank_corr(V)
    with pytest.raises(ValueError):
        eng.gene_rank_corr(core_keys()[:, :-1])
    _equal('after the refusals', eng.gene_rank_corr(core_keys()), core_rank_reference('csr-f32'))


def test_uploads_of_one_matrix_agree(eng):
    """CSR and CSC of one matrix: the same bits; its dense upload: equal integers"""
    Vg, S = core_values()
    V = core_keys()
    out = {}
    for fmt, idx in (('csr', np.int32), ('csc', np.int64)):
        eng.ensure_expression(sparse_of(Vg, S, fmt, np.float64, idx))
        out[fmt] = eng.gene_rank_corr(V)
    ok = ~out['csr'][5]
    _same_bits(out['csr'], out['csc'], ok)
    eng.ensure_expression(np.ascontiguousarray(Vg))
    _same_bits(eng.gene_rank_corr(V), out['csr'], ok)


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_marker_and_rank_correlation_calls_share_their_buffers(eng, form):
    """2-byte levels and 4-byte cells ride in the same buffers, 8-byte column keys in those of the genes' keys: each call finds
    them sized for itself whatever ran before"""
    from test_gpu_gene_markers import _equal as markers_equal, _same_bits as markers_same_bits
    eng.drop_expression()                                                    # fresh buffers: the first call sizes them
    eng.ensure_expression(core_input(form))
    codes, V = core_codes(), core_keys()
    marks = eng.gene_ranksum_by(codes, CORE_LEVELS)
    ranks = eng.gene_rank_corr(V)
    marks2 = eng.gene_ranksum_by(codes, CORE_LEVELS)
    ranks2 = eng.gene_rank_corr(V)
    markers_equal(form, marks, core_reference(form))
    markers_same_bits(marks, marks2, ~marks[3])
    _equal(form, ranks, core_rank_reference(form))
    _same_bits(ranks, ranks2, ~ranks[5])
    # and the other way round from fresh buffers
    eng.drop_expression()
    eng.ensure_expression(core_input(form))
    _same_bits(eng.gene_rank_corr(V), ranks, ~ranks[5])
    markers_same_bits(eng.gene_ranksum_by(codes, CORE_LEVELS), marks, ~marks[3])


def test_the_sum_passes_64_bits(eng):
    """3 100 000 cells: (m^3 - m) / 3 > 2^63 - 1, the smallest shape at which a 64-bit accumulator goes wrong"""
    X, key, S = wide_input()
    m = WIDE_CELLS
    assert S > 2 ** 63 - 1
    eng.ensure_expression(X)
    s_lo, s_hi, tie_gene, tie_key, got_m, nan = eng.gene_rank_corr(key[None, :])
    want_lo, want_hi = limbs(np.array([[S, -S]], dtype=object))
    assert got_m == m and not nan.any() and tie_gene.tolist() == [0.0, 0.0] and tie_key.tolist() == [0.0]
    np.testing.assert_array_equal(s_hi, want_hi)
    np.testing.assert_array_equal(s_lo, want_lo)
    assert s_hi.tolist() == [[0, -1]]
    from cna_amd.tools._gene_rank_corr import rank_corr_statistics
    np.testing.assert_array_equal(rank_corr_statistics(s_lo, s_hi, tie_gene, tie_key, got_m, nan), [[1.0, -1.0]])
    eng.drop_expression()


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f32'])
def test_no_kept_cell_and_one_kept_cell(eng, form):
    from cna_amd.tools._gene_rank_corr import rank_corr_statistics
    eng.ensure_expression(core_input(form))
    for keep in (0, 1):
        V = np.full((2, N_CORE), np.nan)
        V[0, :keep + 3] = 1.0
        V[1, 3:] = 2.0                                                        # the keys share `keep` cells
        got = eng.gene_rank_corr(V)
        assert got[4] == keep and np.isnan(rank_corr_statistics(*got)).all()


# ------------------------------------------------------------------ residency
def test_no_resident_matrix_is_refused_and_drop_frees_the_buffers(eng):
    from cna_amd import _ffi
    eng.unpin_expression()
    eng.drop_expression()
    base = eng.device_bytes()
    m = np.zeros(1, dtype=np.int64)
    out = [np.zeros((1, 1), dtype=np.uint64), np.zeros((1, 1), dtype=np.int64), np.zeros(1), np.zeros(1)]
    V, nan = np.zeros((1, 10)), np.zeros(1, dtype=np.uint8)
    rc = eng.lib.cna_gene_rank_corr(eng.h, _ffi.ptr(V), 1, 0, *[_ffi.ptr(a) for a in out], m.ctypes.data_as(_ffi.c_i64p),
                                    _ffi.ptr(nan))
    assert rc == -4 and b'no expression matrix' in eng.lib.cna_last_error()  # CNA_ESTATE
    for form in ('dense-f64', 'csr-f32'):
        eng.ensure_expression(core_input(form))
        eng.gene_rank_corr(core_keys())
        assert eng.device_bytes() > base
        eng.drop_expression()                       # the work buffers go with the matrix
        assert eng.device_bytes() == base


# ------------------------------------------------------------------ end to end
def test_gene_rank_corr_against_spearmanr(eng):
    import cna_amd as cna
    d = markers_input()
    d.obs['coef'], d.obs['score'] = end_to_end_keys(len(d.obs))
    out = cna.tl.gene_rank_corr(d, ['coef', 'score'], key_added='rho_', engine=eng)
    kept = np.isfinite(d.obs['coef'].values) & np.isfinite(d.obs['score'].values)
    assert out.shape == (6, 2) and out.attrs['n_cells'] == int(kept.sum()) < len(kept)
    Xd = d.X.astype(np.float64)
    for k in ('coef', 'score'):
        for g in range(6):
            want = scipy.stats.spearmanr(Xd[kept, g], d.obs[k].values[kept]).statistic
            print('%s gene %d: rho %.12f scipy %.12f' % (k, g, out[k].iloc[g], want))
            assert abs(out[k].iloc[g] - want) <= RHO_TOL
        np.testing.assert_array_equal(d.var['rho_' + k].values, out[k].values)
