"""cna.tl.gene_markers / cna_gene_ranksum_by on the device (run with -m gpu on an MI355X).

The device returns integers (twice the rank sums, the cells per level, the NaN flags) and a tie term that is an integer below
2^53 on every shape here, so everything is compared with assert_array_equal against the numpy / scipy restatement of
tests/test_gene_markers_host.py, which that file checks against scipy.stats.mannwhitneyu on these same inputs.  It also
proves what the inputs reach: three sort chunks per long gene, two tiles under SMALL_WORK_BYTES, tie runs on and across the
cuts of the rank kernel's unit."""
import numpy as np
import pandas as pd
import pytest
import scipy.stats

from test_gene_markers_host import (FORMS, CORE_LEVELS, N_CORE, SMALL_WORK_BYTES, MID, P_RTOL, Z_MAX, core_codes, core_input,
                                    core_reference, core_values, sparse_of, mid_input, markers_input, restated_ranksum)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()


def _equal(name, got, want):
    """rank2, tie, n, nan against the restatement; the numbers of a flagged gene are unspecified"""
    ok = ~want[3]
    np.testing.assert_array_equal(got[3], want[3], err_msg=name + ' nan')
    np.testing.assert_array_equal(got[2], want[2], err_msg=name + ' n')
    np.testing.assert_array_equal(got[0][:, ok], want[0][:, ok], err_msg=name + ' rank2')
    np.testing.assert_array_equal(got[1][ok], want[1][ok], err_msg=name + ' tie')
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[2].dtype == np.int64 and got[3].dtype == bool


def _same_bits(a, b, ok=slice(None)):
    np.testing.assert_array_equal(a[0][:, ok], b[0][:, ok])
    np.testing.assert_array_equal(a[1][ok].view(np.int64), b[1][ok].view(np.int64))
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])


def _run(eng, form, which='core', work_bytes=0):
    eng.ensure_expression(core_input(form))
    L = {'core': CORE_LEVELS, 'one': 1, '1024': 1024}[which]
    return eng.gene_ranksum_by(core_codes(which), L, work_bytes)


# ------------------------------------------------------------------ the nine genes, four forms
@pytest.mark.parametrize('form', FORMS)
def test_core_case_equals_the_restatement(eng, form):
    got = _run(eng, form)
    assert eng.expression_shape()['format'] == ('dense' if form.startswith('dense') else 'gene-major')
    assert eng.expression_shape()['f64'] == form.endswith('f64')
    want = core_reference(form)
    _equal(form, got, want)
    n, m = want[2], int(want[2].sum())
    np.testing.assert_array_equal(got[0][:, 2], n * (m + 1))                 # the constant gene, one run across every cut
    assert list(np.flatnonzero(got[3])) == [7]                               # the kept NaN; the left-out one sets nothing
    # under the small budget (two tiles at least; float64: a gene that alone exceeds it) the same bits
    _same_bits(eng.gene_ranksum_by(core_codes(), CORE_LEVELS, SMALL_WORK_BYTES), got, ~want[3])
    _same_bits(eng.gene_ranksum_by(core_codes(), CORE_LEVELS), got, ~want[3])          # and on a second run


@pytest.mark.parametrize('which', ['one', '1024'])
@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_one_level_and_1024_levels(eng, form, which):
    got = _run(eng, form, which)
    _equal('%s %s' % (form, which), got, core_reference(form, which))
    if which == 'one':
        from cna_amd.tools._gene_markers import ranksum_statistics
        assert np.isnan(ranksum_statistics(*got)).all()                       # the level holds every kept cell


def test_uploads_of_one_matrix_agree(eng):
    """CSR and CSC of one matrix: the same bits; its dense upload: equal integers"""
    V, S = core_values()
    codes = core_codes()
    out = {}
    for fmt, idx in (('csr', np.int32), ('csc', np.int64)):
        eng.ensure_expression(sparse_of(V, S, fmt, np.float64, idx))
        out[fmt] = eng.gene_ranksum_by(codes, CORE_LEVELS)
    ok = ~out['csr'][3]
    _same_bits(out['csr'], out['csc'], ok)
    eng.ensure_expression(np.ascontiguousarray(V))
    _same_bits(eng.gene_ranksum_by(codes, CORE_LEVELS), out['csr'], ok)


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f32'])
def test_neighbours_on_the_expression_stream_change_no_bit(eng, form):
    X, codes = core_input(form), core_codes()
    V = np.where(codes >= 0, np.arange(N_CORE) % 13 - 6.0, np.nan)[None, :]
    eng.ensure_expression(X)
    first = eng.gene_ranksum_by(codes, CORE_LEVELS)
    bins = eng.expr_to_bins(codes, CORE_LEVELS, 0)
    corr = eng.gene_corr_by(V, codes, CORE_LEVELS)
    second = eng.gene_ranksum_by(codes, CORE_LEVELS)
    _same_bits(first, second, ~first[3])
    for a, b in zip(bins, eng.expr_to_bins(codes, CORE_LEVELS, 0)):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(corr, eng.gene_corr_by(V, codes, CORE_LEVELS)):
        np.testing.assert_array_equal(a, b)


def test_mid_size_case_equals_the_restatement(eng):
    X, codes = mid_input()
    n, G, L = MID
    eng.ensure_expression(X)
    got = eng.gene_ranksum_by(codes, L)
    want = restated_ranksum(X, codes, L)
    assert not want[3].any() and want[1].max() < 2.0 ** 53
    _equal('200001 x 48', got, want)


# ------------------------------------------------------------------ refusals and residency
@pytest.mark.parametrize('form', ['csr-f32', 'dense-f32'])
def test_bad_codes_are_refused_and_nothing_is_written(eng, form):
    from cna_amd import _ffi
    want = core_reference(form)
    _equal(form + ' before', _run(eng, form), want)
    for bad_value in (CORE_LEVELS, -2):
        bad = core_codes().copy()
        bad[N_CORE // 2] = bad_value
        rank2 = np.full((CORE_LEVELS, 9), -77, dtype=np.int64)
        tie = np.full(9, -77.0)
        n = np.full(CORE_LEVELS, -77, dtype=np.int64)
        nan = np.full(9, 77, dtype=np.uint8)
        rc = eng.lib.cna_gene_ranksum_by(eng.h, _ffi.ptr(bad), CORE_LEVELS, 0, _ffi.ptr(rank2), _ffi.ptr(tie), _ffi.ptr(n),
                                         _ffi.ptr(nan))
        assert rc == -1 and b'outside' in eng.lib.cna_last_error()           # CNA_EINVAL
        assert (rank2 == -77).all() and (tie == -77.0).all() and (n == -77).all() and (nan == 77).all()
        with pytest.raises(_ffi.CnaHipError, match='outside'):
            eng.gene_ranksum_by(bad, CORE_LEVELS)
    for levels in (0, 1025):
        with pytest.raises(_ffi.CnaHipError, match='1024'):
            eng.gene_ranksum_by(core_codes(), levels)
    with pytest.raises(ValueError):
        eng.gene_ranksum_by(core_codes()[:-1], CORE_LEVELS)
    _equal(form + ' after', eng.gene_ranksum_by(core_codes(), CORE_LEVELS), want)


def test_no_resident_matrix_is_refused_and_drop_frees_the_buffers(eng):
    from cna_amd import _ffi
    eng.unpin_expression()
    eng.drop_expression()
    base = eng.device_bytes()
    out = [np.zeros((1, 1), dtype=np.int64), np.zeros(1), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint8)]
    rc = eng.lib.cna_gene_ranksum_by(eng.h, _ffi.ptr(np.zeros(10, dtype=np.int32)), 1, 0, *[_ffi.ptr(a) for a in out])
    assert rc == -4 and b'no expression matrix' in eng.lib.cna_last_error()  # CNA_ESTATE
    for form in ('dense-f64', 'csr-f32'):
        _run(eng, form)
        assert eng.device_bytes() > base
        eng.drop_expression()                       # the work buffers go with the matrix
        assert eng.device_bytes() == base


# ------------------------------------------------------------------ end to end
def test_gene_markers_against_mannwhitneyu(eng):
    import cna_amd as cna
    d = markers_input()
    out = cna.tl.gene_markers(d, 'pop', engine=eng)
    codes, levels = pd.factorize(d.obs['pop'])
    assert out.shape == (6, 27) and list(out.columns.get_level_values(0)[::9]) == list(levels)
    Xd = d.X.astype(np.float64)
    m = int((codes >= 0).sum())
    for b, l in enumerate(levels):
        ins, rest = codes == b, (codes >= 0) & (codes != b)
        nb = int(ins.sum())
        for g in range(6):
            x, y = Xd[ins, g], Xd[rest, g]
            res = scipy.stats.mannwhitneyu(x, y, use_continuity=False, method='asymptotic')
            t = np.unique(np.r_[x, y], return_counts=True)[1].astype(np.float64)
            sd = np.sqrt(nb * (m - nb) / 12.0 * ((m + 1) - (t ** 3 - t).sum() / (m * (m - 1.0))))
            z = (res.statistic - nb * (m - nb) / 2.0) / sd
            got = out[l].iloc[g]
            print('%s gene %d: u %.1f z %.6f p %.3e' % (l, g, got['u'], got['z'], got['p']))
            assert got['u'] == res.statistic
            assert abs(got['auc'] - res.statistic / (nb * (m - nb))) <= 1e-10
            assert abs(z) <= Z_MAX and abs(got['z'] - z) <= 1e-10
            assert abs(got['p'] - res.pvalue) <= P_RTOL * res.pvalue
        np.testing.assert_allclose(out[(l, 'mean_in')].values, Xd[ins].mean(axis=0), rtol=1e-10)
        np.testing.assert_allclose(out[(l, 'frac_rest')].values, (Xd[rest] > 0).mean(axis=0), rtol=1e-10)
