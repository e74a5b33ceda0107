"""cna.tl.gene_markers_pairs / cna_gene_ranksum_pairs on the device (run with -m gpu on an MI355X).

The device returns integers (twice the U of every pair, the cells per level, the NaN flags) and a tie term that is an integer
below 2^53 on every shape here, so everything is compared with assert_array_equal against the numpy restatement of
tests/test_gene_markers_pairs_host.py, which that file checks against scipy on these same inputs and which proves what they
reach (a tie run on a cut of the kernel's unit, one across two cuts, for the levels of the tested pairs)."""
import functools

import numpy as np
import pytest

from test_gene_markers_host import (FORMS, CORE_LEVELS, N_CORE, SMALL_WORK_BYTES, MID, core_codes, core_input, core_values,
                                    sparse_of, mid_input, markers_input)
from test_gene_markers_pairs_host import CORE_PAIRS, PairsEngine, core_pairs_reference, restated_pairs

pytestmark = pytest.mark.gpu

CORE_IDX = np.array(CORE_PAIRS, dtype=np.int32)


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()


def _equal(name, got, want):
    """u2, tie, n, nan against the restatement; the numbers of a flagged gene are unspecified"""
    ok = ~want[3]
    np.testing.assert_array_equal(got[3], want[3], err_msg=name + ' nan')
    np.testing.assert_array_equal(got[2], want[2], err_msg=name + ' n')
    np.testing.assert_array_equal(got[0][:, ok], want[0][:, ok], err_msg=name + ' u2')
    np.testing.assert_array_equal(got[1][:, ok], want[1][:, ok], err_msg=name + ' tie')
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[2].dtype == np.int64 and got[3].dtype == bool


def _same_bits(a, b, ok=slice(None)):
    np.testing.assert_array_equal(a[0][:, ok], b[0][:, ok])
    np.testing.assert_array_equal(a[1][:, ok].view(np.int64), b[1][:, ok].view(np.int64))
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])


# ------------------------------------------------------------------ the nine genes, four forms, all 12 ordered pairs
@pytest.mark.parametrize('form', FORMS)
def test_core_case_equals_the_restatement(eng, form):
    eng.ensure_expression(core_input(form))
    got = eng.gene_ranksum_pairs(core_codes(), CORE_LEVELS, CORE_IDX)
    want = core_pairs_reference(form.endswith('f64'))
    _equal(form, got, want)
    assert list(np.flatnonzero(got[3])) == [7]                               # the kept NaN; the left-out one sets nothing
    # under the small budget (two tiles of genes at least) the same bits, and on a second run
    _same_bits(eng.gene_ranksum_pairs(core_codes(), CORE_LEVELS, CORE_IDX, SMALL_WORK_BYTES), got, ~want[3])
    _same_bits(eng.gene_ranksum_pairs(core_codes(), CORE_LEVELS, CORE_IDX), got, ~want[3])


def test_uploads_of_one_matrix_agree(eng):
    """CSR and CSC of one matrix: the same bits; its dense upload: equal integers"""
    V, S = core_values()
    out = {}
    for fmt, idx in (('csr', np.int32), ('csc', np.int64)):
        eng.ensure_expression(sparse_of(V, S, fmt, np.float64, idx))
        out[fmt] = eng.gene_ranksum_pairs(core_codes(), CORE_LEVELS, CORE_IDX)
    ok = ~out['csr'][3]
    _same_bits(out['csr'], out['csc'], ok)
    eng.ensure_expression(np.ascontiguousarray(V))
    _same_bits(eng.gene_ranksum_pairs(core_codes(), CORE_LEVELS, CORE_IDX), out['csr'], ok)


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_the_route_of_the_level_call_gives_the_same(eng, form):
    """what was there before, on the device: a -> 0, b -> 1, the rest -> -1 and one cna_gene_ranksum_by per pair"""
    codes = core_codes()
    eng.ensure_expression(core_input(form))
    asked = [(0, 1), (2, 0), (1, 2)]
    u2, tie, n, nan = eng.gene_ranksum_pairs(codes, CORE_LEVELS, np.array(asked, dtype=np.int32))
    ok = ~nan
    for k, (a, b) in enumerate(asked):
        two = np.where(codes == a, 0, np.where(codes == b, 1, -1)).astype(np.int32)
        rank2, tie1, n1, nan1 = eng.gene_ranksum_by(two, 2)
        assert list(n1) == [n[a], n[b]]
        np.testing.assert_array_equal(rank2[0][ok] - n[a] * (n[a] + 1), u2[k][ok])
        np.testing.assert_array_equal(tie1[ok].view(np.int64), tie[k][ok].view(np.int64))


ALL_64 = [(a, b) for a in range(64) for b in range(a + 1, 64)]


@functools.lru_cache(maxsize=None)
def reference_64(f64):
    V, _ = core_values()
    return restated_pairs(V.astype(np.float64 if f64 else np.float32), codes_64(), 64, ALL_64)


def codes_64():
    return np.where(core_codes() >= 0, np.arange(N_CORE) * 7 % 64, -1).astype(np.int32)


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_64_levels_and_2016_pairs(eng, form):
    """the level cap, the pair cap and every accumulator slot"""
    assert len(ALL_64) == 2016
    eng.ensure_expression(core_input(form))
    got = eng.gene_ranksum_pairs(codes_64(), 64, np.array(ALL_64, dtype=np.int32))
    _equal(form + ' 64 levels', got, reference_64(form.endswith('f64')))


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_a_pair_with_the_empty_level(eng, form):
    from cna_amd.tools._gene_markers import pair_statistics
    eng.ensure_expression(core_input(form))
    asked = np.array([(1, 3), (3, 1)], dtype=np.int32)
    u2, tie, n, nan = eng.gene_ranksum_pairs(core_codes(), CORE_LEVELS, asked)
    ok = ~nan
    assert n[3] == 0 and n[1] > 0 and (u2[:, ok] == 0).all()
    # the tie term of level 1 alone: that of a call whose kept cells are level 1 (one level against the rest)
    only = np.where(core_codes() == 1, 0, -1).astype(np.int32)
    alone = eng.gene_ranksum_by(only, 1)[1]
    np.testing.assert_array_equal(tie[0][ok], alone[ok])
    np.testing.assert_array_equal(tie[1][ok], alone[ok])
    assert np.isnan(pair_statistics(u2, tie, n, nan, asked)).all()


@pytest.mark.parametrize('sparse', [False, True])
def test_short_runs_across_a_cut(eng, sparse):
    """Runs below the length the kernel hands to the whole workgroup (RP_BIG), between distinct values: one of 4 entries
    across the first cut of the unit, one of RP_BIG - 1 across the second, one of 2 that ends on the third; the thread at
    the run's tail reads the counts at a start that lies in the unit before."""
    import scipy.sparse as sp
    from test_gene_markers_host import ranksum_constant
    unit, big = ranksum_constant('RS_UNIT'), ranksum_constant('RP_BIG')
    n = 4 * unit + 37
    rs = np.random.RandomState(3)
    vals = np.arange(1, n + 1, dtype=np.float64)                             # sorted position i holds i + 1: all stored
    for lo, hi in ((unit - 2, unit + 2), (2 * unit - 7, 2 * unit - 7 + big - 1), (3 * unit - 2, 3 * unit)):
        assert hi - lo < big and lo < hi - 1
        vals[lo:hi] = vals[lo]
    X = np.zeros((n, 2), dtype=np.float32)
    X[:, 0] = vals[rs.permutation(n)]
    X[:, 1] = -vals[rs.permutation(n)]                                       # the same below zero
    codes = rs.randint(0, 5, size=n).astype(np.int32)
    asked = [(a, b) for a in range(5) for b in range(5) if a != b]
    eng.ensure_expression(sp.csr_matrix(X) if sparse else X)
    got = eng.gene_ranksum_pairs(codes, 5, np.array(asked, dtype=np.int32))
    _equal('short runs', got, restated_pairs(X, codes, 5, asked))


def test_mid_size_case_equals_the_restatement(eng):
    X, codes = mid_input()
    n, G, L = MID
    asked = [(a, b) for a in range(L) for b in range(a + 1, L)]
    assert len(asked) == 496
    eng.ensure_expression(X)
    got = eng.gene_ranksum_pairs(codes, L, np.array(asked, dtype=np.int32))
    want = restated_pairs(X, codes, L, asked)
    assert not want[3].any() and 1e13 < want[1].max() < 2.0 ** 53
    _equal('200001 x 48', got, want)


# ------------------------------------------------------------------ refusals and residency
def _raw(eng, codes, n_bins, pairs, n_pairs, work_bytes=0):
    """the raw ABI on buffers filled with a mark: (rc, the four buffers)"""
    from cna_amd import _ffi
    P = max(n_pairs, 1)
    out = [np.full((min(P, 2017), 9), -77, dtype=np.int64), np.full((min(P, 2017), 9), -77.0),
           np.full(max(n_bins, 1), -77, dtype=np.int64), np.full(9, 77, dtype=np.uint8)]
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    rc = eng.lib.cna_gene_ranksum_pairs(eng.h, _ffi.ptr(codes), n_bins, _ffi.ptr(pairs), n_pairs, work_bytes,
                                        *[_ffi.ptr(a) for a in out])
    return rc, out


def _untouched(out):
    return (out[0] == -77).all() and (out[1] == -77.0).all() and (out[2] == -77).all() and (out[3] == 77).all()


@pytest.mark.parametrize('form', ['csr-f32', 'dense-f32'])
def test_bad_arguments_are_refused_and_nothing_is_written(eng, form):
    from cna_amd import _ffi
    want = core_pairs_reference(False)
    codes = core_codes()
    eng.ensure_expression(core_input(form))
    _equal(form + ' before', eng.gene_ranksum_pairs(codes, CORE_LEVELS, CORE_IDX), want)
    bad_code = codes.copy()
    bad_code[N_CORE // 2] = CORE_LEVELS
    low_code = codes.copy()
    low_code[N_CORE // 2] = -2
    long_list = np.tile(CORE_IDX, (169, 1))[:2017]
    cases = [('outside [0, n_bins)', codes, CORE_LEVELS, [(0, 1), (1, CORE_LEVELS)], 2, 0),
             ('outside [0, n_bins)', codes, CORE_LEVELS, [(-1, 1)], 1, 0),
             ('with itself', codes, CORE_LEVELS, [(0, 1), (2, 2)], 2, 0),
             ('n_pairs', codes, CORE_LEVELS, [(0, 1)], 0, 0),
             ('n_pairs', codes, CORE_LEVELS, long_list, 2017, 0),
             ('n_bins', codes, 0, [(0, 1)], 1, 0),
             ('n_bins', codes, 65, [(0, 1)], 1, 0),
             ('outside [-1, n_bins)', bad_code, CORE_LEVELS, CORE_IDX, 12, 0),
             ('outside [-1, n_bins)', low_code, CORE_LEVELS, CORE_IDX, 12, 0),
             ('work_bytes', codes, CORE_LEVELS, CORE_IDX, 12, -1)]
    for what, cd, n_bins, pairs, n_pairs, work_bytes in cases:
        rc, out = _raw(eng, cd, n_bins, pairs, n_pairs, work_bytes)
        msg = eng.lib.cna_last_error()
        assert rc == -1, (what, rc)                                           # CNA_EINVAL
        assert b'cna_gene_ranksum_pairs' in msg and what.encode() in msg, (what, msg)
        assert _untouched(out), what
        with pytest.raises(_ffi.CnaHipError, match='cna_gene_ranksum_pairs'):
            eng.gene_ranksum_pairs(cd, n_bins, np.asarray(pairs, dtype=np.int32).reshape(-1, 2)[:n_pairs], work_bytes)
        _equal(form + ' after ' + what, eng.gene_ranksum_pairs(codes, CORE_LEVELS, CORE_IDX), want)
    with pytest.raises(ValueError):
        eng.gene_ranksum_pairs(codes[:-1], CORE_LEVELS, CORE_IDX)
    with pytest.raises(ValueError):
        eng.gene_ranksum_pairs(codes, CORE_LEVELS, CORE_IDX.ravel())


def test_no_resident_matrix_is_refused_and_drop_frees_the_buffers(eng):
    eng.unpin_expression()
    eng.drop_expression()
    base = eng.device_bytes()
    rc, out = _raw(eng, np.zeros(10, dtype=np.int32), 2, [(0, 1)], 1)
    msg = eng.lib.cna_last_error()
    assert rc == -4 and b'cna_gene_ranksum_pairs' in msg and b'no expression matrix' in msg       # CNA_ESTATE
    assert _untouched(out)
    for form in ('dense-f64', 'csr-f32'):
        eng.ensure_expression(core_input(form))
        _equal(form, eng.gene_ranksum_pairs(core_codes(), CORE_LEVELS, CORE_IDX), core_pairs_reference(form.endswith('f64')))
        assert eng.device_bytes() > base
        eng.drop_expression()                       # the work buffers go with the matrix
        assert eng.device_bytes() == base


# ------------------------------------------------------------------ end to end
def test_the_public_call_equals_the_engine_double(eng):
    import cna_amd as cna
    d = markers_input()
    for kw in (dict(pairs=[('pos1', 'neg1'), ('neg1', 'pos1'), ('pos2', 'neg1')]), dict(reference='neg1'), dict(),
               dict(pairs=[('neg1', 'pos2')], tie_correct=False)):
        got = cna.tl.gene_markers_pairs(d, 'pop', engine=eng, **kw)
        want = cna.tl.gene_markers_pairs(d, 'pop', engine=PairsEngine(), **kw)
        assert got.columns.equals(want.columns) and got.index.equals(want.index)
        rank = got.columns.get_level_values(2).isin(['auc', 'u', 'z', 'p', 'q'])
        np.testing.assert_array_equal(got.values[:, rank], want.values[:, rank])       # from equal integers: equal floats
        np.testing.assert_allclose(got.values[:, ~rank], want.values[:, ~rank], rtol=1e-12)
        assert got.attrs['n_cells'].equals(want.attrs['n_cells'])
