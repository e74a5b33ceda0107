"""cna.tl.gene_rank_test_strata / cna_gene_rank_corr_x_by on the device (run with -m gpu on an MI355X).

The entry returns integers, and tie terms that are integers below 2^53 on every shape here: assert_array_equal against the
restatement of tests/test_gene_rank_perm_strata_host.py (checked there against scipy.stats.spearmanr) and against the
library itself -- per level cna_gene_rank_corr_x with xrow set to -1 outside the level, per group of 16 columns
cna_gene_rank_corr_by on the rows cna_x_columns forms.  End to end, rho against scipy within RHO_TOL, the project's figure.

Shapes: the nine core genes on 3001 cells in the four stored forms (three sort chunks per long gene, two tiles of genes at
least under SMALL_WORK_BYTES), 1 to 40 columns from X of 1 to 130 samples, nine levels that the host file proves to reach
empty and tiny levels, lost cells, tie runs on the boundary of two levels and on the cuts of the unit; 255 levels; and the
3.1M cells at which a level's sum passes 64 bits."""
import warnings

import numpy as np
import pytest
import scipy.stats

from test_gene_markers_host import FORMS, N_CORE, SMALL_WORK_BYTES, core_input, core_values
from test_gene_rank_corr_host import RHO_TOL, WIDE_CELLS, limbs, rank_corr_tiles, restated_rank_corr, wide_input
from test_gene_rank_corr_strata_host import as_engine_by, many_codes
from test_gene_rank_perm_host import COLUMN_COUNTS, COLUMN_SAMPLES, X_ROWS, column_case, restated_columns
from test_gene_rank_perm_strata_host import (PERM_LEVELS, case_columns, kept_levels, perm_strata_codes, perm_strata_reference,
                                             restated_rank_corr_x_by)
from test_gpu_gene_rank_corr import _equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()


def _equal_by(name, got, restated):
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


def _same_bits_by(a, b, ok=slice(None)):
    np.testing.assert_array_equal(a[0][:, :, ok], b[0][:, :, ok])
    np.testing.assert_array_equal(a[1][:, :, ok], b[1][:, :, ok])
    np.testing.assert_array_equal(a[2][:, ok].view(np.int64), b[2][:, ok].view(np.int64))
    np.testing.assert_array_equal(a[3].view(np.int64), b[3].view(np.int64))
    np.testing.assert_array_equal(a[4], b[4])
    np.testing.assert_array_equal(a[5], b[5])


def _level_equals(by, l, one, ok, cols=slice(None)):
    """level l (and the columns `cols`) of a per-level result against a whole-gene result, bit for bit over the genes `ok`;
    the flags are the whole call's on one side and the level's on the other, and are not compared"""
    np.testing.assert_array_equal(by[0][l][cols][:, ok], one[0][:, ok])
    np.testing.assert_array_equal(by[1][l][cols][:, ok], one[1][:, ok])
    np.testing.assert_array_equal(by[2][l][ok].view(np.int64), one[2][ok].view(np.int64))
    np.testing.assert_array_equal(by[3][l][cols].view(np.int64), one[3].view(np.int64))
    assert int(by[4][l]) == int(one[4])


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize('integer', [False, True])
@pytest.mark.parametrize('samples,q', list(zip(COLUMN_SAMPLES, COLUMN_COUNTS)))
@pytest.mark.parametrize('form', FORMS)
def test_every_level_equals_the_restatement(eng, form, samples, q, integer):
    X, xrow, Z = column_case(samples, q, integer)
    codes = perm_strata_codes(samples, q, integer)
    eng.ensure_expression(core_input(form))
    eng.upload_x(X)
    got = eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS)
    want = perm_strata_reference(form, samples, q, integer)
    assert got[0].shape == (PERM_LEVELS, q, 9) and got[2].shape == (PERM_LEVELS, 9) and got[3].shape == (PERM_LEVELS, q)
    _equal_by('%s %d x %d %s' % (form, samples, q, integer), got, want)
    kept = kept_levels(samples, q, integer)
    assert list(got[4]) == [int((kept == l).sum()) for l in range(PERM_LEVELS)]            # m per level, exactly
    cell7 = int(np.flatnonzero(np.isnan(core_values()[0][:, 7]))[0])
    assert list(np.flatnonzero(got[5])) == ([7] if kept[cell7] >= 0 else [])               # the known flagged gene


# ------------------------------------------------------------------ against the library itself
@pytest.mark.parametrize('samples,q,integer', [(33, 17, True), (130, 40, False)])
@pytest.mark.parametrize('form', FORMS)
def test_levels_equal_the_masked_route_and_groups_equal_the_entry_by_level(eng, form, samples, q, integer):
    X, xrow, Z = column_case(samples, q, integer)
    codes = perm_strata_codes(samples, q, integer)
    eng.ensure_expression(core_input(form))
    eng.upload_x(X)
    got = eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS)
    ok = ~got[5]
    for l in range(PERM_LEVELS):                       # cna_gene_rank_corr_x with xrow set to -1 outside the level
        _level_equals(got, l, eng.gene_rank_corr_x(np.where(codes == l, xrow, -1), Z), ok)
    V = eng.x_columns(xrow, Z)
    assert V.tobytes() == case_columns(samples, q, integer).tobytes()
    for k0 in range(0, q, 16):                         # cna_gene_rank_corr_by on the group's rows of cna_x_columns
        group = eng.gene_rank_corr_by(V[k0:k0 + 16], codes, PERM_LEVELS)
        np.testing.assert_array_equal(got[0][:, k0:k0 + 16][:, :, ok], group[0][:, :, ok])
        np.testing.assert_array_equal(got[1][:, k0:k0 + 16][:, :, ok], group[1][:, :, ok])
        np.testing.assert_array_equal(got[2][:, ok].view(np.int64), group[2][:, ok].view(np.int64))
        np.testing.assert_array_equal(got[3][:, k0:k0 + 16].view(np.int64), group[3].view(np.int64))
        np.testing.assert_array_equal(got[4], group[4])
        np.testing.assert_array_equal(got[5], group[5])


# ------------------------------------------------------------------ limits and invariances
@pytest.mark.parametrize('form', ['csr-f32', 'dense-f64'])
def test_the_level_limit(eng, form):
    X, xrow, Z = column_case(3, 16)
    codes = many_codes(255)
    eng.ensure_expression(core_input(form))
    eng.upload_x(X)
    got = eng.gene_rank_corr_x_by(xrow, Z, codes, 255)
    Vg, _ = core_values()
    want = restated_rank_corr_x_by(Vg.astype(np.float32 if form.endswith('f32') else np.float64), case_columns(3, 16), xrow, codes,
                                   255)
    _equal_by(form + ' 255 levels', got, want)
    assert (got[4] == 0).any() and got[4][254] > 0


@pytest.mark.parametrize('form', FORMS)
def test_one_level_of_every_kept_cell_is_the_plain_entry(eng, form):
    X, xrow, Z = column_case(33, 17, True)
    eng.ensure_expression(core_input(form))
    eng.upload_x(X)
    plain = eng.gene_rank_corr_x(xrow, Z)
    got = eng.gene_rank_corr_x_by(xrow, Z, np.zeros(N_CORE, dtype=np.int32), 1)
    _level_equals(got, 0, plain, ~plain[5])
    np.testing.assert_array_equal(got[5], plain[5])
    assert got[4].tolist() == [X_ROWS]


@pytest.mark.parametrize('form', FORMS)
def test_the_small_budget_a_rerun_and_the_chunks_give_the_same_bits(eng, form, monkeypatch):
    samples, q, integer = 130, 40, False
    X, xrow, Z = column_case(samples, q, integer)
    codes = perm_strata_codes(samples, q, integer)
    eng.ensure_expression(core_input(form))
    eng.upload_x(X)
    got = eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS)
    ok = ~got[5]
    assert len(rank_corr_tiles(form, SMALL_WORK_BYTES)[0]) >= 2
    _same_bits_by(eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS, SMALL_WORK_BYTES), got, ok)
    _same_bits_by(eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS), got, ok)
    # the engine's chunks, one group of 16 columns per library call: three calls here
    from cna_amd import engine as engine_module
    assert engine_module.RANK_X_BY_HOST_BYTES == 1 << 30
    monkeypatch.setattr(engine_module, 'RANK_X_BY_HOST_BYTES', 16 * 16 * PERM_LEVELS * 9)
    _same_bits_by(eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS), got, ok)


# ------------------------------------------------------------------ the entries beside it are as they were
def test_the_plain_entries_and_x_are_untouched(eng):
    samples, q, integer = 33, 17, True
    X, xrow, Z = column_case(samples, q, integer)
    V = case_columns(samples, q, integer)
    codes = perm_strata_codes(samples, q, integer)
    form = 'csc-f64'
    eng.ensure_expression(core_input(form))
    eng.upload_x(X)
    gen = eng.x_generation()
    want = restated_rank_corr(core_values()[0], V)
    _equal(form + ' x before', eng.gene_rank_corr_x(xrow, Z), want)
    eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS)
    _equal(form + ' x behind the call by level', eng.gene_rank_corr_x(xrow, Z), want)
    _equal(form + ' wide behind the call by level', eng.gene_rank_corr_wide(V), want)
    assert eng.x_generation() == gen                                             # X is read only
    assert np.array_equal(eng.x_full(), X)                                       # ... and as it was


# ------------------------------------------------------------------ refusals, nothing written
def _raw(eng, q, xrow, Z, codes, n_bins, work_bytes=0, null=None, G=9, rows=48, levels=16):
    """(status, untouched, message) of a raw call with pre-filled outputs; `null`: the argument passed as a null pointer"""
    from cna_amd._ffi import ptr
    s_lo = np.full((levels, rows, G), 77, dtype=np.uint64)
    s_hi = np.full((levels, rows, G), -77, dtype=np.int64)
    tie_gene, tie_key = np.full((levels, G), -77.0), np.full((levels, rows), -77.0)
    m = np.full(256, -77, dtype=np.int64)
    nan = np.full(G, 77, dtype=np.uint8)
    args = dict(xrow=ptr(xrow), Z=ptr(Z), codes=ptr(codes), s_lo=ptr(s_lo), s_hi=ptr(s_hi), tie_gene=ptr(tie_gene),
                tie_key=ptr(tie_key), m=ptr(m), nan=ptr(nan))
    if null:
        args[null] = None
    rc = eng.lib.cna_gene_rank_corr_x_by(eng.h, args['xrow'], len(xrow), args['Z'], q, args['codes'], n_bins, work_bytes,
                                         args['s_lo'], args['s_hi'], args['tie_gene'], args['tie_key'], args['m'], args['nan'])
    untouched = ((s_lo == 77).all() and (s_hi == -77).all() and (tie_gene == -77.0).all() and (tie_key == -77.0).all()
                 and (m == -77).all() and (nan == 77).all())
    return rc, untouched, eng.lib.cna_last_error()


def test_bad_arguments_are_refused_and_the_library_stays_usable(eng):
    samples, q, integer = 3, 16, False
    X, xrow, Z = column_case(samples, q, integer)
    codes = np.array(perm_strata_codes(samples, q, integer))
    xrow = np.array(xrow)
    Zbig = np.ascontiguousarray(np.tile(Z, (257, 1))[:4097])
    eng.ensure_expression(core_input('csr-f32'))
    eng.upload_x(X)
    good = eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS)

    def still_good():
        _same_bits_by(eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS), good, ~good[5])

    bad = codes.copy()
    bad[5] = PERM_LEVELS                                               # a code equal to n_bins
    rc, untouched, msg = _raw(eng, q, xrow, Z, bad, PERM_LEVELS)
    assert rc == -1 and untouched and b'a code lies outside [-1, n_bins)' in msg and msg.startswith(b'cna_gene_rank_corr_x_by')
    still_good()
    bad[5] = -2
    rc, untouched, msg = _raw(eng, q, xrow, Z, bad, PERM_LEVELS)
    assert rc == -1 and untouched and b'a code lies outside' in msg
    for n_bins in (0, 256, -1):
        rc, untouched, msg = _raw(eng, q, xrow, Z, np.zeros(N_CORE, dtype=np.int32), n_bins)
        assert rc == -1 and untouched and b'1 <= n_bins <= 255' in msg, n_bins                # CNA_EINVAL
    still_good()
    for bad_q in (0, 4097, -1):
        rc, untouched, msg = _raw(eng, bad_q, xrow, Zbig, codes, PERM_LEVELS)
        assert rc == -1 and untouched and b'1 <= q <= 4096' in msg, bad_q
    still_good()
    for null in ('xrow', 'Z', 'codes', 's_lo', 's_hi', 'tie_gene', 'tie_key', 'm', 'nan'):
        rc, untouched, msg = _raw(eng, q, xrow, Z, codes, PERM_LEVELS, null=null)
        assert rc == -1 and untouched and b'null pointer' in msg, null
    rc, untouched, msg = _raw(eng, q, xrow, Z, codes, PERM_LEVELS, work_bytes=-5)
    assert rc == -1 and untouched and b'work_bytes' in msg
    rc, untouched, msg = _raw(eng, q, xrow[:-1].copy(), Z, codes, PERM_LEVELS)                # another length than the matrix' cells
    assert rc == -1 and untouched and b'3000 entries' in msg
    twice = xrow.copy()
    twice[np.flatnonzero(xrow < 0)[0]] = xrow[np.flatnonzero(xrow >= 0)[40]]
    rc, untouched, msg = _raw(eng, q, twice, Z, codes, PERM_LEVELS)
    assert rc == -1 and untouched and b'two cells name the same row of X' in msg
    Zi = np.array(Z)
    Zi[15, 2] = np.inf                                                 # a formed value that is not finite
    rc, untouched, msg = _raw(eng, q, xrow, Zi, codes, PERM_LEVELS)
    assert rc == -1 and untouched and b'not finite' in msg and msg.startswith(b'cna_gene_rank_corr_x_by')
    with pytest.raises(ValueError):
        eng.gene_rank_corr_x_by(xrow, Z, codes[:-1], PERM_LEVELS)
    still_good()


def test_no_resident_matrix_is_an_estate_error(eng):
    X, xrow, Z = column_case(3, 16)
    codes = np.array(perm_strata_codes(3, 16))
    eng.upload_x(X)
    eng.drop_expression()
    rc, untouched, msg = _raw(eng, 16, np.array(xrow), Z, codes, PERM_LEVELS)
    assert rc == -4 and untouched and b'no expression matrix' in msg                      # CNA_ESTATE
    eng.ensure_expression(core_input('csr-f32'))
    _equal_by('behind the refusal', eng.gene_rank_corr_x_by(xrow, Z, codes, PERM_LEVELS), perm_strata_reference('csr-f32', 3, 16))


# ------------------------------------------------------------------ the 128-bit path
def test_a_level_whose_sum_passes_64_bits(eng):
    """3 100 000 cells in two levels, all but five cells and five cells; X one sample holding the key, Z = [[1]]: S of a
    level is +-(m_l^3 - m_l) / 3, in both limbs for the large one"""
    Xe, key, _ = wide_input()
    m = WIDE_CELLS
    codes = np.zeros(m, dtype=np.int32)
    codes[[7, 1000, 200000, 3000000, m - 1]] = 1
    sizes = [m - 5, 5]
    S = [(v ** 3 - v) // 3 for v in sizes]
    assert S[0] > 2 ** 63 - 1 and S[1] == 40
    eng.ensure_expression(Xe)
    eng.upload_x(key[:, None])
    s_lo, s_hi, tie_gene, tie_key, got_m, nan = eng.gene_rank_corr_x_by(np.arange(m, dtype=np.int64), np.array([[1.0]]), codes, 2)
    want_lo, want_hi = limbs(np.array([[S[0], -S[0]], [S[1], -S[1]]], dtype=object))
    assert got_m.tolist() == sizes and not nan.any() and not tie_gene.any() and not tie_key.any()
    np.testing.assert_array_equal(s_hi[:, 0, :], want_hi)
    np.testing.assert_array_equal(s_lo[:, 0, :], want_lo)
    assert s_hi[:, 0, :].tolist() == [[0, -1], [0, -1]]
    eng.drop_expression()


# ------------------------------------------------------------------ end to end
def test_end_to_end_on_a_synthetic_dataset(eng):
    import cna_amd as cna
    from cna_amd.tools._gene_null import null_phenotypes
    from test_gpu_gene_test import dataset, expression
    data, y, batches, covs = dataset('qc')
    call = dict(nsteps=3, Nnull=40, seed=3)
    E = expression(3000, 12, seed=12)
    rs = np.random.RandomState(5)
    lab = np.array(['b', 'a'], dtype=object)[rs.choice(2, size=3000, p=[0.4, 0.6])]
    lab[rs.rand(3000) < 0.04] = None
    d = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        d0 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'])
        p0 = cna.tl.association(d0, y, 'id', batches=batches, covs=covs, engine=eng, **call)
    kept = np.isfinite(d0.obs['coef'].values)
    assert (~kept).any()
    lab[np.flatnonzero(kept)[[100, 900, 2000]]] = 'tiny'               # three kept cells
    d.obs['cluster'] = lab
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        frame, null_rho = cna.tl.gene_rank_test_strata(d, y, 'id', 'cluster', batches=batches, covs=covs, n_perm=33, return_null=True,
                                                       engine=eng, **call)
        xrow = eng.x_row_of_cells()
        Xk = eng.x_full()
        Zall = null_phenotypes(type(data)(data.obs[['id']].copy(), data.obsp['connectivities']), y, 'id', batches, covs, None, 'coef',
                               eng, dict(call), 'test')[1]
        plain = cna.tl.gene_rank_corr_strata(d, 'cluster', 'coef', engine=eng)
    levels = list(frame.attrs['n_cells'].index)
    assert sorted(levels) == ['a', 'b', 'tiny'] and null_rho.shape == (3, 12, 33) and frame.shape == (12, 18)
    assert frame.attrs['p'] == p0 and frame.attrs['n_null'] == 33 and int(frame.attrs['n_cells']['tiny']) == 3
    assert np.array_equal(xrow >= 0, kept) and Xk.shape[0] == int(kept.sum())
    for k in ('coef', 'coef_fdr'):
        assert d.obs[k].values.tobytes() == d0.obs[k].values.tobytes(), k
    cols = np.full((3, 3000), np.nan)
    cols[:, kept] = restated_columns(Xk, np.arange(Xk.shape[0]), np.ascontiguousarray(Zall[:, 1:].T)[[0, 16, 32]])
    coef = d.obs['coef'].values
    worst_rho = worst_null = 0.0
    for l, lev in enumerate(levels):
        cells = kept & (lab == lev)
        assert int(frame.attrs['n_cells'][lev]) == int(cells.sum())
        rho = frame[(lev, 'rho')].values
        assert rho.tobytes() == plain[lev].values.tobytes()            # gene_rank_corr_strata, bit for bit
        for g in range(12):
            x = E[cells, g]
            if np.ptp(x) == 0:
                assert np.isnan(frame[lev].values[g]).all() and np.isnan(null_rho[l, g]).all()
                continue
            worst_rho = max(worst_rho, abs(rho[g] - scipy.stats.spearmanr(x, coef[cells]).statistic))
            for j, p in enumerate((0, 16, 32)):
                worst_null = max(worst_null, abs(null_rho[l, g, p] - scipy.stats.spearmanr(x, cols[j, cells]).statistic))
        nulls = null_rho[l]
        p = (1.0 + (np.abs(nulls) >= np.abs(rho)[:, None]).sum(axis=1)) / 34.0
        p[np.isnan(rho)] = np.nan
        assert np.array_equal(frame[(lev, 'p')].values, p, equal_nan=True)
    print('end to end: rho and null_rho against scipy.stats.spearmanr: max |d rho| = %.3e, %.3e' % (worst_rho, worst_null))
    assert worst_rho <= RHO_TOL and worst_null <= RHO_TOL
    assert np.isnan(frame[('a', 'rho')].values[1]) and np.isfinite(frame[('a', 'rho')].values[[0, 2, 11]]).all()
