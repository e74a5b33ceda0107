"""The rank entries on the device at the cell, gene and list counts csrc/rank_sort.h branches on (run with -m gpu on an
MI355X): cna_gene_ranksum_by, _pairs, _within, cna_gene_rank_corr, _by, _wide, _x and cna_x_columns on the inputs of
tests/rank_shapes.py.

Every result is an integer, or a double that holds one (each test asserts that the largest tie term lies below 2^53), so
everything is compared with assert_array_equal against the restatements of the entries' own host files, which
tests/test_rank_shapes_host.py holds to scipy.stats.mannwhitneyu, rankdata and spearmanr on these same inputs; the two
weighted sums of cna_gene_ranksum_within and the columns of cna_x_columns are compared bit for bit, as their own tests do.
The numbers of a gene flagged for a kept NaN are unspecified and left out, as in those tests.

  a  130 cells by 64, 65 and 130 dense genes: a second and third RS_TILE block of genes, tiles of genes [0, 70) and
     [70, 130), and every gene a tile of its own
  b  1 ... 2049 cells in three stored forms: lists that are a whole number of walk units or of sort chunks, and one more or less
  c  a gene that keeps 0, 1, 255 ... 512 of its stored entries, the others' keys all ones behind them
  d  the columns formed from X at 1, 255 ... 1025 cells"""
import numpy as np
import pytest

import rank_shapes as rs
from test_gene_rank_corr_host import limbs, restated_rank_corr
from test_gpu_gene_markers import _equal as by_equal, _same_bits as by_same_bits
from test_gpu_gene_markers_pairs import _equal as pairs_equal, _same_bits as pairs_same_bits
from test_gpu_gene_markers_within import _equal as within_equal, _same_bits as within_same_bits
from test_gpu_gene_rank_corr import _equal as corr_equal, _same_bits as corr_same_bits
from test_gpu_gene_rank_corr_strata import _equal as corr_by_equal, _same_bits as corr_by_same_bits

pytestmark = pytest.mark.gpu

EQUAL = {'ranksum_by': by_equal, 'ranksum_pairs': pairs_equal, 'ranksum_within': within_equal, 'rank_corr': corr_equal,
         'rank_corr_by': corr_by_equal, 'rank_corr_wide': corr_equal}
SAME_BITS = {'ranksum_by': by_same_bits, 'ranksum_pairs': pairs_same_bits, 'ranksum_within': within_same_bits,
             'rank_corr': corr_same_bits, 'rank_corr_by': corr_by_same_bits, 'rank_corr_wide': corr_same_bits}
NAN_AT = {'ranksum_by': 3, 'ranksum_pairs': 3, 'ranksum_within': 5, 'rank_corr': 5, 'rank_corr_by': 5, 'rank_corr_wide': 5}
PAIRS_IDX = np.array(rs.PAIRS, dtype=np.int32)


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.unpin_expression()
    e.drop_expression()


def run_entry(eng, case, entry, work_bytes=0):
    if entry == 'ranksum_by':
        return eng.gene_ranksum_by(case.codes, rs.LEVELS, work_bytes)
    if entry == 'ranksum_pairs':
        return eng.gene_ranksum_pairs(case.codes, rs.LEVELS, PAIRS_IDX, work_bytes)
    if entry == 'ranksum_within':
        return eng.gene_ranksum_within(case.codes, rs.LEVELS, case.blocks, rs.BLOCKS, *rs.within_weights_of(case),
                                       work_bytes=work_bytes)
    if entry == 'rank_corr':
        return eng.gene_rank_corr(case.keys, work_bytes)
    if entry == 'rank_corr_by':
        return eng.gene_rank_corr_by(case.keys, case.codes, rs.LEVELS, work_bytes)
    assert entry == 'rank_corr_wide'
    return eng.gene_rank_corr_wide(case.wide, work_bytes)


def check_entries(eng, case, entries, budgets_of):
    """every entry under the default budget against its restatement, then the same bits under each of budgets_of(entry);
    returns {entry: what the device gave}"""
    assert rs.largest_tie_term(case) < 2 ** 53                                   # equality is the right comparison
    eng.ensure_expression(rs.upload_of(case))
    out = {}
    for entry in entries:
        name = '%s %s %s' % (case.name, case.form, entry)
        got = run_entry(eng, case, entry)
        EQUAL[entry](name, got, rs.reference(case, entry))
        for work_bytes in budgets_of(entry):
            SAME_BITS[entry](run_entry(eng, case, entry, work_bytes), got, ~got[NAN_AT[entry]])
        out[entry] = got
    return out


# ------------------------------------------------------------------ a: the dense form's gene axis
@pytest.mark.parametrize('G', rs.AXIS_GENES)
@pytest.mark.parametrize('form', rs.AXIS_FORMS)
def test_dense_genes_beyond_the_first_tile_of_64(eng, form, G):
    case = rs.gene_axis_case(form, G)
    f64 = form.endswith('f64')
    out = check_entries(eng, case, rs.ENTRIES, lambda entry: rs.axis_budgets(entry, f64)[1:])
    assert eng.expression_shape()['format'] == 'dense' and eng.expression_shape()['f64'] == f64
    planted = sorted(rs.axis_nan_cells(G))
    for entry in rs.ENTRIES:
        assert list(np.flatnonzero(out[entry][NAN_AT[entry]])) == planted, entry   # the flags sit on the planted genes


# ------------------------------------------------------------------ b: the lengths
@pytest.mark.parametrize('n', rs.LENGTHS)
@pytest.mark.parametrize('form', rs.LENGTH_FORMS)
def test_lists_of_every_length_around_the_units(eng, form, n):
    case = rs.length_case(n, form)
    again = [rs.ONE_GENE_BUDGET] if form == 'csr-f32' else []                    # ... and with one gene per tile
    out = check_entries(eng, case, rs.ENTRIES, lambda entry: again)
    assert eng.expression_shape()['format'] == ('dense' if form.startswith('dense') else 'gene-major')
    m = n
    rank2, tie, nl, nan = out['ranksum_by']
    assert not nan.any() and int(nl.sum()) == m
    # the constant gene and the gene without entries: every cell has the midrank, one run over the whole list
    for g in (1, 5):
        np.testing.assert_array_equal(rank2[:, g], nl * (m + 1))
        assert tie[g] == float(m ** 3 - m)
    # two values cut at position a = n // 2 of the sorted list: 2 x midrank is a + 1 below the cut and m + a + 1 above it
    a = n // 2
    low = np.array([int(((case.V[:, 2] == -1.0) & (case.codes == l)).sum()) for l in range(rs.LEVELS)])
    np.testing.assert_array_equal(rank2[:, 2], low * (a + 1) + (nl - low) * (m + a + 1))
    assert tie[2] == float(a ** 3 - a + (m - a) ** 3 - (m - a)) and tie[0] == 0.0
    # gene 0 against key 0, each increasing in the other: S = (m^3 - m) / 3; against itself in the wide call as well
    s_lo, s_hi, tie_gene, tie_key, got_m, _ = out['rank_corr']
    want_lo, want_hi = limbs(np.array([[(m ** 3 - m) // 3]], dtype=object))
    assert got_m == m and s_lo[0, 0] == want_lo[0, 0] and s_hi[0, 0] == want_hi[0, 0] and tie_key[0] == 0.0 and tie_gene[0] == 0.0
    assert out['rank_corr_wide'][0][0, 0] == want_lo[0, 0] and (s_lo[:, [1, 5]] == 0).all() and (s_hi[:, [1, 5]] == 0).all()
    runs = np.unique(case.keys[1], return_counts=True)[1]
    assert tie_key[1] == float(sum(int(t) ** 3 - int(t) for t in runs))


# ------------------------------------------------------------------ c: the kept entries against the stored ones
@pytest.mark.parametrize('k', rs.KEPT_COUNTS)
def test_a_list_shorter_than_what_is_stored_of_it(eng, k):
    case = rs.kept_case(k)
    out = check_entries(eng, case, ['ranksum_by', 'rank_corr'], lambda entry: [rs.ONE_GENE_BUDGET])
    rank2, tie, nl, nan = out['ranksum_by']
    s_lo, s_hi, tie_gene, tie_key, m, flagged = out['rank_corr']
    assert not nan.any() and not flagged.any() and m == int(nl.sum()) == 560
    if k == 0:                                                                   # the numbers of a gene without stored entries
        np.testing.assert_array_equal(rank2[:, 0], rank2[:, 2])
        np.testing.assert_array_equal(rank2[:, 0], nl * (m + 1))
        assert tie[0] == tie[2] == tie_gene[0] == tie_gene[2] == float(m ** 3 - m)
        assert (s_lo[:, [0, 2]] == 0).all() and (s_hi[:, [0, 2]] == 0).all()


# ------------------------------------------------------------------ d: the columns formed from X
@pytest.mark.parametrize('n', rs.X_CELLS)
def test_x_route_on_few_cells_and_around_a_block_of_256(eng, n):
    x = rs.x_case(n)
    assert rs.largest_tie_term(x.case) < 2 ** 53
    eng.ensure_expression(rs.upload_of(x.case))
    eng.upload_x(x.X)
    gen = eng.x_generation()
    want = rs.x_columns_of(x)
    got = eng.x_columns(x.xrow, x.Z)
    assert got.shape == (rs.Q_WIDE, n) and got.dtype == np.float64 and got.tobytes() == want.tobytes()
    via_x = eng.gene_rank_corr_x(x.xrow, x.Z)
    wide = eng.gene_rank_corr_wide(want)
    assert via_x[4] == wide[4] == int((x.xrow >= 0).sum()) and not via_x[5].any()
    corr_same_bits(via_x, wide)
    corr_equal('x route n=%d' % n, via_x, restated_rank_corr(rs.typed_values(x.case), want))
    corr_same_bits(eng.gene_rank_corr_x(x.xrow, x.Z, rs.ONE_GENE_BUDGET), via_x)
    assert eng.x_generation() == gen                                             # X is read only
