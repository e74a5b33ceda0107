"""cna_enrichment_extremes and cna.tl.gene_set_test on the device (run with -m gpu on an MI355X), against the textbook
restatement of tests/test_gene_sets_host.py (argsort, then a plain Python walk over every position).

Where the kernels branch (csrc/enrich.hip; EN_TILE, EN_THREADS and EN_TARGETS are read from the source):
  k_en_positions  a workgroup ranks EN_THREADS x EN_TARGETS = 1024 target genes and stages the column in LDS tiles of
                  EN_TILE = 2048 genes.  70 genes: one ragged tile, most lanes idle; 257: a second target per lane starts;
                  EN_TILE + 3 = 2051: a second tile of three genes, three workgroups of targets, so that all three forms of
                  the pair test run (tile before, after and across the targets); 4200: three tiles, five workgroups.
  k_en_extremes   four launches by set size, 64 / 256 / 1024 / 4096 slots (one wave for the first two, four for the others);
                  the sort runs over the next power of two.  Sizes 1, 2, 63, 64 | 65 | 257 | 4096 touch every class, both
                  sides of the first boundary and both ends of a sort.
Columns: 1, 2 and 65 (the column is a grid dimension of both kernels).

Exact cases: r in multiples of 1/8 in [-1, 1] -- heavy ties, both signed zeros, NaN genes (two in every column, others by
column) and one +inf and one -inf, which are invalid too.  With weights 1, |r| or r^2 every S_j is a multiple of 1/64 far
below 2^53, exact in any order; S_j / N_R and m_j / (Gv - k) are single correctly rounded divisions of the same operands on
both sides: up, down, size and valid are compared BIT FOR BIT.
Real-valued cases (standard normal clipped to [-1, 1]): |up - want| and |down - want| <= (2 k + 1) 2^-52 with k the set's
valid members -- two sums of at most k non-negative terms in different fixed orders, each divided by such a sum, and one
subtraction on either side; the miss term is the same expression on both sides.  size and valid exactly, NaN in the same
places.  up and down are compared, never a chosen es: no case is left out for a near-tie."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pandas as pd
import pytest

from test_gene_sets_host import RestatedEngine, restated_extremes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _constant(name):
    src = open(os.path.join(ROOT, 'cna_amd', 'csrc', 'enrich.hip')).read()
    return int(re.search(r'constexpr int %s = (\d+);' % name, src).group(1))


TILE, BLOCK = _constant('EN_TILE'), _constant('EN_THREADS') * _constant('EN_TARGETS')
assert (TILE, BLOCK) == (2048, 1024)
SHAPES = [(70, 65), (70, 1), (257, 2), (TILE + 3, 2), (4200, 3)]              # (genes, columns)
SET_SIZES = [1, 2, 63, 64, 65, 257, 4096]
U = 2.0 ** -52


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import get_engine
    e = get_engine()
    yield e
    e.drop_expression()


_cache = {}


def matrix(G, n_cols, kind):
    rs = np.random.RandomState(1000 * G + n_cols)
    if kind == 'dyadic':
        R = rs.randint(-8, 9, (n_cols, G)) / 8.0
        R[(R == 0) & (rs.rand(n_cols, G) < 0.5)] = -0.0
    else:
        R = np.clip(rs.standard_normal((n_cols, G)), -1.0, 1.0)
    R[rs.rand(n_cols, G) < 0.03] = np.nan
    R[:, [3, G - 2]] = np.nan                    # invalid in every column
    R[0, 5], R[-1, 6] = np.inf, -np.inf          # not finite: invalid as well
    R[0, [8, 9]] = [1.0, -1.0]                   # something finite stays at both ends
    return R


def gene_sets(R):
    """(set_ptr, set_genes, names)."""
    G = R.shape[1]
    rs = np.random.RandomState(G)
    sets = [('size %d' % m, rs.choice(G, m, replace=False)) for m in SET_SIZES if m <= G]
    a = rs.choice(G, 30, replace=False)
    sets += [('overlap a', a), ('overlap b', np.r_[a[:15], rs.choice(G, 15, replace=False)])]
    valid = np.flatnonzero(np.isfinite(R[0]))
    if len(valid) <= 4096:
        sets.append(('every valid gene of column 0', valid))
    sets.append(('all NaN', np.array([3, G - 2])))
    order = valid[np.argsort(-R[0][valid], kind='stable')]
    sets += [('top', order[:20]), ('bottom', order[-20:]), ('alternating', order[0:40:2]), ('empty', np.zeros(0, dtype=int))]
    members = [np.unique(m).astype(np.int32) for _, m in sets]
    ptr = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
    return ptr, np.concatenate(members), [n for n, _ in sets]


def case(G, n_cols, kind, weight):
    key = (G, n_cols, kind, weight)
    if key not in _cache:
        R = matrix(G, n_cols, kind)
        ptr, genes, names = gene_sets(R)
        want = restated_extremes(R, ptr, genes, weight)
        for a in want:
            a.setflags(write=False)
        _cache[key] = (R, ptr, genes, names, want)
    return _cache[key]


def test_the_cases_reach_what_they_are_for():
    R, ptr, genes, names, (up, down, size, valid) = case(70, 65, 'dyadic', 1)
    sizes = dict(zip(names, np.diff(ptr)))
    assert [sizes['size %d' % m] for m in (1, 2, 63, 64, 65)] == [1, 2, 63, 64, 65]
    i = names.index
    assert np.isnan(up[0, i('every valid gene of column 0')]) and size[0, i('every valid gene of column 0')] == valid[0]
    assert np.isfinite(up[1:, i('every valid gene of column 0')]).any()       # other columns have other NaN genes
    assert (size[:, i('all NaN')] == 0).all() and (size[:, i('empty')] == 0).all()
    assert up[0, i('top')] == 1.0 and down[0, i('top')] == 0.0 and up[0, i('bottom')] == 0.0 and down[0, i('bottom')] == -1.0
    assert (valid <= 70 - 2).all() and valid[0] <= 70 - 3 and (np.signbit(R) & (R == 0)).any() and (~np.signbit(R) & (R == 0)).any()
    R, ptr, genes, names, want = case(4200, 3, 'dyadic', 1)
    assert 4096 in np.diff(ptr) and 257 in np.diff(ptr)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('weight', [0, 1, 2])
@pytest.mark.parametrize('G,n_cols', SHAPES)
def test_dyadic_inputs_bit_for_bit(eng, G, n_cols, weight):
    R, ptr, genes, names, want = case(G, n_cols, 'dyadic', weight)
    got = eng.enrichment_extremes(R, ptr, genes, weight)
    for what, a, b in zip(('up', 'down', 'size', 'valid'), got, want):
        if not _same_bits(a, b):
            bad = np.argwhere(~((a == b) | ((a != a) & (b != b))))
            c = tuple(bad[0])
            raise AssertionError('%s differs at %d places, first (column, set) %s %s: got %r, want %r'
                                 % (what, len(bad), c, names[c[1]] if len(c) > 1 else '', a[c], b[c]))
    again = eng.enrichment_extremes(R, ptr, genes, weight)
    assert all(_same_bits(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize('weight', [0, 1, 2])
@pytest.mark.parametrize('G,n_cols', SHAPES)
def test_real_inputs_within_the_bound(eng, G, n_cols, weight):
    R, ptr, genes, names, (up, down, size, valid) = case(G, n_cols, 'real', weight)
    got = eng.enrichment_extremes(R, ptr, genes, weight)
    assert np.array_equal(got[2], size) and np.array_equal(got[3], valid)
    bound = (2.0 * size + 1.0) * U
    worst = 0.0
    for what, a, b in (('up', got[0], up), ('down', got[1], down)):
        assert np.array_equal(np.isnan(a), np.isnan(b)), what
        ok = ~np.isnan(b)
        err = np.abs(a[ok] - b[ok])
        worst = max(worst, float(np.max(err / bound[ok])))
        print('G=%d cols=%d weight=%d %s: max |err| / bound = %.3f' % (G, n_cols, weight, what, float(np.max(err / bound[ok]))))
        assert (err <= bound[ok]).all(), (what, float(np.max(err / bound[ok])))
    assert (got[0][~np.isnan(up)] >= 0).all() and (got[1][~np.isnan(up)] <= 0).all()
    again = eng.enrichment_extremes(R, ptr, genes, weight)                        # two runs: the same bits
    assert all(_same_bits(a, b) for a, b in zip(got, again))


def _raw(eng, R, ptr, genes, weight):
    from cna_amd._ffi import ptr as p
    n_cols, G = R.shape
    n_sets = len(ptr) - 1
    out = [np.full((n_cols, n_sets), 7.5), np.full((n_cols, n_sets), 7.5), np.full((n_cols, n_sets), -5, dtype=np.int32),
           np.full(n_cols, -5, dtype=np.int32)]
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    genes = np.ascontiguousarray(genes, dtype=np.int32)
    rc = eng.lib.cna_enrichment_extremes(eng.h, p(R), n_cols, G, p(ptr), p(genes), n_sets, weight, *[p(a) for a in out])
    return rc, out


def _untouched(out):
    return (out[0] == 7.5).all() and (out[1] == 7.5).all() and (out[2] == -5).all() and (out[3] == -5).all()


def test_refusals_leave_the_outputs_as_they_were(eng):
    R, ptr, genes, names, want = case(257, 2, 'dyadic', 1)
    rc, out = _raw(eng, R, ptr, genes, 1)
    assert rc == 0 and all(_same_bits(a, b) for a, b in zip(out, want))            # the same entry, unrefused
    first65 = int(ptr[names.index('size 65')])

    def changed(at, value):
        g = genes.copy()
        g[at] = value
        return g
    cases = {'an index past the genes': (ptr, changed(first65 + 64, 257), 1),
             'a negative index': (ptr, changed(first65, -1), 1),
             'a descending pair': (ptr, changed(first65 + 11, genes[first65 + 9]), 1),
             'an equal pair': (ptr, changed(first65 + 11, genes[first65 + 10]), 1),
             'weight 3': (ptr, genes, 3), 'weight -1': (ptr, genes, -1)}
    big = np.arange(4200 - 4097, 4200, dtype=np.int32)
    cases['a set of 4097'] = (np.array([0, 4097]), big, 1)
    cases['offsets that fall'] = (np.array([0, 5, 3, len(genes)]), genes, 1)
    cases['offsets that start at 1'] = (np.r_[1, ptr[1:]], genes, 1)
    for name, (p_, g_, w_) in cases.items():
        Rc = R if name != 'a set of 4097' else case(4200, 3, 'dyadic', 1)[0]
        rc, out = _raw(eng, Rc, p_, g_, w_)
        assert rc == EINVAL, (name, rc)
        assert _untouched(out), name
        assert b'cna_enrichment_extremes' in eng.lib.cna_last_error(), name
    rc, out = _raw(eng, case(4200, 3, 'dyadic', 1)[0], np.array([0, 4096]), big[1:], 1)    # 4096 members pass
    assert rc == 0 and (out[2] <= 4096).all() and not _untouched(out)
    rc, out = _raw(eng, R, ptr, genes, 1)                                          # and the entry still works afterwards
    assert rc == 0 and all(_same_bits(a, b) for a, b in zip(out, want))


def test_a_resident_expression_matrix_stays(eng):
    rs = np.random.RandomState(2)
    E = rs.gamma(2.0, 1.0, (500, 40)) * (rs.rand(500, 40) < 0.6)
    eng.ensure_expression(E)
    before = eng.expression_shape()
    v = rs.randn(1, 500)
    r0 = eng.gene_corr(v)
    R, ptr, genes, names, want = case(257, 2, 'dyadic', 2)
    got = eng.enrichment_extremes(R, ptr, genes, 2)
    assert all(_same_bits(a, b) for a, b in zip(got, want))
    assert eng.expression_shape() == before and before['format'] == 'dense' and before['n_genes'] == 40
    assert eng.gene_corr(v).tobytes() == r0.tobytes()
    base = eng.device_bytes()
    eng.drop_expression()                                                          # frees the enrichment buffers too
    assert eng.device_bytes() < base - E.nbytes // 2
    eng.enrichment_extremes(R, ptr, genes, 2)
    held = eng.device_bytes()
    eng.drop_expression()
    assert eng.device_bytes() < held


# ------------------------------------------------------------------ end to end
def expression(n, g, seed):
    """cells x genes float64, about 60 % present; gene 1 all zero (the recipe of tests/test_gpu_gene_test.py)."""
    rs = np.random.RandomState(seed)
    E = rs.gamma(2.0, 1.0, (n, g)) * (rs.rand(n, g) < 0.6)
    E[:, 1] = 0.0
    return E


def test_gene_set_test_end_to_end(eng):
    """3000 cells x 24 samples x 130 genes, Nnull=50, seed=1; a dozen sets of 5 to 40 genes."""
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd.tools._gene_sets import enrichment_stats
    from cna_amd.tools._gene_test import benjamini_hochberg
    data, meta = synth.make_dataset(3000, 24, k=15, seed=24)
    y = meta['y']
    gnames = ['GENE%d' % i for i in range(130)]
    E = expression(3000, 130, seed=130)
    d1 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E, var=pd.DataFrame(index=pd.Index(gnames)))
    d2 = type(data)(data.obs[['id']].copy(), data.obsp['connectivities'], X=E, var=pd.DataFrame(index=pd.Index(gnames)))
    rs = np.random.RandomState(5)
    sets = {}
    for i, m in enumerate([5, 6, 8, 11, 15, 20, 24, 29, 33, 37, 40, 12]):
        sets['set%d' % i] = ['GENE%d' % g for g in rs.choice(130, m, replace=False)] + ['unknown%d' % i]
    sets['set11'] = sets['set11'] + ['GENE1']                                     # the constant gene: matched, never valid
    sets['small'] = gnames[:4]
    call = dict(nsteps=3, Nnull=50, seed=1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        genes, null_r = cna.tl.gene_test(d1, y, 'id', return_null=True, engine=eng, **call)
        out, null_es = cna.tl.gene_set_test(d2, y, 'id', sets, min_size=5, return_null=True, engine=eng, **call)
    for k in ('coef', 'coef_fdr'):
        assert d2.obs[k].values.tobytes() == d1.obs[k].values.tobytes(), k
    assert out.attrs['genes'].equals(genes) and out.attrs['p'] == genes.attrs['p'] and out.attrs['n_null'] == 50
    assert out.attrs['n_dropped'] == 1 and list(out.index) == ['set%d' % i for i in range(12)]
    want, want_null = cna.tl.gene_set_enrich(genes['r'].values, null_r, sets, gnames, min_size=5, return_null=True,
                                             engine=RestatedEngine())
    assert list(out.columns) == list(want.columns) and list(out.index) == list(want.index)
    assert np.array_equal(out['n_given'].values, want['n_given'].values) and np.array_equal(out['size'].values, want['size'].values)
    assert out['size'].values[11] == 12 - ('GENE1' in sets['set11'][:12]) and null_es.shape == (12, 50)
    bound = (2.0 * out['size'].values + 1.0) * U
    d_es = np.abs(out['es'].values - want['es'].values)
    d_null = np.abs(null_es - want_null)
    print('end to end: max |es - want| / bound = %.3f, null es %.3f'
          % (float(np.max(d_es / bound)), float(np.max(d_null / bound[:, None]))))
    assert np.isfinite(out['es'].values).all() and np.isfinite(null_es).all()
    assert (d_es <= bound).all() and (d_null <= bound[:, None]).all()
    # nes, p and q: the module's own statistics of the device's scores, and equal to the restatement's after that
    nes, p = enrichment_stats(out['es'].values, null_es)
    assert np.array_equal(out['nes'].values, nes) and np.array_equal(out['p'].values, p)
    assert np.array_equal(out['q'].values, benjamini_hochberg(p))
    assert np.array_equal(out['p'].values, want['p'].values) and np.array_equal(out['q'].values, want['q'].values)
    # nes = es / mean |null es of its sign|: the bound on both, over the mean, plus the roundings of mean and quotient
    same = np.where((want['es'].values >= 0)[:, None], want_null >= 0, want_null < 0)
    mean = np.array([np.abs(want_null[i][same[i]]).mean() for i in range(12)])
    tol = bound * (1.0 + np.abs(want['nes'].values)) / mean + 64 * U * np.abs(want['nes'].values)
    assert (np.abs(out['nes'].values - want['nes'].values) <= tol).all()
