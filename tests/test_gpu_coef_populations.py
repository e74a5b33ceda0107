"""cna.tl.coef_populations / cna_graph_components_* on the device (run with -m gpu on an MI355X), against the scipy
restatement of tests/test_coef_populations_host.py (itself pinned on hand-written graphs there).

Everything is integers: every returned array is compared with np.array_equal.  The sizes are the smallest at which each
mechanism of csrc/components.hip is exercised: a path of 5 000 cells in a shuffled numbering (the deepest tree for the cell
count), a row of 5 000 entries (beyond CC_HUB: spread over a grid), 5 000 singletons (the compaction crosses workgroups),
cliques of 70 (more entries than the 16 lanes of a row take in one turn), and cell counts around the wave and the
workgroup.  Every case prints the rounds (`sweeps`) it took and asserts 1 <= sweeps <= 32."""
import os
import re
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from test_coef_populations_host import graph, restated_components

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    src = open(os.path.join(ROOT, 'cna_amd', 'csrc', 'components.hip')).read()
    return int(re.search(r'constexpr \w+ %s = (\d+);' % name, src).group(1))


HUB = _constant('CC_HUB')


@pytest.fixture(scope='module')
def eng():
    from cna_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def run(e, A, codes, min_cells=1, n_classes=None, tag=''):
    """Engine.graph_components on A against the restatement, every array; returns what the device gave."""
    codes = np.asarray(codes, dtype=np.int32)
    e.ensure_graph(A)
    got = e.graph_components(codes, min_cells=min_cells, n_classes=n_classes)
    print('%s: cells %d, entries %d, components %d, sweeps %d' % (tag, A.shape[0], A.nnz, len(got[1]['size']), e.sweeps))
    assert 1 <= e.sweeps <= 32, tag
    want = restated_components(A, codes, min_cells, n_classes)
    same(got, want, tag)
    return got


def same(got, want, tag=''):
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), tag
    for k in ('class', 'size', 'first'):
        assert got[1][k].dtype == want[1][k].dtype and np.array_equal(got[1][k], want[1][k]), (tag, k)
    assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2]), tag


def path(n, seed, both=True):
    """a path through all n cells in a shuffled numbering; both=False stores i -> i+1 only"""
    p = np.random.RandomState(seed).permutation(n)
    e = list(zip(p[:-1].tolist(), p[1:].tolist()))
    return graph(n, e + [(j, i) for i, j in e] if both else e), p


def random_graph(n, degree, rs):
    """n * degree entries at uniformly drawn places, duplicates and self loops kept as stored (scipy.sparse.random with a
    RandomState permutes all n * n places: 23 s at 20 000 cells)"""
    m = int(n * degree)
    rows, cols = np.sort(rs.randint(n, size=m)), rs.randint(n, size=m).astype(np.int32)
    indptr = np.searchsorted(rows, np.arange(n + 1)).astype(np.int64)
    return sp.csr_matrix((np.ones(m, dtype=np.float32), cols, indptr), shape=(n, n))


# ------------------------------------------------------------------ path graphs
@pytest.mark.parametrize('both', [True, False])
def test_path_in_a_shuffled_numbering(eng, both):
    A, _ = path(5000, 1, both)
    comp, lst, tot = run(eng, A, np.zeros(5000), tag='path both=%s' % both)
    assert lst['size'].tolist() == [5000] and tot.tolist() == [1] and (comp == 0).all()


def test_path_cut_into_runs_of_classes(eng):
    rs = np.random.RandomState(2)
    A, p = path(5000, 3)
    along = np.concatenate([np.full(rs.randint(1, 301), c) for c in rs.randint(-1, 2, size=200)])[:5000]
    assert len(along) == 5000
    codes = np.empty(5000, dtype=np.int32)
    codes[p] = along
    _, lst, _ = run(eng, A, codes, n_classes=2, tag='runs')
    assert len(lst['size']) >= 10                      # ~33 runs, a third without a class, neighbours of one class merged


def test_every_other_cell_of_a_path(eng):
    A, p = path(5000, 4)
    codes = np.full(5000, -1, dtype=np.int32)
    codes[p[::2]] = 0
    _, lst, tot = run(eng, A, codes, tag='every other')
    assert tot.tolist() == [2500] and (lst['size'] == 1).all()


# ------------------------------------------------------------------ hubs
def star(n_leaves, hub_row=True, leaf_rows=True, seed=5):
    n = n_leaves + 1
    hub = int(np.random.RandomState(seed).randint(n))
    leaves = [i for i in range(n) if i != hub]
    e = ([(hub, v) for v in leaves] if hub_row else []) + ([(v, hub) for v in leaves] if leaf_rows else [])
    return graph(n, e), hub


@pytest.mark.parametrize('hub_row, leaf_rows', [(True, True), (True, False), (False, True)])
def test_star_with_a_classed_hub(eng, hub_row, leaf_rows):
    A, hub = star(5000, hub_row, leaf_rows)
    assert not hub_row or A.indptr[hub + 1] - A.indptr[hub] == 5000 > HUB
    _, lst, _ = run(eng, A, np.zeros(5001), tag='star hub_row=%s leaf_rows=%s' % (hub_row, leaf_rows))
    assert lst['size'].tolist() == [5001]


def test_star_with_an_unclassed_hub(eng):
    A, hub = star(5000)
    codes = np.zeros(5001, dtype=np.int32)
    codes[hub] = -1
    _, lst, tot = run(eng, A, codes, tag='star, hub unclassed')
    assert tot.tolist() == [5000] and len(lst['size']) == 5000


# ------------------------------------------------------------------ cliques
def cliques(bridge):
    """cells 0-69 and 71-140 are cliques; bridge: 'same' joins 0 - 71, 'other' the same edge with the second clique of
    class 1, 'unclassed' joins both to cell 70, which has no class"""
    e = [(i, j) for i in range(70) for j in range(70) if i != j]
    e = e + [(i + 71, j + 71) for i, j in e]
    codes = np.zeros(141, dtype=np.int32)
    codes[70] = -1
    if bridge == 'unclassed':
        e += [(0, 70), (70, 0), (70, 71), (71, 70)]
    else:
        e += [(0, 71), (71, 0)]
        if bridge == 'other':
            codes[71:] = 1
    return graph(141, e), codes


@pytest.mark.parametrize('bridge', ['same', 'other', 'unclassed'])
@pytest.mark.parametrize('min_cells', [1, 2, 71])
def test_two_cliques(eng, bridge, min_cells):
    A, codes = cliques(bridge)
    _, lst, _ = run(eng, A, codes, min_cells=min_cells, tag='cliques %s min_cells=%d' % (bridge, min_cells))
    assert lst['size'].tolist() == ([140] if bridge == 'same' else [] if min_cells == 71 else [70, 70])


# ------------------------------------------------------------------ ragged sizes
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 100003])
def test_random_graph(eng, n):
    """A graph of 100 000 cells or more goes up in the caller's order while its device order is computed on a host thread,
    and a later ensure_graph adopts that order: the first call below runs before the renumbering (engine.perm is None), the
    second, after wait_reorder(), behind it (codes and labels pass through orig_idx)."""
    from cna_amd import engine as E
    rs = np.random.RandomState(n)
    A = random_graph(n, 3, rs)
    codes = np.where(rs.rand(n) < 0.3, -1, rs.randint(0, 3, size=n)).astype(np.int32)
    run(eng, A, codes, n_classes=3, tag='random %d' % n)
    lazy = n >= E._REORDER_ASYNC_CELLS and E._REORDER_ASYNC and os.environ.get('CNA_REORDER', '1') not in ('0', 'off', 'no')
    if lazy:
        assert eng.perm is None
        eng.wait_reorder()
    run(eng, A, codes, min_cells=3, n_classes=3, tag='random %d, min_cells 3' % n)
    if lazy:
        assert eng.perm is not None
        run(eng, A, codes, n_classes=3, tag='random %d, device order' % n)


# ------------------------------------------------------------------ oddities of the stored graph
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_self_loops_duplicates_empty_rows_and_stored_zeros(eng, dtype):
    e = [(0, 0), (1, 2), (1, 2), (1, 2), (2, 1), (4, 4), (4, 1), (5, 6), (7, 6)]      # row 3 is empty
    A = graph(8, e, values=[1, 1, 2, 3, 1, 1, 1, 0, 0.5], dtype=dtype)
    assert A.nnz == 9 and A.data[7] == 0
    comp, lst, _ = run(eng, A, np.zeros(8), tag='oddities %s' % np.dtype(dtype).name)
    assert comp[5] == comp[6] == comp[7]              # the stored zero 5 -> 6 is an edge
    assert lst['size'].tolist() == [3, 3, 1, 1]


def test_bad_codes_are_refused(eng):
    from cna_amd._ffi import CnaHipError
    A, _ = path(100, 0)
    eng.ensure_graph(A)
    for bad in (-2, 2):
        codes = np.zeros(100, dtype=np.int32)
        codes[37] = bad
        with pytest.raises(CnaHipError, match='outside'):
            eng.graph_components(codes, n_classes=2)
    with pytest.raises(ValueError):
        eng.graph_components(np.zeros(99, dtype=np.int32))


def test_two_calls_return_identical_arrays(eng):
    n = 30011
    rs = np.random.RandomState(8)
    A = random_graph(n, 4, rs)
    codes = rs.randint(-1, 2, size=n).astype(np.int32)
    a = run(eng, A, codes, tag='repeat 1')
    b = run(eng, A, codes, tag='repeat 2')
    same(a, b)


# ------------------------------------------------------------------ a real input
@pytest.fixture(scope='module')
def real():
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd.engine import Engine
    data, meta = synth.make_dataset(20000, 30, k=15, seed=0)
    e = Engine()
    e.reuse_nam = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = cna.tl.association(data, meta['y'], 'id', Nnull=200, seed=0, key_added='coef', engine=e)
    yield data, meta, e, res
    e.close()


def codes_of(obs, fdr_thresh=0.1):
    v, f = obs['coef'].values, obs['coef_fdr'].values
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(v) & (f <= fdr_thresh)
    return np.where(ok & (v > 0), 0, np.where(ok & (v < 0), 1, -1)).astype(np.int32)


def named_sets(obs, col='coef_pop'):
    c = obs[col]
    return {(lab[:3], frozenset(c.index[(c == lab).values])) for lab in c.cat.categories}


@pytest.mark.parametrize('fdr_thresh', [None, 0.5])
def test_end_to_end_against_the_restatement_and_under_a_permutation(real, fdr_thresh):
    """The default threshold, and a loose one that lets many small populations of both signs through.  The engine adopts the device's cell order at the upload of a graph of this size (engine.perm is not None: asserted),
    so the codes and the labels pass through orig_idx.  The other state -- resident in the caller's order while the order
    is still being computed -- is reached only by graphs of 100 000 cells and more: test_random_graph's 100 003 cells run
    in it, and behind the renumbering."""
    import cna_amd as cna
    from cna_amd.synth import CellData
    data, meta, e, _ = real
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        frame, info = cna.tl.coef_populations(data, fdr_thresh=fdr_thresh, return_info=True, engine=e)
    assert e.perm is not None
    print('real, fdr_thresh %s: %d populations, selected %s, sweeps %d' % (fdr_thresh, len(frame), info['n_selected'], info['sweeps']))
    assert 1 <= info['sweeps'] <= 32
    A = data.obsp['connectivities']
    codes = codes_of(data.obs, 0.1 if fdr_thresh is None else fdr_thresh)
    assert (codes >= 0).sum() > 100
    comp, lst, tot = restated_components(A, codes, 1, 2)
    lab = np.array(['pos', 'neg'])[lst['class']]
    num = np.arange(len(lab)) + 1 - np.where(lst['class'] == 0, 0, (lst['class'] == 0).sum())
    names = np.array(['%s%d' % t for t in zip(lab, num)], dtype=object)
    keep = len(names) <= 1024
    assert keep, 'the synthetic association is expected to give fewer than 1024 populations'
    assert list(frame.index) == list(names)
    assert np.array_equal(frame['n_cells'].values, lst['size']) and list(frame['first_cell']) == list(data.obs.index[lst['first']])
    want = np.where(comp >= 0, names[np.maximum(comp, 0)], None)
    got = np.asarray(data.obs['coef_pop'].astype(object).where(data.obs['coef_pop'].notna(), None))
    assert np.array_equal(got, want)
    assert info['n_populations'] == {'pos': int(tot[0]), 'neg': int(tot[1])}
    # the caller's cells permuted: the same sets of cells with the same sizes
    p = np.random.RandomState(11).permutation(len(data.obs))
    d2 = CellData(data.obs[['coef', 'coef_fdr']].iloc[p].copy(), sp.csr_matrix(A[p][:, p]))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        f2 = cna.tl.coef_populations(d2, fdr_thresh=fdr_thresh, engine=e)
    assert named_sets(d2.obs) == named_sets(data.obs)
    assert f2['n_cells'].tolist() == frame['n_cells'].tolist() and f2['sign'].tolist() == frame['sign'].tolist()


def test_nothing_else_is_voided_and_the_column_composes(real):
    """association, coef_populations, association: the second association is bit-identical to the first and walks nothing;
    nam_strata on the new column reuses the resident NAM (no nam_* kernel runs: as test_nam_cache_skips_the_walk shows
    it); its rows summed over the levels equal nam_strata of one level holding the labelled cells -- each side a float64
    sum over the same cells in another order: within 2 m 2^-53 of the sum, m the labelled cells (NAM entries are >= 0)."""
    import cna_amd as cna
    data, meta, e, _ = real
    kw = dict(Nnull=200, seed=0, key_added='coef', engine=e, return_full=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a1 = cna.tl.association(data, meta['y'], 'id', **kw).materialize()
        coef1, fdr1 = data.obs['coef'].values.copy(), data.obs['coef_fdr'].values.copy()
        e.prof_reset()
        e.prof_enable(True)
        frame = cna.tl.coef_populations(data, min_cells=5, engine=e)
        a2 = cna.tl.association(data, meta['y'], 'id', **kw).materialize()
        by = cna.tl.nam_strata(data, 'coef_pop', 'id', engine=e)
        e.sync()
        e.prof_enable(False)
    prof = e.prof()
    print('profile:', {k: v for k, v in prof.items() if k.startswith('components')})
    assert 'components_hook' in prof and not any(k.startswith('nam_') for k in prof), prof
    assert a1.p == a2.p and a1.k == a2.k
    np.testing.assert_array_equal(a1.ncorrs.values, a2.ncorrs.values)
    np.testing.assert_array_equal(a1.nam.values, a2.nam.values)
    np.testing.assert_array_equal(data.obs['coef'].values, coef1)
    np.testing.assert_array_equal(data.obs['coef_fdr'].values, fdr1)
    assert len(frame) >= 1 and sorted(by.columns) == sorted(frame.index)       # (levels come in order of first appearance)
    data.obs['labelled'] = np.where(data.obs['coef_pop'].notna(), 'all', None)
    one = cna.tl.nam_strata(data, 'labelled', 'id', engine=e)
    m = int(data.obs['coef_pop'].notna().sum())
    total = by.values.sum(axis=1)
    err = np.abs(total - one['all'].values)
    print('nam_strata: largest difference %.3g, bound %.3g' % (err.max(), (2 * m * 2.0 ** -53 * one['all'].values).min()))
    assert (err <= 2 * m * 2.0 ** -53 * np.abs(one['all'].values)).all()
    # coef_strata on the column: the statistics the tool leaves to it
    st = cna.tl.coef_strata(data, 'coef_pop', key='coef', engine=e)
    assert sorted(st.index) == sorted(frame.index)
    st.index = pd.Index(list(st.index))
    st = st.loc[list(frame.index)]
    assert np.array_equal(st['n'].values, frame['n_cells'].values) and np.array_equal(st['n_kept'].values, frame['n_cells'].values)
    assert (st['min'].values[frame['sign'].values > 0] > 0).all()
    assert (st['max'].values[frame['sign'].values < 0] < 0).all()
