"""cna.tl.coef_populations on the CPU: the scipy restatement of Engine.graph_components (what the GPU tests compare the
device with), pinned on hand-written graphs whose answer is written out here, and the labels, the numbering, the filters,
the selection rule and the refusals of the host side against an engine double defined here whose graph_components is the
restatement."""
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components


# ------------------------------------------------------------------ the restatement (the oracle of the issue)
def restated_components(A, codes, min_cells=1, n_classes=None):
    """What Engine.graph_components returns: per class, scipy's weakly connected components of the class's rows and
    columns, every STORED entry an edge whatever its value (a stored zero included: the pattern is what is read); then the
    components with at least min_cells cells sorted by class, size descending, smallest cell index ascending."""
    A = sp.csr_matrix(A)
    pattern = sp.csr_matrix((np.ones(len(A.indices), dtype=np.int8), A.indices, A.indptr), shape=A.shape)
    codes = np.asarray(codes, dtype=np.int32)
    n = len(codes)
    assert A.shape == (n, n)
    if n_classes is None:
        n_classes = int(codes.max(initial=-1)) + 1
    totals = np.zeros(n_classes, dtype=np.int64)
    cls, size, first = [np.empty(0, dtype=np.int32)], [np.empty(0, dtype=np.int64)], [np.empty(0, dtype=np.int64)]
    found = np.full(n, -1, dtype=np.int64)                       # the cell's component among all that were found
    for c in range(n_classes):
        cells = np.flatnonzero(codes == c)
        if not len(cells):
            continue
        k, lab = connected_components(pattern[cells][:, cells], directed=True, connection='weak')
        found[cells] = totals.sum() + lab
        totals[c] = k
        fc = np.full(k, n, dtype=np.int64)
        np.minimum.at(fc, lab, cells)
        cls.append(np.full(k, c, dtype=np.int32))
        size.append(np.bincount(lab, minlength=k).astype(np.int64))
        first.append(fc)
    cls, size, first = np.concatenate(cls), np.concatenate(size), np.concatenate(first)
    kept = np.flatnonzero(size >= min_cells)
    kept = kept[np.lexsort((first[kept], -size[kept], cls[kept]))]
    place = np.full(len(cls) + 1, -1, dtype=np.int32)            # [-1] serves the cells without a class
    place[kept] = np.arange(len(kept), dtype=np.int32)
    return place[found], {'class': cls[kept], 'size': size[kept], 'first': first[kept]}, totals


def graph(n, edges, values=None, dtype=np.float32):
    """CSR with exactly the entries (i, j) of `edges`, in that order per row, duplicates and zeros kept as stored."""
    edges = sorted(enumerate(edges), key=lambda t: t[1][0])
    vals = np.ones(len(edges)) if values is None else np.asarray(values, dtype=np.float64)
    indptr = np.zeros(n + 1, dtype=np.int64)
    for _, (i, _j) in edges:
        indptr[i + 1] += 1
    A = sp.csr_matrix((np.array([vals[k] for k, _ in edges], dtype=dtype), np.array([j for _, (_i, j) in edges], dtype=np.int32),
                       np.cumsum(indptr)), shape=(n, n))
    assert A.nnz == len(edges)
    return A


TRI = [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)]


def two_triangles(bridge_class):
    """cells 0-2 and 4-6 are triangles of class 0, cell 3 joins them"""
    edges = TRI + [(a + 4, b + 4) for a, b in TRI] + [(2, 3), (3, 2), (3, 4), (4, 3)]
    return graph(7, edges), np.array([0, 0, 0, bridge_class, 0, 0, 0], dtype=np.int32)


def test_restatement_on_a_path():
    A = graph(5, [(i, i + 1) for i in range(4)] + [(i + 1, i) for i in range(4)])
    comp, lst, tot = restated_components(A, [0, 0, 1, 1, 1])
    assert comp.tolist() == [0, 0, 1, 1, 1]
    assert lst['class'].tolist() == [0, 1] and lst['size'].tolist() == [2, 3] and lst['first'].tolist() == [0, 2]
    assert tot.tolist() == [1, 1]


def test_restatement_two_triangles_through_an_unselected_cell():
    comp, lst, tot = restated_components(*two_triangles(-1))
    assert comp.tolist() == [0, 0, 0, -1, 1, 1, 1]
    assert lst['size'].tolist() == [3, 3] and lst['first'].tolist() == [0, 4] and tot.tolist() == [2]


def test_restatement_two_triangles_through_a_cell_of_the_other_sign():
    comp, lst, tot = restated_components(*two_triangles(1))
    assert comp.tolist() == [0, 0, 0, 2, 1, 1, 1]
    assert lst['class'].tolist() == [0, 0, 1] and lst['size'].tolist() == [3, 3, 1] and tot.tolist() == [2, 1]
    joined, _, tot0 = restated_components(*two_triangles(0))
    assert joined.tolist() == [0] * 7 and tot0.tolist() == [1]


def test_restatement_an_edge_stored_in_one_direction_only():
    comp, lst, _ = restated_components(graph(4, [(3, 0), (1, 2)]), [0, 0, 0, 0])
    assert comp.tolist() == [0, 1, 1, 0]                       # sizes tie: the smallest cell index decides
    assert lst['first'].tolist() == [0, 1]


def test_restatement_self_loop_duplicates_and_an_empty_row():
    A = graph(5, [(0, 0), (1, 2), (1, 2), (1, 2), (2, 1), (4, 4), (4, 1)])   # row 3 is empty
    comp, lst, tot = restated_components(A, [0, 0, 0, 0, 0])
    assert comp.tolist() == [1, 0, 0, 2, 0]
    assert lst['size'].tolist() == [3, 1, 1] and lst['first'].tolist() == [1, 0, 3] and tot.tolist() == [3]


def test_restatement_a_stored_zero_is_an_edge():
    """The resident graph keeps every stored entry (the upload copies indptr / indices / data as they are, the device
    renumbering moves entry by entry), and the components read the pattern only: an explicit zero joins its two cells.
    eliminate_zeros() is how a caller says otherwise."""
    A = graph(4, [(0, 1), (2, 3)], values=[0.0, 1.0])
    assert A.nnz == 2 and A.data[0] == 0
    comp, lst, _ = restated_components(A, [0, 0, 0, 0])
    assert comp.tolist() == [0, 0, 1, 1] and lst['size'].tolist() == [2, 2]
    A.eliminate_zeros()
    comp, lst, _ = restated_components(A, [0, 0, 0, 0])
    assert comp.tolist() == [1, 2, 0, 0] and lst['size'].tolist() == [2, 1, 1]


def test_restatement_min_cells_and_class_counts():
    A = graph(6, [(0, 1), (2, 3), (3, 4)])
    comp, lst, tot = restated_components(A, [0, 0, 2, 2, 2, 2], min_cells=2, n_classes=4)
    assert comp.tolist() == [0, 0, 1, 1, 1, -1]
    assert lst['class'].tolist() == [0, 2] and tot.tolist() == [1, 0, 2, 0]


# ------------------------------------------------------------------ the double
class GraphEngine:
    """Records its calls; graph_components is `restated_components` on the graph ensure_graph was given."""

    def __init__(self, nranks=1):
        self.nranks = nranks
        self.view_local = False
        self.calls = []
        self.A = None
        self._nam_sig = 'held'

    def ensure_graph(self, A, shard=None, defer=False):
        new = self.A is not A
        self.calls.append(('ensure_graph', new))
        self.A = A
        return new

    def graph_components(self, codes, min_cells=1, n_classes=None):
        assert codes.dtype == np.int32 and codes.shape == (self.A.shape[0],)
        self.calls.append(('graph_components', int(min_cells), n_classes))
        return restated_components(self.A, codes, min_cells, n_classes)


def _data(A, **cols):
    from cna_amd.synth import CellData
    n = A.shape[0]
    return CellData(pd.DataFrame(cols, index=pd.Index(['c%d' % i for i in range(n)])), A)


def _pops(*a, **k):
    import cna_amd as cna
    return cna.tl.coef_populations(*a, **k)


def _chain(n, cuts=()):
    """a path 0 - 1 - ... - n-1, both directions stored, without the links i - i+1 for i in cuts"""
    e = [(i, i + 1) for i in range(n - 1) if i not in cuts]
    return graph(n, e + [(j, i) for i, j in e])


def _example():
    """12 cells on a path: pos runs {0,1,2}, {5,6} and {11}; neg runs {3,4} and {8,9,10}; cell 7 is zero"""
    coef = np.array([1., 2, 3, -1, -1, .5, .5, 0, -2, -2, -2, 4])
    return _chain(12), coef


def test_labels_numbering_and_frame():
    A, coef = _example()
    d, e = _data(A, coef=coef), GraphEngine()
    frame, info = _pops(d, return_info=True, engine=e)
    assert list(frame.index) == ['pos1', 'pos2', 'pos3', 'neg1', 'neg2'] and frame.index.name == 'coef_pop'
    assert list(frame.columns) == ['sign', 'n_cells', 'first_cell', 'frac']
    assert frame['sign'].dtype == np.int8 and frame['sign'].tolist() == [1, 1, 1, -1, -1]
    assert frame['n_cells'].dtype == np.int64 and frame['n_cells'].tolist() == [3, 2, 1, 3, 2]
    assert frame['first_cell'].tolist() == ['c0', 'c5', 'c11', 'c8', 'c3']
    np.testing.assert_array_equal(frame['frac'].values, np.array([3, 2, 1, 3, 2]) / np.array([6., 6, 6, 5, 5]))
    col = d.obs['coef_pop']
    assert isinstance(col.dtype, pd.CategoricalDtype) and list(col.cat.categories) == list(frame.index)
    want = ['pos1'] * 3 + ['neg2'] * 2 + ['pos2'] * 2 + [np.nan] + ['neg1'] * 3 + ['pos3']
    assert [x if isinstance(x, str) else None for x in col] == [x if isinstance(x, str) else None for x in want]
    assert info == {'n_selected': {'pos': 6, 'neg': 5}, 'n_populations': {'pos': 3, 'neg': 2}, 'n_unlabelled_cells': 0}
    assert e.calls == [('ensure_graph', True), ('graph_components', 1, 2)]
    assert e._nam_sig is None                       # a graph new to the engine voids the NAM it vouched for
    e._nam_sig = 'held'
    _pops(d, engine=e)
    assert e.calls[2:] == [('ensure_graph', False), ('graph_components', 1, 2)] and e._nam_sig == 'held'


def test_size_ties_are_broken_by_the_smallest_cell_index():
    coef = np.array([0, 1., 1, 0, 1, 1, 0, 1, 1])
    d = _data(_chain(9), coef=coef)
    frame = _pops(d, engine=GraphEngine())
    assert frame['n_cells'].tolist() == [2, 2, 2] and frame['first_cell'].tolist() == ['c1', 'c4', 'c7']


def test_min_cells():
    A, coef = _example()
    d = _data(A, coef=coef)
    frame, info = _pops(d, min_cells=3, return_info=True, engine=GraphEngine())
    assert list(frame.index) == ['pos1', 'neg1'] and frame['n_cells'].tolist() == [3, 3]
    assert info['n_populations'] == {'pos': 3, 'neg': 2} and info['n_unlabelled_cells'] == 5
    assert d.obs['coef_pop'].isna().sum() == 6
    np.testing.assert_array_equal(frame['frac'].values, [3 / 6., 3 / 5.])
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            _pops(d, min_cells=bad, engine=GraphEngine())


def test_max_populations_warns_with_the_count():
    A, coef = _example()
    d = _data(A, coef=coef)
    with pytest.warns(UserWarning, match='5 populations.*3 largest.*2 are not'):
        frame, info = _pops(d, max_populations=3, return_info=True, engine=GraphEngine())
    # largest first over both signs, ties by the smallest cell index: pos {0,1,2}, neg {8,9,10}, then neg {3,4} before pos {5,6}
    assert list(frame.index) == ['pos1', 'neg1', 'neg2'] and frame['first_cell'].tolist() == ['c0', 'c8', 'c3']
    assert info['n_unlabelled_cells'] == 3 and d.obs['coef_pop'].notna().sum() == 8
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert len(_pops(d, max_populations=5, engine=GraphEngine())) == 5
    with pytest.raises(ValueError):
        _pops(d, max_populations=0, engine=GraphEngine())


def test_the_default_cap_is_what_the_strata_tools_take():
    from cna_amd.tools._strata import MAX_LEVELS
    n = 2 * (MAX_LEVELS + 3)
    coef = np.zeros(n)
    coef[::2] = 1.0                                  # every other cell of a path: n / 2 singletons
    d = _data(_chain(n), coef=coef)
    with pytest.warns(UserWarning, match='%d populations.*%d largest.*3 are not' % (MAX_LEVELS + 3, MAX_LEVELS)):
        frame = _pops(d, engine=GraphEngine())
    assert len(frame) == MAX_LEVELS and frame.index[-1] == 'pos%d' % MAX_LEVELS


def test_fdr_rule():
    A, coef = _example()
    fdr = np.full(12, 0.05)
    fdr[0] = np.nan                                  # a NaN fdr fails
    fdr[5] = 0.2
    fdr[8] = 0.1                                     # <= passes
    d = _data(A, coef=coef, coef_fdr=fdr)
    frame, info = _pops(d, return_info=True, engine=GraphEngine())
    assert info['n_selected'] == {'pos': 4, 'neg': 5}
    assert frame['first_cell'].tolist() == ['c1', 'c6', 'c11', 'c8', 'c3'] and frame['n_cells'].tolist() == [2, 1, 1, 3, 2]
    frame = _pops(d, fdr_thresh=0.25, engine=GraphEngine())
    assert frame['first_cell'].tolist() == ['c1', 'c5', 'c11', 'c8', 'c3']
    assert len(_pops(d, fdr_thresh=0.01, engine=GraphEngine())) == 0
    no_fdr = _data(A, coef=coef)
    assert len(_pops(no_fdr, engine=GraphEngine())) == 5          # no fdr column at all: the sign alone selects
    with pytest.raises(KeyError, match='coef_fdr'):
        _pops(no_fdr, fdr_thresh=0.1, engine=GraphEngine())
    with pytest.raises(KeyError, match='nope'):
        _pops(no_fdr, key='nope', engine=GraphEngine())


def test_non_finite_and_zero_coefficients_are_not_selected():
    coef = np.array([1., np.nan, 1, np.inf, 1, -np.inf, -1, 0., -1, -0.0, 1])
    d = _data(_chain(11), coef=coef)
    frame, info = _pops(d, return_info=True, engine=GraphEngine())
    assert info['n_selected'] == {'pos': 4, 'neg': 2}
    assert frame['n_cells'].tolist() == [1, 1, 1, 1, 1, 1] and frame['first_cell'].tolist() == ['c0', 'c2', 'c4', 'c10', 'c6', 'c8']


def test_no_cell_selected():
    d, e = _data(_chain(6), coef=np.zeros(6)), GraphEngine()
    frame, info = _pops(d, return_info=True, engine=e)
    assert len(frame) == 0 and list(frame.columns) == ['sign', 'n_cells', 'first_cell', 'frac']
    assert d.obs['coef_pop'].isna().all() and isinstance(d.obs['coef_pop'].dtype, pd.CategoricalDtype)
    assert info == {'n_selected': {'pos': 0, 'neg': 0}, 'n_populations': {'pos': 0, 'neg': 0}, 'n_unlabelled_cells': 0}


def test_key_added_and_other_keys():
    A, coef = _example()
    d = _data(A, other=coef, other_fdr=np.full(12, 0.01))
    frame = _pops(d, key='other', engine=GraphEngine())
    assert 'other_pop' in d.obs and frame.index.name == 'other_pop'
    frame = _pops(d, key='other', key_added='mine', engine=GraphEngine())
    assert 'mine' in d.obs and frame.index.name == 'mine' and list(d.obs['mine'].cat.categories) == list(frame.index)


def test_the_column_goes_into_the_strata_tools():
    from cna_amd.tools._strata import levels_of
    A, coef = _example()
    d = _data(A, coef=coef)
    frame = _pops(d, min_cells=2, engine=GraphEngine())
    codes, levels = levels_of(d.obs, 'coef_pop', 'test')
    assert set(levels) == set(frame.index) and (codes == -1).sum() == d.obs['coef_pop'].isna().sum() == 2       # the zero cell and the singleton
    for lab, n_cells in frame['n_cells'].items():
        assert (codes == list(levels).index(lab)).sum() == n_cells


def test_sharded_data_is_refused():
    A, coef = _example()
    d = _data(A, coef=coef)
    with pytest.raises(NotImplementedError, match='coef_populations'):
        _pops(d, engine=GraphEngine(nranks=2))
    d.uns['cna_shard'] = {'row0': 0, 'n_global': 24}
    with pytest.raises(NotImplementedError, match='coef_populations'):
        _pops(d, engine=GraphEngine())


def test_populations_do_not_depend_on_the_order_of_the_cells():
    rs = np.random.RandomState(3)
    n = 400
    A = sp.random(n, n, density=1.5 / n, random_state=rs, format='csr', dtype=np.float32)
    coef = rs.randn(n) * (rs.rand(n) < 0.8)
    fdr = rs.rand(n) * 0.15
    names = np.array(['c%d' % i for i in range(n)])
    d = _data(A, coef=coef, coef_fdr=fdr)
    f1 = _pops(d, engine=GraphEngine())
    p = rs.permutation(n)                                        # new cell i is old cell p[i]
    from cna_amd.synth import CellData
    d2 = CellData(pd.DataFrame({'coef': coef[p], 'coef_fdr': fdr[p]}, index=pd.Index(names[p])), sp.csr_matrix(A[p][:, p]))
    f2 = _pops(d2, engine=GraphEngine())

    def named_sets(dd):
        col = dd.obs['coef_pop']
        return {(lab[:3], frozenset(col.index[(col == lab).values])) for lab in col.cat.categories}
    assert named_sets(d) == named_sets(d2) and len(f1) == len(f2) > 10
    assert sorted(f1['n_cells'][f1['sign'] == 1]) == sorted(f2['n_cells'][f2['sign'] == 1])
    assert f1['n_cells'].tolist() == f2['n_cells'].tolist()       # sizes descend within a sign in both
    np.testing.assert_array_equal(f1['frac'].values, f2['frac'].values)


def test_abi_has_the_entry_points():
    from cna_amd import _ffi
    for name in ('cna_graph_components_find', 'cna_graph_components_list', 'cna_graph_components_label'):
        assert name in _ffi.SIGNATURES and hasattr(_ffi.load(), name)
    assert len(_ffi.KERNELS) == len(set(_ffi.KERNELS)) and 'components_hook' in _ffi.KERNELS
