"""``cna.tl.coef_populations``: the connected expanded / depleted populations an association finds, on the device.

The method exists so that nobody has to choose a clustering resolution (demo/demo.ipynb 1.3: "CNA automatically picked up
on this without needing to be given a resolution parameter"), and its result is then described as populations: "a
sub-population of the left-hand cluster", "these cells comprise only ~6 % of the cells that pass the threshold and so are
likely false discoveries".  Those sentences ask which connected groups of same-sign, FDR-passing neighbourhoods there are,
how big each is and which cells it holds: connected components of the kNN graph (_nam.py:12-19) restricted to the cells of
one sign.  The graph is resident on the device for the walk; the components are found there (csrc/components.hip,
``cna_graph_components_*``).  This module is the host side only: the classes, the numbering, the column and the frame.
"""
import warnings

import numpy as np
import pandas as pd

from ..engine import get_engine
from ._nam import _as_csr, get_connectivity, refuse_sharded, shard_of
from ._nam_strata import signed_passes
from ._strata import MAX_LEVELS

SIGNS = ('pos', 'neg')          # class 0, class 1


def coef_populations(data, key='coef', fdr_thresh=None, min_cells=1, max_populations=MAX_LEVELS, key_added=None,
                     return_info=False, engine=None):
    """The connected populations of expanded and of depleted neighbourhoods: one row per population, and
    ``data.obs[key_added]`` (default ``key + '_pop'``) naming every cell's population.

    A cell is SELECTED by the rule of ``nam_strata(sign_of=key)``: ``data.obs[key]`` finite and not zero and, when
    ``data.obs`` has ``key + '_fdr'``, ``fdr <= fdr_thresh`` (default 0.1; a NaN fdr fails; ``fdr_thresh`` without that column
    is a KeyError).  Positive cells are one class, negative cells the other.  Two cells of a class belong to one population
    when a chain of entries of the connectivities graph joins them, read in either direction, through cells of that class
    (weak connectivity: the graph need not be symmetric; self loops and duplicate entries change nothing).  An entry is an
    edge whatever its value: an explicitly stored zero stays an entry of the resident graph and joins its two cells, as it
    does for ``scipy.sparse.csgraph.connected_components``; ``A.eliminate_zeros()`` beforehand removes such entries.

    Within a sign the populations are numbered by size descending, ties by their smallest cell index ascending: ``'pos1',
    'pos2', ..., 'neg1', ...`` -- the same sets of cells whatever order the cells are stored in.  Populations of fewer than
    ``min_cells`` cells are not labelled; of the rest at most ``max_populations`` over both signs (largest first, then
    smallest cell index, then pos before neg), the others left unlabelled with a UserWarning that says how many.  The default
    1024 is the most levels the ``*_strata`` tools take, so the column always goes into them:
    ``nam_strata(data, key_added, sid)`` is the abundance of every population per sample,
    ``gene_corr_strata(data, key_added, key)`` the genes inside each, and mean, median and sd of the coefficient per
    population are ``coef_strata(data, key_added, key=key)`` -- they are not computed here.

    The column is a pandas Categorical (categories = the labels in the frame's order), NaN for a cell in no labelled
    population.  The frame has the labels as index and the columns ``sign`` (int8, +1 / -1), ``n_cells`` (int64),
    ``first_cell`` (the ``obs_names`` entry of the population's smallest-index cell) and ``frac`` (``n_cells`` over the
    selected cells of that sign).  With no cell selected the frame is empty and the column all NaN.
    ``return_info=True`` returns ``(frame, info)``: ``n_selected`` and ``n_populations`` (before the filters), each
    ``{'pos', 'neg'}``, and ``n_unlabelled_cells``, the selected cells without a label."""
    engine = engine or get_engine()
    refuse_sharded(data, engine, 'coef_populations', 'a population can cross row blocks: a union across ranks needs a halo '
                                                     'protocol of its own')
    obs = data.obs
    pos, neg = signed_passes(obs, key, fdr_thresh)
    if isinstance(min_cells, bool) or int(min_cells) != min_cells or int(min_cells) < 1:
        raise ValueError('coef_populations: min_cells must be an integer >= 1, got %r' % (min_cells,))
    if isinstance(max_populations, bool) or int(max_populations) != max_populations or int(max_populations) < 1:
        raise ValueError('coef_populations: max_populations must be an integer >= 1, got %r' % (max_populations,))
    min_cells, max_populations = int(min_cells), int(max_populations)
    key_added = '%s_pop' % (key,) if key_added is None else key_added
    n = len(obs)
    codes = np.full(n, -1, dtype=np.int32)
    codes[pos] = 0
    codes[neg] = 1
    n_selected = np.array([np.count_nonzero(pos), np.count_nonzero(neg)], dtype=np.int64)
    if n_selected.sum() == 0:
        comp = codes
        lst = {'class': np.empty(0, dtype=np.int32), 'size': np.empty(0, dtype=np.int64), 'first': np.empty(0, dtype=np.int64)}
        totals = np.zeros(2, dtype=np.int64)
    else:
        A = _as_csr(get_connectivity(data))
        if engine.ensure_graph(A, shard=shard_of(data)):
            engine._nam_sig = None          # new graph: whatever NAM the device holds is stale
        comp, lst, totals = engine.graph_components(codes, min_cells=min_cells, n_classes=2)
    cls = np.asarray(lst['class'], dtype=np.int64)
    size = np.asarray(lst['size'], dtype=np.int64)
    first = np.asarray(lst['first'], dtype=np.int64)
    K = len(cls)
    # the engine's list is sorted by class, size descending, smallest cell: the frame's order
    keep = np.ones(K, dtype=bool)
    if K > max_populations:
        keep[:] = False
        keep[np.lexsort((cls, first, -size))[:max_populations]] = True
        warnings.warn('coef_populations: %d populations of at least %d cells, the %d largest are labelled and %d are not '
                      '(max_populations)' % (K, min_cells, max_populations, K - max_populations), UserWarning, stacklevel=2)
    new_code = np.full(K + 1, -1, dtype=np.int64)             # [-1] serves the cells without a component
    new_code[:K][keep] = np.arange(int(keep.sum()))
    cls, size, first = cls[keep], size[keep], first[keep]
    number = np.arange(len(cls)) + 1 - np.where(cls == 0, 0, np.count_nonzero(cls == 0))      # pos first, then neg
    labels = ['%s%d' % (SIGNS[int(c)], int(k)) for c, k in zip(cls, number)]
    obs[key_added] = pd.Categorical.from_codes(new_code[np.asarray(comp, dtype=np.int64)], categories=labels)
    with np.errstate(invalid='ignore', divide='ignore'):
        frac = size / n_selected[cls].astype(np.float64)
    frame = pd.DataFrame({'sign': np.where(cls == 0, 1, -1).astype(np.int8), 'n_cells': size,
                          'first_cell': np.asarray(obs.index)[first] if len(first) else np.empty(0, dtype=object), 'frac': frac},
                         index=pd.Index(labels, name=key_added), columns=['sign', 'n_cells', 'first_cell', 'frac'])
    if not return_info:
        return frame
    totals = np.asarray(totals, dtype=np.int64)
    info = {'n_selected': dict(zip(SIGNS, (int(v) for v in n_selected))),
            'n_populations': dict(zip(SIGNS, (int(v) for v in totals[:2]))),
            'n_unlabelled_cells': int(n_selected.sum() - size.sum())}
    sweeps = getattr(engine, 'sweeps', None)
    if sweeps is not None and n_selected.sum():
        info['sweeps'] = int(sweeps)
    return frame, info
