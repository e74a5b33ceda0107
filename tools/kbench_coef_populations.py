#!/usr/bin/env python3
"""Time cna.tl.coef_populations' device path (Engine.graph_components) and the scipy route of its restatement.

  kbench_coef_populations.py [--sizes 200000:15 1000000:30 2000000:30] [--samples 50] [--reps 5]
                             [--out profiles/kbench_coef_populations.txt]

Graphs from the device kNN builder (synth.make_dataset); per size two fields of classes:
  assoc    the cells cna.tl.association selects on the synthetic phenotype (finite non-zero coefficient, fdr <= 0.1),
           positive and negative
  all      every cell selected, one class: the whole graph is one population (or a few), the worst case for the union
Per case:
  call     the whole Engine.graph_components call (find, list, the host's sort of the list, label), wall clock, median of
           the repetitions after a warm-up, with the smallest and the largest
  H2D      the copy of the classes to the device          } HIP events on the library's stream (cna_prof_enable:
  hook / flat / check / tally / label   the kernels by stage   } components_*), mean per call; a call of r rounds runs hook,
  D2H      the copies of the list and of the labels back  } flat and check r times
           (hook includes the two flattenings between the first round's three hook launches)
  rounds   hook / flatten / check rounds of the call (`engine.sweeps`)
  host     the route of the restatement on this machine's host cores: per class scipy.sparse.csgraph.connected_components
           on A[cells][:, cells], then sizes, smallest indices and the ordering in numpy
           (tests/test_coef_populations_host.py, restated here so that the tool stands alone)
  GB/round what one round reads at the least: the row offsets and classes of every cell, the entries of the classed rows
           and the class of each entry's other end (hook and check), two parent words per same-class entry in the hook and
           one in the check, the classed cells' parents in the flatten; set against the 8 TB/s HBM peak over hook + flat +
           check of one round.  The gathers are 4-byte reads of 64-byte sectors: the bytes moved are several times that.
No pass / fail figure: the file records the numbers, the cases where the device route is not faster included."""
import argparse
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

HBM_PEAK = 8.0e12
STAGES = ('components_upload', 'components_hook', 'components_flatten', 'components_check', 'components_tally',
          'components_label', 'components_fetch')


def host_route(A, codes, min_cells=1, n_classes=2):
    """The restatement's route: what Engine.graph_components returns."""
    n = len(codes)
    pattern = sp.csr_matrix((np.ones(len(A.indices), dtype=np.int8), A.indices, A.indptr), shape=A.shape)
    totals = np.zeros(n_classes, dtype=np.int64)
    cls, size, first = [np.empty(0, dtype=np.int32)], [np.empty(0, dtype=np.int64)], [np.empty(0, dtype=np.int64)]
    found = np.full(n, -1, dtype=np.int64)
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
    place = np.full(len(cls) + 1, -1, dtype=np.int32)
    place[kept] = np.arange(len(kept), dtype=np.int32)
    return place[found], {'class': cls[kept], 'size': size[kept], 'first': first[kept]}, totals


def round_bytes(A, codes):
    """Least HBM bytes one round reads (module docstring), and the entries it looks at."""
    n = len(codes)
    deg = np.diff(A.indptr)
    classed = codes >= 0
    e_rows = int(deg[classed].sum())
    same = 0
    step = 1 << 22                                   # rows at a time: the entry-sized temporaries stay small
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        lo, hi = int(A.indptr[r0]), int(A.indptr[r1])
        row_cls = np.repeat(codes[r0:r1], deg[r0:r1])
        same += int(np.count_nonzero((row_cls >= 0) & (row_cls == codes[A.indices[lo:hi]])))
    hook = 12 * n + 8 * e_rows + 8 * same
    flat = 4 * n + 4 * int(classed.sum())
    check = 12 * n + 8 * e_rows + 4 * same
    return hook + flat + check, e_rows, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='+', default=['200000:15', '1000000:30', '2000000:30'], help='cells:k')
    ap.add_argument('--samples', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'kbench_coef_populations.txt'))
    a = ap.parse_args()
    import cna_amd as cna
    from cna_amd import synth
    from cna_amd.engine import get_engine
    eng = get_engine()
    lines = ['cna.tl.coef_populations, device path (Engine.graph_components: find + list + host sort of the list + label) against '
             'the scipy route of its restatement; ms.  scipy had %d host threads; connected_components uses one'
             % (int(os.environ.get('OMP_NUM_THREADS', os.cpu_count())),),
             '%9s %3s %6s | %9s %9s | %15s | %6s %6s %6s %6s %6s %6s %6s %2s | %9s %7s | %8s %6s | %s'
             % ('cells', 'k', 'field', 'selected', 'pops', 'call (min-max)', 'H2D', 'hook', 'flat', 'check', 'tally', 'label',
                'D2H', 'r', 'host', 'x call', 'GB/round', '% HBM', 'arrays')]
    for spec in a.sizes:
        n, k = (int(v) for v in spec.split(':'))
        data, meta = synth.make_dataset(n, a.samples, k=k, seed=0)
        A = data.obsp['connectivities']
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            cna.tl.association(data, meta['y'], 'id', Nnull=200, seed=0, engine=eng)
        eng.wait_reorder()
        eng.ensure_graph(A)                              # the device's cell order, where one was being computed, is adopted here
        v, f = data.obs['coef'].values, data.obs['coef_fdr'].values
        with np.errstate(invalid='ignore'):
            ok = np.isfinite(v) & (f <= 0.1)
        fields = {'assoc': np.where(ok & (v > 0), 0, np.where(ok & (v < 0), 1, -1)).astype(np.int32),
                  'all': np.zeros(n, dtype=np.int32)}
        for name, codes in fields.items():
            r = eng.graph_components(codes, n_classes=2)                 # warm-up: work buffers, code objects
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = eng.graph_components(codes, n_classes=2)
                ts.append(time.perf_counter() - t0)
            rounds = eng.sweeps
            eng.prof_reset()
            eng.prof_enable(True)
            for _ in range(a.reps):
                eng.graph_components(codes, n_classes=2)
            eng.prof_enable(False)
            p = eng.prof()
            st = [p[s][0] / a.reps if s in p else 0.0 for s in STAGES]
            t0 = time.perf_counter()
            w = host_route(A, codes)
            host = time.perf_counter() - t0
            same = (np.array_equal(r[0], w[0]) and all(np.array_equal(r[1][q], w[1][q]) for q in w[1])
                    and np.array_equal(r[2], w[2]))
            gb, e_rows, e_same = round_bytes(A, codes)
            call = float(np.median(ts))
            per_round = (st[1] + st[2] + st[3]) / max(rounds, 1)
            lines.append('%9d %3d %6s | %9d %9d | %6.2f (%5.2f-%5.2f) | %6.2f %6.2f %6.2f %6.2f %6.2f %6.2f %6.2f %2d | %9.1f %6.1fx | '
                         '%8.3f %5.1f%% | %s'
                         % (n, k, name, int((codes >= 0).sum()), len(r[1]['size']), call * 1e3, min(ts) * 1e3, max(ts) * 1e3,
                            st[0], st[1], st[2], st[3], st[4], st[5], st[6], rounds, host * 1e3, host / call, gb / 1e9,
                            100.0 * gb / (per_round * 1e-3) / HBM_PEAK, 'equal' if same else 'DIFFERENT'))
            lines.append('%9s %3s %6s   entries of classed rows %d, same-class entries %d, perm %s'
                         % ('', '', '', e_rows, e_same, 'adopted' if eng.perm is not None else 'none (caller order)'))
            print('\n'.join(lines[-2:]), flush=True)
        del data, A
    eng.drop_expression()
    text = '\n'.join(lines) + '\n'
    print(text, end='', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
