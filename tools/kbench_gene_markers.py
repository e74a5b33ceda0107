#!/usr/bin/env python3
"""Time cna.tl.gene_markers' device path (Engine.gene_ranksum_by: one segmented radix sort of the resident matrix, then the
rank kernel) against the host route it replaces -- scipy.stats.rankdata per gene plus np.bincount per level, the same
integers -- on 16 threads.  One GPU, one process:

  timeout 900 tools/kbench_gene_markers.py [--out profiles/kbench_gene_markers.txt] [--reps 5] [--host-genes 128]

Three shapes, 2 000 genes and 32 levels of unequal size each: 200k and 1M cells sparse (CSR, 5 % density, float32 counts) and
200k cells dense float32 (kbench_pseudobulk's generators).  3 % of the cells are left out.  Each call figure is the median of
--reps whole calls after two warm-up calls (the work buffers grow in the first); the codes cross PCIe in it and the results
come back.  The split comes from one further call under the library's event timers (cna_prof_*): key build, the sort's
passes, the rank kernel, the copies back.  For the sort the achieved fraction of 8 TB/s is reported on the bytes a pass must
move: every entry's key and level read once and written once.  The host route is timed on --host-genes genes spread over the
matrix (the gene-major lists densified column by column, as a caller holding a CSC matrix would) and scaled to all genes;
its integers are compared with the device's on those genes (the tie terms, which exceed 2^53 at these sizes, to 1e-12)."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import scipy.stats

from kbench_pseudobulk import make_dense, make_csr

PEAK = 8e12
THREADS = 16
SHAPES = [('csr', 200000, 2000, 100), ('csr', 1000000, 2000, 100), ('dense', 200000, 2000, 0)]


def host_route(X, codes, L, genes):
    """rank2[L, genes] and the tie term by scipy.stats.rankdata and np.bincount, THREADS threads over the genes"""
    kept = codes >= 0
    c = codes[kept]
    Xc = sp.csc_matrix(X) if sp.issparse(X) else None

    def one(g):
        if Xc is None:
            col = X[kept, g].astype(np.float64)
        else:
            full = np.zeros(X.shape[0])
            lo, hi = Xc.indptr[g], Xc.indptr[g + 1]
            full[Xc.indices[lo:hi]] = Xc.data[lo:hi]
            col = full[kept]
        r2 = np.rint(2.0 * scipy.stats.rankdata(col, method='average'))
        t = np.unique(col, return_counts=True)[1].astype(np.float64)
        return np.rint(np.bincount(c, weights=r2, minlength=L)).astype(np.int64), float((t * (t * t - 1.0)).sum())

    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as pool:
        out = list(pool.map(one, genes))
    dt = time.perf_counter() - t0
    return np.stack([o[0] for o in out], axis=1), np.array([o[1] for o in out]), dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'kbench_gene_markers.txt'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-genes', type=int, default=128)
    ap.add_argument('--levels', type=int, default=32)
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    eng = get_engine()
    lines = ['cna_gene_ranksum_by (Engine.gene_ranksum_by) against scipy.stats.rankdata + np.bincount on %d threads; %d levels, '
             'median of %d calls' % (THREADS, a.levels, a.reps)]
    for kind, n, g, per_row in SHAPES:
        X = make_dense(n, g, np.float32) if kind == 'dense' else make_csr(n, g, per_row, np.float32)
        entries = X.nnz if kind == 'csr' else n * g
        rs = np.random.RandomState(1)
        w = np.arange(1, a.levels + 1, dtype=np.float64) ** 2
        codes = rs.choice(a.levels, size=n, p=w / w.sum()).astype(np.int32)
        codes[rs.rand(n) < 0.03] = -1
        eng.ensure_expression(X)
        eng.pin_expression(X)

        def call():
            return eng.gene_ranksum_by(codes, a.levels)

        call()
        call()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = call()
            ts.append(time.perf_counter() - t0)
        ms = float(np.median(ts)) * 1e3
        eng.prof_enable(True)
        eng.prof_reset()
        call()
        prof = eng.prof()
        eng.prof_enable(False)
        part = {k: prof.get('ranksum_' + k, (0.0, 0))[0] for k in ('keys', 'sort', 'rank', 'fetch')}
        passes = 4
        pass_bytes = entries * 2 * (4 + 2)
        sort_frac = passes * pass_bytes / (part['sort'] * 1e-3) / PEAK if part['sort'] > 0 else float('nan')
        genes = np.unique(np.linspace(0, g - 1, a.host_genes).astype(np.int64))
        want, wtie, dt = host_route(X, codes, a.levels, genes)
        same = bool((got[0][:, genes] == want).all() and np.allclose(got[1][genes], wtie, rtol=1e-12, atol=0))   # tie terms pass 2^53 here
        host_ms = dt / len(genes) * g * 1e3
        lines.append('%s %d x %d float32, %d entries (%s): call %.1f ms (min %.1f) = keys %.2f + sort %.2f + rank %.2f + copies back '
                     '%.2f ms + host side and the codes; a sort pass moves %.2f GB, the %d passes reach %.1f %% of 8 TB/s; host route '
                     '%.2f s for %d genes = %.1f s for all %d (scaled); host / device = %.0fx; integers on those genes %s'
                     % (kind, n, g, entries, eng.expression_shape()['format'], ms, min(ts) * 1e3, part['keys'], part['sort'],
                        part['rank'], part['fetch'], pass_bytes / 1e9, passes, 100 * sort_frac, dt, len(genes), host_ms / 1e3, g,
                        host_ms / ms, 'EQUAL' if same else 'DIFFER'))
        print(lines[-1], flush=True)
        eng.unpin_expression()
        eng.drop_expression()
        del X
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
