#!/usr/bin/env python3
"""Time cna.tl.gene_rank_corr's device path (Engine.gene_rank_corr: the ranks of the keys, one segmented radix sort of the
resident matrix with the cell as the payload, then the correlation kernel) against the host route it replaces --
scipy.stats.rankdata per gene and one dot product per key, the same integers -- on 16 threads.  One GPU, one process:

  timeout 900 tools/kbench_gene_rank_corr.py [--out profiles/kbench_gene_rank_corr.txt] [--reps 5] [--host-genes 128]
  tools/kbench_gene_rank_corr.py --sort-baseline [--root OTHER_CHECKOUT] --out FILE     # gene_ranksum_by, one level, only

The shapes of tools/kbench_gene_markers.py, 2 000 genes each: 200k and 1M cells sparse (CSR, 5 % density, float32 counts) and
200k cells dense float32; q = 1, 4 and 16 keys (heavy-tailed floats, 3 % of the cells NaN in key 0: left out of the call).
Each call figure is the median of --reps whole calls after two warm-up calls (the work buffers grow in the first); the keys
cross PCIe in it and the results come back.  The split comes from one further call under the library's event timers
(cna_prof_*): the keys' ranks (upload, kept cells, the kernel behind their sort), key build and sort passes (genes AND keys:
they share the ids), the correlation kernel, the copies back.  For the correlation kernel the achieved fraction of 8 TB/s is
reported on the bytes it must move: every stored entry's key and cell read twice (forward and backward walk) and its cell's
row of 4 W bytes gathered twice, W the least of 1, 2, 4, 8, 16 that holds q.

The sort baseline is Engine.gene_ranksum_by with ONE level on the same matrix: the same keys and passes with a 2-byte
payload.  --sort-baseline times only that (it runs on a checkout from before this tool: --root names it) and --parent-sort
FILE puts such a run of the parent commit beside this commit's.  --include FILE appends other runs' lines (the marker
benchmarks at the parent commit and at this one) to the profile file.

The host route is timed on --host-genes genes spread over the matrix and scaled to all genes; its S is compared with the
device's on those genes, to 1e-12 of (m^3 - m) / 3 (the float64 dot product rounds)."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = HERE
if '--root' in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index('--root') + 1])
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp
import scipy.stats

from kbench_pseudobulk import make_dense, make_csr

PEAK = 8e12
THREADS = 16
SHAPES = [('csr', 200000, 2000, 100), ('csr', 1000000, 2000, 100), ('dense', 200000, 2000, 0)]
QS = [1, 4, 16]


def make_keys(n, q):
    rs = np.random.RandomState(7)
    V = rs.standard_cauchy((q, n))
    V[0, rs.rand(n) < 0.03] = np.nan
    return np.ascontiguousarray(V)


def host_route(X, V, genes):
    """S[q, genes] as float64 dot products of the centred, doubled ranks, by scipy.stats.rankdata and np.dot"""
    kept = np.isfinite(V).all(axis=0)
    m = int(kept.sum())
    Xc = sp.csc_matrix(X) if sp.issparse(X) else None
    t0 = time.perf_counter()
    b = np.stack([2.0 * scipy.stats.rankdata(v[kept]) - (m + 1) for v in V])

    def one(g):
        if Xc is None:
            col = X[kept, g].astype(np.float64)
        else:
            full = np.zeros(X.shape[0])
            lo, hi = Xc.indptr[g], Xc.indptr[g + 1]
            full[Xc.indices[lo:hi]] = Xc.data[lo:hi]
            col = full[kept]
        a = 2.0 * scipy.stats.rankdata(col, method='average') - (m + 1)
        return b.dot(a)

    with ThreadPoolExecutor(THREADS) as pool:
        out = list(pool.map(one, genes))
    dt = time.perf_counter() - t0
    return np.stack(out, axis=1), dt


def timed(call, reps):
    call()
    call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = call()
        ts.append(time.perf_counter() - t0)
    return got, float(np.median(ts)) * 1e3, min(ts) * 1e3


def profiled(eng, call):
    eng.prof_enable(True)
    eng.prof_reset()
    call()
    prof = eng.prof()
    eng.prof_enable(False)
    return lambda name: prof.get(name, (0.0, 0))[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'kbench_gene_rank_corr.txt'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-genes', type=int, default=128)
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--sort-baseline', action='store_true')
    ap.add_argument('--parent-sort', default=None)
    ap.add_argument('--include', action='append', default=[])
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    eng = get_engine()
    lines = []
    if not a.sort_baseline:
        lines.append('cna_gene_rank_corr (Engine.gene_rank_corr) against scipy.stats.rankdata + np.dot on %d threads; median of %d '
                     'calls' % (THREADS, a.reps))
    for kind, n, g, per_row in SHAPES:
        X = make_dense(n, g, np.float32) if kind == 'dense' else make_csr(n, g, per_row, np.float32)
        entries = X.nnz if kind == 'csr' else n * g
        eng.ensure_expression(X)
        eng.pin_expression(X)
        head = '%s %d x %d float32, %d entries (%s)' % (kind, n, g, entries, eng.expression_shape()['format'])
        one_level = np.zeros(n, dtype=np.int32)
        one_level[make_keys(n, 1)[0] != make_keys(n, 1)[0]] = -1          # the cells key 0 leaves out

        def base_call():
            return eng.gene_ranksum_by(one_level, 1)

        _, base_ms, base_min = timed(base_call, a.reps)
        p = profiled(eng, base_call)
        base_sort = p('ranksum_sort')
        lines.append('%s: sort baseline gene_ranksum_by, one level: call %.2f ms (min %.2f) = keys %.2f + sort %.2f + rank %.2f + '
                     'copies back %.2f ms' % (head, base_ms, base_min, p('ranksum_keys'), base_sort, p('ranksum_rank'),
                                               p('ranksum_fetch')))
        print(lines[-1], flush=True)
        if not a.sort_baseline:
            for q in QS:
                V = make_keys(n, q)
                W = [w for w in (1, 2, 4, 8, 16) if w >= q][0]

                def call():
                    return eng.gene_rank_corr(V)

                got, ms, mn = timed(call, a.reps)
                p = profiled(eng, call)
                kept_entries = entries * 0.97
                corr_bytes = 2 * kept_entries * (4 + 4 + 4 * W)
                corr = p('rankcorr_corr')
                frac = corr_bytes / (corr * 1e-3) / PEAK if corr > 0 else float('nan')
                line = ('  q = %2d: call %.1f ms (min %.1f) = keys\' ranks %.2f + key build %.2f + sort %.2f (genes and keys; %.2fx the '
                        'baseline\'s sort) + correlation %.2f + copies back %.2f ms + host side and the keys; the correlation kernel '
                        'moves %.2f GB: %.1f %% of 8 TB/s' % (q, ms, mn, p('rankcorr_keys'), p('ranksum_keys'), p('ranksum_sort'),
                                                             p('ranksum_sort') / base_sort, corr, p('ranksum_fetch'),
                                                             corr_bytes / 1e9, 100 * frac))
                if q == QS[-1]:
                    genes = np.unique(np.linspace(0, g - 1, a.host_genes).astype(np.int64))
                    want, dt = host_route(X, V, genes)
                    from cna_amd.tools._gene_rank_corr import wide_to_float
                    S = wide_to_float(got[0], got[1])[:, genes]
                    full = float(np.isfinite(V).all(axis=0).sum()) ** 3 / 3.0          # S / full = rho without ties
                    same = bool(np.abs(S - want).max() <= 1e-12 * full)
                    host_ms = dt / len(genes) * g * 1e3
                    line += ('; host route %.2f s for %d genes = %.1f s for all %d (scaled); host / device = %.0fx; S on those genes %s'
                             % (dt, len(genes), host_ms / 1e3, g, host_ms / ms, 'EQUAL to 1e-12 of (m^3 - m) / 3' if same else 'DIFFERS'))
                lines.append(line)
                print(line, flush=True)
        eng.unpin_expression()
        eng.drop_expression()
        del X
    if a.parent_sort:
        lines.append('the sort baseline at the parent commit (same session, tools/kbench_gene_rank_corr.py --sort-baseline --root):')
        lines += ['  ' + l for l in open(a.parent_sort).read().splitlines()]
    for path in a.include:
        lines.append('%s:' % os.path.basename(path))
        lines += ['  ' + l for l in open(path).read().splitlines()]
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
