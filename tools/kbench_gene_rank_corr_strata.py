#!/usr/bin/env python3
"""Time cna.tl.gene_rank_corr_strata's device path (Engine.gene_rank_corr_by: the keys' ranks inside every level, one
segmented radix sort of the resident matrix with one more pass on the level, then one correlation workgroup per (gene,
level)) against the two routes it replaces, in the same process:

  masked   one Engine.gene_rank_corr call per level with the keys set to NaN outside it: the same integers (compared here,
           level by level), one whole sort of the matrix per level
  host     scipy.stats.rankdata per gene and level and one dot product per key on 16 threads, on --host-genes genes spread
           over the matrix and scaled to all genes

  timeout 1100 tools/kbench_gene_rank_corr_strata.py [--out profiles/kbench_gene_rank_corr_strata.txt] [--reps 5]
                                                     [--host-genes 32] [--include FILE ...]

2 000 genes, float32, 32 levels of unequal size (tools/kbench_gene_markers.py's, 3 % of the cells in none): 1M cells sparse
(CSR, 5 % density) and 200k cells dense; q = 1, 4 and 16 keys (heavy-tailed floats, 3 % of the cells NaN in key 0).  The one
call and the 32 masked calls ALTERNATE, --reps times after two warm-up rounds (the work buffers grow in the first): per
route the median, the least and the spread (largest - least) of those rounds; the keys cross PCIe in every call and the
results come back.  The verdict compares the margin (median of the masked route - median of the one call) with the masked
route's spread.  The split of the one call comes from one further call under the library's event timers (cna_prof_*); the
sort's and the correlation kernel's share of 8 TB/s is reported on the bytes each must move:
  keys' ranks   per key and cell the sorted {8-byte key, 4-byte cell} read and 4 bytes of the table written
  sort          per entry and value pass the key read for the count, key and cell read and written by the scatter; the pass
                on the level reads the cell instead of the key for its count (genes: 4 value passes of 4-byte keys; keys: 8
                of 8-byte keys)
  correlation   every stored kept entry's key and cell read twice (forward and backward walk) and its cell's row of 4 W
                bytes gathered twice, W the least of 1, 2, 4, 8, 16 that holds q
--include FILE appends other runs' lines (the sibling benchmarks at the parent commit and at this one) to the profile."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
sys.path.insert(0, HERE)
import numpy as np
import scipy.sparse as sp
import scipy.stats

from kbench_gene_rank_corr import make_keys, profiled
from kbench_pseudobulk import make_dense, make_csr

PEAK = 8e12
THREADS = 16
LEVELS = 32
SHAPES = [('csr', 1000000, 2000, 100), ('dense', 200000, 2000, 0)]
QS = [1, 4, 16]


def make_codes(n):
    rs = np.random.RandomState(1)
    w = np.arange(1, LEVELS + 1, dtype=np.float64) ** 2
    codes = rs.choice(LEVELS, size=n, p=w / w.sum()).astype(np.int32)
    codes[rs.rand(n) < 0.03] = -1
    return codes


def host_route(X, V, codes, genes):
    """S[level, q, genes] as float64 dot products of the centred, doubled ranks inside every level"""
    kept = np.isfinite(V).all(axis=0) & (codes >= 0)
    cells = [np.flatnonzero(kept & (codes == l)) for l in range(LEVELS)]
    Xc = sp.csc_matrix(X) if sp.issparse(X) else None
    t0 = time.perf_counter()
    b = [np.stack([2.0 * scipy.stats.rankdata(v[c]) - (len(c) + 1) for v in V]) for c in cells]

    def one(g):
        if Xc is None:
            full = X[:, g].astype(np.float64)
        else:
            full = np.zeros(X.shape[0])
            lo, hi = Xc.indptr[g], Xc.indptr[g + 1]
            full[Xc.indices[lo:hi]] = Xc.data[lo:hi]
        return np.stack([b[l].dot(2.0 * scipy.stats.rankdata(full[c], method='average') - (len(c) + 1))
                         for l, c in enumerate(cells)])

    with ThreadPoolExecutor(THREADS) as pool:
        out = list(pool.map(one, genes))
    dt = time.perf_counter() - t0
    return np.stack(out, axis=2), dt, [len(c) for c in cells]


def stats(ts):
    return float(np.median(ts)) * 1e3, min(ts) * 1e3, (max(ts) - min(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'kbench_gene_rank_corr_strata.txt'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-genes', type=int, default=32)
    ap.add_argument('--include', action='append', default=[])
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    from cna_amd.tools._gene_rank_corr import wide_to_float
    eng = get_engine()
    lines = ['cna_gene_rank_corr_by (Engine.gene_rank_corr_by), %d levels, against %d masked Engine.gene_rank_corr calls (the same '
             'integers) and scipy.stats.rankdata per level on %d threads; the two device routes alternate, %d rounds after 2 '
             'warm-up rounds: median (least; spread = largest - least)' % (LEVELS, LEVELS, THREADS, a.reps)]
    for kind, n, g, per_row in SHAPES:
        X = make_dense(n, g, np.float32) if kind == 'dense' else make_csr(n, g, per_row, np.float32)
        entries = X.nnz if kind == 'csr' else n * g
        codes = make_codes(n)
        eng.ensure_expression(X)
        eng.pin_expression(X)
        lines.append('%s %d x %d float32, %d entries (%s)' % (kind, n, g, entries, eng.expression_shape()['format']))
        print(lines[-1], flush=True)
        for q in QS:
            V = make_keys(n, q)
            W = [w for w in (1, 2, 4, 8, 16) if w >= q][0]

            def call():
                return eng.gene_rank_corr_by(V, codes, LEVELS)

            def masked():
                """-> the results and the seconds inside the calls: building a level's masked keys is not timed"""
                out, dt = [], 0.0
                for l in range(LEVELS):
                    Vl = np.where(codes == l, V, np.nan)
                    t0 = time.perf_counter()
                    out.append(eng.gene_rank_corr(Vl))
                    dt += time.perf_counter() - t0
                return out, dt

            t_new, t_old = [], []
            for r in range(a.reps + 2):
                t0 = time.perf_counter()
                got = call()
                t1 = time.perf_counter()
                old, dt = masked()
                if r >= 2:
                    t_new.append(t1 - t0)
                    t_old.append(dt)
            ok = ~got[5]
            same = all((got[0][l][:, ok] == old[l][0][:, ok]).all() and (got[1][l][:, ok] == old[l][1][:, ok]).all()
                       and (got[2][l][ok] == old[l][2][ok]).all() and (got[3][l] == old[l][3]).all() and got[4][l] == old[l][4]
                       for l in range(LEVELS))
            del old
            new_ms, new_min, new_spread = stats(t_new)
            old_ms, old_min, old_spread = stats(t_old)
            p = profiled(eng, call)
            kept_entries = entries * 0.97 * 0.97
            gene_sort = entries * (4 * (4 + 2 * (4 + 4)) + (4 + 2 * (4 + 4)))
            key_sort = q * n * (8 * (8 + 2 * (8 + 4)) + (4 + 2 * (8 + 4)))
            sort_bytes = gene_sort + key_sort
            corr_bytes = 2 * kept_entries * (4 + 4 + 4 * W)
            rank_bytes = q * n * 0.94 * (8 + 4 + 4)
            share = lambda b, ms: 100 * b / (ms * 1e-3) / PEAK if ms > 0 else float('nan')   # noqa: E731
            margin = old_ms - new_ms
            verdict = 'FASTER beyond that spread' if margin > old_spread else 'NOT faster beyond that spread'
            line = ('  q = %2d: one call %.1f ms (%.1f; spread %.1f) against %d masked calls %.1f ms (%.1f; spread %.1f): margin '
                    '%.1f ms, %.1fx, %s; integers of every level %s.  The one call = keys\' ranks %.2f (%.2f GB: %.1f %% of 8 '
                    'TB/s; the keys\' upload and the kept cells are in it) + key build %.2f + sort %.2f (genes and keys, %.2f GB: '
                    '%.1f %%) + correlation %.2f (%.2f GB: %.1f %%) + copies back %.2f ms + host side and the keys'
                    % (q, new_ms, new_min, new_spread, LEVELS, old_ms, old_min, old_spread, margin, old_ms / new_ms, verdict,
                       'EQUAL' if same else 'DIFFER', p('rankcorr_keys'), rank_bytes / 1e9, share(rank_bytes, p('rankcorr_keys')),
                       p('ranksum_keys'), p('ranksum_sort'), sort_bytes / 1e9, share(sort_bytes, p('ranksum_sort')),
                       p('rankcorr_corr'), corr_bytes / 1e9, share(corr_bytes, p('rankcorr_corr')), p('ranksum_fetch')))
            if q == QS[-1]:
                genes = np.unique(np.linspace(0, g - 1, a.host_genes).astype(np.int64))
                want, dt, sizes = host_route(X, V, codes, genes)
                S = np.stack([wide_to_float(got[0][l], got[1][l])[:, genes] for l in range(LEVELS)])
                full = np.array(sizes, dtype=np.float64)[:, None, None] ** 3 / 3.0        # S / full = rho without ties
                close = bool((np.abs(S - want) <= 1e-12 * full).all() and list(got[4]) == sizes)
                host_ms = dt / len(genes) * g * 1e3
                line += ('; host route %.2f s for %d genes = %.1f s for all %d (scaled); host / device = %.0fx; S on those genes %s'
                         % (dt, len(genes), host_ms / 1e3, g, host_ms / new_ms,
                            'EQUAL to 1e-12 of (m_l^3 - m_l) / 3' if close else 'DIFFERS'))
            lines.append(line)
            print(line, flush=True)
        eng.unpin_expression()
        eng.drop_expression()
        del X
    for path in a.include:
        lines.append('%s:' % os.path.basename(path))
        lines += ['  ' + l for l in open(path).read().splitlines()]
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
