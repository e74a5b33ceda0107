#!/usr/bin/env python3
"""Time cna.tl.gene_markers_within's device path (Engine.gene_ranksum_within: one segmented radix sort of the resident matrix
with one more pass on the block of the entry's cell, then one workgroup per gene that takes the blocks in turn) against its
floor and the two routes it replaces, in the same process:

  (a) within   the new call, three runs, and its split under the library's event timers (cna_prof_*): keys / sort / the
               kernel over the blocks (timed under 'ranksum_rank') / copies back
  (b) pooled   one Engine.gene_ranksum_by call on the same level codes: the floor -- what the extra pass and the loop over
               the blocks cost on top of it
  (c) masked   the route before this entry: one Engine.gene_ranksum_by per block on codes set to -1 outside the block, the
               whole loop, at 50 blocks; the sum over the blocks of rank2 - n_sl (n_s + 1) is compared with (a)'s d2
  (d) host     scipy.stats.rankdata per block and gene on 16 threads, on --host-genes genes spread over the matrix and
               scaled to all genes; d2 on those genes is compared with (a)'s

  timeout 1100 tools/kbench_gene_markers_within.py [--out profiles/kbench_gene_markers_within.txt] [--reps 3]
                                                   [--host-genes 128]

2 000 genes, float32, 32 levels of unequal size (tools/kbench_gene_rank_corr_strata.py's, 3 % of the cells in none), 50 and
200 blocks of unequal size (2 % of the cells in none): 1M cells sparse (CSR, 5 % density), 200k cells sparse and 200k cells
dense.  Per route the median, the least and the spread (largest - least) of --reps runs after one warm-up run (the work
buffers grow in the first); the codes and the weights cross PCIe in every call and the results come back.  The verdict
compares the margin (median of the masked route - median of the new call) with the masked route's spread.  The kernel over
the blocks is set against the bytes it must move: every stored kept entry's 4-byte key and 4-byte cell read by the
forward and by the backward walk and the 4-byte level of its cell gathered in each, 2 x 12 bytes per entry, as a share of
8 TB/s; the sort against its bytes as in tools/kbench_gene_rank_corr_strata.py."""
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

from kbench_gene_rank_corr import profiled
from kbench_gene_rank_corr_strata import LEVELS, PEAK, THREADS, make_codes, stats
from kbench_pseudobulk import make_dense, make_csr

SHAPES = [('csr', 1000000, 2000, 100), ('csr', 200000, 2000, 100), ('dense', 200000, 2000, 0)]
BLOCKS = [50, 200]
MASKED_AT = 50


def make_blocks(n, B):
    rs = np.random.RandomState(7 + B)
    w = rs.gamma(2.0, size=B) + 0.2
    blocks = rs.choice(B, size=n, p=w / w.sum()).astype(np.int32)
    blocks[rs.rand(n) < 0.02] = -1
    return blocks


def host_route(X, codes, blocks, B, genes):
    """d2[levels, genes] from scipy's midranks inside every block, on THREADS threads"""
    kept = (codes >= 0) & (blocks >= 0)
    rows = [np.flatnonzero(kept & (blocks == s)) for s in range(B)]
    levels = [codes[r] for r in rows]
    Xc = sp.csc_matrix(X) if sp.issparse(X) else None
    t0 = time.perf_counter()

    def one(g):
        if Xc is None:
            full = X[:, g].astype(np.float64)
        else:
            full = np.zeros(X.shape[0])
            lo, hi = Xc.indptr[g], Xc.indptr[g + 1]
            full[Xc.indices[lo:hi]] = Xc.data[lo:hi]
        d2 = np.zeros(LEVELS)
        for r, lev in zip(rows, levels):
            if len(r):
                r2 = 2.0 * scipy.stats.rankdata(full[r], method='average')
                d2 += np.bincount(lev, weights=r2, minlength=LEVELS) - np.bincount(lev, minlength=LEVELS) * (len(r) + 1.0)
        return d2

    with ThreadPoolExecutor(THREADS) as pool:
        out = list(pool.map(one, genes))
    return np.stack(out, axis=1), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'kbench_gene_markers_within.txt'))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-genes', type=int, default=128)
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    from cna_amd.tools._gene_markers import within_weights
    eng = get_engine()
    lines = ['cna_gene_ranksum_within (Engine.gene_ranksum_within), %d levels, van Elteren weights, against (b) one pooled '
             'Engine.gene_ranksum_by call, (c) one Engine.gene_ranksum_by call per block on masked codes (at %d blocks) and (d) '
             'scipy.stats.rankdata per block on %d threads; %d runs after 1 warm-up run: median (least; spread = largest - least)'
             % (LEVELS, MASKED_AT, THREADS, a.reps)]
    for kind, n, g, per_row in SHAPES:
        X = make_dense(n, g, np.float32) if kind == 'dense' else make_csr(n, g, per_row, np.float32)
        entries = X.nnz if kind == 'csr' else n * g
        codes = make_codes(n)
        eng.ensure_expression(X)
        eng.pin_expression(X)
        lines.append('%s %d x %d float32, %d entries (%s)' % (kind, n, g, entries, eng.expression_shape()['format']))
        print(lines[-1], flush=True)

        def timed(f):
            ts, out = [], None
            for r in range(a.reps + 1):
                t0 = time.perf_counter()
                out = f()
                if r >= 1:
                    ts.append(time.perf_counter() - t0)
            return out, stats(ts)

        pooled, (b_ms, b_min, b_spread) = timed(lambda: eng.gene_ranksum_by(codes, LEVELS))
        pb = profiled(eng, lambda: eng.gene_ranksum_by(codes, LEVELS))
        lines.append('  (b) pooled: %.1f ms (%.1f; spread %.1f) = keys %.2f + sort %.2f + rank %.2f + copies back %.2f ms + host side'
                     % (b_ms, b_min, b_spread, pb('ranksum_keys'), pb('ranksum_sort'), pb('ranksum_rank'), pb('ranksum_fetch')))
        print(lines[-1], flush=True)
        for B in BLOCKS:
            blocks = make_blocks(n, B)
            kept = (codes >= 0) & (blocks >= 0)
            counts = np.bincount(blocks[kept].astype(np.int64) * LEVELS + codes[kept], minlength=B * LEVELS).reshape(B, LEVELS)
            w_num, w_tie, _, _ = within_weights(counts)

            def call():
                return eng.gene_ranksum_within(codes, LEVELS, blocks, B, w_num, w_tie)

            got, (a_ms, a_min, a_spread) = timed(call)
            p = profiled(eng, call)
            kept_entries = entries * float(kept.mean())
            sort_bytes = entries * (4 * (4 + 2 * (4 + 4)) + (4 + 2 * (4 + 4)))
            walk_bytes = 2 * kept_entries * (4 + 4 + 4)
            share = lambda b, ms: 100 * b / (ms * 1e-3) / PEAK if ms > 0 else float('nan')   # noqa: E731
            walk, sort = p('ranksum_rank'), p('ranksum_sort')
            line = ('  %3d blocks (%d .. %d kept cells): (a) within %.1f ms (%.1f; spread %.1f) = keys %.2f + sort %.2f (%.2f GB: '
                    '%.1f %% of 8 TB/s) + kernel over the blocks %.2f (%.2f GB: %.1f %%) + copies back %.2f ms + host side (the '
                    'pass over the codes and their upload); (a) / (b) = %.2fx; the kernel over the blocks costs %s the sort (%.0f %% '
                    'against %.0f %% of the call)'
                    % (B, counts.sum(axis=1).min(), counts.sum(axis=1).max(), a_ms, a_min, a_spread, p('ranksum_keys'), sort,
                       sort_bytes / 1e9, share(sort_bytes, sort), walk, walk_bytes / 1e9, share(walk_bytes, walk),
                       p('ranksum_fetch'), a_ms / b_ms, 'MORE than' if walk > sort else 'less than', 100 * walk / a_ms,
                       100 * sort / a_ms))
            if B == MASKED_AT:
                def masked():
                    """-> the summed D and the seconds inside the calls: building a block's masked codes is not timed"""
                    total, dt = np.zeros_like(got[0]), 0.0
                    for s in range(B):
                        cs = np.where(blocks == s, codes, -1).astype(np.int32)
                        t0 = time.perf_counter()
                        rank2, _, nl, _ = eng.gene_ranksum_by(cs, LEVELS)
                        dt += time.perf_counter() - t0
                        total += rank2 - (nl * (nl.sum() + 1))[:, None]
                    return total, dt

                ts, total = [], None
                for r in range(a.reps + 1):
                    total, dt = masked()
                    if r >= 1:
                        ts.append(dt)
                c_ms, c_min, c_spread = stats(ts)
                margin = c_ms - a_ms
                verdict = 'FASTER beyond that spread' if margin > c_spread else 'NOT faster beyond that spread'
                line += ('; (c) %d masked calls %.1f ms (%.1f; spread %.1f): margin %.1f ms, %.1fx, %s; d2 %s'
                         % (B, c_ms, c_min, c_spread, margin, c_ms / a_ms, verdict,
                            'EQUAL' if np.array_equal(total, got[0]) else 'DIFFERS'))
            else:
                line += '; (c) not measured at %d blocks' % B
            genes = np.unique(np.linspace(0, g - 1, a.host_genes).astype(np.int64))
            want, dt = host_route(X, codes, blocks, B, genes)
            host_ms = dt / len(genes) * g * 1e3
            line += ('; (d) host route %.2f s for %d genes = %.1f s for all %d (scaled); host / device = %.0fx; d2 on those genes %s'
                     % (dt, len(genes), host_ms / 1e3, g, host_ms / a_ms,
                        'EQUAL' if np.array_equal(want, got[0][:, genes].astype(np.float64)) else 'DIFFERS'))
            lines.append(line)
            print(line, flush=True)
        eng.unpin_expression()
        eng.drop_expression()
        del X
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
