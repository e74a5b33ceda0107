#!/usr/bin/env python3
"""Time cna.tl.gene_markers_pairs' device path (Engine.gene_ranksum_pairs: one segmented radix sort of the resident matrix,
then the pairs kernel) against the route there was before it -- one Engine.gene_ranksum_by per pair on codes recoded to
{level -> 0, versus -> 1, everything else -> -1}, a full sort each -- in the same process.  One GPU, one process:

  timeout 900 tools/kbench_gene_markers_pairs.py [--out profiles/kbench_gene_markers_pairs.txt] [--reps 5]

The shapes of kbench_gene_markers.py, 2 000 genes and 32 levels of unequal size, 3 % of the cells left out: 1M and 200k cells
sparse (CSR, 5 % density, float32 counts 1..5: five tie groups and the implicit zeros per gene), 200k cells dense float32
from kbench_pseudobulk's generator (its rows repeat every BLOCK cells: tie groups of about n / BLOCK cells), and 200k cells
dense float32 of distinct normal floats (tie groups of one).  For P = 1 (the two largest levels), 31 (every level against
the largest, `reference=`) and 496 (all unordered pairs) with all 32 levels taking part, and for the P = 1 pair with only
its two levels taking part (what cna.tl.gene_markers_pairs sends for one pair):

  new    the median of --reps whole calls after two warm-up calls (codes and pairs cross PCIe, the P x genes results come
         back), and its split from one further call under the library's event timers (cna_prof_*): key build, the sort's
         passes, the pairs kernel, the copies back
  before the median of --reps runs of P calls of gene_ranksum_by; the recoded codes are made outside the timed region.  For
         P = 496 the 31 calls of the P = 31 list are timed and scaled by 496 / 31: every such call costs the same sort
The integers of both routes are compared on the P = 1 and P = 31 lists."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from kbench_pseudobulk import make_dense, make_csr

SHAPES = [('csr', 1000000, 2000, 100), ('csr', 200000, 2000, 100), ('dense', 200000, 2000, 0), ('dense-distinct', 200000, 2000, 0)]


def make_distinct(n, g):
    rng = np.random.default_rng(0)
    X = np.empty((n, g), dtype=np.float32)
    for r in range(0, n, 20000):
        X[r:r + 20000] = rng.standard_normal((min(20000, n - r), g), dtype=np.float32)
    return X


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'kbench_gene_markers_pairs.txt'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--levels', type=int, default=32)
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    eng = get_engine()
    L = a.levels
    lists = {1: [(L - 1, L - 2)], L - 1: [(l, L - 1) for l in range(L - 1)],
             L * (L - 1) // 2: [(x, y) for x in range(L) for y in range(x + 1, L)]}
    lines = ['cna_gene_ranksum_pairs (Engine.gene_ranksum_pairs, one sort for all pairs) against one cna_gene_ranksum_by per pair on '
             'recoded codes (a sort per pair); %d levels, median of %d' % (L, a.reps)]
    for kind, n, g, per_row in SHAPES:
        if kind == 'csr':
            X = make_csr(n, g, per_row, np.float32)
        else:
            X = make_dense(n, g, np.float32) if kind == 'dense' else make_distinct(n, g)
        entries = X.nnz if kind == 'csr' else n * g
        rs = np.random.RandomState(1)
        w = np.arange(1, L + 1, dtype=np.float64) ** 2
        codes = rs.choice(L, size=n, p=w / w.sum()).astype(np.int32)
        codes[rs.rand(n) < 0.03] = -1
        eng.ensure_expression(X)
        eng.pin_expression(X)
        lines.append('%s %d x %d float32, %d entries (%s)' % (kind, n, g, entries, eng.expression_shape()['format']))
        print(lines[-1], flush=True)
        recoded = {p: np.where(codes == p[0], 0, np.where(codes == p[1], 1, -1)).astype(np.int32) for p in lists[L - 1] + lists[1]}
        before_31 = None
        for P, pairs in [(0, lists[1])] + list(lists.items()):
            idx = np.array(pairs, dtype=np.int32)
            if P == 0:          # one pair as cna.tl.gene_markers_pairs sends it: only the two levels take part

                def call():
                    return eng.gene_ranksum_pairs(recoded[pairs[0]], 2, np.array([(0, 1)], dtype=np.int32))
            else:

                def call():
                    return eng.gene_ranksum_pairs(codes, L, idx)

            call()
            got = call()
            ms = median_ms(call, a.reps)
            eng.prof_enable(True)
            eng.prof_reset()
            call()
            prof = eng.prof()
            eng.prof_enable(False)
            part = {k: prof.get('ranksum_' + k, (0.0, 0))[0] for k in ('keys', 'sort', 'pairs', 'fetch')}
            name = 'P = %3d' % P if P else 'P = 1, 2 levels'
            P = max(P, 1)
            timed = pairs if P <= L - 1 else lists[L - 1]

            def before():
                return [eng.gene_ranksum_by(recoded[p], 2) for p in timed]

            ref = before()
            if P <= L - 1:
                before_ms = median_ms(before, a.reps)
                if P == L - 1:
                    before_31 = before_ms
                how = '%d calls timed' % P
                same = all((r[0][0] - r[2][0] * (r[2][0] + 1) == got[0][k]).all() and (r[1] == got[1][k]).all()
                           for k, r in enumerate(ref))
                verdict = '; integers of both routes %s' % ('EQUAL' if same else 'DIFFER')
            else:
                before_ms = before_31 * P / (L - 1)
                how = 'the %d calls of the list above, scaled by %d / %d' % (L - 1, P, L - 1)
                verdict = ''
            lines.append('  %s: new %.1f ms = keys %.2f + sort %.2f + pairs %.2f + copies back %.2f ms + host side, codes and '
                         'pairs; the pairs kernel is %.0f %% of the call and %.2fx the sort; before %.1f ms (%s); before / new = '
                         '%.2fx%s' % (name, ms, part['keys'], part['sort'], part['pairs'], part['fetch'], 100 * part['pairs'] / ms,
                                      part['pairs'] / part['sort'] if part['sort'] > 0 else float('nan'), before_ms, how,
                                      before_ms / ms, verdict))
            print(lines[-1], flush=True)
        eng.unpin_expression()
        eng.drop_expression()
        del X
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
