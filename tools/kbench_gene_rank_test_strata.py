#!/usr/bin/env python3
"""Time cna.tl.gene_rank_test_strata's device path (Engine.gene_rank_corr_x_by: the null coefficients formed from X on the
device, ranked inside every level in groups of 16, ONE sort of the resident matrix ending on the level, a rank kernel per
(gene, level) and a dot kernel per (gene, group, level) behind it) against the route that exists without it: one
Engine.gene_rank_corr_x call per level with xrow set to -1 outside the level, each sorting the matrix, and forming and
ranking every column, again.  Both routes are measured in this process, on the same library.  One GPU, one process:

  timeout 1100 tools/kbench_gene_rank_test_strata.py [--out profiles/kbench_gene_rank_test_strata.txt] [--runs 3]
                                                     [--only csr|dense] [--qs 16,208,1008]

2 000 genes, float32: 1M cells sparse (CSR, 5 % density) and 200k cells dense; X of 100 samples, standard normal, with a row
for 97 % of the cells (tools/kbench_gene_rank_test.py's); 32 levels of unequal size (a cell's level is drawn with weights
1 .. 32, so the largest level holds 32 times the cells of the smallest); q = 16, 208 and 1 008 columns (Z standard normal).
Every figure is a whole call: Z, xrow and the codes cross PCIe in it and the results come back (16 x levels x q x genes
bytes for the new entry: 1.03 GB at q = 1 008).  --runs whole calls after one warm-up call (the work buffers grow in the
first): the median and the spread (min .. max) are printed for both routes.

The split of the new entry comes from one further call under the library's event timers (cna_prof_*), whose ids are those
of cna_gene_rank_corr_x (the enum is pinned by the existing tests):
  rankcorr_keys   the column kernel, the columns' rank kernel inside the levels, the memsets of the tables, the codes
  ranksum_keys    the key builds (columns and matrix)
  ranksum_sort    the sort passes (columns: per group, nine passes; matrix: once, five passes for float32)
  ranksum_rank    the rank kernel: a = s + e - m_l per stored entry, one workgroup per (gene, level)
  rankcorr_corr   the dot kernel, one workgroup per (gene, group, level)
  ranksum_fetch   the copies back
The dot kernel's share of 8 TB/s is on the bytes it must move: per stored entry of a kept cell that lies in a level, and
per group, 4 (a) + 4 (cell) + 64 (the cell's row of the group's table).

Every level of the new entry is compared with the masked call at q = 16: the same integers."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
sys.path.insert(0, HERE)
import numpy as np

from kbench_gene_rank_corr import profiled
from kbench_gene_rank_test import PEAK, SAMPLES, SHAPES, make_x, runs_of
from kbench_pseudobulk import make_csr, make_dense

LEVELS = 32
QS = [16, 208, 1008]
SCOPES = ('rankcorr_keys', 'ranksum_keys', 'ranksum_sort', 'ranksum_rank', 'rankcorr_corr', 'ranksum_fetch')


def make_codes(n):
    """int32 per cell: 32 levels drawn with weights 1 .. 32, two cells in a hundred in no level"""
    rs = np.random.RandomState(7)
    w = np.arange(1, LEVELS + 1, dtype=np.float64)
    codes = rs.choice(LEVELS, size=n, p=w / w.sum()).astype(np.int32)
    codes[rs.rand(n) < 0.02] = -1
    return codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'kbench_gene_rank_test_strata.txt'))
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--only', default=None)
    ap.add_argument('--qs', default=','.join(map(str, QS)))
    a = ap.parse_args()
    qs = [int(v) for v in a.qs.split(',')]
    from cna_amd.engine import get_engine
    eng = get_engine()
    lines = ['cna_gene_rank_corr_x_by (Engine.gene_rank_corr_x_by) on %d levels against %d Engine.gene_rank_corr_x calls with xrow '
             'masked to one level each; median (min .. max) of %d whole calls after one warm-up call' % (LEVELS, LEVELS, a.runs)]

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')

    for kind, n, g, per_row in SHAPES:
        if a.only and a.only != kind:
            continue
        E = make_dense(n, g, np.float32) if kind == 'dense' else make_csr(n, g, per_row, np.float32)
        entries = E.nnz if kind == 'csr' else n * g
        X, xrow, took = make_x(n)
        codes = make_codes(n)
        in_level = took & (codes >= 0)
        sizes = np.bincount(codes[in_level], minlength=LEVELS)
        masked = [np.where(codes == l, xrow, -1) for l in range(LEVELS)]
        eng.ensure_expression(E)
        eng.pin_expression(E)
        eng.upload_x(X)
        kept_entries = entries * float(in_level.mean())
        say('%s %d x %d float32, %d entries (%s), X %d x %d, %d cells in a level with a row, levels of %d .. %d cells'
            % (kind, n, g, entries, eng.expression_shape()['format'], X.shape[0], SAMPLES, int(in_level.sum()), sizes.min(), sizes.max()))
        rs = np.random.RandomState(5)
        Zall = rs.standard_normal((max(qs), SAMPLES))
        for q in qs:
            Z = np.ascontiguousarray(Zall[:q])
            groups = (q + 15) // 16

            def new_call():
                return eng.gene_rank_corr_x_by(xrow, Z, codes, LEVELS)

            def old_route():
                return [eng.gene_rank_corr_x(masked[l], Z) for l in range(LEVELS)]

            got, ms, lo, hi = runs_of(new_call, a.runs)
            p = profiled(eng, new_call)
            prof = {k: p(k) for k in SCOPES}
            old, old_ms, old_lo, old_hi = runs_of(old_route, a.runs)
            po = profiled(eng, old_route)
            prof_old = {k: po(k) for k in SCOPES}
            if q == qs[0]:
                ok = ~got[5]
                same = all(np.array_equal(got[0][l][:, ok], old[l][0][:, ok]) and np.array_equal(got[1][l][:, ok], old[l][1][:, ok])
                           and np.array_equal(got[2][l][ok], old[l][2][ok]) and np.array_equal(got[3][l], old[l][3])
                           and int(got[4][l]) == old[l][4] for l in range(LEVELS))
                say('  every level against Engine.gene_rank_corr_x under the masked xrow: %s' % ('the same integers' if same else 'DIFFERS'))
            del got, old
            dot_bytes = kept_entries * groups * 72.0
            dot = prof['rankcorr_corr']
            total = sum(prof.values())
            say("  q = %4d (%2d groups): new entry %.1f ms (%.1f .. %.1f) = columns' side %.2f + key build %.2f + sort %.2f + rank "
                "kernel %.2f + dot kernel %.2f + copies back %.2f ms (of the timed %.1f ms: sort %.0f %%, rank %.0f %%, dot %.0f %%); "
                "the dot kernel moves %.2f GB: %.1f %% of 8 TB/s"
                % (q, groups, ms, lo, hi, prof['rankcorr_keys'], prof['ranksum_keys'], prof['ranksum_sort'], prof['ranksum_rank'], dot,
                   prof['ranksum_fetch'], total, 100 * prof['ranksum_sort'] / total, 100 * prof['ranksum_rank'] / total, 100 * dot / total,
                   dot_bytes / 1e9, 100 * dot_bytes / (dot * 1e-3) / PEAK if dot > 0 else float('nan')))
            wins = hi < old_lo
            loses = lo > old_hi
            say("            the %d masked calls: %.1f ms (%.1f .. %.1f) = columns' side %.2f + key build %.2f + sort %.2f + rank kernel "
                "%.2f + dot kernel %.2f + copies back %.2f ms; masked calls / new entry = %.2fx (%s)"
                % (LEVELS, old_ms, old_lo, old_hi, prof_old['rankcorr_keys'], prof_old['ranksum_keys'], prof_old['ranksum_sort'],
                   prof_old['ranksum_rank'], prof_old['rankcorr_corr'], prof_old['ranksum_fetch'], old_ms / ms,
                   'beyond the spread of both' if wins else
                   'the new entry is SLOWER, beyond the spread of both' if loses else
                   'NOT beyond the spread: new entry %.1f .. %.1f ms, masked calls %.1f .. %.1f ms' % (lo, hi, old_lo, old_hi)))
        eng.unpin_expression()
        eng.drop_expression()
        del E, X


if __name__ == '__main__':
    main()
