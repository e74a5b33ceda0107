#!/usr/bin/env python3
"""Time cna.tl.gene_rank_test's device path (Engine.gene_rank_corr_x: the null coefficients formed from X on the device and
ranked in groups of 16, ONE sort of the resident matrix, a rank kernel and a dot kernel behind it) against the route that
exists without it: ceil(q / 16) calls of Engine.gene_rank_corr, each on 16 columns formed by numpy from Engine.x_full() and
uploaded, each sorting the matrix again.  One GPU, one process:

  timeout 1100 tools/kbench_gene_rank_test.py [--out profiles/kbench_gene_rank_test.txt] [--runs 3] [--only csr|dense]

2 000 genes, float32: 1M cells sparse (CSR, 5 % density) and 200k cells dense; X of 100 samples, standard normal, with a row
for 97 % of the cells in ascending order (xrow = -1 for the others); q = 16, 208 and 1 008 columns (Z standard normal).  Every
figure is a whole call: Z and xrow cross PCIe in it and the results come back.  --runs whole calls after one warm-up call
(the work buffers grow in the first): the median and the spread (min .. max) are printed.  The loop of calls is timed the same
way, the host product (X @ Z_group^T and the scatter into a NaN-filled 16 x cells array) and the device calls separately.

The split comes from one further call under the library's event timers (cna_prof_*).  The ids are those of
cna_gene_rank_corr (the enum is pinned by the existing tests), so two kinds of work share some of them; the tool takes them
apart by two profiled calls, q = 16 (one group) and the q at hand: per further group the difference / (groups - 1) is the
columns' share, the rest the matrix'.
  rankcorr_keys   the column kernel, the columns' rank kernel, the memsets of the tables (per group).  The column kernel
                  alone is timed by a profiled Engine.x_columns call on 16 columns
  ranksum_keys    the columns' key build (per group) | the matrix' key build (once)
  ranksum_sort    the columns' sort passes (per group) | the matrix' sort passes (once)
  ranksum_rank    the rank kernel: a = s + e - m per stored entry (once)
  rankcorr_corr   the dot kernel (once per group, one launch per tile of genes)
  ranksum_fetch   the copies back
The dot kernel's share of 8 TB/s is on the bytes it must move: per stored kept entry and group 4 (a) + 4 (cell) + 64 (the
cell's row of the group's table).

Group 0 of the new entry is compared with Engine.gene_rank_corr on Engine.x_columns' first 16 columns: the same integers."""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
sys.path.insert(0, HERE)
import numpy as np

from kbench_gene_rank_corr import profiled
from kbench_pseudobulk import make_csr, make_dense

PEAK = 8e12
SAMPLES = 100
SHAPES = [('csr', 1000000, 2000, 100), ('dense', 200000, 2000, 0)]
QS = [16, 208, 1008]


def make_x(n):
    rs = np.random.RandomState(3)
    took = rs.rand(n) >= 0.03
    nx = int(took.sum())
    xrow = np.full(n, -1, dtype=np.int64)
    xrow[took] = np.arange(nx)
    return rs.standard_normal((nx, SAMPLES)), xrow, took


def runs_of(call, runs):
    call()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        got = call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return got, float(np.median(ts)), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'kbench_gene_rank_test.txt'))
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--only', default=None)
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    eng = get_engine()
    lines = ['cna_gene_rank_corr_x (Engine.gene_rank_corr_x) against ceil(q / 16) Engine.gene_rank_corr calls on columns formed by '
             'numpy from Engine.x_full(); median (min .. max) of %d whole calls after one warm-up call' % a.runs]

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
        eng.ensure_expression(E)
        eng.pin_expression(E)
        eng.upload_x(X)
        kept_entries = entries * float(took.mean())
        say('%s %d x %d float32, %d entries (%s), X %d x %d, %d cells kept' % (kind, n, g, entries, eng.expression_shape()['format'],
                                                                           X.shape[0], SAMPLES, int(took.sum())))
        rs = np.random.RandomState(5)
        Zall = rs.standard_normal((max(QS), SAMPLES))
        first = {}
        for q in QS:
            Z = np.ascontiguousarray(Zall[:q])
            groups = (q + 15) // 16

            def new_call():
                return eng.gene_rank_corr_x(xrow, Z)

            got, ms, lo, hi = runs_of(new_call, a.runs)
            p = profiled(eng, new_call)
            prof = {k: p(k) for k in ('rankcorr_keys', 'ranksum_keys', 'ranksum_sort', 'ranksum_rank', 'rankcorr_corr', 'ranksum_fetch')}
            if q == QS[0]:
                first = dict(prof)
                pc = profiled(eng, lambda: eng.x_columns(xrow, Z))
                first['column'] = pc('rankcorr_keys')
                cols = eng.x_columns(xrow, Z)
                old = eng.gene_rank_corr(cols)
                same = all(np.array_equal(x, y) for x, y in zip(got[:4], old[:4])) and got[4] == old[4]
                say('  group 0 against Engine.gene_rank_corr on Engine.x_columns: %s' % ('the same integers' if same else 'DIFFERS'))
                del cols
            if groups > 1:
                per = {k: (prof[k] - first[k]) / (groups - 1) for k in ('ranksum_keys', 'ranksum_sort')}
            else:
                per = {k: float('nan') for k in ('ranksum_keys', 'ranksum_sort')}
            dot_bytes = kept_entries * groups * 72.0
            dot = prof['rankcorr_corr']
            say("  q = %4d (%2d groups): new entry %.1f ms (%.1f .. %.1f) = columns' side %.2f (per group %.2f; the column kernel "
                "alone %.2f per group) + key build %.2f (columns %.2f per group, matrix %.2f) + sort %.2f (columns %.2f per group, "
                "matrix %.2f) + rank kernel %.2f + dot kernel %.2f + copies back %.2f ms; the dot kernel moves %.2f GB: %.1f %% of "
                "8 TB/s"
                % (q, groups, ms, lo, hi, prof['rankcorr_keys'], prof['rankcorr_keys'] / groups, first['column'], prof['ranksum_keys'],
                   per['ranksum_keys'], prof['ranksum_keys'] - groups * per['ranksum_keys'] if groups > 1 else float('nan'),
                   prof['ranksum_sort'], per['ranksum_sort'],
                   prof['ranksum_sort'] - groups * per['ranksum_sort'] if groups > 1 else float('nan'), prof['ranksum_rank'], dot,
                   prof['ranksum_fetch'], dot_bytes / 1e9, 100 * dot_bytes / (dot * 1e-3) / PEAK if dot > 0 else float('nan')))

            # the route without the entry: per group the host product, then one gene_rank_corr call
            host_ms, dev_ms = [], []

            def old_route():
                Xf = eng.x_full()
                th = td = 0.0
                for k0 in range(0, q, 16):
                    t0 = time.perf_counter()
                    V = np.full((min(16, q - k0), n), np.nan)
                    V[:, took] = (Xf @ Z[k0:k0 + 16].T).T
                    t1 = time.perf_counter()
                    eng.gene_rank_corr(V)
                    td += time.perf_counter() - t1
                    th += t1 - t0
                host_ms.append(th * 1e3)
                dev_ms.append(td * 1e3)

            _, old_ms, old_lo, old_hi = runs_of(old_route, a.runs)
            host_ms, dev_ms = host_ms[1:], dev_ms[1:]
            wins = hi < old_lo
            say('            the loop of %d calls: %.1f ms (%.1f .. %.1f) = host product %.1f (%.1f .. %.1f) + device calls %.1f '
                '(%.1f .. %.1f) ms, X fetched once per loop on top; loop / new entry = %.2fx (%s)'
                % (groups, old_ms, old_lo, old_hi, float(np.median(host_ms)), min(host_ms), max(host_ms), float(np.median(dev_ms)),
                   min(dev_ms), max(dev_ms), old_ms / ms,
                   'beyond the spread of both' if wins else 'NOT beyond the spread: slowest new call %.1f ms, fastest loop %.1f ms' % (hi, old_lo)))
            say('            device side alone: the calls of the loop / the new entry = %.2fx' % (float(np.median(dev_ms)) / ms))
        eng.unpin_expression()
        eng.drop_expression()
        del E, X


if __name__ == '__main__':
    main()
