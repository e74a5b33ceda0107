#!/usr/bin/env python3
"""Time cna.tl.gene_set_test's device pass (Engine.enrichment_extremes: every gene set under every column of [r | null_r])
against a vectorised numpy route to the same numbers on the same machine.

  timeout -k 10 900 python tools/kbench_gene_sets.py [--shapes 20000x1001x1000,2000x101x200] [--reps 5] [--threads 16]
                                                     [--commit TEXT] [--out profiles/kbench_gene_sets.txt]

Per shape genes x columns x sets: R standard normal / 4 clipped to [-1, 1] (every gene valid), the sets' sizes log-uniform
in [15, 500], members drawn without replacement, weight 1.  "device" is the whole Engine.enrichment_extremes call -- R
(8 x genes x columns bytes) and the sets up over PCIe, the three kernels, the results back; "kernels" the library's own
spans around the position kernel and the extremes kernels (HIP events).  "numpy" per column: np.argsort(-r, kind='stable'),
the members' positions, one lexsort by (set, position), np.cumsum and np.add / np.maximum / np.minimum.reduceat per set,
the columns dealt to `--threads` threads (numpy's sorts release the interpreter lock).  Its running weight is one cumsum over
all members of a column minus the sum in front of the set, so the difference it reports against the device is its own
cancellation (~1e-11 at 140 000 members), not the device's error; tests/test_gpu_gene_sets.py holds the device to its bound.
No ratio is promised; the file says what was measured."""
import argparse
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def numpy_extremes(R, set_ptr, set_genes, threads):
    """(up, down) for all-finite R and weight 1, vectorised per column."""
    n_cols, G = R.shape
    n_sets = len(set_ptr) - 1
    sizes = np.diff(set_ptr)
    owner = np.repeat(np.arange(n_sets), sizes)
    first = set_ptr[:-1]
    j = np.arange(len(set_genes)) - np.repeat(first, sizes)               # 0-based place inside the set
    up, down = np.empty((n_cols, n_sets)), np.empty((n_cols, n_sets))

    def column(c):
        r = R[c]
        order = np.argsort(-r, kind='stable')
        pos = np.empty(G, dtype=np.int64)
        pos[order] = np.arange(G)
        p = pos[set_genes]
        by = np.lexsort((p, owner))                                       # by set, then by position
        p, w = p[by], np.abs(r[set_genes[by]])
        S = np.cumsum(w)
        before = np.repeat(S[first] - w[first], sizes)
        S = S - before                                                    # the running weight inside each set
        NR = np.repeat(np.add.reduceat(w, first), sizes)
        miss = (p - j) / np.repeat((G - sizes).astype(np.float64), sizes)
        up[c] = np.maximum.reduceat(S / NR - miss, first)
        down[c] = np.minimum.reduceat((S - w) / NR - miss, first)
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(column, range(n_cols)))
    return up, down


def median_time(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def head_commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        return subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=root, capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return 'unknown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='20000x1001x1000,2000x101x200')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--commit', default=None)
    ap.add_argument('--out', default=os.path.join('profiles', 'kbench_gene_sets.txt'))
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    eng = get_engine()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
    say('cna.tl.gene_set_test: Engine.enrichment_extremes against a vectorised numpy route on %d threads, weight 1, set sizes '
        'log-uniform in [15, 500], median of %d; commit %s' % (a.threads, a.reps, a.commit or head_commit()))
    for shape in a.shapes.split(','):
        G, n_cols, n_sets = (int(v) for v in shape.split('x'))
        rs = np.random.RandomState(G + n_cols)
        R = np.clip(rs.standard_normal((n_cols, G)) / 4.0, -1.0, 1.0)
        sizes = np.exp(rs.uniform(np.log(15.0), np.log(500.0), n_sets)).round().astype(np.int64)
        set_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        set_genes = np.concatenate([np.sort(rs.choice(G, m, replace=False)) for m in sizes]).astype(np.int32)
        say('%d genes x %d columns x %d sets: R is %.1f MB, %d members in all, %.3g pair tests, %.3g (column, set) walks'
            % (G, n_cols, n_sets, R.nbytes / 1e6, len(set_genes), float(G) * G * n_cols, float(n_cols) * n_sets))
        eng.enrichment_extremes(R, set_ptr, set_genes, 1)                   # warm-up: work buffers, code objects
        eng.prof_reset()
        eng.prof_enable(True)
        t_dev, got = median_time(lambda: eng.enrichment_extremes(R, set_ptr, set_genes, 1), a.reps)
        eng.prof_enable(False)
        prof = eng.prof()
        t_pos = prof['enrich_positions'][0] / prof['enrich_positions'][1] / 1e3
        t_ext = prof['enrich_extremes'][0] / prof['enrich_extremes'][1] / 1e3
        t_np, want = median_time(lambda: numpy_extremes(R, set_ptr, set_genes, a.threads), max(1, a.reps // 2))
        diff = max(float(np.max(np.abs(got[0] - want[0]))), float(np.max(np.abs(got[1] - want[1]))))
        say('  device call  %10.3f ms  (upload of R and the results back included); spans: positions %.3f ms (%.3g pair '
            'tests / s), extremes %.3f ms; positions / call = %.2f'
            % (t_dev * 1e3, t_pos * 1e3, float(G) * G * n_cols / t_pos, t_ext * 1e3, t_pos / t_dev))
        say('  numpy route  %10.3f ms  on %d threads: numpy / device = %.1f x; largest |difference| of up and down %.1e'
            % (t_np * 1e3, a.threads, t_np / t_dev, diff))
    eng.drop_expression()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
