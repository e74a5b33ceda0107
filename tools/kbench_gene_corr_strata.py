#!/usr/bin/env python3
"""Time cna.tl.gene_corr_strata's device path (Engine.gene_corr_by: one pass, the cell's level as the accumulator index)
against the emulation it replaces: ceil(q x levels / 16) calls of Engine.gene_corr with the keys masked to one level each,
sixteen such columns per call -- what the library could do before.  One GPU, one process per line:

  kbench_gene_corr_strata.py dense n_cells n_genes           [--levels 32] [--q 1] [--reps 10] [--f64]
  kbench_gene_corr_strata.py csr   n_cells n_genes per_row   [--levels 32] [--q 1] [--reps 10] [--f64]

  timeout 300 tools/kbench_gene_corr_strata.py dense 200000 2000 --q 1
  timeout 300 tools/kbench_gene_corr_strata.py dense 200000 2000 --q 4
  timeout 300 tools/kbench_gene_corr_strata.py csr 200000 2000 100 --q 1      (5 % density)
  timeout 300 tools/kbench_gene_corr_strata.py csr 200000 2000 100 --q 4

The matrix (kbench_pseudobulk's generators) is resident and pinned; cell i belongs to level `i % levels` of a random
permutation of the cells.  Each figure is the median of --reps whole calls after two warm-up calls (the work buffers grow in
the first): the keys and codes cross PCIe in it and the result comes back.  Prints per-call milliseconds of both, their
ratio, the largest difference between the two results, and the matrix' own bytes on the device over the call's time
against 8 TB/s."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from kbench_pseudobulk import make_dense, make_csr

PEAK = 8e12


def timed(f, reps):
    f()
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, min(ts) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('kind', choices=['dense', 'csr'])
    ap.add_argument('n', type=int)
    ap.add_argument('g', type=int)
    ap.add_argument('per_row', type=int, nargs='?', default=0)
    ap.add_argument('--levels', type=int, default=32)
    ap.add_argument('--q', type=int, default=1)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--f64', action='store_true')
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    dtype = np.float64 if a.f64 else np.float32
    X = make_dense(a.n, a.g, dtype) if a.kind == 'dense' else make_csr(a.n, a.g, a.per_row, dtype)
    esz = np.dtype(dtype).itemsize
    nnz = X.nnz if a.kind == 'csr' else a.n * a.g
    alg = nnz * (esz + (4 if a.kind == 'csr' else 0))
    rs = np.random.RandomState(1)
    codes = (rs.permutation(a.n) % a.levels).astype(np.int32)
    V = rs.randn(a.q, a.n) + np.arange(a.q)[:, None]
    V[:, rs.rand(a.n) < 0.05] = np.nan                       # the cells the association did not keep
    eng = get_engine()
    t0 = time.perf_counter()
    eng.ensure_expression(X)
    eng.pin_expression(X)
    up = time.perf_counter() - t0
    masked = np.where(codes[None, None, :] == np.arange(a.levels)[None, :, None], V[:, None, :], np.nan)
    masked = np.ascontiguousarray(masked.reshape(a.q * a.levels, a.n))
    calls = -(-len(masked) // 16)

    def one_pass():
        eng.ensure_expression(X)
        return eng.gene_corr_by(V, codes, a.levels)

    def emulation():
        eng.ensure_expression(X)
        return np.concatenate([eng.gene_corr(masked[k:k + 16]) for k in range(0, len(masked), 16)])

    ms_new, min_new, got = timed(one_pass, a.reps)
    ms_old, min_old, emu = timed(emulation, a.reps)
    diff = float(np.nanmax(np.abs(got[0].reshape(emu.shape) - emu)))
    same_nan = bool((np.isnan(got[0].reshape(emu.shape)) == np.isnan(emu)).all())
    print('%s %d x %d %s nnz %d (%s, matrix %.3f GB, upload %.2f s), %d levels, q = %d: one pass %.2f ms (min %.2f) = %.0f GB/s of '
          'the matrix = %.1f %% of 8 TB/s; emulation, %d gene_corr calls, %.2f ms (min %.2f); emulation / one pass = %.2f; '
          'max |difference| %.1e, NaN patterns %s'
          % (a.kind, a.n, a.g, np.dtype(dtype).name, nnz, eng.expression_shape()['format'], alg / 1e9, up, a.levels, a.q, ms_new,
             min_new, alg / ms_new / 1e6, 100 * alg / (ms_new * 1e-3) / PEAK, calls, ms_old, min_old, ms_old / ms_new, diff,
             'equal' if same_nan else 'DIFFER'), flush=True)
    eng.unpin_expression()
    eng.drop_expression()


if __name__ == '__main__':
    main()
