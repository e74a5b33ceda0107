#!/usr/bin/env python3
"""Time cna.tl.gene_test's device pass alone (Engine.expr_cross: W = E^T X) and its host algebra on synthetic inputs.

  kbench_gene_cross.py dense  n_cells n_genes           [--samples 200] [--f64] [--no-host] [--reps 5] [--host-cells 200000]
  kbench_gene_cross.py csr    n_cells n_genes per_row   [--samples 200] [--f64] [--no-host] [--reps 5] [--host-cells 200000]

The expression matrix is kbench_pseudobulk.py's (one block of 65536 random rows repeated); the working matrix X is random
float64, n_cells x samples, put on the device with upload_x (every cell has a row: xrow is the identity).  Prints the
upload seconds and per-call milliseconds of the whole call (xrow crosses PCIe in it, 8 bytes x cells; the result comes
back, 8 bytes x genes x samples) with what that time means against the chip: dense -- 2 n G N flops over the 78.6 TFLOP/s
of vector float64, and 4|8 n G + 8 n N bytes over 8 TB/s; lists -- nnz x 8 N gathered bytes per second.  Kernel times
come from a `rocprofv3 --kernel-trace --stats` run of this same command.  Then the host algebra of gene_test's step 5
(genes x samples by samples x 1001 columns) and, unless --no-host, the host computation the pass replaces: float64
E[:m].T @ X[:m] in numpy / scipy on the first --host-cells cells, scaled to all of them."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp

from kbench_pseudobulk import make_csr, make_dense

PEAK_F64 = 78.6e12
PEAK_HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('kind', choices=['dense', 'csr'])
    ap.add_argument('n', type=int)
    ap.add_argument('g', type=int)
    ap.add_argument('per_row', type=int, nargs='?', default=0)
    ap.add_argument('--samples', type=int, default=200)
    ap.add_argument('--f64', action='store_true')
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-cells', type=int, default=200000)
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    from cna_amd.tools._gene_test import null_correlations, permutation_stats
    dtype = np.float64 if a.f64 else np.float32
    N = a.samples
    t0 = time.perf_counter()
    E = make_dense(a.n, a.g, dtype) if a.kind == 'dense' else make_csr(a.n, a.g, a.per_row, dtype)
    X = np.random.default_rng(1).standard_normal((a.n, N))
    esz = np.dtype(dtype).itemsize
    nnz = E.nnz if a.kind == 'csr' else a.n * a.g
    print('%s %d x %d %s nnz %d against X %d x %d float64: generated in %.1f s' % (a.kind, a.n, a.g, np.dtype(dtype).name, nnz,
                                                                                  a.n, N, time.perf_counter() - t0), flush=True)
    eng = get_engine()
    t0 = time.perf_counter()
    eng.ensure_expression(E)
    eng.pin_expression(E)
    eng.upload_x(X)
    eng.sync()
    print('upload %.3f s (%s)' % (time.perf_counter() - t0, eng.expression_shape()['format']), flush=True)
    out = eng.expr_cross()                                     # warm-up: work buffers
    ts = []
    for _ in range(a.reps):
        eng._cross_memo = None
        t0 = time.perf_counter()
        out = eng.expr_cross()
        ts.append(time.perf_counter() - t0)
    ms = float(np.median(ts)) * 1e3
    flops = 2.0 * nnz * N
    line = 'expr_cross call %.2f ms (min %.2f)  %.3e flops' % (ms, min(ts) * 1e3, flops)
    if a.kind == 'dense':
        byts = float(esz) * a.n * a.g + 8.0 * a.n * N
        frac = byts / (ms * 1e-3) / PEAK_HBM
        line += ' = %.1f %% of %.1f TFLOP/s;  %.2f GB compulsory bytes = %.0f ppm (%.2f %%) of 8 TB/s' % (
            100 * flops / (ms * 1e-3) / PEAK_F64, PEAK_F64 / 1e12, byts / 1e9, 1e6 * frac, 100 * frac)
    else:
        gathered = 8.0 * nnz * N
        line += ';  %.2f TB of gathered rows = %.2f TB/s' % (gathered / 1e12, gathered / (ms * 1e-3) / 1e12)
    print(line, flush=True)
    # host algebra of step 5: 1 observed + 1000 null columns
    W, rho, sx, sxx, m = out
    Gamma = eng.gram()
    Z = np.random.default_rng(2).standard_normal((N, 1001))
    t0 = time.perf_counter()
    r = null_correlations(W, rho, sx, sxx, m, Gamma, Z)
    t1 = time.perf_counter()
    permutation_stats(r[:, 0], r[:, 1:])
    t2 = time.perf_counter()
    print('host algebra, %d genes x %d samples x 1001 columns: correlations %.1f ms, p / q %.1f ms' % (a.g, N, (t1 - t0) * 1e3,
                                                                                                     (t2 - t1) * 1e3), flush=True)
    if not a.no_host:
        mc = min(a.host_cells, a.n)
        sub = E[:mc]
        t0 = time.perf_counter()
        ref = (sub.T @ X[:mc]) if sp.issparse(sub) else sub.astype(np.float64).T @ X[:mc]
        th = time.perf_counter() - t0
        # the device on the same cells: the others have no row (xrow -1)
        got = eng.expr_cross(xrow=np.where(np.arange(a.n) < mc, np.arange(a.n), -1))[0]
        err = float(np.max(np.abs(got - np.asarray(ref))))
        print('host float64 E[:m].T @ X[:m] on the first %d cells: %.2f s = %.2f s per %d cells; max |device - host| there %.1e '
              '(max |W| %.1e)' % (mc, th, th * a.n / mc, a.n, err, float(np.max(np.abs(np.asarray(ref))))), flush=True)
    eng.drop_expression()


if __name__ == '__main__':
    main()
