#!/usr/bin/env python3
"""Time cna.ut.expr_to_sample's device path alone (Engine.expr_to_bins) on a resident synthetic expression matrix.

  kbench_pseudobulk.py dense  n_cells n_genes           [--bins 200] [--f64] [--no-host] [--reps 5] [--host-cells 200000]
  kbench_pseudobulk.py csr    n_cells n_genes per_row   [--bins 200] [--f64] [--no-host] [--reps 5] [--host-cells 200000]

The matrix is one block of 65536 random rows repeated (the sums do not care, and the generation stays short); cell i
belongs to bin `i % bins` of a random permutation of the cells ("interleaved": a bin's rows lie all over the matrix)
and, second, to bin `i * bins // n` ("sorted": a bin's rows are contiguous).  Prints the upload seconds, per-call
milliseconds (whole call: the codes cross PCIe in it, 4 bytes x cells, and the result comes back, 8 bytes x bins x
genes), for the dense form the kernel bytes (cells x genes x 4|8, the matrix read once) over 8 TB/s at the CALL's time
-- kernel times come from a `rocprofv3 --kernel-trace --stats` run of this same command -- and the time of pandas'
groupby().mean() over the same host's float64 frame, on the first --host-cells cells when the full frame is larger."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp

PEAK = 8e12
BLOCK = 65536


def make_dense(n, g, dtype):
    rng = np.random.default_rng(0)
    blk = (rng.standard_normal((BLOCK, g), dtype=np.float32) + rng.random(g, dtype=np.float32) * 3).astype(dtype)
    X = np.empty((n, g), dtype=dtype)
    for r in range(0, n, BLOCK):
        X[r:r + BLOCK] = blk[:min(BLOCK, n - r)]
    return X


def make_csr(n, g, per_row, dtype):
    """per_row entries in every row, one in each bucket of g / per_row genes: sorted, no duplicates, no sort needed"""
    assert g % per_row == 0
    rng = np.random.default_rng(0)
    width = g // per_row
    blk = rng.integers(0, width, size=(BLOCK, per_row), dtype=np.int32) + (np.arange(per_row, dtype=np.int32) * width)[None, :]
    vblk = rng.integers(1, 6, size=(BLOCK, per_row)).astype(dtype)
    idx = np.empty((n, per_row), dtype=np.int32)
    val = np.empty((n, per_row), dtype=dtype)
    for r in range(0, n, BLOCK):
        idx[r:r + BLOCK] = blk[:min(BLOCK, n - r)]
        val[r:r + BLOCK] = vblk[:min(BLOCK, n - r)]
    M = sp.csr_matrix((val.reshape(-1), idx.reshape(-1), np.arange(n + 1, dtype=np.int64) * per_row), shape=(n, g))
    M.has_sorted_indices = True
    M.has_canonical_format = True
    return M


def host_groupby(X, codes, cells):
    import pandas as pd
    m = min(cells, X.shape[0])
    sub = X[:m]
    frame = pd.DataFrame(np.asarray(sub.toarray() if sp.issparse(sub) else sub, dtype=np.float64))
    t0 = time.perf_counter()
    out = frame.groupby(codes[:m]).mean()
    return time.perf_counter() - t0, m, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('kind', choices=['dense', 'csr'])
    ap.add_argument('n', type=int)
    ap.add_argument('g', type=int)
    ap.add_argument('per_row', type=int, nargs='?', default=0)
    ap.add_argument('--bins', type=int, default=200)
    ap.add_argument('--f64', action='store_true')
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-cells', type=int, default=200000)
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    dtype = np.float64 if a.f64 else np.float32
    t0 = time.perf_counter()
    X = make_dense(a.n, a.g, dtype) if a.kind == 'dense' else make_csr(a.n, a.g, a.per_row, dtype)
    esz = np.dtype(dtype).itemsize
    nnz = X.nnz if a.kind == 'csr' else a.n * a.g
    alg = nnz * (esz + (4 if a.kind == 'csr' else 0))
    print('%s %d x %d %s nnz %d, %d bins: generated in %.1f s, matrix bytes on the device %.3f GB'
          % (a.kind, a.n, a.g, np.dtype(dtype).name, nnz, a.bins, time.perf_counter() - t0, alg / 1e9), flush=True)
    eng = get_engine()
    t0 = time.perf_counter()
    eng.ensure_expression(X)
    eng.pin_expression(X)
    print('upload %.3f s (%s)' % (time.perf_counter() - t0, eng.expression_shape()['format']), flush=True)
    layouts = {'interleaved': (np.random.RandomState(1).permutation(a.n) % a.bins).astype(np.int32),
               'sorted': (np.arange(a.n, dtype=np.int64) * a.bins // a.n).astype(np.int32)}
    for name, codes in layouts.items():
        for what in (0, 1):
            eng.ensure_expression(X)
            sums, counts = eng.expr_to_bins(codes, a.bins, what)               # warm-up: work buffers
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                eng.ensure_expression(X)
                sums, counts = eng.expr_to_bins(codes, a.bins, what)
                ts.append(time.perf_counter() - t0)
            ms = float(np.median(ts)) * 1e3
            line = ('%-11s %s  call %.2f ms (min %.2f)  matrix %.3f GB (+ %.3f GB codes in, %.3f GB result out over PCIe)'
                    % (name, 'sum x   ' if what == 0 else 'count x>0', ms, min(ts) * 1e3, alg / 1e9, 4e-9 * a.n,
                       8e-9 * a.bins * a.g))
            line += '  %.0f GB/s = %.1f %% of 8 TB/s at the call\'s time' % (alg / ms / 1e6, 100 * alg / (ms * 1e-3) / PEAK)
            print(line, flush=True)
        if not a.no_host:
            th, m, ref = host_groupby(X, codes, a.host_cells)
            got = eng.expr_to_bins(np.where(np.arange(a.n) < m, codes, -1).astype(np.int32), a.bins, 0)
            with np.errstate(invalid='ignore', divide='ignore'):
                mean = (got[0] / got[1][:, None])[ref.index.values]
            print('%-11s pandas groupby().mean() on the first %d cells (float64 frame %.2f GB): %.2f s = %.2f s per 2M cells; '
                  'max |device - pandas| on those cells %.1e'
                  % (name, m, 8e-9 * m * a.g, th, th * 2e6 / m, float(np.nanmax(np.abs(mean - ref.values)))), flush=True)
    eng.drop_expression()


if __name__ == '__main__':
    main()
