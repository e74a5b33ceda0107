#!/usr/bin/env python3
"""Time cna.tl.gene_corr's device path alone: upload of a synthetic expression matrix and the per-call reduction.

  kbench_genecorr.py dense  n_cells n_genes           [--q 1,8] [--f64] [--no-host] [--reps 5]
  kbench_genecorr.py csr    n_cells n_genes per_row   [--q 1,8] [--f64] [--no-host] [--reps 5]

Prints upload seconds, per-call milliseconds (whole call: the q key columns cross PCIe in it, 8 bytes x cells x q),
algorithmic bytes (the matrix read once: cells x genes x 4|8 dense, nnz x (4|8 + 4) gene-major; the gathers of the key
table, nnz x 8 q, are listed beside it) and the fraction of 8 TB/s -- and the time of the host computation the call
replaces: the same sums as a float64 X.T @ Vc formulation in numpy / scipy (row blocks, BLAS threads as the box gives
them), not the (genes + 1)^2 corrcoef."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp

PEAK = 8e12


def make_dense(n, g, dtype):
    rng = np.random.default_rng(0)
    X = np.empty((n, g), dtype=dtype)
    level = rng.random(g, dtype=np.float32) * 3
    for r in range(0, n, 65536):
        X[r:r + 65536] = rng.standard_normal((min(65536, n - r), g), dtype=np.float32) + level
    return X


def make_csr(n, g, per_row, dtype):
    """per_row entries in every row, one in each bucket of g / per_row genes: sorted, no duplicates, no sort needed"""
    assert g % per_row == 0
    rng = np.random.default_rng(0)
    width = g // per_row
    base = (np.arange(per_row, dtype=np.int32) * width)[None, :]
    idx = np.empty((n, per_row), dtype=np.int32)
    val = np.empty(n * per_row, dtype=dtype)
    for r in range(0, n, 65536):
        m = min(65536, n - r)
        idx[r:r + m] = rng.integers(0, width, size=(m, per_row), dtype=np.int32) + base
        val[r * per_row:(r + m) * per_row] = rng.integers(1, 6, size=m * per_row, dtype=np.int32)
    M = sp.csr_matrix((val, idx.reshape(-1), np.arange(n + 1, dtype=np.int64) * per_row), shape=(n, g))
    M.has_sorted_indices = True
    M.has_canonical_format = True
    return M


def host_sums(X, V):
    """the per-gene sums of the call, float64, the way a numpy / scipy user would form them without the corrcoef matrix"""
    Vc = (V - V.mean(axis=1, keepdims=True)).T.copy()          # cells x q
    t0 = time.perf_counter()
    if sp.issparse(X):
        X64 = X.astype(np.float64)
        sxv = X64.T @ Vc
        sx = np.asarray(X64.sum(axis=0)).ravel()
        sxx = np.asarray(X64.multiply(X64).sum(axis=0)).ravel()
    else:
        g = X.shape[1]
        sxv, sx, sxx = np.zeros((g, Vc.shape[1])), np.zeros(g), np.zeros(g)
        for r in range(0, X.shape[0], 131072):
            Xb = X[r:r + 131072].astype(np.float64)
            sxv += Xb.T @ Vc[r:r + 131072]
            sx += Xb.sum(axis=0)
            sxx += np.einsum('ij,ij->j', Xb, Xb)
    n = X.shape[0]
    r = (sxv / np.sqrt(sxx - sx * sx / n)[:, None] / np.sqrt((Vc * Vc).sum(axis=0))[None, :]).T
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('kind', choices=['dense', 'csr'])
    ap.add_argument('n', type=int)
    ap.add_argument('g', type=int)
    ap.add_argument('per_row', type=int, nargs='?', default=0)
    ap.add_argument('--q', default='1,8')
    ap.add_argument('--f64', action='store_true')
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    dtype = np.float64 if a.f64 else np.float32
    t0 = time.perf_counter()
    X = make_dense(a.n, a.g, dtype) if a.kind == 'dense' else make_csr(a.n, a.g, a.per_row, dtype)
    esz = np.dtype(dtype).itemsize
    nnz = X.nnz if a.kind == 'csr' else a.n * a.g
    alg = nnz * (esz + (4 if a.kind == 'csr' else 0))
    print('%s %d x %d %s nnz %d: generated in %.1f s, matrix bytes on the device %.3f GB'
          % (a.kind, a.n, a.g, np.dtype(dtype).name, nnz, time.perf_counter() - t0, alg / 1e9), flush=True)
    eng = get_engine()
    t0 = time.perf_counter()
    eng.ensure_expression(X)
    eng.pin_expression(X)
    print('upload %.3f s (%s)' % (time.perf_counter() - t0, eng.expression_shape()['format']), flush=True)
    rs = np.random.RandomState(1)
    for q in [int(v) for v in a.q.split(',')]:
        V = np.ascontiguousarray(rs.randn(q, a.n))
        eng.ensure_expression(X)
        r = eng.gene_corr(V)                                      # warm-up: work buffers
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            eng.ensure_expression(X)
            r = eng.gene_corr(V)
            ts.append(time.perf_counter() - t0)
        ms = float(np.median(ts)) * 1e3
        line = ('q=%d  call %.2f ms (min %.2f)  algorithmic %.3f GB (+ %.3f GB key columns over PCIe%s)  %.0f GB/s = %.1f %% of 8 TB/s'
                % (q, ms, min(ts) * 1e3, alg / 1e9, 8e-9 * a.n * q,
                   ', gathers %.3f GB' % (8e-9 * nnz * q) if a.kind == 'csr' else '', alg / ms / 1e6, 100 * alg / (ms * 1e-3) / PEAK))
        if not a.no_host:
            th, rh = host_sums(X, V)
            line += '  | host float64 X.T @ Vc: %.2f s (x%.0f), max |dr| %.1e' % (th, th / (ms * 1e-3), np.nanmax(np.abs(r - rh)))
        print(line, flush=True)
    eng.drop_expression()


if __name__ == '__main__':
    main()
