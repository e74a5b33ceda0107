#!/usr/bin/env python3
"""Time the device side of cna.tl.gene_test_strata: cna_expr_cross_by (one pass over the expression matrix for all levels)
against the route the library had before -- one cna_expr_cross per level with xrow masked to that level -- and cna_gram_by
against one cna_gram of the same X (its levels together do the same flops).  For gene-major lists the one-pass kernel lost
this measurement at 1M x 100 and was taken out (profiles/kbench_gene_test_strata.txt keeps its figures): Engine.expr_cross_by_raw
serves that form by the masked route, so on a csc line both times are that route's.  One GPU, one process per line:

  kbench_gene_test_strata.py dense n_cells n_samples [--genes 2000] [--levels 32] [--reps 7] [--out FILE]
  kbench_gene_test_strata.py csc   n_cells n_samples [--genes 2000] [--levels 32] [--reps 7] [--density 0.1] [--out FILE]

  timeout 600 tools/kbench_gene_test_strata.py dense 200000 50
  timeout 600 tools/kbench_gene_test_strata.py csc   200000 50
  timeout 900 tools/kbench_gene_test_strata.py dense 1000000 100
  timeout 900 tools/kbench_gene_test_strata.py csc   1000000 100

The expression matrix (float32; CSC: every gene present in every 1 / density-th cell) is resident and pinned, X is random
float64 from upload_x with one row per cell that has one, xrow a random permutation with 5 % of the cells -1, the levels of
unequal size (level l holds a share proportional to 1 / (l + 1) of the cells, in random order).  Every figure is the median
of --reps whole calls after two warm-up calls (the work buffers grow in the first): host clock around a call that ends in a
device synchronise, xrow and the codes cross PCIe in it and the result comes back.  The kernel-only figures beside them come
from the library's event timers (cna_prof_get) in a separate set of calls: `gram` + `gram_reduce` for cna_gram, `gram_by` (row
list, k_gram_by, fold) for cna_gram_by, as TFLOP/s of 2 rows N^2 and as a share of the f64 matrix peak (78.6 TFLOP/s)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp

from kbench_pseudobulk import make_dense

F64_MFMA_PEAK_TF = 78.6


def make_csc(n, g, every, dtype):
    """gene j present in the cells j % every, j % every + every, ...: n / every entries per gene, g / every per cell"""
    per = (n - 1 - np.arange(g) % every) // every + 1
    indptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    indices = np.empty(int(indptr[-1]), dtype=np.int32)
    for j in range(g):
        indices[indptr[j]:indptr[j + 1]] = np.arange(j % every, n, every, dtype=np.int32)
    vals = (np.random.default_rng(0).integers(1, 6, size=len(indices))).astype(dtype)
    M = sp.csc_matrix((vals, indices, indptr), shape=(n, g))
    M.has_sorted_indices = True
    M.has_canonical_format = True
    return M


def timed(f, reps):
    f()
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, min(ts) * 1e3, out


def kernel_ms(eng, f, names, reps=5):
    eng.prof_reset()
    eng.prof_enable(True)
    for _ in range(reps):
        f()
    eng.prof_enable(False)
    p = eng.prof()
    return sum(p[k][0] / max(p[k][1], 1) for k in names if k in p)        # (a group that never ran: the csc lines' one pass)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('kind', choices=['dense', 'csc'])
    ap.add_argument('n', type=int)
    ap.add_argument('N', type=int)
    ap.add_argument('--genes', type=int, default=2000)
    ap.add_argument('--levels', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--density', type=float, default=0.1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    n, N, G, L = a.n, a.N, a.genes, a.levels
    E = make_dense(n, G, np.float32) if a.kind == 'dense' else make_csc(n, G, int(round(1 / a.density)), np.float32)
    nnz = E.nnz if a.kind == 'csc' else n * G
    rs = np.random.RandomState(1)
    took = rs.rand(n) >= 0.05
    nx = int(took.sum())
    xrow = np.full(n, -1, dtype=np.int64)
    xrow[took] = rs.permutation(nx)
    share = 1.0 / (1.0 + np.arange(L))
    codes = rs.choice(L, size=n, p=share / share.sum()).astype(np.int32)
    X = rs.randn(nx, N)
    eng = get_engine()
    eng.upload_x(X)
    t0 = time.perf_counter()
    eng.ensure_expression(E)
    eng.pin_expression(E)
    up = time.perf_counter() - t0
    masked = [np.where(codes == l, xrow, -1) for l in range(L)]

    def one_pass():
        return eng.expr_cross_by_raw(xrow, codes, L)

    def per_level():
        return [eng.expr_cross(xrow=m) for m in masked]

    ms_new, min_new, got = timed(one_pass, a.reps)
    ms_old, min_old, old = timed(per_level, a.reps)
    Wold = np.stack([o[0] for o in old])
    scale = float(np.max(np.abs(Wold)))
    diff = float(np.max(np.abs(got[0] - Wold))) / scale
    k_new = kernel_ms(eng, one_pass, ['expr_cross_by'], reps=3)
    ms_gby, min_gby, gby = timed(lambda: eng.gram_by(xrow, codes, L), a.reps)
    ms_g, min_g, g1 = timed(eng.gram, a.reps)
    gdiff = float(np.max(np.abs(gby[0].sum(axis=0) - g1))) / float(np.max(np.abs(g1)))
    k_gby = kernel_ms(eng, lambda: eng.gram_by(xrow, codes, L), ['gram_by'])
    k_g = kernel_ms(eng, eng.gram, ['gram', 'gram_reduce'])
    flop = 2.0 * nx * N * N
    cells = np.bincount(codes[took], minlength=L)
    line = ('%s %d cells x %d genes float32 nnz %d (%s, upload %.1f s), X %d x %d, %d levels of %d .. %d cells: '
            'cna_expr_cross_by %.2f ms (min %.2f; sums and folds alone %.2f ms); %d masked cna_expr_cross calls %.2f ms (min %.2f); '
            'masked / one pass = %.2f; max |W difference| / max |W| = %.1e.  '
            'cna_gram_by %.2f ms (min %.2f; kernels %.3f ms = %.1f TFLOP/s = %.1f %% of the f64 matrix peak); cna_gram %.2f ms '
            '(min %.2f; kernels %.3f ms = %.1f TFLOP/s = %.1f %%); gram_by / gram kernels = %.2f; max |sum of levels - gram| / max = %.1e'
            % (a.kind, n, G, nnz, eng.expression_shape()['format'], up, nx, N, L, cells.min(), cells.max(), ms_new, min_new, k_new, L,
               ms_old, min_old, ms_old / ms_new, diff, ms_gby, min_gby, k_gby, flop / k_gby / 1e9, 100 * flop / k_gby / 1e9 / F64_MFMA_PEAK_TF,
               ms_g, min_g, k_g, flop / k_g / 1e9, 100 * flop / k_g / 1e9 / F64_MFMA_PEAK_TF, k_gby / k_g, gdiff))
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    eng.unpin_expression()
    eng.drop_expression()


if __name__ == '__main__':
    main()
