#!/usr/bin/env python3
"""Time cna.tl.coef_raster's device path (Engine.coef_raster) and the numpy route of its restatement.

  kbench_coef_raster.py [--cells 200000 1000000 2000000] [--sides 512 2048] [--keys 1 4] [--reps 5]
                        [--out profiles/kbench_coef_raster.txt]

A synthetic embedding with clustered density: 30 Gaussian clusters of unequal size and width plus 2 % of the cells in one
point (a pixel that holds tens of thousands of cells), normal coefficients with 5 % NaN and a uniform fdr for every key,
radius 0, the automatic extent.  Per configuration:
  call     the whole Engine.coef_raster call, wall clock, median of the repetitions after a warm-up
  H2D      the copies of xy, V and FDR to the device   } HIP events on the library's stream (cna_prof_enable: raster_upload,
  kernels  from the extent to the images               } raster, raster_fetch), mean per call; "kernels" includes the two waits
  D2H      the copies of the images back               } of the host for the extent and for the chunk counts
  numpy    the route of the restatement on this machine's host cores: np.bincount for counts and sums, np.maximum.at /
           np.minimum.at for top and bottom (tests/test_coef_raster_host.py, restated here so that the tool stands alone)
The kernels' traffic is counted from the kernels' own reads and writes (cna_coef_raster) and set against
the 8 TB/s HBM peak.  No pass / fail figure: the file records the numbers."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_PEAK = 8.0e12


def embedding(n, seed=0):
    rs = np.random.RandomState(seed)
    k = 30
    share = rs.dirichlet(np.full(k, 0.7))
    which = rs.choice(k, size=n, p=share)
    centre = rs.randn(k, 2) * 6.0
    width = rs.uniform(0.15, 1.2, size=(k, 1))
    xy = centre[which] + rs.randn(n, 2) * width[which]
    xy[rs.rand(n) < 0.02] = centre[0]
    return np.ascontiguousarray(xy)


def numpy_route(xy, V, FDR, thresh, W, H):
    """The restatement's route, automatic extent, every key with an fdr, radius 0."""
    x, y = xy[:, 0], xy[:, 1]
    x0, x1, y0, y1 = x.min(), x.max(), y.min(), y.max()
    ix = np.minimum(np.floor((x - x0) * (W / (x1 - x0))).astype(np.int64), W - 1)
    iy = np.minimum(np.floor((y - y0) * (H / (y1 - y0))).astype(np.int64), H - 1)
    pix = iy * W + ix
    P = W * H
    out = {'n': np.bincount(pix, minlength=P).reshape(H, W), 'n_pass': [], 'sum': [], 'top': [], 'bottom': []}
    for k in range(V.shape[0]):
        with np.errstate(invalid='ignore'):
            ok = np.isfinite(V[k]) & (FDR[k] <= thresh)
        pk, vk = pix[ok], V[k, ok]
        top, bot = np.full(P, -np.inf), np.full(P, np.inf)
        np.maximum.at(top, pk, vk)
        np.minimum.at(bot, pk, vk)
        out['n_pass'].append(np.bincount(pk, minlength=P).reshape(H, W))
        out['sum'].append(np.bincount(pk, weights=vk, minlength=P).reshape(H, W))
        out['top'].append(np.where(np.isinf(top), np.nan, top).reshape(H, W))
        out['bottom'].append(np.where(np.isinf(bot), np.nan, bot).reshape(H, W))
    return {k: (v if k == 'n' else np.stack(v)) for k, v in out.items()}


def kernel_bytes(n, q, P, inside, passing_reads):
    """HBM bytes of the kernels of one call (DESIGN.md lists them kernel by kernel)."""
    extent = 16 * n
    pixel = 16 * n + 8 * n
    sort = 12 * n + 20 * n + 12 * n          # pass 1: codes twice, list out; pass 2: the same and pass 1's list twice; its codes
    bounds = 8 * P + 8 * inside + 8 * min(P, inside)                     # memset; list and pixel of every position; the two writes
    classify = 8 * P + 4 * P
    reduce_ = q * (8 * P + 4 * inside + 16 * passing_reads + 28 * P)
    return extent + pixel + sort + bounds + classify + reduce_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, nargs='+', default=[200000, 1000000, 2000000])
    ap.add_argument('--sides', type=int, nargs='+', default=[512, 2048])
    ap.add_argument('--keys', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'kbench_coef_raster.txt'))
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    eng = get_engine()
    lines = ['cna.tl.coef_raster, device path (Engine.coef_raster) against the numpy route of its restatement; radius 0, '
             'automatic extent, every key with an fdr; ms.  numpy had 16 host threads; bincount and ufunc.at use one',
             '%9s %6s %2s | %9s %8s %8s %8s | %9s %7s | %8s %7s | %s'
             % ('cells', 'side', 'q', 'call', 'H2D', 'kernels', 'D2H', 'numpy', 'x call', 'GB kern', '% HBM', 'images')]
    for n in a.cells:
        xy = embedding(n)
        rs = np.random.RandomState(1)
        for q in a.keys:
            V = rs.randn(q, n) * 0.05
            V[rs.rand(q, n) < 0.05] = np.nan
            FDR = rs.rand(q, n) * 0.3
            has = np.ones(q, dtype=np.int32)
            for side in a.sides:
                if q * side * side > 2 ** 22:
                    lines.append('%9d %6d %2d | q x side x side exceeds 2^22: refused by design' % (n, side, q))
                    continue
                r = eng.coef_raster(xy, V, FDR, has, 0.1, None, side, side)            # warm-up: work buffers
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    r = eng.coef_raster(xy, V, FDR, has, 0.1, None, side, side)
                    ts.append(time.perf_counter() - t0)
                eng.prof_reset()
                eng.prof_enable(True)
                for _ in range(a.reps):
                    eng.coef_raster(xy, V, FDR, has, 0.1, None, side, side)
                eng.prof_enable(False)
                p = eng.prof()
                up, kern, down = (p[k][0] / p[k][1] for k in ('raster_upload', 'raster', 'raster_fetch'))
                t0 = time.perf_counter()
                w = numpy_route(xy, V, FDR, 0.1, side, side)
                host = time.perf_counter() - t0
                same = all(np.array_equal(r[k], w[k], equal_nan=True) for k in ('n', 'n_pass', 'top', 'bottom'))
                close = bool(np.allclose(r['sum'], w['sum'], rtol=0, atol=1e-9))
                gb = kernel_bytes(n, q, side * side, int(r['n'].sum()), int(r['n'].sum())) / 1e9
                call = float(np.median(ts))
                lines.append('%9d %6d %2d | %9.2f %8.2f %8.2f %8.2f | %9.1f %6.1fx | %8.3f %6.1f%% | %s'
                             % (n, side, q, call * 1e3, up, kern, down, host * 1e3, host / call, gb,
                                100.0 * gb * 1e9 / (kern * 1e-3) / HBM_PEAK,
                                'counts and extremes equal, sums %s' % ('within 1e-9' if close else 'DIFFER') if same else 'DIFFERENT'))
                print(lines[-1], flush=True)
    eng.drop_expression()
    text = '\n'.join(lines) + '\n'
    print(text, end='', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
