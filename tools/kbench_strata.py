#!/usr/bin/env python3
"""Time cna.tl.coef_strata's device path (Engine.coef_strata) and the host computation it replaces.

  kbench_strata.py [--cells 2000000] [--levels 20] [--points 100] [--reps 7] [--out profiles/r10_kbench_strata.txt]

Synthetic coefficient and FDR columns (normal / uniform draws, 2 % of the cells without a coefficient), the cells dealt to
the levels at random.  Per call the three columns cross PCIe (20 bytes x cells, pageable memory) and levels x points
doubles come back.  The split: "upload" and "fetch" are the same copies issued alone with hipMemcpy (pageable host memory
to the device and back, synchronised), "kernels" is the whole call minus the two -- the call waits for the device twice
(the verdict on the codes, the result), so this is the device work plus those two waits.
The host baseline is matplotlib.cbook.violin_stats with mlab.GaussianKDE, what Axes.violinplot runs for cna.pl.violinplot,
on ONE level of the same data, on this machine's host cores; the full host run is that time multiplied by the level count
(the levels are equally large), and the output says so.  No pass / fail figure: the file records the ratio."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def host_one_level(x, points):
    from matplotlib import cbook, mlab

    def method(X, coords):
        if np.all(X[0] == X):
            return (X[0] == coords).astype(float)
        return mlab.GaussianKDE(X, None).evaluate(coords)
    t0 = time.perf_counter()
    stats = cbook.violin_stats(x, method, points=points)[0]
    return time.perf_counter() - t0, stats


def copies_alone(arrays, out_doubles, reps):
    """Median seconds of hipMemcpy of `arrays` to the device (pageable memory, as the call issues them) and of
    `out_doubles` doubles back, through the HIP runtime the library has loaded."""
    import ctypes as C
    try:
        hip = C.CDLL('libamdhip64.so')
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'libamdhip64.so'))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    back = np.empty(out_doubles)
    bufs = []
    for a in list(arrays) + [back]:
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
        bufs.append(p)
    up, down = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        for a, p in zip(arrays, bufs):
            assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0          # hipMemcpyHostToDevice
        assert hip.hipDeviceSynchronize() == 0
        up.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), bufs[-1], back.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        down.append(time.perf_counter() - t0)
    for p in bufs:
        hip.hipFree(p)
    return float(np.median(up[1:])), float(np.median(down[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=2000000)
    ap.add_argument('--levels', type=int, default=20)
    ap.add_argument('--points', type=int, default=100)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join('profiles', 'r10_kbench_strata.txt'))
    a = ap.parse_args()
    from cna_amd.engine import get_engine
    import matplotlib
    rs = np.random.RandomState(0)
    v = rs.randn(a.cells) * 0.05 + 0.01
    v[rs.rand(a.cells) < 0.02] = np.nan
    fdr = rs.rand(a.cells) * 0.3
    codes = (rs.permutation(a.cells) % a.levels).astype(np.int32)
    eng = get_engine()
    lines = ['cna.tl.coef_strata, device path (Engine.coef_strata): %d cells x %d levels x %d points, bandwidth rule Scott'
             % (a.cells, a.levels, a.points)]
    r = eng.coef_strata(v, fdr, codes, a.levels, 0.1, a.points)                    # warm-up: work buffers
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = eng.coef_strata(v, fdr, codes, a.levels, 0.1, a.points)
        ts.append(time.perf_counter() - t0)
    call = float(np.median(ts))
    up, down = copies_alone([v, fdr, codes], a.levels * a.points + 9 * a.levels, a.reps)
    kern = call - up - down
    exps = float(r['n_kept'].sum()) * a.points
    lines.append('whole call          %8.3f ms (median of %d, min %.3f)' % (call * 1e3, a.reps, min(ts) * 1e3))
    lines.append('  upload            %8.3f ms  (%.1f MB of pageable memory, the same copies issued alone)'
                 % (up * 1e3, (v.nbytes + fdr.nbytes + codes.nbytes) / 1e6))
    lines.append('  fetch             %8.3f ms  (%d doubles, issued alone)' % (down * 1e3, a.levels * a.points + 9 * a.levels))
    lines.append('  kernels           %8.3f ms  (the call minus the two; includes its two waits for the device)' % (kern * 1e3))
    lines.append('  float64 exponentials %.3e: %.1f G exp/s at the kernels\' time' % (exps, exps / max(kern, 1e-9) / 1e9))
    x = v[(codes == 0) & np.isfinite(v)]
    th, stats = host_one_level(x, a.points)
    rel = float(np.max(np.abs(r['vals'][0] - stats['vals']) / stats['vals']))
    lines.append('host baseline: matplotlib %s cbook.violin_stats + mlab.GaussianKDE on ONE level (%d cells) on this machine: %.3f s'
                 % (matplotlib.__version__, x.size, th))
    lines.append('  the full host run is that times the level count (levels equally large): %.1f s for %d levels'
                 % (th * a.levels, a.levels))
    lines.append('  ratio host / device: %.0f x against the whole call, %.0f x against the kernels'
                 % (th * a.levels / call, th * a.levels / max(kern, 1e-9)))
    lines.append('  level 0 against matplotlib: median %s, min / max %s, largest relative difference of the density %.2e '
                 '(m = %d, past the %d the tests\' tolerance is derived for)'
                 % ('equal' if r['median'][0] == stats['median'] else 'DIFFERENT',
                    'equal' if (r['min'][0] == stats['min'] and r['max'][0] == stats['max']) else 'DIFFERENT', rel, x.size, 4096 + 37))
    eng.drop_expression()
    text = '\n'.join(lines) + '\n'
    print(text, end='', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
