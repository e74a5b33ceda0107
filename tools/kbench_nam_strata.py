#!/usr/bin/env python3
"""Time cna.tl.nam_strata's device pass (Engine.matrix_to_bins over the resident NAM) against the only other route to the
same numbers: the NAM to the host (engine.nam_full()) and the sums there, in the same process.

  timeout -k 10 900 python tools/kbench_nam_strata.py [--shapes 200000x50,1000000x100] [--levels 32] [--reps 7]
                                                      [--out profiles/kbench_nam_strata.txt]

Per shape a synthetic dataset (cna_amd.synth, the generator of bench.py) is walked three steps, the cells are dealt to the
levels at random, and three cases are timed: no weights (q = 0), one real-valued weight column (q = 1), and the two 0 / 1
columns of sign_of (a tenth of the cells each).  "device" is the whole Engine.matrix_to_bins call -- the codes and weights
mapped to the device's cell order on the host, up over PCIe, the sort, the sums, the result back; "kernels" the library's
own spans around the sort and the sums (HIP events).  "host" is engine.nam_full() plus a scipy.sparse (levels x cells) @ NAM
product per weight column, float64, on this machine's host cores.  Bytes / s are the algorithm's 8 n N over the time named.
The one condition: the device route is not slower than the host route at any shape; the script exits 1 otherwise."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp

HBM_PEAK = 8e12


def host_sums(nam, codes, W, levels):
    out = []
    n = len(codes)
    for w in (np.ones((1, n)) if W is None else W):
        ok = np.flatnonzero((codes >= 0) & np.isfinite(w) & (w != 0))
        S = sp.csr_matrix((w[ok], (codes[ok], ok)), shape=(levels, n))
        out.append(S @ nam)
    return np.stack(out)


def median_time(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='200000x50,1000000x100')
    ap.add_argument('--levels', type=int, default=32)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join('profiles', 'kbench_nam_strata.txt'))
    a = ap.parse_args()
    from cna_amd import synth
    from cna_amd._ffi import MAT_NAM
    from cna_amd.engine import get_engine
    from cna_amd.tools._nam import _nam_device
    eng = get_engine()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
    say('cna.tl.nam_strata: Engine.matrix_to_bins over the resident NAM against engine.nam_full() + scipy.sparse sums, '
        '%d levels, median of %d' % (a.levels, a.reps))
    lost = False
    for shape in a.shapes.split(','):
        n, N = (int(v) for v in shape.split('x'))
        data, _ = synth.make_dataset(n, N, k=15, seed=0)
        _nam_device(eng, data, 'id', nsteps=3)
        eng.sync()
        rs = np.random.RandomState(1)
        codes = (rs.permutation(n) % a.levels).astype(np.int32)
        sign = np.zeros((2, n))
        pick = rs.rand(n)
        sign[0, pick < 0.1], sign[1, pick > 0.9] = 1.0, 1.0
        cases = [('q = 0', None), ('q = 1', rs.randn(1, n)), ('sign_of (q = 2)', sign)]
        nbytes = 8.0 * n * N
        say('%d cells x %d samples: the NAM is %.1f MB' % (n, N, nbytes / 1e6))
        t_fetch, nam = median_time(eng.nam_full, max(3, a.reps // 2))
        say('  engine.nam_full()                %9.3f ms  (%.2f GB/s over PCIe, gather kernel included)'
            % (t_fetch * 1e3, nbytes / t_fetch / 1e9))
        for name, W in cases:
            eng.matrix_to_bins(MAT_NAM, codes, W, n_bins=a.levels)              # warm-up: work buffers, code objects
            eng.prof_reset()
            eng.prof_enable(True)
            t_dev, got = median_time(lambda: eng.matrix_to_bins(MAT_NAM, codes, W, n_bins=a.levels), a.reps)
            eng.prof_enable(False)
            prof = eng.prof()
            t_sum = prof['matrix_bins_sum'][0] / prof['matrix_bins_sum'][1] / 1e3
            t_sort = prof['matrix_bins_sort'][0] / prof['matrix_bins_sort'][1] / 1e3
            t_np, want = median_time(lambda: host_sums(nam, codes, W, a.levels), max(3, a.reps // 2))
            t_host = t_fetch + t_np
            rel = float(np.max(np.abs(got[0] - want)) / np.max(np.abs(want)))
            lost = lost or t_dev > t_host
            say('  %-16s device call  %9.3f ms  (8nN / t = %.3f TB/s); spans: sort %.3f ms, list + sums + fold %.3f ms '
                '(8nN / t = %.3f TB/s, %.3f of the 8 TB/s HBM peak)'
                % (name, t_dev * 1e3, nbytes / t_dev / 1e12, t_sort * 1e3, t_sum * 1e3, nbytes / t_sum / 1e12,
                   nbytes / t_sum / HBM_PEAK))
            say('  %-16s host route   %9.3f ms  (nam_full %.3f + sums %.3f): host / device = %.1f x%s; largest '
                'difference / largest sum %.1e'
                % ('', t_host * 1e3, t_fetch * 1e3, t_np * 1e3, t_host / t_dev,
                   '' if t_dev <= t_host else '  -- THE DEVICE ROUTE LOST', rel))
        del nam
    eng.drop_expression()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    return 1 if lost else 0


if __name__ == '__main__':
    sys.exit(main())
