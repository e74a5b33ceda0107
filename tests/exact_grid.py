"""Inputs on which the integer counts of the local test have an exact reference, and that reference.

Every entry of X and Yc is a multiple of g = 2^-4 with |.| <= 4.  A dot product of up to 1024 such terms is a multiple
of g^2 = 2^-8 below 2^15: exact in float64 in any summation order, with or without FMA, on the matrix cores and in numpy
alike.  z = |d| / N and z * z are one rounding each, the same on both sides.  So #{i : (|x_i . yc| / N)^2 >= e} has ONE
right answer and a kernel either returns it or is wrong: no tolerance.

Such inputs are full of ties.  `cut_line` puts the cuts on the same 2^-8 grid, so many outputs land exactly ON a cut;
moving every edge up by one ulp moves exactly those outputs across and moving it down moves nothing.

Plain helpers, no fixtures: tests/test_exact_grid_host.py checks them on the CPU for every shape that
tests/test_gpu_local_exact.py runs on the device."""
import numpy as np

G = 2.0 ** -4

# (n cells, N samples, P permutations) of the null-count cases, with what they are there for
NULL_SHAPES = [(2000, 12, 70), (2000, 50, 70), (1000, 100, 33),
               (700, 157, 40), (600, 192, 40), (500, 224, 33), (500, 256, 17),      # the padded row strides of X
               (400, 300, 33),                                                       # more than 256 samples: k_null_big
               (31, 64, 64), (16, 12, 5)]                                            # fewer rows than a tile
T_EDGES = [1, 2, 3, 63, 64, 65, 300, 511, 512]
P_EDGES = [1, 15, 16, 17, 64, 65]
EDGE_SHAPE = (2000, 50)


def grid_matrix(rs, rows, cols, g=G, lim=4.0, zero_rows=0, dup_rows=0, single_row=False):
    """rows x cols multiples of g in [-lim, lim].  Then, on rows drawn without replacement: `zero_rows` rows all zero,
    `dup_rows` rows that repeat another row, and (single_row) one row with a single non-zero entry."""
    M = np.clip(np.rint(rs.randn(rows, cols) / g), -lim / g, lim / g) * g
    special = zero_rows + dup_rows + int(bool(single_row))
    if special:
        if 2 * special > rows:
            raise ValueError('grid_matrix: %d special rows do not fit into %d' % (special, rows))
        pick = rs.permutation(rows)
        M[pick[:zero_rows]] = 0.0
        for k in range(dup_rows):
            M[pick[zero_rows + k]] = M[pick[rows - 1 - k]]
        if single_row:
            r = pick[zero_rows + dup_rows]
            keep = rs.randint(cols)
            v = M[r, keep] if M[r, keep] != 0 else lim
            M[r] = 0.0
            M[r, keep] = v
    return M


def cut_line(D, N, T, g=G):
    """(d, edges): T cuts d = c0 + s * arange(T) on the grid of the products (c0 about max|D| / 4, s about max|D| / 400,
    both multiples of g^2) and edges = (d / N)^2 -- an arithmetic progression of cuts, the shape the fast epilogue of
    the f64 kernel and the integer pass take."""
    a = np.abs(D)
    gg = g * g
    s = np.floor(a.max() / 400 / gg) * gg
    c0 = np.ceil(a.max() / 4 / gg) * gg
    d = c0 + s * np.arange(T)
    return d, (d / N) ** 2


def count_ge(values, edges):
    """#{i : values[i] >= e} for every e, by sorting (values without NaN)."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    return (len(v) - np.searchsorted(v, edges, side='left')).astype(np.int64)


def count_gt(values, thr):
    v = np.sort(np.asarray(values, dtype=np.float64))
    return (len(v) - np.searchsorted(v, thr, side='right')).astype(np.int64)


def brute_tails(X, Yc, N, edges):
    """P x T integers #{i : (|X @ Yc|[i, p] / N)^2 >= edges[t]}: the reference's count (_stats.py:47-59) on z^2."""
    z2 = (np.abs(X.dot(Yc)) / N) ** 2
    return np.array([count_ge(z2[:, p], edges) for p in range(z2.shape[1])], dtype=np.int64).reshape(z2.shape[1], len(edges))


def brute_obs(nc, edges, thr):
    """(ranks, num_detected) of the observed coefficients: nc^2 >= e (inclusive) and |nc| > t (strict)."""
    nc = np.asarray(nc, dtype=np.float64)
    return count_ge(nc ** 2, edges), count_gt(np.abs(nc), thr)


def tie_count(a, d):
    """Outputs that sit exactly on one of the cuts."""
    return int(np.isin(a, d).sum())


# The two shapes below a tile have too few outputs (1984 and 80) for 50 of them to sit on a cut with entries up to 4:
# there the entries stay within 1/2, which brings the step of the cut line down to a few 2^-8 -- every grid value in
# range is then a cut -- and (16, 12, 5) takes the seed, out of the first 400, that ties most.
SMALL = {(31, 64, 64): dict(lim=0.5, seed=95), (16, 12, 5): dict(lim=0.5, seed=167)}


def null_case(n, N, P, T=300, seed=None):
    """The inputs of one null-count case: X (n x N, with three zero rows, three repeated rows and one row with a single
    entry where the matrix has room), Yc (N x P), D = X @ Yc, the cut line and its edges.  Seed n + N unless given."""
    small = SMALL.get((n, N, P), {})
    lim = small.get('lim', 4.0)
    rs = np.random.RandomState(small.get('seed', n + N) if seed is None else seed)
    room = n >= 100
    X = grid_matrix(rs, n, N, lim=lim, zero_rows=3 if room else 0, dup_rows=3 if room else 0, single_row=room)
    Yc = grid_matrix(rs, N, P, lim=lim)
    D = X.dot(Yc)
    d, edges = cut_line(D, N, T)
    return dict(X=X, Yc=Yc, D=D, d=d, edges=edges, N=N, ties=tie_count(np.abs(D), d))


def irregular_edges(rs, D, N, T):
    """Squares of T attained values of |D| / N (distinct, ascending, above max / 4): no arithmetic progression, so the
    kernels walk the table for every output -- and every edge is tied with at least one output."""
    a = np.unique(np.abs(D))
    a = a[a >= a.max() / 4]
    pick = np.sort(rs.choice(a, size=min(T, len(a)), replace=False))
    return pick, (pick / N) ** 2


# T and P edges run on one small shape.  The T edges take 256 permutations, so that even the single cut of T = 1 has 50
# outputs sitting on it; the one column of P = 1 takes the seed, out of the first 50, that ties most.
EDGE_P_FOR_T = 256
EDGE_SEED = {1: 43}


def edge_case(P, T):
    n, N = EDGE_SHAPE
    return null_case(n, N, P, T, seed=EDGE_SEED.get(P))


def reference_edges(thr):
    """The reference's edges for thresholds thr (_stats.py:47): thr^2 - atol - rtol thr^2."""
    z2 = np.asarray(thr) ** 2
    return z2 - 1e-8 - 1e-5 * z2


def obs_case(n=3000, N=50, seed=1):
    """Observed coefficients with ties: nc = (X @ y) / N with X and y on the grid (one rounding, the division), and
    threshold sets that sit ON attained values of |nc|.  Returns dict(X, y, nc, sets={name: thr})."""
    rs = np.random.RandomState(seed)
    X = grid_matrix(rs, n, N, zero_rows=3, dup_rows=3, single_row=True)
    y = grid_matrix(rs, N, 1)[:, 0]
    nc = X.dot(y) / N
    a = np.abs(nc)
    top = a.max()
    vals = np.unique(a[a > 0])
    pick = np.sort(rs.choice(vals, size=150, replace=False))
    attained = np.sort(np.concatenate([pick, np.nextafter(pick, np.inf), np.nextafter(pick, 0.0)]))
    d, _ = cut_line(X.dot(y), N, 300)
    sets = {
        'attained': attained,                                                      # 450: value, one ulp below, one above
        'line': d / N,                                                             # arithmetic, on the grid of nc
        'duplicate_first': np.concatenate([pick[:1], pick]),                       # thr[0] == thr[1]: no step to guess with
        'above_max': np.concatenate([pick, [top, np.nextafter(top, np.inf), 1.5 * top, 2.0 * top]]),
        'one': pick[75:76], 'two': pick[[40, 110]], 'three': pick[[20, 75, 130]],
    }
    return dict(X=X, y=y, nc=nc, N=N, sets=sets)


def obs_ties(nc, thr):
    """Cells whose |nc| IS one of the thresholds."""
    return int(np.isin(np.abs(nc), thr).sum())
