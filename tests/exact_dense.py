"""Integer inputs on which the f64 matrix-core products X^T X and X . B have ONE right answer, the shapes at which a
workgroup of those kernels loops, and a transcription of the dispatch that picks the kernel.

X holds integers: entries in -8 ... 8, the last column minus the row sum (the row then sums to zero), every row plus an
integer m_i in -3 ... 3.  The row mean -- k_xb and k_xb_res divide the row sum by N -- is then exactly m_i and the
centred rows are integers.  B, M and W hold integers in -2 ... 2.  Every partial sum of every product is an integer
below 2^53, so the MFMA chains in any order, the fixed-order sum of the per-workgroup tiles and a float64 BLAS product
all give the same bits, and a kernel either returns them or is wrong: no tolerance.  (For X^T X the partial sums of
entry (i, j) are bounded by sqrt(G_ii G_jj) <= max |G|, so the bound on the result is the bound on all of them; for
X . B `xb_bound` bounds them by the product of the absolute values.)

gram_plan() and xb_plan() restate mfma.hip:gram_plan / launch_gram_range / launch_gram_t and mfma.hip:launch_xb
(c_api.hip:x_ld for the row stride) in Python -- what a case is FOR (which kernel, how many slabs or tiles a workgroup
walks, a ragged end) is then asserted by tests/test_dense_exact_host.py instead of being a comment.  Whoever changes the
dispatch changes these and GRAM_CASES / XB_CASES with it.

Plain helpers, no fixtures: tests/test_gpu_dense_exact.py runs the cases on the device."""
import numpy as np

LIMIT = 2.0 ** 53
POISON = 2.0 ** 20
POISON_ROWS = 64
LDS_SOFT = 150 * 1024                   # what the planners leave of the 160 KiB of LDS


def int_matrix(rs, n, N, lim=8, mean_lim=3):
    """(X, m): n x N float64 holding integers, row i with mean exactly m[i]."""
    X = rs.randint(-lim, lim + 1, size=(n, N)).astype(np.int64)
    X[:, -1] -= X.sum(axis=1)
    m = rs.randint(-mean_lim, mean_lim + 1, size=n).astype(np.int64)
    X += m[:, None]
    return X.astype(np.float64), m.astype(np.float64)


def small_matrix(rs, rows, cols, lim=2):
    """rows x cols integers in -lim ... lim; a square one is not symmetric (M and M^T must not be interchangeable)."""
    M = rs.randint(-lim, lim + 1, size=(rows, cols)).astype(np.float64)
    if rows == cols and rows > 1 and np.array_equal(M, M.T):
        M[0, 1] = M[1, 0] + 1.0
    return M


def poison(n, N):
    """What is uploaded ahead of a case: the same N, POISON_ROWS more rows, every entry 2^20.  The X buffer only grows,
    so the rows behind the case keep these values, and a kernel that reads past the last row changes an integer."""
    return np.full((n + POISON_ROWS, N), POISON)


def xb_bound(X, *Bs):
    """max over all entries of |X| . |B_1| . |B_2| ...: bounds every partial sum of the chained products."""
    a = np.abs(X)
    for B in Bs:
        a = a.dot(np.abs(B))
    return a.max()


# ----------------------------------------------------------------------- the dispatch, restated
def x_ld(N):
    ld = (N + 3) // 4 * 4
    if ld > 128 and (ld * 8) % 256 == 0 and ld + 4 <= 256:
        ld += 4
    return ld


def gram_plan(n, N, blk_small=True):
    """Kernel family, slab height, workgroup cap and the walk of the slabs for X^T X of an n x N matrix."""
    nt = (N + 15) // 16
    ntri = nt * (nt + 1) // 2
    ldp = 16 * nt + (0 if nt & 1 else 16)
    ldx = x_ld(N)
    slab = 32 if 32 * ldp * 8 <= LDS_SOFT else 16
    assert slab * ldp * 8 <= 160 * 1024
    nslab = (n + slab - 1) // slab
    cap = min(512, max(1, (1 << 30) // (ntri * 2048)))
    ng = (nt + 2) // 3
    nblk = ng * (ng + 1) // 2
    two_slabs = slab == 32 and 2 * 32 * ldp * 8 <= LDS_SOFT and ldx <= 320
    passes = 1
    if (nt >= 11 or (nt >= 6 and blk_small)) and nblk <= 16 and two_slabs:
        nw = 16 if nt >= 11 else (4 if nblk <= 4 else (8 if nblk <= 8 else 12))
        per_cu = 2 if 4 * 32 * ldp * 8 <= LDS_SOFT and nw <= 8 else 1
        cap = min(cap, 256 * per_cu)
        kernel = 'k_gram_blk<%d>' % nw
        assert 64 * nw * (6 if nw == 4 else 5) * 2 >= 32 * ldx          # the prefetch registers cover a slab
    else:
        tpw = min((ntri + 15) // 16, 9)
        passes = (ntri + 16 * tpw - 1) // (16 * tpw)
        kernel = ('k_gram_db<%d>' % tpw) if two_slabs else ('k_gram<%d,16,%d>' % (tpw, slab))
    nblocks = max(1, min(nslab, cap))
    return dict(kernel=kernel, slab=slab, cap=cap, nblocks=nblocks, nslab=nslab, passes=passes, ldx=ldx,
                slabs=(nslab + nblocks - 1) // nblocks, last_rows=n - (nslab - 1) * slab)


def xb_plan(n, N, ncols):
    """Kernel and tile walk of X . B for an n x N matrix X and B with ncols columns."""
    ldx = x_ld(N)
    kq = ldx // 4
    ldb = (ncols + 15) // 16 * 16
    ntile = (n + 15) // 16
    if kq > 64:
        parts = [min(64, kq - q0) for q0 in range(0, kq, 64)]
        return dict(kernel='k_xb<%s,2> k-split' % '+'.join(map(str, parts)), ntile=ntile, tiles=1, strips=(ldb + 31) // 32,
                    last_rows=n - (ntile - 1) * 16)
    nct = (ldb + 63) // 64 * 4
    if kq <= 32 and 8 * ldx * (16 * nct + 16) <= 160 * 1024 and ntile >= 64:
        grid = min((ntile + 15) // 16, 512)
        return dict(kernel='k_xb_res<%d>' % kq, ntile=ntile, tiles=(ntile + 16 * grid - 1) // (16 * grid), strips=nct // 4,
                    last_rows=n - (ntile - 1) * 16)
    ns = 4 if kq <= 32 else 2
    return dict(kernel='k_xb<%d,%d>' % (kq, ns), ntile=ntile, tiles=1, strips=(ldb + 16 * ns - 1) // (16 * ns),
                last_rows=n - (ntile - 1) * 16)


# ----------------------------------------------------------------------- the cases
def loop_rows(cap, slab, slabs):
    """Rows with which the first six workgroups of `cap` walk `slabs` slabs and the last slab holds 7 rows."""
    return cap * slab * (slabs - 1) + 5 * slab + 7


# (N, n, CNA_GRAM_BLK_SMALL, kernel, workgroup cap, slab height, slabs of the busiest workgroups, grid.y passes)
GRAM_CASES = [
    (48, 32935, 1, 'k_gram_db<1>', 512, 32, 3, 1),
    (80, 32935, 1, 'k_gram_db<1>', 512, 32, 3, 1),           # 5 tiles a side: stays off the block kernel
    (96, 32935, 1, 'k_gram_blk<4>', 512, 32, 3, 1),          # ldx = 96: all that its 6 prefetch registers cover
    (144, 32935, 1, 'k_gram_blk<8>', 512, 32, 3, 1),         # two workgroups per CU
    (160, 16551, 1, 'k_gram_blk<12>', 256, 32, 3, 1),        # ldx = 164 (padded stride)
    (200, 16551, 1, 'k_gram_blk<16>', 256, 32, 3, 1),
    (240, 16551, 1, 'k_gram_blk<16>', 256, 32, 3, 1),
    (256, 32935, 1, 'k_gram_db<9>', 512, 32, 3, 1),
    (272, 32935, 1, 'k_gram_db<9>', 512, 32, 3, 2),          # the widest the two-slab kernel takes
    (300, 16551, 1, 'k_gram<9,16,32>', 512, 32, 2, 2),       # single buffer
    (576, 16551, 1, 'k_gram<9,16,32>', 512, 32, 2, 5),       # 32-row slabs at their LDS limit
    (640, 8279, 1, 'k_gram<9,16,16>', 512, 16, 2, 6),        # 16-row slabs
    (1024, 4119, 1, 'k_gram<9,16,16>', 252, 16, 2, 15),      # the cap that keeps the partial tiles under 1 GiB
    (96, 32935, 0, 'k_gram_db<2>', 512, 32, 3, 1),           # the tile-per-wave kernel where the block kernel serves
    (144, 32935, 0, 'k_gram_db<3>', 512, 32, 3, 1),
    (160, 32935, 0, 'k_gram_db<4>', 512, 32, 3, 1),          # (its cap is 512, not the block kernel's 256)
]
GRAM_SMALL = [(N, n) for N in (48, 96, 200, 640) for n in (1, 31, 33)]

# (N, n, kernel of the N x N products, tiles of the busiest waves): X . W (N x N and N x 5), then X <- (X - m) . M^T
# and X <- X . M2^T in place
XB_CASES = [
    (4, 1029, 'k_xb_res<1>', 1), (50, 1029, 'k_xb_res<13>', 1),
    (100, 1029, 'k_xb_res<25>', 1), (128, 1029, 'k_xb_res<32>', 1),      # two 4-tile strips of B from 65 columns on
    (4, 1008, 'k_xb<1,4>', 1), (50, 1008, 'k_xb<13,4>', 1), (100, 1008, 'k_xb<25,4>', 1), (128, 1008, 'k_xb<32,4>', 1),
    (8, 131155, 'k_xb_res<2>', 2),                                       # 512 x 16 waves take a second tile
    (132, 1029, 'k_xb<33,2>', 1), (256, 1029, 'k_xb<64,2>', 1),
    (260, 1029, 'k_xb<64+1,2> k-split', 1), (520, 1029, 'k_xb<64+64+2,2> k-split', 1),
]


def gram_case(N, n):
    rs = np.random.RandomState(7 * N + n % 1000)
    return int_matrix(rs, n, N)[0]


def xb_case(N, n):
    """X, its row means and the integer operands W (N x N), W5 (N x 5), M, M2 (N x N)."""
    rs = np.random.RandomState(11 * N + n % 1000)
    X, m = int_matrix(rs, n, N)
    return dict(X=X, m=m, W=small_matrix(rs, N, N), W5=small_matrix(rs, N, 5), M=small_matrix(rs, N, N),
                M2=small_matrix(rs, N, N))
