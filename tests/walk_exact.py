"""Inputs and references for the walk kernels (csrc/diffuse.hip, walk.hip) that tell an indexing fault from a rounding
fault.  numpy, scipy and the standard library only.

The walk:  colsums = A.sum(axis=0) + w;  s <- A.(s / colsums) + w * s / colsums  (_nam.py:28,33), NAM = s / C.

EXACT family.  Any sparsity pattern; every stored entry of a column is w (the self weight, a power of two, 1 by default)
except one, which takes what is left of 2^k - w, with 2^k the smallest power of two that leaves it at least w.  Every
column sum, self weight included, is then a power of two (an empty column: 0 + w), every entry of every state is a
dyadic rational, and -- as long as the numerators over one common power-of-two denominator stay below 2^53, which
`exact_walk` asserts -- every product and every partial sum is exact in float64 in any order, fused or not.
The reference keeps int64 numerators (scipy's int64 A.dot plus the self term, a shift per row for the column sums),
converts to float64 once and divides by the per-sample counts once with numpy's correctly rounded `/`.  A kernel that
disagrees with it has read a wrong column, lost an edge, written a padding column or kept a stale accumulator; it has
not rounded differently.

ROUNDING family.  The same patterns with float32 / float64 weights log-uniform over 40 binades: only a multiply followed
by an add, edge by edge in the stored order of the row, the self term after the neighbours, reproduces the bits.
`sequential_walk` restates exactly that (the `mode='f64'` flow of oracle/cna_oracle.py:diffusion_step, whose scipy
A.dot is the second opinion the host test compares it with).

PATTERNS.  Functions of (n, N, seed) -> Pattern (CSR with int32 indices in the stored, unsorted order, sample codes with
every sample owning a cell, a mask of the entries whose stored weight is 0.0, and what the pattern was designed to hold).
"""
import collections

import numpy as np
import scipy.sparse as sp

Pattern = collections.namedtuple('Pattern', 'n N indptr indices codes zero info')

# row degrees on both sides of every batch size of the step kernels: k_nam_step takes U = 8, 10 or 4 neighbour rows at a
# time with a half batch for a short tail, k_nam_step_sparse 5 and a ragged tail of 1 - 4, k_nam_step_pair 32 records per
# half-wave in fours, and every kernel 64 edges per load
LADDER = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 15, 16, 17, 31, 32, 33, 63, 64, 65, 69, 72, 73, 127, 128, 129, 300)
# ... laid out so that rows 2i, 2i + 1 (one wave of k_nam_step_pair when the device keeps the caller's order) pair a long
# row with a short or an empty one
LADDER_CYCLE = (300, 0, 33, 1, 32, 32, 65, 64, 129, 2, 128, 3, 127, 4, 73, 5, 72, 6, 69, 7, 63, 8, 31, 9, 17, 10, 16, 11,
                15, 0)
DESIGNED_ROW_PAIRS = ((300, 0), (33, 1), (32, 32), (65, 64))
LADDER_MIN_EXTRA = 330        # the widths test walks n = N + 330 + (0 ... 39) cells
SP_CAP = 64                   # pairs a row of the compressed state holds (diffuse.hip)


def _codes(rs, n, N):
    codes = np.concatenate([np.arange(N), rs.randint(0, N, size=n - N)]).astype(np.int64)
    rs.shuffle(codes)
    return codes


def ladder(n, N, seed, balanced=False):
    """Row r has LADDER_CYCLE[r % 30] neighbours: distinct, never r itself, in random stored order.  balanced: the columns
    are handed out round robin instead of at random, so that no column collects more entries than the mean degree plus
    a few (no hub columns: small column sums, narrow states)."""
    cyc = LADDER_CYCLE
    if n < max(N, max(cyc) + 1):
        raise ValueError('ladder: n must be at least max(N, largest degree + 1)')
    rs = np.random.RandomState(seed)
    deg = np.array([cyc[r % len(cyc)] for r in range(n)], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.empty(indptr[-1], dtype=np.int32)
    nxt = 0
    for r in range(n):
        d = int(deg[r])
        if not d:
            continue
        if balanced:
            c = (nxt + np.arange(d + 1)) % n
            c = c[c != r][:d]
            nxt = int(c[-1] + 1) % n
            c = rs.permutation(c)
        else:
            c = rs.choice(n - 1, d, replace=False)
            c = c + (c >= r)
        indices[indptr[r]:indptr[r + 1]] = c
    return Pattern(n, N, indptr, indices, _codes(rs, n, N), np.zeros(len(indices), dtype=bool),
                   dict(degrees=sorted(set(cyc))))


def _layout(kind, N, m):
    """m distinct samples: the first m, the last m (all of them in the last 64-column chunk when N is a multiple of 64
    and m <= 64), or spread over the whole sample axis (the running pair count then crosses every chunk)."""
    if kind == 'head':
        return np.arange(m)
    if kind == 'tail':
        return np.arange(N - m, N)
    z = np.unique(np.round(np.linspace(0, N - 1, m)).astype(np.int64))
    assert len(z) == m
    return z


def pair_limit(n, N, seed):
    """Rows on both sides of the 64 pairs of the compressed state, and rows that gather them.

    Cells: a pool (cell j carries sample j, 0 <= j < N), fillers (8 samples over 136 cells), then
      targets    one row per (layout, count in 62 ... 65, own sample among the neighbours' samples or not): its state after
                 the first step has exactly `count` non-zero samples, the row's own included; and per layout a row with 65
                 distinct neighbour samples one of whose edges has the stored weight 0.0 (64 non-zeros: still pairs);
      gatherers  one row of 12 edges per target with the target at edge (5 x index mod 12) -- inside the first or the second
                 batch of five, or in the ragged tail --, and one row of 130 edges per overflowed target: 64 edges
                 without an overflowed neighbour (the loop without the test), 64 with exactly one, a tail of two.
    Every other row has 0 ... 6 random neighbours.  info: targets = [(row, count, dense)], gathered = {target row:
    [(gatherer row, edge position)]}."""
    if N < 96:
        raise ValueError('pair_limit: the compressed state is kept from 96 samples on')
    rs = np.random.RandomState(seed)
    NF = PAIR_LIMIT_FILLERS
    pool0, fill0 = 0, N
    specs = _pair_limit_specs()
    t0 = fill0 + NF
    n_dense = sum(1 for s in specs if s[1] > SP_CAP and not s[3])
    g0 = t0 + len(specs)
    n_min = pair_limit_min_n(N)
    assert n_min == g0 + len(specs) + n_dense
    if n < n_min:
        raise ValueError('pair_limit: n must be at least %d' % n_min)
    codes = np.empty(n, dtype=np.int64)
    codes[:N] = np.arange(N)
    codes[fill0:fill0 + NF] = np.arange(NF) % 8
    codes[t0:] = rs.randint(0, N, size=n - t0)
    rows = [None] * n
    zero_at = {}
    targets = []
    for i, (kind, cnt, own_in, with_zero) in enumerate(specs):
        r = t0 + i
        Z = _layout(kind, N, cnt)
        own = int(Z[rs.randint(cnt)])
        codes[r] = own
        nb = Z if own_in else Z[Z != own]
        nb = rs.permutation(nb)                       # pool cell j carries sample j
        rows[r] = pool0 + nb
        nz = cnt
        if with_zero:
            k = int(rs.choice(np.flatnonzero(nb != own)))
            zero_at[r] = k
            nz = cnt - 1
        targets.append((r, nz, nz > SP_CAP))
    gathered = {}
    g = g0
    for i, (r, nz, dense) in enumerate(targets):
        other = rs.choice(np.r_[np.arange(N + NF), [t for t, _, d in targets if not d and t != r]], 11, replace=False)
        pos = (5 * i) % 12
        rows[g] = np.insert(other, pos, r)
        gathered.setdefault(r, []).append((g, pos))
        g += 1
    for r, nz, dense in targets:
        if not dense:
            continue
        fill = rs.permutation(np.arange(fill0, fill0 + NF))[:129]
        pos = 64 + int(rs.randint(64))
        rows[g] = np.insert(fill, pos, r)
        gathered[r].append((g, pos))
        g += 1
    assert g == n_min
    for r in range(n):
        if rows[r] is None:
            d = int(rs.randint(0, 7))
            c = rs.choice(n - 1, d, replace=False)
            rows[r] = c + (c >= r)
    deg = np.array([len(x) for x in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    zero = np.zeros(len(indices), dtype=bool)
    for r, k in zero_at.items():
        zero[indptr[r] + k] = True
    return Pattern(n, N, indptr, indices, codes, zero, dict(targets=targets, gathered=gathered))


PAIR_LIMIT_FILLERS = 136


def _pair_limit_specs():
    """(layout, non-zero samples before a stored 0.0 is counted out, own sample among the neighbours', one edge stored
    as 0.0)"""
    specs = []
    for kind in ('head', 'tail', 'spread'):
        for cnt in (62, 63, 64, 65):
            for own_in in (True, False):
                specs.append((kind, cnt, own_in, False))
        specs.append((kind, 65, True, True))
    return specs


def pair_limit_min_n(N):
    """pool + fillers + targets + one 12-edge gatherer per target + one 130-edge gatherer per overflowed target"""
    specs = _pair_limit_specs()
    return N + PAIR_LIMIT_FILLERS + 2 * len(specs) + sum(1 for s in specs if s[1] > SP_CAP and not s[3])


def collisions(n, N, seed):
    """130 cells of one sample; row N + 130 has 64 of them as its neighbours, row N + 131 all 130: every term of the first
    step lands in one column of the wave's accumulator (same-address adds must retire in lane order = CSR order, the
    assumption k_nam_first states), and the second load of 64 edges lands where the first did."""
    if n < N + 132:
        raise ValueError('collisions: n must be at least N + 132')
    rs = np.random.RandomState(seed)
    codes = np.empty(n, dtype=np.int64)
    codes[:N] = np.arange(N)
    one = N // 2
    codes[N:N + 130] = one
    codes[N + 130:] = rs.randint(0, N, size=n - N - 130)
    rows = []
    for r in range(n):
        if r == N + 130:
            rows.append(rs.permutation(np.arange(N, N + 130))[:64])
        elif r == N + 131:
            rows.append(rs.permutation(np.arange(N, N + 130)))
        else:
            d = int(rs.randint(0, 7))
            c = rs.choice(n - 1, d, replace=False)
            rows.append(c + (c >= r))
    deg = np.array([len(x) for x in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    return Pattern(n, N, indptr, indices, codes, np.zeros(len(indices), dtype=bool),
                   dict(rows=(N + 130, N + 131), sample=one))


# --------------------------------------------------------------------------------------------------------- weights
def exact_units(pat):
    """int64 weight of every stored entry in units of the self weight, and k per column with (column sum + self weight) =
    2^k units: ones, the last stored entry of a column takes the remainder; entries of pat.zero stay 0 and do not count."""
    nnz = len(pat.indices)
    live = ~pat.zero
    m = np.bincount(pat.indices[live], minlength=pat.n).astype(np.int64)
    k = np.zeros(pat.n, dtype=np.int64)
    while (((1 << k) - 1) < m).any():
        k += ((1 << k) - 1) < m
    units = live.astype(np.int64)
    order = np.flatnonzero(live)                                 # CSR order: ascending row, position in row
    last = np.full(pat.n, -1, dtype=np.int64)
    last[pat.indices[order]] = order                              # (later assignments win: the last stored entry)
    cols = np.flatnonzero(m > 0)
    units[last[cols]] = (1 << k[cols]) - 1 - (m[cols] - 1)
    assert nnz == 0 or units.min() >= 0
    assert (np.bincount(pat.indices, weights=units, minlength=pat.n).astype(np.int64) == (1 << k) - 1).all()
    return units, k


def matrix(pat, data):
    return sp.csr_matrix((np.asarray(data), pat.indices, pat.indptr), shape=(pat.n, pat.n))


def exact_matrix(pat, dtype=np.float32, self_weight=1):
    units, _ = exact_units(pat)
    return matrix(pat, (units * float(self_weight)).astype(dtype))


def rounding_matrix(pat, dtype, seed):
    """Weights log-uniform over 40 binades; the entries of pat.zero are stored zeros."""
    rs = np.random.RandomState(seed)
    v = np.exp2(rs.uniform(-40, 0, size=len(pat.indices))).astype(dtype)
    v[pat.zero] = 0
    return matrix(pat, v)


def onehot(pat):
    S = np.zeros((pat.n, pat.N), dtype=np.int64)
    S[np.arange(pat.n), pat.codes] = 1
    return S


def counts(pat):
    return np.bincount(pat.codes, minlength=pat.N).astype(np.float64)


# ------------------------------------------------------------------------------------------------------ references
def _bit_length(x):
    x = x.copy()
    out = np.zeros(x.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (x >> s) > 0
        out += s * big
        x = np.where(big, x >> s, x)
    return out + (x > 0)


def significand_bits(num):
    """Largest width, in bits, of the significand of num / 2^anything over the entries of an int64 array."""
    num = np.asarray(num, dtype=np.int64)
    if not num.size or num.max() == 0:
        return 0
    nz = num[num > 0]
    low = nz & -nz
    return int((_bit_length(nz) - _bit_length(low) + 1).max())


ExactWalk = collections.namedtuple('ExactWalk', 's t_bits s_bits num_bits')


def exact_walk(pat, nsteps, s0=None, self_weight=1):
    """The states s_1 ... s_nsteps of the exact family as float64 arrays, from integer arithmetic alone.

    Numerators over one common denominator 2^D, in int64.  With A = w A_units and colsums = w 2^k the self weight drops
    out: s' = A.T + w T = A_units.(s / 2^k) + s / 2^k, so s / 2^k is a shift per row to the denominator 2^(D + K), K = the
    largest column exponent, and the numerators of s' over it are A_units.dot(shifted) + shifted.  Nothing may exceed
    62 bits (asserted from a bound computed in Python integers before every product) and every numerator stays below
    2^53, which makes every partial sum of every kernel exact.  t_bits / s_bits: the largest significand width among
    the entries of the scaled states T_0 ... T_(nsteps-1) a walk stores between its steps, and of the states s_i."""
    assert np.frexp(float(self_weight))[0] == 0.5            # a power of two
    units, k = exact_units(pat)
    A = matrix(pat, units)
    assert A.dtype == np.int64
    K = int(k.max())
    rowsum = int(np.bincount(np.repeat(np.arange(pat.n), np.diff(pat.indptr)), weights=units, minlength=pat.n).max()) \
        if len(units) else 0
    num = onehot(pat) if s0 is None else np.asarray(s0)
    assert num.dtype == np.int64 and num.min() >= 0
    D = 0
    out, t_bits, s_bits, num_bits = [], [], [], []
    for _ in range(nsteps):
        assert int(num.max()).bit_length() + K <= 62
        T = num << (K - k)[:, None]
        D += K
        t_bits.append(significand_bits(T))
        assert (rowsum + 1) * int(T.max()) < 1 << 62
        num = A.dot(T) + T
        assert num.dtype == np.int64
        num_bits.append(int(num.max()).bit_length())
        assert num_bits[-1] <= 53, 'partial sums would round'
        s_bits.append(significand_bits(num))
        s = np.ldexp(num.astype(np.float64), -D)
        out.append(s)
        g = int((num & -num)[num > 0].min()) if (num > 0).any() else 1        # keep the numerators short
        sh = min(g.bit_length() - 1, D)
        num >>= sh
        D -= sh
    return ExactWalk(out, t_bits, s_bits, num_bits)


def sequential_walk(A, s0, nsteps, self_weight=1):
    """s_1 ... s_nsteps in float64, row by row and entry by entry in the stored order: acc = acc + a * t (a product, then
    a sum), the row's own term last.  (All rows advance together through their e-th entries: the same sequence of
    roundings for every row as a loop over the rows.)"""
    n = A.shape[0]
    indptr, idx = A.indptr.astype(np.int64), A.indices
    val = A.data.astype(np.float64)
    deg = np.diff(indptr)
    cs = column_sums(A, self_weight)
    s = np.asarray(s0, dtype=np.float64)
    byrank = np.argsort(-deg, kind='stable')
    sdeg = deg[byrank]
    out = []
    for _ in range(nsteps):
        T = s / cs[:, None]
        acc = np.zeros_like(T)
        for e in range(int(deg.max()) if n else 0):
            rows = byrank[:np.searchsorted(-sdeg, -e, side='left')]          # rows with more than e entries
            at = indptr[rows] + e
            acc[rows] = acc[rows] + val[at][:, None] * T[idx[at]]
        s = acc + float(self_weight) * T
        out.append(s)
    return out


def column_sums(A, self_weight=1):
    """A.sum(axis=0) + w in float64, every column summed in ascending (row, position in row) order, as scipy sums a CSR."""
    cs = np.zeros(A.shape[1])
    np.add.at(cs, A.indices, A.data.astype(np.float64))          # unbuffered: one add after the other, in CSR order
    return cs + self_weight


def first_diff(got, want, degrees=None, what=''):
    """None when the two arrays hold the same bits (array_equal semantics: NaNs differ); else a message naming the first
    differing (row, column) and the row's degree."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return '%s: shape %s, expected %s' % (what, got.shape, want.shape)
    bad = got != want
    if not bad.any():
        return None
    r, c = np.argwhere(bad)[0]
    return ('%s: %d of %d entries differ, first at row %d (degree %s), column %d: got %r, expected %r; rows that differ: %s'
            % (what, int(bad.sum()), bad.size, r, '?' if degrees is None else int(degrees[r]), c, got[r, c], want[r, c],
               np.flatnonzero(bad.any(axis=1))[:12].tolist()))


# ---------------------------------------------------------------------------------------- the table of the launcher
WIDTHS = (1, 3, 61, 64, 65, 95, 96, 125, 128, 129, 189, 192, 193, 253, 256, 257, 320, 321, 384, 385, 509, 512, 513, 765,
          768, 769, 1021, 1024)
SPARSE_MIN_N = 96


def _round_up(a, b):
    return (a + b - 1) // b * b


def _nq(chunks, table):
    for top, nq in table:
        if chunks <= top:
            return nq
    return table[-1][1]


FIRST_NQ = ((1, 1), (2, 2), (3, 3), (4, 4), (6, 6), (8, 8), (12, 12), (16, 16))
STEP_NQ2 = ((1, 1), (2, 2), (3, 3), (4, 4), (6, 6), (8, 8))
STEP32_NQ4 = ((1, 1), (2, 2), (3, 3), (4, 4))


def dispatch(N, n, step, sparse_min_n=SPARSE_MIN_N, step_wide=False, select=False, in32=False, step32_wide=False):
    """The kernel instantiation diffuse.hip:launch_step_q picks for step `step` (1-based) of a walk over n cells and N
    samples on one rank, restated: (kernel, template sizes ...)."""
    ld = _round_up(N, 4)
    if step == 1:
        nblk = (n + 3) // 4
        cpx = (nblk + 7) // 8
        chunk = 128 if (ld > 64 and cpx > 128) else cpx
        grid = 8 * _round_up(cpx, chunk)
        return ('k_nam_first2' if grid % 16 == 0 else 'k_nam_first', _nq((ld + 63) // 64, FIRST_NQ))
    sparse = sparse_min_n > 0 and N >= sparse_min_n
    if step == 2 and sparse:
        return ('k_nam_step_sparse', _nq((ld // 2 + 63) // 64, STEP_NQ2))
    if ld <= 64 and not step_wide:
        return ('k_nam_step_pair',)
    if in32:
        if ld <= 128 and not step32_wide:
            return ('k_nam_step32h',)
        nq4 = _nq((ld // 4 + 63) // 64, STEP32_NQ4)
        return ('k_nam_step32', nq4, 8 if nq4 <= 2 else 4)
    nq2 = _nq((ld // 2 + 63) // 64, STEP_NQ2)
    return ('k_nam_step', nq2, (8 if select else 10) if nq2 == 2 else 4 if nq2 >= 6 else 8)


def width_cells(N):
    """Cells of the widths test at N samples: N + 330 + (position in WIDTHS mod 8), so that the row counts cover every
    residue mod 8 (partial last wave, partial last workgroup), plus 32 where that makes the widths of one first-step
    instantiation alternate between k_nam_first and k_nam_first2 (the grid is a multiple of 16 workgroups for every
    other block of 32 rows)."""
    i = WIDTHS.index(N)
    nq = dispatch(N, 1000, 1)[1]
    mates = [w for w in WIDTHS if dispatch(w, 1000, 1)[1] == nq]
    want_two = mates.index(N) % 2 == 0
    n = N + LADDER_MIN_EXTRA + i % 8
    if (dispatch(N, n, 1)[0] == 'k_nam_first2') != want_two:
        n += 32
    return n


# ------------------------------------------------------------------------------------ the cases the two test modules share
FAMILIES = ('exact', 'f32', 'f64')
SMALL_ENDS = ((320, 320), (509, 510), (1021, 1024))                  # n = N, N + 1, N + 3
WIDTH_CASES = tuple((N, width_cells(N)) for N in WIDTHS) + SMALL_ENDS
PAIR_LIMIT_N = (96, 130, 257, 513, 1024)
PLACEMENT_N = (7, 33, 64)
STATE32_N = (96, 128, 129, 256, 257, 512, 513, 1024)
DENSE_M = (1, 2, 63, 64, 65, 128, 129, 257, 1024)
DENSE_CELLS = 363
NSTEPS = 3


def pair_limit_cells(N):
    return pair_limit_min_n(N) + PAIR_LIMIT_N.index(N)


def family_matrix(pat, family, self_weight=1):
    if family == 'exact':
        return exact_matrix(pat, np.float32, self_weight)
    return rounding_matrix(pat, np.float32 if family == 'f32' else np.float64, seed=pat.n + pat.N)


def reference_states(pat, family, A, nsteps=NSTEPS, s0=None, self_weight=1):
    """s_1 ... s_nsteps: the integer reference for the exact family, the sequential restatement for the other two."""
    if family == 'exact':
        return exact_walk(pat, nsteps, s0=None if s0 is None else np.asarray(s0, dtype=np.int64), self_weight=self_weight).s
    return sequential_walk(A, onehot(pat) if s0 is None else s0, nsteps, self_weight)


def dense_input(pat, family, m):
    """cells x m start of a dense diffusion: small integers for the exact family, else values over 20 binades, of one sign
    per column (both signs occur; no sum cancels)."""
    rs = np.random.RandomState(7 * m + pat.n)
    if family == 'exact':
        return rs.randint(0, 8, size=(pat.n, m)).astype(np.int64)
    return np.exp2(rs.uniform(-20, 0, size=(pat.n, m))) * np.where(rs.rand(1, m) < 0.5, -1.0, 1.0)
