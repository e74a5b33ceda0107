"""Inputs on which the global F-test (csrc/stats.hip) has ONE right answer, and that answer.

The five kernels compute, per phenotype column, Zc = M.Y / std(M.Y, ddof=1), the squared projections on the first kmax
columns of U, ssered = |Zc|^2, for every k in ks the statistic F and its survival function, and the min-p over ks.
Here every quantity in front of F is exact on the device, in any order of summation:

- a column z holds small integers with an exactly representable mean (zero, or an integer shift) and
  sum (z - mean)^2 / (N - 1) = 4^m, so sd = 2^m and z / sd is exact.  exact_vector() serves an N from three families
  ('ones': +-1 and one 0, odd N; 'pow4': (N-1, -1, ..., -1), N = 4^m; 'pairs': +-v_i found by a bounded search over sums of
  squares) and check_exact() proves it in fractions.Fraction or raises -- there is no inexact fallback;
- U is a signed permutation matrix, or normalised Sylvester-Hadamard blocks H / 2^m (entries +-2^-m, every entry of a
  block takes part in every projection of it) with an identity remainder, its columns shuffled by a stride;
- M is the identity, or I - J/4 on blocks of four rows (identity on the remainder) with Y = z + block-constant integer
  offsets for a z that sums to zero on every block: M.Y = z exactly while every entry of M is used;
- column p is rotated by p and multiplied by 2^((p mod 7) - 3): Zc does not see the scale, a swapped column does.

reference() then forms red, fit and ssefull as Fractions of exact integer dot products, proves each is a float64, takes
F and r2 with the float64 operations of k_gt_ftest in its order, and p from mpmath's regularised incomplete beta at
DPS digits with x formed in multiprecision from the float64 F.  The conventions of f_sf and k_gt_min stand in front.

f_sf_double() restates betacf / incbet / f_sf of stats.hip in Python doubles (math.lgamma, exp, log1p) and counts
iterations; model() restates the five kernels in numpy with the one-line slips a test must notice.  Plain helpers, no
fixtures: tests/test_global_exact_host.py pins them, tests/test_gpu_global_exact.py runs the cases on the device."""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

DPS = 60
PERIOD = 23                       # column p repeats column p - 23 (bar its scale): prime, so no tile width divides it
SWEEP_ODD = (3, 5, 13, 15, 17, 19, 63, 65, 127, 129, 257, 1023)
SWEEP_EVEN = (4, 6, 16, 64, 256, 1024)
SWEEP_P = (1, 15, 16, 17, 63, 64, 65, 257)
NAN = float('nan')


# ----------------------------------------------------------------------- exact columns
@functools.lru_cache(maxsize=None)
def _squares_table(S):
    """(cnt, last): cnt[s] the fewest positive squares that sum to s, last[s] the root of one of them."""
    cnt, last = [0] + [99] * S, [0] * (S + 1)
    for s in range(1, S + 1):
        v = 1
        while v * v <= s:
            if cnt[s - v * v] + 1 < cnt[s]:
                cnt[s], last[s] = cnt[s - v * v] + 1, v
            v += 1
    return cnt, last


def _varied(i):
    """1, 2 or 3 without a short period (mean square 3.75 < 4: the pairs run out before the sum of squares does)."""
    return (1, 2, 1, 3)[(((i * 40503 + 12345) * 2654435761) >> 16) & 3]


def pair_values(N, max_pairs=None, dense=True):
    """(values v_i >= 1, m): at most N // 2 (or max_pairs) pairs +-v_i with 2 sum v_i^2 = (N - 1) 4^m.  dense: as many
    small varied values as still leave a completion, then the fewest squares that complete the sum; else the fewest
    squares alone (a column with small support).  ValueError when m = 0 ... 3 has no solution."""
    qmax = N // 2 if max_pairs is None else min(int(max_pairs), N // 2)
    for m in (1, 2, 3, 0):
        S2 = (N - 1) * 4 ** m
        if S2 % 2 or S2 == 0:
            continue
        S = S2 // 2
        cnt, last = _squares_table(S)
        if cnt[S] > qmax:
            continue
        vals, rem = [], S
        while dense and len(vals) < qmax:
            v = _varied(len(vals))
            if rem - v * v < 0 or cnt[rem - v * v] > qmax - len(vals) - 1:
                break
            vals.append(v)
            rem -= v * v
        while rem:
            vals.append(last[rem])
            rem -= last[rem] ** 2
        assert len(vals) <= qmax
        return vals, m
    raise ValueError('no exact column of %d samples from at most %d pairs' % (N, qmax))


def _is_pow4(fr):
    """fr = 4^m for an integer m (of either sign)."""
    n, d = fr.numerator, fr.denominator
    if n < 1 or (n != 1 and d != 1):
        return False
    v = max(n, d)
    return v & (v - 1) == 0 and (v.bit_length() - 1) % 2 == 0


def check_exact(z):
    """Raise unless the integer vector z is exact for k_cond_scale: its mean is a float64, every (z - mean)^2 and every
    partial sum of them fits 53 bits, the variance (ddof = 1) is 4^m.  Returns m.  All in Fractions."""
    zi = [int(v) for v in z]
    if any(float(v) != w for v, w in zip(zi, z)):
        raise ValueError('not integers')
    N = len(zi)
    if N < 2:
        raise ValueError('need two samples')
    mean = Fraction(sum(zi), N)
    if Fraction(float(mean)) != mean or sum(abs(v) for v in zi) >= 2 ** 53:
        raise ValueError('the mean of the column is not a float64')
    dev = [Fraction(v) - mean for v in zi]
    den = max(d.denominator for d in dev)
    if den & (den - 1) or sum(d * d for d in dev) * den * den >= 2 ** 53:
        raise ValueError('the squared deviations do not sum exactly')
    var = sum(d * d for d in dev) / (N - 1)
    if not _is_pow4(var):
        raise ValueError('variance %s of the column is no power of four' % var)
    return (max(var.numerator, var.denominator).bit_length() - 1) // 2 * (1 if var.denominator == 1 else -1)


def kinds(N, paired=False):
    """The families that serve N; paired: only those laid out as adjacent (+v, -v) pairs (block centring keeps them)."""
    out = []
    try:
        pair_values(N)
        out.append('pairs')
    except ValueError:
        pass
    if N % 2 == 1 and N >= 3:
        out.append('ones')
    if not paired and N >= 4 and N & (N - 1) == 0 and (N.bit_length() - 1) % 2 == 0:
        out.append('pow4')
    return out


@functools.lru_cache(maxsize=None)
def _vector(N, kind):
    if kind == 'pairs':
        vals, _ = pair_values(N)
    elif kind == 'sparse':
        vals, _ = pair_values(N, dense=False)
    elif kind == 'ones':
        if N % 2 == 0 or N < 3:
            raise ValueError('the +-1 family needs an odd N')
        vals = [1] * (N // 2)
    elif kind == 'pow4':
        if N < 4 or N & (N - 1) or (N.bit_length() - 1) % 2:
            raise ValueError('N is no power of four')
        z = np.full(N, -1, dtype=np.int64)
        z[0] = N - 1
        check_exact(z)
        return z
    else:
        raise ValueError(kind)
    z = np.zeros(N, dtype=np.int64)
    for i, v in enumerate(vals):
        z[2 * i], z[2 * i + 1] = v, -v
    check_exact(z)
    return z


def exact_vector(N, kind=None):
    """An integer vector of N samples that check_exact() accepts (pairs adjacent, zeros last); ValueError when the
    family -- or, with kind None, every family -- cannot serve N."""
    if kind is None:
        ks = kinds(N)
        if not ks:
            raise ValueError('no exact column of %d samples' % N)
        kind = ks[0]
    return _vector(int(N), kind).copy()


def block_centring(N):
    """I - J/4 on blocks of four rows, the identity on the N mod 4 rows behind them."""
    M = np.eye(N)
    for b in range(N // 4):
        M[4 * b:4 * b + 4, 4 * b:4 * b + 4] -= 0.25
    return M


def columns(N, P, block=False, shift=False):
    """dict(Z, Y, M, scale): Z (N x P, integers as float64) is what M.Y / scale must be, column by column.  Column p
    takes the families of N in turn, rotated by p mod PERIOD (block: by whole pairs, so that every block of four still
    sums to zero), times 2^((p mod 7) - 3); shift (identity M only): plus the integer (p mod 5) - 2, so that the mean
    the kernel subtracts is not zero.  Raises ValueError when N has no exact column of the layout asked for."""
    fam = kinds(N, paired=block)
    if not fam or (block and N < 4):
        raise ValueError('no exact column of %d samples%s' % (N, ' in pairs' if block else ''))
    Z = np.empty((N, P))
    for p in range(P):
        q = p % PERIOD
        z = exact_vector(N, fam[q % len(fam)])
        if block:
            n2 = N // 2 * 2
            z[:n2] = np.roll(z[:n2], 2 * q)
        else:
            z = np.roll(z, q) * (-1 if q % 2 else 1)
            if shift:
                z = z + (p % 5 - 2)
                check_exact(z)
        Z[:, p] = z
    scale = 2.0 ** (np.arange(P) % 7 - 3)
    if block:
        M = block_centring(N)
        off = np.zeros((N, P))
        for b in range(N // 4):
            off[4 * b:4 * b + 4] = (5 * b + 3 * np.arange(P)) % 7 - 3
        Y = (Z + off) * scale
        M4, Yi = np.rint(4 * M).astype(np.int64), np.rint(Y / scale).astype(np.int64)
        if not (np.array_equal(M4, 4 * M) and np.array_equal(Yi * scale, Y)
                and np.array_equal(M4.dot(Yi), 4 * Z.astype(np.int64))):
            raise ValueError('M.Y is not the exact column')
    else:
        M, Y = np.eye(N), Z * scale
    return dict(Z=Z, Y=Y, M=M, scale=scale)


# ----------------------------------------------------------------------- exact U
def _stride(N):
    g = max(int(0.618 * N), 1)
    while math.gcd(g, N) != 1:
        g += 1
    return g


def perm_u(N, first=()):
    """Signed permutation matrix: column j is +-e_perm[j]; `first` lists the rows of the leading columns, the others
    follow by a stride coprime to N."""
    first = [int(i) for i in first]
    rest = [i for i in ((j * _stride(N) + 1) % N for j in range(N)) if i not in set(first)]
    U = np.zeros((N, N))
    for j, i in enumerate(first + rest):
        U[i, j] = -1.0 if (j * (j + 1) // 2) % 2 else 1.0
    return U


def hadamard_u(N):
    """Block-diagonal normalised Sylvester-Hadamard matrices of orders 4^m (largest first, whole for N = 4^m), the
    identity on the N mod 4 rows left; columns in stride order so that the leading ones come from every block."""
    U = np.zeros((N, N))
    at = 0
    while N - at >= 4:
        n = 4
        while n * 4 <= N - at:
            n *= 4
        H = np.ones((1, 1))
        while len(H) < n:
            H = np.block([[H, H], [H, -H]])
        U[at:at + n, at:at + n] = H / math.sqrt(n)
        at += n
    U[at:, at:] = np.eye(N - at)
    U = U[:, [(j * _stride(N)) % N for j in range(N)]]
    assert np.array_equal(U.T.dot(U), np.eye(N))
    return U


# ----------------------------------------------------------------------- the reference
@functools.lru_cache(maxsize=None)
def f_sf_mp(f, d1, d2):
    """The F survival function as f_sf of stats.hip defines it, the body from mpmath: (float64, mpf or None)."""
    if not d2 > 0 or f != f:
        return NAN, None
    if f <= 0:
        return 1.0, None
    if f == math.inf:
        return 0.0, None
    with mpmath.workdps(DPS):
        x = mpmath.mpf(d2) / (mpmath.mpf(d2) + mpmath.mpf(d1) * mpmath.mpf(f))
        v = mpmath.betainc(mpmath.mpf(d2) / 2, mpmath.mpf(d1) / 2, 0, x, regularized=True)
        return float(v), v


def _as_float(fr):
    f = float(fr)
    if Fraction(f) != fr:
        raise ValueError('%s is no float64: the case is not exact' % fr)
    return np.float64(f)


def ftest_terms(Z, U, ks, r):
    """Per column and k in ks: (F, p, r2) as float64 (K x P arrays), F and r2 from exact red / fit / ssefull with the
    float64 operations of k_gt_ftest.  A column that is not finite, or constant, is NaN throughout (what IEEE arithmetic
    makes of it in k_cond_gemm and k_cond_scale)."""
    N, P = Z.shape
    ks = [int(k) for k in ks]
    kmax = max(ks)
    SH = 10
    Ui = np.rint(U[:, :kmax] * 2 ** SH).astype(np.int64)
    if not np.array_equal(Ui, U[:, :kmax] * 2 ** SH):
        raise ValueError('U is not on the 2^-10 grid')
    ok = np.isfinite(Z).all(axis=0)
    Zi = np.where(ok, Z, 0).astype(np.int64)
    if not np.array_equal(np.where(ok, Z, 0), Zi) or np.abs(Ui).sum(axis=0).max() * np.abs(Zi).max() >= 2 ** 31:
        raise ValueError('Z does not hold small integers')
    C2 = np.cumsum(Ui.T.dot(Zi).astype(object) ** 2, axis=0)          # Python integers: no overflow
    F, Pv, R2 = (np.full((len(ks), P), NAN) for _ in range(3))
    memo = {}
    for p in range(P):
        s1, s2 = int(Zi[:, p].sum()), int((Zi[:, p] ** 2).sum())
        if not ok[p] or s2 * N == s1 * s1:
            continue
        key = (s1, s2) + tuple(C2[k - 1, p] for k in ks)
        if key not in memo:
            var = Fraction(s2 * N - s1 * s1, N * (N - 1))
            if not _is_pow4(var) or Fraction(float(Fraction(s1, N))) != Fraction(s1, N):
                raise ValueError('column %d is not exact' % p)
            red = Fraction(s2) / var
            out = []
            for a, k in enumerate(ks):
                fit = Fraction(C2[k - 1, p], 4 ** SH) / var
                red64, sse = _as_float(red), _as_float(red - fit)
                _as_float(fit)
                with np.errstate(all='ignore'):
                    f = ((red64 - sse) / np.float64(k)) / (sse / np.float64(N))
                    r2 = np.float64(1.0) - sse / red64
                out.append((float(f), f_sf_mp(float(f), k, N - (1 + r + k))[0], float(r2)))
            memo[key] = out
        for a, (f, pv, r2) in enumerate(memo[key]):
            F[a, p], Pv[a, p], R2[a, p] = f, pv, r2
    return F, Pv, R2


def reference(Z, U, ks, r):
    """(kidx int32, p, r2) per column as k_gt_min states them: the first k of the smallest non-NaN p, and
    (-1, nan, nan) where no k has one."""
    _, Pv, R2 = ftest_terms(Z, U, ks, r)
    P = Pv.shape[1]
    kidx, p, r2 = np.full(P, -1, dtype=np.int32), np.full(P, NAN), np.full(P, NAN)
    for c in range(P):
        for a in range(Pv.shape[0]):
            v = Pv[a, c]
            if v == v and (kidx[c] < 0 or v < p[c]):
                kidx[c], p[c], r2[c] = a, v, R2[a, c]
    return kidx, p, r2


# ----------------------------------------------------------------------- the sweep of section (a)
def sweep_setup(N):
    """(U kind, block M, r, ks) of the P sweep at N: the four U x M combinations and r in {0, 3} in turn over the
    sweep's N (block centring from N = 6 on: below, the paired columns are copies of one; r = 3 where it leaves a valid k)."""
    i = (SWEEP_ODD + SWEEP_EVEN).index(N)
    block = i % 2 == 1 and N >= 6 and bool(kinds(N, paired=True))
    r = 3 if (i // 2) % 2 == 1 and N >= 13 else 0
    top = N - 2 - r
    ks = sorted({k for k in (1, 2, min(5, top), min(17, top)) if 1 <= k <= top})
    return ('hadamard' if (i // 4) % 2 == 0 else 'perm'), block, r, ks


def make_u(kind, N, first=()):
    return hadamard_u(N) if kind == 'hadamard' else perm_u(N, first)


@functools.lru_cache(maxsize=None)
def sweep_case(N):
    """The 257-column case of N, its reference computed once; every P of the sweep is its leading columns."""
    kind, block, r, ks = sweep_setup(N)
    c = columns(N, max(SWEEP_P), block=block)
    c.update(N=N, U=make_u(kind, N), ks=ks, r=r, ukind=kind, block=block)
    c['ref'] = reference(c['Z'], c['U'], ks, r)
    return c


def case(N, P, ukind, block, r, ks, shift=False):
    c = columns(N, P, block=block, shift=shift)
    c.update(N=N, U=make_u(ukind, N), ks=list(ks), r=r)
    c['ref'] = reference(c['Z'], c['U'], ks, r)
    return c


# ----------------------------------------------------------------------- the F tail of section (c)
TAIL_D1 = (1, 2, 3, 16, 17, 100)
TAIL_D2 = (1, 2, 3, 10, 100, 500, 1020)             # the last: at most, 1022 - d1 where that is less (N <= 1023)
TAIL_R_MAX = 64
BRANCH_FACTOR = 1.5


def branch_x(d1, d2):
    """incbet(a = d2/2, b = d1/2, x) takes the direct continued fraction below this x, the reflected one from it on."""
    return (0.5 * d2 + 1.0) / (0.5 * d2 + 0.5 * d1 + 2.0)


def _tail_candidates(k, d2):
    """Exact columns of a pairs of +-2^J, b pairs of +-1 and zeros, 2a 4^J + 2b = (N - 1) 4^m, of which the first k
    PCs see hb entries +-2^J, h1 entries +-1 and zeros: (x, N, J, a, b, hb, h1), fit and ssefull both positive."""
    out = []
    N0 = k + d2 + 1
    for N in range(max(N0, 3), min(N0 + TAIL_R_MAX, 1024) + 1):
        for J in range(0, 14):
            for a in range(1, 9):
                big = 2 * a * 4 ** J
                for m in range(0, J + 1):
                    twob = (N - 1) * 4 ** m - big
                    if twob < 0 or twob % 2:
                        continue
                    if 2 * a + twob > N:
                        break
                    zeros = N - 2 * a - twob
                    ss = big + twob
                    for hb in range(0, min(2 * a, k) + 1):
                        for h1 in sorted({0, 1, 2, 3, k - hb, twob, max(k - hb - zeros, 0)}):
                            if h1 < 0 or h1 > twob or hb + h1 > k or k - hb - h1 > zeros:
                                continue
                            fit = hb * 4 ** J + h1
                            if fit == 0 or fit == ss or ss >= 2 ** 52:
                                continue
                            out.append((d2 / (d2 + N * fit / (ss - fit)), N, J, a, twob // 2, hb, h1))
    return out


@functools.lru_cache(maxsize=None)
def tail_cases():
    """Exact columns that put (d1, d2, F) where f_sf can go wrong: for every d1 x d2 the x nearest the branch point of
    incbet on either side (kept when within BRANCH_FACTOR of it), the largest and the smallest F on offer, and the
    nearest on offer to p = 1e-10 ... 1e-305 and to 1 - p = 1e-6, 1e-3 (shortlisted by the leading term of the tail).  A list of dict(N, k, r, d2, z): z has the entries seen by the first k PCs in its first k rows."""
    picked = {}
    for k in TAIL_D1:
        for d2 in TAIL_D2:
            d2 = min(d2, 1022 - k)
            cand = sorted(set(_tail_candidates(k, d2)))
            x0 = branch_x(k, d2)
            xs = np.array([c[0] for c in cand])
            want = [int(xs.argmin()), int(xs.argmax())]
            below, above = np.flatnonzero(xs < x0), np.flatnonzero(xs >= x0)
            if len(below) and xs[below].max() * BRANCH_FACTOR >= x0:
                want.append(int(below[xs[below].argmax()]))
            if len(above) and xs[above].min() <= x0 * BRANCH_FACTOR:
                want.append(int(above[xs[above].argmin()]))
            for lp in (-10.0, -50.0, -150.0, -250.0, -283.0, -288.0, -295.0, -305.0):
                near = np.argsort(np.abs(np.log10(xs) * 0.5 * d2 - lp))[:6]         # by the leading term, then by mpmath
                lps = [float(mpmath.log10(f_sf_mp(float(k and (1.0 / xs[i] - 1.0) * d2 / k), k, d2)[1])) for i in near]
                want.append(int(near[int(np.abs(np.array(lps) - lp).argmin())]))
            for lq in (-6.0, -3.0):
                want.append(int(np.abs(np.log10(1.0 - xs + 1e-300) * 0.5 * k - lq).argmin()))
            for i in want:
                picked[(k, d2) + cand[i][1:]] = cand[i]
    out = []
    for (k, d2, N, J, a, b, hb, h1), _ in sorted(picked.items()):
        head = [2 ** J * (-1) ** i for i in range(hb)] + [(-1) ** i for i in range(h1)] + [0] * (k - hb - h1)
        rest = ([2 ** J * (-1) ** i for i in range(hb, 2 * a)] + [(-1) ** i for i in range(h1, 2 * b)]
                + [0] * (N - 2 * a - 2 * b - (k - hb - h1)))
        z = np.array(head + rest, dtype=np.int64)
        assert len(z) == N
        check_exact(z)
        out.append(dict(N=N, k=k, r=N - 1 - k - d2, d2=d2, z=z))
    return out


@functools.lru_cache(maxsize=None)
def tail_table():
    """tail_cases() grouped by (N, k, r) -- one device call each -- with the reference per column:
    [dict(N, k, r, d2, Z, U, F, p, p_mp)]."""
    groups = {}
    for c in tail_cases():
        groups.setdefault((c['N'], c['k'], c['r']), []).append(c['z'])
    out = []
    for (N, k, r), zs in sorted(groups.items()):
        Z = np.array(zs, dtype=np.float64).T
        U = perm_u(N, first=range(k))
        F, Pv, _ = ftest_terms(Z, U, [k], r)
        d2 = N - 1 - r - k
        out.append(dict(N=N, k=k, r=r, d2=d2, Z=Z, U=U, F=F[0], p=Pv[0],
                        p_mp=[f_sf_mp(float(f), k, d2)[1] for f in F[0]]))
    return out


# ----------------------------------------------------------------------- stats.hip in Python doubles
def betacf_double(a, b, x):
    """betacf of stats.hip: (h, iterations)."""
    tiny, eps = 1e-300, 1e-16
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for m in range(1, 501):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + aa / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < eps:
            break
    return h, m


def _exp(v):
    return math.exp(v) if v > -745.2 else 0.0


def incbet_double(a, b, x, swap=False):
    """incbet of stats.hip: (value, iterations); swap: the two branches exchanged (a slip the tail test must notice)."""
    if not x > 0.0:
        return 0.0, 0
    if x >= 1.0:
        return 1.0, 0
    lbeta = math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)
    front = _exp(a * math.log(x) + b * math.log1p(-x) - lbeta)
    if (x < (a + 1.0) / (a + b + 2.0)) != swap:
        h, it = betacf_double(a, b, x)
        return front * h / a, it
    h, it = betacf_double(b, a, 1.0 - x)
    return 1.0 - front * h / b, it


def f_sf_double(f, d1, d2, swap=False, inf_line=True):
    """f_sf of stats.hip: (value, iterations)."""
    if not d2 > 0.0 or f != f:
        return NAN, 0
    if f <= 0.0:
        return 1.0, 0
    if inf_line and f == math.inf:
        return 0.0, 0
    with np.errstate(all='ignore'):
        x = float(np.float64(d2) / (np.float64(d2) + np.float64(d1) * np.float64(f)))
    return incbet_double(0.5 * d2, 0.5 * d1, x, swap)


MUTANTS = ('gemm_j', 'proj_i', 'fit_k', 'no_inf', 'swap', 'min_le')


def model(M, Y, U, ks, r, mutant=None):
    """The five kernels of stats.hip in numpy and f_sf_double -> (kidx, p, r2).  mutant names one slip:
    gemm_j  k_cond_gemm guards the sample axis with j + 1 < N     proj_i  k_gt_project guards it with i + 1 < N
    fit_k   k_gt_ftest sums j <= k squared projections (the row behind beta2 is ssered)
    no_inf  f_sf without its f == inf line                        swap    incbet's branches exchanged
    min_le  k_gt_min takes v <= pb (the last of equal p)"""
    assert mutant is None or mutant in MUTANTS
    N, P = Y.shape
    ks = [int(k) for k in ks]
    kmax = max(ks)
    with np.errstate(all='ignore'):
        n = N - 1 if mutant == 'gemm_j' else N
        Z = M[:, :n].dot(Y[:n])
        mean = Z.sum(axis=0) / N
        sd = np.sqrt(((Z - mean) ** 2).sum(axis=0) / (N - 1))
        Zc = Z / sd
        n = N - 1 if mutant == 'proj_i' else N
        red = (Zc[:n] ** 2).sum(axis=0)
        beta2 = np.vstack([U[:n, :kmax].T.dot(Zc[:n]) ** 2, red[None, :]])
        pk, r2k = np.empty((len(ks), P)), np.empty((len(ks), P))
        for a, k in enumerate(ks):
            fit = beta2[:k + 1 if mutant == 'fit_k' else k].sum(axis=0)
            sse = red - fit
            f = ((red - sse) / k) / (sse / N)
            r2k[a] = 1.0 - sse / red
            pk[a] = [f_sf_double(float(v), float(k), N - (1.0 + r + k), swap=mutant == 'swap',
                                 inf_line=mutant != 'no_inf')[0] for v in f]
    kidx, p, r2 = np.full(P, -1, dtype=np.int32), np.full(P, NAN), np.full(P, NAN)
    for c in range(P):
        for a in range(len(ks)):
            v = pk[a, c]
            if v == v and (kidx[c] < 0 or (v <= p[c] if mutant == 'min_le' else v < p[c])):
                kidx[c], p[c], r2[c] = a, v, r2k[a, c]
    return kidx, p, r2


def same(a, b):
    """array_equal with NaN equal to NaN."""
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ----------------------------------------------------------------------- the edges of section (b)
def edge_case(N=67, P=70, r=0, spots=None):
    """Ordinary exact columns with eight special ones at positions 0, 15, 16, P - 1 and their neighbours' gaps:
    dict(Y, M, U, Z, kinds) for a signed permutation U whose first K1 columns see the whole of the 'inside' column and
    whose first 2 K1 columns see nothing of the 'outside' one.  Z keeps NaN / inf / the constant as they are:
    reference() turns them into (-1, nan, nan)."""
    sp = exact_vector(N, 'sparse')
    supp = np.flatnonzero(sp)
    K1 = len(supp)
    assert 2 * K1 + K1 <= N - 1
    other = [i for i in range(N) if i not in set(supp)]
    U = perm_u(N, first=list(supp) + other[:K1])
    outside = np.zeros(N, dtype=np.int64)
    outside[other[K1:2 * K1]] = sp[supp]
    check_exact(outside)
    c = columns(N, P)
    Z, Y, scale = c['Z'], c['Y'], c['scale']
    special = dict(inside=sp.astype(float), outside=outside.astype(float), constant=np.full(N, 3.0),
                   zero=np.zeros(N), nan=Z[:, 2].copy(), inf=Z[:, 3].copy(), neginf=Z[:, 4].copy())
    special['nan'][N // 2] = NAN
    special['inf'][N - 1] = math.inf
    special['neginf'][0] = -math.inf
    spots = spots or {0: 'nan', 15: 'inside', 16: 'constant', P - 1: 'inf', 1: 'outside', 17: 'zero', 14: 'neginf',
                      P - 2: 'inside', 31: 'outside', 32: 'nan'}
    for p, name in spots.items():
        Z[:, p] = special[name]
        Y[:, p] = special[name] * scale[p]
    return dict(N=N, Y=Y, M=c['M'], U=U, Z=Z, K1=K1, r=r, spots=spots)
