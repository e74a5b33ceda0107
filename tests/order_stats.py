"""Inputs for the exact order statistics on the device (plain numpy, importable without a GPU).

Three places in csrc select a median by an eight-pass radix select over the order-preserving 64-bit key of a double:
rows.hip (k_digit_hist2 + k_auto_pick: the walk's stop rule, cna_stat_median, cna_stat_qc), walk.hip (stat_select over
k_digit_hist, CNA_MEDIAN_HOST=1) and strata.hip (k_st_hist + k_st_pick, every bin of cna_coef_strata at once).  Such a
select is right or wrong by bit pattern, so the vectors here are built from integer keys: which digit pass parts the two
middle elements, which digit the middle element has at a pass, and so on, hold exactly and are asserted on the keys
(tests/test_order_stats_host.py).  `radix_median` restates the select in numpy and can be given one deliberate mistake
at a time: a list of cases that such a wrong select passes would pin nothing.

The reference everywhere is np.median under np.errstate(all='ignore'); `same` is the equality used: both NaN, or equal
as floats (a zero may carry either sign: numpy's partition does not order -0.0 before +0.0)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U = np.uint64
TOP = U(0x8000000000000000)
ALL = U(0xffffffffffffffff)
KEY_MIN = U(0x0010000000000000)               # -DBL_MAX
KEY_MAX = U(0xffefffffffffffff)               # +DBL_MAX
KEY_NEG_ZERO, KEY_POS_ZERO = U(0x7fffffffffffffff), U(0x8000000000000000)

# counts: one element, the smallest even and odd ones, one value per thread of a workgroup and one more or less, the
# 1024 values a workgroup is sized for and one more or less (the second workgroup), several workgroups, many
SIZES = [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 70001]
# launch_auto_median asks for ceil(n / 1024) workgroups and caps them at 1024: the smallest count that asks for 1025
N_CAP = 1024 * 1024 + 1
QC_SIZES = [257, 1025, 70001]
DIGITS = (0, 1, 254, 255)                      # the issue's 0 and 255, and their neighbours (an off-by-one at either end)


def st_chunk():
    """ST_CHUNK of csrc/strata.hip: the values of one bin that one workgroup of k_st_hist counts."""
    src = open(os.path.join(ROOT, 'cna_amd', 'csrc', 'strata.hip')).read()
    return int(re.search(r'constexpr int64_t ST_CHUNK = (\d+);', src).group(1))


def strata_lengths():
    """Segment lengths for the per-bin select: 1, 2, 3, around one chunk, and three chunks ([.., 511, 512, 513, 1025])."""
    c = st_chunk()
    return [1, 2, 3, c - 1, c, c + 1, 2 * c + 1]


# ------------------------------------------------------------------ keys
def order_key(v):
    """The kernels' order-preserving key: negatives have all bits flipped, the others have the top bit set."""
    b = np.ascontiguousarray(v, dtype=np.float64).view(U)
    return np.where(b >> U(63) != 0, ~b, b | TOP)


def key_value(k):
    """The inverse of order_key."""
    k = np.ascontiguousarray(k, dtype=U)
    return np.where(k >> U(63) != 0, k & ~TOP, ~k).astype(U).view(np.float64)


def key_byte(k, p):
    """Digit of pass p (p = 0: the most significant byte)."""
    return (np.asarray(k, dtype=U) >> U(56 - 8 * p)) & U(255)


def middle_keys(v):
    """Keys of the lower and the upper middle element of a NaN-free vector."""
    k = np.sort(order_key(v))
    return k[(len(k) - 1) // 2], k[len(k) // 2]


def first_split(a, b):
    """The digit pass at which two keys part ways (8: they are equal)."""
    for p in range(8):
        if key_byte(a, p) != key_byte(b, p):
            return p
    return 8


def same(got, want):
    return bool((np.isnan(got) and np.isnan(want)) or got == want)


def np_median(v):
    with np.errstate(all='ignore'):
        return float(np.median(v))


# ------------------------------------------------------------------ the select, restated
FAULTS = ('last_bin_early', 'no_sign_flip', 'shared_prefix', 'rank_not_reduced', 'nan_in_bin0', 'same_rank')


def radix_median(v, fault=None):
    """np.median by the select of the kernels: histogram of the digit among the keys that share the prefix, the first
    bin whose running sum exceeds the rank (the last bin if none does), rank reduced by what lies before that bin; both
    middle elements side by side, NaN counted apart in the first pass.  `fault`: one of FAULTS, or None."""
    assert fault is None or fault in FAULTS
    v = np.ascontiguousarray(v, dtype=np.float64)
    nan = v != v
    if fault == 'no_sign_flip':
        b = v.view(U)
        keys = b ^ TOP                                           # negatives keep their magnitude order
    else:
        keys = order_key(v)
    n_nan = int(nan.sum())
    if fault == 'nan_in_bin0':
        keys = np.where(nan, U(0), keys)
        n_nan = 0
    else:
        keys = keys[~nan]
    tot = len(keys)
    if tot == 0 or n_nan > 0:
        return float('nan')
    rank = [tot // 2 if fault == 'same_rank' else (tot - 1) // 2, tot // 2]
    prefix = [U(0), U(0)]
    last = 254 if fault == 'last_bin_early' else 255
    for p in range(8):
        shift = U(56 - 8 * p)
        for w in range(2):
            if p == 0:
                among = keys
            else:
                among = keys[(keys >> (shift + U(8))) == prefix[0 if fault == 'shared_prefix' else w]]
            h = np.bincount(((among >> shift) & U(255)).astype(np.int64), minlength=256)
            d, before = 0, 0
            while d < last and before + int(h[d]) <= rank[w]:
                before += int(h[d])
                d += 1
            if fault != 'rank_not_reduced':
                rank[w] -= before
            prefix[w] = (prefix[w] << U(8)) | U(d)
    lo, hi = (float(key_value(np.array([q], dtype=U))[0]) for q in prefix)
    with np.errstate(all='ignore'):
        return lo if tot & 1 else float((np.float64(lo) + np.float64(hi)) / np.float64(2.0))


# ------------------------------------------------------------------ builders
def _rand_u64(rs, n):
    return (rs.randint(0, 2 ** 32, n).astype(U) << U(32)) | rs.randint(0, 2 ** 32, n).astype(U)


def _spread(rs, m):
    """m offsets >= 0 whose magnitudes are spread over all 64 bit lengths (so that the neighbours of a key share its
    prefix to every depth), a few of them zero."""
    return _rand_u64(rs, m) >> rs.randint(0, 65, m).clip(0, 63).astype(U) if m else np.zeros(0, dtype=U)


def _around(rs, n, kl, ku):
    """n finite values whose lower middle key is kl and whose upper middle key is ku (for odd n: kl is the middle)."""
    kl, ku = U(kl), U(ku)
    assert KEY_MIN <= kl <= ku <= KEY_MAX
    n_lo = (n - 1) // 2
    n_mid = 1 if n & 1 else 2
    n_hi = n - n_lo - n_mid
    below = kl - np.minimum(_spread(rs, n_lo), kl - KEY_MIN)
    above = ku + np.minimum(_spread(rs, n_hi), KEY_MAX - ku)
    k = np.concatenate([below, [kl] if n & 1 else [kl, ku], above]).astype(U)
    return key_value(k[rs.permutation(n)])


def _with_byte(k, p, d):
    s = U(56 - 8 * p)
    return (U(k) & ~(U(255) << s)) | (U(d) << s)


def _base_key(rs):
    """A key whose top byte lies in [1, 254]: every lower byte is then free (finite either way)."""
    return _with_byte(_rand_u64(rs, 1)[0], 0, rs.randint(1, 255))


def split_at(p, n, rs, kind=None):
    """n even: the keys of the two middle elements agree above byte p and differ in byte p.  p = 0 comes as 'sign' (the
    lower one negative, the upper one positive) and as 'exp' (one sign, two exponents)."""
    if n < 2 or n & 1:
        raise ValueError('split_at needs an even count')
    if p == 0:
        if kind == 'sign':
            a, b = rs.randint(1, 128), rs.randint(128, 255)
        else:
            lo = 128 if rs.randint(2) else 1
            a, b = sorted(rs.choice(np.arange(lo, lo + 127), 2, replace=False))
    else:
        a, b = sorted(rs.choice(256, 2, replace=False))
    kl = _with_byte(_base_key(rs) if p else _rand_u64(rs, 1)[0], p, a)
    low = (ALL >> U(8 * p + 8)) if p < 7 else U(0)               # the bytes below p are free in the upper key
    ku = (_with_byte(kl, p, b) & ~low) | (_rand_u64(rs, 1)[0] & low)
    return _around(rs, n, kl, ku)


def digit(p, d, n, rs):
    """The key of the middle element (of both, n even) has byte p equal to d.  Byte 0 = 255: a positive value of at
    least 2^1009; byte 0 = 0: a finite negative value near -DBL_MAX."""
    k = _rand_u64(rs, 1)[0]
    if p == 0:
        if d == 0:
            k = _with_byte(k, 1, rs.randint(0x10, 0x100))        # (below that: -inf and the negative NaNs)
        if d == 255:
            k = _with_byte(k, 1, rs.randint(0x00, 0xf0))         # (above that: +inf and the positive NaNs)
    else:
        k = _with_byte(k, 0, rs.randint(1, 255))
    kl = _with_byte(k, p, d)
    low = (ALL >> U(8 * max(p, 1) + 8)) if p < 7 else U(0)     # (p = 0: byte 1 stays as chosen above)
    ku = kl | (_rand_u64(rs, 1)[0] & low)
    return _around(rs, n, kl, ku)


def zeros(n, rs):
    """-0.0 and +0.0 mixed: nearly half of each."""
    v = np.where(rs.rand(n) < 0.5, -0.0, 0.0)
    if n >= 2:
        v[0], v[-1] = 0.0, -0.0
    return v


def denormals(n, rs):
    """+-5e-324 ... +-1e-310 around zero, a few zeros of either sign among them."""
    mag = (_rand_u64(rs, n) >> rs.randint(20, 64, n).astype(U)).clip(0, 20240000000000)      # 2.024e13 * 4.94e-324 = 1e-310
    return np.where(rs.rand(n) < 0.5, mag | TOP, mag).astype(U).view(np.float64)


def all_equal(n, rs):
    return np.full(n, key_value(np.array([_base_key(rs)]))[0])


def two_values(n, rs, share=0.5):
    """Two distinct values: an even split (n even: the median is the mean of two different values) or 60/40."""
    a, b = np.sort(key_value(np.array([_base_key(rs), _base_key(rs) ^ U(1 << 40)])))
    n_a = n // 2 if share == 0.5 else min(int(np.ceil(share * n)), max(n - 1, 1))
    v = np.concatenate([np.full(n_a, a), np.full(n - n_a, b)])
    return v[rs.permutation(n)]


def adjacent(n, rs):
    """x and the double after it, interleaved."""
    x = key_value(np.array([_base_key(rs)]))[0]
    v = np.full(n, x)
    v[1::2] = np.nextafter(x, np.inf)
    return v


def random_bits(n, rs):
    """Uniform 64-bit patterns, NaNs removed."""
    v = _rand_u64(rs, n).view(np.float64)
    while (v != v).any():
        bad = v != v
        v[bad] = _rand_u64(rs, int(bad.sum())).view(np.float64)
    return v


def infinities(n, rs, half=True):
    """Half -inf and half +inf (n even: the median is NaN, as numpy's is), or a minority of infinities among others."""
    if half:
        v = np.concatenate([np.full(n // 2, -np.inf), np.full(n - n // 2, np.inf)])
        return v[rs.permutation(n)]
    v = kurtosis_like(n, rs)
    r = rs.rand(n)
    v[r < 0.1] = -np.inf
    v[r > 0.85] = np.inf
    return v


def huge(n, rs):
    """+-1.7e308 and +-DBL_MAX, seven in ten positive: the sum of the two middle values overflows."""
    v = np.where(rs.rand(n) < 0.5, 1.7e308, np.finfo(np.float64).max)
    v[rs.permutation(n)[:(3 * n) // 10]] *= -1.0
    return v


def kurtosis_like(n, rs):
    """The band the kurtosis kernels produce: about [-2, 10], many near the low end."""
    return rs.gamma(2.0, 1.2, n) - 1.9


def with_nan(n, rs, where):
    v = kurtosis_like(n, rs)
    if where == 'all':
        v[:] = np.nan
    else:
        v[{'first': 0, 'last': n - 1, 'middle': n // 2}[where]] = np.nan
    return v


def cases(n, seed=0):
    """[(name, vector of n float64)]: every named case that exists at this count (the splits need an even one)."""
    out = []

    def add(name, fn, *a, **kw):
        out.append((name, fn(*a, n, np.random.RandomState([seed, n, len(out)]), **kw)))
    if n >= 2 and n % 2 == 0:
        add('split_at(0) sign', split_at, 0, kind='sign')
        add('split_at(0) exp', split_at, 0, kind='exp')
        for p in range(1, 8):
            add('split_at(%d)' % p, split_at, p)
    for p in range(8):
        for d in DIGITS:
            add('digit(%d, %d)' % (p, d), digit, p, d)
    add('zeros', zeros)
    add('denormals', denormals)
    add('all_equal', all_equal)
    add('two_values even', two_values)
    add('two_values 60/40', two_values, share=0.6)
    add('adjacent', adjacent)
    add('random_bits', random_bits)
    add('infinities half', infinities)
    add('infinities minority', infinities, half=False)
    add('huge', huge)
    add('nan_first', with_nan, where='first')
    add('nan_last', with_nan, where='last')
    add('nan_middle', with_nan, where='middle')
    add('all_nan', with_nan, where='all')
    add('kurtosis_like', kurtosis_like)
    return out


def finite_cases(n, seed=0):
    """The cases cna_coef_strata keeps whole: every value finite."""
    return [(name, v) for name, v in cases(n, seed) if np.isfinite(v).all()]


# ------------------------------------------------------------------ the QC count
def py_threshold(med):
    return max(6, 2 * med)                     # _nam.py:94 with Python's max: a NaN median leaves 6


def qc_expected(v):
    """(median, threshold, cells failing `kurtosis < threshold`) as _nam.py:94-96 forms them."""
    med = np_median(v)
    thr = py_threshold(med)
    return med, float(thr), int(np.count_nonzero(~(v < thr)))


def _qc_vector(rs, n, mid, low, pool):
    """n values with median `mid` exactly: (n - 1) // 2 draws of low() below it, one or two copies of it, and the values
    of `pool` (all >= mid) in turn above it."""
    n_lo = (n - 1) // 2
    n_mid = 1 if n & 1 else 2
    n_hi = n - n_lo - n_mid
    pool = np.asarray(pool, dtype=np.float64)
    assert (pool >= mid).all()
    below = low(n_lo)
    assert (below <= mid).all()
    v = np.concatenate([below, np.full(n_mid, mid), pool[np.arange(n_hi) % len(pool)]])
    return v[rs.permutation(n)]


def qc_cases(n, seed=0):
    """[(name, vector)] for cna_stat_qc: the threshold equals entries of the vector (the comparison is strict), lies
    one double beside others, the median is NaN, or nobody fails."""
    rs = np.random.RandomState([seed, n, 77])
    six = 6.0
    beside6 = [np.nextafter(six, 0.0), six, np.nextafter(six, 7.0)]
    out = []
    out.append(('median below 3, entries 6.0',
                _qc_vector(rs, n, 2.25, lambda m: rs.uniform(-1.5, 2.25, m), [2.5, 4.0] + beside6 + [8.0, np.inf])))
    out.append(('median exactly 3',
                _qc_vector(rs, n, 3.0, lambda m: rs.uniform(-1.5, 3.0, m), [3.0, 5.0] + beside6 + [6.5])))
    mid = 3.7
    two = 2.0 * mid
    out.append(('median above 3, entries 2 median',
                _qc_vector(rs, n, mid, lambda m: rs.uniform(-1.5, 3.7, m),
                           [mid, six, 7.0, np.nextafter(two, 0.0), two, np.nextafter(two, 8.0), 11.0])))
    v = _qc_vector(rs, n, 2.0, lambda m: rs.uniform(-1.5, 2.0, m), [2.5] + beside6 + [9.0])
    v[rs.permutation(n)[:max(1, n // 50)]] = np.nan
    out.append(('NaN median', v))
    out.append(('nobody fails', _qc_vector(rs, n, 1.0, lambda m: rs.uniform(-1.9, 1.0, m), [1.0, 3.0, np.nextafter(six, 0.0)])))
    return out


# ------------------------------------------------------------------ the per-bin select
def strata_layout(segments, rs, left_out=0.1):
    """(v, codes, n_bins) for cna_coef_strata: segment b (a vector, possibly empty) is bin b; the cells of all bins
    shuffled together, and further cells coded -1 (a tenth as many, at least three) with arbitrary values."""
    n_bins = len(segments)
    v = np.concatenate([np.asarray(s, dtype=np.float64) for s in segments])
    codes = np.concatenate([np.full(len(s), b, dtype=np.int32) for b, s in enumerate(segments)])
    extra = max(3, int(left_out * len(v)))
    v = np.concatenate([v, random_bits(extra, rs)])
    codes = np.concatenate([codes, np.full(extra, -1, dtype=np.int32)])
    order = rs.permutation(len(v))
    return v[order], codes[order], n_bins


def strata_expected(v, codes, n_bins):
    """n_kept, min, median, max per bin as numpy forms them over the finite values of the bin (NaN for an empty one)."""
    n_kept = np.zeros(n_bins, dtype=np.int64)
    mn, med, mx = (np.full(n_bins, np.nan) for _ in range(3))
    order = np.argsort(codes, kind='stable')
    sc, sv = codes[order], v[order]
    lo = np.searchsorted(sc, np.arange(n_bins), side='left')
    hi = np.searchsorted(sc, np.arange(n_bins), side='right')
    for b in range(n_bins):
        x = sv[lo[b]:hi[b]]
        x = x[np.isfinite(x)]
        n_kept[b] = len(x)
        if len(x):
            mn[b], med[b], mx[b] = x.min(), np_median(x), x.max()
    return dict(n_kept=n_kept, min=mn, median=med, max=mx)
