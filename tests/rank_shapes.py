"""Inputs for the kernels of csrc/rank_sort.h at the cell, gene and list counts they branch on (the builders; the proofs are
in tests/test_rank_shapes_host.py, the device runs in tests/test_gpu_rank_shapes.py).

The rank entries -- cna_gene_ranksum_by, _pairs, _within, cna_gene_rank_corr, _by, _x, _wide and cna_x_columns -- share one
segmented radix sort and two walks over a sorted list.  Their own tests run on 3001 cells by 9 genes; these inputs are
small and sit on the edges of the units that code counts in: RS_TILE genes and cells of the dense transposition, RS_UNIT
entries of a walk, one sort chunk, a list shorter than what is stored of it.  Every value is a small integer or a half, so
float32 and float64 hold the same numbers; the restatements and the constants are those of the entries' own host files."""
import collections
import functools
import re

import numpy as np

from test_gene_markers_host import ranksum_constant, ranksum_source, ranksum_tiles, restated_ranksum, sparse_of
from test_gene_markers_pairs_host import restated_pairs
from test_gene_markers_within_host import restated_within, weight_tables
from test_gene_rank_corr_host import rank_corr_tiles, restated_rank_corr
from test_gene_rank_corr_strata_host import restated_rank_corr_by
from test_gene_rank_perm_host import restated_columns

UNIT = ranksum_constant('RS_UNIT')
TILE = ranksum_constant('RS_TILE')
DENSE_CHUNK = ranksum_constant('RS_DENSE_CHUNK')
BIG = ranksum_constant('RP_BIG')


def chunk_floor():
    """the least length of a sort chunk of the stored lists: build_chunks of csrc/genes.hip"""
    m = re.search(r'len = std::max<int64_t>\((\d+), std::min<int64_t>\(\d+, len\)\);', ranksum_source('genes.hip'))
    assert m
    return int(m.group(1))


ENTRIES = ['ranksum_by', 'ranksum_pairs', 'ranksum_within', 'rank_corr', 'rank_corr_by', 'rank_corr_wide']
PAYLOAD_BYTES = {'ranksum_by': 2, 'ranksum_pairs': 2, 'ranksum_within': 4, 'rank_corr': 4, 'rank_corr_by': 4, 'rank_corr_wide': 4}
LEVELS, BLOCKS = 3, 2
PAIRS = [(a, b) for a in range(LEVELS) for b in range(LEVELS) if a != b]
Q, Q_WIDE = 2, 17
PRIME = 2053            # above every cell count here: i -> i c mod PRIME is one to one on the cells

AXIS_CELLS = 2 * TILE + 2
AXIS_GENES = [TILE, TILE + 1, 2 * TILE + 2]
AXIS_LEFT = [TILE - 1, TILE, 2 * TILE + 1]
AXIS_FORMS = ['dense-f32', 'dense-f64']
AXIS_TILE_GENES = 70
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 2049]
LENGTH_FORMS = ['dense-f32', 'csr-f32', 'csc-f64']
KEPT_CELLS, KEPT_LEFT_STORED = 600, 5
KEPT_COUNTS = [0, 1, 255, 256, 257, 512]
X_CELLS = [1, 255, 256, 257, 1025]
X_SAMPLES = 3

Case = collections.namedtuple('Case', 'name form V S codes blocks keys wide')


def bytes_per_entry(entry, f64):
    """ranksum_sorted: 2 * (sizeof key + sizeof payload), the keys, the payloads and their copies"""
    return 2 * ((8 if f64 else 4) + PAYLOAD_BYTES[entry])


ONE_GENE_BUDGET = 1     # work_bytes below one entry's: a tile takes one gene (or one key column) at least, and here no more


def axis_budgets(entry, f64):
    """work_bytes: the default; AXIS_TILE_GENES genes' entries; one byte, so that every gene is a tile of its own"""
    return [0, AXIS_TILE_GENES * AXIS_CELLS * bytes_per_entry(entry, f64), ONE_GENE_BUDGET]


def tiles_of(case, entry, work_bytes):
    """the tiles [g0, g1) of genes the entry cuts the case into: the entries' own host files restate the rule"""
    X = upload_of(case)
    if PAYLOAD_BYTES[entry] == 2:
        return ranksum_tiles(case.form, work_bytes, X)[0]
    return rank_corr_tiles(case.form, work_bytes, X)[0]


# ------------------------------------------------------------------ what the builders share
def shape_keys(n, q, left=()):
    """float64 [q, n]: row 0 without ties, row 1 in runs of 3, row 3 of -1, -0.0, +0.0 and 1, the rows behind them with few
    values (odd rows) or many (even rows); NaN in the cells of `left`"""
    i = np.arange(n, dtype=np.int64)
    K = np.empty((q, n))
    for k in range(q):
        spread = i * (3 * k + 5) % PRIME
        if k == 0:
            K[k] = i * 101 % PRIME
        elif k == 1:
            K[k] = (i // 3) * 29 % PRIME
        elif k == 3:
            K[k] = np.array([-1.0, -0.0, 0.0, 1.0])[i * 7 % PRIME % 4]
        elif k % 2:
            K[k] = spread % (k + 1) - 2.0
        else:
            K[k] = spread // (1 + 7 * (k % 5))
    K[:, list(left)] = np.nan
    return K


def _frozen(case):
    for a in case[2:]:
        a.setflags(write=False)
    return case


def upload_of(case):
    """what the engine is given: the dense array of the form's type, or the stored entries as CSR / CSC"""
    if case.form == 'csr-f32':
        return sparse_of(case.V, case.S, 'csr', np.float32, np.int32)
    if case.form == 'csc-f64':
        return sparse_of(case.V, case.S, 'csc', np.float64, np.int64)
    return np.ascontiguousarray(case.V.astype(np.float32 if case.form.endswith('f32') else np.float64))


def typed_values(case):
    return case.V.astype(np.float32 if case.form.endswith('f32') else np.float64)


# ------------------------------------------------------------------ a: the dense form's gene axis
def axis_nan_cells(G):
    """{gene: kept cell that holds its NaN}: the last gene of the first 64-block, the first of the second, the last gene"""
    at = {TILE - 1: 10, TILE: 70}
    at[G - 1] = 128
    return {g: c for g, c in at.items() if g < G}


@functools.lru_cache(maxsize=None)
def gene_axis_case(form, G):
    """130 cells by G genes, dense.  V[i, g] = ((i (g + 3) + 5 g) mod 137) mod 11 - 3: eleven small integers, so ties in every
    gene (i -> i (g + 3) mod 137 is one to one: every gene is another scrambling of the cells), and no two genes alike in
    what cna_gene_ranksum_by returns (the host file proves it).  The cells 63, 64 and 129 are left out, by their code and by
    a NaN in every key; level (i + i // 5) mod 3, block (i // 3) mod 2."""
    assert form in AXIS_FORMS and G in AXIS_GENES
    n = AXIS_CELLS
    i, g = np.arange(n, dtype=np.int64)[:, None], np.arange(G, dtype=np.int64)[None, :]
    V = ((i * (g + 3) + 5 * g) % 137 % 11 - 3).astype(np.float64)
    for gene, cell in axis_nan_cells(G).items():
        V[cell, gene] = np.nan
    i = i.ravel()
    codes = ((i + i // 5) % LEVELS).astype(np.int32)
    codes[AXIS_LEFT] = -1
    blocks = (i // 3 % BLOCKS).astype(np.int32)
    return _frozen(Case('axis G=%d' % G, form, V, np.ones(V.shape, dtype=bool), codes, blocks, shape_keys(n, Q, AXIS_LEFT),
                        shape_keys(n, Q_WIDE, AXIS_LEFT)))


# ------------------------------------------------------------------ b: the lengths
@functools.lru_cache(maxsize=None)
def length_case(n, form):
    """n cells, all kept, six genes:
      0  every cell stored, all values distinct, negative and positive halves
      1  every cell stored, one constant
      2  every cell stored, -1.0 in the first n // 2 positions of the sorted list and 4.0 behind them
      3  every cell stored: a third negative, a third zeros (+0.0 and -0.0), a third positive, with ties
      4  every second cell stored, negatives and positives: the others are implicit zeros of the gene-major forms
      5  nothing stored
    Key 0 is an increasing transform of gene 0 (no ties), key 1 runs of 3; level i mod 3, block i mod 2."""
    assert form in LENGTH_FORMS
    i = np.arange(n, dtype=np.int64)
    order = i * 37 % PRIME                               # distinct: the cells in a fixed scrambled order
    place = np.argsort(np.argsort(order))                # the position of every cell in that order
    V = np.zeros((n, 6))
    S = np.zeros((n, 6), dtype=bool)
    V[:, 0] = order * 0.5 - 300.25
    V[:, 1] = 2.5
    V[:, 2] = np.where(place < n // 2, -1.0, 4.0)
    third, step = place % 3, place // 3
    V[:, 3] = np.where(third == 0, -1.0 - step % 5, np.where(third == 1, np.where(step % 2, -0.0, 0.0), 1.0 + step % 4))
    S[:, :4] = True
    half = i % 2 == 0
    small = (i // 2 * 13 % 7 - 3).astype(np.float64)
    V[half, 4] = np.where(small == 0, 5.0, small)[half]
    S[half, 4] = True
    keys = shape_keys(n, Q)
    keys[0] = 2.0 * V[:, 0] + 1.0
    wide = shape_keys(n, Q_WIDE)
    wide[0] = keys[0]
    return _frozen(Case('n=%d' % n, form, V, S, (i % LEVELS).astype(np.int32), (i % BLOCKS).astype(np.int32), keys, wide))


def dense_chunks(n):
    """chunks of a segment of n entries in a table of the dense form's shape (dense_table)"""
    return -(-n // DENSE_CHUNK)


# ------------------------------------------------------------------ c: the kept entries against the stored ones
def kept_left():
    """the 40 cells of the 600 that are left out"""
    return np.flatnonzero(np.arange(KEPT_CELLS) % 15 == 7)


@functools.lru_cache(maxsize=None)
def kept_case(k):
    """CSR float32, 600 cells, 40 of them left out.  Gene 0 stores k entries in kept cells and 5 in left-out ones: in its
    sorted list the k kept entries lie in front of the 5 whose key is all ones.  The kept values are the distinct integers
    j - k // 2 but for the last min(k, 3), which share the largest: a tie run that ends at position k - 1.  The left-out
    entries hold that largest value, values beyond it and one below all.  Gene 1 stores every cell, gene 2 none."""
    n = KEPT_CELLS
    i = np.arange(n, dtype=np.int64)
    left = kept_left()
    kept = np.setdiff1d(i, left)
    assert k <= len(kept) - 40
    V = np.zeros((n, 3))
    S = np.zeros((n, 3), dtype=bool)
    cells = kept[np.argsort(kept * 37 % PRIME)][:k]
    vals = np.arange(k, dtype=np.float64) - k // 2
    vals[max(0, k - 3):] = vals[-1] if k else 0.0
    V[cells, 0] = vals
    S[cells, 0] = True
    top = float(vals[-1]) if k else 0.0
    V[left[:KEPT_LEFT_STORED], 0] = [top, top + 1.0, top + 2.0, top, -1000.0]
    S[left[:KEPT_LEFT_STORED], 0] = True
    V[:, 1] = (i * 11 % 17) - 8.0
    S[:, 1] = True
    codes = (i % LEVELS).astype(np.int32)
    codes[left] = -1
    return _frozen(Case('k=%d' % k, 'csr-f32', V, S, codes, (i % BLOCKS).astype(np.int32), shape_keys(n, Q, left),
                        shape_keys(n, Q_WIDE, left)))


# ------------------------------------------------------------------ d: the columns formed from X
XCase = collections.namedtuple('XCase', 'case X xrow Z')


@functools.lru_cache(maxsize=None)
def x_case(n):
    """length_case(n, 'csr-f32') with X of 3 samples (the row stride of the device's X is not 3), small integers; xrow names
    the rows of X in a scrambled order and leaves out every seventh cell; Z of 17 rows: a full group and one of one column"""
    i = np.arange(n, dtype=np.int64)
    keep = i % 7 != 6
    rows = int(keep.sum())
    r = np.arange(rows, dtype=np.int64)
    X = np.stack([r * 5 % 7 - 3, r * 3 % 5 - 2, r % 4 - 1], axis=1).astype(np.float64)
    xrow = np.full(n, -1, dtype=np.int64)
    xrow[keep] = np.argsort(r * 41 % PRIME)
    j = np.arange(Q_WIDE, dtype=np.int64)
    Z = np.stack([j % 5 - 2, j * 2 % 3 - 1, 1 + j % 2], axis=1).astype(np.float64)
    for a in (X, xrow, Z):
        a.setflags(write=False)
    return XCase(length_case(n, 'csr-f32'), X, xrow, Z)


def x_columns_of(x):
    """float64 [17, n]: the columns cna_x_columns forms on an x_case, NaN where the cell has no row (integers: exact)"""
    return restated_columns(x.X, x.xrow, x.Z)


# ------------------------------------------------------------------ the references, one per case
def within_weights_of(case):
    return weight_tables(case.codes, LEVELS, case.blocks, BLOCKS, 'any')


def reference(case, entry):
    """the restatement of one entry on a case, as the entry's own GPU test compares it: the rank sums in the engine's shape, the
    correlations as restated_rank_corr / restated_rank_corr_by give them (S in Python integers)"""
    X = typed_values(case)
    if entry == 'ranksum_by':
        return restated_ranksum(X, case.codes, LEVELS)
    if entry == 'ranksum_pairs':
        return restated_pairs(X, case.codes, LEVELS, PAIRS)
    if entry == 'ranksum_within':
        return restated_within(X, case.codes, LEVELS, case.blocks, BLOCKS, *within_weights_of(case))
    if entry == 'rank_corr':
        return restated_rank_corr(X, case.keys)
    if entry == 'rank_corr_by':
        return restated_rank_corr_by(X, case.keys, case.codes, LEVELS)
    assert entry == 'rank_corr_wide'
    return restated_rank_corr(X, case.wide)


def largest_tie_term(case):
    """the largest t^3 - t sum any entry can return on the case: that of one run over all its cells"""
    n = case.V.shape[0]
    return n ** 3 - n
