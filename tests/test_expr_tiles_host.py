"""The inputs that send cna_expr_to_bins and cna_expr_cross over MORE THAN ONE GENE TILE, and the proof that they do.

Both entries keep the partial sums of the gene-major kernels under PB_PART_BYTES by going over the genes in tiles of whole
genes: at most max_chunks = PB_PART_BYTES / (8 * width) chunks per tile, width = the bins of cna_expr_to_bins or the
samples of cna_expr_cross (csrc/expr.h: gene_tiles, walked by pb_sparse of expr_bins.hip and xc_sparse of expr_cross.hip).
A chunk is a piece of one gene's list (genes.hip: build_chunks):
its length is nnz / 16384, held to [1024, 65536] and rounded up to a multiple of 64.

This file restates those two rules in Python, builds the two inputs the GPU tests use (tests/test_gpu_expr_to_sample.py,
tests/test_gpu_gene_test.py) and asserts, without a device, that each has more chunks than one tile takes and that the
tile boundary falls where the input wants it: behind an empty gene that follows the last gene the first tile has room for.
The constants are read from the source, so a change of PB_PART_BYTES or of the chunk rule makes these assertions fail
instead of leaving the second tile untested."""
import os
import re

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_built = {}


def source_constant(name):
    """An integer constant of the expression side (csrc/genes.hip, expr_bins.hip, expr_cross.hip), written as `123` or as
    `123ll << 20`."""
    src = ''.join(open(os.path.join(ROOT, 'cna_amd', 'csrc', f)).read() for f in ('genes.hip', 'expr_bins.hip', 'expr_cross.hip'))
    m = re.search(r'constexpr (?:int|int64_t) %s = (\d+)(?:ll)?(?: << (\d+))?;' % name, src)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


# ------------------------------------------------------------------ the two rules, restated
def chunk_length(nnz):
    """build_chunks: nnz / (4096 waves * 4), at least 1024, at most 65536, rounded up to whole batches of 64."""
    return (max(1024, min(65536, nnz // 16384)) + 63) // 64 * 64


def chunks_per_gene(M):
    """Chunks of every gene's list of a cells x genes sparse matrix (its stored entries, explicit zeros included)."""
    M = sp.csc_matrix(M)
    length = np.diff(M.indptr).astype(np.int64)
    return -(-length // chunk_length(int(M.nnz)))


def gene_tiles(chunks, max_chunks):
    """pb_sparse / xc_sparse: tiles [g0, g1) of whole genes, as many as keep the tile's chunks <= max_chunks, one gene at
    least."""
    first = np.r_[0, np.cumsum(chunks)]
    tiles, g0, G = [], 0, len(chunks)
    while g0 < G:
        g1 = g0 + 1
        while g1 < G and first[g1 + 1] - first[g0] <= max_chunks:
            g1 += 1
        tiles.append((g0, g1))
        g0 = g1
    return tiles


def max_chunks_for(width):
    return max(1, source_constant('PB_PART_BYTES') // (8 * width))


def assert_two_tiles(M, width, boundary):
    """More chunks than one tile takes; exactly two tiles, the first ending behind gene `boundary - 1`, which is empty and
    follows a gene that is not; the second tile is not empty either."""
    chunks = chunks_per_gene(M)
    limit = max_chunks_for(width)
    assert chunks.sum() > limit, (int(chunks.sum()), limit)
    tiles = gene_tiles(chunks, limit)
    assert tiles == [(0, boundary), (boundary, M.shape[1])], tiles
    assert chunks[boundary - 1] == 0 and chunks[boundary - 2] > 0 and chunks[boundary] > 0
    assert chunks[:boundary].sum() + chunks[boundary] > limit            # the next gene did not fit: the limit made the cut
    assert chunks[boundary:].sum() > 0
    return chunks, limit


# ------------------------------------------------------------------ cna_expr_to_bins: 4096 bins
BINS_N, BINS_G, BINS_BINS = 20 * 1024 + 37, 420, 4096
BINS_EMPTY = (1, 391)              # 390 genes of 21 chunks are 8190 <= 8192 chunks: gene 391 closes the first tile
BINS_BOUNDARY = 392


def bins_tile_case():
    """(M, codes): 20 517 cells x 420 genes float64 CSC with integer values 0..9, every gene stored in EVERY cell (zeros
    too) but the two of BINS_EMPTY; int32 codes over 4096 bins, one bin without cells, a tenth of the cells left out (the
    recipe of test_gpu_expr_to_sample.codes_for)."""
    if 'bins' not in _built:
        rs = np.random.RandomState(41)
        n, g = BINS_N, BINS_G
        full = np.ones(g, dtype=bool)
        full[list(BINS_EMPTY)] = False
        indptr = np.r_[0, np.cumsum(np.where(full, n, 0))].astype(np.int32)
        indices = np.tile(np.arange(n, dtype=np.int32), int(full.sum()))
        data = rs.randint(0, 10, indices.size).astype(np.float64)
        M = sp.csc_matrix((data, indices, indptr), shape=(n, g))
        M.has_sorted_indices = True
        M.has_canonical_format = True
        codes = rs.randint(0, BINS_BINS, n).astype(np.int32)
        codes[codes == BINS_BINS // 2] = 0
        codes[rs.rand(n) < 0.1] = -1
        _built['bins'] = (M, codes)
    return _built['bins']


def assert_bins_tile_case(M):
    chunks, limit = assert_two_tiles(M, BINS_BINS, BINS_BOUNDARY)
    assert limit == 8192 and chunk_length(int(M.nnz)) == 1024 and M.nnz < 16384 * 1024
    assert chunks.sum() == 418 * 21 and set(chunks) == {0, 21}


# ------------------------------------------------------------------ cna_expr_cross: 1024 samples
CROSS_N, CROSS_G, CROSS_NX = 300, 33100, 1024
CROSS_EMPTY = (5, 20000, 32770, 33000)      # genes 0 .. 32769 hold 32768 lists of one chunk: gene 32770 closes the first tile
CROSS_BOUNDARY = 32771


def cross_tile_case():
    """(E, X, xrow): 300 cells x 33 100 genes float64 CSC, 1 to 5 integer entries 1..9 per gene but the empty ones of
    CROSS_EMPTY (cells ascending inside a gene); X 300 x 1024 with integers -3..3; xrow a permutation of the rows of X
    with a tenth of the cells set to -1."""
    if 'cross' not in _built:
        rs = np.random.RandomState(43)
        n, g = CROSS_N, CROSS_G
        count = rs.randint(1, 6, g)
        count[list(CROSS_EMPTY)] = 0
        indptr = np.r_[0, np.cumsum(count)].astype(np.int32)
        gene = np.repeat(np.arange(g), count)
        rank = np.arange(indptr[-1]) - indptr[gene]
        stride, start = rs.randint(1, 50, g), rs.randint(0, n - 4 * 49, g)
        indices = (start[gene] + rank * stride[gene]).astype(np.int32)       # distinct and ascending inside a gene, < n
        data = rs.randint(1, 10, indices.size).astype(np.float64)
        E = sp.csc_matrix((data, indices, indptr), shape=(n, g))
        E.has_sorted_indices = True
        E.has_canonical_format = True
        X = rs.randint(-3, 4, (n, CROSS_NX)).astype(np.float64)
        xrow = rs.permutation(n).astype(np.int64)
        xrow[rs.rand(n) < 0.1] = -1
        _built['cross'] = (E, X, xrow)
    return _built['cross']


def assert_cross_tile_case(E):
    chunks, limit = assert_two_tiles(E, CROSS_NX, CROSS_BOUNDARY)
    assert limit == 32768 and chunk_length(int(E.nnz)) == 1024
    assert set(chunks) == {0, 1} and chunks[:CROSS_BOUNDARY].sum() == limit       # the first tile is full to the last chunk


def cross_reference(E, X, xrow):
    """(W, rho, sx, sxx, m) in float64: exact on integer-valued input whatever the order."""
    keep = xrow >= 0
    EK, XK = sp.csr_matrix(E)[keep], X[xrow[keep]]
    return (np.asarray(EK.T @ XK), XK.sum(axis=0), np.asarray(EK.sum(axis=0)).ravel(),
            np.asarray(EK.multiply(EK).sum(axis=0)).ravel(), int(keep.sum()))


# ------------------------------------------------------------------ the CPU checks
def test_the_rules_restated_here():
    assert chunk_length(0) == 1024 and chunk_length(16384 * 1024 + 16383) == 1024 and chunk_length(16384 * 1025) == 1088
    assert chunk_length(1 << 40) == 65536
    assert gene_tiles(np.array([3, 0, 3, 3, 9, 0, 1]), 6) == [(0, 3), (3, 4), (4, 5), (5, 7)]    # 9 > 6: a tile of its own
    assert gene_tiles(np.array([2, 2]), 4) == [(0, 2)]
    assert source_constant('PB_PART_BYTES') == 256 << 20 and source_constant('PB_DENSE_CHUNK') == 2048
    assert source_constant('XC_MAX_COLS') == CROSS_NX and source_constant('PB_MAX_BINS') == BINS_BINS


def test_the_bins_input_takes_two_gene_tiles():
    M, codes = bins_tile_case()
    assert M.shape == (BINS_N, BINS_G) and M.has_canonical_format and (M.data == 0).any()
    assert_bins_tile_case(M)
    nnz_of = np.diff(M.indptr)
    assert (nnz_of[list(BINS_EMPTY)] == 0).all() and (np.delete(nnz_of, BINS_EMPTY) == BINS_N).all()
    assert codes.min() == -1 and codes.max() == BINS_BINS - 1 and (codes == BINS_BINS // 2).sum() == 0
    assert 0.05 < (codes == -1).mean() < 0.15


def test_the_cross_input_takes_two_gene_tiles():
    E, X, xrow = cross_tile_case()
    assert E.shape == (CROSS_N, CROSS_G) and X.shape == (CROSS_N, CROSS_NX)
    assert_cross_tile_case(E)
    nnz_of = np.diff(E.indptr)
    assert (nnz_of[list(CROSS_EMPTY)] == 0).all() and np.delete(nnz_of, CROSS_EMPTY).min() == 1 and nnz_of.max() == 5
    assert 0 <= E.indices.min() and E.indices.max() < CROSS_N
    S = E.copy()
    S.has_canonical_format = False
    S.has_sorted_indices = False
    S.sum_duplicates()                                                   # what scipy makes of it: nothing changes
    assert S.nnz == E.nnz and np.array_equal(S.indices, E.indices)
    keep = xrow >= 0
    assert 0 < (~keep).sum() < 60 and len(set(xrow[keep])) == keep.sum() and xrow.max() < CROSS_N
    W, rho, sx, sxx, m = cross_reference(E, X, xrow)
    assert W.shape == (CROSS_G, CROSS_NX) and m == keep.sum() and (W[list(CROSS_EMPTY)] == 0).all()
    assert np.array_equal(W[CROSS_BOUNDARY], E[:, CROSS_BOUNDARY].toarray()[keep, 0] @ X[xrow[keep]])
    assert np.abs(W).max() < 2 ** 20 and np.array_equal(W, np.rint(W))   # integers far below 2^53: exact in any order
