// Private to expr_rankcorr.hip (cna_gene_rank_corr, cna_gene_rank_corr_by) and expr_rankperm.hip (cna_gene_rank_corr_x,
// cna_gene_rank_corr_x_by, cna_gene_rank_corr_wide): what the two files share of Spearman's rho -- the kept cells of a set
// of columns, the ranks of up to 16 columns as a cell-major table, the shape of one row of that table, and what list of a
// gene a workgroup behind the genes' sort walks (the whole gene, or one level of it).  One statement of
// each: the kernels behind rankcorr_keys (k_rc_vkeys, k_rc_keyrank) stay where it is defined, expr_rankcorr.hip.
#pragma once
#include "rank_sort.h"

constexpr int RC_MAX_KEYS = 16;                // per-cell columns of one table: a cell's row is 64 bytes

// codes[i] = 0 where every column is finite, else -1; *m += their number.  BY (cna_gene_rank_corr_by): codes holds the
// caller's levels, all in [-1, n_bins) with n_bins <= 255; a cell keeps its level where every column is finite, else -1;
// lvl8[i] = that level as a byte, 255 for -1 (the digit of the sort's last pass); m[l] += the kept cells of level l
template <bool BY>
__global__ __launch_bounds__(256) void k_rc_mask(const double* __restrict__ V, int q, int64_t n, int32_t* __restrict__ codes,
                                                 uint8_t* __restrict__ lvl8, unsigned long long* __restrict__ m) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool keep = i < n;
  if constexpr (BY) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    if (i < n) {
      const int32_t cd = codes[i];
      keep = cd >= 0;
      for (int k = 0; k < q; ++k) keep = keep && finite_d(V[(int64_t)k * n + i]);
      codes[i] = keep ? cd : -1;
      lvl8[i] = keep ? (uint8_t)cd : (uint8_t)255;
      if (keep) atomicAdd(&h[cd & 255], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&m[threadIdx.x], (unsigned long long)h[threadIdx.x]);
  } else {
    if (i < n) {
      for (int k = 0; k < q; ++k) keep = keep && finite_d(V[(int64_t)k * n + i]);
      codes[i] = keep ? 0 : -1;
    }
    const unsigned long long bal = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(m, (unsigned long long)__popcll(bal));
  }
}

// one cell's row of btab: W columns (the least of 1, 2, 4, 8, 16 that holds q), one aligned load
template <int W>
struct alignas(4 * W) BRow {
  int32_t v[W];
};

// What a workgroup behind the genes' sort walks (k_rc_corr; k_rp_rank and k_rp_dot of expr_rankperm.hip): where its list
// begins inside the gene's segment (at), its k stored kept entries and the cells they are ranked among.  src(gene, gene's
// index in the tile, level, &at, &k, &cells).  WholeGene: the gene's whole list, level 0 only.  GeneLevel: behind the
// sort's pass on the level, the sub-segment of that level with the level's kept cells; an empty level gives k = 0.
struct WholeGene {
  const unsigned int* kept;
  long long m;
  __device__ __forceinline__ void operator()(int64_t g, int64_t, int, long long* at, long long* k, long long* cells) const {
    *at = 0;
    *k = (long long)kept[g];
    *cells = m;
  }
};
struct GeneLevel {
  const unsigned int* dbase;          // [gene of the tile][digit] of the sort's last pass
  const unsigned long long* mlev;     // kept cells per level
  __device__ __forceinline__ void operator()(int64_t, int64_t in_tile, int level, long long* at, long long* k, long long* cells) const {
    *at = (long long)dbase[in_tile * 256 + level];
    *k = (long long)dbase[in_tile * 256 + level + 1] - *at;
    *cells = (long long)mlev[level];
  }
};

// The ranks of the q <= 16 columns in w->vcol (q x n float64) over the m kept cells of w->sort.code: tiles of whole columns
// within the budget, each a segment of n entries in a table of the dense form's shape; sorted by rs_passes, then one thread
// per kept entry writes b = s + e - m to btab[cell * stride + column] and the tails of the tie runs add to the column's
// tie term, 64 low bits in tie_lo[level * RC_MAX_KEYS + column] and what lies above in tie_hi[the same].  btab and the tie
// terms are the caller's, zeroed by it.  With `lvl8` (cna_gene_rank_corr_by) the passes end on the level and the ranks are
// those inside it.  Defined in expr_rankcorr.hip.
int rankcorr_keys(cna_ctx* c, ExprState* s, RankSumWork* w, int q, int stride, int64_t work_bytes, int64_t m,
                  const uint8_t* lvl8, int32_t* btab, unsigned long long* tie_lo, unsigned int* tie_hi, const char* who);
