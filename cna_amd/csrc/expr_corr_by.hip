// cna_gene_corr_by: per-gene Pearson correlation to per-cell columns inside every level of a clustering, and the pooled
// within-level ("cluster-adjusted") correlation, in one pass over the resident expression matrix (cna.tl.gene_corr_strata).
// The question behind it: cna.tl.coef_strata shows a cluster whose violin (the reference's cna.pl.violinplot,
// plotting/_strat.py:21-29) spans both signs -- which genes separate its expanded cells from its depleted ones?  The global
// line of demo/demo.ipynb ("per-gene correlations to neighborhood coefficient") is dominated by the cluster markers.
//
//   sort (expr.h)      checks every code against [-1, n_bins); the cells sorted by level (CellListOf, expr.h), ascending inside a level
//   k_cb_key_stats     per (key, level): finite count, mean, sum (v - mean), sum (v - mean)^2, min, max over the level's
//                      cell list (fixed-order sums: k_key_stats of expr.h, segmented)
//   k_cb_key_table     cells x Q table of key values centred on the mean of the cell's own (key, level), 0 where the cell is
//                      left out, + one word per cell: the keys that keep it (low 16 bits) and its level
//   k_cb_dense         lane = gene, a workgroup walks a chunk (PB_DENSE_CHUNK cells) of one level's cell list; the cell, its
//                      word and its Q key values are the same in every lane: scalar loads.  One record per (chunk, gene)
//                      with plain stores
//   k_cb_sparse        one wave per chunk of a gene's list, a record per level in LDS, indexed by the level of each entry's
//                      cell; lanes of a batch that meet in a level are served lowest lane first, in rounds (k_pb_sparse's
//                      protocol: an integer LDS atomic names the lane whose turn it is).  One record per (chunk, level)
//   k_cb_finish_*      adds the records of a (level, gene) in chunk order, writes r and folds the levels, ascending, into the
//                      within-level sums; after the last level the within-level correlation
//
// The levels are taken in groups of consecutive levels, one launch per group, the within-level sums carried from group to
// group in 5 x q x genes doubles:
//   dense       as many levels as keep a group's records (chunks x F x genes doubles, F = 4 S + Q <= 80 fields, S = 1 when
//               the keys leave out the same cells, else Q) within the result's own size plus cells / PB_DENSE_CHUNK chunks:
//               partial storage is never more than the result plus F / 1024 (<= 8 %; one key: 0.5 %) of the matrix' own
//               size (f32), plus one record of F x genes doubles for a single level that is cut last
//   gene-major  as many levels as fit 64 KB of LDS (F = 5 S + Q fields of 8 bytes and a turn word per level: 4096 / (2 F + 1)
//               levels); every group is a pass over the lists.  Partial storage: chunks x levels of the group x F doubles,
//               held to PB_PART_BYTES (256 MB) by going over the genes in tiles (gene_tiles; a record is at most 64 KB).
//
// Result sums take a fixed order (no floating-point atomics): two runs on one input give the same bits.  Integer
// atomics only count and hand out turns.
#include "expr.h"
#include <cmath>

namespace {

constexpr int CB_MAXQ = 16;
constexpr int CB_MAX_LEVELS = 1024;
constexpr int CB_MAX_ROWS = 4096;     // q x levels, the row cap of cna_expr_to_bins
using CellList = CellListOf<CB_MAX_LEVELS>;   // the sort's policy (expr.h)
constexpr int CB_LDS_BYTES = 65536;   // what a kernel gets without opting in
// KS_LD (expr.h) doubles per (key, level) in the key statistics: n, mean, sum vc^2, sum vc, min, max
constexpr int WA_LD = 5;   // within-level sums per (key, gene): cov, var x, var v, a level with the gene / the key not constant

// the sort with its codes and the chunks of the levels; the cell list; raw key columns, their table, the cells' words, the
// key statistics; partial records; r; the within-level sums and the within-level correlation; the "masks differ" word
struct CorrByWork : BufSet {
  CodeSort sort{*this};
  Buf list{*this}, vraw{*this}, vtab{*this}, word{*this}, kstat{*this}, part{*this}, rout{*this}, wacc{*this}, wout{*this},
      flag{*this};
};

// ------------------------------------------------------------------ key columns
// one block of 256 threads per (level, key): thread t adds the cells t, t + 256, ... of the level's list; the 256 partial
// sums are folded by a fixed tree -- the same bits on every run
__global__ __launch_bounds__(256) void k_cb_key_stats(const double* __restrict__ V, int64_t n, const int32_t* __restrict__ list,
                                                      const int64_t* __restrict__ bptr, int n_bins, double* __restrict__ ks) {
  __shared__ double sh[4][256];
  const int b = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
  const int64_t lo = bptr[b], hi = bptr[b + 1];
  const double* v = V + (int64_t)j * n;
  double cnt = 0, sum = 0, mn = INFINITY, mx = -INFINITY;
  for (int64_t e = lo + t; e < hi; e += 256) {
    const double x = v[list[e]];
    if (finite_d(x)) {
      cnt += 1.0;
      sum += x;
      mn = fmin(mn, x);
      mx = fmax(mx, x);
    }
  }
  sh[0][t] = cnt; sh[1][t] = sum; sh[2][t] = mn; sh[3][t] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
      sh[2][t] = fmin(sh[2][t], sh[2][t + w]);
      sh[3][t] = fmax(sh[3][t], sh[3][t + w]);
    }
    __syncthreads();
  }
  const double N = sh[0][0], mean = N > 0 ? sh[1][0] / N : 0.0, vmin = sh[2][0], vmax = sh[3][0];
  __syncthreads();
  double s1 = 0, s2 = 0;
  for (int64_t e = lo + t; e < hi; e += 256) {
    const double x = v[list[e]];
    if (finite_d(x)) {
      const double d = x - mean;
      s1 += d;
      s2 += d * d;
    }
  }
  sh[0][t] = s1; sh[1][t] = s2;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    double* o = ks + ((int64_t)j * n_bins + b) * KS_LD;
    o[0] = N; o[1] = mean; o[2] = sh[1][0]; o[3] = sh[0][0]; o[4] = vmin; o[5] = vmax; o[6] = 0; o[7] = 0;
  }
}

// cell-major table: one gather brings all Q centred values of a cell.  word = keys that keep the cell | level << 16, 0 for a
// cell without a level or without a finite key.  flag |= 1 when the keys' masks differ in a cell that has a level.
__global__ __launch_bounds__(256) void k_cb_key_table(const double* __restrict__ V, int64_t n, int q, int Q,
                                                      const int32_t* __restrict__ codes, int n_bins,
                                                      const double* __restrict__ ks, double* __restrict__ tab,
                                                      uint32_t* __restrict__ word, int* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t cd = codes[i];
  uint32_t m = 0;
  for (int j = 0; j < Q; ++j) {
    double vc = 0.0;
    if (j < q && cd >= 0) {
      const double x = V[(int64_t)j * n + i];
      if (finite_d(x)) {
        vc = x - ks[((int64_t)j * n_bins + cd) * KS_LD + 1];
        m |= 1u << j;
      }
    }
    tab[i * Q + j] = vc;
  }
  word[i] = m ? (m | (uint32_t)cd << 16) : 0u;
  if (m != 0 && m != (1u << q) - 1u) atomicOr(flag, 1);
}

// ------------------------------------------------------------------ dense
// Field order of a record (F = 4 S + Q doubles, S = 1 when the keys share one mask, else Q), as in k_gc_dense:
//   [s]: sum x   [S + s]: sum x^2   [2S + s]: min x   [3S + s]: max x   [4S + j]: sum x (v_j - mean_j of the level)
// grid.x = (chunk - ch0) * gene_blocks + gene block; rng[2 ch], rng[2 ch + 1]: the chunk's span of the cell list (never empty)
template <typename T, int Q, bool SHARED>
__global__ __launch_bounds__(256) void k_cb_dense(const T* __restrict__ X, int64_t G, int64_t gene_blocks, int64_t ch0,
                                                  const int32_t* __restrict__ list, const int64_t* __restrict__ rng,
                                                  const double* __restrict__ tab, const uint32_t* __restrict__ word,
                                                  double* __restrict__ part) {
  constexpr int S = SHARED ? 1 : Q;
  constexpr int F = 4 * S + Q;
  constexpr int U = 8;
  const int64_t rec = (int64_t)blockIdx.x / gene_blocks, gb = (int64_t)blockIdx.x % gene_blocks;
  const int64_t g = gb * blockDim.x + threadIdx.x;
  const bool act = g < G;
  const int64_t gl = act ? g : G - 1;          // idle lanes of the last gene block reload its last gene; nothing is stored
  const int64_t lo = rng[2 * (ch0 + rec)], hi = rng[2 * (ch0 + rec) + 1];
  double sx[S], sxx[S], sxv[Q];
  T mn[S], mx[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    sx[s] = 0; sxx[s] = 0;
    mn[s] = (T)INFINITY; mx[s] = (T)-INFINITY;
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) sxv[j] = 0;
  for (int64_t e = lo; e < hi; e += U) {
    T xs[U];
    int64_t cell[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ee = e + u < hi ? e + u : hi - 1;
      cell[u] = list[ee];                       // the same in every lane: a scalar load
      xs[u] = X[cell[u] * G + gl];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e + u >= hi) break;
      const uint32_t m = word[cell[u]];         // wave-uniform: a scalar load and a scalar branch
      if (m == 0) continue;
      const double* v = tab + cell[u] * Q;
      const double x = (double)xs[u];
      if (SHARED) {
        sx[0] += x;
        sxx[0] = fma(x, x, sxx[0]);
        mn[0] = xs[u] < mn[0] ? xs[u] : mn[0];
        mx[0] = xs[u] > mx[0] ? xs[u] : mx[0];
#pragma unroll
        for (int j = 0; j < Q; ++j) sxv[j] = fma(x, v[j], sxv[j]);
      } else {
#pragma unroll
        for (int j = 0; j < Q; ++j) {
          if (m >> j & 1) {
            sx[j] += x;
            sxx[j] = fma(x, x, sxx[j]);
            mn[j] = xs[u] < mn[j] ? xs[u] : mn[j];
            mx[j] = xs[u] > mx[j] ? xs[u] : mx[j];
            sxv[j] = fma(x, v[j], sxv[j]);
          }
        }
      }
    }
  }
  if (!act) return;
  double* o = part + rec * F * G + g;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    o[(int64_t)(s)*G] = sx[s];
    o[(int64_t)(S + s) * G] = sxx[s];
    o[(int64_t)(2 * S + s) * G] = (double)mn[s];
    o[(int64_t)(3 * S + s) * G] = (double)mx[s];
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) o[(int64_t)(4 * S + j) * G] = sxv[j];
}

// ------------------------------------------------------------------ one (key, level, gene) from its sums
// r by the rules of gc_r (expr_corr.hip), and the level's share of the within-level sums.  cnt: entries that were added
// (dense: every kept cell; gene-major lists: the stored ones -- the others are zeros).  Constant genes and keys are decided
// exactly (minimum == maximum): such a level adds exactly 0 to the sums it does not bear on.
__device__ __forceinline__ double cb_level(double sx, double sxx, double mn, double mx, double cnt, double sxv,
                                           const double* __restrict__ ks, double* __restrict__ wa) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double N = ks[0];
  if (N < 2.0) return nan;
  if (cnt < N) {
    mn = fmin(mn, 0.0);
    mx = fmax(mx, 0.0);
  }
  const bool key_live = ks[4] < ks[5], gene_live = !(mn == mx);
  const double mean = sx / N;
  const double varx = sxx - sx * mean;
  const double cov = sxv - mean * ks[3];
  if (gene_live) {
    wa[1] += varx;
    wa[3] = 1.0;
  }
  if (key_live) {
    wa[2] += ks[2];
    wa[4] = 1.0;
  }
  if (!key_live || !gene_live) return nan;
  wa[0] += cov;
  double r = cov / sqrt(varx) / sqrt(ks[2]);
  if (r > 1.0) r = 1.0;
  if (r < -1.0) r = -1.0;
  return r;
}

__device__ __forceinline__ void wa_load(const double* __restrict__ wacc, int64_t at, int64_t stride, double* wa) {
#pragma unroll
  for (int k = 0; k < WA_LD; ++k) wa[k] = wacc[at + k * stride];
}
// the sums go back for the next group of levels; after the last one the pooled correlation
__device__ __forceinline__ void wa_store(double* __restrict__ wacc, int64_t at, int64_t stride, const double* wa, bool last,
                                         double* __restrict__ wout) {
#pragma unroll
  for (int k = 0; k < WA_LD; ++k) wacc[at + k * stride] = wa[k];
  if (!last) return;
  double r = __longlong_as_double(0x7ff8000000000000LL);
  if (wa[3] != 0.0 && wa[4] != 0.0) {
    r = wa[0] / sqrt(wa[1] * wa[2]);
    if (r > 1.0) r = 1.0;
    if (r < -1.0) r = -1.0;
  }
  wout[at] = r;
}

// thread = (key j, gene g): the levels [b0, b1) in order; bfirst: first chunk of every level, ch0 = bfirst[b0]
__global__ __launch_bounds__(256) void k_cb_finish_dense(const double* __restrict__ part, int64_t G, int q, int Q, int S,
                                                         int n_bins, int b0, int b1, const int64_t* __restrict__ bfirst,
                                                         const double* __restrict__ ks, double* __restrict__ out,
                                                         double* __restrict__ wacc, double* __restrict__ wout, int last) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)q * G) return;
  const int j = (int)(t / G);
  const int64_t g = t % G;
  const int F = 4 * S + Q, s = S == 1 ? 0 : j;
  const int64_t ch0 = bfirst[b0];
  double wa[WA_LD];
  wa_load(wacc, t, (int64_t)q * G, wa);
  for (int b = b0; b < b1; ++b) {
    double sx = 0, sxx = 0, mn = INFINITY, mx = -INFINITY, sxv = 0;
    for (int64_t ch = bfirst[b]; ch < bfirst[b + 1]; ++ch) {       // chunk order: the order of the cells
      const double* o = part + (ch - ch0) * F * G + g;
      sx += o[(int64_t)s * G];
      sxx += o[(int64_t)(S + s) * G];
      mn = fmin(mn, o[(int64_t)(2 * S + s) * G]);
      mx = fmax(mx, o[(int64_t)(3 * S + s) * G]);
      sxv += o[(int64_t)(4 * S + j) * G];
    }
    const double* k = ks + ((int64_t)j * n_bins + b) * KS_LD;
    out[((int64_t)j * n_bins + b) * G + g] = cb_level(sx, sxx, mn, mx, k[0], sxv, k, wa);
  }
  wa_store(wacc, t, (int64_t)q * G, wa, last != 0, wout);
}

// ------------------------------------------------------------------ gene-major lists
// One wave per chunk c0 + blockIdx.x of the gene lists; the levels [b0, b0 + nl).  Dynamic LDS: F x nl doubles, field-major
// (F = 5 S + Q: as in the dense kernel, then [4S + s]: entries added, [5S + j]: sum x (v_j - mean_j of the level)) and nl
// turn words; the chunk's record in global memory has the same layout.  A batch is 64 consecutive entries.  Where every
// lane of a batch that takes part names the same level, the wave adds them by its fixed tree and lane 0 adds the totals;
// otherwise rounds: every waiting lane posts stamp * 64 + 63 - lane with an integer atomic max, the lowest waiting lane of
// each level finds its own value there and adds.  Both orders depend on the input alone.
template <typename T, int Q, bool SHARED>
__global__ __launch_bounds__(64) void k_cb_sparse(const int64_t* __restrict__ chunk_lo, const int32_t* __restrict__ chunk_gene,
                                                  const int64_t* __restrict__ gptr, int64_t c0, int64_t chunk_len,
                                                  const int32_t* __restrict__ gcell, const T* __restrict__ gval,
                                                  const double* __restrict__ tab, const uint32_t* __restrict__ word, int b0,
                                                  int nl, double* __restrict__ part) {
  constexpr int S = SHARED ? 1 : Q;
  constexpr int F = 5 * S + Q;
  extern __shared__ double cb_lds[];
  double* acc = cb_lds;
  int* turn = reinterpret_cast<int*>(cb_lds + (int64_t)F * nl);
  const int lane = threadIdx.x;
  const int64_t ch = c0 + blockIdx.x;
  for (int i = lane; i < F * nl; i += 64) {
    const int f = i / nl;
    acc[i] = (f >= 2 * S && f < 3 * S) ? INFINITY : ((f >= 3 * S && f < 4 * S) ? -INFINITY : 0.0);
  }
  for (int b = lane; b < nl; b += 64) turn[b] = 0;
  __syncthreads();
  const int64_t lo = chunk_lo[ch];
  const int64_t end = gptr[chunk_gene[ch] + 1];
  const int64_t hi = lo + chunk_len < end ? lo + chunk_len : end;
  int stamp = 0;
  for (int64_t e0 = lo; e0 < hi; e0 += 64) {
    const int64_t e = e0 + lane;
    int lvl = -1;
    uint32_t m = 0;
    double x = 0.0, v[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) v[j] = 0.0;
    if (e < hi) {
      const int64_t cell = gcell[e];
      const uint32_t w = word[cell];
      const int l = (int)(w >> 16) - b0;
      if ((w & 0xffffu) != 0 && l >= 0 && l < nl) {
        lvl = l;
        m = w & 0xffffu;
        x = (double)gval[e];
        const double* row = tab + cell * Q;
#pragma unroll
        for (int j = 0; j < Q; ++j) v[j] = row[j];
      }
    }
    bool wait = lvl >= 0;
    const unsigned long long in = __ballot(wait);
    if (in == 0) continue;
    const int l0 = __shfl(lvl, __ffsll((long long)in) - 1, 64);
    if (__ballot(wait && lvl != l0) == 0) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const bool on = wait && (SHARED || (m >> s & 1));
        const double a = wave_sum(on ? x : 0.0), b = wave_sum(on ? x * x : 0.0), c1 = wave_min(on ? x : INFINITY),
                     c2 = wave_max(on ? x : -INFINITY), d = wave_sum(on ? 1.0 : 0.0);
        if (lane == 0) {
          acc[s * nl + l0] += a;
          acc[(S + s) * nl + l0] += b;
          acc[(2 * S + s) * nl + l0] = fmin(acc[(2 * S + s) * nl + l0], c1);
          acc[(3 * S + s) * nl + l0] = fmax(acc[(3 * S + s) * nl + l0], c2);
          acc[(4 * S + s) * nl + l0] += d;
        }
      }
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        const double a = wave_sum(wait && (SHARED || (m >> j & 1)) ? x * v[j] : 0.0);
        if (lane == 0) acc[(5 * S + j) * nl + l0] += a;
      }
      __syncthreads();
      continue;
    }
    while (true) {
      ++stamp;
      const int mine = stamp * 64 + 63 - lane;
      if (wait) atomicMax(&turn[lvl], mine);
      __syncthreads();
      if (wait && turn[lvl] == mine) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
          if (SHARED || (m >> s & 1)) {
            acc[s * nl + lvl] += x;
            acc[(S + s) * nl + lvl] = fma(x, x, acc[(S + s) * nl + lvl]);
            acc[(2 * S + s) * nl + lvl] = fmin(acc[(2 * S + s) * nl + lvl], x);
            acc[(3 * S + s) * nl + lvl] = fmax(acc[(3 * S + s) * nl + lvl], x);
            acc[(4 * S + s) * nl + lvl] += 1.0;
          }
        }
#pragma unroll
        for (int j = 0; j < Q; ++j)
          if (SHARED || (m >> j & 1)) acc[(5 * S + j) * nl + lvl] = fma(x, v[j], acc[(5 * S + j) * nl + lvl]);
        wait = false;
      }
      __syncthreads();
      if (__ballot(wait) == 0) break;
    }
  }
  __syncthreads();
  double* o = part + (int64_t)blockIdx.x * F * nl;
  for (int i = lane; i < F * nl; i += 64) o[i] = acc[i];
}

// thread = (key j, gene g of the tile [g0, g1) whose first chunk is c0): the levels [b0, b0 + nl) in order
__global__ __launch_bounds__(256) void k_cb_finish_sparse(const double* __restrict__ part, const int64_t* __restrict__ gchunk,
                                                          int64_t g0, int64_t g1, int64_t c0, int64_t G, int q, int Q, int S,
                                                          int n_bins, int b0, int nl, const double* __restrict__ ks,
                                                          double* __restrict__ out, double* __restrict__ wacc,
                                                          double* __restrict__ wout, int last) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)q * (g1 - g0)) return;
  const int j = (int)(t / (g1 - g0));
  const int64_t g = g0 + t % (g1 - g0);
  const int F = 5 * S + Q, s = S == 1 ? 0 : j;
  const int64_t at = (int64_t)j * G + g;
  double wa[WA_LD];
  wa_load(wacc, at, (int64_t)q * G, wa);
  for (int l = 0; l < nl; ++l) {
    double sx = 0, sxx = 0, mn = INFINITY, mx = -INFINITY, cnt = 0, sxv = 0;
    for (int64_t ch = gchunk[g]; ch < gchunk[g + 1]; ++ch) {       // chunk order: the order of the cells
      const double* o = part + (ch - c0) * F * nl + l;
      sx += o[(int64_t)s * nl];
      sxx += o[(int64_t)(S + s) * nl];
      mn = fmin(mn, o[(int64_t)(2 * S + s) * nl]);
      mx = fmax(mx, o[(int64_t)(3 * S + s) * nl]);
      cnt += o[(int64_t)(4 * S + s) * nl];
      sxv += o[(int64_t)(5 * S + j) * nl];
    }
    const double* k = ks + ((int64_t)j * n_bins + b0 + l) * KS_LD;
    out[((int64_t)j * n_bins + b0 + l) * G + g] = cb_level(sx, sxx, mn, mx, cnt, sxv, k, wa);
  }
  wa_store(wacc, at, (int64_t)q * G, wa, last != 0, wout);
}

// f(T, Q slots, shared masks) for the resident matrix' element type
template <class Fn>
void with_kernel(const ExprState* s, int Q, bool shared, Fn&& f) {
  with_bool(s->is_f64 != 0, [&](auto f64) {
    using T = std::conditional_t<decltype(f64)::value, double, float>;
    with_width(Q, [&](auto width) { with_bool(shared, [&](auto sh) { f(T{}, width, sh); }); });
  });
}

int cb_dense(cna_ctx* c, ExprState* s, CorrByWork* w, int q, int Q, bool shared, int n_bins) {
  const int64_t n = s->n, G = s->G;
  const int S = shared ? 1 : Q, F = 4 * S + Q;
  const int threads = (int)std::min<int64_t>(256, (G + 63) / 64 * 64);
  const int64_t gene_blocks = (G + threads - 1) / threads;
  const int64_t* first = w->sort.table_h.data() + n_bins + 1;     // first chunk of every level, on the host
  // groups of levels: their records within the result's own size plus cells / PB_DENSE_CHUNK chunks
  const int64_t max_chunks = std::max<int64_t>(1, (int64_t)q * n_bins / F + n / PB_DENSE_CHUNK);
  std::vector<int> cut{0};
  int64_t largest = 1;
  for (int b0 = 0, b1; b0 < n_bins; b0 = b1) {
    b1 = b0 + 1;
    while (b1 < n_bins && first[b1 + 1] - first[b0] <= max_chunks) ++b1;
    cut.push_back(b1);
    largest = std::max(largest, first[b1] - first[b0]);
  }
  if (largest * gene_blocks > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, "cna_gene_corr_by: more than 2^31 - 1 workgroups (chunks x gene blocks)");
  CNA_TRY(buf_need(c, s->st, w->part, 8 * largest * F * G));
  for (size_t k = 0; k + 1 < cut.size(); ++k) {
    const int b0 = cut[k], b1 = cut[k + 1];
    const int64_t ch0 = first[b0], nch = first[b1] - ch0;
    if (nch)
      with_kernel(s, Q, shared, [&](auto t, auto width, auto sh) {
        hipLaunchKernelGGL((k_cb_dense<decltype(t), decltype(width)::value, decltype(sh)::value>),
                           dim3((unsigned)(nch * gene_blocks)), dim3(threads), 0, s->st, s->X.as<const decltype(t)>(), G, gene_blocks,
                           ch0, w->list.as<const int32_t>(), w->sort.chunks(), w->vtab.as<const double>(),
                           w->word.as<const uint32_t>(), w->part.as<double>());
      });
    hipLaunchKernelGGL(k_cb_finish_dense, dim3((unsigned)(((int64_t)q * G + 255) / 256)), dim3(256), 0, s->st,
                       w->part.as<const double>(), G, q, Q, S, n_bins, b0, b1, w->sort.first(), w->kstat.as<const double>(),
                       w->rout.as<double>(), w->wacc.as<double>(), w->wout.as<double>(), b1 == n_bins ? 1 : 0);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int cb_sparse(cna_ctx* c, ExprState* s, CorrByWork* w, int q, int Q, bool shared, int n_bins) {
  const int S = shared ? 1 : Q, F = 5 * S + Q;
  // groups of levels: what 64 KB of LDS hold, in passes of equal size
  const int fit = CB_LDS_BYTES / (8 * F + 4);
  const int passes = (n_bins + fit - 1) / fit;
  const int per = (n_bins + passes - 1) / passes;
  int64_t need = 1;
  const std::vector<GeneTile> tiles = gene_tiles(s, 8 * (int64_t)F * per, &need);
  if (need > 0x7fffffffll / 256) CNA_FAIL(CNA_EINVAL, "cna_gene_corr_by: one gene has too many chunks");
  CNA_TRY(buf_need(c, s->st, w->part, 8 * need * F * per));
  for (int b0 = 0; b0 < n_bins; b0 += per) {
    const int nl = std::min(per, n_bins - b0);
    const size_t lds = (size_t)nl * (8 * F + 4);
    for (const GeneTile& t : tiles) {
      if (t.nch)
        with_kernel(s, Q, shared, [&](auto tt, auto width, auto sh) {
          hipLaunchKernelGGL((k_cb_sparse<decltype(tt), decltype(width)::value, decltype(sh)::value>), dim3((unsigned)t.nch),
                             dim3(64), lds, s->st, s->chunk_lo.as<const int64_t>(), s->chunk_gene.as<const int32_t>(),
                             s->gptr.as<const int64_t>(), t.c0, s->chunk_len, s->gcell.as<const int32_t>(),
                             s->gval.as<const decltype(tt)>(), w->vtab.as<const double>(), w->word.as<const uint32_t>(), b0, nl,
                             w->part.as<double>());
        });
      hipLaunchKernelGGL(k_cb_finish_sparse, dim3((unsigned)(((int64_t)q * (t.g1 - t.g0) + 255) / 256)), dim3(256), 0, s->st,
                         w->part.as<const double>(), s->gchunk.as<const int64_t>(), t.g0, t.g1, t.c0, s->G, q, Q, S, n_bins, b0, nl,
                         w->kstat.as<const double>(), w->rout.as<double>(), w->wacc.as<double>(), w->wout.as<double>(),
                         b0 + nl == n_bins ? 1 : 0);
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int cna_gene_corr_by(cna_ctx* c, const double* V, int q, const int32_t* codes, int n_bins, double* r_out,
                                double* within_out, int64_t* n_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_corr_by: no expression matrix is resident (cna_expr_upload_*)");
  if (!V || !codes || !r_out || !n_out) CNA_FAIL(CNA_EINVAL, "cna_gene_corr_by: null pointer");
  if (q < 1 || q > CB_MAXQ) CNA_FAIL(CNA_EINVAL, "cna_gene_corr_by: 1 <= q <= 16 key columns");
  if (n_bins < 1 || n_bins > CB_MAX_LEVELS) CNA_FAIL(CNA_EINVAL, "cna_gene_corr_by: 1 <= n_bins <= 1024");
  if (q * n_bins > CB_MAX_ROWS) CNA_FAIL(CNA_EINVAL, "cna_gene_corr_by: q x n_bins <= 4096");
  int Q = 1;
  while (Q < q) Q *= 2;
  const int64_t n = s->n, G = s->G;
  const int64_t rows = (int64_t)q * n_bins;
  CorrByWork* w = expr_work<CorrByWork>(s, EXPR_CORR_BY);
  // the codes are judged before any sum is formed
  CNA_TRY(sort_count(c, s->st, w->sort, CellList{}, codes, n, n_bins, PB_DENSE_CHUNK, 2,
                     "cna_gene_corr_by: a code lies outside [-1, n_bins)"));
  CNA_TRY(buf_need(c, s->st, w->list, 4 * n));
  CNA_TRY(buf_need(c, s->st, w->vraw, 8 * n * q));
  CNA_TRY(buf_need(c, s->st, w->vtab, 8 * n * Q));
  CNA_TRY(buf_need(c, s->st, w->word, 4 * n));
  CNA_TRY(buf_need(c, s->st, w->kstat, 8 * KS_LD * rows));
  CNA_TRY(buf_need(c, s->st, w->flag, 256));
  CNA_TRY(buf_need(c, s->st, w->rout, 8 * rows * G));
  CNA_TRY(buf_need(c, s->st, w->wacc, 8 * WA_LD * q * G));
  CNA_TRY(buf_need(c, s->st, w->wout, 8 * q * G));
  HIP_TRY(hipMemcpyAsync(w->vraw.p, V, (size_t)(8 * n * q), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemsetAsync(w->flag.p, 0, 4, s->st));
  HIP_TRY(hipMemsetAsync(w->wacc.p, 0, (size_t)(8 * WA_LD * q * G), s->st));
  sort_fill(s->st, w->sort, CellList{}, n, w->list.as<int32_t>());
  hipLaunchKernelGGL(k_cb_key_stats, dim3((unsigned)n_bins, (unsigned)q), dim3(256), 0, s->st, w->vraw.as<const double>(), n,
                     w->list.as<const int32_t>(), w->sort.bptr(), n_bins, w->kstat.as<double>());
  hipLaunchKernelGGL(k_cb_key_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, w->vraw.as<const double>(), n, q, Q,
                     w->sort.codes(), n_bins, w->kstat.as<const double>(), w->vtab.as<double>(), w->word.as<uint32_t>(),
                     w->flag.as<int>());
  HIP_TRY(hipGetLastError());
  // keys that leave out the same cells (usually none) share the sums of x and x^2: one set instead of q
  int differ = 0;
  HIP_TRY(hipMemcpyAsync(&differ, w->flag.p, 4, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  const bool shared = differ == 0;
  if (s->format == 1) CNA_TRY(cb_dense(c, s, w, q, Q, shared, n_bins));
  else CNA_TRY(cb_sparse(c, s, w, q, Q, shared, n_bins));
  std::vector<double> ks((size_t)(KS_LD * rows));
  if (within_out)
    CNA_TRY(fetch_results(s->st, "cna_gene_corr_by", {{r_out, w->rout.p, (size_t)(8 * rows * G)},
                                                     {within_out, w->wout.p, (size_t)(8 * q * G)},
                                                     {ks.data(), w->kstat.p, 8 * ks.size()}}));
  else
    CNA_TRY(fetch_results(s->st, "cna_gene_corr_by", {{r_out, w->rout.p, (size_t)(8 * rows * G)},
                                                     {ks.data(), w->kstat.p, 8 * ks.size()}}));
  for (int64_t k = 0; k < rows; ++k) n_out[k] = (int64_t)ks[(size_t)(k * KS_LD)];
  return 0;
}
