// cna_gene_rank_corr_x, cna_gene_rank_corr_x_by, cna_gene_rank_corr_wide, cna_x_columns: Spearman's rank correlation of
// every gene of the resident expression matrix with up to 4096 per-cell columns from ONE sort of the matrix
// (cna.tl.gene_rank_test: the null of cna.tl.gene_rank_corr under the association's permuted phenotypes, reference
// _association.py:94-99).  The null
// coefficient of permutation p is c_p = X z_p per cell (_association.py:99), and ranks are not linear in z_p: every c_p
// is formed, ranked over the kept cells and correlated with every gene's ranks.  cna_gene_rank_corr (expr_rankcorr.hip)
// takes 16 columns from the host and sorts the matrix on every call; here the columns are formed on the device from the
// working matrix X (or given by the host: _wide), ranked in groups of 16 whose tables all stay resident, and the genes are
// sorted once, whatever the number of columns.
//   k_rp_columns          thread = cell, 16 columns at a time: out[j][i] = sum over the samples, ascending, of
//                         X[xrow[i]][s] * Z[j][s], the product rounded, then added (no FMA: the pragma below); NaN for a
//                         cell without a row.  The entry cna_x_columns is this kernel alone
//   rankcorr_keys         (rank_corr.h, expr_rankcorr.hip) the ranks of one group: b = s + e - m into the group's own
//                         cell-major table btabs[group][cell][16], its tie terms into the group's own slots
//   k_rp_rank             behind the genes' sort, one workgroup per gene: the two walks of rank_sort.h once, no gathers:
//                         a = s + e - m of every stored entry, with k_rc_corr's shifts by the implicit zeros, into an int32
//                         buffer of the tile's size (0 for a left-out entry); per gene a_0 of the zero group and the tie term
//   k_rp_dot              grid (genes of the tile, groups): streams {a, cell}, gathers the cell's 64-byte row of the group's
//                         table, a * b[k] into k_rc_corr's 64 + 32-bit integer accumulators, the sum of b beside them; a
//                         fixed tree, then - a_0 * sum b.  No scan and no barrier inside the loop, one gather per entry.  The
//                         group is the slow grid index: the workgroups that run together gather from one table of 64 n bytes
// Every sum is an integer: the results are those of cna_gene_rank_corr on each group of 16 columns under the same kept
// set, integer for integer, whatever the tiling and on every run.
//
// cna_gene_rank_corr_x_by: the same inside every level of a clustering (cna.tl.gene_rank_test_strata), from the one sort
// and one table per group.  k_rp_codes_by leaves a cell its level where it has a row of X (the level as a byte per cell,
// the kept cells per level); rankcorr_keys ranks every group inside the levels; the genes' sort ends on its pass on the
// level, and k_rp_rank runs once per (gene, level), k_rp_dot once per (gene, group, level), on the level's sub-segment
// (GeneLevel of rank_corr.h, as k_rc_corr takes it) with the level's m_l, k_l and z_l.  Level l is cna_gene_rank_corr_x
// with xrow set to -1 outside l, and each group of 16 columns cna_gene_rank_corr_by on them, integer for integer.
#include "rank_corr.h"

// hipcc contracts a*b+c into an fma by default.  cna_x_columns is specified as a product rounded on its own and THEN added
// to the running sum, so that a host restatement forms the same bits term by term; contraction is off for the whole file.
#pragma clang fp contract(off)

namespace {

constexpr int RP_MAX_COLS = 4096;              // columns of one call
constexpr int RP_MAX_SAMPLES = 1024;           // samples of X, as cna_expr_cross has it
constexpr int RP_GROUP = RC_MAX_KEYS;          // columns of one table
constexpr int RP_MAX_LEVELS = 255;             // cna_gene_rank_corr_x_by: the level is a digit of the sort, 255 = left out

// codes[i] = 0 for a cell with a row of X, else -1: the kept cells as ranksum_sorted expects them
__global__ __launch_bounds__(256) void k_rp_codes(const int64_t* __restrict__ xrow, int64_t n, int32_t* __restrict__ codes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) codes[i] = xrow[i] >= 0 ? 0 : -1;
}

// cna_gene_rank_corr_x_by: codes holds the caller's levels, all in [-1, n_bins) with n_bins <= 255; a cell keeps its level
// where it has a row of X, else -1; lvl8[i] = that level as a byte, 255 for -1 (the digit of the sort's last pass);
// m[l] += the kept cells of level l (256 counters).  What k_rc_mask<true> does for finite columns
__global__ __launch_bounds__(256) void k_rp_codes_by(const int64_t* __restrict__ xrow, int64_t n, int32_t* __restrict__ codes,
                                                     uint8_t* __restrict__ lvl8, unsigned long long* __restrict__ m) {
  __shared__ unsigned int h[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  h[threadIdx.x] = 0;
  __syncthreads();
  if (i < n) {
    const int32_t cd = xrow[i] >= 0 ? codes[i] : -1;
    codes[i] = cd;
    lvl8[i] = cd >= 0 ? (uint8_t)cd : (uint8_t)255;
    if (cd >= 0) atomicAdd(&h[cd & 255], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&m[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// thread = cell i, blockIdx.y = 16 columns of the `cols` rows of Z (row-major, Nx each): out[j * n + i].  The row of Z is
// the same in every lane; a column past the last one repeats the last and is not stored.  *bad |= 1 where a formed value is
// not finite (bad may be null: nothing is judged).
__global__ __launch_bounds__(256) void k_rp_columns(const int64_t* __restrict__ xrow, int64_t n, const double* __restrict__ Xw,
                                                    int ldx, int Nx, const double* __restrict__ Z, int cols,
                                                    double* __restrict__ out, int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j0 = (int)blockIdx.y * RP_GROUP;
  const int64_t xr = xrow[i];
  double acc[RP_GROUP];
#pragma unroll
  for (int j = 0; j < RP_GROUP; ++j) acc[j] = xr >= 0 ? 0.0 : __longlong_as_double(0x7ff8000000000000ll);
  if (xr >= 0) {
    const double* row = Xw + xr * ldx;
    for (int s = 0; s < Nx; ++s) {
      const double x = row[s];
#pragma unroll
      for (int j = 0; j < RP_GROUP; ++j) {
        const int jj = j0 + j < cols ? j0 + j : cols - 1;
        const double p = x * Z[(int64_t)jj * Nx + s];
        acc[j] = acc[j] + p;
      }
    }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < RP_GROUP; ++j)
    if (j0 + j < cols) {
      out[(int64_t)(j0 + j) * n + i] = acc[j];
      ok = ok && (xr < 0 || finite_d(acc[j]));
    }
  if (bad && !ok) atomicOr(bad, 1);
}

// workgroup = (gene g0 + blockIdx.x, level blockIdx.y) over the k sorted entries {key, cell} its source names (rank_corr.h:
// the gene's whole list among m kept cells, or the sub-segment of the level among the level's m_l), z = m - k implicit
// zeros.  a = s + e - m as k_rc_corr splits it: the walk forward stores s - m (+ z above the zero group), the walk backward
// adds e (+ z from the zero group on) -- the same thread holds an entry in both.  a[] is indexed like the tile's entries;
// a_0 and the tie term go to [level][gene].  A list of no entry walks nothing, meets the fold's barriers and writes the
// zero group alone: a_0 = 0 and its tie term.
template <typename K, class Src>
__global__ __launch_bounds__(RS_UNIT) void k_rp_rank(const K* __restrict__ key, const uint32_t* __restrict__ cell,
                                                     const int64_t* __restrict__ seg, int64_t base, int64_t g0, int64_t G,
                                                     Src src, int64_t n, int32_t* __restrict__ a, long long* __restrict__ a0,
                                                     double* __restrict__ tie) {
  constexpr K K0 = rs_key_zero<K>();
  __shared__ long long sh[RS_UNIT];
  __shared__ double tsh[RS_UNIT];
  __shared__ unsigned int below, zeros;
  const int64_t g = g0 + blockIdx.x;
  long long at, k, m;
  src(g, (int64_t)blockIdx.x, (int)blockIdx.y, &at, &k, &m);
  const long long z = m - k;
  key += seg[g] - base + at;
  cell += seg[g] - base + at;
  a += seg[g] - base + at;
  a0 += (int64_t)blockIdx.y * G;
  tie += (int64_t)blockIdx.y * G;
  if (threadIdx.x == 0) below = zeros = 0;
  __syncthreads();
  RankWalkMine mine;
  rs_walk_forward(key, k, sh, mine, [&](long long p, K kk, long long s) {
    a[p] = (int64_t)cell[p] < n ? (int32_t)(s + (kk > K0 ? z : 0) - m) : 0;     // (a left-out entry: a gene with a kept NaN)
  });
  rs_walk_backward(key, k, sh, [&](long long p, K kk, long long e) {
    if ((int64_t)cell[p] < n) a[p] += (int32_t)(e + (kk >= K0 ? z : 0));
  });
  const RankWalkZero zero = rs_walk_fold(mine, z, tsh, &below, &zeros);
  if (threadIdx.x == 0) {
    tie[g] = zero.tie;
    a0[g] = 2 * zero.below + zero.t0 - m;
  }
}

// workgroup = (gene g0 + blockIdx.x, group blockIdx.y, level blockIdx.z): sum over the stored kept entries its source names
// (k_rp_rank's: the gene's, or those of the level's sub-segment) of a x b[k] for the 16 columns of the group, k_rc_corr's
// accumulators (64 low bits and a 32-bit count of carries less borrows per thread and column) and its fold; the zero group's share is -a_0 x (sum of b over the stored kept entries).  Column k of the call is
// column k % 16 of group k / 16; the columns from q on are not stored.  Results go to [level][column][gene].  The level
// moves the pointers once, in front of the loop, which holds what it held.  A list of no entry writes zeros.
template <class Src>
__global__ __launch_bounds__(RS_UNIT) void k_rp_dot(const int32_t* __restrict__ a, const uint32_t* __restrict__ cell,
                                                    const int64_t* __restrict__ seg, int64_t base, int64_t g0, int64_t G,
                                                    Src src, int64_t n, int q,
                                                    const BRow<RP_GROUP>* __restrict__ btabs, const long long* __restrict__ a0,
                                                    unsigned long long* __restrict__ s_lo, long long* __restrict__ s_hi) {
  constexpr int W = RP_GROUP;
  __shared__ unsigned long long flo[RS_UNIT], fhi[RS_UNIT];
  __shared__ long long fsb[RS_UNIT];
  const int t = threadIdx.x;
  const int64_t g = g0 + blockIdx.x;
  const int k0 = (int)blockIdx.y * W;
  long long at, k, m;
  src(g, (int64_t)blockIdx.x, (int)blockIdx.z, &at, &k, &m);
  a += seg[g] - base + at;
  cell += seg[g] - base + at;
  a0 += (int64_t)blockIdx.z * G;
  s_lo += (int64_t)blockIdx.z * q * G;
  s_hi += (int64_t)blockIdx.z * q * G;
  const BRow<W>* __restrict__ btab = btabs + (int64_t)blockIdx.y * n;
  unsigned long long lo[W];
  int hi[W];
  long long sb[W];
#pragma unroll
  for (int j = 0; j < W; ++j) lo[j] = hi[j] = sb[j] = 0;
  for (long long p = t; p < k; p += RS_UNIT) {
    const uint32_t cl = cell[p];
    if ((int64_t)cl >= n) continue;
    const long long coef = (long long)a[p];
    const BRow<W> row = btab[cl];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const long long x = coef * (long long)row.v[j];
      const unsigned long long old = lo[j];
      lo[j] = old + (unsigned long long)x;
      hi[j] += (lo[j] < old ? 1 : 0) - (x < 0 ? 1 : 0);
      sb[j] += row.v[j];
    }
  }
  const long long na0 = -a0[g];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    if (k0 + j < q) {                                   // (the workgroup's: the barriers are met by all or none)
      flo[t] = lo[j];
      fhi[t] = (unsigned long long)(long long)hi[j];    // sign-extended: two's complement on 128 bits
      fsb[t] = sb[j];
      __syncthreads();
      for (int w = RS_UNIT / 2; w > 0; w >>= 1) {
        if (t < w) {
          const U128 x = u128_add({flo[t], fhi[t]}, {flo[t + w], fhi[t + w]});
          flo[t] = x.lo;
          fhi[t] = x.hi;
          fsb[t] += fsb[t + w];
        }
        __syncthreads();
      }
      if (t == 0) {
        const long long B = fsb[0];
        const U128 x = u128_add({flo[0], fhi[0]}, {(unsigned long long)na0 * (unsigned long long)B,
                                                  (unsigned long long)__mul64hi(na0, B)});
        s_lo[(int64_t)(k0 + j) * G + g] = x.lo;
        s_hi[(int64_t)(k0 + j) * G + g] = (long long)x.hi;
      }
      __syncthreads();
    }
  }
}

// The levels of a call: one of all kept cells (lvl8 null: cna_gene_rank_corr_x, _wide), or the caller's (_x_by): the kept
// cell's level as a byte in lvl8, the sort ending on its pass on the level, and the kept cells of every level on the
// device (w->vm) and on the host (mlev)
struct RankPermLevels {
  int n_bins = 1;
  const uint8_t* lvl8 = nullptr;
  const unsigned long long* mlev = nullptr;
};

// the genes' side: one sort of the matrix per tile of genes, the rank kernel and the dot kernel behind each; with levels,
// the rank kernel once per (gene, level) and the dot kernel once per (gene, group, level), each on the level's sub-segment
template <typename T>
int rankperm_genes(cna_ctx* c, ExprState* s, RankSumWork* w, const char* who, int q, int groups, int64_t m, int64_t work_bytes,
                   const RankPermLevels& lv) {
  using K = typename KeyOf<T>::K;
  const int64_t G = s->G, n = s->n;
  int rc = 0;
  CNA_TRY((ranksum_sorted<T, uint32_t>(
      c, s, w, work_bytes, m, who,
      [&](const GeneTile& t, int64_t base, const K* key, const uint32_t* cell, const int64_t* seg) {
        if (rc != 0) return;
        const unsigned genes = (unsigned)(t.g1 - t.g0);
        const int64_t entries = s->format == 1 ? (int64_t)genes * n : t.nch * s->chunk_len;   // of the tile, at most
        rc = buf_need(c, s->st, w->aent, 4 * std::max<int64_t>(1, entries));
        if (rc != 0) return;
        const auto launch = [&](auto src) {
          {
            ProfScope ps(c, CNA_K_RANKSUM_RANK, s->st);
            hipLaunchKernelGGL((k_rp_rank<K, decltype(src)>), dim3(genes, (unsigned)lv.n_bins), dim3(RS_UNIT), 0, s->st, key, cell,
                               seg, base, t.g0, G, src, n, w->aent.as<int32_t>(), w->azero.as<long long>(), w->tie.as<double>());
          }
          ProfScope ps(c, CNA_K_RANKCORR_CORR, s->st);
          hipLaunchKernelGGL((k_rp_dot<decltype(src)>), dim3(genes, (unsigned)groups, (unsigned)lv.n_bins), dim3(RS_UNIT), 0, s->st,
                             w->aent.as<const int32_t>(), cell, seg, base, t.g0, G, src, n, q,
                             w->btabs.as<const BRow<RP_GROUP>>(), w->azero.as<const long long>(),
                             w->slo.as<unsigned long long>(), w->shi.as<long long>());
        };
        if (lv.lvl8) launch(GeneLevel{w->dbase.as<const unsigned int>(), w->vm.as<const unsigned long long>()});
        else launch(WholeGene{w->kept.as<const unsigned int>(), (long long)m});
      },
      lv.lvl8)));
  return rc;
}

struct RankPermOut {
  uint64_t* s_lo;
  int64_t* s_hi;
  double *tie_gene, *tie_key;
  int64_t* m;
  uint8_t* nan;
};

// What the entries share behind their checks, with the kept cells in w->sort.code and their number m (over all levels).
// fill(k0, cols) queues what puts the columns [k0, k0 + cols) of the call into w->vcol (cols x n); verdict() is asked once
// behind the last group, before the matrix is sorted.  Every group's table and tie terms stay resident: 64 n bytes and, per
// level, 16 x 12 bytes each (slot [group][level][column of the group], as rankcorr_keys lays a group's out).  Outputs per
// level: s_lo, s_hi [n_bins, q, G], tie_gene [n_bins, G], tie_key [n_bins, q], m [n_bins].
template <class Fill, class Verdict>
int rankperm_core(cna_ctx* c, ExprState* s, RankSumWork* w, const char* who, int q, int64_t m, int64_t work_bytes, Fill&& fill,
                  Verdict&& verdict, const RankPermOut& out, const RankPermLevels& lv = {}) {
  const int64_t G = s->G, n = s->n;
  const int groups = (q + RP_GROUP - 1) / RP_GROUP;
  const int64_t group_slots = (int64_t)lv.n_bins * RP_GROUP, slots = groups * group_slots;
  const int64_t tab_bytes = 4 * (int64_t)RP_GROUP * n, tie_bytes = 12 * slots;
  const int64_t s_bytes = 8 * (int64_t)lv.n_bins * q * G, t_bytes = 8 * (int64_t)lv.n_bins * G;
  CNA_TRY(result_bufs_need(c, s->st, {{&w->vcol, 8 * (int64_t)RP_GROUP * n},
                                      {&w->btabs, tab_bytes * groups},
                                      {&w->tieks, tie_bytes},
                                      {&w->slo, s_bytes},
                                      {&w->shi, s_bytes},
                                      {&w->tie, t_bytes},
                                      {&w->azero, t_bytes}}));
  unsigned long long* tie_lo = w->tieks.as<unsigned long long>();          // [slot] 64 low bits, then [slot] 32 high bits
  unsigned int* tie_hi = w->tieks.as<unsigned int>() + 2 * slots;
  {
    // the rows of the tables of the cells left out, and the columns from q on, are never meant: zero, so that what the
    // gather reads of them is defined
    ProfScope ps(c, CNA_K_RANKCORR_KEYS, s->st);
    HIP_TRY(hipMemsetAsync(w->btabs.p, 0, (size_t)(tab_bytes * groups), s->st));
    HIP_TRY(hipMemsetAsync(w->tieks.p, 0, (size_t)tie_bytes, s->st));
  }
  for (int gi = 0; gi < groups; ++gi) {
    const int k0 = gi * RP_GROUP, cols = std::min(RP_GROUP, q - k0);
    CNA_TRY(fill(k0, cols));
    CNA_TRY(rankcorr_keys(c, s, w, cols, RP_GROUP, work_bytes, m, lv.lvl8, w->btabs.as<int32_t>() + (int64_t)k0 * n,
                          tie_lo + gi * group_slots, tie_hi + gi * group_slots, who));
  }
  CNA_TRY(verdict());
  if (s->is_f64) CNA_TRY(rankperm_genes<double>(c, s, w, who, q, groups, m, work_bytes, lv));
  else CNA_TRY(rankperm_genes<float>(c, s, w, who, q, groups, m, work_bytes, lv));
  std::vector<unsigned int> nanf((size_t)G);
  std::vector<unsigned long long> tie_words((size_t)(tie_bytes / 8) + 1);
  {
    ProfScope ps(c, CNA_K_RANKSUM_FETCH, s->st);
    CNA_TRY(fetch_results(s->st, who, {{out.s_lo, w->slo.p, (size_t)s_bytes},
                                       {out.s_hi, w->shi.p, (size_t)s_bytes},
                                       {out.tie_gene, w->tie.p, (size_t)t_bytes},
                                       {tie_words.data(), w->tieks.p, (size_t)tie_bytes},
                                       {nanf.data(), w->nanf.p, (size_t)(4 * G)}}));
  }
  for (int64_t g = 0; g < G; ++g) out.nan[g] = nanf[(size_t)g] ? 1 : 0;
  const unsigned int* tie_high = reinterpret_cast<const unsigned int*>(tie_words.data() + slots);
  for (int l = 0; l < lv.n_bins; ++l) {
    for (int k = 0; k < q; ++k) {                       // rounded once
      const size_t slot = (size_t)((k / RP_GROUP) * group_slots + (int64_t)l * RP_GROUP + k % RP_GROUP);
      out.tie_key[(int64_t)l * q + k] = (double)tie_high[slot] * 18446744073709551616.0 + (double)tie_words[slot];
    }
    out.m[l] = lv.mlev ? (int64_t)lv.mlev[l] : m;
  }
  return 0;
}

// What cna_x_columns and cna_gene_rank_corr_x check alike, in cna_expr_cross's order and words; then xrow on the device,
// judged, and the expression stream behind whatever the main stream has queued that produces X
int x_entry(cna_ctx* c, const char* who, const int64_t* xrow, int64_t n_cells, const double* Z, int q, bool null_out,
            ExprState** s_out, RankSumWork** w_out, int64_t* m) {
  const std::string me(who);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, me + ": no expression matrix is resident (cna_expr_upload_*)");
  if (c->auto_pending) CNA_TRY(cna_nam_auto_finish(c, nullptr, nullptr));
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, me + ": X not available");
  if (comm_active(c)) CNA_FAIL(CNA_ESTATE, me + ": one rank only (the rows of X of other ranks are not here)");
  if (!xrow || !Z || null_out) CNA_FAIL(CNA_EINVAL, me + ": null pointer");
  if (n_cells != s->n)
    CNA_FAIL(CNA_EINVAL, me + ": xrow has " + std::to_string(n_cells) + " entries, the expression matrix " +
                             std::to_string(s->n) + " cells");
  if (q < 1 || q > RP_MAX_COLS) CNA_FAIL(CNA_EINVAL, me + ": 1 <= q <= 4096");
  if (c->Nx < 1 || c->Nx > RP_MAX_SAMPLES) CNA_FAIL(CNA_EINVAL, me + ": 1 <= columns of X <= 1024");
  RankSumWork* w = expr_work<RankSumWork>(s, EXPR_RANKSUM);
  const int64_t n = s->n;
  CNA_TRY(buf_need(c, s->st, w->xrow, 8 * n));
  CNA_TRY(buf_need(c, s->st, w->zrows, 8 * (int64_t)q * c->Nx));
  HIP_TRY(hipMemcpyAsync(w->xrow.p, xrow, (size_t)(8 * n), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemcpyAsync(w->zrows.p, Z, (size_t)(8 * (int64_t)q * c->Nx), hipMemcpyHostToDevice, s->st));
  CNA_TRY(xrow_check(c, s->st, w->xrow.as<const int64_t>(), n, c->nx, w->xseen, w->xflag, who, m));   // (drains the stream)
  HIP_TRY(hipEventRecord(s->x_ready, c->stream));
  HIP_TRY(hipStreamWaitEvent(s->st, s->x_ready, 0));
  *s_out = s;
  *w_out = w;
  return 0;
}

// What cna_gene_rank_corr_x and cna_gene_rank_corr_x_by share behind x_entry, with the kept cells in w->sort.code: the
// columns formed from X group by group, the verdict on what was formed, the core
int rankperm_x(cna_ctx* c, ExprState* s, RankSumWork* w, const char* who, int q, int64_t m, int64_t work_bytes,
               const RankPermOut& out, const RankPermLevels& lv) {
  const int64_t n = s->n;
  const dim3 cells((unsigned)((n + 255) / 256));
  CNA_TRY(buf_need(c, s->st, w->vcol, 8 * (int64_t)RP_GROUP * n));
  int* bad = w->xflag.as<int>() + 8;                   // (behind xrow_check's verdict and count)
  HIP_TRY(hipMemsetAsync(bad, 0, 4, s->st));
  const auto fill = [&](int k0, int cols) {
    ProfScope ps(c, CNA_K_RANKCORR_KEYS, s->st);
    hipLaunchKernelGGL(k_rp_columns, cells, dim3(256), 0, s->st, w->xrow.as<const int64_t>(), n, (const double*)c->X, c->ldx, c->Nx,
                       w->zrows.as<const double>() + (int64_t)k0 * c->Nx, cols, w->vcol.as<double>(), bad);
    HIP_TRY(hipGetLastError());
    return 0;
  };
  const auto verdict = [&]() {
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, bad, 4, hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
    if (flag) CNA_FAIL(CNA_EINVAL, std::string(who) + ": a formed value X[xrow[i]] . Z[j] is not finite (an inf or a NaN in X or in Z)");
    return 0;
  };
  return rankperm_core(c, s, w, who, q, m, work_bytes, fill, verdict, out, lv);
}

}  // namespace

extern "C" int cna_x_columns(cna_ctx* c, const int64_t* xrow, int64_t n_cells, const double* Z, int q, double* out) {
  CHECK_CTX(c);
  ExprState* s = nullptr;
  RankSumWork* w = nullptr;
  int64_t m = 0;
  CNA_TRY(x_entry(c, "cna_x_columns", xrow, n_cells, Z, q, !out, &s, &w, &m));
  const int64_t n = s->n, bytes = 8 * (int64_t)q * n;
  CNA_TRY(result_bufs_need(c, s->st, {{&w->xcols, bytes}}));
  {
    ProfScope ps(c, CNA_K_RANKCORR_KEYS, s->st);
    hipLaunchKernelGGL(k_rp_columns, dim3((unsigned)((n + 255) / 256), (unsigned)((q + RP_GROUP - 1) / RP_GROUP)), dim3(256), 0,
                       s->st, w->xrow.as<const int64_t>(), n, (const double*)c->X, c->ldx, c->Nx, w->zrows.as<const double>(), q,
                       w->xcols.as<double>(), (int*)nullptr);
  }
  ProfScope ps(c, CNA_K_RANKSUM_FETCH, s->st);
  return fetch_results(s->st, "cna_x_columns", {{out, w->xcols.p, (size_t)bytes}});
}

extern "C" int cna_gene_rank_corr_x(cna_ctx* c, const int64_t* xrow, int64_t n_cells, const double* Z, int q, int64_t work_bytes,
                                    uint64_t* s_lo, int64_t* s_hi, double* tie_gene, double* tie_key, int64_t* m_out,
                                    uint8_t* nan_out) {
  CHECK_CTX(c);
  const char* who = "cna_gene_rank_corr_x";
  if (work_bytes < 0) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_x: work_bytes is 0 (the default) or a number of bytes");
  ExprState* s = nullptr;
  RankSumWork* w = nullptr;
  int64_t m = 0;
  CNA_TRY(x_entry(c, who, xrow, n_cells, Z, q, !s_lo || !s_hi || !tie_gene || !tie_key || !m_out || !nan_out, &s, &w, &m));
  const int64_t n = s->n;
  CNA_TRY(buf_need(c, s->st, w->sort.code, 4 * n));
  hipLaunchKernelGGL(k_rp_codes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, w->xrow.as<const int64_t>(), n,
                     w->sort.code.as<int32_t>());
  return rankperm_x(c, s, w, who, q, m, work_bytes, {s_lo, s_hi, tie_gene, tie_key, m_out, nan_out}, {});
}

extern "C" int cna_gene_rank_corr_x_by(cna_ctx* c, const int64_t* xrow, int64_t n_cells, const double* Z, int q,
                                       const int32_t* codes, int n_bins, int64_t work_bytes, uint64_t* s_lo, int64_t* s_hi,
                                       double* tie_gene, double* tie_key, int64_t* m_out, uint8_t* nan_out) {
  CHECK_CTX(c);
  const char* who = "cna_gene_rank_corr_x_by";
  if (work_bytes < 0) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_x_by: work_bytes is 0 (the default) or a number of bytes");
  ExprState* s = nullptr;
  RankSumWork* w = nullptr;
  int64_t with_row = 0;
  CNA_TRY(x_entry(c, who, xrow, n_cells, Z, q, !codes || !s_lo || !s_hi || !tie_gene || !tie_key || !m_out || !nan_out, &s, &w,
                  &with_row));
  if (n_bins < 1 || n_bins > RP_MAX_LEVELS) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_x_by: 1 <= n_bins <= 255");
  const int64_t n = s->n;
  // the caller's codes into w->sort.code, judged; then a cell keeps its level where it has a row of X
  CNA_TRY(sort_count(c, s->st, w->sort, CellListOf<256>{}, codes, n, n_bins, 0, 2,
                     "cna_gene_rank_corr_x_by: a code lies outside [-1, n_bins)"));
  CNA_TRY(buf_need(c, s->st, w->lvl8, n));
  CNA_TRY(buf_need(c, s->st, w->vm, 8 * 256));
  std::vector<unsigned long long> mlev((size_t)n_bins);
  {
    ProfScope ps(c, CNA_K_RANKCORR_KEYS, s->st);
    HIP_TRY(hipMemsetAsync(w->vm.p, 0, 8 * 256, s->st));
    hipLaunchKernelGGL(k_rp_codes_by, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, w->xrow.as<const int64_t>(), n,
                       w->sort.code.as<int32_t>(), w->lvl8.as<uint8_t>(), w->vm.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mlev.data(), w->vm.p, 8 * (size_t)n_bins, hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
  }
  int64_t m = 0;
  for (int b = 0; b < n_bins; ++b) m += (int64_t)mlev[(size_t)b];
  return rankperm_x(c, s, w, who, q, m, work_bytes, {s_lo, s_hi, tie_gene, tie_key, m_out, nan_out},
                    {n_bins, w->lvl8.as<const uint8_t>(), mlev.data()});
}

extern "C" int cna_gene_rank_corr_wide(cna_ctx* c, const double* V, int q, int64_t work_bytes, uint64_t* s_lo, int64_t* s_hi,
                                       double* tie_gene, double* tie_key, int64_t* m_out, uint8_t* nan_out) {
  CHECK_CTX(c);
  const char* who = "cna_gene_rank_corr_wide";
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_rank_corr_wide: no expression matrix is resident (cna_expr_upload_*)");
  if (!V || !s_lo || !s_hi || !tie_gene || !tie_key || !m_out || !nan_out) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_wide: null pointer");
  if (q < 1 || q > RP_MAX_COLS) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_wide: 1 <= q <= 4096");
  if (work_bytes < 0) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_wide: work_bytes is 0 (the default) or a number of bytes");
  RankSumWork* w = expr_work<RankSumWork>(s, EXPR_RANKSUM);
  const int64_t n = s->n;
  const int groups = (q + RP_GROUP - 1) / RP_GROUP;
  CNA_TRY(buf_need(c, s->st, w->sort.code, 4 * n));
  CNA_TRY(buf_need(c, s->st, w->vcol, 8 * (int64_t)RP_GROUP * n));
  CNA_TRY(buf_need(c, s->st, w->lvl8, n));
  CNA_TRY(buf_need(c, s->st, w->vm, 8 * 256));
  const auto upload = [&](int k0, int cols) {
    HIP_TRY(hipMemcpyAsync(w->vcol.p, V + (int64_t)k0 * n, (size_t)(8 * (int64_t)cols * n), hipMemcpyHostToDevice, s->st));
    return 0;
  };
  // the kept cells: every one of the q columns finite, one set per call.  k_rc_mask<true> on one level of all cells keeps a
  // cell only while every group so far is finite there; the count behind the last group is m
  unsigned long long m = 0;
  {
    ProfScope ps(c, CNA_K_RANKCORR_KEYS, s->st);
    HIP_TRY(hipMemsetAsync(w->sort.code.p, 0, (size_t)(4 * n), s->st));
    for (int gi = 0; gi < groups; ++gi) {
      const int k0 = gi * RP_GROUP, cols = std::min(RP_GROUP, q - k0);
      CNA_TRY(upload(k0, cols));
      HIP_TRY(hipMemsetAsync(w->vm.p, 0, 8 * 256, s->st));
      hipLaunchKernelGGL(k_rc_mask<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, w->vcol.as<const double>(), cols,
                         n, w->sort.code.as<int32_t>(), w->lvl8.as<uint8_t>(), w->vm.as<unsigned long long>());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&m, w->vm.p, 8, hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
  }
  const auto fill = [&](int k0, int cols) {
    if (groups == 1) return 0;                          // (the one group is in w->vcol since the kept cells were found)
    ProfScope ps(c, CNA_K_RANKCORR_KEYS, s->st);
    return upload(k0, cols);
  };
  return rankperm_core(c, s, w, who, q, (int64_t)m, work_bytes, fill, []() { return 0; },
                       {s_lo, s_hi, tie_gene, tie_key, m_out, nan_out});
}
