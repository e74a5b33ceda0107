// cna_gene_rank_corr: Spearman's rank correlation of every gene of the resident expression matrix with up to 16 per-cell
// columns (cna.tl.gene_rank_corr), as exact integers.  The genes are sorted with the cell as an entry's payload (uint32_t),
// and the columns are ranked by the same passes (rank_sort.h): rs_passes knows a chunk table and nothing of the matrix.
//   k_rc_mask             (rank_corr.h, shared with expr_rankperm.hip) the kept cells (every column finite) as the codes
//                         ranksum_sorted expects, and their number m
//   k_rc_vkeys            the columns as q segments of n entries {float64 key, cell} in a table of the dense form's shape
//   k_rc_keyrank          behind their sort, one thread per kept entry: its tie run [s, e), by binary search where a neighbour
//                         ties -> b = s + e - m (twice the midrank less m + 1) into the cell-major table btab[cell][W]; the
//                         column's tie term in integers
//   k_rc_corr             behind the genes' sort, one workgroup per gene: a = s + e - m of every entry by the two walks of
//                         rank_sort.h, the cell's row of btab gathered in each, sum a b per column in 96-bit integer
//                         registers, the implicit zeros by arithmetic; the two limbs of S and the gene's tie term
// (two walks and not one that keeps its runs open: a = (s - m) + e is linear, so each adds its own half and nothing about
// an open run is carried but its start; the price is the second gather of the row, from the same table in reverse order)
//
// cna_gene_rank_corr_by: the same inside every level of a clustering (cna.tl.gene_rank_corr_strata), from one sort.  The
// kept cells keep their level (k_rc_mask<true>: the level as a byte per cell, the kept cells per level) and the sort ends
// on its pass on the level, so a gene's list, and a column's segment, is level-major and dbase says where every (segment,
// level) begins.  k_rc_keyrank<true> keeps its searches inside the level's range and k_rc_corr runs once per (gene, level)
// on the sub-segment (GeneLevel) with the level's m_l, k_l and z_l: level l is cna_gene_rank_corr on columns set to NaN
// outside l, integer for integer.
#include "rank_corr.h"

namespace {

constexpr int RC_MAX_LEVELS = 255;             // cna_gene_rank_corr_by: the level is a digit of the sort, 255 = left out

// With r the midrank over the m kept cells, a_i = 2 r_gene(i) - (m + 1) and b_i = 2 r_column(i) - (m + 1) are integers
// that sum to 0 over the kept cells, and a tie run [s, e) of a sorted list gives each of its entries s + e - m.
//   S[k, g] = sum over the kept cells of a_i b_i[k]      rho = 3 S / sqrt((m^3 - m - T_g) (m^3 - m - T_k))   (the host's line)
// |S| <= (m^3 - m) / 3 passes 2^63 from 3 024 617 cells on, so S is summed and returned in 128 bits.

// column k0 + blockIdx.y as a segment of n entries {key of the float64 value, cell}; a left-out cell sorts behind the kept
__global__ __launch_bounds__(256) void k_rc_vkeys(const double* __restrict__ V, int64_t n, int k0,
                                                  const int32_t* __restrict__ codes, uint64_t* __restrict__ key,
                                                  uint32_t* __restrict__ cell) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t at = (int64_t)blockIdx.y * n + i;
  uint64_t k = ~0ull;
  uint32_t cl = rs_left<uint32_t>();
  if (codes[i] >= 0) {
    bool is_nan;
    k = rs_key<double>(V[(int64_t)(k0 + blockIdx.y) * n + i], &is_nan);      // (a kept cell is finite)
    cl = (uint32_t)i;
  }
  key[at] = k;
  cell[at] = cl;
}

// thread = kept position p of column k0 + blockIdx.y, whose m kept entries head its sorted segment.  The segment is sorted,
// so the tie run [s, e) of an entry is where its key begins and ends: the entry itself when its neighbour differs, else a
// binary search (a column is one segment of up to 2^31 entries: one workgroup walking it, as k_rc_corr walks a gene, took
// 13 ms for a million cells).  btab[cell][column] = s + e - m; the tail of a run adds t^3 - t to the column's tie term in
// integers, per workgroup in LDS and then once to the device's (exact and commutative: rp_add128).
// BY (cna_gene_rank_corr_by): the segment is level-major behind the sort's last pass and level l of this column is its
// positions [dbase[l], dbase[l + 1]): the entry is ranked inside its level -- the searches stay in that range, so a run ends
// where the level does -- and b = s + e - 2 start - m_l; the tie terms are kept per level, tie[l][column], the workgroup's
// LDS sum serving the level of its first entry and the few entries of a later level adding to the device's themselves.
template <bool BY>
__global__ __launch_bounds__(256) void k_rc_keyrank(const uint64_t* __restrict__ key, const uint32_t* __restrict__ cell,
                                                    int64_t n, int k0, long long m, int stride, int32_t* __restrict__ btab,
                                                    unsigned long long* __restrict__ tie_lo, unsigned int* __restrict__ tie_hi,
                                                    const uint8_t* __restrict__ lvl8, const unsigned int* __restrict__ dbase) {
  __shared__ unsigned long long tl;
  __shared__ unsigned int th;
  __shared__ int first_level;
  const int col = k0 + (int)blockIdx.y;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  key += (int64_t)blockIdx.y * n;
  cell += (int64_t)blockIdx.y * n;
  if (threadIdx.x == 0) {
    tl = 0;
    th = 0;
    first_level = 0;
    if constexpr (BY) {
      if (p < m && (int64_t)cell[p] < n) first_level = (int)lvl8[cell[p]];
    }
  }
  __syncthreads();
  if (p < m) {
    const uint64_t kk = key[p];
    const uint32_t cl = cell[p];
    long long from = 0, to = m;                       // the positions the entry is ranked among
    int level = 0;
    if constexpr (BY) {
      level = (int64_t)cl < n ? (int)lvl8[cl] : 255;
      if (level < 255) {                              // (a kept entry: the first m of the segment are)
        from = (long long)dbase[(int64_t)blockIdx.y * 256 + level];
        to = (long long)dbase[(int64_t)blockIdx.y * 256 + level + 1];
      }
    }
    long long s = p, e = p + 1;
    if (p > from && key[p - 1] == kk) {               // the first position of [from, p) with this key
      long long lo = from, hi = p - 1;
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (key[mid] < kk) lo = mid + 1;
        else hi = mid;
      }
      s = lo;
    }
    if (p + 1 < to && key[p + 1] == kk) {             // one past the last position of (p, to) with this key
      long long lo = p + 2, hi = to;
      while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (key[mid] > kk) hi = mid;
        else lo = mid + 1;
      }
      e = lo;
    }
    if ((int64_t)cl < n) btab[(int64_t)cl * stride + col] = (int32_t)(s + e - 2 * from - (to - from));
    if (e == p + 1 && e - s > 1) {
      const U128 term = rp_tie_term((unsigned long long)(e - s));
      if (level == first_level) rp_add128(&tl, &th, term);
      else if (level < 255) rp_add128(&tie_lo[level * RC_MAX_KEYS + col], &tie_hi[level * RC_MAX_KEYS + col], term);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) rp_add128(&tie_lo[first_level * RC_MAX_KEYS + col], &tie_hi[first_level * RC_MAX_KEYS + col], {tl, (unsigned long long)th});
}

// workgroup = gene g0 + blockIdx.x over its kept[g] sorted entries {key, cell}.  a_i = s + e - m splits into a walk forward
// (s - m, in [-m, 0)) and one backward (e, in [1, m]), with their shifts by the z implicit zeros; each walk gathers the
// entry's row and adds coefficient x b[k] -- a product below 2^62 in absolute value -- into the thread's sum for column k:
// 64 low bits and a 32-bit count of carries less borrows (|sum| < 2^93 whatever the order).  The forward walk also sums b:
// the implicit zeros are one group with a_0 = 2 below + t0 - m, and because b sums to 0 over the kept cells their share is
// -a_0 x (sum of b over the stored kept entries), one 64 x 64 -> 128-bit product at the end.  The threads' sums are folded
// by a fixed tree (integers: exact in any order).  Registers: W x (2 + 1 + 2) for the sums and W for the row, 96 of them
// at W = 16.
//
// What the workgroup walks is its source's to say -- where the list begins inside the gene's segment, its k stored kept
// entries and the m cells they are ranked among: the gene's whole list (cna_gene_rank_corr) or, behind the sort's pass on
// the level, the sub-segment of level blockIdx.y (cna_gene_rank_corr_by: k_l, m_l, z_l = m_l - k_l; a run cannot cross a
// level because the list is one level's, and b sums to 0 over the level's kept cells, so the zero group's share holds).
// Results go to [level][column][gene] and [level][gene].  (WholeGene and GeneLevel: rank_corr.h.)
template <typename K, int W, class Src>
__global__ __launch_bounds__(RS_UNIT) void k_rc_corr(const K* __restrict__ key, const uint32_t* __restrict__ cell,
                                                     const int64_t* __restrict__ seg, int64_t base, int64_t g0, int64_t G,
                                                     Src src, int64_t n, int q,
                                                     const BRow<W>* __restrict__ btab, unsigned long long* __restrict__ s_lo,
                                                     long long* __restrict__ s_hi, double* __restrict__ tie) {
  constexpr K K0 = rs_key_zero<K>();
  __shared__ long long sh[RS_UNIT];
  __shared__ double tsh[RS_UNIT];
  __shared__ unsigned long long flo[RS_UNIT], fhi[RS_UNIT];
  __shared__ long long fsb[RS_UNIT];
  __shared__ unsigned int below, zeros;
  const int t = threadIdx.x;
  const int64_t g = g0 + blockIdx.x;
  long long at, k, m;
  src(g, (int64_t)blockIdx.x, (int)blockIdx.y, &at, &k, &m);
  const long long z = m - k;
  key += seg[g] - base + at;
  cell += seg[g] - base + at;
  s_lo += (int64_t)blockIdx.y * q * G;
  s_hi += (int64_t)blockIdx.y * q * G;
  tie += (int64_t)blockIdx.y * G;
  if (t == 0) below = zeros = 0;
  __syncthreads();
  unsigned long long lo[W];
  int hi[W];
  long long sb[W];
#pragma unroll
  for (int j = 0; j < W; ++j) lo[j] = hi[j] = sb[j] = 0;
  const auto add = [&](long long coef, const BRow<W>& row) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const long long x = coef * (long long)row.v[j];
      const unsigned long long old = lo[j];
      lo[j] = old + (unsigned long long)x;
      hi[j] += (lo[j] < old ? 1 : 0) - (x < 0 ? 1 : 0);
    }
  };
  RankWalkMine mine;
  rs_walk_forward(key, k, sh, mine, [&](long long p, K kk, long long s) {
    const uint32_t cl = cell[p];
    if ((int64_t)cl < n) {                            // (only a gene with a kept NaN can show a left-out entry here)
      const BRow<W> row = btab[cl];
      add(s + (kk > K0 ? z : 0) - m, row);
#pragma unroll
      for (int j = 0; j < W; ++j) sb[j] += row.v[j];
    }
  });
  rs_walk_backward(key, k, sh, [&](long long p, K kk, long long e) {
    const uint32_t cl = cell[p];
    if ((int64_t)cl < n) add(e + (kk >= K0 ? z : 0), btab[cl]);
  });
  const RankWalkZero zero = rs_walk_fold(mine, z, tsh, &below, &zeros);
  const long long a0 = 2 * zero.below + zero.t0 - m;
  if (t == 0) tie[g] = zero.tie;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    if (j < q) {                                      // (q is the workgroup's: the barriers are met by all or none)
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
        const long long na0 = -a0, B = fsb[0];
        const U128 x = u128_add({flo[0], fhi[0]}, {(unsigned long long)na0 * (unsigned long long)B,
                                                  (unsigned long long)__mul64hi(na0, B)});
        s_lo[(int64_t)j * G + g] = x.lo;
        s_hi[(int64_t)j * G + g] = (long long)x.hi;
      }
      __syncthreads();
    }
  }
}

}  // namespace

// The columns' ranks: tiles of whole columns within the budget, each a segment of n entries in a table of the dense form's
// shape; sorted by the same passes, then k_rc_keyrank writes btab and the tie terms.  With `lvl8` (cna_gene_rank_corr_by)
// the passes end on the level and the ranks are those inside it.  Declared in rank_corr.h: expr_rankperm.hip calls it once
// per group of 16 columns, each with a table and tie slots of its own.
int rankcorr_keys(cna_ctx* c, ExprState* s, RankSumWork* w, int q, int stride, int64_t work_bytes, int64_t m,
                  const uint8_t* lvl8, int32_t* btab, unsigned long long* tie_lo, unsigned int* tie_hi, const char* who) {
  const int64_t n = s->n;
  std::vector<int64_t> seg_h, gchunk_h;
  SortTable tb;
  SortTiles ts;
  CNA_TRY(dense_table(c, s, w, n, q, seg_h, gchunk_h, &tb));
  const int64_t per_entry = 2 * (int64_t)(sizeof(uint64_t) + sizeof(uint32_t));
  CNA_TRY(rs_tiles(seg_h, gchunk_h, q, per_entry, work_bytes, who, "columns", &ts));
  CNA_TRY((rs_sort_bufs<uint64_t, uint32_t>(c, s, w, ts.entries, ts.chunks, ts.segs)));
  uint64_t *ka = w->keyA.as<uint64_t>(), *kb = w->keyB.as<uint64_t>();
  uint32_t *pa = w->lvlA.as<uint32_t>(), *pb = w->lvlB.as<uint32_t>();
  for (const GeneTile& t : ts.tiles) {                // its "genes" are the columns [g0, g1)
    const int k0 = (int)t.g0;
    const unsigned cols = (unsigned)(t.g1 - t.g0);
    {
      ProfScope ps(c, CNA_K_RANKSUM_KEYS, s->st);
      hipLaunchKernelGGL(k_rc_vkeys, dim3((unsigned)((n + 255) / 256), cols), dim3(256), 0, s->st,
                         w->vcol.as<const double>(), n, k0, w->sort.codes(), ka, pa);
    }
    {
      ProfScope ps(c, CNA_K_RANKSUM_SORT, s->st);
      rs_passes<uint64_t, uint32_t>(s->st, tb, t.c0, t.nch, t.g0, cols, seg_h[(size_t)t.g0], ka, pa, kb, pb,
                                    w->cnt.as<unsigned int>(), w->dbase.as<unsigned int>(), lvl8);
    }
    ProfScope ps(c, CNA_K_RANKCORR_KEYS, s->st);
    const dim3 grid((unsigned)((m + 255) / 256), cols);
    if (m > 0 && lvl8)
      hipLaunchKernelGGL(k_rc_keyrank<true>, grid, dim3(256), 0, s->st, (const uint64_t*)kb, (const uint32_t*)pb, n, k0,
                         (long long)m, stride, btab, tie_lo, tie_hi, lvl8, w->dbase.as<const unsigned int>());
    else if (m > 0)
      hipLaunchKernelGGL(k_rc_keyrank<false>, grid, dim3(256), 0, s->st, (const uint64_t*)ka, (const uint32_t*)pa, n, k0,
                         (long long)m, stride, btab, tie_lo, tie_hi, (const uint8_t*)nullptr,
                         (const unsigned int*)nullptr);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

namespace {

template <typename T>
int rankcorr_run(cna_ctx* c, ExprState* s, RankSumWork* w, int q, int64_t work_bytes, int64_t m, int n_bins, const uint8_t* lvl8,
                 const char* who) {
  using K = typename KeyOf<T>::K;
  const int64_t G = s->G, n = s->n;
  int rc = 0;
  with_width(q, [&](auto width) {
    constexpr int W = decltype(width)::value;
    rc = ranksum_sorted<T, uint32_t>(
        c, s, w, work_bytes, m, who,
        [&](const GeneTile& t, int64_t base, const K* key, const uint32_t* cell, const int64_t* seg) {
          ProfScope ps(c, CNA_K_RANKCORR_CORR, s->st);
          const auto launch = [&](auto src) {
            hipLaunchKernelGGL((k_rc_corr<K, W, decltype(src)>), dim3((unsigned)(t.g1 - t.g0), (unsigned)n_bins), dim3(RS_UNIT), 0,
                               s->st, key, cell, seg, base, t.g0, G, src, n, q, w->btab.as<const BRow<W>>(),
                               w->slo.as<unsigned long long>(), w->shi.as<long long>(), w->tie.as<double>());
          };
          if (lvl8) launch(GeneLevel{w->dbase.as<const unsigned int>(), w->vm.as<const unsigned long long>()});
          else launch(WholeGene{w->kept.as<const unsigned int>(), (long long)m});
        },
        lvl8);
  });
  return rc;
}

// What cna_gene_rank_corr and cna_gene_rank_corr_by share behind their argument checks.  `codes` null: one level of all
// cells (n_bins = 1), the whole-gene kernels; else the levels, judged before anything is written.  Outputs per level:
// s_lo, s_hi [n_bins, q, G], tie_gene [n_bins, G], tie_key [n_bins, q], m_out [n_bins].
int rankcorr_entry(cna_ctx* c, ExprState* s, const char* who, const double* V, int q, const int32_t* codes, int n_bins,
                   int64_t work_bytes, uint64_t* s_lo, int64_t* s_hi, double* tie_gene, double* tie_key, int64_t* m_out,
                   uint8_t* nan_out) {
  const int64_t G = s->G, n = s->n;
  const bool by = codes != nullptr;
  int stride = 1;
  with_width(q, [&](auto width) { stride = decltype(width)::value; });
  RankSumWork* w = expr_work<RankSumWork>(s, EXPR_RANKSUM);
  if (by) CNA_TRY(sort_count(c, s->st, w->sort, CellListOf<256>{}, codes, n, n_bins, 0, 2,
                             (std::string(who) + ": a code lies outside [-1, n_bins)").c_str()));
  const int64_t tie_bytes = 12 * RC_MAX_KEYS * (int64_t)n_bins;   // per (level, column) 64 low bits, then 32 high bits, of its tie term
  const int64_t s_bytes = 8 * (int64_t)n_bins * q * G, t_bytes = 8 * (int64_t)n_bins * G;
  CNA_TRY(buf_need(c, s->st, w->vcol, 8 * (int64_t)q * n));
  CNA_TRY(buf_need(c, s->st, w->sort.code, 4 * n));
  CNA_TRY(buf_need(c, s->st, w->vm, 8 * 256));
  CNA_TRY(buf_need(c, s->st, w->btab, 4 * (int64_t)stride * n));
  CNA_TRY(buf_need(c, s->st, w->tiek, tie_bytes));
  if (by) CNA_TRY(buf_need(c, s->st, w->lvl8, n));
  CNA_TRY(result_bufs_need(c, s->st, {{&w->slo, s_bytes}, {&w->shi, s_bytes}, {&w->tie, t_bytes}}));
  const uint8_t* lvl8 = by ? w->lvl8.as<const uint8_t>() : nullptr;
  std::vector<unsigned long long> mlev((size_t)n_bins);
  {
    // the kept cells: every column finite.  The rows of btab of the other cells, and its columns from q on, are never
    // meant: zero, so that what the gather reads of them is defined
    ProfScope ps(c, CNA_K_RANKCORR_KEYS, s->st);
    HIP_TRY(hipMemcpyAsync(w->vcol.p, V, (size_t)(8 * (int64_t)q * n), hipMemcpyHostToDevice, s->st));
    HIP_TRY(hipMemsetAsync(w->vm.p, 0, 8 * 256, s->st));
    HIP_TRY(hipMemsetAsync(w->tiek.p, 0, (size_t)tie_bytes, s->st));
    HIP_TRY(hipMemsetAsync(w->btab.p, 0, (size_t)(4 * (int64_t)stride * n), s->st));
    const dim3 grid((unsigned)((n + 255) / 256));
    with_bool(by, [&](auto levels) {
      hipLaunchKernelGGL(k_rc_mask<decltype(levels)::value>, grid, dim3(256), 0, s->st, w->vcol.as<const double>(), q, n,
                         w->sort.code.as<int32_t>(), by ? w->lvl8.as<uint8_t>() : nullptr, w->vm.as<unsigned long long>());
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mlev.data(), w->vm.p, 8 * (size_t)n_bins, hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));             // the caller has its columns back
  }
  int64_t m = 0;
  for (int b = 0; b < n_bins; ++b) m += (int64_t)mlev[(size_t)b];
  CNA_TRY(rankcorr_keys(c, s, w, q, stride, work_bytes, m, lvl8, w->btab.as<int32_t>(), w->tiek.as<unsigned long long>(),
                        w->tiek.as<unsigned int>() + 2 * RC_MAX_KEYS * n_bins, who));
  if (s->is_f64) CNA_TRY(rankcorr_run<double>(c, s, w, q, work_bytes, m, n_bins, lvl8, who));
  else CNA_TRY(rankcorr_run<float>(c, s, w, q, work_bytes, m, n_bins, lvl8, who));
  std::vector<unsigned int> nanf((size_t)G);
  std::vector<unsigned long long> tie_words((size_t)(tie_bytes / 8));
  {
    ProfScope ps(c, CNA_K_RANKSUM_FETCH, s->st);
    CNA_TRY(fetch_results(s->st, who, {{s_lo, w->slo.p, (size_t)s_bytes},
                                       {s_hi, w->shi.p, (size_t)s_bytes},
                                       {tie_gene, w->tie.p, (size_t)t_bytes},
                                       {tie_words.data(), w->tiek.p, (size_t)tie_bytes},
                                       {nanf.data(), w->nanf.p, (size_t)(4 * G)}}));
  }
  for (int64_t g = 0; g < G; ++g) nan_out[g] = nanf[(size_t)g] ? 1 : 0;
  const unsigned int* tie_high = reinterpret_cast<const unsigned int*>(tie_words.data() + RC_MAX_KEYS * n_bins);
  for (int b = 0; b < n_bins; ++b) {
    for (int k = 0; k < q; ++k)                       // rounded once
      tie_key[b * q + k] = (double)tie_high[b * RC_MAX_KEYS + k] * 18446744073709551616.0 + (double)tie_words[(size_t)(b * RC_MAX_KEYS + k)];
    m_out[b] = (int64_t)mlev[(size_t)b];
  }
  return 0;
}

}  // namespace

extern "C" int cna_gene_rank_corr(cna_ctx* c, const double* V, int q, int64_t work_bytes, uint64_t* s_lo, int64_t* s_hi,
                                  double* tie_gene, double* tie_key, int64_t* m_out, uint8_t* nan_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_rank_corr: no expression matrix is resident (cna_expr_upload_*)");
  if (!V || !s_lo || !s_hi || !tie_gene || !tie_key || !m_out || !nan_out) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr: null pointer");
  if (q < 1 || q > RC_MAX_KEYS) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr: 1 <= q <= 16");
  if (work_bytes < 0) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr: work_bytes is 0 (the default) or a number of bytes");
  return rankcorr_entry(c, s, "cna_gene_rank_corr", V, q, nullptr, 1, work_bytes, s_lo, s_hi, tie_gene, tie_key, m_out, nan_out);
}

extern "C" int cna_gene_rank_corr_by(cna_ctx* c, const double* V, int q, const int32_t* codes, int n_bins, int64_t work_bytes,
                                     uint64_t* s_lo, int64_t* s_hi, double* tie_gene, double* tie_key, int64_t* m_out,
                                     uint8_t* nan_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_rank_corr_by: no expression matrix is resident (cna_expr_upload_*)");
  if (!V || !codes || !s_lo || !s_hi || !tie_gene || !tie_key || !m_out || !nan_out)
    CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_by: null pointer");
  if (q < 1 || q > RC_MAX_KEYS) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_by: 1 <= q <= 16");
  if (n_bins < 1 || n_bins > RC_MAX_LEVELS) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_by: 1 <= n_bins <= 255");
  if (work_bytes < 0) CNA_FAIL(CNA_EINVAL, "cna_gene_rank_corr_by: work_bytes is 0 (the default) or a number of bytes");
  return rankcorr_entry(c, s, "cna_gene_rank_corr_by", V, q, codes, n_bins, work_bytes, s_lo, s_hi, tie_gene, tie_key, m_out, nan_out);
}
