// cna_gene_ranksum_by: twice the Wilcoxon rank sum of every level of a clustering against all other kept cells, for every
// gene of the resident expression matrix, with the tie term of its normal approximation (cna.tl.gene_markers).  One ranking
// of the kept cells per gene serves every level: the level's rank sum is the sum of those global midranks over its cells.
// All results are integers (the tie term a double that holds one), so the device path is tested for equality.
//
//   sort_count (expr.h)   checks every code against [-1, n_bins) before anything is written; the sizes of the levels
//   ranksum_sorted (rank_sort.h)
//                         the genes' lists sorted by value, the level of an entry's cell (uint16_t) as its payload
//   k_rs_rank             behind it, one workgroup per gene: the walks of rank_sort.h give less = s and lesseq = e of every
//                         entry.  The implicit zeros of the gene-major form, z = m - kept stored entries, join the run of
//                         the stored zeros by arithmetic: entries above it move up by z, and every level gets (its cells -
//                         its stored entries) times the zero group's 2 x midrank.  Per-level sums are integer LDS atomics
//                         (exact, so their order is immaterial)
//
// cna_gene_ranksum_pairs: one level against another (cna.tl.gene_markers_pairs) from the same sort -- order within the union
// of two levels is the order within all kept cells.
//   k_rs_pairs            behind the sort, one workgroup per gene, forward only: per-level prefix counts of the unit from
//                         wave ballots, so that every tie run knows its cells per level and those below it; 2 U and the tie
//                         term of every unordered pair of at most 64 levels in integer accumulators in LDS (stated at the
//                         kernel)
//
// cna_gene_ranksum_within: every level against the rest INSIDE every block of a second column (samples, batches) and the
// blocks folded with the caller's weights -- van Elteren's stratified rank-sum test (cna.tl.gene_markers_within) -- from
// one sort with the cell as the payload and one more pass on the block of the entry's cell (rank_sort.h: `lvl8`).
//   k_rs_within           behind that sort, one workgroup per gene: k_rs_rank's arithmetic on the sub-list of each block in
//                         turn, then one thread per level folds the block into the level's integer sum and its two weighted
//                         float64 sums, in block order and without FMA contraction
#include "rank_sort.h"
#include <cmath>

namespace {

constexpr int RS_MAX_LEVELS = 1024;
constexpr int RP_MAX_LEVELS = 64;              // cna_gene_ranksum_pairs: levels that take part,
constexpr int RP_SLOTS = 2016;                 // their unordered pairs (the accumulators in LDS) and
constexpr int RP_MAX_PAIRS = 2016;             // the pairs of one call
constexpr int RP_BIG = 16;                     // a tie run of this many entries is added by the whole workgroup
constexpr int RP_BIG_MOST = RS_UNIT / RP_BIG + 1;   // such runs that can end in one unit: one from before, the rest inside
constexpr int RW_MAX_BLOCKS = 255;             // cna_gene_ranksum_within: the block is a digit of the sort, 255 = left out
static_assert(RP_SLOTS == RP_MAX_LEVELS * (RP_MAX_LEVELS - 1) / 2, "one slot per unordered pair of levels");
using CellList = CellListOf<RS_MAX_LEVELS>;

// ------------------------------------------------------------------ ranks
// workgroup = gene g0 + blockIdx.x over its kept[g] sorted entries; nlev[b]: cells of level b; m: kept cells
template <typename K>
__global__ __launch_bounds__(RS_UNIT) void k_rs_rank(const K* __restrict__ key, const uint16_t* __restrict__ lvl,
                                                     const int64_t* __restrict__ seg, int64_t base, int64_t g0, int64_t G,
                                                     const unsigned int* __restrict__ kept, const int64_t* __restrict__ nlev,
                                                     int64_t m, int n_bins, long long* __restrict__ rank2,
                                                     double* __restrict__ tie) {
  constexpr K K0 = rs_key_zero<K>();
  __shared__ unsigned long long sum[RS_MAX_LEVELS];
  __shared__ unsigned int stored[RS_MAX_LEVELS];
  __shared__ long long sh[RS_UNIT];
  __shared__ double tsh[RS_UNIT];
  __shared__ unsigned int below, zeros;
  const int t = threadIdx.x;
  const int64_t g = g0 + blockIdx.x;
  const long long k = (long long)kept[g], z = (long long)m - k;
  key += seg[g] - base;
  lvl += seg[g] - base;
  for (int b = t; b < n_bins; b += RS_UNIT) {
    sum[b] = 0;
    stored[b] = 0;
  }
  if (t == 0) below = zeros = 0;
  __syncthreads();
  RankWalkMine mine;
  rs_walk_forward(key, k, sh, mine, [&](long long p, K kk, long long s) {
    const unsigned int l = lvl[p];
    if (l < (unsigned)n_bins) {                       // (only a gene with a kept NaN can show RS_LEFT here)
      atomicAdd(&sum[l], (unsigned long long)(s + (kk > K0 ? z : 0)));
      atomicAdd(&stored[l], 1u);
    }
  });
  rs_walk_backward(key, k, sh, [&](long long p, K kk, long long e) {
    const unsigned int l = lvl[p];
    if (l < (unsigned)n_bins) atomicAdd(&sum[l], (unsigned long long)(e + (kk >= K0 ? z : 0)));
  });
  const RankWalkZero zero = rs_walk_fold(mine, z, tsh, &below, &zeros);
  if (t == 0) tie[g] = zero.tie;
  for (int b = t; b < n_bins; b += RS_UNIT) {
    const long long st = (long long)stored[b];
    rank2[(int64_t)b * G + g] = (long long)sum[b] + st + ((long long)nlev[b] - st) * (2 * zero.below + zero.t0 + 1);
  }
}

// ------------------------------------------------------------------ level against level
// the accumulators are kept per unordered pair a < b
__device__ __forceinline__ int rp_slot(int a, int b) { return b * (b - 1) / 2 + a; }

// workgroup = gene g0 + blockIdx.x over its kept[g] sorted entries, RS_UNIT at a time, forward only.  With cnt_l(p) the
// entries of level l before position p, a tie run [s, e) holds c[l] = cnt_l(e) - cnt_l(s) cells of level l above
// C[l] = cnt_l(s) of them; the thread at the run's tail adds, for the levels a that occur in it and every b > a,
//   acc_u[a, b] += c[a] (2 C[b] + c[b])          (2 U_ab, a < b; U_ba = n_a n_b - U_ab at the end)
//   acc_x[a, b] += c[a] c[b] (c[a] + c[b])       and f[a] += c[a]^3 - c[a]: sum (c[a] + c[b])^3 - (c[a] + c[b]) = f[a] + f[b] + 3 x[a, b]
// in integer LDS atomics (exact: their order is immaterial); a run of RP_BIG entries or more is handed to the whole
// workgroup instead, a slot per thread, behind a barrier (measured: one thread walking levels x levels for a run of 10 000
// cells held its workgroup for longer than the sort took).  cnt_l(p) = at[wave of p][l] + pre[l][p]: the exclusive count
// inside the wave from ballots (<= 63: a byte) on the absolute count at the wave's first entry; a run that began in an
// earlier unit finds its start counts in open_at.  The run of the stored zeros is left out of the walk: with the implicit
// zeros, nlev[l] - stored[l] per level, it is one group added at the end from the counts below it, and the groups above it
// see the implicit zeros in their C.
template <typename K>
__global__ __launch_bounds__(RS_UNIT) void k_rs_pairs(const K* __restrict__ key, const uint16_t* __restrict__ lvl,
                                                      const int64_t* __restrict__ seg, int64_t base, int64_t g0, int64_t G,
                                                      const unsigned int* __restrict__ kept, const int64_t* __restrict__ nlev,
                                                      int n_bins, const int32_t* __restrict__ pairs, int n_pairs,
                                                      long long* __restrict__ u2, double* __restrict__ tie) {
  constexpr K K0 = rs_key_zero<K>();
  constexpr int WAVES = RS_UNIT / 64;
  __shared__ unsigned long long acc_u[RP_SLOTS], acc_xlo[RP_SLOTS], f_lo[RP_MAX_LEVELS];
  __shared__ unsigned int acc_xhi[RP_SLOTS], f_hi[RP_MAX_LEVELS];
  __shared__ uint8_t pre[RP_MAX_LEVELS][RS_UNIT + 4];                 // column RS_UNIT stays 0: the end of the unit
  __shared__ unsigned int at[WAVES + 1][RP_MAX_LEVELS], wtot[WAVES][RP_MAX_LEVELS];
  __shared__ unsigned int open_at[RP_MAX_LEVELS], below[RP_MAX_LEVELS], upto[RP_MAX_LEVELS];   // upto: below and the stored zeros
  __shared__ unsigned int zgrp[RP_MAX_LEVELS], above[RP_MAX_LEVELS], impl[RP_MAX_LEVELS];
  __shared__ long long sh[RS_UNIT];
  __shared__ unsigned int gc[RP_MAX_LEVELS], gC[RP_MAX_LEVELS];      // c and C of the long run in hand
  __shared__ long long open_s;
  __shared__ int has_below, has_upto, big_n, big_e[RP_BIG_MOST], big_s[RP_BIG_MOST];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t g = g0 + blockIdx.x;
  const long long k = (long long)kept[g];
  key += seg[g] - base;
  lvl += seg[g] - base;
  for (int i = t; i < RP_SLOTS; i += RS_UNIT) {
    acc_u[i] = 0;
    acc_xlo[i] = 0;
    acc_xhi[i] = 0;
  }
  if (t < RP_MAX_LEVELS) {
    f_lo[t] = 0;
    f_hi[t] = 0;
    pre[t][RS_UNIT] = 0;
    at[WAVES][t] = 0;
    open_at[t] = below[t] = upto[t] = 0;
  }
  if (t == 0) has_below = has_upto = 0;
  __syncthreads();
  const auto cnt = [&](int p, int l) -> unsigned int { return at[p >> 6][l] + pre[l][p]; };   // p in [0, RS_UNIT]
  long long carry = 0;
  for (long long u0 = 0; u0 < k; u0 += RS_UNIT) {
    const long long p = u0 + t;
    const bool valid = p < k;
    K kk = 0, before = 0;
    bool head = false, tail = false;
    unsigned int lv = RS_LEFT;
    if (valid) {
      kk = key[p];
      lv = lvl[p];
      if (p > 0) before = key[p - 1];
      head = p == 0 || before != kk;
      tail = p == k - 1 || key[p + 1] != kk;
    }
    const long long s = rs_scan_max(head ? p : (t == 0 ? carry : -1), sh, false);
    carry = sh[RS_UNIT - 1];
    // the counts of this unit
    unsigned int mine = 0;
    const unsigned long long lower = (1ull << lane) - 1ull;
    for (int l = 0; l < n_bins; ++l) {
      const unsigned long long mk = __ballot(lv == (unsigned int)l);
      pre[l][t] = (uint8_t)__popcll(mk & lower);
      if (lane == l) mine = (unsigned int)__popcll(mk);
    }
    if (lane < n_bins) wtot[wv][lane] = mine;
    if (t == 0) big_n = 0;
    __syncthreads();
    if (t < n_bins) {
      unsigned int run = at[WAVES][t];                // the end of the unit before
      for (int w = 0; w < WAVES; ++w) {
        at[w][t] = run;
        run += wtot[w][t];
      }
      at[WAVES][t] = run;
    }
    __syncthreads();
    const int pl = (int)(p - u0);
    if (valid && kk >= K0 && (p == 0 || before < K0)) {               // the first entry that is not below zero
      for (int l = 0; l < n_bins; ++l) below[l] = cnt(pl, l);
      has_below = 1;
    }
    if (valid && kk > K0 && (p == 0 || before <= K0)) {               // the first entry above zero
      for (int l = 0; l < n_bins; ++l) upto[l] = cnt(pl, l);
      has_upto = 1;
    }
    if (valid && tail && kk != K0) {
      const long long r = p + 1 - s;
      if (r == 1) {                                                   // a run of one: c[a] = 1, nothing for the tie term
        for (int b = (int)lv + 1; b < n_bins; ++b) {
          const unsigned int Cb = cnt(pl, b);
          if (Cb) atomicAdd(&acc_u[rp_slot((int)lv, b)], 2ull * Cb);
        }
      } else if (r >= RP_BIG) {                                       // for everybody, below
        const int i = atomicAdd(&big_n, 1);
        big_e[i] = pl + 1;
        big_s[i] = s >= u0 ? (int)(s - u0) : -1;
      } else {
        const bool here = s >= u0;
        const int sl = here ? (int)(s - u0) : 0;
        unsigned long long present = 0;                               // the levels of its few entries, as a mask
        for (long long j = s; j <= p; ++j) {
          const unsigned int l = lvl[j];
          if (l < (unsigned int)n_bins) present |= 1ull << l;         // (only a gene with a kept NaN can show RS_LEFT here)
        }
        for (unsigned long long todo = present; todo; todo &= todo - 1ull) {
          const int a = __ffsll((long long)todo) - 1;
          const unsigned long long ca = cnt(pl + 1, a) - (here ? cnt(sl, a) : open_at[a]);
          rp_add128(&f_lo[a], &f_hi[a], rp_tie_term(ca));
          for (int b = a + 1; b < n_bins; ++b) {
            const unsigned int Cb = here ? cnt(sl, b) : open_at[b];
            const unsigned long long cb = (present >> b & 1ull) ? cnt(pl + 1, b) - Cb : 0ull;
            const unsigned long long add = ca * (2ull * Cb + cb);
            if (add) atomicAdd(&acc_u[rp_slot(a, b)], add);
            if (cb) rp_add128(&acc_xlo[rp_slot(a, b)], &acc_xhi[rp_slot(a, b)], u128_mul(ca * cb, ca + cb));
          }
        }
      }
    }
    if (t == RS_UNIT - 1) open_s = valid && !tail && s >= u0 ? s : -1;   // a run that starts here and goes on
    __syncthreads();
    // the long runs that end in this unit, one after the other (in any order: the sums are integers), a slot per thread;
    // nobody else adds meanwhile, so these are plain adds
    for (int i = 0, nb = big_n; i < nb; ++i) {
      if (t < n_bins) {
        const unsigned int Cs = big_s[i] >= 0 ? cnt(big_s[i], t) : open_at[t];
        gC[t] = Cs;
        gc[t] = cnt(big_e[i], t) - Cs;
      }
      __syncthreads();
      if (t < n_bins) {
        const U128 f = u128_add({f_lo[t], (unsigned long long)f_hi[t]}, rp_tie_term(gc[t]));
        f_lo[t] = f.lo;
        f_hi[t] = (unsigned int)f.hi;
      }
      for (int j = t; j < RP_MAX_LEVELS * RP_MAX_LEVELS; j += RS_UNIT) {
        const int a = j / RP_MAX_LEVELS, b = j % RP_MAX_LEVELS;
        if (a >= b || b >= n_bins) continue;
        const unsigned long long ca = gc[a], cb = gc[b];
        if (!ca) continue;
        const int q = rp_slot(a, b);
        acc_u[q] += ca * (2ull * gC[b] + cb);
        if (cb) {
          const U128 x = u128_add({acc_xlo[q], (unsigned long long)acc_xhi[q]}, u128_mul(ca * cb, ca + cb));
          acc_xlo[q] = x.lo;
          acc_xhi[q] = (unsigned int)x.hi;
        }
      }
      __syncthreads();
    }
    if (t < n_bins && open_s >= 0) open_at[t] = cnt((int)(open_s - u0), t);
    __syncthreads();                                  // pre, at and sh are read before the next unit writes them
  }
  // the zero group and the shift of the groups above it
  if (t < n_bins) {
    const unsigned int st = at[WAVES][t];             // the stored entries of the level
    const unsigned int up = has_upto ? upto[t] : st;
    const unsigned int bl = has_below ? below[t] : up;
    const long long im = (long long)nlev[t] - (long long)st;
    below[t] = bl;
    impl[t] = im > 0 ? (unsigned int)im : 0u;        // (only a gene with a kept NaN can show less)
    zgrp[t] = up - bl + impl[t];
    above[t] = st - up;
    const U128 f = u128_add({f_lo[t], (unsigned long long)f_hi[t]}, rp_tie_term(zgrp[t]));
    f_lo[t] = f.lo;
    f_hi[t] = (unsigned int)f.hi;
  }
  __syncthreads();
  for (int i = t; i < n_bins * n_bins; i += RS_UNIT) {
    const int a = i / n_bins, b = i % n_bins;
    if (a >= b) continue;
    const int q = rp_slot(a, b);
    const unsigned long long ca = zgrp[a], cb = zgrp[b];
    acc_u[q] += ca * (2ull * below[b] + cb) + 2ull * above[a] * impl[b];
    const U128 x = u128_add({acc_xlo[q], (unsigned long long)acc_xhi[q]}, u128_mul(ca * cb, ca + cb));
    acc_xlo[q] = x.lo;
    acc_xhi[q] = (unsigned int)x.hi;
  }
  __syncthreads();
  for (int j = t; j < n_pairs; j += RS_UNIT) {
    const int a = pairs[2 * j], b = pairs[2 * j + 1];
    const int q = a < b ? rp_slot(a, b) : rp_slot(b, a);
    const long long uab = (long long)acc_u[q];
    u2[(int64_t)j * G + g] = a < b ? uab : 2ll * (long long)nlev[a] * (long long)nlev[b] - uab;
    const U128 x = {acc_xlo[q], (unsigned long long)acc_xhi[q]};
    const U128 tt = u128_add(u128_add({f_lo[a], (unsigned long long)f_hi[a]}, {f_lo[b], (unsigned long long)f_hi[b]}),
                             u128_add(x, u128_add(x, x)));
    tie[(int64_t)j * G + g] = (double)tt.hi * 18446744073709551616.0 + (double)tt.lo;
  }
}

// ------------------------------------------------------------------ level against the rest inside every block
// The operands of k_rs_within that do not depend on the gene, one upload (WithinTables::bytes): the weights of the tie
// terms [block][level] and of the rank sums [block], the kept cells per (block, level) and per block.
struct WithinTables {
  const double *w_tie, *w_num;
  const unsigned int *nsl, *ns;
  static int64_t bytes(int n_blocks, int n_bins) { return (8 + 4) * ((int64_t)n_blocks * n_bins + n_blocks); }
  static WithinTables at(void* p, int n_blocks, int n_bins) {
    const int64_t cells = (int64_t)n_blocks * n_bins;
    const double* d = static_cast<const double*>(p);
    const unsigned int* u = reinterpret_cast<const unsigned int*>(d + cells + n_blocks);
    return {d, d + cells, u, u + cells};
  }
};

// acc + w x with the product and the sum rounded one after the other, as a numpy loop rounds them.  hipcc contracts
// a * b + c into an FMA by default, and through __dmul_rn / __dadd_rn as well (plain operators in its headers: measured,
// the sums came out one and two ulps off), so contraction is switched off for these two operations
__device__ __forceinline__ double rw_mul_then_add(double acc, double w, double x) {
#pragma clang fp contract(off)
  const double p = w * x;
  return acc + p;
}

// workgroup = gene g0 + blockIdx.x, behind the sort's pass on the block of the entry's cell: the gene's list is block-major
// and sorted by value inside a block, block s in the positions [dbase[s], dbase[s + 1]) of its segment.  The blocks are
// taken in order, each with k_rs_rank's arithmetic on its sub-list -- k stored kept entries among the n_s kept cells of the
// block, z = n_s - k implicit zeros, the level of an entry read from codes[its cell] -- so that level b has twice its rank
// sum inside the block and D = that - n_sb (n_s + 1).  Behind a block thread b (and b + RS_UNIT, ...) folds level b into
// its accumulators: one thread per level and the blocks in order fix the order of the float adds, and the products and
// sums are rounded one by one (rw_mul_then_add), which is what a numpy loop over the blocks does.  A block in which the gene is constant -- its zero group holds all n_s cells, or it stores
// them all in one run -- counts for no level's `live`.
// LDS: 40 bytes per level behind the kernel's own 4 KB (the scans), sized by the launch: 44 KB at 1024 levels, three
// workgroups to a CU; 5.3 KB at 32 levels, where the 256 threads' registers and not the LDS bound the occupancy.
template <typename K>
__global__ __launch_bounds__(RS_UNIT) void k_rs_within(const K* __restrict__ key, const uint32_t* __restrict__ cell,
                                                       const int64_t* __restrict__ seg, int64_t base, int64_t g0, int64_t G,
                                                       const unsigned int* __restrict__ dbase, const int32_t* __restrict__ codes,
                                                       int64_t n, WithinTables tab, int n_bins, int n_blocks,
                                                       long long* __restrict__ d2_out, double* __restrict__ num_out,
                                                       double* __restrict__ tiew_out, int* __restrict__ live_out) {
  constexpr K K0 = rs_key_zero<K>();
  extern __shared__ unsigned long long within_lds[];
  unsigned long long* sum = within_lds;                                       // [n_bins] each, the 8-byte arrays first
  long long* d2 = reinterpret_cast<long long*>(sum + n_bins);
  double* num = reinterpret_cast<double*>(d2 + n_bins);
  double* tiew = num + n_bins;
  unsigned int* stored = reinterpret_cast<unsigned int*>(tiew + n_bins);
  int* live = reinterpret_cast<int*>(stored + n_bins);
  __shared__ long long sh[RS_UNIT];
  __shared__ double tsh[RS_UNIT];
  __shared__ unsigned int below, zeros;
  const int t = threadIdx.x;
  const int64_t g = g0 + blockIdx.x;
  key += seg[g] - base;
  cell += seg[g] - base;
  dbase += (int64_t)blockIdx.x * 256;
  for (int b = t; b < n_bins; b += RS_UNIT) {
    d2[b] = 0;
    num[b] = 0.0;
    tiew[b] = 0.0;
    live[b] = 0;
  }
  for (int s = 0; s < n_blocks; ++s) {
    const long long at = (long long)dbase[s], k = (long long)dbase[s + 1] - at;
    const long long cells = (long long)tab.ns[s], z = cells - k;
    const K* bkey = key + at;
    const uint32_t* bcell = cell + at;
    for (int b = t; b < n_bins; b += RS_UNIT) {
      sum[b] = 0;
      stored[b] = 0;
    }
    if (t == 0) below = zeros = 0;
    __syncthreads();
    RankWalkMine mine;
    rs_walk_forward(bkey, k, sh, mine, [&](long long p, K kk, long long ps) {
      const uint32_t cl = bcell[p];
      const unsigned int l = (int64_t)cl < n ? (unsigned int)codes[cl] : ~0u;   // (a block's entries are kept cells')
      if (l < (unsigned)n_bins) {
        atomicAdd(&sum[l], (unsigned long long)(ps + (kk > K0 ? z : 0)));
        atomicAdd(&stored[l], 1u);
      }
    });
    rs_walk_backward(bkey, k, sh, [&](long long p, K kk, long long pe) {
      const uint32_t cl = bcell[p];
      const unsigned int l = (int64_t)cl < n ? (unsigned int)codes[cl] : ~0u;
      if (l < (unsigned)n_bins) atomicAdd(&sum[l], (unsigned long long)(pe + (kk >= K0 ? z : 0)));
    });
    const RankWalkZero zero = rs_walk_fold(mine, z, tsh, &below, &zeros);
    const bool constant = zero.t0 == cells || (z == 0 && k > 0 && bkey[0] == bkey[k - 1]);
    const double wn = tab.w_num[s];
    for (int b = t; b < n_bins; b += RS_UNIT) {
      const long long st = (long long)stored[b], nl = (long long)tab.nsl[(int64_t)s * n_bins + b];
      const long long rank2 = (long long)sum[b] + st + (nl - st) * (2 * zero.below + zero.t0 + 1);
      const long long D = rank2 - nl * (cells + 1);
      d2[b] += D;
      num[b] = rw_mul_then_add(num[b], wn, (double)D);
      tiew[b] = rw_mul_then_add(tiew[b], tab.w_tie[(int64_t)s * n_bins + b], zero.tie);
      if (nl > 0 && nl < cells && !constant) ++live[b];
    }
    __syncthreads();                                  // sum, stored, below and zeros are read before the next block resets them
  }
  for (int b = t; b < n_bins; b += RS_UNIT) {         // (its own accumulators: no barrier is needed)
    d2_out[(int64_t)b * G + g] = d2[b];
    num_out[(int64_t)b * G + g] = num[b];
    tiew_out[(int64_t)b * G + g] = tiew[b];
    live_out[(int64_t)b * G + g] = live[b];
  }
}

template <typename T>
int within_run(cna_ctx* c, ExprState* s, RankSumWork* w, int n_bins, int n_blocks, int64_t work_bytes, int64_t m) {
  using K = typename KeyOf<T>::K;
  const int64_t G = s->G;
  const WithinTables tab = WithinTables::at(w->wtab.p, n_blocks, n_bins);
  return ranksum_sorted<T, uint32_t>(
      c, s, w, work_bytes, m, "cna_gene_ranksum_within",
      [&](const GeneTile& t, int64_t base, const K* key, const uint32_t* cell, const int64_t* seg) {
        ProfScope ps(c, CNA_K_RANKSUM_RANK, s->st);
        hipLaunchKernelGGL(k_rs_within<K>, dim3((unsigned)(t.g1 - t.g0)), dim3(RS_UNIT), (size_t)(40 * n_bins), s->st, key, cell,
                           seg, base, t.g0, G, w->dbase.as<const unsigned int>(), w->sort.codes(), s->n, tab, n_bins, n_blocks,
                           w->wd2.as<long long>(), w->wnum.as<double>(), w->wtiew.as<double>(), w->wlive.as<int>());
      },
      w->lvl8.as<const uint8_t>());
}

template <typename T>
int ranksum_run(cna_ctx* c, ExprState* s, RankSumWork* w, int n_bins, int64_t work_bytes, int64_t m) {
  using K = typename KeyOf<T>::K;
  const int64_t G = s->G;
  CNA_TRY(buf_need(c, s->st, w->rank2, 8 * (int64_t)n_bins * G));
  CNA_TRY(buf_need(c, s->st, w->tie, 8 * G));
  return ranksum_sorted<T, uint16_t>(c, s, w, work_bytes, m, "cna_gene_ranksum_by",
                           [&](const GeneTile& t, int64_t base, const K* key, const uint16_t* lvl, const int64_t* seg) {
                             ProfScope ps(c, CNA_K_RANKSUM_RANK, s->st);
                             hipLaunchKernelGGL(k_rs_rank<K>, dim3((unsigned)(t.g1 - t.g0)), dim3(RS_UNIT), 0, s->st, key, lvl, seg,
                                                base, t.g0, G, w->kept.as<const unsigned int>(), w->sort.tot.as<const int64_t>(),
                                                m, n_bins, w->rank2.as<long long>(), w->tie.as<double>());
                           });
}

template <typename T>
int pairs_run(cna_ctx* c, ExprState* s, RankSumWork* w, int n_bins, int n_pairs, int64_t work_bytes, int64_t m) {
  using K = typename KeyOf<T>::K;
  const int64_t G = s->G;
  return ranksum_sorted<T, uint16_t>(c, s, w, work_bytes, m, "cna_gene_ranksum_pairs",
                           [&](const GeneTile& t, int64_t base, const K* key, const uint16_t* lvl, const int64_t* seg) {
                             ProfScope ps(c, CNA_K_RANKSUM_PAIRS, s->st);
                             hipLaunchKernelGGL(k_rs_pairs<K>, dim3((unsigned)(t.g1 - t.g0)), dim3(RS_UNIT), 0, s->st, key, lvl, seg,
                                                base, t.g0, G, w->kept.as<const unsigned int>(), w->sort.tot.as<const int64_t>(),
                                                n_bins, w->pairs.as<const int32_t>(), n_pairs, w->u2.as<long long>(),
                                                w->ptie.as<double>());
                           });
}

// What the two entries share around their kernels, behind their argument checks.  Before: the codes are judged before
// anything is written, and the sizes of the levels with their sum m, the kept cells.  `run(m)` grows what it needs and
// queues the work.  After: the two results, the genes with a kept NaN and the sizes of the levels.
struct RankSumOut {
  void* dst;
  const Buf* src;                                    // (grown by `run`)
  int64_t bytes;
};
template <class Run>
int ranksum_entry(cna_ctx* c, ExprState* s, RankSumWork* w, const char* who, const int32_t* codes, int n_bins, Run&& run,
                  RankSumOut a, RankSumOut b, int64_t* n_out, uint8_t* nan_out) {
  const int64_t G = s->G;
  CNA_TRY(sort_count(c, s->st, w->sort, CellList{}, codes, s->n, n_bins, 0, 2,
                     (std::string(who) + ": a code lies outside [-1, n_bins)").c_str()));
  int64_t m = 0;
  for (int l = 0; l < n_bins; ++l) m += w->sort.tot_h[(size_t)l];
  CNA_TRY(run(m));
  std::vector<unsigned int> nanf((size_t)G);
  {
    ProfScope ps(c, CNA_K_RANKSUM_FETCH, s->st);
    CNA_TRY(fetch_results(s->st, who, {{a.dst, a.src->p, (size_t)a.bytes},
                                       {b.dst, b.src->p, (size_t)b.bytes},
                                       {nanf.data(), w->nanf.p, (size_t)(4 * G)}}));
  }
  for (int64_t g = 0; g < G; ++g) nan_out[g] = nanf[(size_t)g] ? 1 : 0;
  for (int l = 0; l < n_bins; ++l) n_out[l] = w->sort.tot_h[(size_t)l];
  return 0;
}

}  // namespace

extern "C" int cna_gene_ranksum_by(cna_ctx* c, const int32_t* codes, int n_bins, int64_t work_bytes, int64_t* rank2_out,
                                   double* tie_out, int64_t* n_out, uint8_t* nan_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_ranksum_by: no expression matrix is resident (cna_expr_upload_*)");
  if (!codes || !rank2_out || !tie_out || !n_out || !nan_out) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_by: null pointer");
  if (n_bins < 1 || n_bins > RS_MAX_LEVELS) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_by: 1 <= n_bins <= 1024");
  if (work_bytes < 0) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_by: work_bytes is 0 (the default) or a number of bytes");
  RankSumWork* w = expr_work<RankSumWork>(s, EXPR_RANKSUM);
  return ranksum_entry(
      c, s, w, "cna_gene_ranksum_by", codes, n_bins,
      [&](int64_t m) {
        return s->is_f64 ? ranksum_run<double>(c, s, w, n_bins, work_bytes, m) : ranksum_run<float>(c, s, w, n_bins, work_bytes, m);
      },
      {rank2_out, &w->rank2, 8 * (int64_t)n_bins * s->G}, {tie_out, &w->tie, 8 * s->G}, n_out, nan_out);
}

// The codes are judged on the host here: the kept cells are an intersection of two columns and the table of their sizes has
// up to 255 x 1024 cells, more than sort_count's counters in LDS hold; the caller's host has made the same pass over the
// cells for its weights.
extern "C" int cna_gene_ranksum_within(cna_ctx* c, const int32_t* codes, int n_bins, const int32_t* blocks, int n_blocks,
                                       const double* w_num, const double* w_tie, int64_t work_bytes, int64_t* d2_out,
                                       double* num_out, double* tiew_out, int32_t* live_out, int64_t* n_out, uint8_t* nan_out) {
  CHECK_CTX(c);
  const char* who = "cna_gene_ranksum_within";
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_ranksum_within: no expression matrix is resident (cna_expr_upload_*)");
  if (!codes || !blocks || !w_num || !w_tie || !d2_out || !num_out || !tiew_out || !live_out || !n_out || !nan_out)
    CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_within: null pointer");
  if (n_bins < 1 || n_bins > RS_MAX_LEVELS) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_within: 1 <= n_bins <= 1024");
  if (n_blocks < 1 || n_blocks > RW_MAX_BLOCKS) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_within: 1 <= n_blocks <= 255");
  if (work_bytes < 0) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_within: work_bytes is 0 (the default) or a number of bytes");
  const int64_t n = s->n, G = s->G, cells = (int64_t)n_blocks * n_bins;
  for (int64_t j = 0; j < cells + n_blocks; ++j)
    if (!std::isfinite(j < cells ? w_tie[j] : w_num[j - cells])) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_within: a weight is not finite");
  // the kept cells: a level and a block.  lev[i] = the level or -1, blk8[i] = the block or 255: the digit of the sort's last pass
  std::vector<int32_t> lev((size_t)n);
  std::vector<uint8_t> blk8((size_t)n);
  std::vector<int64_t> nsl((size_t)cells, 0);
  int64_t m = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t cd = codes[i], bl = blocks[i];
    if (cd < -1 || cd >= n_bins) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_within: a level code lies outside [-1, n_bins)");
    if (bl < -1 || bl >= n_blocks) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_within: a block code lies outside [-1, n_blocks)");
    const bool keep = cd >= 0 && bl >= 0;
    lev[(size_t)i] = keep ? cd : -1;
    blk8[(size_t)i] = keep ? (uint8_t)bl : (uint8_t)255;
    if (keep) {
      ++nsl[(size_t)bl * n_bins + cd];
      ++m;
    }
  }
  std::vector<unsigned char> tables((size_t)WithinTables::bytes(n_blocks, n_bins));
  {
    double* d = reinterpret_cast<double*>(tables.data());
    unsigned int* u = reinterpret_cast<unsigned int*>(d + cells + n_blocks);
    std::copy(w_tie, w_tie + cells, d);
    std::copy(w_num, w_num + n_blocks, d + cells);
    for (int b = 0; b < n_blocks; ++b) {
      int64_t ns = 0;
      for (int l = 0; l < n_bins; ++l) {
        u[(int64_t)b * n_bins + l] = (unsigned int)nsl[(size_t)b * n_bins + l];
        ns += nsl[(size_t)b * n_bins + l];
      }
      u[cells + b] = (unsigned int)ns;
    }
  }
  RankSumWork* w = expr_work<RankSumWork>(s, EXPR_RANKSUM);
  const int64_t out_count = (int64_t)n_bins * G;
  CNA_TRY(result_bufs_need(c, s->st, {{&w->wd2, 8 * out_count}, {&w->wnum, 8 * out_count}, {&w->wtiew, 8 * out_count},
                                      {&w->wlive, 4 * out_count}}));
  CNA_TRY(buf_need(c, s->st, w->sort.code, 4 * n));
  CNA_TRY(buf_need(c, s->st, w->lvl8, n));
  CNA_TRY(buf_need(c, s->st, w->wtab, (int64_t)tables.size()));
  HIP_TRY(hipMemcpyAsync(w->sort.code.p, lev.data(), (size_t)(4 * n), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemcpyAsync(w->lvl8.p, blk8.data(), (size_t)n, hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemcpyAsync(w->wtab.p, tables.data(), tables.size(), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));               // (the host vectors may go; the sort's own setup waits here anyway)
  if (s->is_f64) CNA_TRY(within_run<double>(c, s, w, n_bins, n_blocks, work_bytes, m));
  else CNA_TRY(within_run<float>(c, s, w, n_bins, n_blocks, work_bytes, m));
  std::vector<unsigned int> nanf((size_t)G);
  {
    ProfScope ps(c, CNA_K_RANKSUM_FETCH, s->st);
    CNA_TRY(fetch_results(s->st, who, {{d2_out, w->wd2.p, (size_t)(8 * out_count)},
                                       {num_out, w->wnum.p, (size_t)(8 * out_count)},
                                       {tiew_out, w->wtiew.p, (size_t)(8 * out_count)},
                                       {live_out, w->wlive.p, (size_t)(4 * out_count)},
                                       {nanf.data(), w->nanf.p, (size_t)(4 * G)}}));
  }
  for (int64_t g = 0; g < G; ++g) nan_out[g] = nanf[(size_t)g] ? 1 : 0;
  for (int64_t j = 0; j < cells; ++j) n_out[j] = nsl[(size_t)j];
  return 0;
}

extern "C" int cna_gene_ranksum_pairs(cna_ctx* c, const int32_t* codes, int n_bins, const int32_t* pairs, int n_pairs,
                                      int64_t work_bytes, int64_t* u2_out, double* tie_out, int64_t* n_out, uint8_t* nan_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_ranksum_pairs: no expression matrix is resident (cna_expr_upload_*)");
  if (!codes || !pairs || !u2_out || !tie_out || !n_out || !nan_out) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_pairs: null pointer");
  if (n_bins < 1 || n_bins > RP_MAX_LEVELS) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_pairs: 1 <= n_bins <= 64");
  if (n_pairs < 1 || n_pairs > RP_MAX_PAIRS) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_pairs: 1 <= n_pairs <= 2016");
  if (work_bytes < 0) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_pairs: work_bytes is 0 (the default) or a number of bytes");
  for (int j = 0; j < n_pairs; ++j) {
    const int32_t a = pairs[2 * j], b = pairs[2 * j + 1];
    if (a < 0 || a >= n_bins || b < 0 || b >= n_bins)
      CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_pairs: a pair names a level outside [0, n_bins)");
    if (a == b) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_pairs: a pair of one level with itself");
  }
  const int64_t out_count = (int64_t)n_pairs * s->G;
  RankSumWork* w = expr_work<RankSumWork>(s, EXPR_RANKSUM);
  return ranksum_entry(
      c, s, w, "cna_gene_ranksum_pairs", codes, n_bins,
      [&](int64_t m) {
        CNA_TRY(result_bufs_need(c, s->st, {{&w->u2, 8 * out_count}, {&w->ptie, 8 * out_count}}));
        CNA_TRY(buf_need(c, s->st, w->pairs, 8 * (int64_t)n_pairs));
        // (ranksum_sorted waits for the stream before the caller has its list back)
        HIP_TRY(hipMemcpyAsync(w->pairs.p, pairs, (size_t)(8 * n_pairs), hipMemcpyHostToDevice, s->st));
        return s->is_f64 ? pairs_run<double>(c, s, w, n_bins, n_pairs, work_bytes, m)
                         : pairs_run<float>(c, s, w, n_bins, n_pairs, work_bytes, m);
      },
      {u2_out, &w->u2, 8 * out_count}, {tie_out, &w->ptie, 8 * out_count}, n_out, nan_out);
}
