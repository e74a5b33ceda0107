// cna_gene_ranksum_by: twice the Wilcoxon rank sum of every level of a clustering against all other kept cells, for every
// gene of the resident expression matrix, with the tie term of its normal approximation (cna.tl.gene_markers).  One ranking
// of the kept cells per gene serves every level: the level's rank sum is the sum of those global midranks over its cells.
// All results are integers (the tie term a double that holds one), so the device path is tested for equality.
//
//   sort_count (expr.h)   checks every code against [-1, n_bins) before anything is written; the sizes of the levels
//   k_rs_keys_sparse      one workgroup per chunk of a gene's list: every entry -> an order-preserving unsigned key (-0.0
//                         and a stored zero = the key of +0.0; float64 on all 64 bits) and the level of its cell.  An entry
//                         of a left-out cell gets the largest key and the level RS_LEFT: it sorts behind the kept ones and
//                         the rank kernel never reads it.  Counts the kept entries of the gene, flags a kept NaN
//   k_rs_keys_dense       a 64 x 64 tile of cells x genes through LDS into the same gene-major form: every kept cell is
//                         present in every gene (so its kept count is m), a left-out cell rides along as above
//   k_rs_count / k_rs_scan / k_rs_scatter
//                         a stable LSD radix sort segmented by gene, 8 bits per pass (float32: 4 passes, float64: 8), on the
//                         chunk tables of build_chunks (dense: a table of the same shape with chunks of RS_DENSE_CHUNK): a
//                         count per (chunk, digit) in LDS; per gene a scan over its chunks and then over the digits; one wave
//                         per chunk scatters, lanes with the same digit ranked by lane (k_sort_fill's rule, by ballots), the
//                         cursors carried from batch to batch: the result does not depend on scheduling
//   k_rs_rank             one workgroup per gene walks the sorted list in units of RS_UNIT entries, forward for the start s
//                         of every entry's tie run (a prefix maximum over the run heads, carried across units) and backward
//                         for its end e (a suffix minimum over the run tails): less = s, lesseq = e.  The implicit zeros of
//                         the gene-major form, z = m - kept stored entries, join the run of the stored zeros by arithmetic:
//                         entries above it move up by z, and every level gets (its cells - its stored entries) times the
//                         zero group's 2 x midrank.  Per-level sums are integer LDS atomics (exact, so their order is
//                         immaterial); the tie terms t^3 - t are added per thread in list order and folded by a fixed tree
//
// cna_gene_ranksum_pairs: one level against another (cna.tl.gene_markers_pairs) from the same sort -- order within the union
// of two levels is the order within all kept cells.  ranksum_sorted is the part both entries share (tiles, keys, passes);
//   k_rs_pairs            behind it, one workgroup per gene, forward only: per-level prefix counts of the unit from wave
//                         ballots, so that every tie run knows its cells per level and those below it; 2 U and the tie term
//                         of every unordered pair of at most 64 levels in integer accumulators in LDS (stated at the kernel)
//
// cna_gene_rank_corr: Spearman's rank correlation of every gene with up to 16 per-cell columns (cna.tl.gene_rank_corr), as
// exact integers.  The payload of the sort is a template parameter: the level of the entry's cell (uint16_t, the two entries
// above, bit for bit what they were) or the cell itself (uint32_t); rs_passes is the part of the sort that knows a chunk
// table and nothing of the resident matrix, so the columns are ranked by the same passes.
//   k_rc_mask             the kept cells (every column finite) as the codes ranksum_sorted expects, and their number m
//   k_rc_vkeys            the columns as q segments of n entries {float64 key, cell} in a table of the dense form's shape
//   k_rc_keyrank          behind their sort, one thread per kept entry: its tie run [s, e), by binary search where a neighbour
//                         ties -> b = s + e - m (twice the midrank less m + 1) into the cell-major table btab[cell][W]; the
//                         column's tie term in integers
//   k_rc_corr             behind the genes' sort, one workgroup per gene: a = s + e - m of every entry by the forward and
//                         backward walks of k_rs_rank, the cell's row of btab gathered in each, sum a b per column in 96-bit
//                         integer registers, the implicit zeros by arithmetic; the two limbs of S and the gene's tie term
// (forward / backward and not the single forward walk of k_rs_pairs: a = (s - m) + e is linear, so each walk adds its own
// half with the coefficient it has in hand and nothing about an open run is carried from unit to unit but its start; the
// price is the second gather of the row, which comes from the same table in reverse order)
//
// cna_gene_rank_corr_by: the same inside every level of a clustering (cna.tl.gene_rank_corr_strata), from one sort.  The
// kept cells keep their level (k_rc_mask<true>: the level as a byte per cell, the kept cells per level); behind the value
// passes one more stable pass takes that byte as its digit (DigitOfLevel; 255: a left-out entry), so a gene's list, and a
// column's segment, is level-major and sorted by value inside a level, and the scan of that pass (dbase) says where every
// (segment, level) begins.  k_rc_keyrank<true> keeps its searches inside the level's range and k_rc_corr runs once per
// (gene, level) on the sub-segment (GeneLevel) with the level's m_l, k_l and z_l: level l is cna_gene_rank_corr on columns
// set to NaN outside l, integer for integer.  The pass count is odd: the sorted lists are in the other buffer of each pair.
//
// The genes go in tiles of whole genes whose keys, payloads and their ping-pong copies stay within work_bytes (0:
// RS_WORK_BYTES); a gene that alone exceeds it is one tile.  The counters of the sort (1 KB per chunk) come on top.
#include "expr.h"

namespace {

constexpr int RS_MAX_LEVELS = 1024;
constexpr int64_t RS_WORK_BYTES = 1ll << 30;   // keys + levels + their copies of one tile, when the caller names no budget
constexpr int64_t RS_DENSE_CHUNK = 1024;       // cells of one gene per sort chunk of the dense form (build_chunks' least)
constexpr int RS_UNIT = 256;                   // entries of a gene's sorted list the rank kernel takes at a time
constexpr int RS_TILE = 64;                    // the dense gather's square tile
constexpr uint16_t RS_LEFT = 0xffff;           // "level" of an entry whose cell is left out (rs_left<uint16_t>())
constexpr int RC_MAX_KEYS = 16;                // cna_gene_rank_corr: per-cell columns of one call
constexpr int RC_MAX_LEVELS = 255;             // cna_gene_rank_corr_by: the level is a digit of the sort, 255 = left out
constexpr int RP_MAX_LEVELS = 64;              // cna_gene_ranksum_pairs: levels that take part,
constexpr int RP_SLOTS = 2016;                 // their unordered pairs (the accumulators in LDS) and
constexpr int RP_MAX_PAIRS = 2016;             // the pairs of one call
constexpr int RP_BIG = 16;                     // a tie run of this many entries is added by the whole workgroup
constexpr int RP_BIG_MOST = RS_UNIT / RP_BIG + 1;   // such runs that can end in one unit: one from before, the rest inside
static_assert(RP_SLOTS == RP_MAX_LEVELS * (RP_MAX_LEVELS - 1) / 2, "one slot per unordered pair of levels");
using CellList = CellListOf<RS_MAX_LEVELS>;

struct RankSumWork : BufSet {
  CodeSort sort{*this};
  Buf keyA{*this}, keyB{*this}, lvlA{*this}, lvlB{*this}, cnt{*this}, dbase{*this}, kept{*this}, nanf{*this}, rank2{*this},
      tie{*this};
  Buf pairs{*this}, u2{*this}, ptie{*this};                            // cna_gene_ranksum_pairs: its pairs and results
  Buf seg{*this}, chunk_lo{*this}, chunk_gene{*this}, gchunk{*this};   // the dense form's table (the lists have the state's)
  // cna_gene_rank_corr: the columns, the kept cells' count, b[cell][W], the columns' tie terms (96 bits), the two limbs of S
  Buf vcol{*this}, vm{*this}, btab{*this}, tiek{*this}, slo{*this}, shi{*this};
  Buf lvl8{*this};                                                     // cna_gene_rank_corr_by: the kept cell's level as a byte
};

// What an entry carries through the sort beside its key: the level of its cell (uint16_t: the rank sums) or the cell
// itself (uint32_t: cna_gene_rank_corr).  All ones: the cell is left out.
template <typename P>
constexpr P rs_left() { return (P) ~(P)0; }
template <typename P>
__device__ __forceinline__ P rs_payload(int64_t cell, int32_t code) {
  if constexpr (sizeof(P) == 2) return (P)code;
  else return (P)cell;
}
static_assert(rs_left<uint16_t>() == RS_LEFT, "the rank and pairs kernels compare with RS_LEFT");

// a chunk table on the device: segment g holds the entries [seg[g], seg[g + 1]) in the chunks [gchunk[g], gchunk[g + 1])
struct SortTable {
  const int64_t *seg, *chunk_lo, *gchunk;
  const int32_t* chunk_gene;
  int64_t chunk_len;
};

// ------------------------------------------------------------------ keys
// value -> unsigned key in the order of the values; bits alone decide: denormals stay apart whatever the float mode
template <typename T>
struct KeyOf;
template <>
struct KeyOf<float> {
  using K = uint32_t;
  static constexpr K SIGN = 0x80000000u, MAG = 0x7fffffffu, INF = 0x7f800000u;
  __device__ static K bits(float x) { return __float_as_uint(x); }
};
template <>
struct KeyOf<double> {
  using K = uint64_t;
  static constexpr K SIGN = 0x8000000000000000ull, MAG = 0x7fffffffffffffffull, INF = 0x7ff0000000000000ull;
  __device__ static K bits(double x) { return (K)__double_as_longlong(x); }
};
template <typename T>
__device__ __forceinline__ typename KeyOf<T>::K rs_key(T x, bool* is_nan) {
  using P = KeyOf<T>;
  typename P::K b = P::bits(x);
  *is_nan = (b & P::MAG) > P::INF;
  if ((b & P::MAG) == 0) b = 0;                         // -0.0 is +0.0
  return (b & P::SIGN) ? ~b : (b | P::SIGN);
}

// workgroup = chunk c0 + blockIdx.x of the gene lists; tile arrays are indexed by entry - base
template <typename T, typename P>
__global__ __launch_bounds__(256) void k_rs_keys_sparse(const int64_t* __restrict__ chunk_lo, const int32_t* __restrict__ chunk_gene,
                                                        const int64_t* __restrict__ gptr, int64_t c0, int64_t chunk_len,
                                                        const int32_t* __restrict__ gcell, const T* __restrict__ gval,
                                                        const int32_t* __restrict__ codes, int64_t base,
                                                        typename KeyOf<T>::K* __restrict__ key, P* __restrict__ lvl,
                                                        unsigned int* __restrict__ kept, unsigned int* __restrict__ nanf) {
  using K = typename KeyOf<T>::K;
  const int64_t ch = c0 + blockIdx.x;
  const int32_t g = chunk_gene[ch];
  const int64_t lo = chunk_lo[ch], end = gptr[g + 1];
  const int64_t hi = lo + chunk_len < end ? lo + chunk_len : end;
  unsigned int mine = 0;
  bool seen_nan = false;
  for (int64_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
    const int32_t cell = gcell[e], cd = codes[cell];
    K k = ~(K)0;
    P l = rs_left<P>();
    if (cd >= 0) {
      bool is_nan;
      k = rs_key<T>(gval[e], &is_nan);
      l = rs_payload<P>(cell, cd);
      seen_nan = seen_nan || is_nan;
      ++mine;
    }
    key[e - base] = k;
    lvl[e - base] = l;
  }
  __shared__ unsigned int tot;
  if (threadIdx.x == 0) tot = 0;
  __syncthreads();
  if (mine) atomicAdd(&tot, mine);
  if (seen_nan) nanf[g] = 1u;
  __syncthreads();
  if (threadIdx.x == 0 && tot) atomicAdd(&kept[g], tot);
}

// workgroup = RS_TILE cells x RS_TILE genes of the tile [g0, g1): X[cell][gene] in, entry (gene * n + cell) - base out
template <typename T, typename P>
__global__ __launch_bounds__(256) void k_rs_keys_dense(const T* __restrict__ X, int64_t n, int64_t G, int64_t g0, int64_t g1,
                                                       const int32_t* __restrict__ codes, int64_t base,
                                                       typename KeyOf<T>::K* __restrict__ key, P* __restrict__ lvl,
                                                       unsigned int* __restrict__ nanf) {
  using K = typename KeyOf<T>::K;
  __shared__ K tk[RS_TILE][RS_TILE + 1];
  __shared__ P tl[RS_TILE];
  const int tx = threadIdx.x % RS_TILE, ty = threadIdx.x / RS_TILE;
  const int64_t cell0 = (int64_t)blockIdx.x * RS_TILE, gene0 = g0 + (int64_t)blockIdx.y * RS_TILE;
  if (threadIdx.x < RS_TILE) {
    const int64_t i = cell0 + threadIdx.x;
    const int32_t cd = i < n ? codes[i] : -1;
    tl[threadIdx.x] = cd >= 0 ? rs_payload<P>(i, cd) : rs_left<P>();
  }
  __syncthreads();
  for (int r = ty; r < RS_TILE; r += 256 / RS_TILE) {
    const int64_t i = cell0 + r, g = gene0 + tx;
    K k = ~(K)0;
    if (i < n && g < g1 && tl[r] != rs_left<P>()) {
      bool is_nan;
      k = rs_key<T>(X[i * G + g], &is_nan);
      if (is_nan) nanf[g] = 1u;
    }
    tk[r][tx] = k;
  }
  __syncthreads();
  for (int r = ty; r < RS_TILE; r += 256 / RS_TILE) {
    const int64_t g = gene0 + r, i = cell0 + tx;
    if (g < g1 && i < n) {
      key[g * n + i - base] = tk[tx][r];
      lvl[g * n + i - base] = tl[tx];
    }
  }
}

// ------------------------------------------------------------------ the sort: one pass of 8 bits
// Where a pass takes its digit from: 8 bits of the key (the value passes), or the level of the entry's cell from a byte
// per cell (the one pass behind them in cna_gene_rank_corr_by; the payload is the cell, 255 = a left-out entry).  What a
// source does not read of an entry is not loaded.
template <typename K, typename P>
struct DigitOfKey {
  int shift;
  __device__ __forceinline__ unsigned int operator()(K k, P) const { return (unsigned)(k >> shift) & 255u; }
};
template <typename K, typename P>
struct DigitOfLevel {
  const uint8_t* lvl8;
  __device__ __forceinline__ unsigned int operator()(K, P cell) const { return cell == rs_left<P>() ? 255u : (unsigned)lvl8[cell]; }
};

// cnt[chunk - c0][digit] = entries of the chunk with that digit
template <typename K, typename P, class D>
__global__ __launch_bounds__(256) void k_rs_count(const int64_t* __restrict__ chunk_lo, const int32_t* __restrict__ chunk_gene,
                                                  const int64_t* __restrict__ seg, int64_t c0, int64_t chunk_len, int64_t base,
                                                  const K* __restrict__ key, const P* __restrict__ pay, D digit,
                                                  unsigned int* __restrict__ cnt) {
  __shared__ unsigned int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t ch = c0 + blockIdx.x;
  const int64_t lo = chunk_lo[ch], end = seg[chunk_gene[ch] + 1];
  const int64_t hi = lo + chunk_len < end ? lo + chunk_len : end;
  for (int64_t e = lo + threadIdx.x; e < hi; e += blockDim.x) atomicAdd(&h[digit(key[e - base], pay[e - base])], 1u);
  __syncthreads();
  cnt[(int64_t)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

// workgroup = gene g0 + blockIdx.x, thread = digit: cnt -> the entries of the gene with that digit in the chunks before;
// dbase[gene - g0][digit] = the gene's entries with a smaller digit
__global__ __launch_bounds__(256) void k_rs_scan(const int64_t* __restrict__ gchunk, int64_t g0, int64_t c0,
                                                 unsigned int* __restrict__ cnt, unsigned int* __restrict__ dbase) {
  __shared__ unsigned int tot[256];
  const int64_t g = g0 + blockIdx.x;
  unsigned int run = 0;
  for (int64_t ch = gchunk[g] - c0; ch < gchunk[g + 1] - c0; ++ch) {
    const unsigned int t = cnt[ch * 256 + threadIdx.x];
    cnt[ch * 256 + threadIdx.x] = run;
    run += t;
  }
  tot[threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int acc = 0;
    for (int d = 0; d < 256; ++d) {
      const unsigned int t = tot[d];
      tot[d] = acc;
      acc += t;
    }
  }
  __syncthreads();
  dbase[(int64_t)blockIdx.x * 256 + threadIdx.x] = tot[threadIdx.x];
}

// one wave per chunk; cur[digit] = where the chunk's next entry with that digit goes inside the gene's segment.  In a batch
// of 64 entries the lanes with one digit find each other with 8 ballots and take consecutive places in lane order.
template <typename K, typename P, class D>
__global__ __launch_bounds__(64) void k_rs_scatter(const int64_t* __restrict__ chunk_lo, const int32_t* __restrict__ chunk_gene,
                                                   const int64_t* __restrict__ seg, int64_t c0, int64_t chunk_len, int64_t base,
                                                   int64_t g0, const K* __restrict__ kin, const P* __restrict__ lin,
                                                   K* __restrict__ kout, P* __restrict__ lout, D digit,
                                                   const unsigned int* __restrict__ cnt, const unsigned int* __restrict__ dbase) {
  __shared__ unsigned int cur[256];
  const int lane = threadIdx.x;
  const int64_t ch = c0 + blockIdx.x;
  const int32_t g = chunk_gene[ch];
  for (int d = lane; d < 256; d += 64) cur[d] = cnt[(int64_t)blockIdx.x * 256 + d] + dbase[(int64_t)(g - g0) * 256 + d];
  __syncthreads();
  const int64_t lo = chunk_lo[ch], end = seg[g + 1], at = seg[g] - base;
  const int64_t hi = lo + chunk_len < end ? lo + chunk_len : end;
  for (int64_t e0 = lo; e0 < hi; e0 += 64) {
    const int64_t e = e0 + lane;
    const bool valid = e < hi;
    K k = 0;
    P l = 0;
    if (valid) {
      k = kin[e - base];
      l = lin[e - base];
    }
    const unsigned int d = digit(k, l);               // (a lane past the end: entry 0's, and never used)
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b & 1u) != 0;
      const unsigned long long bal = __ballot(valid && bit);
      same &= bit ? bal : ~bal;
    }
    const unsigned int rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    const bool last = (same >> lane) == 1ull;
    if (valid) {
      const int64_t to = at + (int64_t)(cur[d] + rank);
      kout[to] = k;
      lout[to] = l;
    }
    __syncthreads();
    if (valid && last) cur[d] += rank + 1u;
    __syncthreads();
  }
}

// ------------------------------------------------------------------ ranks
// inclusive scan over the 256 threads: the maximum of v over the threads up to this one (rev: from this one on)
__device__ __forceinline__ long long rs_scan_max(long long v, long long* sh, bool rev) {
  const int t = rev ? RS_UNIT - 1 - (int)threadIdx.x : (int)threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < RS_UNIT; o <<= 1) {
    const long long x = t >= o ? sh[t - o] : v;
    __syncthreads();
    if (x > v) v = x;
    sh[t] = v;
    __syncthreads();
  }
  return v;
}

// workgroup = gene g0 + blockIdx.x over its kept[g] sorted entries; nlev[b]: cells of level b; m: kept cells
template <typename K>
__global__ __launch_bounds__(RS_UNIT) void k_rs_rank(const K* __restrict__ key, const uint16_t* __restrict__ lvl,
                                                     const int64_t* __restrict__ seg, int64_t base, int64_t g0, int64_t G,
                                                     const unsigned int* __restrict__ kept, const int64_t* __restrict__ nlev,
                                                     int64_t m, int n_bins, long long* __restrict__ rank2,
                                                     double* __restrict__ tie) {
  constexpr K K0 = (K)1 << (8 * sizeof(K) - 1);       // the key of +0.0
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
  // forward: s = the first entry of the run an entry lies in
  double tacc = 0.0;
  unsigned int my_below = 0, my_zeros = 0;
  long long carry = 0;
  for (long long u0 = 0; u0 < k; u0 += RS_UNIT) {
    const long long p = u0 + t;
    const bool valid = p < k;
    K kk = 0;
    bool head = false, tail = false;
    if (valid) {
      kk = key[p];
      head = p == 0 || key[p - 1] != kk;
      tail = p == k - 1 || key[p + 1] != kk;
    }
    const long long s = rs_scan_max(head ? p : (t == 0 ? carry : -1), sh, false);
    carry = sh[RS_UNIT - 1];
    if (valid) {
      const unsigned int l = lvl[p];
      if (l < (unsigned)n_bins) {                     // (only a gene with a kept NaN can show RS_LEFT here)
        atomicAdd(&sum[l], (unsigned long long)(s + (kk > K0 ? z : 0)));
        atomicAdd(&stored[l], 1u);
      }
      my_below += kk < K0 ? 1u : 0u;
      my_zeros += kk == K0 ? 1u : 0u;
      if (tail && kk != K0) {
        const long long r = p + 1 - s;
        tacc += (double)r * (double)(r * r - 1);
      }
    }
    __syncthreads();                                  // sh is read (carry) before the next scan writes it
  }
  // backward: e = one past the last entry of the run
  carry = 0;
  for (long long u0 = k > 0 ? (k - 1) / RS_UNIT * RS_UNIT : -1; u0 >= 0; u0 -= RS_UNIT) {
    const long long p = u0 + t;
    const bool valid = p < k;
    K kk = 0;
    bool tail = false;
    if (valid) {
      kk = key[p];
      tail = p == k - 1 || key[p + 1] != kk;
    }
    // the minimum of the run ends from here on, as a maximum of their negatives; the last thread of a full unit carries
    const long long none = -0x7fffffffffffffffll;
    const long long e = -rs_scan_max(tail ? -(p + 1) : (valid && t == RS_UNIT - 1 ? carry : none), sh, true);
    carry = sh[RS_UNIT - 1];                          // reversed index: thread 0's value, negated as it is used
    if (valid) {
      const unsigned int l = lvl[p];
      if (l < (unsigned)n_bins) atomicAdd(&sum[l], (unsigned long long)(e + (kk >= K0 ? z : 0)));
    }
    __syncthreads();
  }
  if (my_below) atomicAdd(&below, my_below);
  if (my_zeros) atomicAdd(&zeros, my_zeros);
  tsh[t] = tacc;
  __syncthreads();
  for (int w = RS_UNIT / 2; w > 0; w >>= 1) {
    if (t < w) tsh[t] += tsh[t + w];
    __syncthreads();
  }
  const long long t0 = (long long)zeros + z;          // the zero group: stored and implicit zeros
  if (t == 0) tie[g] = tsh[0] + (t0 > 0 ? (double)t0 * (double)(t0 * t0 - 1) : 0.0);
  for (int b = t; b < n_bins; b += RS_UNIT) {
    const long long st = (long long)stored[b];
    rank2[(int64_t)b * G + g] = (long long)sum[b] + st + ((long long)nlev[b] - st) * (2 * (long long)below + t0 + 1);
  }
}

// ------------------------------------------------------------------ level against level
// 128-bit sums as {low 64 bits, what lies above}: a tie term t^3 - t of up to 2^31 cells passes 2^64
struct U128 {
  unsigned long long lo, hi;
};
__device__ __forceinline__ U128 u128_mul(unsigned long long a, unsigned long long b) { return {a * b, __umul64hi(a, b)}; }
__device__ __forceinline__ U128 u128_add(U128 a, U128 b) {
  const unsigned long long lo = a.lo + b.lo;
  return {lo, a.hi + b.hi + (lo < a.lo ? 1ull : 0ull)};
}
__device__ __forceinline__ U128 rp_tie_term(unsigned long long t) { return t ? u128_mul(t * t - 1ull, t) : U128{0ull, 0ull}; }
// an exact, commutative add in LDS: the carry out of the low word is that of this add in whatever order the adds land
__device__ __forceinline__ void rp_add128(unsigned long long* lo, unsigned int* hi, U128 x) {
  if (!(x.lo | x.hi)) return;
  const unsigned long long old = atomicAdd(lo, x.lo);
  const unsigned int up = (unsigned int)x.hi + (old + x.lo < old ? 1u : 0u);
  if (up) atomicAdd(hi, up);
}
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
  constexpr K K0 = (K)1 << (8 * sizeof(K) - 1);       // the key of +0.0
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

// ------------------------------------------------------------------ rank correlation (cna_gene_rank_corr)
// With r the midrank over the m kept cells, a_i = 2 r_gene(i) - (m + 1) and b_i = 2 r_column(i) - (m + 1) are integers
// that sum to 0 over the kept cells, and a tie run [s, e) of a sorted list gives each of its entries s + e - m.
//   S[k, g] = sum over the kept cells of a_i b_i[k]      rho = 3 S / sqrt((m^3 - m - T_g) (m^3 - m - T_k))   (the host's line)
// |S| <= (m^3 - m) / 3 passes 2^63 from 3 024 617 cells on, so S is summed and returned in 128 bits.

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
// binary search (a column is one segment of up to 2^31 entries: one workgroup walking it, as k_rs_rank walks a gene, took
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

// one cell's row of btab: W columns (the least of 1, 2, 4, 8, 16 that holds q), one aligned load
template <int W>
struct alignas(4 * W) BRow {
  int32_t v[W];
};

// workgroup = gene g0 + blockIdx.x over its kept[g] sorted entries {key, cell}.  a_i = s + e - m splits into a walk forward
// (s - m, in [-m, 0)) and one backward (e, in [1, m]), found as in k_rs_rank and with its shifts by the z implicit zeros;
// each walk gathers the entry's row and adds coefficient x b[k] -- a product below 2^62 in absolute value -- into the
// thread's sum for column k: 64 low bits and a 32-bit count of carries less borrows (|sum| < 2^93 whatever the order).  The
// forward walk also sums b: the implicit zeros are one group with a_0 = 2 below + t0 - m, and because b sums to 0 over the
// kept cells their share is -a_0 x (sum of b over the stored kept entries), one 64 x 64 -> 128-bit product at the end.
// The threads' sums are folded by a fixed tree (integers: exact in any order).  Registers: W x (2 + 1 + 2) for the sums
// and W for the row, 96 of them at W = 16.
//
// What the workgroup walks is its source's to say -- where the list begins inside the gene's segment, its k stored kept
// entries and the m cells they are ranked among: the gene's whole list (cna_gene_rank_corr) or, behind the sort's pass on
// the level, the sub-segment of level blockIdx.y (cna_gene_rank_corr_by: k_l, m_l, z_l = m_l - k_l; a run cannot cross a
// level because the list is one level's, and b sums to 0 over the level's kept cells, so the zero group's share holds).
// Results go to [level][column][gene] and [level][gene].
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

template <typename K, int W, class Src>
__global__ __launch_bounds__(RS_UNIT) void k_rc_corr(const K* __restrict__ key, const uint32_t* __restrict__ cell,
                                                     const int64_t* __restrict__ seg, int64_t base, int64_t g0, int64_t G,
                                                     Src src, int64_t n, int q,
                                                     const BRow<W>* __restrict__ btab, unsigned long long* __restrict__ s_lo,
                                                     long long* __restrict__ s_hi, double* __restrict__ tie) {
  constexpr K K0 = (K)1 << (8 * sizeof(K) - 1);       // the key of +0.0
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
  for (int j = 0; j < W; ++j) {
    lo[j] = 0;
    hi[j] = 0;
    sb[j] = 0;
  }
  const auto add = [&](long long coef, const BRow<W>& row) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const long long x = coef * (long long)row.v[j];
      const unsigned long long old = lo[j];
      lo[j] = old + (unsigned long long)x;
      hi[j] += (lo[j] < old ? 1 : 0) - (x < 0 ? 1 : 0);
    }
  };
  double tacc = 0.0;
  unsigned int my_below = 0, my_zeros = 0;
  long long carry = 0;
  for (long long u0 = 0; u0 < k; u0 += RS_UNIT) {
    const long long p = u0 + t;
    const bool valid = p < k;
    K kk = 0;
    bool head = false, tail = false;
    if (valid) {
      kk = key[p];
      head = p == 0 || key[p - 1] != kk;
      tail = p == k - 1 || key[p + 1] != kk;
    }
    const long long s = rs_scan_max(head ? p : (t == 0 ? carry : -1), sh, false);
    carry = sh[RS_UNIT - 1];
    if (valid) {
      const uint32_t cl = cell[p];
      if ((int64_t)cl < n) {                          // (only a gene with a kept NaN can show a left-out entry here)
        const BRow<W> row = btab[cl];
        add(s + (kk > K0 ? z : 0) - m, row);
#pragma unroll
        for (int j = 0; j < W; ++j) sb[j] += row.v[j];
      }
      my_below += kk < K0 ? 1u : 0u;
      my_zeros += kk == K0 ? 1u : 0u;
      if (tail && kk != K0) {
        const long long r = p + 1 - s;
        tacc += (double)r * (double)(r * r - 1);
      }
    }
    __syncthreads();                                  // sh is read (carry) before the next scan writes it
  }
  carry = 0;
  for (long long u0 = k > 0 ? (k - 1) / RS_UNIT * RS_UNIT : -1; u0 >= 0; u0 -= RS_UNIT) {
    const long long p = u0 + t;
    const bool valid = p < k;
    K kk = 0;
    bool tail = false;
    if (valid) {
      kk = key[p];
      tail = p == k - 1 || key[p + 1] != kk;
    }
    const long long none = -0x7fffffffffffffffll;
    const long long e = -rs_scan_max(tail ? -(p + 1) : (valid && t == RS_UNIT - 1 ? carry : none), sh, true);
    carry = sh[RS_UNIT - 1];
    if (valid) {
      const uint32_t cl = cell[p];
      if ((int64_t)cl < n) add(e + (kk >= K0 ? z : 0), btab[cl]);
    }
    __syncthreads();
  }
  if (my_below) atomicAdd(&below, my_below);
  if (my_zeros) atomicAdd(&zeros, my_zeros);
  tsh[t] = tacc;
  __syncthreads();
  for (int w = RS_UNIT / 2; w > 0; w >>= 1) {
    if (t < w) tsh[t] += tsh[t + w];
    __syncthreads();
  }
  const long long t0 = (long long)zeros + z;          // the zero group: stored and implicit zeros
  const long long a0 = 2 * (long long)below + t0 - m;
  if (t == 0) tie[g] = tsh[0] + (t0 > 0 ? (double)t0 * (double)(t0 * t0 - 1) : 0.0);
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

// a chunk table of the lists' shape for `segs` segments of `len` entries each (the dense form: a gene holds the entries
// [g n, (g + 1) n); the columns of cna_gene_rank_corr: q segments of n cells)
int dense_table(cna_ctx* c, ExprState* s, RankSumWork* w, int64_t len, int64_t segs, std::vector<int64_t>& seg_h,
                std::vector<int64_t>& gchunk_h, SortTable* tb) {
  const int64_t per = (len + RS_DENSE_CHUNK - 1) / RS_DENSE_CHUNK;
  std::vector<int64_t> lo((size_t)(segs * per));
  std::vector<int32_t> gene((size_t)(segs * per));
  seg_h.resize((size_t)segs + 1);
  gchunk_h.resize((size_t)segs + 1);
  for (int64_t g = 0; g <= segs; ++g) {
    seg_h[(size_t)g] = g * len;
    gchunk_h[(size_t)g] = g * per;
  }
  for (int64_t g = 0; g < segs; ++g)
    for (int64_t j = 0; j < per; ++j) {
      lo[(size_t)(g * per + j)] = g * len + j * RS_DENSE_CHUNK;
      gene[(size_t)(g * per + j)] = (int32_t)g;
    }
  CNA_TRY(buf_need(c, s->st, w->seg, 8 * (segs + 1)));
  CNA_TRY(buf_need(c, s->st, w->gchunk, 8 * (segs + 1)));
  CNA_TRY(buf_need(c, s->st, w->chunk_lo, 8 * segs * per));
  CNA_TRY(buf_need(c, s->st, w->chunk_gene, 4 * segs * per));
  HIP_TRY(hipMemcpyAsync(w->seg.p, seg_h.data(), 8 * (size_t)(segs + 1), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemcpyAsync(w->gchunk.p, gchunk_h.data(), 8 * (size_t)(segs + 1), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemcpyAsync(w->chunk_lo.p, lo.data(), 8 * lo.size(), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemcpyAsync(w->chunk_gene.p, gene.data(), 4 * gene.size(), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));               // the host vectors end with this scope
  *tb = {w->seg.as<const int64_t>(), w->chunk_lo.as<const int64_t>(), w->gchunk.as<const int64_t>(),
         w->chunk_gene.as<const int32_t>(), RS_DENSE_CHUNK};
  return 0;
}

// The radix passes over the chunks [c0, c0 + nch) of the segments [g0, g0 + genes) of a table, whose entries begin at
// `base`: an even number of value passes, so the sorted {key, payload} are in (ka, pa) again.  With `lvl8` (the payload is
// the cell) one more stable pass on the level of the entry's cell: every segment is then level-major and sorted by value
// inside a level, in (kb, pb), the entries of the left-out cells last, and dbase[segment - g0][l] is where level l begins
// inside the segment (so dbase[..][l + 1] is where it ends: l <= 254)
template <typename K, typename P, class D>
void rs_pass(hipStream_t st, const SortTable& tb, int64_t c0, int64_t nch, int64_t g0, unsigned genes, int64_t base, const K* ka,
             const P* pa, K* kb, P* pb, D digit, unsigned int* cnt, unsigned int* dbase) {
  hipLaunchKernelGGL((k_rs_count<K, P, D>), dim3((unsigned)nch), dim3(256), 0, st, tb.chunk_lo, tb.chunk_gene, tb.seg, c0,
                     tb.chunk_len, base, ka, pa, digit, cnt);
  hipLaunchKernelGGL(k_rs_scan, dim3(genes), dim3(256), 0, st, tb.gchunk, g0, c0, cnt, dbase);
  hipLaunchKernelGGL((k_rs_scatter<K, P, D>), dim3((unsigned)nch), dim3(64), 0, st, tb.chunk_lo, tb.chunk_gene, tb.seg, c0,
                     tb.chunk_len, base, g0, ka, pa, kb, pb, digit, (const unsigned int*)cnt, (const unsigned int*)dbase);
}
template <typename K, typename P>
void rs_passes(hipStream_t st, const SortTable& tb, int64_t c0, int64_t nch, int64_t g0, unsigned genes, int64_t base, K* ka,
               P* pa, K* kb, P* pb, unsigned int* cnt, unsigned int* dbase, const uint8_t* lvl8 = nullptr) {
  static_assert(sizeof(K) % 2 == 0, "the result of the value passes is to land where the keys were");
  for (int pass = 0; pass < (int)sizeof(K); ++pass) {
    rs_pass(st, tb, c0, nch, g0, genes, base, (const K*)ka, (const P*)pa, kb, pb, DigitOfKey<K, P>{8 * pass}, cnt, dbase);
    std::swap(ka, kb);
    std::swap(pa, pb);
  }
  if constexpr (sizeof(P) == 4) {
    if (lvl8) rs_pass(st, tb, c0, nch, g0, genes, base, (const K*)ka, (const P*)pa, kb, pb, DigitOfLevel<K, P>{lvl8}, cnt, dbase);
  }
}

// the sort's buffers for tiles of at most `entries` entries in `chunks` chunks of `genes` segments
template <typename K, typename P>
int rs_sort_bufs(cna_ctx* c, ExprState* s, RankSumWork* w, int64_t entries, int64_t chunks, int64_t genes) {
  CNA_TRY(buf_need(c, s->st, w->keyA, (int64_t)sizeof(K) * entries));
  CNA_TRY(buf_need(c, s->st, w->keyB, (int64_t)sizeof(K) * entries));
  CNA_TRY(buf_need(c, s->st, w->lvlA, (int64_t)sizeof(P) * entries));
  CNA_TRY(buf_need(c, s->st, w->lvlB, (int64_t)sizeof(P) * entries));
  CNA_TRY(buf_need(c, s->st, w->cnt, 4 * 256 * chunks));
  CNA_TRY(buf_need(c, s->st, w->dbase, 4 * 256 * genes));
  return 0;
}

// Tiling, keys and the radix passes of the resident matrix, shared by the entry points: for every tile of whole genes
// `behind(tile, base, keys, payloads, seg)` queues the kernel that reads the tile's sorted lists.  P: what an entry carries
// (rs_payload); the cells with codes[i] >= 0 (w->sort.code) are kept.  `who` names the entry in what is refused.  With `lvl8`
// the lists are level-major (rs_passes) and w->dbase holds, per gene of the tile, where each level begins.
template <typename T, typename P, class Behind>
int ranksum_sorted(cna_ctx* c, ExprState* s, RankSumWork* w, int64_t work_bytes, int64_t m, const char* who, Behind&& behind,
                   const uint8_t* lvl8 = nullptr) {
  using K = typename KeyOf<T>::K;
  const int64_t n = s->n, G = s->G;
  const bool dense = s->format == 1;
  std::vector<int64_t> seg_h, gchunk_own;
  SortTable tb;
  if (dense) {
    CNA_TRY(dense_table(c, s, w, n, G, seg_h, gchunk_own, &tb));
  } else {
    seg_h.resize((size_t)G + 1);
    HIP_TRY(hipMemcpyAsync(seg_h.data(), s->gptr.p, 8 * (size_t)(G + 1), hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
    tb = {s->gptr.as<const int64_t>(), s->chunk_lo.as<const int64_t>(), s->gchunk.as<const int64_t>(),
          s->chunk_gene.as<const int32_t>(), s->chunk_len};
  }
  const std::vector<int64_t>& gchunk_h = dense ? gchunk_own : s->gchunk_h;
  // tiles of whole genes: keys, payloads and their copies within the budget
  const int64_t per_entry = 2 * (int64_t)(sizeof(K) + sizeof(P));
  const int64_t max_entries = std::max<int64_t>(1, (work_bytes > 0 ? work_bytes : RS_WORK_BYTES) / per_entry);
  std::vector<GeneTile> tiles;
  int64_t most_entries = 1, most_chunks = 1, most_genes = 1;
  for (int64_t g0 = 0, g1; g0 < G; g0 = g1) {
    g1 = g0 + 1;
    while (g1 < G && seg_h[(size_t)g1 + 1] - seg_h[(size_t)g0] <= max_entries) ++g1;
    tiles.push_back({g0, g1, gchunk_h[(size_t)g0], gchunk_h[(size_t)g1] - gchunk_h[(size_t)g0]});
    most_entries = std::max(most_entries, seg_h[(size_t)g1] - seg_h[(size_t)g0]);
    most_chunks = std::max(most_chunks, tiles.back().nch);
    most_genes = std::max(most_genes, g1 - g0);
  }
  if (most_chunks > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, std::string(who) + ": more than 2^31 - 1 chunks in one tile of genes");
  CNA_TRY((rs_sort_bufs<K, P>(c, s, w, most_entries, most_chunks, most_genes)));
  CNA_TRY(buf_need(c, s->st, w->kept, 4 * G));
  CNA_TRY(buf_need(c, s->st, w->nanf, 4 * G));
  HIP_TRY(hipMemsetAsync(w->nanf.p, 0, (size_t)(4 * G), s->st));
  if (dense) {
    std::vector<unsigned int> all((size_t)G, (unsigned int)m);    // every kept cell is present in every gene
    HIP_TRY(hipMemcpyAsync(w->kept.p, all.data(), (size_t)(4 * G), hipMemcpyHostToDevice, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
  } else {
    HIP_TRY(hipMemsetAsync(w->kept.p, 0, (size_t)(4 * G), s->st));
  }
  K *ka = w->keyA.as<K>(), *kb = w->keyB.as<K>();
  P *la = w->lvlA.as<P>(), *lb = w->lvlB.as<P>();
  unsigned int *cnt = w->cnt.as<unsigned int>(), *dbase = w->dbase.as<unsigned int>();
  for (const GeneTile& t : tiles) {
    const int64_t base = seg_h[(size_t)t.g0];
    const unsigned genes = (unsigned)(t.g1 - t.g0);
    if (t.nch) {
      {
        ProfScope ps(c, CNA_K_RANKSUM_KEYS, s->st);
        if (dense)
          hipLaunchKernelGGL((k_rs_keys_dense<T, P>), dim3((unsigned)((n + RS_TILE - 1) / RS_TILE), (genes + RS_TILE - 1) / RS_TILE),
                             dim3(256), 0, s->st, s->X.as<const T>(), n, G, t.g0, t.g1, w->sort.codes(), base, ka, la,
                             w->nanf.as<unsigned int>());
        else
          hipLaunchKernelGGL((k_rs_keys_sparse<T, P>), dim3((unsigned)t.nch), dim3(256), 0, s->st, tb.chunk_lo, tb.chunk_gene,
                             tb.seg, t.c0, tb.chunk_len, s->gcell.as<const int32_t>(), s->gval.as<const T>(), w->sort.codes(),
                             base, ka, la, w->kept.as<unsigned int>(), w->nanf.as<unsigned int>());
      }
      ProfScope ps(c, CNA_K_RANKSUM_SORT, s->st);
      rs_passes<K, P>(s->st, tb, t.c0, t.nch, t.g0, genes, base, ka, la, kb, lb, cnt, dbase, lvl8);
    } else if (lvl8) {
      HIP_TRY(hipMemsetAsync(dbase, 0, (size_t)(4 * 256) * genes, s->st));   // no entry, no pass: every level is empty
    }
    if (lvl8) behind(t, base, (const K*)kb, (const P*)lb, tb.seg);           // an odd number of passes: the other buffers
    else behind(t, base, (const K*)ka, (const P*)la, tb.seg);
  }
  HIP_TRY(hipGetLastError());
  return 0;
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

// The columns' ranks: tiles of whole columns within the budget, each a segment of n entries in a table of the dense form's
// shape; sorted by the same passes, then k_rc_keyrank writes btab and the tie terms.  With `lvl8` (cna_gene_rank_corr_by)
// the passes end on the level and the ranks are those inside it.
int rankcorr_keys(cna_ctx* c, ExprState* s, RankSumWork* w, int q, int stride, int64_t work_bytes, int64_t m, int n_bins,
                  const uint8_t* lvl8, const char* who) {
  const int64_t n = s->n, per = (n + RS_DENSE_CHUNK - 1) / RS_DENSE_CHUNK;
  const int64_t per_entry = 2 * (int64_t)(sizeof(uint64_t) + sizeof(uint32_t));
  const int64_t max_entries = std::max<int64_t>(1, (work_bytes > 0 ? work_bytes : RS_WORK_BYTES) / per_entry);
  const int cols = (int)std::min<int64_t>(q, std::max<int64_t>(1, max_entries / n));
  if (cols * per > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, std::string(who) + ": more than 2^31 - 1 chunks in one tile of columns");
  std::vector<int64_t> seg_h, gchunk_h;
  SortTable tb;
  CNA_TRY(dense_table(c, s, w, n, q, seg_h, gchunk_h, &tb));
  CNA_TRY((rs_sort_bufs<uint64_t, uint32_t>(c, s, w, cols * n, cols * per, cols)));
  uint64_t *ka = w->keyA.as<uint64_t>(), *kb = w->keyB.as<uint64_t>();
  uint32_t *pa = w->lvlA.as<uint32_t>(), *pb = w->lvlB.as<uint32_t>();
  unsigned long long* tie_lo = w->tiek.as<unsigned long long>();
  unsigned int* tie_hi = w->tiek.as<unsigned int>() + 2 * RC_MAX_KEYS * n_bins;
  for (int k0 = 0; k0 < q; k0 += cols) {
    const int k1 = std::min(q, k0 + cols);
    {
      ProfScope ps(c, CNA_K_RANKSUM_KEYS, s->st);
      hipLaunchKernelGGL(k_rc_vkeys, dim3((unsigned)((n + 255) / 256), (unsigned)(k1 - k0)), dim3(256), 0, s->st,
                         w->vcol.as<const double>(), n, k0, w->sort.codes(), ka, pa);
    }
    {
      ProfScope ps(c, CNA_K_RANKSUM_SORT, s->st);
      rs_passes<uint64_t, uint32_t>(s->st, tb, k0 * per, (k1 - k0) * per, k0, (unsigned)(k1 - k0), k0 * n, ka, pa, kb, pb,
                                    w->cnt.as<unsigned int>(), w->dbase.as<unsigned int>(), lvl8);
    }
    ProfScope ps(c, CNA_K_RANKCORR_KEYS, s->st);
    const dim3 grid((unsigned)((m + 255) / 256), (unsigned)(k1 - k0));
    if (m > 0 && lvl8)
      hipLaunchKernelGGL(k_rc_keyrank<true>, grid, dim3(256), 0, s->st, (const uint64_t*)kb, (const uint32_t*)pb, n, k0,
                         (long long)m, stride, w->btab.as<int32_t>(), tie_lo, tie_hi, lvl8, w->dbase.as<const unsigned int>());
    else if (m > 0)
      hipLaunchKernelGGL(k_rc_keyrank<false>, grid, dim3(256), 0, s->st, (const uint64_t*)ka, (const uint32_t*)pa, n, k0,
                         (long long)m, stride, w->btab.as<int32_t>(), tie_lo, tie_hi, (const uint8_t*)nullptr,
                         (const unsigned int*)nullptr);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

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
          const dim3 grid((unsigned)(t.g1 - t.g0), (unsigned)n_bins);
          if (lvl8)
            hipLaunchKernelGGL((k_rc_corr<K, W, GeneLevel>), grid, dim3(RS_UNIT), 0, s->st, key, cell, seg, base, t.g0, G,
                               GeneLevel{w->dbase.as<const unsigned int>(), w->vm.as<const unsigned long long>()}, n, q,
                               w->btab.as<const BRow<W>>(), w->slo.as<unsigned long long>(), w->shi.as<long long>(),
                               w->tie.as<double>());
          else
            hipLaunchKernelGGL((k_rc_corr<K, W, WholeGene>), grid, dim3(RS_UNIT), 0, s->st, key, cell, seg, base, t.g0, G,
                               WholeGene{w->kept.as<const unsigned int>(), (long long)m}, n, q, w->btab.as<const BRow<W>>(),
                               w->slo.as<unsigned long long>(), w->shi.as<long long>(), w->tie.as<double>());
        },
        lvl8);
  });
  return rc;
}

// What cna_gene_rank_corr and cna_gene_rank_corr_by share behind their argument checks.  `codes` null: one level of all
// cells (n_bins = 1), the whole-gene kernels, bit for bit the entry as it was; else the levels, judged before anything is
// written.  Outputs per level: s_lo, s_hi [n_bins, q, G], tie_gene [n_bins, G], tie_key [n_bins, q], m_out [n_bins].
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
  CNA_TRY(buf_need(c, s->st, w->vcol, 8 * (int64_t)q * n));
  CNA_TRY(buf_need(c, s->st, w->sort.code, 4 * n));
  CNA_TRY(buf_need(c, s->st, w->vm, 8 * 256));
  CNA_TRY(buf_need(c, s->st, w->btab, 4 * (int64_t)stride * n));
  CNA_TRY(buf_need(c, s->st, w->tiek, tie_bytes));
  if (by) CNA_TRY(buf_need(c, s->st, w->lvl8, n));
  for (Buf* b : {&w->slo, &w->shi, &w->tie}) {
    const int rc = buf_need(c, s->st, *b, 8 * (int64_t)n_bins * (b == &w->tie ? 1 : q) * G);
    if (rc == CNA_ENOMEM) (void)hipGetLastError();    // the refusal is the caller's to see, not the next launch's
    CNA_TRY(rc);
  }
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
    if (by)
      hipLaunchKernelGGL(k_rc_mask<true>, grid, dim3(256), 0, s->st, w->vcol.as<const double>(), q, n, w->sort.code.as<int32_t>(),
                         w->lvl8.as<uint8_t>(), w->vm.as<unsigned long long>());
    else
      hipLaunchKernelGGL(k_rc_mask<false>, grid, dim3(256), 0, s->st, w->vcol.as<const double>(), q, n,
                         w->sort.code.as<int32_t>(), (uint8_t*)nullptr, w->vm.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mlev.data(), w->vm.p, 8 * (size_t)n_bins, hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));             // the caller has its columns back
  }
  int64_t m = 0;
  for (int b = 0; b < n_bins; ++b) m += (int64_t)mlev[(size_t)b];
  CNA_TRY(rankcorr_keys(c, s, w, q, stride, work_bytes, m, n_bins, lvl8, who));
  if (s->is_f64) CNA_TRY(rankcorr_run<double>(c, s, w, q, work_bytes, m, n_bins, lvl8, who));
  else CNA_TRY(rankcorr_run<float>(c, s, w, q, work_bytes, m, n_bins, lvl8, who));
  std::vector<unsigned int> nanf((size_t)G);
  std::vector<unsigned long long> tie_words((size_t)(tie_bytes / 8));
  {
    ProfScope ps(c, CNA_K_RANKSUM_FETCH, s->st);
    CNA_TRY(fetch_results(s->st, who, {{s_lo, w->slo.p, (size_t)(8 * (int64_t)n_bins * q * G)},
                                       {s_hi, w->shi.p, (size_t)(8 * (int64_t)n_bins * q * G)},
                                       {tie_gene, w->tie.p, (size_t)(8 * (int64_t)n_bins * G)},
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

extern "C" int cna_gene_ranksum_by(cna_ctx* c, const int32_t* codes, int n_bins, int64_t work_bytes, int64_t* rank2_out,
                                   double* tie_out, int64_t* n_out, uint8_t* nan_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_gene_ranksum_by: no expression matrix is resident (cna_expr_upload_*)");
  if (!codes || !rank2_out || !tie_out || !n_out || !nan_out) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_by: null pointer");
  if (n_bins < 1 || n_bins > RS_MAX_LEVELS) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_by: 1 <= n_bins <= 1024");
  if (work_bytes < 0) CNA_FAIL(CNA_EINVAL, "cna_gene_ranksum_by: work_bytes is 0 (the default) or a number of bytes");
  const int64_t G = s->G;
  RankSumWork* w = expr_work<RankSumWork>(s, EXPR_RANKSUM);
  // the codes are judged before anything is written; the sizes of the levels
  CNA_TRY(sort_count(c, s->st, w->sort, CellList{}, codes, s->n, n_bins, 0, 2,
                     "cna_gene_ranksum_by: a code lies outside [-1, n_bins)"));
  int64_t m = 0;
  for (int b = 0; b < n_bins; ++b) m += w->sort.tot_h[(size_t)b];
  if (s->is_f64) CNA_TRY(ranksum_run<double>(c, s, w, n_bins, work_bytes, m));
  else CNA_TRY(ranksum_run<float>(c, s, w, n_bins, work_bytes, m));
  std::vector<unsigned int> nanf((size_t)G);
  {
    ProfScope ps(c, CNA_K_RANKSUM_FETCH, s->st);
    CNA_TRY(fetch_results(s->st, "cna_gene_ranksum_by", {{rank2_out, w->rank2.p, (size_t)(8 * (int64_t)n_bins * G)},
                                                        {tie_out, w->tie.p, (size_t)(8 * G)},
                                                        {nanf.data(), w->nanf.p, (size_t)(4 * G)}}));
  }
  for (int64_t g = 0; g < G; ++g) nan_out[g] = nanf[(size_t)g] ? 1 : 0;
  for (int b = 0; b < n_bins; ++b) n_out[b] = w->sort.tot_h[(size_t)b];
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
  const int64_t G = s->G, out_count = (int64_t)n_pairs * G;
  RankSumWork* w = expr_work<RankSumWork>(s, EXPR_RANKSUM);
  // the codes are judged before anything is written; the sizes of the levels
  CNA_TRY(sort_count(c, s->st, w->sort, CellList{}, codes, s->n, n_bins, 0, 2,
                     "cna_gene_ranksum_pairs: a code lies outside [-1, n_bins)"));
  int64_t m = 0;
  for (int b = 0; b < n_bins; ++b) m += w->sort.tot_h[(size_t)b];
  for (Buf* b : {&w->u2, &w->ptie}) {
    const int rc = buf_need(c, s->st, *b, 8 * out_count);
    if (rc == CNA_ENOMEM) (void)hipGetLastError();    // the refusal is the caller's to see, not the next launch's
    CNA_TRY(rc);
  }
  CNA_TRY(buf_need(c, s->st, w->pairs, 8 * (int64_t)n_pairs));
  // (ranksum_sorted waits for the stream before the caller has its list back)
  HIP_TRY(hipMemcpyAsync(w->pairs.p, pairs, (size_t)(8 * n_pairs), hipMemcpyHostToDevice, s->st));
  if (s->is_f64) CNA_TRY(pairs_run<double>(c, s, w, n_bins, n_pairs, work_bytes, m));
  else CNA_TRY(pairs_run<float>(c, s, w, n_bins, n_pairs, work_bytes, m));
  std::vector<unsigned int> nanf((size_t)G);
  {
    ProfScope ps(c, CNA_K_RANKSUM_FETCH, s->st);
    CNA_TRY(fetch_results(s->st, "cna_gene_ranksum_pairs", {{u2_out, w->u2.p, (size_t)(8 * out_count)},
                                                           {tie_out, w->ptie.p, (size_t)(8 * out_count)},
                                                           {nanf.data(), w->nanf.p, (size_t)(4 * G)}}));
  }
  for (int64_t g = 0; g < G; ++g) nan_out[g] = nanf[(size_t)g] ? 1 : 0;
  for (int b = 0; b < n_bins; ++b) n_out[b] = w->sort.tot_h[(size_t)b];
  return 0;
}

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
