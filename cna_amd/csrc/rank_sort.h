// Private to expr_ranksum.hip (the rank sums), expr_rankcorr.hip and expr_rankperm.hip (Spearman): a ranking of the kept
// cells of every gene of the resident matrix, which no entry point owns, and the buffers the entries share (RankSumWork).
//   k_rs_keys_sparse / k_rs_keys_dense
//                         every entry of a gene's list, or of a 64 x 64 tile of the dense matrix, -> an order-preserving
//                         unsigned key (-0.0 and a stored zero = the key of +0.0; float64 on all 64 bits) and its payload P,
//                         what it carries through the sort: the level of its cell (uint16_t) or the cell (uint32_t).  An
//                         entry of a left-out cell gets the largest key and rs_left<P>(): it sorts behind the kept ones and
//                         no kernel behind the sort reads it.  The kept entries of every gene; a kept NaN is flagged
//   k_rs_count / k_rs_scan / k_rs_scatter
//                         one pass of an LSD radix sort segmented by gene, 8 bits at a time, on a chunk table (the lists'
//                         of build_chunks, or dense_table's of the same shape): a count per (chunk, digit) in LDS; per
//                         segment a scan over its chunks and then over the digits; one wave per chunk scatters, lanes with
//                         the same digit ranked by lane (k_sort_fill's rule, by ballots), cursors carried from batch to batch
//   rs_tiles, ranksum_sorted
//                         tiles of whole segments within work_bytes; the keys and passes of every tile of the matrix
//   rs_walk_*             behind the sort, a workgroup on one sorted list: the tie run [s, e) of every entry for the caller's
//                         visitor, the list's tie term and its zero group
//
// The contract of the sort (rs_passes).  Every pass is stable and its result does not depend on scheduling.  The value
// passes, one per byte of the key, are an even number: the sorted {key, payload} are where the keys were written, (ka, pa).
// With `lvl8` (the payload is the cell) one more pass takes the level of the entry's cell as its digit (255: left out), an
// odd number in all: the lists are in the other buffers, (kb, pb), every segment level-major and sorted by value inside a
// level, and dbase[segment - g0][l], the scan that pass leaves, is where level l begins inside the segment (and l + 1: ends).
#pragma once
#include "expr.h"

constexpr int64_t RS_WORK_BYTES = 1ll << 30;   // keys + payloads + their copies of one tile, when the caller names no budget
constexpr int64_t RS_DENSE_CHUNK = 1024;       // cells of one gene per sort chunk of the dense form (build_chunks' least)
constexpr int RS_UNIT = 256;                   // entries of a sorted list a walk takes at a time
constexpr int RS_TILE = 64;                    // the dense gather's square tile
constexpr uint16_t RS_LEFT = 0xffff;           // "level" of an entry whose cell is left out (rs_left<uint16_t>())

// The one slot EXPR_RANKSUM: the five entry points share keys, payloads, counters and the dense table.  One definition with
// external linkage: the translation unit that creates it and the one that casts to it (expr_work) mean the same type.
struct RankSumWork : BufSet {
  CodeSort sort{*this};
  Buf keyA{*this}, keyB{*this}, lvlA{*this}, lvlB{*this}, cnt{*this}, dbase{*this}, kept{*this}, nanf{*this}, rank2{*this},
      tie{*this};
  Buf pairs{*this}, u2{*this}, ptie{*this};                            // cna_gene_ranksum_pairs: its pairs and results
  Buf seg{*this}, chunk_lo{*this}, chunk_gene{*this}, gchunk{*this};   // the dense form's table (the lists have the state's)
  // cna_gene_rank_corr: the columns, the kept cells' count, b[cell][W], the columns' tie terms (96 bits), the two limbs of S
  Buf vcol{*this}, vm{*this}, btab{*this}, tiek{*this}, slo{*this}, shi{*this};
  Buf lvl8{*this};                                                     // cna_gene_rank_corr_by: the kept cell's level as a byte
  // cna_gene_rank_corr_x / _x_by / _wide (expr_rankperm.hip): the tables b[group][cell][16] and the tie terms of every group
  // of 16 columns (per level in _x_by); a = s + e - m of every entry of a tile of genes and a_0 of every (level, gene); xrow
  // with its verdict, Z, the columns.  _x_by adds no buffer: its levels ride in lvl8 and vm, as cna_gene_rank_corr_by's
  Buf btabs{*this}, tieks{*this}, aent{*this}, azero{*this}, xrow{*this}, xseen{*this}, xflag{*this}, zrows{*this}, xcols{*this};
  // cna_gene_ranksum_within (its blocks ride in lvl8): the weights and the sizes of its (block, level) table; the results
  Buf wtab{*this}, wd2{*this}, wnum{*this}, wtiew{*this}, wlive{*this};
};

// What an entry carries through the sort beside its key.  All ones: the cell is left out.
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
template <typename K>
constexpr K rs_key_zero() { return (K)1 << (8 * sizeof(K) - 1); }   // the key of +0.0

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
// per cell (the one pass behind them; the payload is the cell).  What a source does not read of an entry is not loaded.
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
// dbase[gene - g0][digit] = the gene's entries with a smaller digit.  (static: a kernel of each file that includes this)
static __global__ __launch_bounds__(256) void k_rs_scan(const int64_t* __restrict__ gchunk, int64_t g0, int64_t c0,
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

// the radix passes over the chunks [c0, c0 + nch) of the segments [g0, g0 + genes) of a table, whose entries begin at `base`
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

// a chunk table of the lists' shape for `segs` segments of `len` entries each (the dense form: a gene holds the entries
// [g n, (g + 1) n); the columns of cna_gene_rank_corr: q segments of n cells)
inline int dense_table(cna_ctx* c, ExprState* s, RankSumWork* w, int64_t len, int64_t segs, std::vector<int64_t>& seg_h,
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

// Tiles of whole segments of a host table -- segment g: the entries [seg_h[g], seg_h[g + 1]) in the chunks [gchunk_h[g],
// gchunk_h[g + 1]) -- whose entries, at per_entry bytes each, stay within work_bytes (0: RS_WORK_BYTES); a segment that alone
// exceeds it is one tile.  The counters of the sort (1 KB per chunk) come on top.  `who` and `what` name the caller and its
// segments in what is refused.
struct SortTiles {
  std::vector<GeneTile> tiles;
  int64_t entries = 1, chunks = 1, segs = 1;          // the most of any tile
};
inline int rs_tiles(const std::vector<int64_t>& seg_h, const std::vector<int64_t>& gchunk_h, int64_t segs, int64_t per_entry,
                    int64_t work_bytes, const char* who, const char* what, SortTiles* out) {
  const int64_t max_entries = std::max<int64_t>(1, (work_bytes > 0 ? work_bytes : RS_WORK_BYTES) / per_entry);
  for (int64_t g0 = 0, g1; g0 < segs; g0 = g1) {
    g1 = g0 + 1;
    while (g1 < segs && seg_h[(size_t)g1 + 1] - seg_h[(size_t)g0] <= max_entries) ++g1;
    out->tiles.push_back({g0, g1, gchunk_h[(size_t)g0], gchunk_h[(size_t)g1] - gchunk_h[(size_t)g0]});
    out->entries = std::max(out->entries, seg_h[(size_t)g1] - seg_h[(size_t)g0]);
    out->chunks = std::max(out->chunks, out->tiles.back().nch);
    out->segs = std::max(out->segs, g1 - g0);
  }
  if (out->chunks > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, std::string(who) + ": more than 2^31 - 1 chunks in one tile of " + what);
  return 0;
}

// Tiling, keys and the radix passes of the resident matrix: for every tile of whole genes `behind(tile, base, keys,
// payloads, seg)` queues the kernel that reads the tile's sorted lists.  P: what an entry carries (rs_payload); the cells
// with codes[i] >= 0 (w->sort.code) are kept, m of them.  `who` names the entry in what is refused.  With `lvl8` the lists
// are level-major and w->dbase holds, per gene of the tile, where each level begins.
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
  SortTiles ts;
  const int64_t per_entry = 2 * (int64_t)(sizeof(K) + sizeof(P));   // keys, payloads and their copies
  CNA_TRY(rs_tiles(seg_h, dense ? gchunk_own : s->gchunk_h, G, per_entry, work_bytes, who, "genes", &ts));
  CNA_TRY((rs_sort_bufs<K, P>(c, s, w, ts.entries, ts.chunks, ts.segs)));
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
  for (const GeneTile& t : ts.tiles) {
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

// ------------------------------------------------------------------ behind the sort: the walks over one sorted list
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

// A workgroup of RS_UNIT threads walks the k sorted keys of one list, RS_UNIT entries at a time: forward for the start s of
// every entry's tie run (a prefix maximum over the run heads, carried across units), backward for one past its end e (a
// suffix minimum over the run tails, as a maximum of their negatives).  visit(p, kk, s or e) is called for every entry p
// with its key kk by the thread that holds it; the barriers are outside it, so every thread meets them.  The forward walk
// keeps for its thread (RankWalkMine) the entries below zero, the stored zeros and the tie terms t^3 - t of the runs that
// end with it, the run of the stored zeros left out: with the implicit zeros of the gene-major form, z = cells - k, it is
// one group, which rs_walk_fold puts together.  Entries above that group lie z higher than in the list: the visitor's shift.
// The workgroup's LDS is the kernel's to declare: sh and tsh of RS_UNIT entries; below and zeros, 0 before the fold.
struct RankWalkMine { double tacc = 0.0; unsigned int below = 0, zeros = 0; };
template <typename K, class Visit>
__device__ __forceinline__ void rs_walk_forward(const K* __restrict__ key, long long k, long long* sh, RankWalkMine& mine,
                                                Visit&& visit) {
  constexpr K K0 = rs_key_zero<K>();
  const int t = threadIdx.x;
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
      visit(p, kk, s);
      mine.below += kk < K0 ? 1u : 0u;
      mine.zeros += kk == K0 ? 1u : 0u;
      if (tail && kk != K0) {
        const long long r = p + 1 - s;
        mine.tacc += (double)r * (double)(r * r - 1);
      }
    }
    __syncthreads();                                  // sh is read (carry) before the next scan writes it
  }
}
template <typename K, class Visit>
__device__ __forceinline__ void rs_walk_backward(const K* __restrict__ key, long long k, long long* sh, Visit&& visit) {
  const int t = threadIdx.x;
  long long carry = 0;
  for (long long u0 = k > 0 ? (k - 1) / RS_UNIT * RS_UNIT : -1; u0 >= 0; u0 -= RS_UNIT) {
    const long long p = u0 + t;
    const bool valid = p < k;
    K kk = 0;
    bool tail = false;
    if (valid) {
      kk = key[p];
      tail = p == k - 1 || key[p + 1] != kk;
    }
    const long long none = -0x7fffffffffffffffll;   // (the last thread of a full unit carries)
    const long long e = -rs_scan_max(tail ? -(p + 1) : (valid && t == RS_UNIT - 1 ? carry : none), sh, true);
    carry = sh[RS_UNIT - 1];                      // reversed index: thread 0's value, negated as it is used
    if (valid) visit(p, kk, e);
    __syncthreads();
  }
}
// behind both walks: the entries below zero, the zero group t0 (stored and implicit zeros) and the list's tie term, the
// threads' added in list order and folded by a fixed tree
struct RankWalkZero { long long below, t0; double tie; };
__device__ __forceinline__ RankWalkZero rs_walk_fold(const RankWalkMine& mine, long long z, double* tsh, unsigned int* below,
                                                     unsigned int* zeros) {
  const int t = threadIdx.x;
  if (mine.below) atomicAdd(below, mine.below);
  if (mine.zeros) atomicAdd(zeros, mine.zeros);
  tsh[t] = mine.tacc;
  __syncthreads();
  for (int w = RS_UNIT / 2; w > 0; w >>= 1) {
    if (t < w) tsh[t] += tsh[t + w];
    __syncthreads();
  }
  const long long t0 = (long long)*zeros + z;
  return {(long long)*below, t0, tsh[0] + (t0 > 0 ? (double)t0 * (double)(t0 * t0 - 1) : 0.0)};
}

// ------------------------------------------------------------------ 128-bit sums
// {low 64 bits, what lies above}: a tie term t^3 - t of up to 2^31 cells passes 2^64
struct U128 { unsigned long long lo, hi; };
__device__ __forceinline__ U128 u128_mul(unsigned long long a, unsigned long long b) { return {a * b, __umul64hi(a, b)}; }
__device__ __forceinline__ U128 u128_add(U128 a, U128 b) {
  const unsigned long long lo = a.lo + b.lo;
  return {lo, a.hi + b.hi + (lo < a.lo ? 1ull : 0ull)};
}
__device__ __forceinline__ U128 rp_tie_term(unsigned long long t) { return t ? u128_mul(t * t - 1ull, t) : U128{0ull, 0ull}; }
// an exact, commutative add: the carry out of the low word is that of this add in whatever order the adds land
__device__ __forceinline__ void rp_add128(unsigned long long* lo, unsigned int* hi, U128 x) {
  if (!(x.lo | x.hi)) return;
  const unsigned long long old = atomicAdd(lo, x.lo);
  const unsigned int up = (unsigned int)x.hi + (old + x.lo < old ? 1u : 0u);
  if (up) atomicAdd(hi, up);
}
