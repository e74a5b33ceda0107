// Private to the expression side of the library -- the resident expression matrix (genes.hip) and the entry points that
// work on the expression stream, one file each: cna_gene_corr (expr_corr.hip), cna_expr_to_bins (expr_bins.hip),
// cna_expr_cross (expr_cross.hip), cna_coef_strata (strata.hip), cna_gene_corr_by (expr_corr_by.hip), cna_matrix_to_bins
// (nam_bins.hip: the NAM or X by bin, on this stream with this sort), cna_enrichment_extremes (enrich.hip: no matrix at all,
// this stream and these buffers), cna_expr_cross_by (expr_cross_by.hip), cna_gram_by (gram_by.hip: X alone) and
// cna_coef_raster (raster.hip: no matrix, this stream, the sort twice); cna_graph_components_* (components.hip) borrows the
// stream and a slot of buffers and reads the resident graph; cna_gene_ranksum_by, cna_gene_ranksum_pairs and
// cna_gene_ranksum_within (expr_ranksum.hip: rank sums from a ranking of the cells of every gene), cna_gene_rank_corr and
// cna_gene_rank_corr_by (expr_rankcorr.hip: Spearman's rho against per-cell columns from the same ranking) and
// cna_gene_rank_corr_x, cna_gene_rank_corr_wide and cna_x_columns (expr_rankperm.hip: rho against up to 4096 columns, formed
// from X or given, from one sort), the three files sharing rank_sort.h: a
// radix sort on the chunk tables, the walk over a sorted list and their buffers; cna_nbhd_expr and cna_gene_nbhd_corr
// (expr_nbhd.hip: the random walk over tiles of gene columns, reading the resident graph as components.hip does).  What two
// of them need is here once:
//   Buf / BufSet    grow-only device buffers that are freed by having been declared
//   ExprState       the resident matrix, the stream, and one slot of work buffers per entry point
//   sort_*          the counting sort of the cells by code (cell list of cna_expr_to_bins and cna_gene_corr_by, value
//                   segments of cna_coef_strata): one count kernel, one fill kernel, one host half; CellListOf
//   gene_tiles      the walk over tiles of whole genes of the gene-major kernels
//   xrow_check      the verdict on a map cells -> rows of X (cna_expr_cross, the two entries by level, the two of
//                   expr_rankperm.hip that read X)
//   k_key_stats     the statistics of per-cell key columns (cna_gene_corr, cna_gene_nbhd_corr)
//   with_bool / with_width, fetch_results, result_bufs_need, finite_d, wave_min / wave_max
// Templates are instantiated where they are used; nothing here needs relocatable device code.
#pragma once
#include "common.h"
#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

// ------------------------------------------------------------------ buffers
// A grow-only device buffer (contents discarded when it grows, after the stream has drained).  It joins a set where it
// is declared -- `Buf x{set};` -- and the set frees whatever it holds: there is no second list to extend.
struct BufSet;
struct Buf {
  void* p = nullptr;
  int64_t cap = 0;
  explicit Buf(BufSet& set);
  Buf(const Buf&) = delete;
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};
struct BufSet {
  std::vector<Buf*> all;
  BufSet() = default;
  BufSet(const BufSet&) = delete;
  virtual ~BufSet() = default;
};
inline Buf::Buf(BufSet& set) { set.all.push_back(this); }
int buf_need(cna_ctx* c, hipStream_t st, Buf& b, int64_t bytes);
void buf_free(cna_ctx* c, Buf& b);
void bufs_free(cna_ctx* c, BufSet& set);
// temporaries of one scope: freed on every way out of it, once the stream has drained
struct ScopedBufs : BufSet {
  cna_ctx* c;
  hipStream_t st;
  ScopedBufs(cna_ctx* c_, hipStream_t st_) : c(c_), st(st_) {}
  ~ScopedBufs() override {
    (void)hipStreamSynchronize(st);
    bufs_free(c, *this);
  }
};

// ------------------------------------------------------------------ state (cna_ctx::expr)
enum ExprUser { EXPR_CORR, EXPR_BINS, EXPR_CROSS, EXPR_STRATA, EXPR_CORR_BY, EXPR_MAT_BINS, EXPR_ENRICH, EXPR_CROSS_BY,
                EXPR_GRAM_BY, EXPR_RASTER, EXPR_COMPONENTS, EXPR_RANKSUM, EXPR_NBHD, EXPR_USERS };

struct ExprState {
  hipStream_t st = nullptr;
  hipEvent_t x_ready = nullptr;    // main stream -> expression stream: what was queued there that produces X is done
  int format = 0;   // 0: none, 1: dense cells x genes, 2: gene-major lists
  int is_f64 = 0;
  int64_t n = 0, G = 0, nnz = 0;
  int64_t n_uploads = 0;
  BufSet bufs;
  Buf X{bufs};                                        // dense
  Buf gptr{bufs}, gcell{bufs}, gval{bufs};            // gene-major: G + 1 offsets, cell of every entry (ascending inside a gene), values
  Buf chunk_lo{bufs}, chunk_gene{bufs}, gchunk{bufs};   // first entry / gene of every chunk; first chunk of every gene (G + 1)
  int64_t nchunks = 0, chunk_len = 0;
  std::vector<int64_t> gchunk_h;   // host copy of gchunk (tiles over genes)
  // per entry point: its work buffers (grow-only until cna_expr_drop or the next upload), made on first use
  std::unique_ptr<BufSet> work[EXPR_USERS];
};

inline ExprState* expr_state(cna_ctx* c) { return static_cast<ExprState*>(c->expr); }
int expr_get_state(cna_ctx* c, ExprState** out);   // creates the state with its stream on first use
template <class W>
W* expr_work(ExprState* s, ExprUser user) {
  if (!s->work[user]) s->work[user].reset(new W());
  return static_cast<W*>(s->work[user].get());
}

// the scan of a counting sort: cnt[b][g] (B blocks x G) -> the count in the blocks before b; total[g]
void launch_block_scan(hipStream_t st, unsigned int* cnt, int64_t G, int B, int64_t* total);

// Tiles of whole genes (one gene at least) for a gene-major kernel that keeps one record of record_bytes per chunk of a
// tile, the records of a tile held to PB_PART_BYTES (genes.hip): genes [g0, g1), first chunk c0, nch chunks
struct GeneTile {
  int64_t g0, g1, c0, nch;
};
std::vector<GeneTile> gene_tiles(const ExprState* s, int64_t record_bytes, int64_t* largest);
// cells of one bin in a chunk of the dense form's cell list (genes.hip, beside the other rules that cut the matrix into pieces)
extern const int64_t PB_DENSE_CHUNK;

// The tail of an entry point: the first error of what was launched, of the copies to the host and of draining the stream,
// reported under the entry's name
struct HostCopy {
  void* dst;
  const void* src;
  size_t bytes;
};
int fetch_results(hipStream_t st, const char* who, std::initializer_list<HostCopy> copies);
// Result buffers whose size is the caller's to choose (outputs x genes): grown in turn; CNA_ENOMEM is the caller's to see,
// not the next launch's -- the runtime's sticky error is cleared
struct BufSize {
  Buf* buf;
  int64_t bytes;
};
int result_bufs_need(cna_ctx* c, hipStream_t st, std::initializer_list<BufSize> bufs);

// The verdict on a map cells -> rows of X (xrow_dev: n entries on the device; expr_cross.hip, k_xc_check): CNA_EINVAL under
// who's name for a value outside [-1, nx) or a row named twice, before any sum is formed; *m = the cells with a row
int xrow_check(cna_ctx* c, hipStream_t st, const int64_t* xrow_dev, int64_t n, int64_t nx, Buf& seen, Buf& flag,
               const char* who, int64_t* m);

// ------------------------------------------------------------------ run-time value -> template argument
// f(std::true_type / std::false_type); f(std::integral_constant<int, W>) for the least W of 1, 2, 4, 8, 16 that holds w
template <class F>
void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
template <class F>
void with_width(int w, F&& f) {
  if (w <= 1) f(std::integral_constant<int, 1>{});
  else if (w <= 2) f(std::integral_constant<int, 2>{});
  else if (w <= 4) f(std::integral_constant<int, 4>{});
  else if (w <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

// ------------------------------------------------------------------ device helpers
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.79769313486231570815e308; }
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// ------------------------------------------------------------------ statistics of per-cell key columns
// (cna_gene_corr, cna_gene_nbhd_corr)
constexpr int KS_LD = 8;   // doubles per key in the key statistics block: n, mean, sum vc^2, sum vc, min, max
// one block of 1024 threads per key: thread t adds the cells t, t + 1024, ...; the 1024 partial sums are folded by a
// fixed tree -- the same bits on every run
static __global__ __launch_bounds__(1024) void k_key_stats(const double* __restrict__ V, int64_t n, double* __restrict__ ks) {
  __shared__ double sh[4][1024];
  const int j = blockIdx.x, t = threadIdx.x;
  const double* v = V + (int64_t)j * n;
  double cnt = 0, sum = 0, mn = INFINITY, mx = -INFINITY;
  for (int64_t i = t; i < n; i += 1024) {
    const double x = v[i];
    if (finite_d(x)) {
      cnt += 1.0;
      sum += x;
      mn = fmin(mn, x);
      mx = fmax(mx, x);
    }
  }
  sh[0][t] = cnt; sh[1][t] = sum; sh[2][t] = mn; sh[3][t] = mx;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
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
  for (int64_t i = t; i < n; i += 1024) {
    const double x = v[i];
    if (finite_d(x)) {
      const double d = x - mean;
      s1 += d;
      s2 += d * d;
    }
  }
  sh[0][t] = s1; sh[1][t] = s2;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    double* o = ks + j * KS_LD;
    o[0] = N; o[1] = mean; o[2] = sh[1][0]; o[3] = sh[0][0]; o[4] = vmin; o[5] = vmax; o[6] = 0; o[7] = 0;
  }
}

// ------------------------------------------------------------------ counting sort of the cells by code
// The cells are cut into at most SORT_MAX_BLOCKS blocks of rows_per_block cells (a multiple of 64).  A caller is a
// policy P, passed to both kernels by value:
//   P::MAX_BINS, P::TALLIES     LDS: TALLIES x MAX_BINS counters in the count kernel, MAX_BINS cursors in the fill kernel
//   P::payload, load(i)         what is stored for cell i
//   keep(x)                     whether a cell with a code >= 0 is sorted (tally 0 counts those)
//   tally(h, cd, i, x, kept)    the tallies 1 .. TALLIES - 1 of a cell with a code >= 0 (TALLIES > 1 only)
constexpr int SORT_MAX_BLOCKS = 1024;

// block b: cnt[b][bin] = kept cells of [r0, r1) with that code; tot[k][bin] += tally k of the block, k >= 1; *bad |= 1 for
// a code outside [-1, n_bins)
template <class P>
__global__ __launch_bounds__(256) void k_sort_count(P p, const int32_t* __restrict__ codes, int64_t n, int n_bins,
                                                    int64_t rows_per_block, unsigned int* __restrict__ cnt,
                                                    unsigned long long* __restrict__ tot, int* __restrict__ bad) {
  __shared__ unsigned int h[P::TALLIES][P::MAX_BINS];
  for (int b = threadIdx.x; b < n_bins; b += blockDim.x)
    for (int k = 0; k < P::TALLIES; ++k) h[k][b] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += blockDim.x) {
    const int32_t cd = codes[i];
    if (cd < -1 || cd >= n_bins) {
      atomicOr(bad, 1);
    } else if (cd >= 0) {
      const typename P::payload x = p.load(i);
      const bool kept = p.keep(x);
      if (kept) atomicAdd(&h[0][cd], 1u);
      if constexpr (P::TALLIES > 1) p.tally(h, cd, i, x, kept);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_bins; b += blockDim.x) {
    cnt[(int64_t)blockIdx.x * n_bins + b] = h[0][b];
    for (int k = 1; k < P::TALLIES; ++k)
      if (h[k][b]) atomicAdd(&tot[(int64_t)k * n_bins + b], (unsigned long long)h[k][b]);
  }
}

// one wave per block of cells; cur[bin] = kept cells of the bin in the blocks before this one plus those already placed.
// Among the 64 cells of a batch equal codes are ranked by lane, so a bin's payloads keep the order of the cells whatever
// the scheduling; cur[] is carried from one batch of the block to the next behind two barriers.
template <class P>
__global__ __launch_bounds__(64) void k_sort_fill(P p, const int32_t* __restrict__ codes, int64_t n, int n_bins,
                                                  int64_t rows_per_block, const unsigned int* __restrict__ cnt,
                                                  const int64_t* __restrict__ bptr, typename P::payload* __restrict__ out) {
  __shared__ unsigned int cur[P::MAX_BINS];
  const int lane = threadIdx.x;
  for (int b = lane; b < n_bins; b += 64) cur[b] = cnt[(int64_t)blockIdx.x * n_bins + b];
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  for (int64_t base = r0; base < r1; base += 64) {
    const int64_t i = base + lane;
    typename P::payload x{};
    int32_t cd = -1;
    if (i < r1) {
      x = p.load(i);
      cd = codes[i];
    }
    if (cd < 0 || !p.keep(x)) cd = -1;          // (sort_count has refused codes >= n_bins)
    unsigned int rank = 0;
    bool last = true;
    for (int j = 0; j < 64; ++j) {
      const bool same = __shfl(cd, j, 64) == cd;
      rank += (same && j < lane) ? 1u : 0u;
      last = last && !(same && j > lane);
    }
    if (cd >= 0) out[bptr[cd] + (int64_t)(cur[cd] + rank)] = x;
    __syncthreads();
    if (cd >= 0 && last) cur[cd] += rank + 1u;
    __syncthreads();
  }
}

// The host half and its buffers.  table = [bptr (n_bins + 1) | first chunk of every bin (n_bins + 1) | one record per
// chunk: {lo, hi} (record 2) or {bin, lo, hi} (record 3), a chunk being at most chunk_len payloads of one bin, never empty]
struct CodeSort {
  Buf code, cnt, tot, flag, table;
  int n_bins = 0;
  int64_t rows_per_block = 0, blocks = 0, nch = 0;
  std::vector<int64_t> tot_h;      // [tally][bin] as counted
  std::vector<int64_t> table_h;    // the table on the host: it outlives the copy that reads it
  explicit CodeSort(BufSet& set) : code(set), cnt(set), tot(set), flag(set), table(set) {}
  const int32_t* codes() const { return code.as<const int32_t>(); }
  const int64_t* bptr() const { return table.as<const int64_t>(); }
  const int64_t* first() const { return bptr() + n_bins + 1; }
  const int64_t* chunks() const { return first() + n_bins + 1; }
  const unsigned long long* totals() const { return tot.as<const unsigned long long>(); }
};

// Sizes the blocks, uploads the codes, counts and scans; the codes are judged before any sum is formed: a bad one is
// refused with the caller's message.  Then the chunk table for chunk_len (0: none is wanted).
template <class P>
int sort_count(cna_ctx* c, hipStream_t st, CodeSort& s, const P& p, const int32_t* codes, int64_t n, int n_bins,
               int64_t chunk_len, int record, const char* refusal) {
  const int64_t rpb = round_up64((n + SORT_MAX_BLOCKS - 1) / SORT_MAX_BLOCKS, 64);
  const int64_t B = (n + rpb - 1) / rpb;
  const size_t tot_count = (size_t)P::TALLIES * n_bins;
  s.n_bins = n_bins;
  s.rows_per_block = rpb;
  s.blocks = B;
  s.nch = 0;
  CNA_TRY(buf_need(c, st, s.code, 4 * n));
  CNA_TRY(buf_need(c, st, s.cnt, 4 * B * n_bins));
  CNA_TRY(buf_need(c, st, s.tot, 8 * (int64_t)tot_count));
  CNA_TRY(buf_need(c, st, s.flag, 256));
  HIP_TRY(hipMemcpyAsync(s.code.p, codes, (size_t)(4 * n), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(s.flag.p, 0, 4, st));
  if (P::TALLIES > 1) HIP_TRY(hipMemsetAsync(s.tot.p, 0, 8 * tot_count, st));
  hipLaunchKernelGGL((k_sort_count<P>), dim3((unsigned)B), dim3(256), 0, st, p, s.codes(), n, n_bins, rpb,
                     s.cnt.as<unsigned int>(), s.tot.as<unsigned long long>(), s.flag.as<int>());
  launch_block_scan(st, s.cnt.as<unsigned int>(), n_bins, (int)B, s.tot.as<int64_t>());   // kept counts -> offsets, tot[0][bin]
  HIP_TRY(hipGetLastError());
  int bad = 0;
  s.tot_h.resize(tot_count);
  HIP_TRY(hipMemcpyAsync(&bad, s.flag.p, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s.tot_h.data(), s.tot.p, 8 * tot_count, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bad) CNA_FAIL(CNA_EINVAL, refusal);
  if (chunk_len == 0) return 0;
  const size_t nb1 = (size_t)n_bins + 1;
  std::vector<int64_t>& table = s.table_h;
  table.assign(2 * nb1, 0);
  for (int b = 0; b < n_bins; ++b) {
    const int64_t lo = table[(size_t)b], hi = lo + s.tot_h[(size_t)b];
    table[(size_t)b + 1] = hi;
    table[nb1 + (size_t)b] = s.nch;
    for (int64_t e = lo; e < hi; e += chunk_len, ++s.nch) {
      if (record == 3) table.push_back(b);
      table.push_back(e);
      table.push_back(std::min(e + chunk_len, hi));
    }
  }
  table[nb1 + (size_t)n_bins] = s.nch;
  CNA_TRY(buf_need(c, st, s.table, 8 * (int64_t)table.size()));
  // the per-bin part and the records go up separately, as cna_expr_to_bins always sent them: at 2M cells in 200 bins its
  // records take 16 000 bytes, and one copy of both parts crosses the size from which a copy takes the runtime 0.2 ms longer
  HIP_TRY(hipMemcpyAsync(s.table.p, table.data(), 8 * 2 * nb1, hipMemcpyHostToDevice, st));
  if (s.nch)
    HIP_TRY(hipMemcpyAsync(s.table.as<int64_t>() + 2 * nb1, table.data() + 2 * nb1, 8 * (table.size() - 2 * nb1),
                           hipMemcpyHostToDevice, st));
  return 0;
}

// the payloads sorted by bin into out (bptr[n_bins] of them), after sort_count with a table
template <class P>
void sort_fill(hipStream_t st, const CodeSort& s, const P& p, int64_t n, typename P::payload* out) {
  hipLaunchKernelGGL((k_sort_fill<P>), dim3((unsigned)s.blocks), dim3(64), 0, st, p, s.codes(), n, s.n_bins, s.rows_per_block,
                     s.cnt.as<const unsigned int>(), s.bptr(), out);
}

// the policy of a cell list (cna_expr_to_bins, cna_gene_corr_by; BINS: the entry's own cap): every cell with a code >= 0 is
// kept, what is stored is its index
template <int BINS>
struct CellListOf {
  static constexpr int MAX_BINS = BINS, TALLIES = 1;
  using payload = int32_t;
  __device__ int32_t load(int64_t i) const { return (int32_t)i; }
  __device__ bool keep(int32_t) const { return true; }
};
