// cna_expr_to_bins: per-bin sums of the resident expression matrix (cna.ut.expr_to_sample: the samples x genes
// "pseudobulk" that stands beside the reference's utils/multisample.py:4-11 obs_to_sample).
//   sort (expr.h)   checks every code against [-1, n_bins) and counts the cells of every bin per block of cells; dense form
//                   only: the cells sorted by bin, ascending inside a bin (the lists carry their cell already)
//   k_pb_dense      lane = gene, a workgroup walks a chunk (PB_DENSE_CHUNK cells) of one bin's cell list, every row read
//                   a coalesced run of genes; one partial per (chunk, gene) with plain stores
//   k_pb_sparse     one wave per chunk of a gene's list, the bins' accumulators in LDS (4096 doubles at most); lanes of
//                   one batch that meet in a bin are served lowest lane first, in rounds (an integer LDS atomic names
//                   the lane whose turn it is); one partial per (chunk, bin) with plain stores
//   k_pb_finish_*   adds the partials of a (bin, gene) in chunk order
// Partial storage: dense (cells / PB_DENSE_CHUNK + min(cells, n_bins)) x genes doubles -- never more than the result plus
// 1 / 1024 of the matrix' own size (f32); gene-major lists: chunks x n_bins doubles, held to PB_PART_BYTES (256 MB) by
// going over the genes in tiles (a single gene whose chunks alone exceed it gets a tile of its own: at most 2^31 / 65536
// chunks x 4096 bins x 8 bytes = 1 GB).
//
// Result sums take a fixed order (no floating-point atomics): two runs on one input give the same bits.  Integer
// atomics only count and hand out turns.
#include "expr.h"
#include <cstring>

namespace {

constexpr int PB_MAX_BINS = 4096;
using CellList = CellListOf<PB_MAX_BINS>;   // the sort's policy (expr.h)

// the sort with its codes and chunks of the bins; the cell list; partial sums; the sums
struct BinsWork : BufSet {
  CodeSort sort{*this};
  Buf list{*this}, part{*this}, rout{*this};
};

// grid.x = chunk * gene_blocks + gene block (neighbouring workgroups read neighbouring pieces of the same rows);
// rng[2 ch], rng[2 ch + 1]: the chunk's span of the cell list (never empty).  COUNT: add 1 where x > 0 instead of x.
template <typename T, bool COUNT>
__global__ __launch_bounds__(256) void k_pb_dense(const T* __restrict__ X, int64_t G, int64_t gene_blocks,
                                                  const int32_t* __restrict__ list, const int64_t* __restrict__ rng,
                                                  double* __restrict__ part) {
  constexpr int U = 8;
  const int64_t ch = (int64_t)blockIdx.x / gene_blocks, gb = (int64_t)blockIdx.x % gene_blocks;
  const int64_t g = gb * blockDim.x + threadIdx.x;
  const bool act = g < G;
  const int64_t gl = act ? g : G - 1;          // idle lanes of the last gene block reload its last gene; nothing is stored
  const int64_t lo = rng[2 * ch], hi = rng[2 * ch + 1];
  double acc = 0.0;
  for (int64_t e = lo; e < hi; e += U) {
    T xs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ee = e + u < hi ? e + u : hi - 1;
      xs[u] = X[(int64_t)list[ee] * G + gl];   // list[ee] is the same in every lane: a scalar load
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e + u >= hi) break;
      acc += COUNT ? (xs[u] > (T)0 ? 1.0 : 0.0) : (double)xs[u];
    }
  }
  if (act) part[ch * G + g] = acc;
}

// out[bin][gene] = the bin's partials added in chunk order (bfirst: first chunk of every bin, n_bins + 1 entries)
__global__ __launch_bounds__(256) void k_pb_finish_dense(const double* __restrict__ part, int64_t G, int n_bins,
                                                         const int64_t* __restrict__ bfirst, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n_bins * G) return;
  const int64_t b = t / G, g = t % G;
  double s = 0.0;
  for (int64_t ch = bfirst[b]; ch < bfirst[b + 1]; ++ch) s += part[ch * G + g];
  out[t] = s;
}

// one wave per chunk c0 + blockIdx.x of the gene lists; dynamic LDS: n_bins doubles (the sums) and n_bins ints (turns).
// A batch is 64 consecutive entries.  Where every lane of a batch that takes part names the same bin, the wave adds them
// by its fixed tree and lane 0 adds the total; otherwise rounds: every waiting lane posts stamp * 64 + 63 - lane with an
// integer atomic max, the lowest waiting lane of each bin finds its own value there and adds.  Both orders depend on the
// input alone.
template <typename T, bool COUNT>
__global__ __launch_bounds__(64) void k_pb_sparse(const int64_t* __restrict__ chunk_lo, const int32_t* __restrict__ chunk_gene,
                                                  const int64_t* __restrict__ gptr, int64_t c0, int64_t chunk_len,
                                                  const int32_t* __restrict__ gcell, const T* __restrict__ gval,
                                                  const int32_t* __restrict__ codes, int n_bins, double* __restrict__ part) {
  extern __shared__ double pb_lds[];
  double* acc = pb_lds;
  int* turn = reinterpret_cast<int*>(pb_lds + n_bins);
  const int lane = threadIdx.x;
  const int64_t ch = c0 + blockIdx.x;
  for (int b = lane; b < n_bins; b += 64) {
    acc[b] = 0.0;
    turn[b] = 0;
  }
  __syncthreads();
  const int64_t lo = chunk_lo[ch];
  const int64_t end = gptr[chunk_gene[ch] + 1];
  const int64_t hi = lo + chunk_len < end ? lo + chunk_len : end;
  int stamp = 0;
  for (int64_t e0 = lo; e0 < hi; e0 += 64) {
    const int64_t e = e0 + lane;
    int32_t bin = -1;
    double v = 0.0;
    if (e < hi) {
      bin = codes[gcell[e]];
      const T x = gval[e];
      v = COUNT ? (x > (T)0 ? 1.0 : 0.0) : (double)x;
    }
    bool wait = bin >= 0;
    const unsigned long long in = __ballot(wait);
    if (in == 0) continue;
    const int32_t b0 = __shfl(bin, __ffsll((long long)in) - 1, 64);
    if (__ballot(wait && bin != b0) == 0) {
      const double s = wave_sum(wait ? v : 0.0);
      if (lane == 0) acc[b0] += s;
      __syncthreads();
      continue;
    }
    while (true) {
      ++stamp;
      const int mine = stamp * 64 + 63 - lane;
      if (wait) atomicMax(&turn[bin], mine);
      __syncthreads();
      if (wait && turn[bin] == mine) {
        acc[bin] += v;
        wait = false;
      }
      __syncthreads();
      if (__ballot(wait) == 0) break;
    }
  }
  __syncthreads();
  double* o = part + (int64_t)blockIdx.x * n_bins;
  for (int b = lane; b < n_bins; b += 64) o[b] = acc[b];
}

// genes [g0, g1) of a tile whose first chunk is c0: out[bin][gene] = the gene's partials added in chunk order
__global__ __launch_bounds__(256) void k_pb_finish_sparse(const double* __restrict__ part, const int64_t* __restrict__ gchunk,
                                                          int64_t g0, int64_t g1, int64_t c0, int n_bins, int64_t G,
                                                          double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (g1 - g0) * n_bins) return;
  const int64_t g = g0 + t / n_bins, b = t % n_bins;
  double s = 0.0;
  for (int64_t ch = gchunk[g]; ch < gchunk[g + 1]; ++ch) s += part[(ch - c0) * n_bins + b];
  out[b * G + g] = s;
}

template <typename T>
int pb_dense(cna_ctx* c, ExprState* s, BinsWork* w, int n_bins, bool count) {
  const int64_t n = s->n, G = s->G, nch = w->sort.nch;
  const int threads = (int)std::min<int64_t>(256, (G + 63) / 64 * 64);
  const int64_t gene_blocks = (G + threads - 1) / threads;
  if (nch * gene_blocks > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: more than 2^31 - 1 workgroups (chunks x gene blocks)");
  CNA_TRY(buf_need(c, s->st, w->list, 4 * n));
  CNA_TRY(buf_need(c, s->st, w->part, 8 * std::max<int64_t>(1, nch) * G));
  sort_fill(s->st, w->sort, CellList{}, n, w->list.as<int32_t>());
  if (nch)
    with_bool(count, [&](auto cnt) {
      hipLaunchKernelGGL((k_pb_dense<T, decltype(cnt)::value>), dim3((unsigned)(nch * gene_blocks)), dim3(threads), 0, s->st,
                         s->X.as<const T>(), G, gene_blocks, w->list.as<const int32_t>(), w->sort.chunks(), w->part.as<double>());
    });
  hipLaunchKernelGGL(k_pb_finish_dense, dim3((unsigned)(((int64_t)n_bins * G + 255) / 256)), dim3(256), 0, s->st,
                     w->part.as<const double>(), G, n_bins, w->sort.first(), w->rout.as<double>());
  HIP_TRY(hipGetLastError());
  return 0;
}

template <typename T>
int pb_sparse(cna_ctx* c, ExprState* s, BinsWork* w, int n_bins, bool count) {
  int64_t need = 1;
  const std::vector<GeneTile> tiles = gene_tiles(s, 8 * (int64_t)n_bins, &need);
  if (need > 0x7fffffffll / 256) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: one gene has too many chunks");
  CNA_TRY(buf_need(c, s->st, w->part, 8 * need * n_bins));
  const size_t lds = (size_t)n_bins * 12;
  for (const GeneTile& t : tiles) {
    if (t.nch)
      with_bool(count, [&](auto cnt) {
        hipLaunchKernelGGL((k_pb_sparse<T, decltype(cnt)::value>), dim3((unsigned)t.nch), dim3(64), lds, s->st,
                           s->chunk_lo.as<const int64_t>(), s->chunk_gene.as<const int32_t>(), s->gptr.as<const int64_t>(), t.c0,
                           s->chunk_len, s->gcell.as<const int32_t>(), s->gval.as<const T>(), w->sort.codes(), n_bins,
                           w->part.as<double>());
      });
    hipLaunchKernelGGL(k_pb_finish_sparse, dim3((unsigned)(((t.g1 - t.g0) * n_bins + 255) / 256)), dim3(256), 0, s->st,
                       w->part.as<const double>(), s->gchunk.as<const int64_t>(), t.g0, t.g1, t.c0, n_bins, s->G,
                       w->rout.as<double>());
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int cna_expr_to_bins(cna_ctx* c, const int32_t* codes, int n_bins, int what, double* sums_out, int64_t* counts_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_expr_to_bins: no expression matrix is resident (cna_expr_upload_*)");
  if (!codes || !sums_out || !counts_out) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: null pointer");
  if (n_bins < 1 || n_bins > PB_MAX_BINS) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: 1 <= n_bins <= 4096");
  if (what != 0 && what != 1) CNA_FAIL(CNA_EINVAL, "cna_expr_to_bins: what is 0 (sums of x) or 1 (counts of x > 0)");
  const bool dense = s->format == 1, count = what == 1;
  BinsWork* w = expr_work<BinsWork>(s, EXPR_BINS);
  CNA_TRY(buf_need(c, s->st, w->rout, 8 * s->G * n_bins));
  CNA_TRY(sort_count(c, s->st, w->sort, CellList{}, codes, s->n, n_bins, dense ? PB_DENSE_CHUNK : 0, 2,
                     "cna_expr_to_bins: a code lies outside [-1, n_bins)"));
  if (dense) CNA_TRY(s->is_f64 ? pb_dense<double>(c, s, w, n_bins, count) : pb_dense<float>(c, s, w, n_bins, count));
  else CNA_TRY(s->is_f64 ? pb_sparse<double>(c, s, w, n_bins, count) : pb_sparse<float>(c, s, w, n_bins, count));
  HIP_TRY(hipMemcpyAsync(sums_out, w->rout.p, (size_t)(8 * s->G * n_bins), hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  std::memcpy(counts_out, w->sort.tot_h.data(), 8 * (size_t)n_bins);
  return 0;
}
