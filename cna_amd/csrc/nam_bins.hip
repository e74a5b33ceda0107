// cna_matrix_to_bins: weighted per-bin sums over the rows of the resident NAM or of the working matrix X
// (cna.tl.nam_strata: the NAM mass of every sample in every cluster, or in a cluster's expanded / depleted neighbourhoods --
// the reference reaches both through the NAM of _nam.py:73 on the host, demo/demo.ipynb section 3.2, aggregated as
// utils/multisample.py:4-11 aggregates per-cell columns).
//   sort (expr.h)   checks every code against [-1, n_bins); keeps a row with a code >= 0 and at least one contributing
//                   weight (finite and non-zero; every row with a code >= 0 without weights); the kept row indices by
//                   bin, ascending inside a bin, cut into chunks of NB_CHUNK rows of one bin
//   k_nb_sum        one workgroup per (chunk, block of columns), lane = column; the row index and the row's q weights are
//                   the same in every lane (scalar loads), NB_UNROLL rows are loaded before they are added; the q sums of
//                   a lane in registers; per chunk and weight column one partial per matrix column and the number of
//                   contributing rows, plain stores
//   k_nb_finish     adds the partials and the counts of a (weight column, bin) in chunk order
// The product is FUSED: sum = fma(w, x, sum), one rounding per row and column.  A row that does not contribute to a weight
// column is skipped there, not multiplied: a zero weight against a NaN entry adds nothing.  Without weights sum += x.
// Sums take a fixed order (no floating-point atomics): two runs on one input give the same bits.
//
// Partial storage: max(q, 1) x chunks x n_cols doubles with chunks <= kept rows / NB_CHUNK + n_bins -- at most q / NB_CHUNK
// of the matrix' own size plus the size of the result; the weights are held as they came (q x n_rows doubles).
//
// The matrix is read and left as it is and nothing derived from it is kept.  Runs on the expression stream, which waits
// through an event for what the main stream has queued that produces the matrix; returns after its own stream has drained.
#include "expr.h"
#include <cstring>

namespace {

constexpr int NB_MAX_BINS = 1024;
constexpr int NB_MAX_Q = 16;
constexpr int NB_MAX_SUMS = 4096;       // max(q, 1) x n_bins
constexpr int64_t NB_CHUNK = 512;       // rows of one bin per workgroup: 2M rows leave ~4000 workgroups, partials 1/512 of the matrix
constexpr int NB_UNROLL = 8;            // rows whose loads are in flight before the adds

__device__ __forceinline__ bool contributes(double w) { return finite_d(w) && w != 0.0; }

// the sort's policy: what is stored is the row index; a row with a code >= 0 is kept when one weight column takes it
struct KeptRows {
  static constexpr int MAX_BINS = NB_MAX_BINS, TALLIES = 1;
  using payload = int32_t;
  const double* W;       // q x n, or null
  int q;
  int64_t n;
  __device__ int32_t load(int64_t i) const { return (int32_t)i; }
  __device__ bool keep(int32_t r) const {
    if (!W) return true;
    for (int j = 0; j < q; ++j)
      if (contributes(W[(int64_t)j * n + r])) return true;
    return false;
  }
};

// the weights; the sort with its codes and chunks; the kept rows by bin; partial sums and counts; sums | counts
struct MatBinsWork : BufSet {
  Buf w{*this};
  CodeSort sort{*this};
  Buf list{*this}, part{*this}, pcnt{*this}, rout{*this};
};

// grid.x = chunk * col_blocks + column block; rng[2 ch], rng[2 ch + 1]: the chunk's span of the row list (never empty).
// part[(ch * qq + j) * N + s], pcnt[ch * qq + j] with qq = max(q, 1).  UNIT: no weights (Q = 1).
template <int Q, bool UNIT>
__global__ __launch_bounds__(256) void k_nb_sum(const double* __restrict__ M, int ld, int N, int64_t col_blocks,
                                                const double* __restrict__ W, int q, int64_t n,
                                                const int32_t* __restrict__ list, const int64_t* __restrict__ rng,
                                                double* __restrict__ part, int64_t* __restrict__ pcnt) {
  constexpr int U = NB_UNROLL;
  const int64_t ch = (int64_t)blockIdx.x / col_blocks, cb = (int64_t)blockIdx.x % col_blocks;
  const int64_t s = cb * blockDim.x + threadIdx.x;
  const bool act = s < N;
  const int64_t sl = act ? s : N - 1;          // idle lanes of the last column block reload its last column; nothing is stored
  const int64_t lo = rng[2 * ch], hi = rng[2 * ch + 1];
  const int qq = UNIT ? 1 : q;
  double acc[Q];
  int cnt[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    acc[j] = 0.0;
    cnt[j] = 0;
  }
  for (int64_t e = lo; e < hi; e += U) {
    double xs[U];
    int32_t rs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ee = e + u < hi ? e + u : hi - 1;
      rs[u] = list[ee];                        // the same in every lane: a scalar load
      xs[u] = M[(int64_t)rs[u] * ld + sl];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e + u >= hi) break;
      if (UNIT) {
        acc[0] += xs[u];
        cnt[0] += 1;
      } else {
#pragma unroll
        for (int j = 0; j < Q; ++j) {
          if (j < q) {
            const double w = W[(int64_t)j * n + rs[u]];      // wave-uniform, and so is the branch
            if (contributes(w)) {
              acc[j] = fma(w, xs[u], acc[j]);
              cnt[j] += 1;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    if (j < qq) {
      if (act) part[(ch * qq + j) * N + s] = acc[j];
      if (cb == 0 && threadIdx.x == 0) pcnt[ch * qq + j] = cnt[j];
    }
  }
}

// out[(j * n_bins + b) * N + s] = the bin's partials added in chunk order, cnt_out[j * n_bins + b] likewise (bfirst: first
// chunk of every bin, n_bins + 1 entries)
__global__ __launch_bounds__(256) void k_nb_finish(const double* __restrict__ part, const int64_t* __restrict__ pcnt, int N,
                                                   int n_bins, int qq, const int64_t* __restrict__ bfirst,
                                                   double* __restrict__ out, int64_t* __restrict__ cnt_out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)qq * n_bins * N) return;
  const int64_t jb = t / N, s = t % N;
  const int64_t j = jb / n_bins, b = jb % n_bins;
  double sum = 0.0;
  for (int64_t ch = bfirst[b]; ch < bfirst[b + 1]; ++ch) sum += part[(ch * qq + j) * N + s];
  out[t] = sum;
  if (s == 0) {
    int64_t m = 0;
    for (int64_t ch = bfirst[b]; ch < bfirst[b + 1]; ++ch) m += pcnt[ch * qq + j];
    cnt_out[jb] = m;
  }
}

}  // namespace

extern "C" int cna_matrix_to_bins(cna_ctx* c, int which, const int32_t* codes, const double* W, int q, int64_t n_rows,
                                  int n_bins, double* sums_out, int64_t* n_out) {
  CHECK_CTX(c);
  if (!codes || !sums_out || !n_out) CNA_FAIL(CNA_EINVAL, "cna_matrix_to_bins: null pointer");
  if (which != CNA_MAT_NAM && which != CNA_MAT_X) CNA_FAIL(CNA_EINVAL, "cna_matrix_to_bins: which is CNA_MAT_NAM or CNA_MAT_X");
  if (q < 0 || q > NB_MAX_Q || (q > 0) != (W != nullptr))
    CNA_FAIL(CNA_EINVAL, "cna_matrix_to_bins: 0 <= q <= 16, W = NULL exactly when q = 0");
  if (n_bins < 1 || n_bins > NB_MAX_BINS) CNA_FAIL(CNA_EINVAL, "cna_matrix_to_bins: 1 <= n_bins <= 1024");
  const int qq = std::max(q, 1);
  if ((int64_t)qq * n_bins > NB_MAX_SUMS) CNA_FAIL(CNA_EINVAL, "cna_matrix_to_bins: max(q, 1) x n_bins <= 4096");
  if (comm_active(c)) CNA_FAIL(CNA_ESTATE, "cna_matrix_to_bins: one rank only (the rows of other ranks are not here)");
  // a pending walk's verdict is collected and a lazy NAM produced here, on the main stream
  int64_t rows = 0;
  int N = 0;
  CNA_TRY(cna_matrix_shape(c, which, &rows, &N));
  if (n_rows != rows)
    CNA_FAIL(CNA_EINVAL, "cna_matrix_to_bins: " + std::to_string(n_rows) + " codes, the matrix has " + std::to_string(rows) +
                             " local rows");
  if (rows >= (1ll << 31)) CNA_FAIL(CNA_EINVAL, "cna_matrix_to_bins: rows must lie in [0, 2^31)");
  const double* M = which == CNA_MAT_NAM ? c->nam : c->X;
  const int ld = which == CNA_MAT_NAM ? c->ld : c->ldx;
  const int64_t n = rows, n_sums = (int64_t)qq * n_bins * N, n_cnt = (int64_t)qq * n_bins;
  if (n == 0 || N == 0) {
    std::memset(sums_out, 0, 8 * (size_t)n_sums);
    std::memset(n_out, 0, 8 * (size_t)n_cnt);
    return 0;
  }
  ExprState* es = nullptr;
  CNA_TRY(expr_get_state(c, &es));
  hipStream_t st = es->st;
  MatBinsWork* w = expr_work<MatBinsWork>(es, EXPR_MAT_BINS);
  if (q) {
    CNA_TRY(buf_need(c, st, w->w, 8 * (int64_t)q * n));
    HIP_TRY(hipMemcpyAsync(w->w.p, W, (size_t)(8 * (int64_t)q * n), hipMemcpyHostToDevice, st));
  }
  const double* Wd = q ? w->w.as<const double>() : nullptr;
  const KeptRows kept{Wd, q, n};
  {
    ProfScope ps(c, CNA_K_MATRIX_BINS_SORT, st);
    CNA_TRY(sort_count(c, st, w->sort, kept, codes, n, n_bins, NB_CHUNK, 2, "cna_matrix_to_bins: a code lies outside [-1, n_bins)"));
  }
  const int64_t nch = w->sort.nch;
  const int threads = (int)std::min<int64_t>(256, (N + 63) / 64 * 64);
  const int64_t col_blocks = (N + threads - 1) / threads;
  if (nch * col_blocks > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, "cna_matrix_to_bins: more than 2^31 - 1 workgroups (chunks x column blocks)");
  CNA_TRY(buf_need(c, st, w->list, 4 * n));
  CNA_TRY(buf_need(c, st, w->part, 8 * std::max<int64_t>(1, nch) * qq * N));
  CNA_TRY(buf_need(c, st, w->pcnt, 8 * std::max<int64_t>(1, nch) * qq));
  CNA_TRY(buf_need(c, st, w->rout, 8 * (n_sums + n_cnt)));
  // whatever the main stream has queued that produces the matrix comes first (an event, no host sync).  The other direction
  // needs nothing: this entry returns only after the expression stream has drained
  HIP_TRY(hipEventRecord(es->x_ready, c->stream));
  HIP_TRY(hipStreamWaitEvent(st, es->x_ready, 0));
  double* sums = w->rout.as<double>();
  int64_t* cnts = reinterpret_cast<int64_t*>(sums + n_sums);
  {
    ProfScope ps(c, CNA_K_MATRIX_BINS_SUM, st);
    sort_fill(st, w->sort, kept, n, w->list.as<int32_t>());
    if (nch) {
      const dim3 grid((unsigned)(nch * col_blocks)), block(threads);
      if (!q)
        hipLaunchKernelGGL((k_nb_sum<1, true>), grid, block, 0, st, M, ld, N, col_blocks, Wd, q, n, w->list.as<const int32_t>(),
                           w->sort.chunks(), w->part.as<double>(), w->pcnt.as<int64_t>());
      else
        with_width(q, [&](auto width) {
          hipLaunchKernelGGL((k_nb_sum<decltype(width)::value, false>), grid, block, 0, st, M, ld, N, col_blocks, Wd, q, n,
                             w->list.as<const int32_t>(), w->sort.chunks(), w->part.as<double>(), w->pcnt.as<int64_t>());
        });
    }
    hipLaunchKernelGGL(k_nb_finish, dim3((unsigned)((n_sums + 255) / 256)), dim3(256), 0, st, w->part.as<const double>(),
                       w->pcnt.as<const int64_t>(), N, n_bins, qq, w->sort.first(), sums, cnts);
  }
  // the caller's buffers are written only once everything has succeeded
  std::vector<double> host((size_t)(n_sums + n_cnt));
  CNA_TRY(fetch_results(st, "cna_matrix_to_bins", {{host.data(), w->rout.p, 8 * host.size()}}));
  std::memcpy(sums_out, host.data(), 8 * (size_t)n_sums);
  std::memcpy(n_out, host.data() + n_sums, 8 * (size_t)n_cnt);
  return 0;
}
