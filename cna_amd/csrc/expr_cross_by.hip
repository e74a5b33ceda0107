// cna_expr_cross_by: cna_expr_cross inside every level of a clustering, in one pass over the resident expression matrix
// (cna.tl.gene_test_strata): W_l = E_{C_l}^T X_{C_l}, genes x samples, and the per-gene sums of x and x^2 over the cells C_l
// of level l that have a row in X -- the cell-sized contraction behind the null correlations of every gene with the permuted
// phenotypes' coefficients c_p = X^T z_p / N (the reference's null of _association.py:94-99) restricted to one cluster, the
// question cna.pl.violinplot(d, 'leiden', key='coef') (plotting/_strat.py:21-29) raises.
//   xrow_check (expr.h)  xrow as cna_expr_cross judges it
//   sort (expr.h)        checks every code against [-1, n_bins); the cells with a code >= 0 and a row in X sorted by level,
//                        ascending inside a level, cut into chunks of one level
//   k_xcb_dense          k_xc_dense with the row taken through the list: lane = gene, a wave walks a chunk of one level's cell
//                        list for a tile of 32 samples; the cell, its row of X and that row's values are the same in every
//                        lane (scalar loads), the gathered row of E one coalesced read.  One partial per (chunk, gene, sample)
//                        with plain stores; the first tile also takes sum x and sum x^2
//   k_xcb_finish_dense*  add the partials of a (level, gene) in chunk order
//
// Levels [bin0, bin0 + nb) of n_bins.  The chunk length is the slab of cna_expr_cross for these cells, so there are at most
// its slabs plus one chunk per level, and the partial sums take what cna_expr_cross needs plus one chunk per level.
//
// The dense form only.  For gene-major lists a one-pass kernel was written and measured -- k_xc_sparse with the accumulators
// in LDS, [levels of a pass][samples + 2] doubles indexed by the level of each entry's cell -- and lost to one cna_expr_cross
// per level with xrow masked to that level at 1M cells x 100 samples, 32 levels (129 ms against 109 ms,
// profiles/kbench_gene_test_strata.txt: every entry pays a dependent LDS read-add-write where k_xc_sparse adds in
// registers).  By the rule set before the measurement it is not here: Engine.expr_cross_by serves that form by the masked
// route, and this entry refuses it with CNA_ESTATE.
//
// Result sums take a fixed order (no floating-point atomics): two runs on one input give the same bits.
#include "expr.h"
#include <cstring>

namespace {

constexpr int XCB_TS = 32;             // samples per tile of k_xcb_dense: 64 accumulator registers per lane
constexpr int XCB_MAX_COLS = 1024;
constexpr int XCB_MAX_LEVELS = 1024;
constexpr int64_t XCB_PART_BYTES = 1ll << 30;   // partial sums of the dense kernel at most, before one chunk per level
constexpr int64_t XCB_MIN_CHUNK = 128;          // cells of a chunk of the dense kernel at least

// the sort's policy: what is stored is the cell; a cell with a code >= 0 is kept when it has a row in X
struct KeptCells {
  static constexpr int MAX_BINS = XCB_MAX_LEVELS, TALLIES = 1;
  using payload = int32_t;
  const int64_t* xrow;
  __device__ int32_t load(int64_t i) const { return (int32_t)i; }
  __device__ bool keep(int32_t cell) const { return xrow[cell] >= 0; }
};

// xrow and the table of named X rows with the verdict; the sort with its codes and chunks; the cell list; partial sums
// (W | sum x, sum x^2); the results
struct CrossByWork : BufSet {
  Buf xrow{*this}, xseen{*this}, flag{*this};
  CodeSort sort{*this};
  Buf list{*this}, part{*this}, part2{*this}, out{*this};
};

// the entries [lo, hi) of the cell list against the samples [s0, s0 + ns) of X; FULL: ns == XCB_TS (no index is clamped)
template <typename T, bool FULL>
__device__ __forceinline__ void xcb_chunk(const T* __restrict__ E, int64_t G, int64_t gl, const int32_t* __restrict__ list,
                                          int64_t lo, int64_t hi, const int64_t* __restrict__ xrow,
                                          const double* __restrict__ Xw, int ldx, int s0, int ns, bool first, double* acc,
                                          double& sx, double& sxx) {
  constexpr int U = 4;
  for (int64_t e = lo; e < hi; e += U) {
    T xs[U];
    int64_t cell[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ee = e + u < hi ? e + u : hi - 1;
      cell[u] = list[ee];                        // the same in every lane: a scalar load
      xs[u] = E[cell[u] * G + gl];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e + u >= hi) break;
      const int64_t xr = xrow[cell[u]];          // wave-uniform; >= 0: the sort kept the cell
      const double* v = Xw + xr * ldx + s0;      // ... and so is the row of X: scalar loads, one uniform operand per FMA
      const double x = (double)xs[u];
      if (first) {
        sx += x;
        sxx = fma(x, x, sxx);
      }
#pragma unroll
      for (int s = 0; s < XCB_TS; ++s) acc[s] = fma(x, v[FULL ? s : (s < ns ? s : ns - 1)], acc[s]);
    }
  }
}

// grid.x = gene block * ntile + tile, grid.y = chunk - ch0; rng[2 ch], rng[2 ch + 1]: the chunk's span of the cell list (never
// empty).  part[(rec * Nx + s) * G + g], part2[(rec * 2 + {0: sum x, 1: sum x^2}) * G + g] with rec = blockIdx.y
template <typename T>
__global__ __launch_bounds__(64) void k_xcb_dense(const T* __restrict__ E, int64_t G, const int32_t* __restrict__ list,
                                                  const int64_t* __restrict__ rng, int64_t ch0,
                                                  const int64_t* __restrict__ xrow, const double* __restrict__ Xw, int ldx,
                                                  int Nx, int ntile, double* __restrict__ part, double* __restrict__ part2) {
  const int tile = (int)(blockIdx.x % (unsigned)ntile);
  const int64_t g = (int64_t)(blockIdx.x / (unsigned)ntile) * 64 + threadIdx.x;
  const bool act = g < G;
  const int64_t gl = act ? g : G - 1;          // idle lanes of the last gene block reload its last gene; nothing is stored
  const int64_t lo = rng[2 * (ch0 + blockIdx.y)], hi = rng[2 * (ch0 + blockIdx.y) + 1];
  const int s0 = tile * XCB_TS;
  const int ns = Nx - s0 < XCB_TS ? Nx - s0 : XCB_TS;
  const bool first = tile == 0;
  double acc[XCB_TS];
#pragma unroll
  for (int s = 0; s < XCB_TS; ++s) acc[s] = 0.0;
  double sx = 0.0, sxx = 0.0;
  if (ns == XCB_TS) xcb_chunk<T, true>(E, G, gl, list, lo, hi, xrow, Xw, ldx, s0, ns, first, acc, sx, sxx);
  else xcb_chunk<T, false>(E, G, gl, list, lo, hi, xrow, Xw, ldx, s0, ns, first, acc, sx, sxx);
  if (!act) return;
  double* o = part + ((int64_t)blockIdx.y * Nx + s0) * G + g;
#pragma unroll
  for (int s = 0; s < XCB_TS; ++s)
    if (s < ns) o[(int64_t)s * G] = acc[s];
  if (first) {
    part2[((int64_t)blockIdx.y * 2) * G + g] = sx;
    part2[((int64_t)blockIdx.y * 2 + 1) * G + g] = sxx;
  }
}

// W[l][g][s] = the partials of (level bin0 + l, g, s) added in chunk order (bfirst: first chunk of every level, ch0 = bfirst[bin0])
// (lane = gene: the partials are read coalesced, W is written with a stride of Nx doubles between lanes, as k_xc_finish_dense
// writes it; the fold's share of the call has not been measured on its own -- a transpose through LDS is the follow-up if it shows)
__global__ __launch_bounds__(256) void k_xcb_finish_dense(const double* __restrict__ part, int64_t G, int Nx, int bin0, int nb,
                                                          const int64_t* __restrict__ bfirst, double* __restrict__ W) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nb * Nx * G) return;
  const int64_t l = t / ((int64_t)Nx * G), s = t / G % Nx, g = t % G;
  const int64_t ch0 = bfirst[bin0];
  double a = 0.0;
  for (int64_t ch = bfirst[bin0 + l]; ch < bfirst[bin0 + l + 1]; ++ch) a += part[((ch - ch0) * Nx + s) * G + g];
  W[(l * G + g) * Nx + s] = a;
}

// sx[l][g], sxx[l][g] likewise
__global__ __launch_bounds__(256) void k_xcb_finish_dense_sx(const double* __restrict__ part2, int64_t G, int bin0, int nb,
                                                             const int64_t* __restrict__ bfirst, double* __restrict__ sx,
                                                             double* __restrict__ sxx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nb * G) return;
  const int64_t l = t / G, g = t % G;
  const int64_t ch0 = bfirst[bin0];
  double a = 0.0, b = 0.0;
  for (int64_t ch = bfirst[bin0 + l]; ch < bfirst[bin0 + l + 1]; ++ch) {
    a += part2[((ch - ch0) * 2) * G + g];
    b += part2[((ch - ch0) * 2 + 1) * G + g];
  }
  sx[t] = a;
  sxx[t] = b;
}

// cells of a chunk of the dense kernel: the slab of cna_expr_cross for n cells (enough single-wave workgroups to fill the
// device, partials held to XCB_PART_BYTES), at least XCB_MIN_CHUNK
int64_t xcb_chunk_len(int64_t n, int64_t G, int Nx) {
  const int ntile = (Nx + XCB_TS - 1) / XCB_TS;
  const int64_t gene_blocks = (G + 63) / 64;
  int64_t nslab = std::min<int64_t>(2048, (8192 + gene_blocks * ntile - 1) / (gene_blocks * ntile));
  nslab = std::min<int64_t>(nslab, std::max<int64_t>(1, XCB_PART_BYTES / (8 * (int64_t)Nx * G)));
  nslab = std::max<int64_t>(1, std::min<int64_t>(nslab, n / XCB_MIN_CHUNK));
  return std::max<int64_t>(XCB_MIN_CHUNK, (n + nslab - 1) / nslab);
}

template <typename T>
int xcb_dense(cna_ctx* c, ExprState* s, CrossByWork* w, const double* Xw, int ldx, int Nx, int bin0, int nb, double* W,
              double* sx) {
  const int64_t G = s->G;
  const int ntile = (Nx + XCB_TS - 1) / XCB_TS;
  const int64_t gene_blocks = (G + 63) / 64;
  if (gene_blocks * ntile > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, "cna_expr_cross_by: more than 2^31 - 1 workgroups (gene blocks x sample tiles)");
  const int64_t* first = w->sort.table_h.data() + w->sort.n_bins + 1;     // first chunk of every level, on the host
  const int64_t ch0 = first[bin0], nch = first[bin0 + nb] - ch0;
  if (nch > 65535) CNA_FAIL(CNA_EINVAL, "cna_expr_cross_by: more than 65535 chunks");
  CNA_TRY(buf_need(c, s->st, w->part, 8 * std::max<int64_t>(1, nch) * Nx * G));
  CNA_TRY(buf_need(c, s->st, w->part2, 16 * std::max<int64_t>(1, nch) * G));
  if (nch)
    hipLaunchKernelGGL((k_xcb_dense<T>), dim3((unsigned)(gene_blocks * ntile), (unsigned)nch), dim3(64), 0, s->st,
                       s->X.as<const T>(), G, w->list.as<const int32_t>(), w->sort.chunks(), ch0, w->xrow.as<const int64_t>(), Xw,
                       ldx, Nx, ntile, w->part.as<double>(), w->part2.as<double>());
  hipLaunchKernelGGL(k_xcb_finish_dense, dim3((unsigned)(((int64_t)nb * G * Nx + 255) / 256)), dim3(256), 0, s->st,
                     w->part.as<const double>(), G, Nx, bin0, nb, w->sort.first(), W);
  hipLaunchKernelGGL(k_xcb_finish_dense_sx, dim3((unsigned)(((int64_t)nb * G + 255) / 256)), dim3(256), 0, s->st,
                     w->part2.as<const double>(), G, bin0, nb, w->sort.first(), sx, sx + (int64_t)nb * G);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int cna_expr_cross_by(cna_ctx* c, const int64_t* xrow, const int32_t* codes, int64_t n_cells, int n_bins, int bin0,
                                 int nb, double* W_out, double* sx_out, double* sxx_out, int64_t* m_out) {
  CHECK_CTX(c);
  ExprState* s = expr_state(c);
  if (!s || s->format == 0) CNA_FAIL(CNA_ESTATE, "cna_expr_cross_by: no expression matrix is resident (cna_expr_upload_*)");
  if (s->format != 1)
    CNA_FAIL(CNA_ESTATE, "cna_expr_cross_by: the resident matrix is gene-major lists; this entry serves the dense form (take "
                         "cna_expr_cross per level with xrow masked to the level, as Engine.expr_cross_by does)");
  if (c->auto_pending) CNA_TRY(cna_nam_auto_finish(c, nullptr, nullptr));
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "cna_expr_cross_by: X not available");
  if (comm_active(c)) CNA_FAIL(CNA_ESTATE, "cna_expr_cross_by: one rank only (the rows of X of other ranks are not here)");
  if (!xrow || !codes || !W_out || !sx_out || !sxx_out || !m_out) CNA_FAIL(CNA_EINVAL, "cna_expr_cross_by: null pointer");
  if (n_bins < 1 || n_bins > XCB_MAX_LEVELS) CNA_FAIL(CNA_EINVAL, "cna_expr_cross_by: 1 <= n_bins <= 1024");
  if (bin0 < 0 || nb < 1 || bin0 > n_bins - nb) CNA_FAIL(CNA_EINVAL, "cna_expr_cross_by: the levels [bin0, bin0 + nb) must lie in [0, n_bins), nb >= 1");
  if (n_cells != s->n)
    CNA_FAIL(CNA_EINVAL, "cna_expr_cross_by: xrow and codes have " + std::to_string(n_cells) + " entries, the expression matrix " +
                             std::to_string(s->n) + " cells");
  const int64_t n = s->n, G = s->G, nx = c->nx;
  const int Nx = c->Nx, ldx = c->ldx;
  if (Nx < 1 || Nx > XCB_MAX_COLS) CNA_FAIL(CNA_EINVAL, "cna_expr_cross_by: 1 <= columns of X <= 1024");
  const double* Xw = c->X;
  CrossByWork* w = expr_work<CrossByWork>(s, EXPR_CROSS_BY);
  const int64_t n_w = (int64_t)nb * G * Nx, n_out = n_w + 2 * (int64_t)nb * G;
  CNA_TRY(buf_need(c, s->st, w->xrow, 8 * n));
  CNA_TRY(buf_need(c, s->st, w->list, 4 * n));
  CNA_TRY(buf_need(c, s->st, w->out, 8 * n_out));
  HIP_TRY(hipMemcpyAsync(w->xrow.p, xrow, (size_t)(8 * n), hipMemcpyHostToDevice, s->st));
  // xrow and the codes are judged before any sum is formed (and before X is touched)
  int64_t m_all = 0;
  CNA_TRY(xrow_check(c, s->st, w->xrow.as<const int64_t>(), n, nx, w->xseen, w->flag, "cna_expr_cross_by", &m_all));
  const KeptCells kept{w->xrow.as<const int64_t>()};
  const int64_t chunk_len = xcb_chunk_len(n, G, Nx);
  CNA_TRY(sort_count(c, s->st, w->sort, kept, codes, n, n_bins, chunk_len, 2, "cna_expr_cross_by: a code lies outside [-1, n_bins)"));
  // whatever the main stream has queued that produces X comes first (an event, no host sync).  The other direction needs
  // nothing: this entry returns only after the expression stream has drained, so a later producer of X finds the read done
  HIP_TRY(hipEventRecord(s->x_ready, c->stream));
  HIP_TRY(hipStreamWaitEvent(s->st, s->x_ready, 0));
  double* W = w->out.as<double>();
  double* sx = W + n_w;
  int rc;
  {
    ProfScope ps(c, CNA_K_EXPR_CROSS_BY, s->st);
    sort_fill(s->st, w->sort, kept, n, w->list.as<int32_t>());
    rc = s->is_f64 ? xcb_dense<double>(c, s, w, Xw, ldx, Nx, bin0, nb, W, sx) : xcb_dense<float>(c, s, w, Xw, ldx, Nx, bin0, nb, W, sx);
  }
  if (rc != 0) {
    (void)hipStreamSynchronize(s->st);
    return rc;
  }
  // the caller's buffers are written only once everything has succeeded
  std::vector<double> host((size_t)(2 * (int64_t)nb * G));
  CNA_TRY(fetch_results(s->st, "cna_expr_cross_by", {{W_out, w->out.p, (size_t)(8 * n_w)},
                                                      {host.data(), sx, 8 * host.size()}}));
  std::memcpy(sx_out, host.data(), 8 * (size_t)((int64_t)nb * G));
  std::memcpy(sxx_out, host.data() + (int64_t)nb * G, 8 * (size_t)((int64_t)nb * G));
  for (int l = 0; l < nb; ++l) m_out[l] = w->sort.tot_h[(size_t)(bin0 + l)];
  return 0;
}
