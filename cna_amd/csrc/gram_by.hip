// cna_gram_by: the Gram matrix of the working matrix X inside every level of a clustering, Gamma_l = X_{C_l}^T X_{C_l}
// (samples x samples) over the cells C_l of level l that have a row in X (cna.tl.gene_test_strata: sum_i c_p[i]^2 over one
// cluster = z_p^T Gamma_l z_p / N^2 for the null coefficient c_p = X^T z_p / N of _association.py:94-99; all cells together
// it is the NAM.dot(NAM.T) of _nam.py:105 that cna_gram computes).  X is read through the level-sorted list of its rows and
// is not copied; all levels together do the flops of one cna_gram.
//   xrow_check (expr.h)  xrow as cna_expr_cross judges it
//   sort (expr.h)        checks every code against [-1, n_bins); the rows of X of the cells with a code >= 0, sorted by
//                        level, in cell order inside a level, cut into chunks of one level
//   k_gram_by            one workgroup of four waves per (chunk, pair of 64-sample blocks bi <= bj): slabs of GB_SLAB rows are
//                        gathered into LDS (the 64 columns of either block, zero beyond the chunk and beyond Nx) and wave w
//                        feeds the 16 x 16 tiles (w, 0 .. 3) of the 64 x 64 block with v_mfma_f64_16x16x4_f64, one A and up
//                        to four B fragments per k step (operand maps: mfma.hip).  Of a diagonal block only the tiles on and
//                        above the diagonal are computed.  One partial block per (chunk, pair), plain stores
//   k_gram_by_finish     adds the partials of a (level, pair) in chunk order and mirrors the upper triangle
// The tile loaders of mfma.hip:k_gram_blk copy contiguous slabs of all of X's columns as double2 and rest on its wave
// table; a gathered slab of 64 columns shares neither, so this file has its own (a dozen lines).
//
// Partial storage: (chunks x pairs) blocks of 32 KB with chunks <= rows / chunk + n_bins; the chunk (GB_MIN_CHUNK rows at
// least) grows until rows / chunk x pairs x 32 KB fit GB_PART_BYTES, and the share of the levels is about the result's size.
// Sums take a fixed order (the rows of a chunk in list order through the MFMA's own accumulation, chunks in order; no
// floating-point atomics): two runs on one input give the same bits.
#include "expr.h"
#include <cstring>

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int GB_MAX_LEVELS = 1024;
constexpr int GB_MAX_COLS = 1024;
constexpr int GB_BLK = 64;              // samples of a block side: four 16-wide tiles, one tile row per wave
constexpr int GB_SLAB = 32;             // rows of X in LDS at a time: eight k steps of the MFMA
constexpr int GB_LDP = 80;              // row stride in LDS: the four k rows of a fragment read fall into different banks
constexpr int64_t GB_MIN_CHUNK = 1024;  // rows of one level per workgroup at least
constexpr int64_t GB_PART_BYTES = 1ll << 30;    // partial blocks beyond one chunk per level
constexpr int64_t GB_OUT_BYTES = 1ll << 30;     // the result at most (XC_PART_BYTES of expr_cross.hip)

// the sort's policy: what is stored is the cell's row of X; a cell with a code >= 0 is kept when it has one
struct RowsOfX {
  static constexpr int MAX_BINS = GB_MAX_LEVELS, TALLIES = 1;
  using payload = int32_t;
  const int64_t* xrow;
  __device__ int32_t load(int64_t i) const { return (int32_t)xrow[i]; }      // (xrow_check has passed: in [-1, rows of X))
  __device__ bool keep(int32_t r) const { return r >= 0; }
};

struct GramByWork : BufSet {
  Buf xrow{*this}, xseen{*this}, flag{*this};
  CodeSort sort{*this};
  Buf list{*this}, part{*this}, out{*this};
};

// grid.x = chunk * npair + pair; rng[2 ch], rng[2 ch + 1]: the chunk's span of the row list (never empty).
// part[(ch * npair + pair) * 4096 + (tile row * 4 + tile column) * 256 + i * 16 + j]
__global__ __launch_bounds__(256) void k_gram_by(const double* __restrict__ X, int ldx, int Nx, int nbk, int npair,
                                                 const int32_t* __restrict__ list, const int64_t* __restrict__ rng,
                                                 double* __restrict__ part) {
  __shared__ double sm[2][GB_SLAB][GB_LDP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t ch = (int64_t)blockIdx.x / npair;
  int bi = 0, bj = (int)((int64_t)blockIdx.x % npair);
  while (bj >= nbk - bi) {                     // pair -> (bi, bj), bi <= bj, row-major over the upper triangle
    bj -= nbk - bi;
    ++bi;
  }
  bj += bi;
  const bool diag = bi == bj;
  const int64_t lo = rng[2 * ch], hi = rng[2 * ch + 1];
  const int ak = lane >> 4, ai = lane & 15;
  const int ca = GB_BLK * bi + lane, cb = GB_BLK * bj + lane;      // the column this thread loads of either block
  bool live[4];
  v4d acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    live[t] = (!diag || t >= wv) && GB_BLK * bi + 16 * wv < Nx && GB_BLK * bj + 16 * t < Nx;
  }
  const double(*A)[GB_LDP] = sm[0];
  const double(*B)[GB_LDP] = sm[diag ? 0 : 1];
  for (int64_t e0 = lo; e0 < hi; e0 += GB_SLAB) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < GB_SLAB / 4; ++k) {
      const int row = wv + 4 * k;
      const int64_t e = e0 + row;
      const int64_t xr = e < hi ? (int64_t)list[e] : -1;             // the same in every lane of a wave: a scalar load
      sm[0][row][lane] = (xr >= 0 && ca < Nx) ? X[xr * ldx + ca] : 0.0;
      if (!diag) sm[1][row][lane] = (xr >= 0 && cb < Nx) ? X[xr * ldx + cb] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kq = 0; kq < GB_SLAB / 4; ++kq) {
      const double a = A[4 * kq + ak][16 * wv + ai];
      const double b0 = B[4 * kq + ak][ai], b1 = B[4 * kq + ak][16 + ai], b2 = B[4 * kq + ak][32 + ai],
                   b3 = B[4 * kq + ak][48 + ai];
      if (live[0]) acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[0], 0, 0, 0);
      if (live[1]) acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[1], 0, 0, 0);
      if (live[2]) acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, acc[2], 0, 0, 0);
      if (live[3]) acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b3, acc[3], 0, 0, 0);
    }
  }
  double* p = part + (int64_t)blockIdx.x * (GB_BLK * GB_BLK) + wv * 4 * 256;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (live[t]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) p[t * 256 + r * 64 + lane] = acc[t][r];      // D[i][j]: i = (lane >> 4) + 4 r, j = lane & 15
    }
}

// out[l][a][b] = the partials of (level l, the upper one of (a, b) and (b, a)) added in chunk order (bfirst: first chunk of
// every level)
__global__ __launch_bounds__(256) void k_gram_by_finish(const double* __restrict__ part, int Nx, int nbk, int npair, int n_bins,
                                                        const int64_t* __restrict__ bfirst, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n_bins * Nx * Nx) return;
  const int64_t l = t / ((int64_t)Nx * Nx);
  const int a = (int)(t / Nx % Nx), b = (int)(t % Nx);
  const int u = a < b ? a : b, v = a < b ? b : a;
  const int bi = u / GB_BLK, bj = v / GB_BLK, I = u % GB_BLK, J = v % GB_BLK;
  const int pair = bi * nbk - bi * (bi - 1) / 2 + (bj - bi);
  const int64_t at = (int64_t)pair * (GB_BLK * GB_BLK) + ((I / 16) * 4 + J / 16) * 256 + (I % 16) * 16 + J % 16;
  double sum = 0.0;
  for (int64_t ch = bfirst[l]; ch < bfirst[l + 1]; ++ch) sum += part[ch * npair * (GB_BLK * GB_BLK) + at];
  out[t] = sum;
}

}  // namespace

extern "C" int cna_gram_by(cna_ctx* c, const int64_t* xrow, const int32_t* codes, int64_t n_cells, int n_bins, double* gram_out,
                           int64_t* m_out) {
  CHECK_CTX(c);
  if (c->auto_pending) CNA_TRY(cna_nam_auto_finish(c, nullptr, nullptr));
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "cna_gram_by: X not available");
  if (comm_active(c)) CNA_FAIL(CNA_ESTATE, "cna_gram_by: one rank only (the rows of X of other ranks are not here)");
  if (!xrow || !codes || !gram_out || !m_out) CNA_FAIL(CNA_EINVAL, "cna_gram_by: null pointer");
  if (n_bins < 1 || n_bins > GB_MAX_LEVELS) CNA_FAIL(CNA_EINVAL, "cna_gram_by: 1 <= n_bins <= 1024");
  if (n_cells < 1 || n_cells >= (1ll << 31)) CNA_FAIL(CNA_EINVAL, "cna_gram_by: 1 <= n_cells < 2^31");
  const int64_t n = n_cells, nx = c->nx;
  const int Nx = c->Nx, ldx = c->ldx;
  if (Nx < 1 || Nx > GB_MAX_COLS) CNA_FAIL(CNA_EINVAL, "cna_gram_by: 1 <= columns of X <= 1024");
  if (nx >= (1ll << 31)) CNA_FAIL(CNA_EINVAL, "cna_gram_by: rows of X must lie in [0, 2^31)");
  const int64_t n_out = (int64_t)n_bins * Nx * Nx;
  if (8 * n_out > GB_OUT_BYTES) CNA_FAIL(CNA_EINVAL, "cna_gram_by: n_bins x columns of X squared x 8 bytes exceed 1 GiB; take fewer levels per call");
  ExprState* es = nullptr;
  CNA_TRY(expr_get_state(c, &es));
  hipStream_t st = es->st;
  GramByWork* w = expr_work<GramByWork>(es, EXPR_GRAM_BY);
  CNA_TRY(buf_need(c, st, w->xrow, 8 * n));
  CNA_TRY(buf_need(c, st, w->list, 4 * n));
  CNA_TRY(buf_need(c, st, w->out, 8 * n_out));
  HIP_TRY(hipMemcpyAsync(w->xrow.p, xrow, (size_t)(8 * n), hipMemcpyHostToDevice, st));
  // xrow and the codes are judged before any sum is formed (and before X is touched)
  int64_t m_all = 0;
  CNA_TRY(xrow_check(c, st, w->xrow.as<const int64_t>(), n, nx, w->xseen, w->flag, "cna_gram_by", &m_all));
  const int nbk = (Nx + GB_BLK - 1) / GB_BLK, npair = nbk * (nbk + 1) / 2;
  const int64_t block_bytes = 8ll * GB_BLK * GB_BLK;
  const int64_t chunk_len =
      std::max<int64_t>(GB_MIN_CHUNK, round_up64((n * npair * block_bytes + GB_PART_BYTES - 1) / GB_PART_BYTES, GB_SLAB));
  const RowsOfX rows{w->xrow.as<const int64_t>()};
  CNA_TRY(sort_count(c, st, w->sort, rows, codes, n, n_bins, chunk_len, 2, "cna_gram_by: a code lies outside [-1, n_bins)"));
  const int64_t nch = w->sort.nch;
  if (nch * npair > 0x7fffffffll) CNA_FAIL(CNA_EINVAL, "cna_gram_by: more than 2^31 - 1 workgroups (chunks x block pairs)");
  CNA_TRY(buf_need(c, st, w->part, std::max<int64_t>(1, nch) * npair * block_bytes));
  // whatever the main stream has queued that produces X comes first (an event, no host sync).  The other direction needs
  // nothing: this entry returns only after the expression stream has drained
  HIP_TRY(hipEventRecord(es->x_ready, c->stream));
  HIP_TRY(hipStreamWaitEvent(st, es->x_ready, 0));
  {
    ProfScope ps(c, CNA_K_GRAM_BY, st);
    sort_fill(st, w->sort, rows, n, w->list.as<int32_t>());
    if (nch)
      hipLaunchKernelGGL(k_gram_by, dim3((unsigned)(nch * npair)), dim3(256), 0, st, c->X, ldx, Nx, nbk, npair,
                         w->list.as<const int32_t>(), w->sort.chunks(), w->part.as<double>());
    hipLaunchKernelGGL(k_gram_by_finish, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, w->part.as<const double>(), Nx, nbk,
                       npair, n_bins, w->sort.first(), w->out.as<double>());
  }
  // the caller's buffers are written only once everything has succeeded
  CNA_TRY(fetch_results(st, "cna_gram_by", {{gram_out, w->out.p, (size_t)(8 * n_out)}}));
  for (int l = 0; l < n_bins; ++l) m_out[l] = w->sort.tot_h[(size_t)l];
  return 0;
}
