// The expression matrix that stays resident on the device, one per context, in the CALLER's cell order: dense cells x
// genes, or gene-major lists {cell, value} cut into chunks.  The entry points that read it have a file each (expr.h);
// here are the state, the upload path and what they share that is not a template.
//
// Nothing here writes the state of c_api.hip (graph, walk, NAM, X, cell order): the buffers and the stream are this
// side's own (cna_ctx::expr).
//
//   k_narrow_idx    indices of 4 or 8 bytes -> int32, checked
//   k_tr_*          counting transpose of a CSR upload into the gene-major form, stable in the cell index; k_tr_scan is
//                   also the scan of the counting sort by code (launch_block_scan)
#include "expr.h"
#include <cstring>

namespace {

void release_matrix(cna_ctx* c, ExprState* s) {
  (void)hipStreamSynchronize(s->st);
  bufs_free(c, s->bufs);
  for (auto& w : s->work)
    if (w) bufs_free(c, *w);
  s->gchunk_h.clear();
  s->format = 0;
  s->n = s->G = s->nnz = 0;
  s->nchunks = s->chunk_len = 0;
}

// ------------------------------------------------------------------ upload helpers
// indices as the caller stores them (4 or 8 bytes) -> int32, checked against [0, limit); offsets -> int64
// (src may be dst when the indices already take 4 bytes: the pass then only checks)
__global__ __launch_bounds__(256) void k_narrow_idx(const void* src, int index_bytes, int64_t count, int64_t limit, int32_t* dst,
                                                    int* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const int64_t v = index_bytes == 8 ? static_cast<const int64_t*>(src)[i] : (int64_t) static_cast<const int32_t*>(src)[i];
    if (v < 0 || v >= limit) {
      atomicOr(bad, 1);
      dst[i] = 0;
    } else {
      dst[i] = (int32_t)v;
    }
  }
}

// CSR -> gene-major, stable in the cell index.  The cells are cut into B blocks of rows_per_block rows:
//   k_tr_count  cnt[b][g] = entries of gene g in block b (integer atomics)
//   k_tr_scan   per gene: cnt[b][g] -> entries of g in the blocks before b; total[g]
//   k_tr_fill   one workgroup per block walks its rows IN ORDER (a barrier between two rows): an entry of gene g goes to
//               gptr[g] + cursor[b][g]++.  A row names a gene once (canonical input), so within a gene the cells ascend.
__global__ __launch_bounds__(256) void k_tr_count(const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx, int64_t n,
                                                  int64_t G, int64_t rows_per_block, unsigned int* __restrict__ cnt) {
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  if (r0 >= r1) return;
  unsigned int* mine = cnt + (int64_t)blockIdx.x * G;
  for (int64_t e = rptr[r0] + threadIdx.x; e < rptr[r1]; e += blockDim.x) atomicAdd(mine + ridx[e], 1u);
}

__global__ __launch_bounds__(256) void k_tr_scan(unsigned int* __restrict__ cnt, int64_t G, int B, int64_t* __restrict__ total) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  int64_t run = 0;
  for (int b = 0; b < B; ++b) {
    const unsigned int t = cnt[(int64_t)b * G + g];
    cnt[(int64_t)b * G + g] = (unsigned int)run;
    run += t;
  }
  total[g] = run;
}

template <typename T>
__global__ __launch_bounds__(256) void k_tr_fill(const int64_t* __restrict__ rptr, const int32_t* __restrict__ ridx,
                                                 const T* __restrict__ rval, int64_t n, int64_t G, int64_t rows_per_block,
                                                 unsigned int* __restrict__ cnt, const int64_t* __restrict__ gptr,
                                                 int32_t* __restrict__ gcell, T* __restrict__ gval) {
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  unsigned int* mine = cnt + (int64_t)blockIdx.x * G;
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t lo = rptr[r], hi = rptr[r + 1];
    for (int64_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
      const int32_t g = ridx[e];
      const int64_t pos = gptr[g] + (int64_t)atomicAdd(mine + g, 1u);
      gcell[pos] = (int32_t)r;
      gval[pos] = rval[e];
    }
    __syncthreads();
  }
}

// offsets the caller stores in 4 or 8 bytes -> int64 on the host, checked: start at 0, never fall, end at nnz
bool widen_offsets(const void* p, int index_bytes, int64_t count, int64_t nnz, std::vector<int64_t>& out) {
  out.resize((size_t)count);
  for (int64_t i = 0; i < count; ++i)
    out[(size_t)i] = index_bytes == 8 ? static_cast<const int64_t*>(p)[i] : (int64_t) static_cast<const int32_t*>(p)[i];
  if (out[0] != 0 || out[(size_t)count - 1] != nnz) return false;
  for (int64_t i = 1; i < count; ++i)
    if (out[(size_t)i] < out[(size_t)i - 1]) return false;
  return true;
}

// chunks of the gene lists (Appendix B's split rule: a list longer than a chunk is cut into fixed chunks summed by
// separate waves, the partials are added in chunk order)
int build_chunks(cna_ctx* c, ExprState* s, const std::vector<int64_t>& gptr) {
  const int64_t waves = 256 * 16;
  int64_t len = s->nnz / (waves * 4);
  len = std::max<int64_t>(1024, std::min<int64_t>(65536, len));
  len = (len + 63) / 64 * 64;
  std::vector<int64_t> lo, first((size_t)s->G + 1);
  std::vector<int32_t> gene;
  for (int64_t g = 0; g < s->G; ++g) {
    first[(size_t)g] = (int64_t)lo.size();
    for (int64_t e = gptr[(size_t)g]; e < gptr[(size_t)g + 1]; e += len) {
      lo.push_back(e);
      gene.push_back((int32_t)g);
    }
  }
  first[(size_t)s->G] = (int64_t)lo.size();
  s->gchunk_h = first;
  s->nchunks = (int64_t)lo.size();
  s->chunk_len = len;
  CNA_TRY(buf_need(c, s->st, s->chunk_lo, 8 * std::max<int64_t>(1, s->nchunks)));
  CNA_TRY(buf_need(c, s->st, s->chunk_gene, 4 * std::max<int64_t>(1, s->nchunks)));
  CNA_TRY(buf_need(c, s->st, s->gchunk, 8 * (s->G + 1)));
  if (s->nchunks) {
    HIP_TRY(hipMemcpyAsync(s->chunk_lo.p, lo.data(), 8 * (size_t)s->nchunks, hipMemcpyHostToDevice, s->st));
    HIP_TRY(hipMemcpyAsync(s->chunk_gene.p, gene.data(), 4 * (size_t)s->nchunks, hipMemcpyHostToDevice, s->st));
  }
  HIP_TRY(hipMemcpyAsync(s->gchunk.p, first.data(), 8 * (size_t)(s->G + 1), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  return 0;
}

// the caller's indices (4 or 8 bytes each) on the device as int32 in dst, checked against [0, limit): *bad |= 1.  Indices of
// 8 bytes pass through `wide`, those of 4 are checked where they lie
int upload_indices(cna_ctx* c, ExprState* s, const void* indices, int index_bytes, int64_t nnz, int64_t limit, Buf& wide,
                   int32_t* dst, int* bad) {
  const int64_t nz1 = std::max<int64_t>(1, nnz);
  void* src = dst;
  if (index_bytes == 8) {
    CNA_TRY(buf_need(c, s->st, wide, 8 * nz1));
    src = wide.p;
  }
  HIP_TRY(hipMemcpyAsync(src, indices, (size_t)(index_bytes * nnz), hipMemcpyHostToDevice, s->st));
  hipLaunchKernelGGL(k_narrow_idx, dim3((unsigned)std::min<int64_t>((nz1 + 255) / 256, 1 << 20)), dim3(256), 0, s->st,
                     (const void*)src, index_bytes, nnz, limit, dst, bad);
  HIP_TRY(hipGetLastError());
  return 0;
}

// gptr, gcell, gval of the state from a CSC upload as it is, from a CSR upload by the counting transpose; gptr_h: the
// offsets on the host.  The temporaries are gone when this returns, whichever way.
int upload_lists(cna_ctx* c, ExprState* s, const std::vector<int64_t>& off, const void* indices, const void* data,
                 int index_bytes, int is_csc, std::vector<int64_t>& gptr_h) {
  const int64_t n = s->n, G = s->G, nnz = s->nnz;
  const int64_t vb = s->is_f64 ? 8 : 4;
  const int64_t nz1 = std::max<int64_t>(1, nnz);
  ScopedBufs tmp(c, s->st);
  Buf raw_idx{tmp}, raw_val{tmp}, rptr{tmp}, ridx{tmp}, cnt{tmp}, total{tmp}, bad{tmp};
  CNA_TRY(buf_need(c, s->st, bad, 256));
  HIP_TRY(hipMemsetAsync(bad.p, 0, 4, s->st));
  CNA_TRY(buf_need(c, s->st, s->gptr, 8 * (G + 1)));
  CNA_TRY(buf_need(c, s->st, s->gcell, 4 * nz1));
  CNA_TRY(buf_need(c, s->st, s->gval, vb * nz1));
  int bad_h = 0;
  if (is_csc) {
    // gene-major already: the cell of every entry, narrowed to 4 bytes and checked on the device
    CNA_TRY(upload_indices(c, s, indices, index_bytes, nnz, n, raw_idx, s->gcell.as<int32_t>(), bad.as<int>()));
    HIP_TRY(hipMemcpyAsync(s->gval.p, data, (size_t)(vb * nnz), hipMemcpyHostToDevice, s->st));
    HIP_TRY(hipMemcpyAsync(&bad_h, bad.p, 4, hipMemcpyDeviceToHost, s->st));
    HIP_TRY(hipStreamSynchronize(s->st));
    if (bad_h) CNA_FAIL(CNA_EINVAL, "expression matrix: a row index lies outside [0, n_cells)");
    gptr_h = off;
    HIP_TRY(hipMemcpyAsync(s->gptr.p, gptr_h.data(), 8 * (size_t)(G + 1), hipMemcpyHostToDevice, s->st));
    return 0;
  }
  // the transpose needs the rows' indices and values beside the gene-major copy for a moment
  CNA_TRY(buf_need(c, s->st, rptr, 8 * (n + 1)));
  CNA_TRY(buf_need(c, s->st, ridx, 4 * nz1));
  CNA_TRY(buf_need(c, s->st, raw_val, vb * nz1));
  HIP_TRY(hipMemcpyAsync(rptr.p, off.data(), 8 * (size_t)(n + 1), hipMemcpyHostToDevice, s->st));
  CNA_TRY(upload_indices(c, s, indices, index_bytes, nnz, G, raw_idx, ridx.as<int32_t>(), bad.as<int>()));
  HIP_TRY(hipMemcpyAsync(raw_val.p, data, (size_t)(vb * nnz), hipMemcpyHostToDevice, s->st));
  HIP_TRY(hipMemcpyAsync(&bad_h, bad.p, 4, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  if (bad_h) CNA_FAIL(CNA_EINVAL, "expression matrix: a column index lies outside [0, n_genes)");
  buf_free(c, raw_idx);
  // blocks of rows: at most 2048, and a counter table of at most 64M words
  int64_t B = std::min<int64_t>(2048, std::max<int64_t>(1, (64ll << 20) / G));
  B = std::min<int64_t>(B, n);
  const int64_t rpb = (n + B - 1) / B;
  B = (n + rpb - 1) / rpb;
  CNA_TRY(buf_need(c, s->st, cnt, 4 * B * G));
  CNA_TRY(buf_need(c, s->st, total, 8 * G));
  HIP_TRY(hipMemsetAsync(cnt.p, 0, (size_t)(4 * B * G), s->st));
  hipLaunchKernelGGL(k_tr_count, dim3((unsigned)B), dim3(256), 0, s->st, rptr.as<const int64_t>(), ridx.as<const int32_t>(), n, G,
                     rpb, cnt.as<unsigned int>());
  launch_block_scan(s->st, cnt.as<unsigned int>(), G, (int)B, total.as<int64_t>());
  HIP_TRY(hipGetLastError());
  std::vector<int64_t> tot((size_t)G);
  HIP_TRY(hipMemcpyAsync(tot.data(), total.p, 8 * (size_t)G, hipMemcpyDeviceToHost, s->st));
  HIP_TRY(hipStreamSynchronize(s->st));
  gptr_h.assign((size_t)G + 1, 0);
  for (int64_t g = 0; g < G; ++g) gptr_h[(size_t)g + 1] = gptr_h[(size_t)g] + tot[(size_t)g];
  if (gptr_h[(size_t)G] != nnz) CNA_FAIL(CNA_EINVAL, "expression matrix: the transpose lost entries (internal error)");
  HIP_TRY(hipMemcpyAsync(s->gptr.p, gptr_h.data(), 8 * (size_t)(G + 1), hipMemcpyHostToDevice, s->st));
  with_bool(s->is_f64 != 0, [&](auto f64) {
    using T = std::conditional_t<decltype(f64)::value, double, float>;
    hipLaunchKernelGGL(k_tr_fill<T>, dim3((unsigned)B), dim3(256), 0, s->st, rptr.as<const int64_t>(), ridx.as<const int32_t>(),
                       raw_val.as<const T>(), n, G, rpb, cnt.as<unsigned int>(), s->gptr.as<const int64_t>(),
                       s->gcell.as<int32_t>(), s->gval.as<T>());
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->st));
  return 0;
}

int upload_sparse(cna_ctx* c, ExprState* s, const void* indptr, const void* indices, const void* data, int64_t n, int64_t G,
                  int64_t nnz, int index_bytes, int is_f64, int is_csc) {
  std::vector<int64_t> off, gptr_h;
  if (!widen_offsets(indptr, index_bytes, (is_csc ? G : n) + 1, nnz, off))
    CNA_FAIL(CNA_EINVAL, "expression matrix: indptr must start at 0, never fall and end at nnz");
  s->n = n; s->G = G; s->nnz = nnz; s->is_f64 = is_f64;
  CNA_TRY(upload_lists(c, s, off, indices, data, index_bytes, is_csc, gptr_h));
  return build_chunks(c, s, gptr_h);
}

}  // namespace

// The pieces the resident matrix is cut into, beside build_chunks' rule for the lists: the partial sums a gene-major
// kernel keeps at a time (gene_tiles), the cells of one bin that one workgroup of the dense per-bin kernel adds up
constexpr int64_t PB_PART_BYTES = 256ll << 20;
constexpr int64_t PB_DENSE_CHUNK = 2048;

void buf_free(cna_ctx* c, Buf& b) {
  if (b.p) dev_free(c, b.p, (size_t)b.cap);
  b.p = nullptr;
  b.cap = 0;
}

void bufs_free(cna_ctx* c, BufSet& set) {
  for (Buf* b : set.all) buf_free(c, *b);
}

int buf_need(cna_ctx* c, hipStream_t st, Buf& b, int64_t bytes) {
  if (b.p && b.cap >= bytes) return 0;
  if (b.p) {
    HIP_TRY(hipStreamSynchronize(st));
    buf_free(c, b);
  }
  if (bytes < 256) bytes = 256;
  CNA_TRY(dev_alloc(c, &b.p, (size_t)bytes));
  b.cap = bytes;
  return 0;
}

void launch_block_scan(hipStream_t st, unsigned int* cnt, int64_t G, int B, int64_t* total) {
  hipLaunchKernelGGL(k_tr_scan, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, cnt, G, B, total);
}

std::vector<GeneTile> gene_tiles(const ExprState* s, int64_t record_bytes, int64_t* largest) {
  const int64_t max_chunks = std::max<int64_t>(1, PB_PART_BYTES / record_bytes);
  const std::vector<int64_t>& gc = s->gchunk_h;
  std::vector<GeneTile> tiles;
  *largest = 1;
  for (int64_t g0 = 0, g1; g0 < s->G; g0 = g1) {
    g1 = g0 + 1;
    while (g1 < s->G && gc[(size_t)g1 + 1] - gc[(size_t)g0] <= max_chunks) ++g1;
    tiles.push_back({g0, g1, gc[(size_t)g0], gc[(size_t)g1] - gc[(size_t)g0]});
    *largest = std::max(*largest, tiles.back().nch);
  }
  return tiles;
}

int fetch_results(hipStream_t st, const char* who, std::initializer_list<HostCopy> copies) {
  hipError_t e = hipGetLastError();
  for (const HostCopy& h : copies)
    if (e == hipSuccess) e = hipMemcpyAsync(h.dst, h.src, h.bytes, hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) {
    cna_set_error(std::string(who) + ": " + hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

int result_bufs_need(cna_ctx* c, hipStream_t st, std::initializer_list<BufSize> bufs) {
  for (const BufSize& b : bufs) {
    const int rc = buf_need(c, st, *b.buf, b.bytes);
    if (rc == CNA_ENOMEM) (void)hipGetLastError();
    CNA_TRY(rc);
  }
  return 0;
}

int expr_get_state(cna_ctx* c, ExprState** out) {
  if (!c->expr) {
    ExprState* s = new ExprState();
    hipError_t e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->x_ready, hipEventDisableTiming);
    if (e != hipSuccess) {
      if (s->st) (void)hipStreamDestroy(s->st);
      if (s->x_ready) (void)hipEventDestroy(s->x_ready);
      delete s;
      cna_set_error(std::string("hipStreamCreate: ") + hipGetErrorString(e));
      return (int)e;
    }
    c->expr = s;
  }
  *out = expr_state(c);
  return 0;
}

void expr_destroy(cna_ctx* c) {
  ExprState* s = expr_state(c);
  if (!s) return;
  release_matrix(c, s);
  if (s->st) (void)hipStreamDestroy(s->st);
  if (s->x_ready) (void)hipEventDestroy(s->x_ready);
  delete s;
  c->expr = nullptr;
}

extern "C" {

int cna_expr_drop(cna_ctx* c) {
  CHECK_CTX(c);
  if (expr_state(c)) release_matrix(c, expr_state(c));
  return 0;
}

int cna_expr_shape(cna_ctx* c, int64_t* n_cells, int64_t* n_genes, int64_t* nnz, int* format, int* is_f64, int64_t* n_uploads) {
  CHECK_CTX(c);
  const ExprState* s = expr_state(c);
  if (n_cells) *n_cells = s ? s->n : 0;
  if (n_genes) *n_genes = s ? s->G : 0;
  if (nnz) *nnz = s ? s->nnz : 0;
  if (format) *format = s ? s->format : 0;
  if (is_f64) *is_f64 = s ? s->is_f64 : 0;
  if (n_uploads) *n_uploads = s ? s->n_uploads : 0;
  return 0;
}

int cna_expr_upload_dense(cna_ctx* c, const void* x, int64_t n_cells, int64_t n_genes, int is_f64) {
  CHECK_CTX(c);
  if (!x) CNA_FAIL(CNA_EINVAL, "expression matrix: null pointer");
  if (n_cells < 1 || n_genes < 1 || n_cells >= (1ll << 31) || n_genes >= (1ll << 31))
    CNA_FAIL(CNA_EINVAL, "expression matrix: cells and genes must lie in [1, 2^31)");
  ExprState* s = nullptr;
  CNA_TRY(expr_get_state(c, &s));
  release_matrix(c, s);
  const int64_t bytes = n_cells * n_genes * (is_f64 ? 8 : 4);
  int rc = buf_need(c, s->st, s->X, bytes);
  if (rc != 0) {
    release_matrix(c, s);
    if (rc == CNA_ENOMEM)
      cna_set_error("expression matrix: " + std::to_string(bytes) + " bytes do not fit on the device; nothing is resident");
    return rc;
  }
  hipError_t e = hipMemcpyAsync(s->X.p, x, (size_t)bytes, hipMemcpyHostToDevice, s->st);
  if (e == hipSuccess) e = hipStreamSynchronize(s->st);
  if (e != hipSuccess) {
    release_matrix(c, s);
    cna_set_error(std::string("expression matrix upload: ") + hipGetErrorString(e));
    return (int)e;
  }
  s->format = 1;
  s->is_f64 = is_f64 != 0;
  s->n = n_cells; s->G = n_genes; s->nnz = n_cells * n_genes;
  s->n_uploads += 1;
  return 0;
}

int cna_expr_upload_sparse(cna_ctx* c, const void* indptr, const void* indices, const void* data, int64_t n_cells,
                           int64_t n_genes, int64_t nnz, int index_bytes, int is_f64, int is_csc) {
  CHECK_CTX(c);
  if (!indptr || (nnz > 0 && (!indices || !data))) CNA_FAIL(CNA_EINVAL, "expression matrix: null pointer");
  if (n_cells < 1 || n_genes < 1 || n_cells >= (1ll << 31) || n_genes >= (1ll << 31) || nnz < 0)
    CNA_FAIL(CNA_EINVAL, "expression matrix: cells and genes must lie in [1, 2^31), nnz in [0, 2^63)");
  if (index_bytes != 4 && index_bytes != 8) CNA_FAIL(CNA_EINVAL, "expression matrix: indices take 4 or 8 bytes");
  ExprState* s = nullptr;
  CNA_TRY(expr_get_state(c, &s));
  release_matrix(c, s);
  const int rc = upload_sparse(c, s, indptr, indices, data, n_cells, n_genes, nnz, index_bytes, is_f64 != 0, is_csc != 0);
  if (rc != 0) {
    const std::string why = cna_last_error();
    release_matrix(c, s);
    if (rc == CNA_ENOMEM)
      cna_set_error("expression matrix: the device has no room for the gene-major copy" +
                    std::string(is_csc ? "" : " and the rows it is transposed from") + " (" + why + "); nothing is resident");
    return rc;
  }
  s->format = 2;
  s->n_uploads += 1;
  return 0;
}

}  // extern "C"
