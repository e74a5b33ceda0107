// extern "C" entry points of libcna_hip.so (see include/cna_hip.h for the contract): the core -- context, allocator, profiler,
// the transitions of derived state and the fetches.  The walk is in walk.hip, the producers of X in xprod.hip, the host
// side of the Gram matrix and the F-tests in gram_host.hip.
#include "common.h"
#include <cstring>

static thread_local std::string g_err;
void cna_set_error(const std::string& msg) { g_err = msg; }

// ------------------------------------------------------------------ memory / profiling
// Two host threads may use one context at a time (the association's helper thread conditions the
// phenotypes -- its own buffers, the second stream -- while the main thread launches kernels): the
// allocator's bookkeeping and the alloc / free calls themselves are serialised by c->alloc_mu.  Each
// buffer still has one owner: the helper only ever (re)allocates zc and gt.
int dev_alloc(cna_ctx* c, void** p, size_t bytes) {
  std::lock_guard<std::recursive_mutex> lk(c->alloc_mu);
  *p = nullptr;
  if (bytes == 0) bytes = 256;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    cna_set_error(std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    return CNA_ENOMEM;
  }
  c->dev_bytes += (int64_t)bytes;
  return 0;
}
int dev_free(cna_ctx* c, void* p, size_t bytes) {
  std::lock_guard<std::recursive_mutex> lk(c->alloc_mu);
  if (p) {
    (void)hipFree(p);
    c->dev_bytes -= (int64_t)(bytes ? bytes : 256);
  }
  return 0;
}

int dev_reserve(cna_ctx* c, void** p, int64_t* cap, int64_t need) {
  std::lock_guard<std::recursive_mutex> lk(c->alloc_mu);
  if (need <= *cap && *p) return 0;
  if (*p) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    dev_free(c, *p, (size_t)*cap);
    *p = nullptr;
    *cap = 0;
  }
  if (need < 256) need = 256;
  CNA_TRY(dev_alloc(c, p, (size_t)need));
  *cap = need;
  return 0;
}

static hipEvent_t ev_get(cna_ctx* c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
void prof_begin(cna_ctx* c, int kid, hipStream_t st) {
  std::lock_guard<std::mutex> lock(c->prof_mu);
  ProfSpan s;
  s.kid = kid;
  s.a = ev_get(c);
  s.b = ev_get(c);
  (void)hipEventRecord(s.a, st);
  c->prof_pending.push_back(s);
}
void prof_end(cna_ctx* c, int kid, hipStream_t st) {
  std::lock_guard<std::mutex> lock(c->prof_mu);
  for (size_t i = c->prof_pending.size(); i-- > 0;) {
    if (c->prof_pending[i].kid == kid) {
      (void)hipEventRecord(c->prof_pending[i].b, st);
      return;
    }
  }
}
static void prof_flush(cna_ctx* c) {
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->copy_stream);
  if (c->coef_stream) (void)hipStreamSynchronize(c->coef_stream);
  if (c->gram_stream) (void)hipStreamSynchronize(c->gram_stream);
  if (c->halo_stream) (void)hipStreamSynchronize(c->halo_stream);
  std::lock_guard<std::mutex> lock(c->prof_mu);
  if (c->prof_pending.empty()) return;
  for (auto& s : c->prof_pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
      c->prof_ms[s.kid] += ms;
      c->prof_n[s.kid] += 1;
    }
    c->ev_pool.push_back(s.a);
    c->ev_pool.push_back(s.b);
  }
  c->prof_pending.clear();
}

static const char* kKernelNames[CNA_K_COUNT] = {
    "colsum", "nam_first", "nam_step", "batch_kurtosis", "zero_variance", "select", "resid_xb",
    "standardize", "gram", "gram_reduce", "ncorrs", "null_local", "obs_counts", "percell_fdr",
    "project_xb", "transpose", "rccl", "condition", "global_test", "nam_step_sparse", "halo_exchange", "halo_wait",
    "matrix_bins_sort", "matrix_bins_sum", "enrich_positions", "enrich_extremes", "expr_cross_by", "gram_by",
    "raster_upload", "raster", "raster_fetch",
    "components_upload", "components_hook", "components_flatten", "components_check", "components_tally", "components_label",
    "components_fetch", "ranksum_keys", "ranksum_sort", "ranksum_rank", "ranksum_fetch",
    "ranksum_pairs", "rankcorr_keys", "rankcorr_corr"};

// Derived state holds only as long as what it was derived from.  Four nested transitions, and void_x_nam_link beside them,
// are the only places that clear it (common.h tags every flag with the innermost transition that clears it); they assign
// fields and nothing else.
void void_coef(cna_ctx* c) {       // the per-cell columns copied from the coefficients (new coefficients on the same X: cna_ncorrs)
  c->cells.coef_early = false;
  c->cells.fdr_inline = false;
}
void void_x(cna_ctx* c) {          // X and everything derived from it
  c->x_valid = c->x_from_nam = c->x_ident = false;
  c->ncorrs_valid = c->xq_valid = c->byp_valid = c->gram_pre = c->proj_valid = false;
  c->gram_n = 0;
  void_coef(c);
  c->x_gen = c->x_gen + 1;         // (what callers key their own memos of X-derived results with: cna_x_generation)
}
void void_walk(cna_ctx* c) {       // the walk (state, NAM), then X
  c->t_valid = c->nam_valid = c->nam_lazy = false;
  c->steps_done = 0;
  c->t_f32[0] = c->t_f32[1] = false;
  void_x(c);
}
void void_cells(cna_ctx* c) {      // the cell space the first step reads, then the walk
  c->cellinfo_valid = false;
  void_walk(c);
}
// What ties X to the NAM that a walk step is about to replace: X itself stands (the step does not write it, unless it is armed
// to -- and then through x_begin), but it is no longer the by-product of a walk's last step, no longer a function of the
// resident NAM, and neither a second run of a last step nor the Gram matrix taken under one belongs to the new NAM.
void void_x_nam_link(cna_ctx* c) {
  c->byp_valid = false;
  c->x_ident = false;
  c->nam_lazy = false;
  c->gram_pre = false;
}

// Every producer of X brackets its work with x_begin (refused while a local-null pass is pending; whatever was derived
// from the old X goes) and x_commit (the flags the producer vouches for).  A producer that fails in between leaves X
// invalid.  In place: the shape stays.
int x_begin(cna_ctx* c, const char* who) {
  NO_NULL_PENDING(c, who);
  void_x(c);
  return 0;
}
// Row stride of the working matrix X: a multiple of 4 (MFMA k-depth).  Beyond 128 samples a stride
// that is a multiple of 256 bytes sends the 16 rows of every MFMA A tile to the same memory channels
// (local null at N = 160 / 192 / 224: 37.6 TFLOP/s; with one more quad of zero columns 51 / 56 / 57);
// up to 128 samples the plain stride is as fast or faster (measured at 64, 96, 128).  N = 256 stays
// as it is: the MFMA kernels' instantiations end at 64 quads.
int x_ld(int Nx) {
  int ld = round_up(Nx, 4);
  if (ld > 128 && (ld * 8) % 256 == 0 && ld + 4 <= 256) ld += 4;
  return ld;
}
// ... a new shape: nx rows (the local NAM rows keep_idx[0 .. nx), or every local row when keep_idx is null) x Nx samples
int x_begin(cna_ctx* c, const char* who, int64_t nx, int Nx, const int64_t* keep_idx) {
  CNA_TRY(x_begin(c, who));
  c->nx = nx;
  c->Nx = Nx;
  c->ldx = x_ld(Nx);
  void* xp = c->X;
  CNA_TRY(dev_reserve(c, &xp, &c->x_cap, (int64_t)sizeof(double) * std::max<int64_t>(nx, 1) * c->ldx));
  c->X = (double*)xp;
  c->keep_idx = nullptr;
  if (keep_idx) {
    void* kp = c->keep_store;
    CNA_TRY(dev_reserve(c, &kp, &c->keep_cap, 8 * std::max<int64_t>(nx, 1)));
    c->keep_store = (int64_t*)kp;
    HIP_TRY(hipMemcpyAsync(c->keep_store, keep_idx, 8 * nx, hipMemcpyHostToDevice, c->stream));
    c->keep_idx = c->keep_store;
  }
  return 0;
}
void x_commit(cna_ctx* c, bool from_nam, bool ncorrs, bool xq, bool ident) {
  c->x_valid = true;
  c->x_from_nam = from_nam;
  c->ncorrs_valid = ncorrs;
  c->xq_valid = xq;
  c->x_ident = ident;
}

// concatenate count_local doubles from every rank (rank order) into a host buffer
static int ragged_gather(cna_ctx* c, const double* src_dev, int64_t count_local, double* out, int64_t n_expected) {
  NO_NULL_PENDING(c, "cna_fetch_cell_stat / cna_allgather_host");
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, 256 * 2 + 8 * c->nranks));
  int64_t* cnt_dev = (int64_t*)c->scratch;
  std::vector<int64_t> cnt(c->nranks, 0);
  cnt[c->rank] = count_local;
  HIP_TRY(hipMemcpyAsync(cnt_dev, cnt.data(), 8 * c->nranks, hipMemcpyHostToDevice, c->stream));
  CNA_TRY(comm_allreduce_i64_sum(c, cnt_dev, c->nranks));
  HIP_TRY(hipMemcpyAsync(cnt.data(), cnt_dev, 8 * c->nranks, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  int64_t mx = 1, tot = 0;
  for (auto v : cnt) { mx = std::max(mx, v); tot += v; }
  if (tot != n_expected) CNA_FAIL(CNA_EINVAL, "ragged gather: expected total does not match the ranks' counts");
  CNA_TRY(dev_reserve(c, &c->scratch2, &c->scratch2_cap, 8 * mx * c->nranks));
  double* all = (double*)c->scratch2;
  if (count_local > 0)
    HIP_TRY(hipMemcpyAsync(all + mx * c->rank, src_dev, 8 * count_local, hipMemcpyDeviceToDevice, c->stream));
  CNA_TRY(comm_allgather_bytes(c, all + mx * c->rank, all, 8 * mx));
  std::vector<double> host(mx * c->nranks);
  HIP_TRY(hipMemcpyAsync(host.data(), all, 8 * mx * c->nranks, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  int64_t o = 0;
  for (int r = 0; r < c->nranks; ++r) {
    std::memcpy(out + o, host.data() + mx * r, 8 * cnt[r]);
    o += cnt[r];
  }
  return 0;
}

extern "C" {

const char* cna_last_error(void) { return g_err.c_str(); }
int cna_abi_version(void) { return 1; }
const char* cna_kernel_name(int k) { return (k >= 0 && k < CNA_K_COUNT) ? kKernelNames[k] : "?"; }

int cna_device_count(int* count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    cna_set_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return (int)e;
  }
  *count = n;
  return 0;
}

int cna_ctx_create(int device, cna_ctx** out) {
  if (!out) CNA_FAIL(CNA_EINVAL, "null out pointer");
  *out = nullptr;
  int n = 0;
  CNA_TRY(cna_device_count(&n));
  if (n <= 0) CNA_FAIL(CNA_EINVAL, "no HIP device visible: cna_amd has no CPU fallback");
  if (device < 0 || device >= n) CNA_FAIL(CNA_EINVAL, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  cna_ctx* c = new cna_ctx();
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) {
    // the second stream carries short sample-space kernels (F-tests, conditioning) that should slip in
    // between the workgroup rounds of a long kernel on the main stream: highest priority
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    e = hipStreamCreateWithPriority(&c->copy_stream, hipStreamNonBlocking, hi);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->coef_stream, hipStreamNonBlocking);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->gram_done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->cells.coef_ready, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->gt_done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->scal_ready, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->stage_done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->cells.coef_copied, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->null_done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->cells.bins_copied, hipEventDisableTiming);
  if (e != hipSuccess) {
    delete c;
    cna_set_error(std::string("hipStreamCreate: ") + hipGetErrorString(e));
    return (int)e;
  }
  *out = c;
  return 0;
}

int cna_ctx_destroy(cna_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->gram_stream) (void)hipStreamSynchronize(c->gram_stream);
  if (c->auto_state) { (void)hipFree(c->auto_state); c->auto_state = nullptr; }
  if (c->byp_buf) { (void)hipFree(c->byp_buf); c->byp_buf = nullptr; }
  if (c->pair_buf) { (void)hipFree(c->pair_buf); c->pair_buf = nullptr; }
  prof_flush(c);
  comm_destroy(c);
  expr_destroy(c);
  void* bufs[] = {c->halo_rows_safe, c->halo_rows_need, c->idx_t, c->i8_buf, c->xq, c->xq_scale, c->cells.coef_dev, c->proj, c->sp_pair, c->sp_cnt, c->null_part, c->rp16_buf, c->halo_send_idx, c->halo_recv_idx, c->halo_rows_b, c->halo_rows_i, c->halo_sbuf, c->halo_rbuf, c->orig_idx, c->indptr, c->indices, c->data, c->colsum, c->sid, c->counts, c->T[0], c->T[1], c->dense_s,
                  c->nam, c->X, c->X2, c->resid_f, c->keep_store, c->stat, c->ncorrs, c->scratch, c->scratch2, c->cellinfo, c->zc, c->gt, c->gram_tiles_ptr, c->gram_buf, c->gram_part, c->cells.bins_dev};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  for (auto e : c->ev_pool) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(c->stream);
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->coef_stream) (void)hipStreamDestroy(c->coef_stream);
  if (c->gram_done) (void)hipEventDestroy(c->gram_done);
  if (c->gt_done) (void)hipEventDestroy(c->gt_done);
  if (c->scal_ready) (void)hipEventDestroy(c->scal_ready);
  if (c->stage_done) (void)hipEventDestroy(c->stage_done);
  if (c->h_gt) (void)hipHostFree(c->h_gt);
  if (c->null_done) (void)hipEventDestroy(c->null_done);
  if (c->gram_stream) (void)hipStreamDestroy(c->gram_stream);
  for (hipEvent_t e : {c->gram_pre_done, c->range_done, c->cells.coef_ready, c->cells.coef_copied, c->cells.bins_copied})
    if (e) (void)hipEventDestroy(e);
  if (c->halo_stream) (void)hipStreamDestroy(c->halo_stream);
  if (c->halo_e1) (void)hipEventDestroy(c->halo_e1);
  if (c->halo_e2) (void)hipEventDestroy(c->halo_e2);
  if (c->cells.h_bins) (void)hipHostFree(c->cells.h_bins);
  if (c->cells.h_tab) (void)hipHostFree(c->cells.h_tab);
  if (c->h_res) (void)hipHostFree(c->h_res);
  if (c->h_scal) (void)hipHostFree(c->h_scal);
  if (c->h_gram) (void)hipHostFree(c->h_gram);
  if (c->h_hint) (void)hipHostFree(c->h_hint);
  if (c->cells.h_cell) (void)hipHostFree(c->cells.h_cell);
  delete c;
  return 0;
}

int cna_ctx_sync(cna_ctx* c) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  CNA_TRY(halo_settle(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->gram_stream && c->gram_pre_pending) HIP_TRY(hipStreamSynchronize(c->gram_stream));
  return 0;
}

int cna_ctx_device_bytes(cna_ctx* c, int64_t* bytes) {
  if (!c || !bytes) CNA_FAIL(CNA_EINVAL, "null argument");
  *bytes = c->dev_bytes.load();
  return 0;
}

int cna_x_generation(cna_ctx* c, int64_t* gen) {
  if (!c || !gen) CNA_FAIL(CNA_EINVAL, "null argument");
  *gen = c->x_gen;
  return 0;
}

int cna_set_state_f32(cna_ctx* c, int on) {
  CHECK_CTX(c);
  // takes effect at the next step that writes the state: every buffer carries its own format (t_f32), so a walk in
  // progress stays consistent; the caller decides what a NAM already on the device is worth (engine.set_state_f32)
  c->state_f32_mode = on != 0;
  return 0;
}

int cna_fetch_cell_stat(cna_ctx* c, double* out, int64_t n_expected) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  const bool nam = c->stat_space == CNA_MAT_NAM;
  if (!nam && c->stat_space != CNA_MAT_X) CNA_FAIL(CNA_ESTATE, "no per-cell statistic available");
  if (!nam && c->nranks > 1 && !c->local_view) return ragged_gather(c, c->stat, c->nx, out, n_expected);
  // NAM space: every rank holds all n_global entries, a local view takes its own block of them; X space: this rank's rows
  const int64_t n = !nam ? c->nx : c->local_view ? c->n_local : c->n_global;
  const char* name = !nam ? "nx" : c->local_view ? "n_local" : "n_global";
  if (n_expected != n) CNA_FAIL(CNA_EINVAL, std::string("cna_fetch_cell_stat: expected ") + name + " entries");
  HIP_TRY(hipMemcpyAsync(out, c->stat + (nam && c->local_view ? c->row0 : 0), sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// For tests: the caller's own vector as the NAM-space per-cell statistic, so that the medians and the QC count below
// can be fed values no kurtosis kernel produces (one rank holding the whole graph: n_global entries, device cell order)
int cna_load_cell_stat(cna_ctx* c, const double* v, int64_t n) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_load_cell_stat");
  AUTO_FINISH(c);
  if (!c->indptr || !c->stat) CNA_FAIL(CNA_ESTATE, "cna_load_cell_stat before cna_graph_upload");
  if (c->nranks != 1 || c->local_view || c->n_local != c->n_global)
    CNA_FAIL(CNA_ESTATE, "cna_load_cell_stat: one rank holding the whole graph only");
  if (!v) CNA_FAIL(CNA_EINVAL, "cna_load_cell_stat: null pointer");
  if (n != c->n_global) CNA_FAIL(CNA_EINVAL, "cna_load_cell_stat: expected n_global entries");
  HIP_TRY(hipMemcpyAsync(c->stat, v, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));      // (the caller's vector may go out of scope)
  c->stat_space = CNA_MAT_NAM;
  return 0;
}

// -------------------------------------------------------------------------------- D2H
int cna_matrix_shape(cna_ctx* c, int which, int64_t* n_rows_local, int* n_cols) {
  CHECK_CTX(c);                                  // (the NAM may be materialised here: kernels on this context's device)
  if (which == CNA_MAT_NAM) AUTO_FINISH(c);
  if (which == CNA_MAT_NAM) {
    CNA_TRY(need_nam(c));
    *n_rows_local = c->n_local; *n_cols = c->N;
  } else if (which == CNA_MAT_X) {
    if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
    *n_rows_local = c->nx; *n_cols = c->Nx;
  } else {
    CNA_FAIL(CNA_EINVAL, "bad matrix selector");
  }
  return 0;
}

int cna_fetch_matrix(cna_ctx* c, int which, double* out, int transposed) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  int64_t rows;
  int cols;
  CNA_TRY(cna_matrix_shape(c, which, &rows, &cols));
  const double* src = which == CNA_MAT_NAM ? c->nam : c->X;
  const int ld = which == CNA_MAT_NAM ? c->ld : c->ldx;
  if (rows == 0) return 0;
  if (transposed) {
    CNA_TRY(dev_reserve(c, &c->scratch2, &c->scratch2_cap, 8 * rows * cols));
    CNA_TRY(launch_transpose(c, src, rows, cols, ld, (double*)c->scratch2));
    HIP_TRY(hipMemcpyAsync(out, c->scratch2, 8 * rows * cols, hipMemcpyDeviceToHost, c->stream));
  } else {
    HIP_TRY(hipMemcpy2DAsync(out, 8 * (size_t)cols, src, 8 * (size_t)ld, 8 * (size_t)cols, rows,
                             hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// For tests: what stands in the padding columns N <= col < ld of the NAM's rows on the device (finish_row writes zeros
// there; no other fetch reaches them).  The NAM only, not the state buffers.
int cna_fetch_nam_padding(cna_ctx* c, double* out, int* n_pad_cols) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  if (!n_pad_cols) CNA_FAIL(CNA_EINVAL, "cna_fetch_nam_padding: null pointer");
  CNA_TRY(need_nam(c));
  const int pad = c->ld - c->N;
  *n_pad_cols = pad;
  if (!out || pad <= 0 || c->n_local == 0) return 0;
  HIP_TRY(hipMemcpy2DAsync(out, 8 * (size_t)pad, c->nam + c->N, 8 * (size_t)c->ld, 8 * (size_t)pad, c->n_local,
                           hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// cna_fetch_matrix with the rows (and columns) picked and ordered on the device: out[i][j] =
// matrix[rows[i]][cols[j]], or its transpose.  which = CNA_MAT_NAM / CNA_MAT_X, or CNA_MAT_PROJ for the
// result of the last cna_project_keep.  One gather kernel and one contiguous copy instead of a
// strided copy plus cells x samples sized reshuffles on the host.
int cna_fetch_rows(cna_ctx* c, int which, const int64_t* rows, int64_t n_out, const int32_t* cols, int n_cols,
                   double* out, int transposed) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  const double* src;
  int ld, width;
  int64_t have;
  if (which == CNA_MAT_PROJ) {
    if (!c->proj_valid) CNA_FAIL(CNA_ESTATE, "no projection resident (cna_project_keep)");
    src = (const double*)c->proj; ld = c->proj_ld; width = c->proj_cols; have = c->proj_rows;
  } else {
    int cc;
    CNA_TRY(cna_matrix_shape(c, which, &have, &cc));
    width = cc;
    src = which == CNA_MAT_NAM ? c->nam : c->X;
    ld = which == CNA_MAT_NAM ? c->ld : c->ldx;
  }
  if (!rows) n_out = have;
  if (!cols) n_cols = width;
  if (n_out < 0 || n_cols < 0) CNA_FAIL(CNA_EINVAL, "cna_fetch_rows: bad sizes");
  if (n_out == 0 || n_cols == 0) return 0;
  if (rows)
    for (int64_t i = 0; i < n_out; ++i)
      if (rows[i] < 0 || rows[i] >= have) CNA_FAIL(CNA_EINVAL, "cna_fetch_rows: row index out of range");
  if (cols)
    for (int j = 0; j < n_cols; ++j)
      if (cols[j] < 0 || cols[j] >= width) CNA_FAIL(CNA_EINVAL, "cna_fetch_rows: column index out of range");
  CNA_TRY(dev_reserve(c, &c->scratch2, &c->scratch2_cap, carve_bytes({8 * n_out * (int64_t)n_cols, 8 * n_out, 4 * (int64_t)n_cols})));
  Carver cv(c->scratch2);
  double* dst = cv.take<double>(n_out * (int64_t)n_cols);
  int64_t* rd = cv.take<int64_t>(n_out);
  int32_t* cd = cv.take<int32_t>(n_cols);
  if (rows) HIP_TRY(hipMemcpyAsync(rd, rows, 8 * n_out, hipMemcpyHostToDevice, c->stream));
  if (cols) HIP_TRY(hipMemcpyAsync(cd, cols, 4 * (size_t)n_cols, hipMemcpyHostToDevice, c->stream));
  CNA_TRY(launch_gather_rows(c, src, ld, rows ? rd : nullptr, n_out, cols ? cd : nullptr, n_cols, dst, transposed));
  HIP_TRY(hipMemcpyAsync(out, dst, 8 * (size_t)n_out * n_cols, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int cna_allgather_host(cna_ctx* c, const double* local, int64_t count_local, double* out_all, int64_t count_total) {
  CHECK_CTX(c);
  if (count_local < 0 || count_total < count_local) CNA_FAIL(CNA_EINVAL, "cna_allgather_host: bad counts");
  if (c->nranks == 1) {
    if (count_total != count_local) CNA_FAIL(CNA_EINVAL, "cna_allgather_host: single rank but totals differ");
    std::memcpy(out_all, local, 8 * count_local);
    return 0;
  }
  void* tmp = nullptr;
  CNA_TRY(dev_alloc(c, &tmp, 8 * std::max<int64_t>(count_local, 1)));
  int r = 0;
  if (count_local > 0) {
    hipError_t e = hipMemcpyAsync(tmp, local, 8 * count_local, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { cna_set_error(hipGetErrorString(e)); r = (int)e; }
  }
  if (r == 0) r = ragged_gather(c, (const double*)tmp, count_local, out_all, count_total);
  (void)hipStreamSynchronize(c->stream);
  dev_free(c, tmp, 8 * std::max<int64_t>(count_local, 1));
  return r;
}

// -------------------------------------------------------------------------- profiling
int cna_prof_enable(cna_ctx* c, int on) {
  if (!c) CNA_FAIL(CNA_EINVAL, "null context");
  if (!on) prof_flush(c);
  c->prof = on != 0;
  static_assert(CNA_K_COUNT <= 64, "prof_mask is one word");
  c->prof_mask = on == 2 ? (1ull << CNA_K_NAM_FIRST | 1ull << CNA_K_NAM_STEP | 1ull << CNA_K_NAM_STEP_SPARSE | 1ull << CNA_K_ALLGATHER |
                            1ull << CNA_K_HALO_EXCHANGE | 1ull << CNA_K_HALO_WAIT)
                         : ~0ull;
  return 0;
}
int cna_prof_reset(cna_ctx* c) {
  if (!c) CNA_FAIL(CNA_EINVAL, "null context");
  prof_flush(c);
  for (int i = 0; i < CNA_K_COUNT; ++i) { c->prof_ms[i] = 0; c->prof_n[i] = 0; }
  return 0;
}
int cna_prof_get(cna_ctx* c, int k, double* total_ms, int64_t* launches) {
  if (!c || k < 0 || k >= CNA_K_COUNT) CNA_FAIL(CNA_EINVAL, "bad kernel id");
  prof_flush(c);
  if (total_ms) *total_ms = c->prof_ms[k];
  if (launches) *launches = c->prof_n[k];
  return 0;
}

}  // extern "C"
