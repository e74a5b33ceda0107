// The walk on the host (extern "C" entry points of libcna_hip.so, see include/cna_hip.h): the graph and the samples, the halo
// exchange, the steps of the walk with the selection by-product of its last one, the dense diffusion, and the order
// statistics of the per-cell vector that the walk's stop rule and the QC read.  The kernels are in diffuse.hip and rows.hip.
#include "common.h"
#include <cstring>

static void halo_clear(cna_ctx* c) {
  if (c->halo_wait_pending && c->halo_stream) (void)hipStreamSynchronize(c->halo_stream);     // (nothing may still write into buffers about to go)
  c->halo_wait_pending = false;
  if (c->halo_rows_safe) dev_free(c, c->halo_rows_safe, sizeof(int32_t) * std::max<int64_t>(c->halo_nsafe, 1));
  if (c->halo_rows_need) dev_free(c, c->halo_rows_need, sizeof(int32_t) * std::max<int64_t>(c->halo_nneed, 1));
  c->halo_rows_safe = c->halo_rows_need = nullptr;
  c->halo_nsafe = c->halo_nneed = 0;
  if (c->idx_t) dev_free(c, c->idx_t, sizeof(int32_t) * std::max<int64_t>(c->idx_t_n, 1));
  c->idx_t = nullptr;
  c->idx_t_n = 0;
  if (c->t_compact) {          // the state's row space changes: whatever is in it is void
    c->t_compact = false;
    c->t_rows = 0;
    void_cells(c);
  }
  if (c->halo_send_idx) dev_free(c, c->halo_send_idx, sizeof(int64_t) * std::max<int64_t>(c->halo_ns, 1));
  if (c->halo_recv_idx) dev_free(c, c->halo_recv_idx, sizeof(int64_t) * std::max<int64_t>(c->halo_nr, 1));
  c->halo_send_idx = c->halo_recv_idx = nullptr;
  c->halo_ns = c->halo_nr = 0;
  c->halo_on = false;
  if (c->halo_rows_b) dev_free(c, c->halo_rows_b, sizeof(int32_t) * std::max<int64_t>(c->halo_nb, 1));
  if (c->halo_rows_i) dev_free(c, c->halo_rows_i, sizeof(int32_t) * std::max<int64_t>(c->halo_ni, 1));
  c->halo_rows_b = c->halo_rows_i = nullptr;
  c->halo_nb = c->halo_ni = 0;
}

// the main stream waits for an exchange still in flight on the halo stream (see cna_nam_step); no-op when none is
int halo_settle(cna_ctx* c) {
  if (!c->halo_wait_pending) return 0;
  c->halo_wait_pending = false;
  // (profiling: how long the main stream stands still here -- the part of the exchange the walk did not hide)
  ProfScope ps(c, CNA_K_HALO_WAIT);
  HIP_TRY(hipStreamWaitEvent(c->stream, c->halo_e2, 0));
  return 0;
}

// every rank gets every rank's block of the NAM-space per-cell statistic
int exchange_stat(cna_ctx* c) {
  if (c->nranks == 1) return 0;
  const size_t block = sizeof(double) * (size_t)c->rows_per_rank;
  return comm_allgather_bytes(c, (char*)c->stat + block * c->rank, c->stat, block);
}

// The NAM on the device, for whoever reads it.  A last step that left the selection pass's results instead (see
// cna_nam_select_hint) is run once more, now for the NAM: its input state is still in T[t_cur] (a step that ends a walk
// writes no state), so are the pairs of a two-step walk; same kernel, same inputs, same bits as a first run would give.
int need_nam(cna_ctx* c) {
  if (!c->nam_valid && c->nam_lazy) {
    const int done = c->steps_done;
    c->steps_done = c->lazy_steps_before;                 // launch_nam_step picks the compressed second step by it
    const int rc = launch_nam_step(c, false, false, false, true, false);
    c->steps_done = done;
    CNA_TRY(rc);
    c->nam_valid = true;
    c->nam_lazy = false;
  }
  if (!c->nam_valid) CNA_FAIL(CNA_ESTATE, "NAM not available");
  return 0;
}

// the device-side bookkeeping block of the medians (rows.hip:AutoState) + 2 x 257 histogram words behind it
int ensure_auto_state(cna_ctx* c, unsigned long long** hist) {
  const size_t sb = (auto_state_bytes() + 255) & ~(size_t)255;
  if (!c->auto_state) HIP_TRY(hipMalloc(&c->auto_state, sb + 8 * 2 * 257));
  if (hist) *hist = (unsigned long long*)((char*)c->auto_state + sb);
  return 0;
}

extern "C" {

// ------------------------------------------------------------------------------ graph
int cna_graph_upload(cna_ctx* c, int64_t n_global, int64_t row0, int64_t n_local, const int64_t* indptr,
                     const int32_t* indices, const void* data, int data_is_f64) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  if (n_global <= 0 || n_local < 0 || row0 < 0 || row0 + n_local > n_global || !indptr)
    CNA_FAIL(CNA_EINVAL, "cna_graph_upload: bad shape");
  const int64_t rpr = (n_global + c->nranks - 1) / c->nranks;
  if (row0 != (int64_t)c->rank * rpr && !(n_local == 0))
    CNA_FAIL(CNA_EINVAL, "cna_graph_upload: row0 must be rank*ceil(n/nranks)");
  const int64_t want_local = std::max<int64_t>(0, std::min(rpr, n_global - (int64_t)c->rank * rpr));
  if (n_local != want_local) CNA_FAIL(CNA_EINVAL, "cna_graph_upload: n_local must be the rank's block size");
  if (indptr[0] != 0) CNA_FAIL(CNA_EINVAL, "cna_graph_upload: indptr must be rebased to start at 0");
  const int64_t nnz = indptr[n_local];
  HIP_TRY(hipStreamSynchronize(c->stream));
  void_cells(c);
  if (c->indptr) dev_free(c, c->indptr, sizeof(int64_t) * (c->n_local + 1));
  if (c->indices) dev_free(c, c->indices, sizeof(int32_t) * c->nnz);
  if (c->data) dev_free(c, c->data, (c->data_f64 ? 8 : 4) * c->nnz);
  if (c->colsum) dev_free(c, c->colsum, sizeof(double) * c->n_pad);
  if (c->stat) dev_free(c, c->stat, sizeof(double) * c->n_pad);
  if (c->orig_idx) dev_free(c, c->orig_idx, sizeof(int64_t) * c->n_local);
  c->indptr = nullptr; c->indices = nullptr; c->data = nullptr; c->colsum = nullptr; c->stat = nullptr;
  c->orig_idx = nullptr;
  halo_clear(c);
  c->n_global = n_global;
  c->row0 = (int64_t)c->rank * rpr;
  c->n_local = n_local;
  c->rows_per_rank = rpr;
  c->n_pad = rpr * c->nranks;
  c->nnz = nnz;
  c->data_f64 = data_is_f64 ? 1 : 0;
  const size_t vb = data_is_f64 ? 8 : 4;
  CNA_TRY(dev_alloc(c, (void**)&c->indptr, sizeof(int64_t) * (n_local + 1)));
  CNA_TRY(dev_alloc(c, (void**)&c->indices, sizeof(int32_t) * nnz));
  CNA_TRY(dev_alloc(c, (void**)&c->data, vb * nnz));
  CNA_TRY(dev_alloc(c, (void**)&c->colsum, sizeof(double) * c->n_pad));
  CNA_TRY(dev_alloc(c, (void**)&c->stat, sizeof(double) * c->n_pad));
  HIP_TRY(hipMemcpy(c->indptr, indptr, sizeof(int64_t) * (n_local + 1), hipMemcpyHostToDevice));
  if (nnz > 0) {
    HIP_TRY(hipMemcpy(c->indices, indices, sizeof(int32_t) * nnz, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->data, data, vb * nnz, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemset(c->stat, 0, sizeof(double) * c->n_pad));
  c->have_colsum = false;
  return 0;
}

int cna_set_cell_order(cna_ctx* c, const int64_t* orig_index) {
  CHECK_CTX(c);
  if (!c->indptr) CNA_FAIL(CNA_ESTATE, "cna_set_cell_order before cna_graph_upload");
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!orig_index) {
    if (c->orig_idx) dev_free(c, c->orig_idx, sizeof(int64_t) * c->n_local);
    c->orig_idx = nullptr;
    return 0;
  }
  const int64_t lim = c->local_view ? c->n_local : c->n_global;
  for (int64_t i = 0; i < c->n_local; ++i)
    if (orig_index[i] < 0 || orig_index[i] >= lim)
      CNA_FAIL(CNA_EINVAL, "cna_set_cell_order: index out of range");
  if (!c->orig_idx && c->n_local > 0) CNA_TRY(dev_alloc(c, (void**)&c->orig_idx, sizeof(int64_t) * c->n_local));
  if (c->n_local > 0)
    HIP_TRY(hipMemcpy(c->orig_idx, orig_index, sizeof(int64_t) * c->n_local, hipMemcpyHostToDevice));
  return 0;
}

int cna_graph_reorder(cna_ctx* c, const int64_t* perm) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  if (!c->indptr || !perm) CNA_FAIL(CNA_ESTATE, "cna_graph_reorder before cna_graph_upload");
  if (c->nranks != 1 || c->halo_on || c->local_view || c->n_local != c->n_global || c->n_pad != c->n_global)
    CNA_FAIL(CNA_ESTATE, "cna_graph_reorder: one rank holding the whole graph only");
  if (c->orig_idx) CNA_FAIL(CNA_ESTATE, "cna_graph_reorder: the resident graph already has a device cell order");
  CNA_TRY(halo_settle(c));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->gram_stream && c->gram_pre_pending) HIP_TRY(hipStreamSynchronize(c->gram_stream));
  const int64_t n = c->n_global;
  int64_t* pd = nullptr;
  CNA_TRY(dev_alloc(c, (void**)&pd, sizeof(int64_t) * n));
  hipError_t e = hipMemcpyAsync(pd, perm, sizeof(int64_t) * n, hipMemcpyHostToDevice, c->stream);
  int rc = e == hipSuccess ? graph_reorder_device(c, pd) : (int)e;
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    dev_free(c, pd, sizeof(int64_t) * n);
    if (e != hipSuccess) cna_set_error(hipGetErrorString(e));
    return rc;
  }
  c->orig_idx = pd;                       // (what cna_set_cell_order would have uploaded)
  HIP_TRY(hipMemsetAsync(c->stat, 0, sizeof(double) * c->n_pad, c->stream));
  // everything that hangs on the order of the cells goes, as after an upload; the column sums and the sample codes were
  // permuted with the graph and stay
  void_cells(c);
  return 0;
}

int cna_set_local_view(cna_ctx* c, int on) {
  CHECK_CTX(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((on != 0) != c->local_view) {
    void_x(c);                      // (the per-cell columns derived from X are laid out for the old view)
    if (c->orig_idx) dev_free(c, c->orig_idx, sizeof(int64_t) * c->n_local);     // a cell order belongs to the view it was given in
    c->orig_idx = nullptr;
  }
  c->local_view = on != 0;
  return 0;
}

int cna_colsums(cna_ctx* c, double self_weight) {
  CHECK_CTX(c);
  if (!c->indptr) CNA_FAIL(CNA_ESTATE, "cna_colsums before cna_graph_upload");
  c->self_weight = self_weight;
  CNA_TRY(launch_colsum(c));
  CNA_TRY(comm_allreduce_f64_sum(c, c->colsum, (size_t)c->n_pad));
  CNA_TRY(launch_add_scalar(c, c->colsum, c->n_global, self_weight));
  c->have_colsum = true;
  c->cellinfo_valid = false;
  return 0;
}

int cna_fetch_colsums(cna_ctx* c, double* out) {
  CHECK_CTX(c);
  if (!c->have_colsum) CNA_FAIL(CNA_ESTATE, "colsums not computed");
  HIP_TRY(hipMemcpyAsync(out, c->colsum, sizeof(double) * c->n_global, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

static int64_t state_rows(const cna_ctx* c) { return c->t_compact ? c->t_rows : c->n_pad; }

static int ensure_T(cna_ctx* c, int ld) {
  // + 64 doubles: the gather kernel lets lanes past the row width read into the following row
  const int64_t need = (int64_t)sizeof(double) * (state_rows(c) * ld + 64);
  // (a buffer left over from a much larger row space -- the graph's halo plan came after a first allocation -- goes:
  // the point of the compact row space is the memory)
  if (need > c->t_cap || !c->T[0] || (c->t_compact && c->t_cap > need + need / 2 + (1 << 20))) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->halo_wait_pending && c->halo_stream) { HIP_TRY(hipStreamSynchronize(c->halo_stream)); c->halo_wait_pending = false; }
    for (int i = 0; i < 2; ++i) {
      if (c->T[i]) dev_free(c, c->T[i], (size_t)c->t_cap);
      c->T[i] = nullptr;
    }
    for (int i = 0; i < 2; ++i) {
      CNA_TRY(dev_alloc(c, (void**)&c->T[i], (size_t)need));
      HIP_TRY(hipMemsetAsync(c->T[i], 0, (size_t)need, c->stream));
    }
    c->t_cap = need;
  }
  return 0;
}

// The second walk step can gather a compressed copy of the state (diffuse.hip: k_nam_step_sparse).
// Worth it when rows are mostly zeros after one step, i.e. many more samples than neighbours.  Sharded over
// ranks (round 3): the exchange between ranks still carries dense rows -- the first step then writes the dense row
// of every cell as well, and the rows that arrive from other ranks are marked "dense" in sp_cnt once (this rank's
// steps only ever write the marks of its own rows), so the second step takes its local neighbours -- nine in ten
// at eight ranks -- from their pairs and the others from the dense rows the halo exchange delivered, exactly as it
// does for a row that overflowed its pairs.  Needs the halo exchange (with the all-gather fallback every row would
// be foreign).  CNA_SPARSE_MIN_N moves the switch-over (0 = never).
static int ensure_sparse_state(cna_ctx* c) {
  int min_n = 96;
  if (const char* e = getenv("CNA_SPARSE_MIN_N")) min_n = atoi(e);
  const bool multi = c->nranks > 1 || comm_active(c);
  const bool want = min_n > 0 && c->N >= min_n && (!multi || c->halo_on);
  // compact row space: counts for every row of the state (halo rows stay "dense"), pairs for this rank's own rows only
  const int64_t cnt_rows = state_rows(c), pair_rows = c->t_compact ? std::max<int64_t>(c->n_local, 1) : c->n_pad;
  if (want && c->sp_cnt && c->sp_rows == cnt_rows && c->sp_pair_rows == pair_rows) return 0;
  if (c->sp_cnt) {                         // not wanted any more, or sized for another row space
    HIP_TRY(hipStreamSynchronize(c->stream));
    dev_free(c, c->sp_pair, 16 * 64 * (size_t)c->sp_pair_rows);
    dev_free(c, c->sp_cnt, (size_t)c->sp_rows);
    c->sp_pair = c->sp_cnt = nullptr;
    c->sp_rows = c->sp_pair_rows = 0;
  }
  if (!want) return 0;
  c->sp_rows = cnt_rows;
  c->sp_pair_rows = pair_rows;
  CNA_TRY(dev_alloc(c, &c->sp_pair, 16 * 64 * (size_t)c->sp_pair_rows));   // 64 = SP_CAP records of 16 bytes (diffuse.hip)
  CNA_TRY(dev_alloc(c, &c->sp_cnt, (size_t)c->sp_rows));
  // every row "dense" (255 = SP_DENSE) until a first step of this rank says otherwise: rows of other ranks stay so
  HIP_TRY(hipMemsetAsync(c->sp_cnt, 0xff, (size_t)c->sp_rows, c->stream));
  return 0;
}

// -------------------------------------------------------------------------------- NAM
int cna_set_samples(cna_ctx* c, const int32_t* codes, int n_samples, const double* counts) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  if (!c->indptr) CNA_FAIL(CNA_ESTATE, "cna_set_samples before cna_graph_upload");
  if (n_samples < 1 || n_samples > 1024) CNA_FAIL(CNA_EINVAL, "n_samples must be in [1, 1024]");
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!c->sid || !c->counts || c->N != n_samples || c->sid_n != c->n_global) {
    if (c->sid) dev_free(c, c->sid, sizeof(int32_t) * c->sid_n);
    if (c->counts) dev_free(c, c->counts, sizeof(double) * c->N);
    c->sid = nullptr; c->counts = nullptr;
    CNA_TRY(dev_alloc(c, (void**)&c->sid, sizeof(int32_t) * c->n_global));
    CNA_TRY(dev_alloc(c, (void**)&c->counts, sizeof(double) * n_samples));
    c->sid_n = c->n_global;
  }
  c->N = n_samples;
  int ld_align = 4;
  c->ld = round_up(n_samples, ld_align);
  HIP_TRY(hipMemcpyAsync(c->sid, codes, sizeof(int32_t) * c->n_global, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->counts, counts, sizeof(double) * n_samples, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  void_cells(c);
  CNA_TRY(ensure_T(c, c->ld));
  void* nm = c->nam;
  CNA_TRY(dev_reserve(c, &nm, &c->nam_cap, (int64_t)sizeof(double) * std::max<int64_t>(c->n_local, 1) * c->ld));
  c->nam = (double*)nm;
  c->t_width = c->N;
  c->t_ld = c->ld;
  c->t_cur = 0;
  CNA_TRY(ensure_sparse_state(c));
  return 0;
}

int cna_restart_nam(cna_ctx* c) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  if (!c->sid || !c->counts) CNA_FAIL(CNA_ESTATE, "cna_restart_nam needs cna_set_samples first");
  // (no wait for the stream here: the new walk is queued behind whatever still runs on it, and ensure_T waits by itself
  // in the one case that needs it, a reallocation -- the wait cost 20-40 us at the front of every call)
  void_walk(c);
  CNA_TRY(ensure_T(c, c->ld));
  c->t_width = c->N;
  c->t_ld = c->ld;
  c->t_cur = 0;
  return 0;
}

int cna_set_halo(cna_ctx* c, const int64_t* send_rows, const int64_t* send_counts, const int64_t* recv_rows,
                 const int64_t* recv_counts) {
  CHECK_CTX(c);
  if (!c->indptr) CNA_FAIL(CNA_ESTATE, "cna_set_halo before cna_graph_upload");
  HIP_TRY(hipStreamSynchronize(c->stream));
  halo_clear(c);
  if (!send_counts || !recv_counts) return 0;
  if (!comm_active(c)) CNA_FAIL(CNA_ESTATE, "cna_set_halo needs cna_comm_init");
  int64_t ns = 0, nr = 0;
  for (int p = 0; p < c->nranks; ++p) {
    if (send_counts[p] < 0 || recv_counts[p] < 0) CNA_FAIL(CNA_EINVAL, "cna_set_halo: negative count");
    ns += send_counts[p];
    nr += recv_counts[p];
  }
  if ((ns > 0 && !send_rows) || (nr > 0 && !recv_rows)) CNA_FAIL(CNA_EINVAL, "cna_set_halo: missing row list");
  for (int64_t k = 0; k < ns; ++k)
    if (send_rows[k] < 0 || send_rows[k] >= c->n_local) CNA_FAIL(CNA_EINVAL, "cna_set_halo: send row outside the local block");
  for (int64_t k = 0; k < nr; ++k)
    if (recv_rows[k] < 0 || recv_rows[k] >= c->n_global) CNA_FAIL(CNA_EINVAL, "cna_set_halo: recv row out of range");
  CNA_TRY(dev_alloc(c, (void**)&c->halo_send_idx, sizeof(int64_t) * std::max<int64_t>(ns, 1)));
  c->halo_ns = ns;
  CNA_TRY(dev_alloc(c, (void**)&c->halo_recv_idx, sizeof(int64_t) * std::max<int64_t>(nr, 1)));
  c->halo_nr = nr;
  if (ns) HIP_TRY(hipMemcpy(c->halo_send_idx, send_rows, sizeof(int64_t) * ns, hipMemcpyHostToDevice));
  if (nr) HIP_TRY(hipMemcpy(c->halo_recv_idx, recv_rows, sizeof(int64_t) * nr, hipMemcpyHostToDevice));
  c->halo_send_cnt.assign(send_counts, send_counts + c->nranks);
  c->halo_recv_cnt.assign(recv_counts, recv_counts + c->nranks);
  c->halo_on = true;
  // the block's rows in two lists -- those some other rank has asked for, and the rest: a step that is followed by an
  // exchange walks the first list, hands its rows to the exchange and walks the second meanwhile (cna_nam_step)
  {
    std::vector<char> wanted((size_t)std::max<int64_t>(c->n_local, 1), 0);
    for (int64_t k = 0; k < ns; ++k) wanted[(size_t)send_rows[k]] = 1;
    std::vector<int32_t> rb, ri;
    for (int64_t r = 0; r < c->n_local; ++r) (wanted[(size_t)r] ? rb : ri).push_back((int32_t)r);
    c->halo_nb = (int64_t)rb.size();
    c->halo_ni = (int64_t)ri.size();
    CNA_TRY(dev_alloc(c, (void**)&c->halo_rows_b, sizeof(int32_t) * std::max<int64_t>(c->halo_nb, 1)));
    CNA_TRY(dev_alloc(c, (void**)&c->halo_rows_i, sizeof(int32_t) * std::max<int64_t>(c->halo_ni, 1)));
    if (c->halo_nb) HIP_TRY(hipMemcpy(c->halo_rows_b, rb.data(), sizeof(int32_t) * c->halo_nb, hipMemcpyHostToDevice));
    if (c->halo_ni) HIP_TRY(hipMemcpy(c->halo_rows_i, ri.data(), sizeof(int32_t) * c->halo_ni, hipMemcpyHostToDevice));
    // (the stream may exist already: cna_comm_selftest makes it for its own exchange)
    if (!c->halo_stream) HIP_TRY(hipStreamCreateWithFlags(&c->halo_stream, hipStreamNonBlocking));
    if (!c->halo_e1) HIP_TRY(hipEventCreateWithFlags(&c->halo_e1, hipEventDisableTiming));
    if (!c->halo_e2) HIP_TRY(hipEventCreateWithFlags(&c->halo_e2, hipEventDisableTiming));
  }
  // the rows that read no foreign row, and the rest (from the graph block itself: no symmetry assumed)
  if (c->n_local > 0) {
    unsigned char* fl = nullptr;
    HIP_TRY(hipMalloc(&fl, (size_t)c->n_local));
    struct Free { unsigned char* p; ~Free() { (void)hipFree(p); } } free_fl{fl};
    CNA_TRY(launch_rows_need_halo(c, fl));
    std::vector<unsigned char> hf((size_t)c->n_local);
    HIP_TRY(hipMemcpyAsync(hf.data(), fl, (size_t)c->n_local, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int32_t> rs, rn;
    for (int64_t r = 0; r < c->n_local; ++r) (hf[(size_t)r] ? rn : rs).push_back((int32_t)r);
    c->halo_nsafe = (int64_t)rs.size();
    c->halo_nneed = (int64_t)rn.size();
    CNA_TRY(dev_alloc(c, (void**)&c->halo_rows_safe, sizeof(int32_t) * std::max<int64_t>(c->halo_nsafe, 1)));
    CNA_TRY(dev_alloc(c, (void**)&c->halo_rows_need, sizeof(int32_t) * std::max<int64_t>(c->halo_nneed, 1)));
    if (c->halo_nsafe) HIP_TRY(hipMemcpy(c->halo_rows_safe, rs.data(), sizeof(int32_t) * c->halo_nsafe, hipMemcpyHostToDevice));
    if (c->halo_nneed) HIP_TRY(hipMemcpy(c->halo_rows_need, rn.data(), sizeof(int32_t) * c->halo_nneed, hipMemcpyHostToDevice));
  }
  // State for local + halo rows only: the rows this rank receives are the ONLY foreign rows its graph block
  // references (that is what the plan is), so the state needs n_local + nr rows, not n_global -- and what arrives can land
  // in the tail directly, in the order it is sent.  The walk steps read the graph through column indices renumbered
  // into that row space (one pass, here).  CNA_COMPACT_STATE=0 keeps the global row space (A/B, tests).
  {
    const char* e = getenv("CNA_COMPACT_STATE");
    bool ascending = true;
    for (int64_t k = 1; k < nr && ascending; ++k) ascending = recv_rows[k] > recv_rows[k - 1];
    for (int64_t k = 0; k < nr && ascending; ++k) ascending = recv_rows[k] < c->row0 || recv_rows[k] >= c->row0 + c->n_local;
    if (!(e && atoi(e) == 0) && ascending && c->n_local + nr < ((int64_t)1 << 31)) {
      CNA_TRY(dev_alloc(c, (void**)&c->idx_t, sizeof(int32_t) * std::max<int64_t>(c->nnz, 1)));
      c->idx_t_n = c->nnz;
      int bad = 0;
      CNA_TRY(launch_remap_indices(c, c->halo_recv_idx, nr, c->idx_t, &bad));
      if (bad) {
        dev_free(c, c->idx_t, sizeof(int32_t) * std::max<int64_t>(c->idx_t_n, 1));
        c->idx_t = nullptr;
        c->idx_t_n = 0;
        CNA_FAIL(CNA_EINVAL, "cna_set_halo: the graph block references rows that are neither local nor in the receive list");
      }
      c->t_compact = true;
      c->t_rows = c->n_local + nr;
      void_cells(c);
      if (c->sid) {                      // (a plan that arrives after cna_set_samples: size the buffers for the new row space)
        CNA_TRY(ensure_T(c, c->ld));
        CNA_TRY(ensure_sparse_state(c));
      }
    }
  }
  return 0;
}

// Between diffusion steps every rank needs the state rows of its cells' neighbours.  Default: ring
// all-gather of the row blocks (every rank ends up with everything).  With cna_set_halo: pack the
// rows other ranks asked for, one grouped send/recv per peer, scatter what arrives -- with a banded
// cell order that is a few per cent of the all-gather volume.
static int exchange_state(cna_ctx* c, double* T, hipStream_t st = nullptr) {
  if (c->halo_on) {
    const int ld = c->t_ld;
    CNA_TRY(dev_reserve(c, &c->halo_sbuf, &c->halo_sbuf_cap, 8 * std::max<int64_t>(c->halo_ns, 1) * ld));
    ProfScope ps(c, CNA_K_HALO_EXCHANGE, st);              // pack + send / receive + unpack, on the stream that carries them
    if (c->t_compact) {
      // the rows that arrive ARE the tail of the state, in the order of the receive list: no staging, no scatter
      CNA_TRY(launch_pack_rows(c, T, c->halo_send_idx, c->halo_ns, ld, (double*)c->halo_sbuf, st));
      if (c->halo_ns + c->halo_nr > 0)
        CNA_TRY(comm_halo_exchange(c, (const double*)c->halo_sbuf, T + c->n_local * (int64_t)ld, ld, st));
      return 0;
    }
    CNA_TRY(dev_reserve(c, &c->halo_rbuf, &c->halo_rbuf_cap, 8 * std::max<int64_t>(c->halo_nr, 1) * ld));
    CNA_TRY(launch_pack_rows(c, T + c->row0 * ld, c->halo_send_idx, c->halo_ns, ld, (double*)c->halo_sbuf, st));
    if (c->halo_ns + c->halo_nr > 0)
      CNA_TRY(comm_halo_exchange(c, (const double*)c->halo_sbuf, (double*)c->halo_rbuf, ld, st));
    CNA_TRY(launch_unpack_rows(c, (const double*)c->halo_rbuf, c->halo_recv_idx, c->halo_nr, ld, T, st));
    return 0;
  }
  if (c->nranks == 1) return 0;
  const size_t block = sizeof(double) * (size_t)c->rows_per_rank * c->t_ld;
  return comm_allgather_bytes(c, (char*)T + block * c->rank, T, block);
}

// y: the standardised phenotype the analysis will pass to cna_select_standardized[_fused] (n = number of samples);
// the next walk step that is the last of its walk then also leaves that call's results (see common.h: byp_*).
// y = NULL clears.  A hint, never a promise: a selection call that asks for anything else runs its own pass.
int cna_nam_select_hint(cna_ctx* c, const double* y, int n) {
  CHECK_CTX(c);
  c->byp_hint.clear();
  if (!y || n < 2 || n > 1024) return 0;
  if (!c->byp_buf) HIP_TRY(hipMalloc(&c->byp_buf, 16 + 8 * 1024));
  // Through pinned staging, queued on the MAIN stream behind the steps already there: asynchronous (this call does not wait
  // for them) and in stream order in front of the step that reads y.  (Round 5 copied from the caller's pageable array on
  // the copy stream and waited for it: ~15 us of the host in front of the walk's last launch.)  The staging is free again:
  // the previous analysis that used it has been collected.
  if (!c->h_hint) HIP_TRY(hipHostMalloc(&c->h_hint, 8 * 1024, hipHostMallocDefault));
  std::memcpy(c->h_hint, y, 8 * (size_t)n);
  HIP_TRY(hipMemcpyAsync((char*)c->byp_buf + 16, c->h_hint, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  c->byp_hint.assign(y, y + n);
  return 0;
}

// 1: the launch that follows is to produce the by-product (buffers sized, y and counters on the device); 0: no.  Never
// while a local-null pass is pending: the by-product rewrites X, which that pass's f64 rerun may still read (the step
// then writes the NAM, and the next selection makes the same X from it).
static int arm_select_byproduct(cna_ctx* c) {
  const char* sw = getenv("CNA_WALK_SELECT");              // A/B switch, read at every walk (tests flip it)
  const bool off = sw && atoi(sw) == 0;
  std::vector<double> y;
  y.swap(c->byp_hint);                                  // one-shot
  if (off || c->null.phase == NULL_PENDING || (int)y.size() != c->N || c->t_ld != c->ld || c->t_ld <= 64 || c->N < 2 || c->n_local < 1)
    return 0;
  const int64_t nx = c->n_local;
  const int Nx = c->N;
  if (x_begin(c, "cna_nam_step", nx, Nx, nullptr)) return 0;
  if (reserve_ncorrs(c, nx)) return 0;
  c->byp_with_q = Nx <= 256 && null_i8_enabled();
  if (c->byp_with_q && ensure_xq(c, (Nx + 31) / 32)) return 0;
  if (!c->byp_buf) return 0;
  c->byp_y.swap(y);
  if (hipMemsetAsync(c->byp_buf, 0, 16, c->stream) != hipSuccess) return 0;
  return 1;
}

static int64_t lcm64(int64_t a, int64_t b) {
  int64_t x = a, y = b;
  while (y) { const int64_t t = x % y; x = y; y = t; }
  return a / x * b;
}
// The last step of a walk that leaves the selection by-product, in K row ranges with the Gram kernel of every range
// behind it on gram_stream.  1: queued that way (c->gram_pre set), 0: not eligible (the caller launches the step as
// one kernel), < 0 never; errors are returned as positive codes through *rc.
static int ranged_last_step(cna_ctx* c, bool first, bool want_kurt, bool may_stop, int* rc) {
  *rc = 0;
  const int K = gram_overlap_ranges();
  if (K < 2 || c->nx != c->n_local || c->Nx < 2 || c->Nx > 1024) return 0;
  if (ensure_gram_stream(c) != 1) return 0;
  const int64_t turn = nam_step_turn_rows(c, c->n_local);
  if (turn <= 0) return 0;
  if ((*rc = gram_pre_settle(c)) != 0) return 1;
  int64_t unit_g = 0;
  if ((*rc = gram_pre_begin(c, &unit_g)) != 0) return 1;
  const int64_t unit = lcm64(turn, unit_g);
  const int64_t nunits = c->n_local / unit;
  if (nunits < 2 * K || nam_step_turn_rows(c, unit) != turn) return 0;
  void* g = c->gram_buf;
  if ((*rc = dev_reserve(c, &g, &c->gram_cap, (int64_t)sizeof(double) * c->Nx * c->Nx)) != 0) return 1;
  c->gram_buf = (double*)g;
  hipStream_t W = c->stream;
  // an error from here on: close the profiling span that was opened and wait for what already sits on the Gram stream
  // (nobody would otherwise: gram_pre_pending stays false, and the next writer of X or of the partial tiles must not
  // find those kernels still reading them)
  bool span_open = false;
  int kid_of_span = CNA_K_NAM_STEP;
  auto fail = [&]() { if (span_open) prof_end(c, kid_of_span, c->stream); (void)hipStreamSynchronize(c->gram_stream); return 1; };
#define RL_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cna_set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); *rc = (int)e_; return fail(); } } while (0)
  const bool sparse_step = c->sp_cnt && c->steps_done == 1;
  const int kid = sparse_step ? CNA_K_NAM_STEP_SPARSE : CNA_K_NAM_STEP;
  kid_of_span = kid;
  if (c->prof) { prof_begin(c, kid, W); span_open = true; }   // one span over all ranges: the step as the other launches report it
  int64_t b0 = 0;
  for (int r = 0; r < K; ++r) {
    const int64_t b1 = r + 1 == K ? c->n_local : (nunits * (r + 1) / K) * unit;
    if ((*rc = launch_nam_step(c, first, want_kurt, false, may_stop, false, nullptr, 0, b0, b1 - b0, W, false)) != 0) break;
    if (r + 1 == K && span_open) { prof_end(c, kid, W); span_open = false; }
    RL_TRY(hipEventRecord(c->range_done, W));
    RL_TRY(hipStreamWaitEvent(c->gram_stream, c->range_done, 0));
    if ((*rc = gram_pre_range(c, b0, b1, c->gram_stream)) != 0) break;
    b0 = b1;
  }
  if (*rc) return fail();
  if ((*rc = gram_pre_finish(c, c->gram_buf, c->gram_stream)) != 0) return fail();
  RL_TRY(hipEventRecord(c->gram_pre_done, c->gram_stream));
#undef RL_TRY
  c->gram_pre = true;
  c->gram_pre_pending = true;
  return 1;
}

int cna_nam_step(cna_ctx* c, int want_kurt, int may_continue, int may_stop) {
  CHECK_CTX(c);
  if (!c->sid || !c->have_colsum) CNA_FAIL(CNA_ESTATE, "cna_nam_step needs cna_colsums and cna_set_samples");
  if (c->t_ld != c->ld) CNA_FAIL(CNA_ESTATE, "state buffers hold a dense diffusion; call cna_set_samples again");
  const bool first = c->steps_done == 0;
  if (!first && !c->t_valid) CNA_FAIL(CNA_ESTATE, "previous step did not keep its state (may_continue=0)");
  void_x_nam_link(c);
  const bool arm = !first && !may_continue && may_stop && !c->auto_stop && arm_select_byproduct(c) == 1;
  // ... and then the NAM itself is not written: the analysis reads X, and whoever does ask for the NAM (res.nam, a later
  // call with other covariates) gets it from a second run of this step (need_nam), whose input state stays where it is
  const bool skip_nam = arm;
  c->byp_arm = arm;
  c->byp_skip_nam = skip_nam;
  // A step whose state other ranks need (halo exchange): the rows they asked for first, their exchange on its own
  // stream while the rest of the block is walked; the next step waits for both.  (The buffers are sized before anything
  // is queued: a reallocation would wait for the device.)
  const char* ov = getenv("CNA_HALO_OVERLAP");
  // (RCCL: only with a communicator of the halo stream's own, cna_comm_init; the shared-memory test backend stages
  // through the host and has no such constraint)
  const bool overlap_ok = c->halo_on && c->halo_stream && !(ov && atoi(ov) == 0) && (c->shm || c->comm_halo);
  // (NOT a function of this rank's own row counts: a rank nobody asks for rows, or one without interior rows, takes the
  // same path with an empty launch -- which communicator carries the exchange must be the same decision on every rank)
  const bool overlap = may_continue && overlap_ok;
  // Round 5: the main stream no longer waits for an exchange where it is queued (halo_wait_pending) but where its rows
  // are first needed.  A step that reads a state walks the rows WITHOUT a foreign neighbour first -- under the exchange that
  // brings the foreign rows -- then waits, then walks the rest; its own exchange starts when both are done and is in turn
  // hidden under the next step's safe rows (the last step included: row list and selection by-product combine).  The
  // first step reads no state: the rows other ranks asked for first, their exchange beside the interior.
  const bool two_lists = overlap_ok && c->halo_nsafe > 0 && c->halo_nneed > 0;
  auto walk_safe_then_rest = [&](bool wt) -> int {
    c->halo_safe_launch = true;
    int rc2 = launch_nam_step(c, first, want_kurt != 0, wt, may_stop != 0, false, c->halo_rows_safe, c->halo_nsafe);
    c->halo_safe_launch = false;
    if (rc2 == 0) rc2 = launch_nam_step(c, first, want_kurt != 0, wt, may_stop != 0, false, c->halo_rows_need, c->halo_nneed);
    return rc2;
  };
  if (overlap) {
    c->byp_arm = false;
    c->byp_skip_nam = false;
    const int ld = c->t_ld;
    double* Tn = c->T[c->t_cur ^ 1];
    CNA_TRY(dev_reserve(c, &c->halo_sbuf, &c->halo_sbuf_cap, 8 * std::max<int64_t>(c->halo_ns, 1) * ld));
    if (!c->t_compact) CNA_TRY(dev_reserve(c, &c->halo_rbuf, &c->halo_rbuf_cap, 8 * std::max<int64_t>(c->halo_nr, 1) * ld));
    if (first || !two_lists) {
      CNA_TRY(launch_nam_step(c, first, want_kurt != 0, true, may_stop != 0, false, c->halo_rows_b, c->halo_nb));
      HIP_TRY(hipEventRecord(c->halo_e1, c->stream));
      // (the interior rows: nobody else reads their state after the FIRST step -- this rank's second step takes its local
      // neighbours from their pairs -- so their dense rows, 8N bytes each, are not written: only rows that overflow the pairs)
      c->sp_dense_interior_off = first;
      const int rc_int = launch_nam_step(c, first, want_kurt != 0, true, may_stop != 0, false, c->halo_rows_i, c->halo_ni);
      c->sp_dense_interior_off = false;
      CNA_TRY(rc_int);
    } else {
      CNA_TRY(walk_safe_then_rest(true));
      HIP_TRY(hipEventRecord(c->halo_e1, c->stream));
    }
    HIP_TRY(hipStreamWaitEvent(c->halo_stream, c->halo_e1, 0));
    CNA_TRY(exchange_state(c, Tn, c->halo_stream));
    HIP_TRY(hipEventRecord(c->halo_e2, c->halo_stream));
    c->halo_wait_pending = true;                 // (halo_settle: before the first launch that reads those rows, before any collective)
    c->t_cur ^= 1;
    c->lazy_steps_before = c->steps_done;
  } else {
    int rc_step = 0;
    if (!first && !may_continue && c->halo_wait_pending && two_lists && !c->auto_stop && gram_overlap_ranges() < 2) {
      rc_step = walk_safe_then_rest(false);     // the walk's last step: safe rows under the last exchange, then the rest
    } else if (!(arm && ranged_last_step(c, first, want_kurt != 0, may_stop != 0, &rc_step) == 1)) {
      rc_step = launch_nam_step(c, first, want_kurt != 0, may_continue != 0, may_stop != 0, false);
    }
    c->byp_arm = false;
    c->byp_skip_nam = false;
    CNA_TRY(rc_step);
    c->byp_valid = arm;
    c->lazy_steps_before = c->steps_done;
    if (may_continue) {
      CNA_TRY(exchange_state(c, c->T[c->t_cur ^ 1]));
      c->t_cur ^= 1;
    }
  }
  c->t_valid = may_continue != 0;
  c->nam_valid = may_stop != 0 && !skip_nam;
  c->nam_lazy = skip_nam;
  c->steps_done += 1;
  if (want_kurt) {
    c->stat_space = CNA_MAT_NAM;
    CNA_TRY(exchange_stat(c));
  }
  return 0;
}

int cna_nam_steps(cna_ctx* c, int nsteps) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  if (nsteps < 1) CNA_FAIL(CNA_EINVAL, "nsteps < 1");
  for (int i = 0; i < nsteps; ++i) CNA_TRY(cna_nam_step(c, 0, i + 1 < nsteps, i + 1 == nsteps));
  return 0;
}

// Exact median of the per-cell statistic (np.median semantics: NaN if any entry is NaN, mean of the
// two middle values for an even count) by radix select on the device: 8 passes of an 8-bit digit
// histogram per order statistic, a 2 KB read-back each -- ~0.3 ms instead of the 1-6 ms numpy's
// partition takes on 200k-1M values, and no cells-sized transfer.  NAM-space statistics are
// replicated on every rank (all n_global values); X-space ones are the local rows, so the
// histograms are summed over ranks.
static int stat_select(cna_ctx* c, const double* v, int64_t n_loc, bool sharded, int64_t k, unsigned long long* hist_dev,
                       double* value, int64_t* n_nan, int64_t* n_total) {
  unsigned long long prefix = 0;
  std::vector<unsigned long long> h(257);
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    CNA_TRY(launch_digit_hist(c, v, n_loc, prefix, shift, hist_dev));
    if (sharded) CNA_TRY(comm_allreduce_i64_sum(c, (int64_t*)hist_dev, 257));
    HIP_TRY(hipMemcpyAsync(h.data(), hist_dev, 8 * 257, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (pass == 0) {
      int64_t tot = 0;
      for (int d = 0; d < 256; ++d) tot += (int64_t)h[d];
      *n_nan = (int64_t)h[256];
      *n_total = tot + *n_nan;
      if (*n_nan > 0 || tot == 0) return 0;
      if (k < 0) k = (tot - 1) / 2;                        // caller asked for the lower middle
      if (k >= tot) k = tot - 1;
    }
    int d = 0;
    int64_t before = 0;
    while (d < 255 && before + (int64_t)h[d] <= k) before += (int64_t)h[d++];
    k -= before;
    prefix = (prefix << 8) | (unsigned long long)d;
  }
  const unsigned long long bits = (prefix >> 63) ? (prefix & 0x7fffffffffffffffull) : ~prefix;
  std::memcpy(value, &bits, 8);
  return 0;
}

// median (and, with qc, threshold and count of _qc_nam) of the current per-cell statistic; everything is queued, the
// host waits once.  out3 = {median, threshold, count}
static int stat_median_device(cna_ctx* c, bool qc, double* out3) {
  const double* v = c->stat;
  int64_t n_loc;
  bool sharded;
  if (c->stat_space == CNA_MAT_NAM) { n_loc = c->n_global; sharded = false; }
  else if (c->stat_space == CNA_MAT_X) { n_loc = c->nx; sharded = c->nranks > 1 || comm_active(c); }
  else CNA_FAIL(CNA_ESTATE, "no per-cell statistic available");
  unsigned long long* hist = nullptr;
  CNA_TRY(ensure_auto_state(c, &hist));
  const size_t sb = (auto_state_bytes() + 255) & ~(size_t)255;
  HIP_TRY(hipMemsetAsync(c->auto_state, 0, sb, c->stream));
  CNA_TRY(launch_auto_median(c, v, n_loc, c->auto_state, hist, -1, 0, sharded));
  if (qc) {
    CNA_TRY(launch_qc_count(c, v, n_loc, c->auto_state));
    if (sharded) CNA_FAIL(CNA_ESTATE, "cna_stat_qc is for the NAM-space statistic");
  }
  struct { double median, threshold; unsigned long long count; } res;
  HIP_TRY(hipMemcpyAsync(&res, (const char*)c->auto_state + auto_state_result_offset(), sizeof(res), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  out3[0] = res.median;
  out3[1] = res.threshold;
  out3[2] = (double)res.count;
  return 0;
}

int cna_stat_median(cna_ctx* c, double* median_out) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_stat_median");
  AUTO_FINISH(c);
  if (!median_out) CNA_FAIL(CNA_EINVAL, "cna_stat_median: null output");
  if (getenv("CNA_MEDIAN_HOST")) {            // the first implementation: digit choice on the host, 16 round trips
    const double* v = c->stat;
    int64_t n_loc;
    bool sharded;
    if (c->stat_space == CNA_MAT_NAM) { n_loc = c->n_global; sharded = false; }
    else if (c->stat_space == CNA_MAT_X) { n_loc = c->nx; sharded = c->nranks > 1 || comm_active(c); }
    else CNA_FAIL(CNA_ESTATE, "no per-cell statistic available");
    CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, 8 * 257 + 64));   // main-stream scratch (not c->gt:
    unsigned long long* hist = (unsigned long long*)c->scratch;            // the helper thread may be conditioning)
    double lo = 0.0, hi = 0.0;
    int64_t n_nan = 0, n_tot = 0;
    CNA_TRY(stat_select(c, v, n_loc, sharded, -1, hist, &lo, &n_nan, &n_tot));
    if (n_tot == 0 || n_nan > 0) { *median_out = __builtin_nan(""); return 0; }
    if (n_tot & 1) { *median_out = lo; return 0; }
    CNA_TRY(stat_select(c, v, n_loc, sharded, n_tot / 2, hist, &hi, &n_nan, &n_tot));
    *median_out = (lo + hi) / 2.0;
    return 0;
  }
  double out3[3];
  CNA_TRY(stat_median_device(c, false, out3));
  *median_out = out3[0];
  return 0;
}

// _qc_nam's decision (_nam.py:94-96) on the batch kurtosis left by cna_batch_kurtosis(CNA_MAT_NAM, ..): the median,
// threshold = max(6, 2 median) and the number of cells that fail `kurtosis < threshold` -- zero means "every cell
// stays", and then nothing cells-sized has to travel to the host (cna_fetch_cell_stat otherwise).  One wait.
int cna_stat_qc(cna_ctx* c, double* median_out, double* threshold_out, int64_t* n_dropped_out) {
  CHECK_CTX(c);
  AUTO_FINISH(c);
  if (c->stat_space != CNA_MAT_NAM) CNA_FAIL(CNA_ESTATE, "cna_stat_qc needs the NAM-space statistic of cna_batch_kurtosis");
  double out3[3];
  CNA_TRY(stat_median_device(c, true, out3));
  if (median_out) *median_out = out3[0];
  if (threshold_out) *threshold_out = out3[1];
  if (n_dropped_out) *n_dropped_out = (int64_t)out3[2];
  return 0;
}

// The walk of _nam.py:57-70 with nsteps=None: steps until the median kurtosis stops falling by 3 or more (checked from
// the third step on, at most maxnsteps).  Steps, medians and the rule are queued without waiting for a verdict --
// four steps by cna_nam_auto_launch, which returns at once, then two at a time by cna_nam_auto_finish, which reads
// one word per batch; the steps queued behind the one that met the rule return at once (StepArgs::stop).  The first
// step's kurtosis is never looked at by the rule (_nam.py:65: i + 1 >= 3 compares steps 2 and 3) and is not
// computed.  Same steps, same NAM as cna_nam_step + cna_stat_median in a host loop.
static int auto_queue(cna_ctx* c, int upto) {
  const size_t sb = (auto_state_bytes() + 255) & ~(size_t)255;
  unsigned long long* hist = (unsigned long long*)((char*)c->auto_state + sb);
  struct Guard { cna_ctx* c; ~Guard() { c->auto_stop = nullptr; } } guard{c};
  c->auto_stop = (const int*)((const char*)c->auto_state + auto_state_stopped_offset());
  for (int i = c->auto_queued; i < upto; ++i) {
    const bool last = i + 1 == c->auto_max;
    CNA_TRY(cna_nam_step(c, i >= 1, !last, last || i + 1 >= 3));
    if (i >= 1) CNA_TRY(launch_auto_median(c, c->stat, c->n_global, c->auto_state, hist, i, 3));
    c->auto_queued = i + 1;
  }
  return 0;
}

int cna_nam_auto_launch(cna_ctx* c, int maxnsteps) {
  CHECK_CTX(c);
  if (maxnsteps < 1 || maxnsteps > 16) CNA_FAIL(CNA_EINVAL, "cna_nam_auto: 1 <= maxnsteps <= 16");
  if (c->steps_done != 0) CNA_FAIL(CNA_ESTATE, "cna_nam_auto starts a walk: call cna_set_samples / cna_restart_nam first");
  const size_t sb = (auto_state_bytes() + 255) & ~(size_t)255;
  CNA_TRY(ensure_auto_state(c, nullptr));
  HIP_TRY(hipMemsetAsync(c->auto_state, 0, sb, c->stream));
  c->auto_max = maxnsteps;
  c->auto_queued = 0;
  c->auto_pending = true;
  const int rc = auto_queue(c, std::min(4, maxnsteps));
  if (rc) c->auto_pending = false;
  return rc;
}

int cna_nam_auto_finish(cna_ctx* c, int* steps_out, double* medkurt_out) {
  CHECK_CTX(c);
  if (!c->auto_pending) CNA_FAIL(CNA_ESTATE, "cna_nam_auto_finish without cna_nam_auto_launch");
  c->auto_pending = false;
  const size_t sb = (auto_state_bytes() + 255) & ~(size_t)255;
  std::vector<char> host(sb);
  int taken = 0;
  for (;;) {
    HIP_TRY(hipMemcpyAsync(host.data(), c->auto_state, sb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int stopped;
    std::memcpy(&stopped, host.data() + auto_state_stopped_offset(), 4);
    taken = stopped ? stopped : c->auto_queued;
    if (stopped || c->auto_queued >= c->auto_max) break;
    CNA_TRY(auto_queue(c, std::min(c->auto_queued + 2, c->auto_max)));
  }
  // the steps queued behind the last one taken did nothing: the NAM on the device is that of step `taken`
  c->steps_done = taken;
  c->nam_valid = true;
  c->t_valid = false;
  c->stat_space = CNA_MAT_NAM;
  if (steps_out) *steps_out = taken;
  if (medkurt_out) {
    const size_t off = 2 * 8 + 2 * 8 + 2 * 8;             // AutoState: prefix[2], k[2], n_tot, n_nan, then med[16]
    std::memcpy(medkurt_out, host.data() + off, 8 * (size_t)taken);
    medkurt_out[0] = __builtin_nan("");                    // (not computed: the rule never reads it)
  }
  return 0;
}

int cna_nam_auto(cna_ctx* c, int maxnsteps, int* steps_out, double* medkurt_out) {
  CNA_TRY(cna_nam_auto_launch(c, maxnsteps));
  return cna_nam_auto_finish(c, steps_out, medkurt_out);
}

// --------------------------------------------------------------------- dense diffusion
int cna_dense_load(cna_ctx* c, const double* s_local, int m) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_dense_load");
  AUTO_FINISH(c);
  if (!c->have_colsum) CNA_FAIL(CNA_ESTATE, "cna_dense_load needs cna_colsums");
  if (m < 1 || m > 1024) CNA_FAIL(CNA_EINVAL, "dense state must have 1..1024 columns");
  const int ld = round_up(m, 4);
  CNA_TRY(ensure_T(c, ld));
  void* ds = c->dense_s;
  CNA_TRY(dev_reserve(c, &ds, &c->dense_cap, (int64_t)sizeof(double) * std::max<int64_t>(c->n_local, 1) * ld));
  c->dense_s = (double*)ds;
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, (int64_t)sizeof(double) * std::max<int64_t>(c->n_local, 1) * m));
  HIP_TRY(hipMemcpyAsync(c->scratch, s_local, sizeof(double) * c->n_local * m, hipMemcpyHostToDevice, c->stream));
  c->t_width = m;
  c->t_ld = ld;
  c->t_cur = 0;
  c->t_f32[0] = c->t_f32[1] = false;
  CNA_TRY(launch_scale_rows(c, (const double*)c->scratch, c->T[0], m, ld));
  CNA_TRY(exchange_state(c, c->T[0]));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->t_valid = true;
  c->nam_valid = false; c->nam_lazy = false;
  c->steps_done = 1;  // never take the one-hot path
  return 0;
}

int cna_dense_step(cna_ctx* c) {
  CHECK_CTX(c);
  if (!c->t_valid || !c->dense_s) CNA_FAIL(CNA_ESTATE, "cna_dense_step before cna_dense_load");
  CNA_TRY(launch_nam_step(c, false, false, true, false, true));
  CNA_TRY(exchange_state(c, c->T[c->t_cur ^ 1]));
  c->t_cur ^= 1;
  return 0;
}

int cna_dense_fetch(cna_ctx* c, double* out) {
  CHECK_CTX(c);
  if (!c->dense_s) CNA_FAIL(CNA_ESTATE, "no dense state");
  if (c->n_local > 0)
    HIP_TRY(hipMemcpy2DAsync(out, sizeof(double) * c->t_width, c->dense_s, sizeof(double) * c->t_ld,
                             sizeof(double) * c->t_width, c->n_local, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
