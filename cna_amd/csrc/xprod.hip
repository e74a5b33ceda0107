// The producers of the working matrix X on the host (extern "C" entry points of libcna_hip.so, see include/cna_hip.h): QC,
// selection from the NAM, upload, residualisation and standardisation -- each bracketed by x_begin / x_commit -- and what
// reads X row by row: projection and the coefficients.  The kernels are in rows.hip, rows16.hip and mfma.hip.
#include "common.h"
#include <cstring>

// the coefficient buffer c->ncorrs, one double for each of `rows` rows of X
int reserve_ncorrs(cna_ctx* c, int64_t rows) {
  void* np = c->ncorrs;
  CNA_TRY(dev_reserve(c, &np, &c->ncorrs_cap, 8 * std::max<int64_t>(rows, 1)));
  c->ncorrs = (double*)np;
  return 0;
}

extern "C" {

// ------------------------------------------------------------------------ QC / select
// The samples batch by batch: order[boff[b] .. boff[b + 1]) are those of batch b (a code outside [0, n_batches): none)
static void batch_order(const int32_t* codes, int ncols, int n_batches, std::vector<int32_t>& order, std::vector<int32_t>& boff) {
  boff.assign(n_batches + 1, 0);
  for (int s = 0; s < ncols; ++s)
    if (codes[s] >= 0 && codes[s] < n_batches) boff[codes[s] + 1]++;
  for (int b = 0; b < n_batches; ++b) boff[b + 1] += boff[b];
  order.assign(std::max(boff[n_batches], 1), 0);
  std::vector<int32_t> cur(boff.begin(), boff.end() - 1);
  for (int s = 0; s < ncols; ++s)
    if (codes[s] >= 0 && codes[s] < n_batches) order[cur[codes[s]]++] = s;
}

// W (r x Nx) and C^T (C: Nx x r, row-major) of the projector M = I - C.W to the device, into Wd / Ctd; Ct is the host
// copy of C^T, kept by the caller until its next wait.  r = 0: nothing is sent.
static int upload_factors(cna_ctx* c, const double* C, const double* W, int r, int Nx, double* Wd, double* Ctd,
                          std::vector<double>& Ct) {
  Ct.assign((size_t)std::max(r, 1) * Nx, 0.0);
  for (int i = 0; i < Nx; ++i)
    for (int k = 0; k < r; ++k) Ct[(size_t)k * Nx + i] = C[(size_t)i * r + k];
  if (r > 0) {
    HIP_TRY(hipMemcpyAsync(Wd, W, 8 * (size_t)r * Nx, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(Ctd, Ct.data(), 8 * (size_t)r * Nx, hipMemcpyHostToDevice, c->stream));
  }
  return 0;
}

// What a pass over the rows reads besides the rows, carved out of c->scratch and sent on the main stream: the factors W and
// C^T of the projector (upload_factors), the phenotype y (null: none is sent and `y` stays null), the samples batch by batch
// (batch_order; codes null: none), 2 049 words for max |coefficient| and its per-workgroup maxima, and `counters` words of
// the caller's behind them, zeroed.  The host copies of what was sent live here: keep the struct until the next wait.
struct RowOperands {
  double *W = nullptr, *Ct = nullptr, *y = nullptr;
  int32_t *order = nullptr, *boff = nullptr;
  unsigned long long *maxw = nullptr, *counters = nullptr;
  std::vector<double> Ct_host;
  std::vector<int32_t> order_host, boff_host;
};
static int stage_row_operands(cna_ctx* c, RowOperands& op, const double* C, const double* W, int r, int Nx, const double* y,
                              const int32_t* codes = nullptr, int n_batches = 0, int counters = 0) {
  if (codes) batch_order(codes, Nx, n_batches, op.order_host, op.boff_host);
  const int64_t rn = (int64_t)std::max(r, 1) * Nx, no = (int64_t)op.order_host.size(), nb = (int64_t)op.boff_host.size();
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, carve_bytes({8 * rn, 8 * rn, 8 * (int64_t)Nx, 8 * 2049, 4 * no, 4 * nb, 8 * (int64_t)counters})));
  Carver cv(c->scratch);
  op.W = cv.take<double>(rn);
  op.Ct = cv.take<double>(rn);
  double* yd = cv.take<double>(Nx);
  op.maxw = cv.take<unsigned long long>(2049);
  op.order = cv.take<int32_t>(no);
  op.boff = cv.take<int32_t>(nb);
  op.counters = cv.take<unsigned long long>(counters);
  CNA_TRY(upload_factors(c, C, W, r, Nx, op.W, op.Ct, op.Ct_host));
  if (y) {
    HIP_TRY(hipMemcpyAsync(yd, y, 8 * Nx, hipMemcpyHostToDevice, c->stream));
    op.y = yd;
  }
  if (codes) {
    HIP_TRY(hipMemcpyAsync(op.order, op.order_host.data(), 4 * no, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(op.boff, op.boff_host.data(), 4 * nb, hipMemcpyHostToDevice, c->stream));
  }
  if (counters) HIP_TRY(hipMemsetAsync(op.counters, 0, 8 * counters, c->stream));
  return 0;
}

// Behind a pass that left the batch kurtosis of X's rows in c->stat: its median formed on the device, then max
// |coefficient| (*mb) and that median queued for the host -- in *m and *med after the caller's next wait
static int queue_bk_results(cna_ctx* c, const unsigned long long* mb, double* m, double* med) {
  const bool sharded = c->nranks > 1 || comm_active(c);
  unsigned long long* hist = nullptr;
  CNA_TRY(ensure_auto_state(c, &hist));
  const size_t sb = (auto_state_bytes() + 255) & ~(size_t)255;
  HIP_TRY(hipMemsetAsync(c->auto_state, 0, sb, c->stream));
  CNA_TRY(launch_auto_median(c, c->stat, c->nx, c->auto_state, hist, -1, 0, sharded));
  HIP_TRY(hipMemcpyAsync(m, mb, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(med, (const char*)c->auto_state + auto_state_result_offset(), 8, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

// The operand of launch_xb in c->scratch: ldx x ldb (ldb = ncols rounded up to 16), zero beyond Nx x ncols, where row k
// holds row k of A (Nx x ncols, row-major), column k of A when `transposed` (A: ncols x Nx), or (A null) of the identity.
// B is the host copy, kept by the caller until its next wait.
static int xb_operand(cna_ctx* c, const double* A, int ncols, bool transposed, std::vector<double>& B, int* ldb_out) {
  const int Nx = c->Nx, ldx = c->ldx;
  const int ldb = round_up(ncols, 16);
  B.assign((size_t)ldx * ldb, 0.0);
  for (int k = 0; k < Nx; ++k)
    for (int j = 0; j < ncols; ++j)
      B[(size_t)k * ldb + j] = !A ? (j == k ? 1.0 : 0.0) : transposed ? A[(size_t)j * Nx + k] : A[(size_t)k * ncols + j];
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, (int64_t)sizeof(double) * ldx * ldb));
  HIP_TRY(hipMemcpyAsync(c->scratch, B.data(), sizeof(double) * ldx * ldb, hipMemcpyHostToDevice, c->stream));
  *ldb_out = ldb;
  return 0;
}

int cna_batch_kurtosis(cna_ctx* c, int which, const int32_t* batch_codes, int n_batches) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_batch_kurtosis");
  AUTO_FINISH(c);
  const double* mat;
  int64_t rows;
  int ncols, ld;
  double* out;
  if (which == CNA_MAT_NAM) {
    CNA_TRY(need_nam(c));
    mat = c->nam; rows = c->n_local; ncols = c->N; ld = c->ld; out = c->stat + c->row0;
  } else if (which == CNA_MAT_X) {
    if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
    mat = c->X; rows = c->nx; ncols = c->Nx; ld = c->ldx; out = c->stat;
    if (c->nx > c->n_pad) CNA_FAIL(CNA_EINVAL, "X larger than the stat buffer");
  } else {
    CNA_FAIL(CNA_EINVAL, "bad matrix selector");
  }
  if (n_batches < 1) CNA_FAIL(CNA_EINVAL, "n_batches < 1");
  RowOperands op;                            // (the batches alone: no factors, no phenotype)
  CNA_TRY(stage_row_operands(c, op, nullptr, nullptr, 0, ncols, nullptr, batch_codes, n_batches));
  CNA_TRY(launch_batch_kurtosis(c, mat, rows, ncols, ld, op.order, op.boff, n_batches, out));
  c->stat_space = which;
  if (which == CNA_MAT_NAM) CNA_TRY(exchange_stat(c));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (op holds what the uploads read)
  return 0;
}

int cna_zero_variance(cna_ctx* c, const int32_t* colmap, int n_sel, uint8_t* flags_out, int64_t* n_zero_out) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_zero_variance");
  AUTO_FINISH(c);
  CNA_TRY(need_nam(c));
  if (!colmap) n_sel = c->N;
  if (n_sel < 1) CNA_FAIL(CNA_EINVAL, "no samples selected");
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, carve_bytes({4 * (int64_t)n_sel, c->n_pad, 8})));
  Carver cv(c->scratch);
  int32_t* cm = cv.take<int32_t>(n_sel);
  uint8_t* flags = cv.take<uint8_t>(c->n_pad);        // all cells; this rank fills [row0, row0+n_local)
  unsigned long long* cnt = cv.take<unsigned long long>(1);
  if (colmap) HIP_TRY(hipMemcpyAsync(cm, colmap, 4 * n_sel, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(cnt, 0, 8, c->stream));
  HIP_TRY(hipMemsetAsync(flags, 0, c->n_pad, c->stream));
  CNA_TRY(launch_zero_variance(c, colmap ? cm : nullptr, n_sel, flags + c->row0, cnt));
  CNA_TRY(comm_allreduce_i64_sum(c, (int64_t*)cnt, 1));
  unsigned long long h = 0;
  HIP_TRY(hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_zero_out) *n_zero_out = (int64_t)h;
  if (flags_out) {
    if (c->local_view) {
      HIP_TRY(hipMemcpyAsync(flags_out, flags + c->row0, c->n_local, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    } else if (h == 0) {
      std::memset(flags_out, 0, c->n_global);
    } else {
      if (c->nranks > 1)
        CNA_TRY(comm_allgather_bytes(c, flags + c->rows_per_rank * c->rank, flags, (size_t)c->rows_per_rank));
      HIP_TRY(hipMemcpyAsync(flags_out, flags, c->n_global, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
  }
  return 0;
}

int cna_select(cna_ctx* c, const int64_t* keep_idx, int64_t n_keep, const int32_t* colmap, int n_sel) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_select");
  AUTO_FINISH(c);
  CNA_TRY(need_nam(c));
  const int64_t nx = keep_idx ? n_keep : c->n_local;
  const int Nx = colmap ? n_sel : c->N;
  if (nx < 0 || nx > c->n_local || Nx < 1) CNA_FAIL(CNA_EINVAL, "cna_select: bad sizes");
  CNA_TRY(x_begin(c, "cna_select", nx, Nx, keep_idx));
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, 4 * (int64_t)Nx + 256));
  int32_t* cm = (int32_t*)c->scratch;
  if (colmap) HIP_TRY(hipMemcpyAsync(cm, colmap, 4 * Nx, hipMemcpyHostToDevice, c->stream));
  CNA_TRY(launch_select(c, colmap ? cm : nullptr));
  HIP_TRY(hipStreamSynchronize(c->stream));
  x_commit(c, true, false, false, false);
  return 0;
}

// Factors of a projector M = I - C.W (C: N x r, W: r x N, row-major; see cna_resid_lowrank) for the NEXT
// cna_select_standardized[_fused] call over N selected samples: that pass then leaves X residualised as well
// (select + zero-variance count + centre + M + /std [+ coefficients] in one read of the NAM).  r = 0 clears.
int cna_set_resid_factors(cna_ctx* c, const double* C, const double* W, int r, int N) {
  CHECK_CTX(c);
  if (r < 0 || N < 1 || (r > 0 && (!C || !W))) CNA_FAIL(CNA_EINVAL, "cna_set_resid_factors: bad arguments");
  c->resid_rk = 0;
  if (r == 0) return 0;
  if ((int64_t)2 * r * N * 8 > 128 * 1024) CNA_FAIL(CNA_EINVAL, "cna_set_resid_factors: factors exceed 128 KB");
  void* p = c->resid_f;
  CNA_TRY(dev_reserve(c, &p, &c->resid_f_cap, 16 * (int64_t)r * N));
  c->resid_f = (double*)p;
  std::vector<double> buf((size_t)2 * r * N);
  std::memcpy(buf.data(), W, 8 * (size_t)r * N);
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < r; ++k) buf[(size_t)r * N + (size_t)k * N + i] = C[(size_t)i * r + k];
  // on the copy stream: the main stream is busy with the walk kernels and this call must not wait for them
  HIP_TRY(hipMemcpyAsync(c->resid_f, buf.data(), 16 * (size_t)r * N, hipMemcpyHostToDevice, c->copy_stream));
  HIP_TRY(hipStreamSynchronize(c->copy_stream));                 // buf is a local; the kernels that read resid_f are issued later
  c->resid_rk = r;
  c->resid_n = N;
  return 0;
}

// cna_select that also counts the selected cells with zero variance over the selected samples
// (_association.py:182) in the same pass; *n_zero_out > 0: redo with cna_zero_variance + cna_select
int cna_select_checked(cna_ctx* c, const int64_t* keep_idx, int64_t n_keep, const int32_t* colmap, int n_sel,
                       int64_t* n_zero_out) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_select_checked");
  AUTO_FINISH(c);
  CNA_TRY(need_nam(c));
  const int64_t nx = keep_idx ? n_keep : c->n_local;
  const int Nx = colmap ? n_sel : c->N;
  if (nx < 0 || nx > c->n_local || Nx < 1) CNA_FAIL(CNA_EINVAL, "cna_select_checked: bad sizes");
  CNA_TRY(x_begin(c, "cna_select_checked", nx, Nx, keep_idx));
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, carve_bytes({4 * (int64_t)Nx, 8})));
  Carver cv(c->scratch);
  int32_t* cm = cv.take<int32_t>(Nx);
  unsigned long long* cnt = cv.take<unsigned long long>(1);
  if (colmap) HIP_TRY(hipMemcpyAsync(cm, colmap, 4 * Nx, hipMemcpyHostToDevice, c->stream));
  CNA_TRY(launch_select_zv(c, colmap ? cm : nullptr, cnt));
  CNA_TRY(comm_allreduce_i64_sum(c, (int64_t*)cnt, 1));
  unsigned long long h = 0;
  HIP_TRY(hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_zero_out) *n_zero_out = (int64_t)h;
  x_commit(c, true, false, false, false);
  return 0;
}

// gram_too != nullptr: the caller will want the Gram matrix of the result next.  When the selection is "all cells,
// samples in place, no projector" and the shape suits it, selection and Gram kernels are ONE launch
// (mfma.hip:k_selgram_blk) and *gram_too comes back true: the matrix is in c->gram_buf, summed over the ranks, as
// after cna_gram_launch (meaningless, like X, when *n_zero_out != 0).
static int select_standardized_impl(cna_ctx* c, const int64_t* keep_idx, int64_t n_keep, const int32_t* colmap, int n_sel,
                                    int64_t* n_zero_out, const double* y, double* max_abs_out, bool* gram_too) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_select_standardized");
  AUTO_FINISH(c);
  if (gram_too) *gram_too = false;
  if (!c->nam_valid && !c->nam_lazy) CNA_FAIL(CNA_ESTATE, "NAM not available");
  const int64_t nx = keep_idx ? n_keep : c->n_local;
  const int Nx = colmap ? n_sel : c->N;
  if (nx < 0 || nx > c->n_local || Nx < 2) CNA_FAIL(CNA_EINVAL, "cna_select_standardized: bad sizes");
  const bool byp_was = c->byp_valid;      // (the walk's by-product and the Gram matrix taken under it: x_begin voids both)
  const bool gram_pre_was = c->gram_pre;
  CNA_TRY(x_begin(c, "cna_select_standardized", nx, Nx, keep_idx));
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, carve_bytes({4 * (int64_t)Nx, 8 * (int64_t)Nx, 8 * 4099})));
  Carver cv(c->scratch);
  int32_t* cm = cv.take<int32_t>(Nx);
  double* yd = cv.take<double>(Nx);
  unsigned long long* nz = cv.take<unsigned long long>(4099);      // {zero-variance rows, bits of max |coefficient|, per-workgroup maxima}:
  unsigned long long* mb = nz + 1;                                  // the two results adjacent, one copy to the host
  if (colmap) HIP_TRY(hipMemcpyAsync(cm, colmap, 4 * Nx, hipMemcpyHostToDevice, c->stream));
  if (y) {
    CNA_TRY(reserve_ncorrs(c, nx));
    HIP_TRY(hipMemcpyAsync(yd, y, 8 * Nx, hipMemcpyHostToDevice, c->stream));
  }
  const int rk = (c->resid_rk > 0 && c->resid_n == Nx) ? c->resid_rk : 0;     // one-shot: cna_set_resid_factors
  // the rows leave this pass final: their fixed-point digit planes for the integer local null go out with them
  const bool with_q = y != nullptr && Nx <= 256 && nx > 0 && null_i8_enabled();
  const int KSq = (Nx + 31) / 32;
  if (with_q) CNA_TRY(ensure_xq(c, KSq));
  bool in_place = colmap == nullptr || n_sel == c->N;
  for (int i = 0; colmap && in_place && i < n_sel; ++i) in_place = colmap[i] == i;
  // the walk's last step may have done this pass already (cna_nam_select_hint): same cells, samples in place, nothing
  // regressed out, the same phenotype bit for bit -- then X, planes, coefficients and the two counters are there
  const bool byp = byp_was && y && !keep_idx && in_place && rk == 0 && Nx == c->N && nx == c->n_local &&
                   with_q == c->byp_with_q && (int)c->byp_y.size() == Nx && std::memcmp(y, c->byp_y.data(), 8 * (size_t)Nx) == 0;
  if (byp) {
    nz = (unsigned long long*)c->byp_buf;
    mb = nz + 1;
  }
  if (!byp) CNA_TRY(need_nam(c));           // (a last step that left X instead of the NAM is run again for the NAM)
  if (!byp) CNA_TRY(gram_pre_settle(c));    // (... and a Gram matrix taken under it is dropped; its kernels read the X this pass rewrites)
  const bool fused = !byp && gram_too && y && !keep_idx && in_place && rk == 0 && gram_fused_ok(c, Nx, c->ldx, 32 * KSq);
  if (byp) {
  } else if (fused) {
    void* g = c->gram_buf;
    CNA_TRY(dev_reserve(c, &g, &c->gram_cap, (int64_t)sizeof(double) * Nx * Nx));
    c->gram_buf = (double*)g;
    CNA_TRY(gram_host_reserve(c, Nx));
    c->gram_mirrored = false;
    c->gram_mirror = gram_solo(c) ? (double*)c->h_gram : nullptr;
    const int rc_sg = launch_selgram(c, c->gram_buf, nz, yd, mb, with_q ? (unsigned char*)c->xq : nullptr,
                                     with_q ? c->xq_scale : nullptr, 32 * KSq);
    c->gram_mirror = nullptr;
    CNA_TRY(rc_sg);
  } else {
    CNA_TRY(launch_select_std(c, (colmap && !in_place) ? cm : nullptr, nz, y ? yd : nullptr, y ? mb : nullptr, c->resid_f,
                              c->resid_f ? c->resid_f + (size_t)rk * Nx : nullptr, rk,
                              with_q ? (unsigned char*)c->xq : nullptr, with_q ? c->xq_scale : nullptr, 32 * KSq));
  }
  c->resid_rk = 0;
  if (y && comm_active(c) && c->nranks > 1 && c->nranks <= 64) {
    // the two counters of this pass in ONE collective: every rank's {zero-variance rows, bits of max |coefficient|}
    // gathered (16 bytes per rank), summed / maximised by a one-wave kernel -- the same numbers as an integer sum and
    // a floating-point maximum over the ranks (non-negative doubles and the NaN pattern order like their bit patterns)
    if (!c->pair_buf) HIP_TRY(hipMalloc(&c->pair_buf, 16 * 65));
    unsigned long long* pb = (unsigned long long*)c->pair_buf;
    CNA_TRY(launch_pair_pack(c, nz, mb, pb + 2 * (size_t)c->rank));
    CNA_TRY(comm_allgather_bytes(c, pb + 2 * (size_t)c->rank, pb, 16));
    CNA_TRY(launch_pair_fold(c, pb, c->nranks, nz, mb));
  } else {
    CNA_TRY(comm_allreduce_i64_sum(c, (int64_t*)nz, 1));
    if (y) CNA_TRY(comm_allreduce_f64_max(c, (double*)mb, 1));
  }
  if (!c->h_scal) HIP_TRY(hipHostMalloc(&c->h_scal, 256, hipHostMallocDefault));
  volatile unsigned long long* hs = (volatile unsigned long long*)c->h_scal;
  hs[0] = 0;
  hs[1] = 0;
  HIP_TRY(hipMemcpyAsync((void*)&hs[0], nz, y ? 16 : 8, hipMemcpyDeviceToHost, c->stream));
  // The caller wants the Gram matrix of this X next: its kernels are queued NOW, behind the two scalars on their way to the
  // host, and the host waits for the scalars only -- the device goes from the selection pass (or from the walk's last step
  // that left X as a by-product) straight into the product instead of idling through the host's round trip (30-35 us,
  // profiles/r06_timeline_C2.txt).  Should the scalars say "rows of zero variance", the matrix is dropped with X.
  const bool gram_early = gram_too && y && !fused && !(byp && gram_pre_was);
  if (gram_early) {
    HIP_TRY(hipEventRecord(c->scal_ready, c->stream));
    CNA_TRY(gram_launch_now(c));
    *gram_too = true;
    HIP_TRY(hipEventSynchronize(c->scal_ready));
  } else {
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  const unsigned long long h = hs[0];
  double m = 0.0;
  {
    const unsigned long long bits = hs[1];
    std::memcpy(&m, &bits, 8);
  }
  if (n_zero_out) *n_zero_out = (int64_t)h;
  if (max_abs_out) *max_abs_out = m;
  // (coefficients: meaningful only when no cell had zero variance, the caller checks.)  With ident, X is the standardised
  // NAM of every cell with the samples in place and nothing regressed out: a function of the NAM alone, so a further
  // analysis of the resident dataset that asks for the same selection can keep it (cna_x_identity) and take only its
  // coefficients (cna_ncorrs)
  x_commit(c, true, y != nullptr, with_q, !keep_idx && in_place && rk == 0 && h == 0 && Nx == c->N && nx == c->n_local);
  if (fused) {                                   // what cna_gram_launch does after its kernels
    CNA_TRY(comm_allreduce_f64_sum(c, c->gram_buf, (size_t)Nx * Nx));
    CNA_TRY(gram_host_finish(c, Nx));
    *gram_too = true;
  } else if (byp && gram_pre_was) {
    c->gram_pre = true;                          // X^T X of this X was taken under the walk: cna_gram_launch finds it
    if (gram_too) {
      CNA_TRY(cna_gram_launch(c));
      *gram_too = true;
    }
  }
  if (h != 0 && gram_too && *gram_too) {
    // rows of zero variance: X is void and so is the Gram matrix queued with it (early, fused or taken under the walk)
    // -- cna_gram_fetch refuses until the caller's next selection has a Gram matrix of its own
    c->gram_n = 0;
    *gram_too = false;
  }
  return 0;
}

int cna_select_standardized(cna_ctx* c, const int64_t* keep_idx, int64_t n_keep, const int32_t* colmap, int n_sel,
                            int64_t* n_zero_out, const double* y, double* max_abs_out) {
  return select_standardized_impl(c, keep_idx, n_keep, colmap, n_sel, n_zero_out, y, max_abs_out, nullptr);
}

// select + standardise + coefficients (cna_select_standardized with y) and, when no selected cell has
// zero variance, everything the host would issue next from values it has to wait for anyway -- the
// Gram kernels, the thresholds of the local null from max|ncorrs|, the threshold-only half of the
// local-null pass (cna_null_local_prepare) and the early coefficient column -- in the same call, so
// that none of it waits for the interpreter.  *T_out = 0: nothing beyond the selection was issued.
int cna_select_standardized_fused(cna_ctx* c, const int64_t* keep_idx, int64_t n_keep, const int32_t* colmap, int n_sel,
                                  int64_t* n_zero_out, const double* y, double* max_abs_out, int null_P, int* T_out,
                                  double* thr_out, int* gram_queued, int* coef_queued, int null_col0, const int* null_flag,
                                  int* null_launched) {
  if (T_out) *T_out = 0;
  if (gram_queued) *gram_queued = 0;
  if (coef_queued) *coef_queued = 0;
  if (null_launched) *null_launched = 0;
  int64_t nz = 0;
  double m = 0.0;
  bool gram_done = false;
  CNA_TRY(select_standardized_impl(c, keep_idx, n_keep, colmap, n_sel, &nz, y, &m, &gram_done));
  if (n_zero_out) *n_zero_out = nz;
  if (max_abs_out) *max_abs_out = m;
  if (nz != 0 || !y) return 0;
  double edges[512];
  int T = 0;
  if (null_P >= 1 && T_out && thr_out && c->null.phase != NULL_PENDING) T = cna_reference_thresholds(m, 512, thr_out, edges);
  // The Gram kernels first (round 6): every call issued here costs the host ~5 us and the device has nothing to do
  // until the first kernel arrives -- 0.18 ms between the selection pass and the Gram kernel at 200 000 cells when the
  // coefficient column's five calls went first (rocprofv3 --kernel-trace, profiles/r06_timeline_C2_*.txt).  Whoever
  // consumes the Gram matrix (the eigenpairs) is the longer chain; the coefficient column (short kernels, a copy on
  // its own stream) follows and still reaches the host under the local null.
  if (!gram_done) CNA_TRY(cna_gram_launch(c));
  if (gram_queued) *gram_queued = 1;
  if (T >= 1 && coef_queued && !((c->nranks > 1 || comm_active(c)) && !c->local_view)) {
    CNA_TRY(cna_percell_coef_launch(c));
    *coef_queued = 1;
  }
  if (T < 1) return 0;
  CNA_TRY(null_local_prepare(c, null_P, edges, T, 0, thr_out));
  *T_out = T;
  // ... and, when the conditioned phenotypes of THIS analysis are already resident (columns null_col0 .. null_col0 +
  // null_P of Zc: the draw and cna_condition_phenotypes ran beside the walk -- the caller vouches for it, or *null_flag,
  // set by the library's draw thread when its conditioning has returned, says so at this very moment), the local-null
  // pass itself: it then starts right behind the Gram kernel instead of after the interpreter's next few statements
  if (null_col0 >= 0 && null_launched && (!null_flag || __atomic_load_n(null_flag, __ATOMIC_ACQUIRE) == 1) && c->zc &&
      null_col0 + null_P <= c->zc_cols && c->zc_rows == c->Nx) {
    CNA_TRY(null_local_go(c, null_col0));
    *null_launched = 1;
  }
  return 0;
}

int cna_upload_x(cna_ctx* c, const double* x_local, int64_t n_rows, int n_cols) {
  CHECK_CTX(c);
  if (n_rows < 0 || n_cols < 1 || n_cols > 1024) CNA_FAIL(CNA_EINVAL, "cna_upload_x: bad shape");
  CNA_TRY(x_begin(c, "cna_upload_x", n_rows, n_cols, nullptr));
  HIP_TRY(hipMemsetAsync(c->X, 0, sizeof(double) * std::max<int64_t>(n_rows, 1) * c->ldx, c->stream));
  if (n_rows > 0)
    HIP_TRY(hipMemcpy2DAsync(c->X, sizeof(double) * c->ldx, x_local, sizeof(double) * n_cols,
                             sizeof(double) * n_cols, n_rows, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  x_commit(c, false, false, false, false);
  return 0;
}

// ------------------------------------------------------------------- residualise + PCA
int cna_resid_apply(cna_ctx* c, const double* M, int center) {
  CHECK_CTX(c);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  const bool from_nam = c->x_from_nam;
  CNA_TRY(x_begin(c, "cna_resid_apply"));
  std::vector<double> B;
  int ldb;
  CNA_TRY(xb_operand(c, M, c->Nx, true, B, &ldb));      // M^T
  CNA_TRY(launch_xb(c, (const double*)c->scratch, ldb, c->Nx, center != 0, c->X, c->ldx));
  HIP_TRY(hipStreamSynchronize(c->stream));
  x_commit(c, from_nam, false, false, false);
  return 0;
}

// X <- (X - mean).M^T [/ std] [and ncorrs = X.y/N] for M = I - C.W given by its factors (C: N x r, W: r x N,
// both row-major): one row-local pass (rows.hip:k_resid_lowrank) instead of cna_resid_apply + cna_standardize
// + cna_ncorrs.  y == NULL: no coefficients.  r = 0: centring (and standardisation) only.
int cna_resid_lowrank(cna_ctx* c, const double* C, const double* W, int r, int center, int standardize, const double* y,
                      double* max_abs_out) {
  CHECK_CTX(c);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  if (r < 0 || (r > 0 && (!C || !W))) CNA_FAIL(CNA_EINVAL, "cna_resid_lowrank: bad factors");
  const bool from_nam = c->x_from_nam;
  CNA_TRY(x_begin(c, "cna_resid_lowrank"));
  if (y) CNA_TRY(reserve_ncorrs(c, c->nx));
  RowOperands op;
  CNA_TRY(stage_row_operands(c, op, C, W, r, c->Nx, y));
  CNA_TRY(launch_resid_lowrank(c, op.W, op.Ct, r, center, standardize, op.y, op.maxw));
  double m = 0.0;
  if (y) {
    CNA_TRY(comm_allreduce_f64_max(c, (double*)op.maxw, 1));
    HIP_TRY(hipMemcpyAsync(&m, op.maxw, 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));        // (op holds what the uploads read)
  if (max_abs_out) *max_abs_out = m;
  x_commit(c, from_nam, y != nullptr, false, false);
  return 0;
}

// One ridge of the schedule of _nam.py:142-156 in ONE pass over X and one wait: X <- (X - mean).M^T for M = I - C.W, the
// batch kurtosis of the result (_nam.py:150: its median decides whether the schedule ends here), then -- optimistically --
// the division by the std (_nam.py:159) and the coefficients X.y/N (_association.py:77).  *median_out: np.median of the
// batch kurtosis (formed on the device).  When it is <= 6 the schedule is over and X is final; otherwise the caller
// restores X (selection from the NAM) and continues with cna_resid_lowrank + cna_batch_kurtosis ridge by ridge.
int cna_resid_lowrank_bk(cna_ctx* c, const double* C, const double* W, int r, const double* y, double* max_abs_out,
                         const int32_t* batch_codes, int n_batches, double* median_out) {
  CHECK_CTX(c);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  if (r < 0 || (r > 0 && (!C || !W)) || !y || !batch_codes || n_batches < 1 || n_batches > 256 || !median_out)
    CNA_FAIL(CNA_EINVAL, "cna_resid_lowrank_bk: bad arguments");
  if (c->nx > c->n_pad) CNA_FAIL(CNA_EINVAL, "X larger than the stat buffer");
  const bool from_nam = c->x_from_nam;
  CNA_TRY(x_begin(c, "cna_resid_lowrank_bk"));
  CNA_TRY(reserve_ncorrs(c, c->nx));
  RowOperands op;
  CNA_TRY(stage_row_operands(c, op, C, W, r, c->Nx, y, batch_codes, n_batches));
  CNA_TRY(launch_resid_lowrank(c, op.W, op.Ct, r, 1, 1, op.y, op.maxw, op.order, op.boff, n_batches, c->stat));
  c->stat_space = CNA_MAT_X;
  CNA_TRY(comm_allreduce_f64_max(c, (double*)op.maxw, 1));
  // the median of the batch kurtosis, on the device; its result and max |coefficient| come back with one wait
  double m = 0.0, med = 0.0;
  CNA_TRY(queue_bk_results(c, op.maxw, &m, &med));
  HIP_TRY(hipStreamSynchronize(c->stream));        // (op holds what the uploads read)
  if (max_abs_out) *max_abs_out = m;
  *median_out = med;
  x_commit(c, from_nam, true, false, false);
  return 0;
}

// Selection + QC + the first ridge in ONE pass over the NAM (round 6).  For the demo's call shape -- covariates AND batches
// (demo/demo.ipynb:149) with every cell and every sample kept in place and at most seven batches -- the three passes
// cna_batch_kurtosis(CNA_MAT_NAM) + cna_stat_qc, cna_select_checked and cna_resid_lowrank_bk read the NAM / X three times
// and write X twice; here the rows go NAM -> registers -> X once (rows16.hip:k_rowpass16<.., QC>), and the answers of all
// three come back with one wait:
//   *n_qc_failed   rows whose batch kurtosis is NaN (with <= 7 batches the only way to fail `kurtosis < max(6, 2 median)`,
//                  _nam.py:94-96: the kurtosis of so few batch means is below 6)
//   *n_zero        rows that are constant over the samples (_association.py:182)
//   *median_out    np.median of the batch kurtosis of the residualised rows (_nam.py:150); *max_abs_out as cna_resid_lowrank_bk
// All of n_qc_failed == 0, n_zero == 0, median <= 6: X is final (what the three calls leave).  Anything else: the caller takes
// the three calls (the NAM is untouched).  *done = 0: shape not covered, nothing was queued.
int cna_select_resid_bk(cna_ctx* c, const double* C, const double* W, int r, const double* y, double* max_abs_out,
                        const int32_t* batch_codes, int n_batches, double* median_out, int64_t* n_qc_failed, int64_t* n_zero,
                        int* done) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_select_resid_bk");
  AUTO_FINISH(c);
  if (!done || !median_out || !n_qc_failed || !n_zero || !y || !batch_codes) CNA_FAIL(CNA_EINVAL, "cna_select_resid_bk: null argument");
  *done = 0;
  if (!c->nam_valid && !c->nam_lazy) CNA_FAIL(CNA_ESTATE, "NAM not available");
  const int Nx = c->N;
  if (r < 1 || r > 16 || !C || !W || n_batches < 2 || n_batches > 7 || Nx < 2 || Nx > 128 || c->n_local < 1) return 0;
  for (int s = 0; s < Nx; ++s)
    if (batch_codes[s] < 0 || batch_codes[s] >= n_batches) return 0;      // (a sample of no batch: the general sequence)
  if (c->n_local > c->n_pad) return 0;
  CNA_TRY(need_nam(c));
  CNA_TRY(gram_pre_settle(c));
  CNA_TRY(x_begin(c, "cna_select_resid_bk", c->n_local, Nx, nullptr));
  CNA_TRY(reserve_ncorrs(c, c->nx));
  RowOperands op;
  CNA_TRY(stage_row_operands(c, op, C, W, r, Nx, y, batch_codes, n_batches, 2));   // counters: {QC failures, constant rows}
  int rc;
  {
    ProfScope ps(c, CNA_K_RESID);
    rc = launch_rowpass16(c, c->nam, c->ld, c->X, c->ldx, c->nx, Nx, op.W, op.Ct, r, 1, 1, 1, op.y, op.maxw, op.order, op.boff,
                          n_batches, c->stat, op.counters);
  }
  if (rc < 0) return rc;
  if (rc == 0) {                                   // (CNA_ROWPASS16=0 or a shape the sixteen-row pass does not take: X stays void)
    HIP_TRY(hipStreamSynchronize(c->stream));      // (op holds what the uploads read)
    return 0;
  }
  // every cell is a row of X, also where the NAM has padding columns beyond ldx
  c->stat_space = CNA_MAT_X;
  CNA_TRY(comm_allreduce_f64_max(c, (double*)op.maxw, 1));
  CNA_TRY(comm_allreduce_i64_sum(c, (int64_t*)op.counters, 2));
  double m = 0.0, med = 0.0;
  unsigned long long cnt[2] = {0, 0};
  CNA_TRY(queue_bk_results(c, op.maxw, &m, &med));
  HIP_TRY(hipMemcpyAsync(cnt, op.counters, 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));        // (op holds what the uploads read)
  if (max_abs_out) *max_abs_out = m;
  *median_out = med;
  *n_qc_failed = (int64_t)cnt[0];
  *n_zero = (int64_t)cnt[1];
  x_commit(c, true, true, false, false);
  *done = 1;
  return 0;
}

int cna_standardize(cna_ctx* c, int center) {
  CHECK_CTX(c);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  const bool from_nam = c->x_from_nam;
  CNA_TRY(x_begin(c, "cna_standardize"));
  CNA_TRY(launch_standardize(c, center));
  x_commit(c, from_nam, false, false, false);
  return 0;
}

// X.W (W: Nx x n_w, row-major) queued into *dst, grown to the rows of X x *ldb; B is the host copy of the operand, kept by the
// caller until its next wait
static int project_into(cna_ctx* c, const char* who, const double* W, int n_w, void** dst, int64_t* dst_cap, std::vector<double>& B,
                        int* ldb) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, who);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  if (n_w < 1) CNA_FAIL(CNA_EINVAL, "n_w < 1");
  CNA_TRY(xb_operand(c, W, n_w, false, B, ldb));
  CNA_TRY(dev_reserve(c, dst, dst_cap, (int64_t)sizeof(double) * std::max<int64_t>(c->nx, 1) * *ldb));
  return launch_xb(c, (const double*)c->scratch, *ldb, n_w, false, (double*)*dst, *ldb);
}

int cna_project(cna_ctx* c, const double* W, int n_w, double* out_local) {
  std::vector<double> B;
  int ldb;
  CNA_TRY(project_into(c, "cna_project", W, n_w, &c->scratch2, &c->scratch2_cap, B, &ldb));
  const double* out = (const double*)c->scratch2;
  if (c->nx > 0)
    HIP_TRY(hipMemcpy2DAsync(out_local, sizeof(double) * n_w, out, sizeof(double) * ldb, sizeof(double) * n_w,
                             c->nx, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

// cna_project with the result left on the device (rows of X x n_w), to be read with
// cna_fetch_rows(CNA_MAT_PROJ, ...) in whatever row order the caller wants
int cna_project_keep(cna_ctx* c, const double* W, int n_w) {
  std::vector<double> B;
  int ldb;
  CNA_TRY(project_into(c, "cna_project_keep", W, n_w, &c->proj, &c->proj_cap, B, &ldb));
  HIP_TRY(hipStreamSynchronize(c->stream));               // B is a local
  c->proj_ld = ldb;
  c->proj_cols = n_w;
  c->proj_rows = c->nx;
  c->proj_valid = true;
  return 0;
}

// ------------------------------------------------------------------------- association
int cna_x_identity(cna_ctx* c, int* yes) {
  CHECK_CTX(c);
  if (!yes) CNA_FAIL(CNA_EINVAL, "cna_x_identity: yes is required");
  *yes = (c->x_valid && c->x_ident && !c->auto_pending) ? 1 : 0;
  return 0;
}

int cna_ncorrs(cna_ctx* c, const double* y, double* out_local, double* max_abs) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_ncorrs");
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  if (!y) CNA_FAIL(CNA_EINVAL, "cna_ncorrs: y is required");
  CNA_TRY(reserve_ncorrs(c, c->nx));
  RowOperands op;                            // (the phenotype and the max words alone)
  CNA_TRY(stage_row_operands(c, op, nullptr, nullptr, 0, c->Nx, y));
  CNA_TRY(launch_ncorrs(c, op.y, op.maxw));
  CNA_TRY(comm_allreduce_f64_max(c, (double*)op.maxw, 1));
  double m = 0.0;
  HIP_TRY(hipMemcpyAsync(&m, op.maxw, 8, hipMemcpyDeviceToHost, c->stream));
  if (out_local && c->nx > 0)
    HIP_TRY(hipMemcpyAsync(out_local, c->ncorrs, 8 * c->nx, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (max_abs) *max_abs = m;
  c->ncorrs_valid = true;
  void_coef(c);                     // (the columns copied from the coefficients this call has replaced)
  return 0;
}

}  // extern "C"
