// The local-null pass (prepare / go / collect), the conditioned phenotypes it reads and the per-cell columns that ride
// on it: host orchestration only -- the kernels are in mfma.hip, null_i8.hip, rows.hip and stats.hip.
#include "common.h"
#include <sched.h>
#include <cmath>
#include <cstring>

static void guess_from_thr(const double* thr, int T, double* thr0, double* inv_step) {
  *thr0 = T > 0 ? thr[0] : 0.0;
  const double step = T > 1 ? thr[1] - thr[0] : 0.0;
  *inv_step = step > 0 ? 1.0 / step : 0.0;
}

// cut[t] = smallest double a >= 0 with fl(fl(a/N)^2) >= edges[t]: the reference's test on
// z^2 = (|x.yc|/N)^2 (_association.py:99, _stats.py:47-54) moved onto the raw dot product.  Both
// roundings are monotone, so a bisection over the bit patterns of the positive doubles finds the
// exact switch point.  The cuts are (nearly) an arithmetic progression cut0 + t*step; eps bounds,
// in steps, how far any cut is from that line (the kernel trusts floor((x-cut0)/step) outside
// +-eps of a cut and walks the table otherwise).
static void exact_cuts(const double* edges, int T, int Nx, std::vector<double>& cuts, double* cut0,
                       double* inv_step, double* eps) {
  cuts.resize(T);
  const double dn = (double)Nx;
  for (int t = 0; t < T; ++t) {
    const double e = edges[t];
    auto ok = [&](double a) { volatile double z = a / dn; volatile double z2 = z * z; return z2 >= e; };
    if (e <= 0.0 || ok(0.0)) { cuts[t] = 0.0; continue; }
    // bracket the switch point around N*sqrt(e) (a few ulps wide), then bisect the bit patterns
    uint64_t lo = 0, hi = 0x7ff0000000000000ull;          // lo fails, hi (+inf) passes
    const double guess = dn * std::sqrt(e);
    uint64_t g;
    std::memcpy(&g, &guess, 8);
    if (guess > 0.0 && g > 64 && g < hi - 64) {
      double a;
      uint64_t b = g - 64;
      std::memcpy(&a, &b, 8);
      if (!ok(a)) lo = b;
      b = g + 64;
      std::memcpy(&a, &b, 8);
      if (ok(a)) hi = b;
    }
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      double a;
      std::memcpy(&a, &mid, 8);
      if (ok(a)) hi = mid; else lo = mid;
    }
    std::memcpy(&cuts[t], &hi, 8);
  }
  *cut0 = cuts[0];
  *inv_step = 0.0;
  *eps = 2.0;                                             // eps >= 1: always walk the table
  if (T >= 3 && cuts[T - 1] > cuts[0]) {
    const double step = (cuts[T - 1] - cuts[0]) / (T - 1);
    double dev = 0.0;
    for (int t = 0; t < T; ++t) dev = std::max(dev, std::fabs(cuts[t] - (*cut0 + t * step)) / step);
    *inv_step = 1.0 / step;
    *eps = 2.0 * dev + 1e-9;
    if (!(*eps < 0.25)) *eps = 2.0;
  }
}

static int ensure_zc(cna_ctx* c, int N, int P, hipStream_t st) {
  const int ldy = round_up(P, 64) + 64;   // one spare tile: a resident read may start at any column
  // = ldx of a working matrix with N samples, INCLUDING the bank-spreading pad quad x_ld() adds at
  // N = 157...160 / 189...192 / 221...224: the local-null kernel loads ldx rows of Zc (the matching
  // pad columns of X are zero, but 0 * whatever-lies-past-the-buffer is only 0 while that is finite)
  const int rows = x_ld(N);
  void* p = c->zc;
  CNA_TRY(dev_reserve(c, &p, &c->zc_cap, (int64_t)sizeof(double) * rows * ldy));
  c->zc = (double*)p;
  HIP_TRY(hipMemsetAsync(c->zc, 0, sizeof(double) * rows * ldy, st));   // zero pads (rows >= N, cols >= P)
  c->zc_ld = ldy;
  c->zc_cols = P;
  c->zc_rows = N;
  return 0;
}

// The two blocks of a pass, each laid out in one place.  Device: the pieces of c->scratch, in order ...
static NullCarve null_carve(void* scratch, int P, int T) {
  Carver cv(scratch);
  NullCarve k;
  k.cuts = cv.take<double>(T);
  k.hist = cv.take<unsigned long long>((int64_t)P * T);
  k.tails = cv.take<int64_t>((int64_t)P * T);
  k.sums = cv.take<int64_t>(T);
  k.obs_edges = cv.take<double>(T);
  k.obs_thr = cv.take<double>(T);
  k.obs_hist = cv.take<unsigned long long>(2 * (int64_t)T);
  k.obs_tails = cv.take<int64_t>(2 * (int64_t)T);
  return k;
}
static int64_t null_carve_bytes(int P, int T) {            // ... and their sizes, in the same order
  const int64_t t = 8 * (int64_t)T, pt = t * P;
  return carve_bytes({t, pt, pt, t, t, t, 2 * t, 2 * t});
}
// Pinned (c->h_res): with tails the observed counts, the staging area and the status word all move behind them
static NullHostLayout null_host_layout(int P, int T, int want_tails) {
  NullHostLayout h;
  h.tails = h.sums + 8 * (int64_t)T;
  h.obs = h.tails + (want_tails ? 8 * (int64_t)P * T : 0);
  h.stage = h.obs + 16 * (int64_t)T;
  h.status = h.stage + 24 * (int64_t)T;
  h.bytes = h.status + 16;
  return h;
}

// One local-null pass in two halves.  prepare: everything that needs only the thresholds (exact cuts, their upload, the
// threshold counts of the observed coefficients) -- the caller can issue it while the permuted phenotypes are still on
// their way.  go: the kernel and its reductions; results land in the pinned buffer h_res (NullHostLayout) and null_done
// fires when they are there.  Nothing else may use c->scratch between the two (NO_NULL_PENDING).
int null_local_prepare(cna_ctx* c, int P, const double* edges, int T, int want_tails, const double* thr) {
  NullPass& np = c->null;
  CellColumns& cc = c->cells;
  if (cc.bins_pending) {          // the per-cell counts of the previous pass read its thresholds out of c->scratch (coef_stream)
    HIP_TRY(hipStreamWaitEvent(c->stream, cc.bins_copied, 0));
    cc.bins_pending = false;
  }
  if (P < 1 || T < 1) CNA_FAIL(CNA_EINVAL, "cna_null_local: P and T must be positive");
  if (np.phase == NULL_PENDING) CNA_FAIL(CNA_ESTATE, "a local-null pass is still pending: fetch it first");
  for (int t = 1; t < T; ++t)
    if (!(edges[t] >= edges[t - 1])) CNA_FAIL(CNA_EINVAL, "cna_null_local: edges must ascend");
  np.phase = NULL_IDLE;
  cc.fdr_inline = false;
  std::vector<double> cuts;
  exact_cuts(edges, T, c->Nx, cuts, &np.cut0, &np.inv_step, &np.eps);
  const NullHostLayout h = null_host_layout(P, T, want_tails);
  HIP_TRY(hipEventSynchronize(c->stage_done));            // uploads of the previous pass out of the staging area (long done)
  if (h.bytes > c->h_res_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->h_res) HIP_TRY(hipHostFree(c->h_res));
    c->h_res = nullptr;
    HIP_TRY(hipHostMalloc(&c->h_res, (size_t)h.bytes, hipHostMallocDefault));
    c->h_res_cap = h.bytes;
  }
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, null_carve_bytes(P, T)));
  const NullCarve k = null_carve(c->scratch, P, T);
  char* hr = (char*)c->h_res;
  double* st = (double*)(hr + h.stage);                   // cuts | edges | thr
  np.has_obs = 0;
  if (thr) {
    // threshold counts of the observed coefficients (cna_obs_counts) ride along: tiny kernels in front
    // of the long one, results in the same pinned block
    if (!c->ncorrs_valid) CNA_FAIL(CNA_ESTATE, "threshold counts need cna_ncorrs");
    guess_from_thr(thr, T, &np.thr0, &np.thr_step);
    std::memcpy(st + T, edges, 8 * (size_t)T);
    std::memcpy(st + 2 * T, thr, 8 * (size_t)T);
    HIP_TRY(hipMemcpyAsync(k.obs_edges, st + T, 8 * T, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(k.obs_thr, st + 2 * T, 8 * T, hipMemcpyHostToDevice, c->stream));
    CNA_TRY(launch_obs_counts(c, k.obs_edges, k.obs_thr, T, np.thr0, np.thr_step, k.obs_hist));
    CNA_TRY(comm_allreduce_i64_sum(c, (int64_t*)k.obs_hist, (size_t)2 * T));
    CNA_TRY(launch_suffix_sum(c, k.obs_hist, 2, T, k.obs_tails));
    HIP_TRY(hipMemcpyAsync(hr + h.obs, k.obs_tails, 16 * (size_t)T, hipMemcpyDeviceToHost, c->stream));
    np.has_obs = 1;
  }
  std::memcpy(st, cuts.data(), 8 * (size_t)T);
  HIP_TRY(hipMemcpyAsync(k.cuts, st, 8 * T, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->stage_done, c->stream));
  np.host = h;
  np.P = P;
  np.T = T;
  np.has_tails = want_tails;
  np.phase = NULL_PREPARED;
  return 0;
}

int null_local_go(cna_ctx* c, int col0) {
  NullPass& np = c->null;
  CellColumns& cc = c->cells;
  if (np.phase != NULL_PREPARED) CNA_FAIL(CNA_ESTATE, "local-null pass not prepared");
  np.phase = NULL_IDLE;
  const int P = np.P, T = np.T;
  if (!c->zc || col0 < 0 || col0 + P > c->zc_cols || c->zc_rows != c->Nx ||
      c->zc_cap < (int64_t)sizeof(double) * c->ldx * c->zc_ld)
    CNA_FAIL(CNA_ESTATE, "no conditioned phenotypes resident for these columns");
  const NullCarve k = null_carve(c->scratch, P, T);
  char* hr = (char*)c->h_res;
  // columns beyond col0+P inside the last 64-wide tile are other phenotypes: the kernel only flushes counters of p < P,
  // and reads stay inside the zero-padded leading dimension.  Only the sums over permutations wanted (the analysis): the
  // integer matrix cores do the products (null_i8.hip: exact counts, outputs near a cut rechecked in f64).
  // The per-cell half of the FDR lookup -- how many thresholds lie at or below |coef_i| -- needs nothing from the null: its
  // kernel goes IN FRONT of the null on the main stream (beside it, on the coefficient stream, it was starved for the
  // whole pass: 2.1 ms at 2M cells, profiles/r06_kernel_stats_C4.csv), its 2 bytes per cell cross PCIe under the null
  // from the coefficient stream, and the host puts table and counts together (cna_percell_fdr_copy_early).
  const bool inline_fdr = cc.coef_early && np.has_obs && T <= 512;
  if (inline_fdr) {
    const int64_t n_out = c->local_view ? c->n_local : c->n_global;
    void* bp = cc.bins_dev;
    CNA_TRY(dev_reserve(c, &bp, &cc.bins_cap, 2 * std::max<int64_t>(std::max(c->n_pad, n_out), 1)));
    cc.bins_dev = (unsigned short*)bp;
    if (2 * n_out > cc.h_bins_cap) {
      if (cc.h_bins) HIP_TRY(hipHostFree(cc.h_bins));
      cc.h_bins = nullptr;
      HIP_TRY(hipHostMalloc((void**)&cc.h_bins, (size_t)std::max<int64_t>(2 * n_out, 64), hipHostMallocDefault));
      cc.h_bins_cap = 2 * n_out;
    }
    hipStream_t cs = c->coef_stream;
    CNA_TRY(launch_percell_bins(c, c->stream, cc.coef_dev, k.obs_thr, T, np.thr0, np.thr_step, cc.bins_dev));
    HIP_TRY(hipEventRecord(c->stage_done, c->stream));      // (a later point of the stream than the one prepare recorded)
    HIP_TRY(hipStreamWaitEvent(cs, c->stage_done, 0));
    if (n_out > 0) HIP_TRY(hipMemcpyAsync(cc.h_bins, cc.bins_dev, 2 * (size_t)n_out, hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipEventRecord(cc.bins_copied, cs));
    cc.bins_pending = true;
  }
  int* i8_status = nullptr;
  int64_t* sums = k.sums;
  np.i8_last = false;
  if (!np.has_tails && null_i8_eligible(c, P, T, np.cut0, np.inv_step, np.eps))
    CNA_TRY(launch_null_local_i8(c, c->zc + col0, c->zc_ld, P, k.cuts, T, np.cut0, np.inv_step, np.eps, &sums, &i8_status));
  np.i8_last = i8_status != nullptr;
  np.col0 = col0;
  np.status_off = -1;
  if (i8_status) {
    // Round 6: the f64 kernel is no longer queued behind the integer pass as a stand-by (two guarded launches, the
    // reductions of an empty histogram and the pick: 45 us of device time and seven launches on the tail of EVERY call,
    // rocprofv3 timeline profiles/r06_timeline_C2.txt).  The pass's status word travels with its sums; should it be
    // raised (recheck queue overflow: never seen outside the test that forces it) whoever collects the pass runs the f64
    // kernel then (null_local_collect).  Several ranks: the word is summed over the ranks, so that all of them decide alike.
    CNA_TRY(comm_allreduce_i64_sum(c, sums, (size_t)T));
    int64_t* stw = (int64_t*)i8_status;                    // (the word's upper half is zero: launch_null_local_i8 clears the block)
    CNA_TRY(comm_allreduce_i64_sum(c, stw, 1));
    np.status_off = np.host.status;
    HIP_TRY(hipMemcpyAsync(hr + np.host.status, stw, 8, hipMemcpyDeviceToHost, c->stream));
  } else {
    CNA_TRY(launch_null_local(c, c->zc + col0, c->zc_ld, P, k.cuts, T, np.cut0, np.inv_step, np.eps, k.hist, nullptr));
    // suffix sums and the sum over permutations are linear: when only the sums are wanted the ranks
    // exchange T integers instead of the P x T histogram
    if (np.has_tails) CNA_TRY(comm_allreduce_i64_sum(c, (int64_t*)k.hist, (size_t)P * T));
    CNA_TRY(launch_suffix_sum(c, k.hist, P, T, k.tails));
    CNA_TRY(launch_tail_sums(c, k.tails, P, T, sums));
    if (!np.has_tails) CNA_TRY(comm_allreduce_i64_sum(c, sums, (size_t)T));
  }
  HIP_TRY(hipMemcpyAsync(hr + np.host.sums, sums, 8 * (size_t)T, hipMemcpyDeviceToHost, c->stream));
  if (inline_fdr) {
    // the caller already has the coefficient column (cna_percell_coef_launch): the FDR column can follow the null without
    // the host in between -- behind the null only the FDR table is formed from the tail sums and the observed counts
    // (still in the scratch carve of the prepare half) and sent (2.4 KB).  (Round 2 stored the finished 8-byte column
    // from a kernel behind the null: 16 MB over PCIe on the critical path at 2M cells.)
    double* tab = cc.coef_dev + 4 * c->n_pad;
    CNA_TRY(launch_fdr_table(c, sums, k.obs_tails, T, P, tab, tab + 512));
    if (!cc.h_tab) HIP_TRY(hipHostMalloc((void**)&cc.h_tab, 8 * 512, hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(cc.h_tab, tab + 512, 8 * (size_t)T, hipMemcpyDeviceToHost, c->stream));
    cc.fdr_inline = true;
  }
  if (np.has_tails)
    HIP_TRY(hipMemcpyAsync(hr + np.host.tails, k.tails, 8 * (size_t)P * T, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(c->null_done, c->stream));
  cc.fdr_early_copied = false;
  cc.fdr_early_dst = nullptr;
  cc.fdr_early_served = false;
  np.phase = NULL_PENDING;
  return 0;
}

static int null_local_collect(cna_ctx* c, int64_t* tails_out, int64_t* sums_out, int64_t* ranks_out = nullptr,
                              int64_t* numdet_out = nullptr) {
  NullPass& np = c->null;
  if (np.phase != NULL_PENDING) CNA_FAIL(CNA_ESTATE, "no local-null pass pending");
  np.phase = NULL_IDLE;
  HIP_TRY(hipEventSynchronize(c->null_done));
  const int P = np.P, T = np.T;
  char* hr = (char*)c->h_res;
  const int64_t status_off = np.status_off;
  if (status_off >= 0 && *(volatile const int64_t*)(hr + status_off) != 0) {
    // the integer pass gave up (on some rank): the same counts from the f64 kernel, now.  The FDR table that followed
    // the pass on the device was made of the wrong sums: fdr_inline goes first, the status word's offset after the rerun
    // (the rule at NullPass).  The cuts are uploaded again from the pinned copy the prepare half kept, into the pass's
    // carve of c->scratch (still reserved: the buffer only grows), in stream order; X and Zc are the launch's.
    c->cells.fdr_inline = false;
    const NullCarve k = null_carve(c->scratch, P, T);
    HIP_TRY(hipMemcpyAsync(k.cuts, hr + np.host.stage, 8 * (size_t)T, hipMemcpyHostToDevice, c->stream));
    CNA_TRY(launch_null_local(c, c->zc + np.col0, c->zc_ld, P, k.cuts, T, np.cut0, np.inv_step, np.eps, k.hist, nullptr));
    CNA_TRY(launch_suffix_sum(c, k.hist, P, T, k.tails));
    CNA_TRY(launch_tail_sums(c, k.tails, P, T, k.sums));
    CNA_TRY(comm_allreduce_i64_sum(c, k.sums, (size_t)T));
    HIP_TRY(hipMemcpyAsync(hr + np.host.sums, k.sums, 8 * (size_t)T, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  np.status_off = -1;                                    // (after the rerun)
  if (ranks_out || numdet_out) {
    if (!np.has_obs) CNA_FAIL(CNA_EINVAL, "the pending pass was launched without thresholds");
    if (ranks_out) std::memcpy(ranks_out, hr + np.host.obs, 8 * (size_t)T);
    if (numdet_out) std::memcpy(numdet_out, hr + np.host.obs + 8 * (size_t)T, 8 * (size_t)T);
  }
  if (sums_out) std::memcpy(sums_out, hr + np.host.sums, 8 * (size_t)T);
  if (tails_out) {
    if (!np.has_tails) CNA_FAIL(CNA_EINVAL, "the pending pass was launched without want_tails");
    std::memcpy(tails_out, hr + np.host.tails, 8 * (size_t)P * T);
  }
  return 0;
}

static int null_local_on_resident(cna_ctx* c, int col0, int P, const double* edges, int T, int64_t* tails_out,
                                  int64_t* sums_out) {
  CNA_TRY(null_local_prepare(c, P, edges, T, tails_out != nullptr, nullptr));
  CNA_TRY(null_local_go(c, col0));
  return null_local_collect(c, tails_out, sums_out);
}

extern "C" {

// thresholds = np.arange(maxcorr/4, maxcorr, maxcorr/400) and edges = thr**2 - 1e-8 - 1e-5*thr**2
// exactly as numpy evaluates them (_association.py:101-103, _stats.py:47): arange's length is
// ceil((stop - start) / step) and its values start + i*delta with delta = (start + step) - start;
// the edge expression rounds after every operation, left to right.  Returns T (0: out of range).
int cna_reference_thresholds(double maxabs, int cap, double* thr, double* edges) {
#pragma clang fp contract(off)
  const double maxcorr = maxabs > 0.001 ? maxabs : 0.001;
  if (!(maxcorr < 1e300)) return 0;
  const double start = maxcorr / 4, stop = maxcorr, step = maxcorr / 400;
  const double len = std::ceil((stop - start) / step);
  if (!(len >= 1) || len > cap) return 0;
  const int T = (int)len;
  const double next = start + step;
  const double delta = next - start;
  for (int i = 0; i < T; ++i) {
    volatile double t = i == 0 ? start : (i == 1 ? next : start + (double)i * delta);
    thr[i] = t;
    volatile double z2 = t * t;
    volatile double a = z2 - 1e-8;
    volatile double b = 1e-5 * z2;
    edges[i] = a - b;
  }
  return T;
}

int cna_null_local_prepare(cna_ctx* c, int P, const double* edges, int T, int want_tails, const double* thr) {
  CHECK_CTX(c);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  if (!edges) CNA_FAIL(CNA_EINVAL, "cna_null_local_prepare: edges required");
  return null_local_prepare(c, P, edges, T, want_tails, thr);
}

int cna_null_local_launch(cna_ctx* c, int col0, int P, const double* edges, int T, int want_tails, const double* thr) {
  CHECK_CTX(c);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  if (edges) CNA_TRY(null_local_prepare(c, P, edges, T, want_tails, thr));
  else if (c->null.phase != NULL_PREPARED || P != c->null.P || T != c->null.T)   // second half of a prepared pass
    CNA_FAIL(CNA_ESTATE, "cna_null_local_launch without edges needs a matching cna_null_local_prepare");
  return null_local_go(c, col0);
}

int cna_null_local_fetch(cna_ctx* c, int64_t* tails_out, int64_t* tail_sums_out, int64_t* ranks_out,
                         int64_t* num_detected_out) {
  CHECK_CTX(c);
  return null_local_collect(c, tails_out, tail_sums_out, ranks_out, num_detected_out);
}

// A pass that was launched and never collected (the caller raised between launch and fetch: a bad `ks`, a failed
// draw, Ctrl-C): wait for its kernels, drop its results and the prepared half, so that the next analysis on this
// context starts clean instead of failing with "still pending".  A no-op when nothing is pending.
int cna_null_local_discard(cna_ctx* c) {
  CHECK_CTX(c);
  if (c->null.phase.exchange(NULL_IDLE) != NULL_PENDING) return 0;
  HIP_TRY(hipEventSynchronize(c->null_done));
  return 0;
}

int cna_null_local_i8_stats(cna_ctx* c, int* used_out, int64_t* rechecked_out, int* fallback_out) {
  CHECK_CTX(c);
  unsigned long long v[2] = {0, 0};
  if (c->null.i8_last) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(v, c->i8_qcount, 16, hipMemcpyDeviceToHost));
  }
  if (used_out) *used_out = c->null.i8_last ? 1 : 0;
  if (rechecked_out) *rechecked_out = (int64_t)v[0];
  if (fallback_out) *fallback_out = (int)(v[1] & 0xffffffffull) != 0;
  return 0;
}

int cna_null_local(cna_ctx* c, const double* Yc, int P, const double* edges, int T, int64_t* tails_out) {
  CHECK_CTX(c);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  if (P < 1) CNA_FAIL(CNA_EINVAL, "cna_null_local: P must be positive");
  CNA_TRY(ensure_zc(c, c->Nx, P, c->stream));
  HIP_TRY(hipMemcpy2DAsync(c->zc, sizeof(double) * c->zc_ld, Yc, sizeof(double) * P, sizeof(double) * P, c->Nx,
                           hipMemcpyHostToDevice, c->stream));
  return null_local_on_resident(c, 0, P, edges, T, tails_out, nullptr);
}

int cna_null_local_resident(cna_ctx* c, int col0, int P, const double* edges, int T, int64_t* tails_out,
                            int64_t* tail_sums_out) {
  CHECK_CTX(c);
  if (!c->x_valid) CNA_FAIL(CNA_ESTATE, "X not available");
  return null_local_on_resident(c, col0, P, edges, T, tails_out, tail_sums_out);
}

int cna_condition_phenotypes(cna_ctx* c, const double* M, const double* Y, int N, int P) {
  CHECK_CTX(c);
  if (P < 1) CNA_FAIL(CNA_EINVAL, "P must be positive");
  if (N < 2) CNA_FAIL(CNA_EINVAL, "need at least two samples");
  if (c->null.phase == NULL_PENDING) CNA_FAIL(CNA_ESTATE, "a local-null pass is still pending: fetch it first");
  // Sample-space only, so it runs on the second stream: the caller may issue it while the diffusion
  // kernels of the same analysis are still executing on the main stream.  Synchronised before
  // returning, hence complete for every later consumer on either stream.
  hipStream_t st = c->copy_stream;
  CNA_TRY(ensure_zc(c, N, P, st));
  void* g = c->gt;
  CNA_TRY(dev_reserve(c, &g, &c->gt_cap, carve_bytes({8 * (int64_t)N * N, 8 * (int64_t)N * P})));
  c->gt = g;
  Carver cv(c->gt);
  double* Md = cv.take<double>((int64_t)N * N);
  double* Yd = cv.take<double>((int64_t)N * P);
  HIP_TRY(hipMemcpyAsync(Md, M, 8 * (size_t)N * N, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(Yd, Y, 8 * (size_t)N * P, hipMemcpyHostToDevice, st));
  CNA_TRY(launch_condition(c, st, Md, Yd, N, P, c->zc, c->zc_ld));
  HIP_TRY(hipStreamSynchronize(st));               // host buffers may be released
  return 0;
}

int cna_obs_counts(cna_ctx* c, const double* edges, const double* thr, int T, int64_t* ranks_out,
                   int64_t* num_detected_out) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_obs_counts");
  if (!c->ncorrs_valid) CNA_FAIL(CNA_ESTATE, "cna_obs_counts needs cna_ncorrs");
  if (T < 1) CNA_FAIL(CNA_EINVAL, "T < 1");
  double thr0, inv_step;
  guess_from_thr(thr, T, &thr0, &inv_step);
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap, carve_bytes({8 * (int64_t)T, 8 * (int64_t)T, 16 * (int64_t)T, 16 * (int64_t)T})));
  Carver cv(c->scratch);
  double* ed = cv.take<double>(T);
  double* td = cv.take<double>(T);
  unsigned long long* hist = cv.take<unsigned long long>(2 * T);
  int64_t* tails = cv.take<int64_t>(2 * T);
  HIP_TRY(hipMemcpyAsync(ed, edges, 8 * T, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(td, thr, 8 * T, hipMemcpyHostToDevice, c->stream));
  CNA_TRY(launch_obs_counts(c, ed, td, T, thr0, inv_step, hist));
  CNA_TRY(comm_allreduce_i64_sum(c, (int64_t*)hist, (size_t)2 * T));
  CNA_TRY(launch_suffix_sum(c, hist, 2, T, tails));
  std::vector<int64_t> h(2 * T);
  HIP_TRY(hipMemcpyAsync(h.data(), tails, 16 * T, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (ranks_out) std::memcpy(ranks_out, h.data(), 8 * T);
  if (num_detected_out) std::memcpy(num_detected_out, h.data() + T, 8 * T);
  return 0;
}

static int ensure_cell_pinned(cna_ctx* c, int64_t n_out) {
  const int64_t need = 16 * std::max<int64_t>(n_out, 1);
  if (need > c->cells.h_cell_cap) {
    if (c->cells.h_cell) HIP_TRY(hipHostFree(c->cells.h_cell));
    c->cells.h_cell = nullptr;
    void_coef(c);                   // (the pinned block that held the columns is gone)
    HIP_TRY(hipHostMalloc(&c->cells.h_cell, (size_t)need, hipHostMallocDefault));
    c->cells.h_cell_cap = need;
  }
  return 0;
}

// The coefficient column of the result (data.obs[key_added], _association.py:230-233) depends on
// the observed phenotype only, not on the permutation null: queued here -- ahead of the local-null
// kernel in stream order, copied out on the second stream -- it reaches the host while that kernel
// runs, and the caller can write the column before the null is even finished.
int cna_percell_coef_launch(cna_ctx* c) {
  CHECK_CTX(c);
  if (!c->ncorrs_valid || !c->x_from_nam) CNA_FAIL(CNA_ESTATE, "cna_percell_coef_launch needs cna_select + cna_ncorrs");
  if ((c->nranks > 1 || comm_active(c)) && !c->local_view)
    CNA_FAIL(CNA_ESTATE, "cna_percell_coef_launch: replicated multi-rank outputs are assembled by cna_percell_fdr");
  const int64_t n_out = c->local_view ? c->n_local : c->n_global;
  CNA_TRY(ensure_cell_pinned(c, n_out));
  void* p = c->cells.coef_dev;
  CNA_TRY(dev_reserve(c, &p, &c->cells.coef_dev_cap, 32 * std::max<int64_t>(c->n_pad, 1) + 16 * 512));   // coef, coef_u, fdr, fdr_u, FDR table
  c->cells.coef_dev = (double*)p;
  double* tmp = c->cells.coef_dev;
  double* out = tmp;
  CNA_TRY(launch_percell_fdr(c, nullptr, nullptr, 0, 0.0, 0.0, tmp, nullptr));
  if (c->orig_idx) {
    out = c->cells.coef_dev + c->n_pad;
    CNA_TRY(launch_unpermute2(c, tmp, nullptr, c->orig_idx, c->n_local, out, nullptr));
  }
  HIP_TRY(hipEventRecord(c->cells.coef_ready, c->stream));
  hipStream_t cs = c->coef_stream;   // not copy_stream: the helper thread's conditioning call waits on that one
  HIP_TRY(hipStreamWaitEvent(cs, c->cells.coef_ready, 0));
  if (n_out > 0)
    HIP_TRY(hipMemcpyAsync(c->cells.h_cell, out, 8 * n_out, hipMemcpyDeviceToHost, cs));
  HIP_TRY(hipEventRecord(c->cells.coef_copied, cs));
  c->cells.coef_early = true;
  return 0;
}

int cna_percell_coef_wait(cna_ctx* c, double** coef_ptr) {
  CHECK_CTX(c);
  if (!coef_ptr) CNA_FAIL(CNA_EINVAL, "cna_percell_coef_wait: coef_ptr is required");
  if (!c->cells.coef_early) CNA_FAIL(CNA_ESTATE, "cna_percell_coef_wait without cna_percell_coef_launch");
  HIP_TRY(hipEventSynchronize(c->cells.coef_copied));
  *coef_ptr = (double*)c->cells.h_cell;
  return 0;
}

// The FDR column of the pending local-null pass, copied into the caller's own storage as soon as the device has
// stored it in the pinned block -- meant for a helper thread while the main thread is busy on the host (the
// samples x samples SVD outlasts the local null by ~0.5 ms at 2M x 200 and the copy of 16 MB takes 0.4 ms).
// Touches nothing but the event, the pinned block and one flag.  *done = 0: not applicable (the column does not
// follow this pass on the device), nothing was copied.
int cna_percell_fdr_copy_early(cna_ctx* c, double* dst, int64_t n, int nthreads, int* done) {
  CHECK_CTX(c);
  if (!dst || !done) CNA_FAIL(CNA_EINVAL, "cna_percell_fdr_copy_early: dst and done are required");
  *done = 0;
  const int64_t n_out = c->local_view ? c->n_local : c->n_global;
  if (!c->cells.coef_early || !c->cells.fdr_inline || c->null.phase != NULL_PENDING || !c->cells.h_cell || n != n_out) return 0;
  // (the main thread's cna_percell_fdr_pinned waits while this one is at work instead of doing the same work again)
  struct Flight { std::atomic<int>& f; Flight(std::atomic<int>& f_) : f(f_) { f.store(1); } ~Flight() { f.store(0); } } flight(c->cells.fdr_early_inflight);
  HIP_TRY(hipEventSynchronize(c->cells.bins_copied));
  HIP_TRY(hipEventSynchronize(c->null_done));
  const int64_t status_off = c->null.status_off;
  if (status_off >= 0 && *(volatile int64_t*)((char*)c->h_res + status_off) != 0)
    return 0;                                   // the integer pass gave up: its table is void (cna_null_local_fetch reruns in f64)
  if (!c->cells.fdr_inline) return 0;           // ... and the rerun is over already (the rule at NullPass)
  if (cna_host_expand_u16(dst, c->cells.h_bins, n, c->cells.h_tab, c->null.T, nthreads) != 0)
    CNA_FAIL(CNA_ESTATE, "cna_percell_fdr_copy_early: expansion failed");
  c->cells.fdr_early_dst = dst;
  c->cells.fdr_early_copied = true;
  *done = 1;
  return 0;
}

// 1 when the FDR column cna_percell_fdr_pinned last returned is the one cna_percell_fdr_copy_early copied
int cna_percell_fdr_copied_early(cna_ctx* c, int* yes) {
  CHECK_CTX(c);
  if (!yes) CNA_FAIL(CNA_EINVAL, "cna_percell_fdr_copied_early: yes is required");
  *yes = c->cells.fdr_early_copied && c->cells.fdr_inline && c->cells.fdr_early_served;
  return 0;
}

int cna_percell_fdr_pinned(cna_ctx* c, const double* thr, const double* runmin_fdr, int T, double** coef_ptr,
                           double** fdr_ptr) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_percell_fdr_pinned");
  if (!coef_ptr) CNA_FAIL(CNA_EINVAL, "cna_percell_fdr_pinned: coef_ptr is required");
  const int64_t n_out = c->local_view ? c->n_local : c->n_global;
  CNA_TRY(ensure_cell_pinned(c, n_out));
  double* hc = (double*)c->cells.h_cell;
  const bool want_fdr = fdr_ptr && thr && runmin_fdr && T > 0;
  if (c->cells.coef_early) HIP_TRY(hipEventSynchronize(c->cells.coef_copied));     // coefficients already on the host
  if (c->cells.coef_early && c->cells.fdr_inline && want_fdr && T == c->null.T && c->null.phase != NULL_PENDING) {
    // the coefficient column is in the pinned block; the FDR column is the table that followed the local null looked
    // up with the per-cell counts that left before it -- already put together in the caller's own storage by
    // cna_percell_fdr_copy_early (then that is what *fdr_ptr names), else put together here
    HIP_TRY(hipEventSynchronize(c->cells.bins_copied));
    HIP_TRY(hipEventSynchronize(c->null_done));
    while (c->cells.fdr_early_inflight.load()) sched_yield();
    *coef_ptr = hc;
    if (c->cells.fdr_early_copied && c->cells.fdr_early_dst) {
      *fdr_ptr = c->cells.fdr_early_dst;
    } else {
      if (cna_host_expand_u16(hc + n_out, c->cells.h_bins, n_out, c->cells.h_tab, T, 4) != 0)
        CNA_FAIL(CNA_ESTATE, "cna_percell_fdr_pinned: expansion failed");
      *fdr_ptr = hc + n_out;
    }
    c->cells.fdr_early_served = true;
    return 0;
  }
  c->cells.fdr_early_served = false;
  CNA_TRY(cna_percell_fdr(c, thr, runmin_fdr, T, c->cells.coef_early ? nullptr : hc, want_fdr ? hc + n_out : nullptr));
  *coef_ptr = hc;
  if (fdr_ptr) *fdr_ptr = want_fdr ? hc + n_out : nullptr;
  return 0;
}

int cna_percell_fdr(cna_ctx* c, const double* thr, const double* runmin_fdr, int T, double* coef_out,
                    double* fdr_out) {
  CHECK_CTX(c);
  NO_NULL_PENDING(c, "cna_percell_fdr");
  if (!c->ncorrs_valid || !c->x_from_nam) CNA_FAIL(CNA_ESTATE, "cna_percell_fdr needs cna_select + cna_ncorrs");
  const bool want_fdr = fdr_out && thr && runmin_fdr && T > 0;
  double thr0 = 0, inv_step = 0;
  if (want_fdr) guess_from_thr(thr, T, &thr0, &inv_step);
  const int64_t Tn = want_fdr ? T : 1;
  CNA_TRY(dev_reserve(c, &c->scratch, &c->scratch_cap,
                      carve_bytes({8 * Tn, 8 * Tn, 8 * c->n_pad, 8 * c->n_pad, 8 * c->n_pad, 8 * c->n_pad})));
  Carver cv(c->scratch);
  double* td = cv.take<double>(Tn);
  double* rd = cv.take<double>(Tn);
  double* coef = cv.take<double>(c->n_pad);
  double* fdr = cv.take<double>(c->n_pad);
  double* coef_u = cv.take<double>(c->n_pad);
  double* fdr_u = cv.take<double>(c->n_pad);
  if (want_fdr) {
    HIP_TRY(hipMemcpyAsync(td, thr, 8 * T, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(rd, runmin_fdr, 8 * T, hipMemcpyHostToDevice, c->stream));
  }
  CNA_TRY(launch_percell_fdr(c, td, rd, want_fdr ? T : 0, thr0, inv_step, coef + c->row0, want_fdr ? fdr + c->row0 : nullptr));
  const bool sharded = (c->nranks > 1 || comm_active(c)) && !c->local_view;
  int64_t n_out = c->n_global;
  if (c->local_view) {
    // this rank's rows only, in the caller's (local) order: nothing crosses the fabric
    n_out = c->n_local;
    if (c->orig_idx) {
      CNA_TRY(launch_unpermute2(c, coef + c->row0, want_fdr ? fdr + c->row0 : nullptr, c->orig_idx, c->n_local, coef_u,
                                fdr_u));
      coef = coef_u;
      fdr = fdr_u;
    } else {
      coef += c->row0;
      fdr += c->row0;
    }
  } else if (c->orig_idx) {
    // back to the caller's numbering: every rank scatters its rows into a zeroed vector, the sum
    // over ranks (x + 0 keeps NaNs and bit patterns) is the full answer
    if (sharded) {
      HIP_TRY(hipMemsetAsync(coef_u, 0, 8 * c->n_pad, c->stream));
      if (want_fdr) HIP_TRY(hipMemsetAsync(fdr_u, 0, 8 * c->n_pad, c->stream));
    }
    CNA_TRY(launch_unpermute2(c, coef + c->row0, want_fdr ? fdr + c->row0 : nullptr, c->orig_idx, c->n_local, coef_u,
                              fdr_u));
    if (sharded) {
      CNA_TRY(comm_allreduce_f64_sum(c, coef_u, (size_t)c->n_global));
      if (want_fdr) CNA_TRY(comm_allreduce_f64_sum(c, fdr_u, (size_t)c->n_global));
    }
    coef = coef_u;
    fdr = fdr_u;
  } else if (c->nranks > 1) {
    const size_t block = 8 * (size_t)c->rows_per_rank;
    CNA_TRY(comm_allgather_bytes(c, (char*)coef + block * c->rank, coef, block));
    if (want_fdr) CNA_TRY(comm_allgather_bytes(c, (char*)fdr + block * c->rank, fdr, block));
  }
  if (coef_out && n_out > 0) HIP_TRY(hipMemcpyAsync(coef_out, coef, 8 * n_out, hipMemcpyDeviceToHost, c->stream));
  if (want_fdr && n_out > 0) HIP_TRY(hipMemcpyAsync(fdr_out, fdr, 8 * n_out, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
