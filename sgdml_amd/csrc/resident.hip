// What the entries on the resident Cholesky factor share on the host side: the check of the state they may be
// called in, rows of L^-T for a chunk of training points, log det A, and the commit of a replaced factor.
// A = -K + lam I = L L^T resident in ctx->K (lower triangle, row-major, pitch K_ld = n rounded up to 16), n = 3N M.
#include "common.h"

int resident_factor_check(gdml_ctx* ctx, const char* who, bool need_prepared, GramSplit* g_out) {
  if (!ctx->ts.x) return gdml_fail(ctx, GDML_ERR_STATE, "%s: call gdml_train_upload first", who);
  if (ctx->K && ctx->K_factored && ctx->K_use_E)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "%s: the resident factor carries energy-constraint rows", who);
  if (need_prepared && !(ctx->uncert_ready && ctx->K && ctx->K_factored))
    return gdml_fail(ctx, GDML_ERR_STATE, "%s: no factor prepared (gdml_uncert_prepare; an assembly since then overwrote it)", who);
  if (!ctx->K || !ctx->K_factored)
    return gdml_fail(ctx, GDML_ERR_STATE, "%s: no Cholesky factor resident (gdml_uncert_prepare or gdml_chol_factor)", who);
  const GramSplit g = gram_split(ctx->ts.M * 3 * ctx->ts.N, 3 * ctx->ts.N);
  if (ctx->K_rows != g.n || ctx->K_cols != g.n || ctx->K_ld != g.ld || ctx->K_sharded)
    return gdml_fail(ctx, GDML_ERR_STATE, "%s: the resident factor does not belong to the resident training set", who);
  *g_out = g;
  return GDML_OK;
}

// unit entries of the right-hand side E_j^T: row r of the chunk is coordinate r of the chunk's points
__global__ void __launch_bounds__(256) factor_seed_kernel(double* __restrict__ rows, int64_t ld, int64_t col0, int64_t nrows) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < nrows) rows[r * ld + col0 + r] = 1.0;
}

__global__ void __launch_bounds__(256) factor_diag_kernel(const double* __restrict__ Lf, int64_t ld, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = Lf[i * ld + i];
}

int factor_inverse_rows(gdml_ctx* ctx, const GramSplit& g, double* rows, int64_t j0, int64_t bc, const char* t_seed,
                        const char* t_solve, double* keep) {
  hipStream_t st = ctx->stream;
  const int64_t n = g.n, ld = g.ld, nrows = bc * g.n3, rows_pad = pad_rows128(nrows);
  const int64_t first = j0 * g.n3, c0 = first / 512 * 512;
  // everything left of c0 is zero in every row of the chunk, and because c0 lies on the panel grid the panels, tiles and edge
  // tiles that meet the non-zero part are those of a solve from column 0
  int slot = ktime_begin(ctx);
  HIP_CHECK(ctx, hipMemset2DAsync(rows + c0, ld * 8, 0, (ld - c0) * 8, rows_pad, st));
  hipLaunchKernelGGL(factor_seed_kernel, dim3((unsigned)ceil_div(nrows, 256)), dim3(256), 0, st, rows, ld, first, nrows);
  ctx->launch_counter++;
  ktime_end(ctx, slot, t_seed, (double)rows_pad * (double)(ld - c0) * 8.0);
  // right-looking: few rows, long factor (uncert.hip)
  slot = ktime_begin(ctx);
  GDML_TRY(tall_trsm(ctx, ctx->K + c0 * ld + c0, rows + c0, rows_pad, n - c0, ld, 0));
  if (keep)
    HIP_CHECK(ctx, hipMemcpy2DAsync(keep + first * ld + c0, ld * 8, rows + c0, ld * 8, (ld - c0) * 8, nrows, hipMemcpyDeviceToDevice, st));
  ktime_end(ctx, slot, t_solve, (double)(n - c0) * (double)(n - c0) * (double)nrows);
  return GDML_OK;
}

int factor_logdet(gdml_ctx* ctx, const GramSplit& g, double* d_diag, double* logdet_out) {
  std::vector<double> diag((size_t)g.n);
  hipLaunchKernelGGL(factor_diag_kernel, dim3((unsigned)ceil_div(g.n, 256)), dim3(256), 0, ctx->stream, ctx->K, g.ld, g.n, d_diag);
  HIP_CHECK(ctx, hipMemcpyAsync(diag.data(), d_diag, g.n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  double ld_sum = 0.0;
  for (int64_t i = 0; i < g.n; ++i) ld_sum += log(diag[i]);
  *logdet_out = 2.0 * ld_sum;
  return GDML_OK;
}

void factor_commit(gdml_ctx* ctx, double* Kn, int64_t Kn_bytes, int64_t n1, int64_t ld1, double* x1, double* g1, int64_t M1) {
  TrainSet& ts = ctx->ts;
  (void)ctx_free(ctx, ctx->K);
  ctx->K = Kn;
  ctx->K_bytes = Kn_bytes;
  ctx->K_rows = ctx->K_cols = ctx->K_rows_global = n1;
  ctx->K_ld = ld1;
  ctx->K_extra = 0;
  ctx->K_rhs_row = false;
  ctx->K_factored = true;
  ctx->precon = nullptr;
  (void)ctx_free(ctx, ts.x);
  (void)ctx_free(ctx, ts.g);
  (void)ctx_free(ctx, ts.XF);
  (void)ctx_free(ctx, ts.GD);
  (void)ctx_free(ctx, ts.TS);
  (void)ctx_free(ctx, ts.p2);
  (void)ctx_free(ctx, ts.p2_TP);
  ts.XF = ts.GD = ts.TS = ts.p2_TP = nullptr;
  ts.p2 = nullptr;
  ts.x = x1;
  ts.g = g1;
  ts.M = M1;
}
