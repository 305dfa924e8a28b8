// Appending training points to the resident Cholesky factor without factoring again (no counterpart in the reference, which
// retrains from nothing).
//
// Conventions: A = -K + lam I = L L^T resident in ctx->K (lower triangle, row-major, pitch K_ld = n rounded up
// to 16), n = 3N M.  Appending b points (m = 3N b rows) borders the matrix and its factor:
//   A' = | A  C^T |     L' = | L  0   |     C   = -Kx of the new points against the old ones  (cross_rows_kernel of uncert.hip)
//        | C  D   |          | W  L_S |     W   = C L^-T                                       (tall_trsm of chol_solve.hip, right-looking)
//                                           S   = D - W W^T = L_S L_S^T                        (block_gram.hip + schur_reduce_kernel,
//                                                                                               chol_factor_device)
// The points go through in chunks (option chol.extend_chunk); a chunk's rows are rows of L' once it is through, and the next chunk
// solves against them as well.  The rows are built in place in a NEW buffer of pitch n' rounded up to 16 (the invariant
// K_ld == round16(K_rows) the other users of the factor rely on), into which the lower triangle of L is copied first; the old
// buffer, the old training-set tables and every flag of the context are replaced only after the last chunk has been factored,
// so a failure (no memory, a non-positive pivot) leaves the context as it was.
// The Schur complement of a chunk is factored in a work buffer of its own and stored back: its place in the factor starts at
// column n, which need not be a multiple of 4, and the panel solves of chol_factor_device want 32-byte aligned rows.
#include "common.h"

typedef double d4 __attribute__((ext_vector_type(4)));

// Lower triangle of src (pitch lds, n rows) into dst (pitch ldd >= lds): row r, columns 0 .. r rounded up to the 64-column
// grid of the diagonal blocks (what the old buffer held there: the solves load whole diagonal blocks), as 32-byte groups; the
// rest of the row up to the 512-column panel grid is zeroed, beyond it nothing reads.  Both pitches are multiples of 16.
// A workgroup takes rows r and n - 1 - r together: every workgroup moves about the same number of bytes.
__global__ void __launch_bounds__(256) extend_copy_lower_kernel(const double* __restrict__ src, int64_t lds, double* __restrict__ dst,
                                                                int64_t ldd, int64_t n) {
  const int64_t half = (n + 1) / 2;
  for (int64_t i = blockIdx.x; i < half; i += gridDim.x) {
    for (int k = 0; k < 2; ++k) {
      const int64_t r = k == 0 ? i : n - 1 - i;
      if (k == 1 && r == i) break;
      const d4* __restrict__ s = reinterpret_cast<const d4*>(src + r * lds);
      d4* __restrict__ d = reinterpret_cast<d4*>(dst + r * ldd);
      int64_t c_copy = (r / 64 + 1) * 64, c_zero = (r / 512 + 1) * 512;
      if (c_copy > lds) c_copy = lds;
      if (c_zero > ldd) c_zero = ldd;
      for (int64_t v = threadIdx.x; v < c_copy / 4; v += 256) d[v] = s[v];
      for (int64_t v = c_copy / 4 + threadIdx.x; v < c_zero / 4; v += 256) d[v] = (d4){0.0, 0.0, 0.0, 0.0};
    }
  }
}

// S = (D + lam I) - W W^T on the lower triangle of a chunk of mc rows: W W^T over the columns [0, n16) comes as the partial
// tiles of block_gram_kernel (one item; summed here in the order s = 0 .. S - 1), the columns [n16, ncur) that do not fill a
// group of 16 are added behind them in index order, one fused multiply-add each.  One workgroup per lower 64 x 64 block pair;
// every element has one owner.  W: the chunk's rows in the factor buffer (pitch ld), D their columns from ncur on.
struct SchurArgs {
  const double* part;  // [pair][s][64 x 64]
  const double* W;
  double* S;           // mc x mc, pitch lds
  int64_t ld, lds, n16, ncur;
  int mc, nsplit;
  double lam;
};

__global__ void __launch_bounds__(256) schur_reduce_kernel(SchurArgs a) {
  const int pr = blockIdx.x;
  int I = (int)((sqrt(8.0 * (double)pr + 1.0) - 1.0) * 0.5);
  while (I * (I + 1) / 2 > pr) --I;
  while ((I + 1) * (I + 2) / 2 <= pr) ++I;
  const int J = pr - I * (I + 1) / 2;
  const double* __restrict__ p = a.part + (int64_t)pr * a.nsplit * 4096;
  for (int e = threadIdx.x; e < 4096; e += 256) {
    const int r = I * 64 + (e >> 6), c = J * 64 + (e & 63);
    if (r >= a.mc || c > r) continue;
    double acc = 0.0;
    for (int s = 0; s < a.nsplit; ++s) acc += p[(int64_t)s * 4096 + e];
    const double* __restrict__ wr = a.W + (int64_t)r * a.ld;
    const double* __restrict__ wc = a.W + (int64_t)c * a.ld;
    for (int64_t k = a.n16; k < a.ncur; ++k) acc = __builtin_fma(wr[k], wc[k], acc);
    const double d = wr[a.ncur + c] + (r == c ? a.lam : 0.0);
    a.S[(int64_t)r * a.lds + c] = d - acc;
  }
}

// the factored chunk back into its place: row r of the chunk, columns ncur .. ncur + r of the factor
__global__ void __launch_bounds__(256) extend_store_lower_kernel(const double* __restrict__ S, int64_t lds, double* __restrict__ dst,
                                                                 int64_t ld) {
  const int64_t r = blockIdx.x;
  for (int64_t c = threadIdx.x; c <= r; c += 256) dst[r * ld + c] = S[r * lds + c];
}

// (gram_split's S = min(32, ceil(n / 1024)) does not fall as n grows: the plan for n1 columns covers every chunk's n_cur / 16 * 16)
static int64_t extend_ws_doubles(int64_t n1, int64_t bc, int64_t n3) {
  const int64_t mc = bc * n3;
  const GramSplit g = gram_split(n1, (int)mc);
  return bc * n3 * n3 + (int64_t)g.npairs * g.S * 4096 + mc * round16(mc);
}

extern "C" int gdml_factor_extend(gdml_ctx* ctx, const double* R_desc_new, const double* R_d_desc_new, int64_t b, int* info) {
  if (!ctx) return GDML_ERR_INVALID;
  if (info) *info = 0;
  if (b < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_factor_extend: b < 0");
  if (b > 0 && (!R_desc_new || !R_d_desc_new))
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_factor_extend: R_desc_new or R_d_desc_new is NULL");
  if (comm_active(ctx) && ctx->world > 1)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "gdml_factor_extend: the factor of a multi-rank context is distributed");
  GramSplit g0;
  GDML_TRY(resident_factor_check(ctx, "gdml_factor_extend", true, &g0));
  TrainSet& ts = ctx->ts;
  const int64_t M0 = ts.M, n3 = g0.n3, D = ts.D, n0 = g0.n, ld0 = g0.ld;
  if (b == 0) return GDML_OK;
  const int64_t n1 = n0 + b * n3, ld1 = round16(n1);
  if (n1 > INT32_MAX) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_factor_extend: %lld rows exceed the factorisation's range", (long long)n1);
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // the Gram work buffers of gdml_predict_cov / gdml_loo were sized for n: they are carved anew at the next call
  GDML_TRY(ctx_slot_release(ctx, SLOT_GRAM_WS));
  GDML_TRY(ctx_slot_release(ctx, SLOT_GRAM_ROWS));

  // everything new lives in buffers of its own until the commit
  double *Kn = nullptr, *x1 = nullptr, *g1 = nullptr, *ws = nullptr;
  auto drop = [&](int rc) {
    (void)hipStreamSynchronize(st);
    if (ws) (void)ctx_free(ctx, ws);
    if (g1) (void)ctx_free(ctx, g1);
    if (x1) (void)ctx_free(ctx, x1);
    if (Kn) (void)ctx_free(ctx, Kn);
    return rc;
  };

  // the matrix with up to 127 pad rows behind it: the solve runs on whole 128-row tiles (pad_rows128)
  const int64_t Kn_bytes = (n1 + 127) * ld1 * 8;
  DROP_TRY(ctx_alloc(ctx, (void**)&Kn, Kn_bytes));
  DROP_TRY(ctx_alloc(ctx, (void**)&x1, (M0 + b) * D * 8));
  DROP_TRY(ctx_alloc(ctx, (void**)&g1, (M0 + b) * D * 24));
  // chunk length: the option's cap, the point count, then halved while the work buffers exceed 90 % of free memory
  int64_t bc = ctx_opt_i(ctx, "chol.extend_chunk", 64);
  if (bc < 1) bc = 1;
  if (bc > b) bc = b;
  size_t mem_free = 0, mem_total = 0;
  DROP_HIP(hipMemGetInfo(&mem_free, &mem_total));
  while (bc > 1 && extend_ws_doubles(n1, bc, n3) * 8 > (int64_t)mem_free / 10 * 9) bc = (bc + 1) / 2;
  DROP_TRY(ctx_alloc(ctx, (void**)&ws, extend_ws_doubles(n1, bc, n3) * 8));
  const int64_t mc_max = bc * n3, lds = round16(mc_max);
  double* const Sb = ws;                      // Schur complement of a chunk, pitch lds (32-byte aligned rows: first)
  double* const kqq = Sb + mc_max * lds;      // the cross-kernel's k_qq output (the same blocks arrive as columns of D)
  double* const part = kqq + bc * n3 * n3;

  phase_begin(ctx);
  DROP_HIP(hipMemcpyAsync(x1, ts.x, M0 * D * 8, hipMemcpyDeviceToDevice, st));
  DROP_HIP(hipMemcpyAsync(g1, ts.g, M0 * D * 24, hipMemcpyDeviceToDevice, st));
  DROP_HIP(hipMemcpyAsync(x1 + M0 * D, R_desc_new, b * D * 8, hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemcpyAsync(g1 + M0 * D * 3, R_d_desc_new, b * D * 24, hipMemcpyHostToDevice, st));
  int slot = ktime_begin(ctx);
  {
    int64_t grid = (n0 + 1) / 2;
    if (grid > 64 * (int64_t)ctx->num_cus) grid = 64 * (int64_t)ctx->num_cus;
    hipLaunchKernelGGL(extend_copy_lower_kernel, dim3((unsigned)grid), dim3(256), 0, st, ctx->K, ld0, Kn, ld1, n0);
    ctx->launch_counter++;
  }
  ktime_end(ctx, slot, "extend_copy", (double)n0 * (double)(n0 + 1) * 8.0);  // bytes read + written

  int64_t n_cur = n0, M_cur = M0;
  for (int64_t p0 = 0; p0 < b; p0 += bc) {
    const int64_t c = b - p0 < bc ? b - p0 : bc, mc = c * n3, rows_pad = pad_rows128(mc);
    double* const rows = Kn + n_cur * ld1;
    if (rows_pad > mc) DROP_HIP(hipMemsetAsync(rows + mc * ld1, 0, (rows_pad - mc) * ld1 * 8, st));
    // [C | D] = -Kx of the chunk's points against the old points, the earlier chunks and the chunk itself
    DROP_TRY(cross_rows_launch(ctx, x1, g1, M_cur + c, x1 + M_cur * D, g1 + M_cur * D * 3, (int)c, rows, ld1, kqq, -1.0, ctx->K_sig,
                              "extend_cross"));
    // W = C L'^-T over the n_cur finished rows, right-looking (few rows, long factor: uncert.hip)
    slot = ktime_begin(ctx);
    DROP_TRY(tall_trsm(ctx, Kn, rows, rows_pad, n_cur, ld1, 0));
    ktime_end(ctx, slot, "extend_solve", (double)n_cur * (double)n_cur * (double)mc);
    // S = D + lam I - W W^T
    slot = ktime_begin(ctx);
    SchurArgs a;
    a.part = part; a.W = rows; a.S = Sb; a.ld = ld1; a.lds = lds; a.n16 = n_cur / 16 * 16; a.ncur = n_cur;
    a.mc = (int)mc; a.nsplit = 0; a.lam = ctx->K_lam;
    DROP_HIP(hipMemsetAsync(Sb, 0, mc * lds * 8, st));  // (the factorisation loads whole diagonal blocks: no stale upper triangle)
    const int nblk = (int)((mc + 63) / 64), npairs = nblk * (nblk + 1) / 2;
    if (a.n16 > 0) {
      const GramSplit g = gram_split(a.n16, (int)mc);
      a.nsplit = g.S;
      block_gram_launch(ctx, g, rows, part, 1, false, 0, 0, ld1);
    }
    hipLaunchKernelGGL(schur_reduce_kernel, dim3((unsigned)npairs), dim3(256), 0, st, a);
    ctx->launch_counter++;
    ktime_end(ctx, slot, "extend_schur", (double)mc * (double)mc * (double)n_cur);
    DROP_HIP(hipGetLastError());
    slot = ktime_begin(ctx);
    int inf = 0;
    DROP_TRY(chol_factor_device(ctx, Sb, mc, lds, &inf));
    if (inf != 0) {
      if (info) *info = (int)(n_cur + inf);
      return drop(gdml_fail(ctx, GDML_ERR_NOT_PD, "gdml_factor_extend: %lld-th leading minor of the extended matrix is not positive definite",
                            (long long)(n_cur + inf)));
    }
    hipLaunchKernelGGL(extend_store_lower_kernel, dim3((unsigned)mc), dim3(256), 0, st, Sb, lds, rows + n_cur, ld1);
    ctx->launch_counter++;
    ktime_end(ctx, slot, "extend_chol", (double)mc * (double)mc * (double)mc / 3.0);
    DROP_HIP(hipGetLastError());
    n_cur += mc;
    M_cur += c;
  }
  DROP_TRY(phase_end(ctx, "extend"));
  DROP_HIP(hipStreamSynchronize(st));

  // ---- commit
  (void)ctx_free(ctx, ws);
  factor_commit(ctx, Kn, Kn_bytes, n1, ld1, x1, g1, M0 + b);
  return GDML_OK;
}
