// Leave-one-out force errors and log det A from the resident Cholesky factor (no counterpart in the reference, which holds
// back a validation split instead).
//
// Conventions: A = -K + lam I = L L^T resident in ctx->K (lower triangle, row-major, pitch K_ld), n = 3N M,
// a = A^-1 y = -alphas, E_j the n x 3N selector of training point j's rows.  With G_j = E_j^T A^-1 E_j (Rasmussen &
// Williams 5.4.2, block form):
//   Z_j = E_j^T L^-T                 rows 3N j .. 3N j + 3N - 1 of L^-T: zero left of column 3N j   (tall_trsm of cg.hip)
//   G_j = Z_j Z_j^T                                                                                 (loo_gram_kernel)
//   r_j = G_j^-1 a_j,  C_j = G_j^-1                                                                 (loo_block_kernel)
// r_j is the force error at x_j of the model trained without point j, C_j the predictive covariance of that left-out
// label (noise lam included), both in the units of the normalised labels.
//
// The points go through in chunks of consecutive points.  A chunk's rows are solved on the trailing sub-problem that
// starts at c0 = its first column rounded down to the 512-column panel grid of tall_trsm: everything left of c0 is zero in
// every row of the chunk, and because c0 lies on the panel grid the panels, tiles and edge tiles that meet the non-zero
// part are those of a solve from column 0.  The k splits of the Gram step lie on a grid that depends on n alone, a point
// skips the splits wholly left of its first column and starts the first one it keeps at its first column rounded down to
// 16 (left of it the row holds zeros -- or, left of c0, nothing at all).  None of this depends on the chunk length, so
// neither do the results.
#include "common.h"

typedef double d4 __attribute__((ext_vector_type(4)));

#define LOO_SLOT_WS 13    // shared with uncert.hip (UC_SLOT_WS): coefficients, partial Gram tiles, G_j scratch, staged output
#define LOO_SLOT_ROWS 14  // shared with uncert.hip (UC_SLOT_ROWS): the (3N chunk) x K_ld row buffer
#define LOO_LDS_MAX_N3 128

// unit entries of Z's right-hand side E_j^T: row r of the chunk is coordinate r of the chunk's points
__global__ void __launch_bounds__(256) loo_seed_kernel(double* __restrict__ rows, int64_t ld, int64_t col0, int64_t nrows) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < nrows) rows[r * ld + col0 + r] = 1.0;
}

__global__ void __launch_bounds__(256) loo_diag_kernel(const double* __restrict__ Lf, int64_t ld, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = Lf[i * ld + i];
}

// ---- block Gram ----------------------------------------------------------------------------------------------------------
// G_j = Z_j Z_j^T with the tile and k-bijection scheme of cov_gram_kernel (uncert.hip): 64 x 64 blocks of 4 x 4 tiles of
// v_mfma_f64_16x16x4_f64, one wavefront per (point, lower block pair (I, J), k split s), both operands straight from global
// memory as 32-byte runs, rows past 3N re-read row 3N - 1 (their results are stored and never read).
struct LooGramArgs {
  const double* Z;
  double* part;  // [p][pair][s][64 x 64]
  int64_t ld, L, units, j0;
  int n3, npairs, S;
};

__global__ void __launch_bounds__(256) loo_gram_kernel(LooGramArgs g) {
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= g.units) return;
  const int s = (int)(unit % g.S);
  const int64_t up = unit / g.S;
  const int pr = (int)(up % g.npairs);
  const int64_t p = up / g.npairs;
  const int64_t first = (g.j0 + p) * g.n3;  // the point's first column
  int64_t k_beg = (int64_t)s * g.L;
  const int64_t k_end = k_beg + g.L < g.ld ? k_beg + g.L : g.ld;
  if (k_end <= first) return;  // wholly left of the point: loo_block_kernel does not read this tile
  if (k_beg < first) k_beg = first / 16 * 16;
  int I = (int)((sqrt(8.0 * (double)pr + 1.0) - 1.0) * 0.5);
  while (I * (I + 1) / 2 > pr) --I;
  while ((I + 1) * (I + 2) / 2 <= pr) ++I;
  const int J = pr - I * (I + 1) / 2;
  const double* pa[4];
  const double* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int ra = I * 64 + 16 * i + li, rb = J * 64 + 16 * i + li;
    ra = ra < g.n3 ? ra : g.n3 - 1;
    rb = rb < g.n3 ? rb : g.n3 - 1;
    pa[i] = g.Z + (p * g.n3 + ra) * g.ld + 4 * lk;
    pb[i] = g.Z + (p * g.n3 + rb) * g.ld + 4 * lk;
  }
  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int64_t k0 = k_beg; k0 < k_end; k0 += 16) {
    d4 av[4], bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const d4*>(pa[i] + k0);
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[i] = *reinterpret_cast<const d4*>(pb[i] + k0);
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i][st], bv[j][st], acc[i][j], 0, 0, 0);
  }
  // f64 MFMA C/D layout: col = lane & 15, row = (lane >> 4) + 4 r
  double* o = g.part + ((p * g.npairs + pr) * g.S + s) * 4096;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(16 * i + lk + 4 * r) * 64 + 16 * j + li] = acc[i][j][r];
}

// ---- block solve ---------------------------------------------------------------------------------------------------------
// One workgroup per training point.  G_j (lower triangle; pitch gp, odd: a column walk meets every LDS bank) is summed from
// its partial tiles in the order s = s0 .. S - 1, factored G_j = R R^T in place (right-looking, every element updated in
// the order k = 0, 1, ...), r_j comes from the two substitutions, and on request W = R^-1 is built into the strict upper
// triangle (row c holds column c of W; the diagonal is then overwritten by 1 / R_ii) and C_j = W^T W is summed from it:
//   C_j[a][b] = sum_{k >= max(a, b)} W[k][a] W[k][b],
// by the same function for the full form and for the diagonal.  Every sum is a chain of fused multiply-adds in a fixed order.
// LDS form: (3N + 1) x gp doubles, 130 KB at 3N = 128 -- one workgroup per CU there; GLOBAL form (3N > 128): the same walk
// on a scratch slot per point.
struct LooBlockArgs {
  const double* part;
  const double* alphas;  // (n) device copy of the library's coefficients: a = -alphas
  double* gscr;          // GLOBAL form: [p][(3N + 1) x gp]
  double* resid;         // (M,3N)
  double* cov;           // chunk staging: [p][3N] or [p][3N x 3N], or null
  int* flags;            // (M): set to 1 when G_j has a non-positive pivot
  int64_t L, j0;
  int n3, gp, npairs, S, cov_mode;
};

__device__ __forceinline__ double loo_cov_elem(const double* G, int gp, int n3, int a, int b) {
  const double* wa = G + (int64_t)a * gp;
  const double* wb = G + (int64_t)b * gp;
  double acc = 0.0;
  for (int k = a > b ? a : b; k < n3; ++k) acc = __builtin_fma(wa[k], wb[k], acc);
  return acc;
}

template <bool LDS>
__global__ void __launch_bounds__(256) loo_block_kernel(LooBlockArgs b) {
  extern __shared__ double loo_lds[];
  const int tid = threadIdx.x, n3 = b.n3, gp = b.gp;
  const int64_t p = blockIdx.x, j = b.j0 + p;
  double* const G = LDS ? loo_lds : b.gscr + p * (int64_t)(n3 + 1) * gp;
  double* const v = G + (int64_t)n3 * gp;
  const int s0 = (int)(j * n3 / b.L);
  for (int e = tid; e < n3 * n3; e += 256) {
    const int r = e / n3, c = e - r * n3;
    if (c > r) continue;
    const int I = r >> 6, J = c >> 6;
    const double* q = b.part + ((p * b.npairs + I * (I + 1) / 2 + J) * b.S) * 4096 + (r & 63) * 64 + (c & 63);
    double acc = 0.0;
    for (int s = s0; s < b.S; ++s) acc += q[(int64_t)s * 4096];
    G[(int64_t)r * gp + c] = acc;
  }
  for (int i = tid; i < n3; i += 256) v[i] = -b.alphas[j * n3 + i];
  __syncthreads();
  // G = R R^T
  for (int k = 0; k < n3; ++k) {
    const double d = G[(int64_t)k * gp + k];
    if (!(d > 0.0)) {  // (also NaN) the same value in every thread: the workgroup leaves together
      if (tid == 0) b.flags[j] = 1;
      return;
    }
    const double rk = sqrt(d);
    for (int i = k + 1 + tid; i < n3; i += 256) G[(int64_t)i * gp + k] /= rk;
    __syncthreads();
    if (tid == 0) G[(int64_t)k * gp + k] = rk;  // not read again before the substitutions
    const int m = n3 - k - 1;
    for (int e = tid; e < m * m; e += 256) {
      const int ii = e / m, cc = e - ii * m;
      if (cc > ii) continue;
      const int i = k + 1 + ii, c = k + 1 + cc;
      G[(int64_t)i * gp + c] = __builtin_fma(-G[(int64_t)i * gp + k], G[(int64_t)c * gp + k], G[(int64_t)i * gp + c]);
    }
    __syncthreads();
  }
  // R z = a_j, R^T r_j = z.  Every thread reads the pivot entry of v before the step's barrier; thread 0 replaces it after.
  for (int k = 0; k < n3; ++k) {
    const double zk = v[k] / G[(int64_t)k * gp + k];
    for (int i = k + 1 + tid; i < n3; i += 256) v[i] = __builtin_fma(-G[(int64_t)i * gp + k], zk, v[i]);
    __syncthreads();
    if (tid == 0) v[k] = zk;
  }
  __syncthreads();
  for (int k = n3 - 1; k >= 0; --k) {
    const double xk = v[k] / G[(int64_t)k * gp + k];
    for (int i = tid; i < k; i += 256) v[i] = __builtin_fma(-G[(int64_t)k * gp + i], xk, v[i]);
    __syncthreads();
    if (tid == 0) v[k] = xk;
  }
  __syncthreads();
  for (int i = tid; i < n3; i += 256) b.resid[j * n3 + i] = v[i];
  if (b.cov_mode == 0) return;
  // column c of W = R^-1 by forward substitution, one thread per column (the lower triangle is only read)
  for (int c = tid; c < n3; c += 256) {
    double* wc = G + (int64_t)c * gp;
    const double wcc = 1.0 / wc[c];
    for (int i = c + 1; i < n3; ++i) {
      const double* ri = G + (int64_t)i * gp;
      double s = ri[c] * wcc;
      for (int k = c + 1; k < i; ++k) s = __builtin_fma(ri[k], wc[k], s);
      wc[i] = -s / ri[i];
    }
  }
  __syncthreads();
  for (int i = tid; i < n3; i += 256) G[(int64_t)i * gp + i] = 1.0 / G[(int64_t)i * gp + i];
  __syncthreads();
  if (b.cov_mode == 1) {
    double* o = b.cov + p * n3;
    for (int a = tid; a < n3; a += 256) o[a] = loo_cov_elem(G, gp, n3, a, a);
  } else {
    double* o = b.cov + p * (int64_t)n3 * n3;
    for (int e = tid; e < n3 * n3; e += 256) {
      const int a = e / n3, c = e - a * n3;
      o[e] = loo_cov_elem(G, gp, n3, a, c);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// Work buffers of one chunk of points.  The Gram split (S, L) depends on n (and the pitch) alone, as in uncert_plan.
struct LooPlan {
  int n3, nblk, npairs, S, gp;
  int64_t n, ld, L, bc, per_out;
  bool lds;
  double *alphas, *resid, *diag, *part, *gscr, *out, *rows;
  int* flags;
};

static inline int64_t loo_pad_rows(int64_t rows) { return (rows + 127) / 128 * 128; }  // whole 128-row tiles: see uc_pad_rows

static int loo_plan(gdml_ctx* ctx, int cov_mode, LooPlan* p) {
  const TrainSet& ts = ctx->ts;
  const int64_t M = ts.M;
  p->n3 = 3 * ts.N;
  p->n = M * p->n3;
  p->ld = ctx->K_ld;
  p->nblk = (p->n3 + 63) / 64;
  p->npairs = p->nblk * (p->nblk + 1) / 2;
  p->S = (int)((p->n + 1023) / 1024);
  if (p->S > 32) p->S = 32;
  if (p->S < 1) p->S = 1;
  p->L = ((p->ld + p->S - 1) / p->S + 15) / 16 * 16;
  p->S = (int)((p->ld + p->L - 1) / p->L);  // no empty split
  p->gp = p->n3 | 1;
  p->lds = p->n3 <= LOO_LDS_MAX_N3;
  const int64_t n3 = p->n3;
  p->per_out = cov_mode == 2 ? n3 * n3 : cov_mode == 1 ? n3 : 0;
  const int64_t gscr = p->lds ? 0 : (n3 + 1) * p->gp;
  const int64_t small = (int64_t)p->npairs * p->S * 4096 + gscr + p->per_out;  // doubles per point of a chunk
  const int64_t fixed = 3 * p->n + (M + 1) / 2 + 16;                           // coefficients, residuals, diag L, flags
  int64_t bc = ctx_opt_i(ctx, "chol.loo_chunk", 64);
  if (bc < 1) bc = 1;
  if (bc > M) bc = M;
  size_t f = 0, t = 0;
  HIP_CHECK(ctx, hipMemGetInfo(&f, &t));
  const int64_t have = (int64_t)f + ctx->slot_bytes[LOO_SLOT_WS] + ctx->slot_bytes[LOO_SLOT_ROWS];
  while (bc > 1 && bc * (n3 * p->ld + small) * 8 + (127 * p->ld + fixed) * 8 > have / 10 * 9) bc = (bc + 1) / 2;
  p->bc = bc;
  double* ws;
  GDML_TRY(ctx_slot(ctx, LOO_SLOT_ROWS, loo_pad_rows(bc * n3) * p->ld * 8, &p->rows));
  GDML_TRY(ctx_slot(ctx, LOO_SLOT_WS, (fixed + bc * small) * 8, &ws));
  p->alphas = ws;
  p->resid = p->alphas + p->n;
  p->diag = p->resid + p->n;
  p->flags = (int*)(p->diag + p->n);
  p->part = p->diag + p->n + (M + 1) / 2;
  p->gscr = p->part + bc * (int64_t)p->npairs * p->S * 4096;
  p->out = p->gscr + bc * gscr;
  return GDML_OK;
}

extern "C" int gdml_loo(gdml_ctx* ctx, const double* alphas, int64_t n, int cov_mode, double* resid_out, double* cov_out,
                        double* logdet_out, int* info) {
  if (!ctx) return GDML_ERR_INVALID;
  if (info) *info = 0;
  if (!alphas || !resid_out || !logdet_out) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_loo: alphas, resid_out or logdet_out is NULL");
  if (cov_mode < 0 || cov_mode > 2) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_loo: cov_mode %d (0, 1 or 2)", cov_mode);
  if (cov_mode != 0 && !cov_out) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_loo: cov_out is NULL");
  if (ctx->world > 1)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "gdml_loo: the factor of a multi-rank context is distributed");
  if (!ctx->ts.x) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_loo: call gdml_train_upload first");
  if (ctx->K && ctx->K_factored && ctx->K_use_E)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "gdml_loo: the resident factor carries energy-constraint rows");
  if (!ctx->K || !ctx->K_factored)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_loo: no Cholesky factor resident (gdml_uncert_prepare or gdml_chol_factor)");
  const int64_t M = ctx->ts.M, n3 = 3 * ctx->ts.N;
  if (ctx->K_rows != M * n3 || ctx->K_cols != ctx->K_rows || ctx->K_sharded)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_loo: the resident factor does not belong to the resident training set");
  if (n != M * n3) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_loo: n (%lld) is not 3N M = %lld", (long long)n, (long long)(M * n3));
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LooPlan p;
  GDML_TRY(loo_plan(ctx, cov_mode, &p));
  hipStream_t st = ctx->stream;
  HIP_CHECK(ctx, hipMemcpyAsync(p.alphas, alphas, n * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemsetAsync(p.flags, 0, M * sizeof(int), st));
  const size_t lds_bytes = p.lds ? (size_t)(n3 + 1) * p.gp * 8 : 0;
  if (lds_bytes > 64 * 1024)
    HIP_CHECK(ctx, hipFuncSetAttribute((const void*)loo_block_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  phase_begin(ctx);
  for (int64_t j0 = 0; j0 < M; j0 += p.bc) {
    const int64_t bc = M - j0 < p.bc ? M - j0 : p.bc;
    const int64_t rows = bc * n3, rows_pad = loo_pad_rows(rows);
    const int64_t first = j0 * n3, c0 = first / 512 * 512;
    // seed: E_j^T from column c0 on (columns left of c0 are not part of the sub-problem and are never read)
    int slot = ktime_begin(ctx);
    HIP_CHECK(ctx, hipMemset2DAsync(p.rows + c0, p.ld * 8, 0, (p.ld - c0) * 8, rows_pad, st));
    hipLaunchKernelGGL(loo_seed_kernel, dim3((unsigned)ceil_div(rows, 256)), dim3(256), 0, st, p.rows, p.ld, first, rows);
    ctx->launch_counter++;
    ktime_end(ctx, slot, "loo_seed", (double)rows_pad * (double)(p.ld - c0) * 8.0);
    // Z = E^T L^-T on the trailing sub-problem, right-looking (few rows, long factor: uncert.hip)
    slot = ktime_begin(ctx);
    GDML_TRY(tall_trsm(ctx, ctx->K + c0 * p.ld + c0, p.rows + c0, rows_pad, n - c0, p.ld, 0));
    ktime_end(ctx, slot, "loo_solve", (double)(n - c0) * (double)(n - c0) * (double)rows);
    LooGramArgs g;
    g.Z = p.rows; g.part = p.part; g.ld = p.ld; g.L = p.L; g.j0 = j0; g.n3 = p.n3; g.npairs = p.npairs; g.S = p.S;
    g.units = bc * g.npairs * g.S;
    slot = ktime_begin(ctx);
    hipLaunchKernelGGL(loo_gram_kernel, dim3((unsigned)ceil_div(g.units, 4)), dim3(256), 0, st, g);
    ctx->launch_counter++;
    ktime_end(ctx, slot, "loo_gram", 2.0 * (double)n3 * (double)n3 * ((double)p.ld * bc - (double)n3 * (j0 * bc + bc * (bc - 1) / 2)));
    LooBlockArgs b;
    b.part = p.part; b.alphas = p.alphas; b.gscr = p.gscr; b.resid = p.resid; b.cov = cov_mode ? p.out : nullptr;
    b.flags = p.flags; b.L = p.L; b.j0 = j0; b.n3 = p.n3; b.gp = p.gp; b.npairs = p.npairs; b.S = p.S; b.cov_mode = cov_mode;
    slot = ktime_begin(ctx);
    if (p.lds)
      hipLaunchKernelGGL(loo_block_kernel<true>, dim3((unsigned)bc), dim3(256), lds_bytes, st, b);
    else
      hipLaunchKernelGGL(loo_block_kernel<false>, dim3((unsigned)bc), dim3(256), 0, st, b);
    ctx->launch_counter++;
    ktime_end(ctx, slot, "loo_block", (double)bc * (double)n3 * n3 * n3 * (cov_mode ? 1.0 : 1.0 / 3.0));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gdml_fail(ctx, GDML_ERR_HIP, "gdml_loo launch: %s", hipGetErrorString(e));
    if (cov_mode) {  // the staging buffer is rewritten by the next chunk
      HIP_CHECK(ctx, hipMemcpyAsync(cov_out + j0 * p.per_out, p.out, bc * p.per_out * 8, hipMemcpyDeviceToHost, st));
      HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
  }
  GDML_TRY(phase_end(ctx, "loo"));
  // log det A = 2 sum log L_ii: a strided copy and a host sum in index order
  std::vector<double> diag((size_t)n);
  std::vector<int> flags((size_t)M);
  hipLaunchKernelGGL(loo_diag_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, ctx->K, p.ld, n, p.diag);
  HIP_CHECK(ctx, hipMemcpyAsync(diag.data(), p.diag, n * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(flags.data(), p.flags, M * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(resid_out, p.resid, n * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipStreamSynchronize(st));
  double ld_sum = 0.0;
  for (int64_t i = 0; i < n; ++i) ld_sum += log(diag[i]);
  *logdet_out = 2.0 * ld_sum;
  for (int64_t j = 0; j < M; ++j)
    if (flags[j]) {
      if (info) *info = (int)(j + 1);
      return gdml_fail(ctx, GDML_ERR_NOT_PD, "gdml_loo: (A^-1)_jj of training point %lld is not positive definite", (long long)j);
    }
  return GDML_OK;
}
