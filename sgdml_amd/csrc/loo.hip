// Leave-one-out force errors and log det A from the resident Cholesky factor (no counterpart in the reference, which holds
// back a validation split instead).
//
// Conventions: A = -K + lam I = L L^T resident in ctx->K (lower triangle, row-major, pitch K_ld), n = 3N M,
// a = A^-1 y = -alphas, E_j the n x 3N selector of training point j's rows.  With G_j = E_j^T A^-1 E_j (Rasmussen &
// Williams 5.4.2, block form):
//   Z_j = E_j^T L^-T                 rows 3N j .. 3N j + 3N - 1 of L^-T: zero left of column 3N j   (factor_inverse_rows)
//   G_j = Z_j Z_j^T                                                                                 (block_gram.hip) 
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

#define LOO_LDS_MAX_N3 128

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
// Work buffers of one chunk of points (the chunk length: option chol.loo_chunk).
struct LooPlan {
  int gp;
  int64_t bc, per_out;
  bool lds;
  double *alphas, *resid, *diag, *part, *gscr, *out, *rows;
  int* flags;
};

static int loo_plan(gdml_ctx* ctx, const GramSplit& g, int cov_mode, LooPlan* p) {
  const int64_t M = ctx->ts.M, n3 = g.n3, n = g.n;
  p->gp = g.n3 | 1;
  p->lds = n3 <= LOO_LDS_MAX_N3;
  p->per_out = cov_mode == 2 ? n3 * n3 : cov_mode == 1 ? n3 : 0;
  const int64_t gscr = p->lds ? 0 : (n3 + 1) * p->gp;
  const int64_t tiles = (int64_t)g.npairs * g.S * 4096;
  const int64_t small = tiles + gscr + p->per_out;     // doubles per point of a chunk
  const int64_t fixed = 3 * n + (M + 1) / 2 + 16;      // coefficients, residuals, diag L, flags
  double* ws;
  GDML_TRY(gram_workspace(ctx, g, "chol.loo_chunk", M, small, fixed, &p->bc, &p->rows, &ws));
  p->alphas = ws;
  p->resid = p->alphas + n;
  p->diag = p->resid + n;
  p->flags = (int*)(p->diag + n);
  p->part = p->diag + n + (M + 1) / 2;
  p->gscr = p->part + p->bc * tiles;
  p->out = p->gscr + p->bc * gscr;
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
  GramSplit g;
  GDML_TRY(resident_factor_check(ctx, "gdml_loo", false, &g));
  const int64_t M = ctx->ts.M, n3 = g.n3;
  if (n != M * n3) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_loo: n (%lld) is not 3N M = %lld", (long long)n, (long long)(M * n3));
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  LooPlan p;
  GDML_TRY(loo_plan(ctx, g, cov_mode, &p));
  hipStream_t st = ctx->stream;
  HIP_CHECK(ctx, hipMemcpyAsync(p.alphas, alphas, n * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemsetAsync(p.flags, 0, M * sizeof(int), st));
  const size_t lds_bytes = p.lds ? (size_t)(n3 + 1) * p.gp * 8 : 0;
  if (lds_bytes > 64 * 1024)
    HIP_CHECK(ctx, hipFuncSetAttribute((const void*)loo_block_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  phase_begin(ctx);
  for (int64_t j0 = 0; j0 < M; j0 += p.bc) {
    const int64_t bc = M - j0 < p.bc ? M - j0 : p.bc;
    const int64_t first = j0 * n3;
    // Z = E^T L^-T on the trailing sub-problem
    GDML_TRY(factor_inverse_rows(ctx, g, p.rows, j0, bc, "loo_seed", "loo_solve"));
    // G_j = Z_j Z_j^T: point j0 + p is zero left of its first column (j0 + p) 3N
    int slot = ktime_begin(ctx);
    block_gram_launch(ctx, g, p.rows, p.part, bc, false, first, n3);
    ktime_end(ctx, slot, "loo_gram", 2.0 * (double)n3 * (double)n3 * ((double)g.ld * bc - (double)n3 * (j0 * bc + bc * (bc - 1) / 2)));
    LooBlockArgs b;
    b.part = p.part; b.alphas = p.alphas; b.gscr = p.gscr; b.resid = p.resid; b.cov = cov_mode ? p.out : nullptr;
    b.flags = p.flags; b.L = g.L; b.j0 = j0; b.n3 = g.n3; b.gp = p.gp; b.npairs = g.npairs; b.S = g.S; b.cov_mode = cov_mode;
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
  GDML_TRY(factor_logdet(ctx, g, p.diag, logdet_out));
  std::vector<int> flags((size_t)M);
  HIP_CHECK(ctx, hipMemcpyAsync(flags.data(), p.flags, M * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(resid_out, p.resid, n * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipStreamSynchronize(st));
  for (int64_t j = 0; j < M; ++j)
    if (flags[j]) {
      if (info) *info = (int)(j + 1);
      return gdml_fail(ctx, GDML_ERR_NOT_PD, "gdml_loo: (A^-1)_jj of training point %lld is not positive definite", (long long)j);
    }
  return GDML_OK;
}
