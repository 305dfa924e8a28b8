// The Nystroem factor of the preconditioner on the device.
//
// Replaces sgdml/solvers/iterative.py: _nystroem_cholesky_factor (:208-351), _cho_factor_stable (:414-471) and the leverage
// scores (:107-109).  The Gram matrices come from gram_tn.hip, the triangular solves from chol_solve.hip (tall_trsm), the
// application of what is built here lives in precon_apply.hip, the branch arithmetic in precon_plan.h.
//
// Device layout: the (n+m) x m matrix of gdml_assemble_K(GDML_COLS_INDEX, alloc_extra_rows = m):
// rows [0,n) = K_nm (un-negated), rows [n,n+m) = work area for the m x m blocks (K_mm, then
// K_nm^T K_nm + lam I), exactly like the reference's K_nmm (iterative.py:237-253).  After the
// factorisation rows [0,n) hold X = (L^-1 K_mn)^T, the preconditioner is P v = (X X^T v - v)/lam.
#include <math.h>

#include "common.h"
#include "precon_plan.h"

__global__ void __launch_bounds__(256) add_diag_kernel(double* __restrict__ A, int64_t ld, int64_t m,
                                                       double v) {
  int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < m) A[t * ld + t] += v;
}
static void add_diag(gdml_ctx* ctx, double* A, int64_t ld, int64_t m, double v) {
  hipLaunchKernelGGL(add_diag_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, ctx->stream, A, ld, m, v);
}
// A (m x ld) <- I
static int set_identity(gdml_ctx* ctx, double* A, int64_t m, int64_t ld) {
  HIP_CHECK(ctx, hipMemsetAsync(A, 0, m * ld * 8, ctx->stream));
  add_diag(ctx, A, ld, m, 1.0);
  return GDML_OK;
}
// the diagonal of A (m x ld, on the device) to the host; synchronises the stream
static int download_diag(gdml_ctx* ctx, const double* A, int64_t m, int64_t ld, std::vector<double>& diag) {
  diag.resize((size_t)m);
  hipError_t e = hipMemcpy2DAsync(diag.data(), 8, A, (ld + 1) * 8, 8, m, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return gdml_fail(ctx, GDML_ERR_HIP, "Gram diagonal: %s", hipGetErrorString(e));
  return GDML_OK;
}

// out[r] = sum_c X[r][c]^2   (leverage scores, iterative.py:107-109)
__global__ void __launch_bounds__(256) row_sqnorm_kernel(const double* __restrict__ X, int64_t ld,
                                                         int64_t n, int64_t m, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  double s = 0.0;
  for (int64_t c = lane; c < m; c += 64) {
    const double v = X[r * ld + c];
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) out[r] = s;
}

// ---- fp32-stored form of the factor (pcg.precon_form = 3).  The two GEMVs of an application are HBM bound at the rate
// the memory delivers (16 n m bytes per application); the factor's information content is not: what the preconditioner needs
// from X is its column SPACE to an angle theta with theta^2 sigma_max << lam (fp32: 6e-8), and the spectrum
// 1 - lam / (sigma_i + lam) on it -- which no rounded X can carry (1 - 1e-12), and which the stored fp64 factor itself only
// holds to ~1e-10 (profiles/r05_pcg_bisect.txt).  So X is rounded to fp32 (half the bytes) and the spectrum is put back
// by an m x m matrix:   P v = (X32 T0 X32^T v - v) / lam,   T0 = L_G^-T M0 L_G^-1,
// G = X32^T X32 = L_G L_G^T (fp64 Gram of the rounded factor: Q32 = X32 L_G^-T is orthonormal to rounding), and M0 the
// exact factor's operator in ITS orthonormal basis: X = Q L0^T with L0 L0^T = G0 = X^T X = I - lam L^-1 L^-T (the Gram of the
// exact factor; L L^T = K_nm^T K_nm + lam I, iterative.py:293-306), so X X^T = Q (L0^T L0) Q^T and M0 = L0^T L0.
// In exact arithmetic and without rounding (X32 = X, L_G = L0: T0 = I) this IS (X X^T v - v)/lam; with it, it is that
// operator carried over to range(X32).  Round 5 used G0 = L0 L0^T in the place of M0 = L0^T L0: the same eigenvalues on
// eigenvectors rotated by O(1 - s_min^2) inside range(X) -- invisible at lam = 1e-10 on well-supported inducing columns
// (s^2 ~ 1 - 1e-10), 3 % of the operator on the round-6 fixture n10_p2_pbc (lam = 1e-4, s_min^2 = 0.06), where the test
// that compares the forms found it.  M0 = G0 + (C^T C - C C^T) with C = I - L0: the difference is second order in C, so
// the entries ~1 of G0 (the spectrum 1 - lam / (sigma + lam) the form exists to carry) are never re-rounded.
// X32 <- float(X); pad columns [m, ld) of X32 <- 0.  X itself stays as it is (leverage scores, fall-back to the fp64 form)
__global__ void __launch_bounds__(256) round_f32_kernel(const double* __restrict__ X, int64_t ld, int64_t n, int64_t m,
                                                        float* __restrict__ X32) {
  const int64_t r = blockIdx.x;
  const double* row = X + r * ld;
  float* row32 = X32 + r * ld;
  for (int64_t c = threadIdx.x; c < ld; c += 256) row32[c] = c < m ? (float)row[c] : 0.0f;
}
// Compensated accumulation of the chunk Gram matrices (lower tiles): G += Gp with the running compensation in Gc.  The
// products of two fp32 values are exact in fp64, a chunk of 2048 rows is one short MFMA chain per entry, and the chunks are
// summed here with Kahan's scheme: the diagonal of G (entries ~1, the only ones whose rounding matters on the scale
// lam / sigma_max ~ 1e-13 the operator lives on) comes out to ~2e-16 instead of eps sqrt(n / 4) ~ 3e-14.
__global__ void __launch_bounds__(256) kahan_acc_lower_kernel(double* __restrict__ G, double* __restrict__ Gc,
                                                              const double* __restrict__ Gp, int64_t ld, int64_t m, int first) {
  const int64_t r = blockIdx.x;
  const int64_t cend = ((r / TT) + 1) * TT < m ? ((r / TT) + 1) * TT : m;  // the lower TILES hold valid data
  for (int64_t c = threadIdx.x; c < cend; c += 256) {
    const int64_t e = r * ld + c;
    if (first) {
      G[e] = Gp[e];
      Gc[e] = 0.0;
    } else {
      const double y = Gp[e] - Gc[e];
      const double t = G[e] + y;
      Gc[e] = (t - G[e]) - y;
      G[e] = t;
    }
  }
}
// T0 <- G0 - H - H^T + S   (in place on the buffer that holds G0)
__global__ void __launch_bounds__(256) t0_combine_kernel(double* __restrict__ T0, const double* __restrict__ H,
                                                         const double* __restrict__ S, int64_t ld, int64_t m) {
  const int64_t r = blockIdx.x;
  for (int64_t c = threadIdx.x; c < m; c += 256) T0[r * ld + c] = ((T0[r * ld + c] - H[r * ld + c]) - H[c * ld + r]) + S[r * ld + c];
}
// D (rows x ld doubles) <- double(float(X rows)), pad columns 0: what widen_f32_kernel gives for a rounded copy, without the copy
__global__ void __launch_bounds__(256) widen_round_kernel(const double* __restrict__ X, int64_t ld, int64_t m, double* __restrict__ D) {
  const int64_t r = blockIdx.x;
  for (int64_t c = threadIdx.x; c < ld; c += 256) D[r * ld + c] = c < m ? (double)(float)X[r * ld + c] : 0.0;
}
// In-place rounding of the factor (option pcg.f32_inplace, round 6): row r of X (ld doubles) becomes ld floats at the START of
// the same row -- X32 with a row pitch of 2 ld floats, no second buffer.  Chunks of 256 columns front to back: the floats of
// chunk k overlay doubles [128 k, 128 k + 128), all of which were read in this or an earlier chunk; floats [m, ld) <- 0.
__global__ void __launch_bounds__(256) round_f32_inplace_kernel(double* __restrict__ X, int64_t ld, int64_t m) {
  const int64_t r = blockIdx.x;
  const double* row = X + r * ld;
  float* row32 = reinterpret_cast<float*>(X + r * ld);
  for (int64_t c0 = 0; c0 < ld; c0 += 256) {
    const int64_t c = c0 + threadIdx.x;
    const float v = (c < m) ? (float)row[c < ld ? c : ld - 1] : 0.0f;
    __syncthreads();
    if (c < ld) row32[c] = v;
    __syncthreads();
  }
}
// D (rows x ld doubles) <- double(X32 rows): the Gram matrix of the rounded factor is accumulated chunk by chunk
__global__ void __launch_bounds__(256) widen_f32_kernel(const float* __restrict__ X32, int64_t ld, double* __restrict__ D) {
  const int64_t r = blockIdx.x;
  const float* src = X32 + r * ld;
  double* dst = D + r * ld;
  for (int64_t c = threadIdx.x; c < ld; c += 256) dst[c] = (double)src[c];
}
__global__ void __launch_bounds__(256) cg_scale_kernel(double* __restrict__ A, int64_t count, double f) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) A[i] *= f;
}
// A (lower triangle valid) mirrored into the upper triangle; then A <- I - A
__global__ void __launch_bounds__(256) sym_fill_kernel(double* __restrict__ A, int64_t ld, int64_t m) {
  const int64_t r = blockIdx.x;
  for (int64_t c = threadIdx.x; c < r; c += 256) A[c * ld + r] = A[r * ld + c];
}
__global__ void __launch_bounds__(256) eye_minus_kernel(double* __restrict__ A, int64_t ld, int64_t m) {
  const int64_t r = blockIdx.x;
  for (int64_t c = threadIdx.x; c < m; c += 256) A[r * ld + c] = (c == r ? 1.0 : 0.0) - A[r * ld + c];
}
// C <- I - L (lower triangle incl. the diagonal of L), 0 above the diagonal and in the pad columns [m, ld)
__global__ void __launch_bounds__(256) eye_minus_lower_kernel(const double* __restrict__ L, double* __restrict__ C, int64_t ld,
                                                              int64_t m) {
  const int64_t r = blockIdx.x;
  for (int64_t c = threadIdx.x; c < ld; c += 256) C[r * ld + c] = c > r || c >= m ? 0.0 : (c == r ? 1.0 : 0.0) - L[r * ld + c];
}

// Cholesky with escalating diagonal jitter (iterative.py:414-471).  A: m x m (lower referenced).
// Returns GDML_OK with *ok = 1 on success, *ok = 0 if every attempt failed.
// force_fail (test hook nys.force_fail): treat the first force_fail attempts as failed, whatever the factorisation says.
static int cho_factor_stable_dev(gdml_ctx* ctx, double* A, int64_t m, int64_t ld, double* backup,
                                 bool pre_reg, int eps_mag_max, int* ok, int force_fail = 0, int* n_jitter = nullptr) {
  const double eps = 2.220446049250313e-16;
  int eps_mag = (int)floor(log10(eps));  // -16
  if (pre_reg) {
    add_diag(ctx, A, ld, m, eps);
    eps_mag += 1;
  }
  *ok = 0;
  int attempt = 0;
  for (int mag = eps_mag; mag <= eps_mag_max; ++mag, ++attempt) {
    HIP_CHECK(ctx, hipMemcpy2DAsync(backup, m * 8, A, ld * 8, m * 8, m, hipMemcpyDeviceToDevice,
                                    ctx->stream));
    int info = 0;
    GDML_TRY(chol_factor_device(ctx, A, m, ld, &info));
    if (info == 0 && attempt >= force_fail) {
      *ok = 1;
      if (n_jitter) *n_jitter = attempt;
      return GDML_OK;
    }
    HIP_CHECK(ctx, hipMemcpy2DAsync(A, ld * 8, backup, m * 8, m * 8, m, hipMemcpyDeviceToDevice,
                                    ctx->stream));
    add_diag(ctx, A, ld, m, pow(10.0, (double)mag));
  }
  return GDML_OK;
}

// Row-shard geometry of the resident Nystroem matrix: this rank's n_loc rows are the entries [row0, row0 + n_loc) of the
// replicated device vectors, which are padded to n_pad = world * chunk doubles (VecLayout, common.h: the reference order when
// only forces are trained; rank-major with each rank's energy rows behind its force rows under energy constraints).
ShardGeo shard_geo(const gdml_ctx* ctx) {
  if (ctx->K_sharded) {
    ShardGeo g = vec_layout(ctx, ctx->K_use_E);
    g.n = ctx->K_rows_global;
    return g;
  }
  ShardGeo g;
  g.M = ctx->ts.M; g.N3 = 3 * (int64_t)ctx->ts.N; g.n_ff = g.M * g.N3; g.per = g.M;
  g.n = g.n_loc = g.chunk = g.n_pad = ctx->K_rows;
  g.row0 = 0;
  return g;
}

// dst rows (work block) <- -K[idx[q], :] for the rows this rank owns, zero otherwise (iterative.py:250)
__global__ void __launch_bounds__(256) gather_neg_rows_sharded_kernel(const double* __restrict__ X,
                                                                      double* __restrict__ S, int64_t ld,
                                                                      const int64_t* __restrict__ idx,
                                                                      int64_t m, VecLayout L) {
  const int64_t q = blockIdx.x;
  const int64_t r = L.pos(idx[q]) - L.row0;  // idx: reference order; the rank's rows: one run of the vector layout
  double* dst = S + q * ld;
  if (r >= 0 && r < L.n_loc) {
    const double* src = X + r * ld;
    for (int64_t c = threadIdx.x; c < m; c += 256) dst[c] = -src[c];
  } else {
    for (int64_t c = threadIdx.x; c < m; c += 256) dst[c] = 0.0;
  }
}

// fp32 copy and Gram correction of form 3, the matrix-free form's Z: released when the form is rejected and when the
// matrix buffer they belong to changes size (assemble.hip) -- not on every assembly: PCG restarts re-factor at one size
void precon_release_f32(gdml_ctx* ctx) {
  if (ctx->precon_X32 && !ctx->precon_X32_inplace) ctx_free(ctx, ctx->precon_X32);
  ctx->precon_X32_inplace = false;
  if (ctx->precon_T0) ctx_free(ctx, ctx->precon_T0);
  ctx->precon_X32 = nullptr; ctx->precon_X32_bytes = 0;
  ctx->precon_T0 = nullptr; ctx->precon_T0_bytes = 0;
}
void precon_release_aux(gdml_ctx* ctx) {
  precon_release_f32(ctx);
  if (ctx->precon_Z) ctx_free(ctx, ctx->precon_Z);
  ctx->precon_Z = nullptr; ctx->precon_Z_bytes = 0;
}

static int ensure_buf(gdml_ctx* ctx, void** p, int64_t* have, int64_t want) {
  if (*have >= want) return GDML_OK;
  if (*p) GDML_TRY(ctx_free(ctx, *p));
  *p = nullptr;
  *have = 0;
  GDML_TRY(ctx_alloc(ctx, p, want));
  *have = want;
  return GDML_OK;
}

// fp32 form: X (complete fp64 factor, rows of this rank) and S = L (lower, L L^T = K_nm^T K_nm + lam I) -> X32, T0.
// X itself is not modified.  *usable = 0 when the Gram matrix of the rounded factor cannot be factored or is too ill
// conditioned for X32 L_G^-T to be orthonormal to ~1e-9 (squared singular values sigma_i / (sigma_i + lam) of X below the
// threshold: inducing columns the data does not support, a numerically rank-deficient K_mm).  The caller then keeps the
// reference's fp64 form.
static int build_f32_form(gdml_ctx* ctx, double lam, double* X, const double* S, int64_t n_loc, int64_t m, int64_t ld,
                          int* usable, bool inplace) {
  *usable = 0;
  ctx->opts["pcg.f32_last_min_pivot"] = 0.0;
  hipStream_t st = ctx->stream;
  void* tmp = nullptr;
  {  // no room for the fp32 copy next to the fp64 factor: keep the reference's form (X is untouched at this point)
    int rc_a = inplace ? GDML_OK  // (the rounded factor will overlay the fp64 one: gdml_nystroem_factor converts it at the end)
                       : ensure_buf(ctx, (void**)&ctx->precon_X32, &ctx->precon_X32_bytes, (n_loc > 0 ? n_loc : 1) * ld * 4);
    if (rc_a == GDML_OK) rc_a = ensure_buf(ctx, (void**)&ctx->precon_T0, &ctx->precon_T0_bytes, m * ld * 8);
    if (rc_a == GDML_OK) rc_a = ctx_alloc(ctx, &tmp, 4 * m * ld * 8);
    // sharded: every rank must apply the same form (row blocks of ONE operator) -- free HBM differs between the ranks, so
    // the decision is collective: the form is kept only if the buffers fit everywhere.  EVERY local outcome goes through
    // the collective first (a rank that returned early on a non-OOM error left the others hanging in it); the error is
    // reported afterwards.
    double fits = rc_a == GDML_OK ? 1.0 : 0.0;
    if (comm_active(ctx)) {
      double* d_flag;
      GDML_TRY(ctx_slot(ctx, SLOT_PRECON_MF, 64, &d_flag));
      HIP_CHECK(ctx, hipMemcpyAsync(d_flag, &fits, 8, hipMemcpyHostToDevice, st));
      GDML_TRY(comm_allreduce_sum(ctx, d_flag, 1));
      HIP_CHECK(ctx, hipMemcpyAsync(&fits, d_flag, 8, hipMemcpyDeviceToHost, st));
      HIP_CHECK(ctx, hipStreamSynchronize(st));
      fits = fits >= (double)ctx->world - 0.5 ? 1.0 : 0.0;
    }
    if (fits < 0.5) {
      if (tmp) ctx_free(ctx, tmp);
      precon_release_f32(ctx);  // a partly allocated form (X32 fits, T0 or the work space does not) holds no memory
      return (rc_a != GDML_OK && rc_a != GDML_ERR_OOM) ? rc_a : GDML_OK;
    }
  }
  double* Rb = (double*)tmp;   // L^-T, later E_z = L_G^-T - I
  double* G = Rb + m * ld;     // Gram of the rounded factor, then its Cholesky factor, then S = W1 E_z^T
  double* Gc = G + m * ld;     // Kahan compensation of the Gram sum, then H = -W1
  double* Gp = Gc + m * ld;    // Gram matrix of one chunk of rows
  double* G0 = ctx->precon_T0; // lives in the T0 buffer until T0 itself is formed in place
  auto body = [&]() -> int {
    // G0 = I - lam L^-1 L^-T: R = L^-T (the solve applied to the identity), lam R^T R on the MFMA Gram kernel
    GDML_TRY(set_identity(ctx, Rb, m, ld));
    GDML_TRY(tall_trsm(ctx, S, Rb, m, m, ld));
    hipLaunchKernelGGL(cg_scale_kernel, dim3(ceil_div(m * ld, 256)), dim3(256), 0, st, Rb, m * ld, sqrt(lam));
    launch_gram_one_pass(ctx, Rb, ld, m, m, G0, ld);
    hipLaunchKernelGGL(sym_fill_kernel, dim3((unsigned)m), dim3(256), 0, st, G0, ld, m);
    hipLaunchKernelGGL(eye_minus_kernel, dim3((unsigned)m), dim3(256), 0, st, G0, ld, m);
    // rounded factor and its Gram matrix (summed over the row shards).  The fp32 values are widened chunk by chunk into a
    // work buffer (X stays untouched), every chunk's Gram matrix is one short MFMA chain per entry, and the chunks are
    // summed with compensation (kahan_acc_lower_kernel): the diagonal of G is what the spectrum correction hangs on
    if (n_loc > 0 && !inplace)
      hipLaunchKernelGGL(round_f32_kernel, dim3((unsigned)n_loc), dim3(256), 0, st, X, ld, n_loc, m, ctx->precon_X32);
    {
      const int64_t chunk = f32_gram_chunk((int64_t)ctx_opt(ctx, "pcg.f32_gram_rows", 2048), n_loc);
      double* D;
      GDML_TRY(ctx_slot(ctx, SLOT_F32_GRAM_ROWS, chunk * ld * 8, &D));
      HIP_CHECK(ctx, hipMemsetAsync(G, 0, 2 * m * ld * 8, st));  // G and Gc (upper tiles are never written again)
      for (int64_t r0 = 0; r0 < n_loc; r0 += chunk) {
        const int64_t rows = (n_loc - r0 < chunk) ? n_loc - r0 : chunk;
        if (inplace)
          hipLaunchKernelGGL(widen_round_kernel, dim3((unsigned)rows), dim3(256), 0, st, X + r0 * ld, ld, m, D);
        else
          hipLaunchKernelGGL(widen_f32_kernel, dim3((unsigned)rows), dim3(256), 0, st, ctx->precon_X32 + r0 * ld, ld, D);
        launch_gram_one_pass(ctx, D, ld, rows, m, Gp, ld);
        hipLaunchKernelGGL(kahan_acc_lower_kernel, dim3((unsigned)m), dim3(256), 0, st, G, Gc, Gp, ld, m, r0 == 0 ? 1 : 0);
      }
    }
    GDML_TRY(comm_allreduce_sum(ctx, G, m * ld));
    int inf = 0;
    int rcg = chol_factor_device(ctx, G, m, ld, &inf);
    if (rcg == GDML_ERR_NOT_PD || inf != 0) return GDML_OK;  // *usable stays 0: X is intact, the caller keeps the fp64 form
    GDML_TRY(rcg);
    {  // conditioning of the rounded factor's Gram matrix, from its Cholesky pivots: X32 L_G^-T is orthonormal to
       // eps cond(G); beyond ~1e7 the reference's form is kept (pcg.f32_min_pivot: threshold on the smallest squared pivot)
      std::vector<double> diag;
      GDML_TRY(download_diag(ctx, G, m, ld, diag));
      double dmin = 1e300;
      for (double d : diag) dmin = d < dmin ? d : dmin;
      ctx->opts["pcg.f32_last_min_pivot"] = dmin * dmin;  // diagnostic, read back with gdml_get_option
      if (!(dmin * dmin >= ctx_opt(ctx, "pcg.f32_min_pivot", 1e-7))) return GDML_OK;
    }
    // G0 <- M0 = L0^T L0 = G0 + (C^T C - C C^T), C = I - L0, L0 L0^T = G0 (see the derivation above build_f32_form's kernels)
    {
      HIP_CHECK(ctx, hipMemcpyAsync(Gp, G0, m * ld * 8, hipMemcpyDeviceToDevice, st));
      int inf0 = 0;
      const int rc0 = chol_factor_device(ctx, Gp, m, ld, &inf0);
      if (rc0 == GDML_ERR_NOT_PD || inf0 != 0) return GDML_OK;  // (cannot happen for a Gram matrix that passed the pivot test above)
      GDML_TRY(rc0);
      hipLaunchKernelGGL(eye_minus_lower_kernel, dim3((unsigned)m), dim3(256), 0, st, Gp, Rb, ld, m);
      launch_gram_one_pass(ctx, Rb, ld, m, m, Gc, ld);  // C^T C (lower tiles)
      hipLaunchKernelGGL(sym_fill_kernel, dim3((unsigned)m), dim3(256), 0, st, Gc, ld, m);
      GDML_TRY(launch_gemm_nt_sub(ctx, st, Rb, ld, Rb, ld, Gc, ld, m, m, m, 0));                   // - C C^T
      launch_vec_axpy(ctx, G0, Gc, 1.0, m * ld);
    }
    // T0 = Zt M0 Zt^T with Zt = L_G^-T = I + E_z.  Formed as G0 + W1 + W1^T + W1 E_z^T, W1 = E_z G0: every product has a
    // small factor (|E_z| ~ 1 - s_min^2), so the MFMA sums carry errors far below eps, and the entries ~1 of T0 come from
    // G0 by three additions -- as a plain triple product the diagonal would lose eps sqrt(m) ~ 5e-15, the scale of the
    // spectrum the matrix exists to carry.
    GDML_TRY(set_identity(ctx, Rb, m, ld));
    GDML_TRY(tall_trsm(ctx, G, Rb, m, m, ld));
    add_diag(ctx, Rb, ld, m, -1.0);  // Rb = E_z
    double* H = Gc;
    double* Sx = G;
    HIP_CHECK(ctx, hipMemsetAsync(H, 0, m * ld * 8, st));
    GDML_TRY(launch_gemm_nt_sub(ctx, st, Rb, ld, G0, ld, H, ld, m, m, m, 0));   // H = -(E_z G0^T) = -W1
    HIP_CHECK(ctx, hipMemsetAsync(Sx, 0, m * ld * 8, st));
    GDML_TRY(launch_gemm_nt_sub(ctx, st, H, ld, Rb, ld, Sx, ld, m, m, m, 0));   // S = -(H E_z^T) = W1 E_z^T
    hipLaunchKernelGGL(t0_combine_kernel, dim3((unsigned)m), dim3(256), 0, st, ctx->precon_T0, H, Sx, ld, m);
    HIP_CHECK(ctx, hipGetLastError());
    *usable = 1;
    return GDML_OK;
  };
  int rc = body();
  int rc2 = ctx_free(ctx, tmp);
  if (rc != GDML_OK || !*usable) precon_release_f32(ctx);  // rejected form: the fp64 factor is what stays resident
  return rc != GDML_OK ? rc : rc2;
}

// leverage scores = squared row norms of the complete factor X (iterative.py:107-109), replicated on every rank
static int lev_scores_to_host(gdml_ctx* ctx, const ShardGeo& sg, double* lev_scores_out) {
  const int64_t n_loc = sg.n_loc, m = ctx->precon_m, ld = ctx->K_ld;
  double* X = ctx->precon;
  if (ctx->precon_stage < 2) {  // the matrix-free form left X = K_nm L_mm^-T: the second solve (iterative.py:335-345) now
    GDML_TRY(tall_trsm(ctx, ctx->K + n_loc * ld, X, n_loc, m, ld));
    ctx->precon_stage = 2;
  }
  double* d_lev;
  GDML_TRY(ctx_slot(ctx, SLOT_LEV_SCORES, sg.n_pad * 8, &d_lev));
  if (n_loc > 0)
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3(ceil_div(n_loc, 4)), dim3(256), 0, ctx->stream, X, ld, n_loc, m,
                       d_lev + sg.row0);
  GDML_TRY(comm_allgather_inplace(ctx, d_lev, sg.chunk));
  return vec_download(ctx, sg, d_lev, lev_scores_out);  // reference order
}

extern "C" int gdml_nystroem_lev_scores(gdml_ctx* ctx, double* lev_scores_out) {
  if (!ctx || !lev_scores_out) return GDML_ERR_INVALID;
  if (!ctx->precon || !ctx->K)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_nystroem_lev_scores: no Nystroem factor resident (an assembly since "
                                          "gdml_nystroem_factor overwrites it)");
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const ShardGeo sg = shard_geo(ctx);
  if (ctx->precon_X32_inplace) {  // the fp64 factor was rounded in place: the scores were taken before that
    if ((int64_t)ctx->precon_lev_cache.size() != sg.n) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_nystroem_lev_scores: no cached scores");
    memcpy(lev_scores_out, ctx->precon_lev_cache.data(), (size_t)sg.n * 8);
    return GDML_OK;
  }
  int rc = lev_scores_to_host(ctx, sg, lev_scores_out);
  if (rc == GDML_ERR_HIP) comm_abort(ctx);
  return rc;
}

extern "C" int gdml_nystroem_factor(gdml_ctx* ctx, double lam, const int64_t* idx, int64_t m,
                                    double* lev_scores_out, double* LinvKmn_host_out, int* info) {
  if (!ctx || !idx || m < 1) return GDML_ERR_INVALID;
  if (!ctx->K || ctx->K_cols != m || ctx->K_extra < m)
    return gdml_fail(ctx, GDML_ERR_STATE,
                     "gdml_nystroem_factor: needs the (n+m) x m matrix of gdml_assemble_K(INDEX, extra=m)");
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const ShardGeo sg = shard_geo(ctx);
  const int64_t n_loc = sg.n_loc, ld = ctx->K_ld;
  if (info) *info = 0;
  double* X = ctx->K;               // this rank's rows of K_nm
  double* S = ctx->K + n_loc * ld;  // m x m work block (replicated)
  int form = choose_precon_form(ctx_opt_i(ctx, "pcg.precon_form", 2), sg.chunk, m);
  // fp32 form: the rounded factor overlays the fp64 one (no 1.5 x footprint; leverage scores are cached first) unless the
  // caller wants the fp64 factor kept (pcg.f32_inplace = 0)
  const bool f32_inplace = ctx_opt_i(ctx, "pcg.f32_inplace", 1) != 0;
  if (ctx->precon_X32_inplace) {  // the overlay of the previous factor went with the assembly that rebuilt this matrix
    ctx->precon_X32 = nullptr;
    ctx->precon_X32_inplace = false;
  }
  ctx->precon_lev_cache.clear();
  // matrix-free form: Z = L_mm^-T L^-T, built by applying to the m x m identity every triangular solve X receives
  double* Z = nullptr;
  if (form == 1) {
    GDML_TRY(ensure_buf(ctx, (void**)&ctx->precon_Z, &ctx->precon_Z_bytes, m * ld * 8));
    Z = ctx->precon_Z;
  }
  GDML_TRY(ensure_buf(ctx, (void**)&ctx->precon_idx, &ctx->precon_idx_bytes, m * 8));
  int64_t* d_idx = ctx->precon_idx;
  void* tmp = nullptr;
  GDML_TRY(ctx_alloc(ctx, &tmp, m * m * 8));
  double* backup = (double*)tmp;
  // the second solve of X is only needed by the stored form, the leverage scores and the host copy
  const bool want_X = form != 1 || lev_scores_out || LinvKmn_host_out;
  int stage = 1;
  int rc = GDML_OK;
  auto body = [&]() -> int {
    HIP_CHECK(ctx, hipMemcpyAsync(d_idx, idx, m * 8, hipMemcpyHostToDevice, ctx->stream));
    phase_begin(ctx);
    if (Z) GDML_TRY(set_identity(ctx, Z, m, ld));
    // K_mm = -K[idx, :]: every rank contributes the rows it owns, the sum replicates the block
    hipLaunchKernelGGL(gather_neg_rows_sharded_kernel, dim3((unsigned)m), dim3(256), 0, ctx->stream, X, S,
                       ld, d_idx, m, sg);
    GDML_TRY(comm_allreduce_sum(ctx, S, m * ld));
    int ok = 0;
    int n_jit = 0;
    GDML_TRY(cho_factor_stable_dev(ctx, S, m, ld, backup, true, 1, &ok, ctx_opt_i(ctx, "nys.force_fail", 0), &n_jit));  // iterative.py:263
    if (info) *info |= n_jit << 8;
    if (!ok)
      return gdml_fail(ctx, GDML_ERR_NOT_PD,
                       "Failed to factorize despite strong regularization (max: 10)! You could try a larger sigma.");
    GDML_TRY(tall_trsm(ctx, S, X, n_loc, m, ld));  // K_nm <- K_nm L_mm^-T  (iterative.py:276-286)
    if (Z) GDML_TRY(tall_trsm(ctx, S, Z, m, m, ld));
    // inner = K_nm^T K_nm + lam I  (iterative.py:293-294): local SYRK, summed over the shards
    GDML_TRY(gram_tn(ctx, X, ld, n_loc, m, S, ld));
    GDML_TRY(comm_allreduce_sum(ctx, S, m * ld));
    add_diag(ctx, S, ld, m, lam);
    GDML_TRY(cho_factor_stable_dev(ctx, S, m, ld, backup, false, -14, &ok));  // iterative.py:304-306
    if (ok && ctx_opt_i(ctx, "nys.force_qr", 0)) ok = 0;  // test hook: take the alternative branch
    if (ok) {
      if (want_X) {
        GDML_TRY(tall_trsm(ctx, S, X, n_loc, m, ld));  // iterative.py:335-345
        stage = 2;
      }
      if (Z) GDML_TRY(tall_trsm(ctx, S, Z, m, m, ld));
      if (form == 3) {
        int usable = 0;
        GDML_TRY(build_f32_form(ctx, lam, X, S, n_loc, m, ld, &usable, f32_inplace));
        if (!usable) form = 0;
      }
    } else {
      if (form == 3) form = 0;  // no Cholesky factor of the inner matrix to take the exact Gram from: the reference's form
      // "QR fact. (alt.)" (iterative.py:313-324): R of the stacked matrix [K_nm; sqrt(lam) I], i.e. the Cholesky
      // factor of K_nm^T K_nm + lam I obtained WITHOUT trusting the Gram matrix.  Here: shifted CholeskyQR3 -- three
      // rounds of (Gram on fp64 MFMA, small Cholesky, tall triangular solve); the first Gram is shifted so that
      // its factorisation cannot fail, the two repetitions remove the shift's error (R = R3 R2 R1 is never
      // formed: the triangular solves apply R1^-1, R2^-1, R3^-1 to K_nm in turn).  Backward stable like
      // Householder QR for cond([K_nm; sqrt(lam) I]) up to ~1/eps, and GEMM-shaped instead of panel-bound.
      if (info) *info |= 1;
      const double eps = 2.220446049250313e-16;
      double* B = S;  // the stacked sqrt(lam) I block lives right below X: one Gram launch covers both
      HIP_CHECK(ctx, hipMemsetAsync(B, 0, m * ld * 8, ctx->stream));
      add_diag(ctx, B, ld, m, sqrt(lam));
      void* gtmp = nullptr;
      GDML_TRY(ctx_alloc(ctx, &gtmp, m * ld * 8));
      double* G = (double*)gtmp;
      int rcq = GDML_OK;
      for (int pass = 0; pass < 3 && rcq == GDML_OK; ++pass) {
        // the replicated block B enters the Gram sum once: on rank 0 (or when nothing is sharded)
        const int64_t rows = n_loc + ((!ctx->K_sharded || ctx->rank == 0) ? m : 0);
        launch_gram_one_pass(ctx, X, ld, rows, m, G, ld);
        rcq = comm_allreduce_sum(ctx, G, m * ld);
        if (rcq != GDML_OK) break;
        if (pass == 0) {
          std::vector<double> diag;
          rcq = download_diag(ctx, G, m, ld, diag);
          if (rcq != GDML_OK) break;
          double tr = 0.0;
          for (double d : diag) tr += d;  // ||A||_2^2 <= ||A||_F^2 = trace(A^T A)
          const double rows_tot = (double)sg.n + (double)m;
          const double shift = 11.0 * ((double)m * rows_tot + (double)m * ((double)m + 1.0)) * eps * tr;
          add_diag(ctx, G, ld, m, shift);
        }
        int inf = 0;
        rcq = chol_factor_device(ctx, G, m, ld, &inf);
        if (rcq == GDML_OK && inf != 0)
          rcq = gdml_fail(ctx, GDML_ERR_NOT_PD, "Nystroem factor: K_nm^T K_nm + lam I is singular to working precision "
                                                "(shifted CholeskyQR pass %d failed at pivot %d)", pass + 1, inf);
        if (rcq == GDML_OK) rcq = tall_trsm(ctx, G, X, n_loc + m, m, ld);  // X and B (every rank its own copy of B)
        if (rcq == GDML_OK && Z) rcq = tall_trsm(ctx, G, Z, m, m, ld);
      }
      stage = 2;  // the three factors are gone after this branch: X is always completed here
      int rcf = ctx_free(ctx, gtmp);
      GDML_TRY(rcq);
      GDML_TRY(rcf);
    }
    GDML_TRY(phase_end(ctx, "precon"));
    return GDML_OK;
  };
  rc = body();
  if (rc == GDML_ERR_HIP) comm_abort(ctx);  // a LOCAL failure (errors computed from replicated data hit every rank alike)
  if (rc == GDML_OK) {
    ctx->precon = X;
    ctx->precon_m = m;
    ctx->precon_n = sg.n;
    ctx->precon_form = form;
    ctx->precon_stage = stage;
    ctx->precon_sig = ctx->K_sig;
    ctx->precon_use_E = ctx->K_use_E;
    if (info && form == 1) *info |= 2;
    if (info && form == 3) *info |= 4;
    if (lev_scores_out) {
      rc = lev_scores_to_host(ctx, sg, lev_scores_out);
      if (rc == GDML_ERR_HIP) comm_abort(ctx);
    }
    if (rc == GDML_OK && LinvKmn_host_out) {
      // host gets this rank's columns of L^-1 K_mn as an (m x n_loc) array: transpose of X
      std::vector<double> h((size_t)n_loc * m);
      hipError_t e = hipMemcpy2DAsync(h.data(), m * 8, X, ld * 8, m * 8, n_loc, hipMemcpyDeviceToHost,
                                      ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess)
        rc = gdml_fail(ctx, GDML_ERR_HIP, "factor copy: %s", hipGetErrorString(e));
      else
        for (int64_t r = 0; r < n_loc; ++r)
          for (int64_t c = 0; c < m; ++c) LinvKmn_host_out[c * n_loc + r] = h[(size_t)r * m + c];
    }
    ctx->precon_lev_cache.clear();
    ctx->precon_X32_ld = ld;
    if (rc == GDML_OK && form == 3 && f32_inplace) {
      // everything that needs the fp64 factor has happened; the leverage scores (restart policy, iterative.py:107-109) are
      // taken now and served from the cache, then X is rounded where it stands
      ctx->precon_lev_cache.resize((size_t)sg.n);
      rc = lev_scores_to_host(ctx, sg, ctx->precon_lev_cache.data());
      if (rc == GDML_ERR_HIP) comm_abort(ctx);
      if (rc == GDML_OK) {
        if (n_loc > 0) hipLaunchKernelGGL(round_f32_inplace_kernel, dim3((unsigned)n_loc), dim3(256), 0, ctx->stream, X, ld, m);
        ctx->precon_X32 = reinterpret_cast<float*>(X);
        ctx->precon_X32_bytes = 0;
        ctx->precon_X32_inplace = true;
        ctx->precon_X32_ld = 2 * ld;
        if (hipGetLastError() != hipSuccess) rc = gdml_fail(ctx, GDML_ERR_HIP, "in-place rounding of the factor failed to launch");
      }
    }
  }
  int rc2 = ctx_free(ctx, tmp);
  return rc != GDML_OK ? rc : rc2;
}
