// Triangular solves with the factor of chol.hip, the tall solve X L^-T of the Nystroem build and of the resident-factor entries
// (tall_trsm), and the C entries of the analytic solve (gdml_chol_set_rhs / _factor / _solve).
#include "common.h"
// A <- -A + lam I on the lower triangle (analytic.py:65,82), tiled copy-free.
__global__ void __launch_bounds__(256) negate_shift_kernel(double* __restrict__ A, int64_t n,
                                                           int64_t ld, double lam) {
  const int64_t r = blockIdx.x;
  double* row = A + r * ld;
  for (int64_t c = threadIdx.x; c <= r; c += 256) {
    double v = -row[c];
    if (c == r) v += lam;
    row[c] = v;
  }
}

// ------------------------------------------------------------------------------------------
// Triangular solves with the factor (cho_solve, analytic.py:97-99), blocked by 64.
// Forward  L z = b : per block J the kernel first solves the 64x64 diagonal system in LDS (every
// workgroup redundantly: 32 KB from L2), then updates its rows below: b[r] -= L[r,J] z_J.
// Backward L^T x = z : per block I (from the bottom) solve L_II^T x_I = z_I, then
// z[c] -= sum_{r in I} L[r,c] x[r] for the columns c left of the block (one thread per column).
// ------------------------------------------------------------------------------------------
// 64x64 triangular solve by ONE wavefront, operands in registers.
//   TRANS = false: L z = b, lane r holds row r of L;    TRANS = true: L^T x = b, lane c holds column c.
// Ls: LDS copy of the block ([64][65], identity-padded), b: this lane's right-hand side entry.
template <bool TRANS>
__device__ __forceinline__ double tri_solve64_wave(const double* Ls, double b, int lane) {
  double v[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) v[k] = TRANS ? Ls[k * 65 + lane] : Ls[lane * 65 + k];
  double sol = 0.0;
  if (!TRANS) {
#pragma unroll
    for (int c = 0; c < 64; ++c) {
      const double t = b / v[c];            // meaningful on lane c
      const double zc = __shfl(t, c, 64);
      if (lane == c) sol = zc;
      b -= v[c] * zc;                       // lanes r > c use it; others ignore their b afterwards
    }
  } else {
#pragma unroll
    for (int r = 63; r >= 0; --r) {
      const double t = b / v[r];            // lane r: v[r] = L[r][r]
      const double xr = __shfl(t, r, 64);
      if (lane == r) sol = xr;
      b -= v[r] * xr;                       // lane c < r: L[r][c] x_r
    }
  }
  return sol;
}

__device__ __forceinline__ void load_block64(const double* __restrict__ L, int64_t ld, int64_t c0,
                                             int w, double* Ls, int tid, int T) {
  for (int e = tid; e < 64 * 64; e += T) {
    int r = e >> 6, c = e & 63;
    double v = (r == c) ? 1.0 : 0.0;
    if (r < w && c < w && c <= r) v = L[(c0 + r) * ld + c0 + c];
    Ls[r * 65 + c] = v;
  }
}

__global__ void __launch_bounds__(256) trsv_fwd_kernel(const double* __restrict__ L, int64_t ld,
                                                       int64_t n, int64_t c0, int w,
                                                       double* __restrict__ b,
                                                       double* __restrict__ z_out) {
  __shared__ __attribute__((aligned(16))) double Ls[64 * 65];
  __shared__ double z[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  load_block64(L, ld, c0, w, Ls, tid, 256);
  __syncthreads();
  if (wave == 0) {
    const double bi = lane < w ? b[c0 + lane] : 0.0;
    const double zi = tri_solve64_wave<false>(Ls, bi, lane);
    z[lane] = zi;
    if (blockIdx.x == 0 && lane < w) z_out[c0 + lane] = zi;
  }
  __syncthreads();
  // rows below: one wave per row, lanes over the w columns
  const int64_t first = c0 + w;
  const double zl = lane < w ? z[lane] : 0.0;
  for (int64_t r = first + (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
    double v = lane < w ? L[r * ld + c0 + lane] * zl : 0.0;
    v = wave_sum(v);
    if (lane == 0) b[r] -= v;
  }
}

__global__ void __launch_bounds__(256) trsv_bwd_kernel(const double* __restrict__ L, int64_t ld,
                                                       int64_t c0, int w, double* __restrict__ b,
                                                       double* __restrict__ x_out) {
  __shared__ __attribute__((aligned(16))) double Ls[64 * 65];
  __shared__ double x[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  load_block64(L, ld, c0, w, Ls, tid, 256);
  __syncthreads();
  if (wave == 0) {
    const double bi = lane < w ? b[c0 + lane] : 0.0;
    const double xi = tri_solve64_wave<true>(Ls, bi, lane);
    x[lane] = xi;
    if (blockIdx.x == 0 && lane < w) x_out[c0 + lane] = xi;
  }
  __syncthreads();
  // columns left of the block: z[c] -= sum_{r in block} L[r,c] x[r]   (one thread per column)
  for (int64_t c = (int64_t)blockIdx.x * 256 + tid; c < c0; c += (int64_t)gridDim.x * 256) {
    double s = 0.0;
    for (int r = 0; r < w; ++r) s += L[(c0 + r) * ld + c] * x[r];
    b[c] -= s;
  }
}

// d_b: right-hand side (destroyed), d_z: scratch (n), d_x: solution (n).  All device vectors.
static int chol_fwd_device(gdml_ctx* ctx, const double* L, int64_t n, int64_t ld, double* d_b, double* d_z) {
  for (int64_t c0 = 0; c0 < n; c0 += 64) {
    int w = (int)((n - c0 < 64) ? n - c0 : 64);
    int64_t rows = n - c0 - w;
    int grid = (int)((rows + 3) / 4);
    if (grid < 1) grid = 1;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(trsv_fwd_kernel, dim3(grid), dim3(256), 0, ctx->stream, L, ld, n, c0, w, d_b,
                       d_z);
    ctx->launch_counter++;
  }
  return GDML_OK;
}

// ------------------------------------------------------------------------------------------
// Backward substitution L^T x = z as ONE persistent launch (default for n >= 2048; option trsv.persist = 0
// restores the per-block launches).  Left-looking: the workgroup that owns 64-block k accumulates
//   s = sum_{c > k} L[c,k]^T x_c      (rows below the block, 512-byte row segments, 4 wavefronts over the blocks c)
// as the x_c become available, then solves the transposed diagonal block and publishes x_k.  Blocks are
// owned cyclically (from the bottom) by one workgroup per CU, all resident at once.  The solution vector itself is the
// availability signal: it is pre-filled with a NaN sentinel, x_k is published with relaxed agent-scope 8-byte stores and
// the consumers poll the elements they need (x crosses
// XCDs, i.e. L2s).  Blocks are dealt round-robin, so a workgroup also waits for blocks of workgroups with a HIGHER
// index (workgroup 0 at round 2 needs the last workgroup's block of round 1): all min(nbk, CUs) workgroups must
// be resident at once.  One workgroup per CU on an otherwise idle stream satisfies that; where it does not (GPU
// shared with another process) the bounded spins give up, `err` is set and the host falls back to the
// per-block launches below.
// ------------------------------------------------------------------------------------------
// Sentinel of "not yet solved" in the solution vector of the persistent backward substitution: a quiet NaN with a
// payload no arithmetic produces (hardware NaNs are 0x7FF8000000000000 / 0xFFF8...).
#define TRSV_PENDING 0x7FF8A5A5C3C30001ull

__global__ void __launch_bounds__(256) trsv_fill_pending_kernel(unsigned long long* __restrict__ x, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) x[t] = TRSV_PENDING;
}

__global__ void __launch_bounds__(256) trsv_bwd_persist_kernel(const double* __restrict__ L, int64_t ld,
                                                               int64_t n, int nbk, const double* __restrict__ z,
                                                               double* x, int* err) {
  __shared__ __attribute__((aligned(16))) double Ls[64 * 65];
  __shared__ double part[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned long long* xb = reinterpret_cast<unsigned long long*>(x);
  for (int kk = blockIdx.x; kk < nbk; kk += gridDim.x) {  // kk counts blocks from the bottom
    const int k = nbk - 1 - kk;
    const int64_t c0 = (int64_t)k * 64;
    const int wk = (int)((n - c0 < 64) ? n - c0 : 64);
    load_block64(L, ld, c0, wk, Ls, tid, 256);  // diagonal block (independent of x): overlaps the waiting
    __syncthreads();
    const double rdiag = 1.0 / Ls[lane * 65 + lane];  // reciprocal pivots off the critical path (identity on padding)
    double acc = 0.0;
    for (int cc = wv; cc < kk; cc += 4) {  // blocks below, bottom first; this wavefront takes every 4th
      const int c = nbk - 1 - cc;
      const int64_t r0 = (int64_t)c * 64;
      const int rows = (int)((n - r0 < 64) ? n - r0 : 64);
      // the L block does not depend on x: its 64 row segments are in flight while the wavefront waits for x_c
      const double* Lp = L + r0 * ld + c0 + (lane < wk ? lane : 0);
      double lreg[64];
#pragma unroll
      for (int i = 0; i < 64; ++i) lreg[i] = (i < rows) ? Lp[(int64_t)i * ld] : 0.0;
      // x_c is published element by element (relaxed agent-scope stores of the 8-byte values over the sentinel): the
      // consumer polls the data itself -- one memory round trip, no separate flag, no fences
      unsigned long long xv = 0;
      int spins = 0;
      for (;;) {
        xv = (lane < rows) ? __hip_atomic_load(xb + r0 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        if (!__any(xv == TRSV_PENDING)) break;
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 26)) {  // ~1 min: only reachable if the GPU is shared with another process for that long
          if (lane == 0) atomicExch(err, 1);
          xv = 0;
          break;
        }
      }
      const double xd = __longlong_as_double((long long)xv);
#pragma unroll
      for (int i = 0; i < 64; ++i) acc += lreg[i] * __shfl(xd, i, 64);
    }
    part[wv][lane] = (lane < wk) ? acc : 0.0;
    __syncthreads();
    if (wv == 0) {
      const double s = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
      double bi = lane < wk ? z[c0 + lane] - s : 0.0;
      // transposed 64 x 64 solve, row r of L broadcast from lane r: x_r = b_r / L_rr; b_c -= L_rc x_r (c < r)
      double sol = 0.0;
#pragma unroll
      for (int r = 63; r >= 0; --r) {
        const double xr = __shfl(bi * rdiag, r, 64);
        if (lane == r) sol = xr;
        bi -= Ls[r * 65 + lane] * xr;
      }
      if (lane < wk)
        __hip_atomic_store(xb + c0 + lane, (unsigned long long)__double_as_longlong(sol), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
  }
}

// d_z is destroyed
int chol_bwd_device(gdml_ctx* ctx, const double* L, int64_t n, int64_t ld, double* d_z, double* d_x) {
  const int persist = ctx_opt_i(ctx, "trsv.persist", 1);
  if (persist && n >= 2048) {
    const int nbk = (int)((n + 63) / 64);
    int* err = ctx->d_info + 5;
    HIP_CHECK(ctx, hipMemsetAsync(err, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(trsv_fill_pending_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<unsigned long long*>(d_x), n);
    const int grid = nbk < ctx->num_cus ? nbk : ctx->num_cus;  // one workgroup per CU, all resident
    hipLaunchKernelGGL(trsv_bwd_persist_kernel, dim3(grid), dim3(256), 0, ctx->stream, L, ld, n, nbk, d_z, d_x, err);
    ctx->launch_counter++;
    int h_err = 0;
    HIP_CHECK(ctx, hipMemcpyAsync(&h_err, err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (h_err == 0) return GDML_OK;
    // a workgroup gave up waiting (the persistent launch needs all its workgroups co-resident: not guaranteed when
    // the GPU is shared): d_z was only read so far, redo the substitution with one launch per block
  }
  int64_t last = ((n - 1) / 64) * 64;
  for (int64_t c0 = last; c0 >= 0; c0 -= 64) {
    int w = (int)((n - c0 < 64) ? n - c0 : 64);
    int grid = (int)((c0 + 255) / 256);
    if (grid < 1) grid = 1;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(trsv_bwd_kernel, dim3(grid), dim3(256), 0, ctx->stream, L, ld, c0, w, d_z,
                       d_x);
    ctx->launch_counter++;
  }
  HIP_CHECK(ctx, hipGetLastError());
  return GDML_OK;
}

int chol_solve_device(gdml_ctx* ctx, const double* L, int64_t n, int64_t ld, double* d_b,
                      double* d_z, double* d_x) {
  GDML_TRY(chol_fwd_device(ctx, L, n, ld, d_b, d_z));
  return chol_bwd_device(ctx, L, n, ld, d_z, d_x);
}

// X[:, 0:m] <- X L^-T  for the n rows of X (L: m x m lower), blocked 512 / 64 like the Cholesky.
// Round 6: LEFT-looking (option nys.trsm_left, default 1): a 512-column strip receives everything the solved strips to its left
// owe it in ONE product of depth k0 and is then solved, instead of being read, updated by 512 and written back once per earlier
// strip -- m / 1024 times less traffic on X and long k loops (the K = 512 update ran at 0.55 of the MFMA peak inside the
// configs[3] build, profiles/r06_cfg34_kernel_stats.txt).  Same flops, same operations in another order.
int tall_trsm(gdml_ctx* ctx, const double* L, double* X, int64_t n, int64_t m, int64_t ld, int look) {
  const int64_t NB = 512;
  hipStream_t st = ctx->stream;
  const bool left = look < 0 ? ctx_opt_i(ctx, "nys.trsm_left", 1) != 0 : look != 0;
  for (int64_t k0 = 0; k0 < m; k0 += NB) {
    const int64_t nb = (m - k0 < NB) ? m - k0 : NB;
    if (left && k0 > 0)  // X[:, k0:k0+nb] -= X[:, 0:k0] L[k0:k0+nb, 0:k0]^T
      GDML_TRY(launch_gemm_nt_sub(ctx, st, X, ld, L + k0 * ld, ld, X + k0, ld, n, nb, k0, 0));
    const bool aligned = ((reinterpret_cast<uintptr_t>(L) | reinterpret_cast<uintptr_t>(X)) & 31) == 0 && (ld % 4 == 0);
    if (nb % 64 == 0 && aligned) {
      // whole NB-wide strip in one row-local launch (the kernel of the Cholesky panels) instead of 8 x (trsm64 + K = 64 GEMM)
      GDML_TRY(launch_panel_trsm(ctx, st, L + k0 * ld + k0, X + k0, ld, (int)nb, n));
    } else
    for (int64_t jj = 0; jj < nb; jj += 64) {
      const int64_t c0 = k0 + jj;
      const int w = (int)((nb - jj < 64) ? nb - jj : 64);
      GDML_TRY(launch_trsm64(ctx, st, L + c0 * ld + c0, X + c0, ld, w, n));
      const int64_t ncols = k0 + nb - (c0 + w);
      if (ncols > 0)
        GDML_TRY(launch_gemm_nt_sub(ctx, st, X + c0, ld, L + (c0 + w) * ld + c0, ld, X + c0 + w, ld, n,
                                    ncols, w, 0));
    }
    const int64_t t0 = k0 + nb;
    if (!left && t0 < m)
      GDML_TRY(launch_gemm_nt_sub(ctx, st, X + k0, ld, L + t0 * ld + k0, ld, X + t0, ld, n, m - t0, nb, 0));
  }
  return GDML_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" int gdml_chol_set_rhs(gdml_ctx* ctx, const double* y, int64_t n) {
  if (!ctx || !y) return GDML_ERR_INVALID;
  if (!ctx->K || ctx->K_rows != ctx->K_cols)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_chol_set_rhs: assemble a square K first");
  if (ctx->K_factored) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_chol_set_rhs: K is already factored");
  if (ctx->K_extra < 1)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_chol_set_rhs: K was assembled without an extra row");
  if (n != ctx->K_rows) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_chol_set_rhs: n mismatch");
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (ctx->d_rhs) GDML_TRY(ctx_free(ctx, ctx->d_rhs));
  ctx->d_rhs = nullptr;
  GDML_TRY(ctx_alloc(ctx, (void**)&ctx->d_rhs, n * 8));
  HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_rhs, y, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(ctx, hipMemcpyAsync(ctx->K + n * ctx->K_ld, ctx->d_rhs, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // y is a pageable host array owned by the caller
  ctx->K_rhs_row = true;
  return GDML_OK;
}

extern "C" int gdml_chol_factor(gdml_ctx* ctx, double lam, int* info) {
  if (!ctx) return GDML_ERR_INVALID;
  if (!ctx->K) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_chol_factor: assemble K first");
  if (ctx->K_rows != ctx->K_cols)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_chol_factor: resident K is %lld x %lld, not square",
                     (long long)ctx->K_rows, (long long)ctx->K_cols);
  if (ctx->K_factored) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_chol_factor: already factored");
  if (ctx->K_destroyed)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_chol_factor: the resident matrix was consumed by a failed factorisation: assemble again");
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t n = ctx->K_rows;
  if (ctx->K_is_A && lam != ctx->K_lam)
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_chol_factor: lam (%g) differs from the one gdml_assemble_A used (%g)",
                     lam, ctx->K_lam);
  phase_begin(ctx);
  if (!ctx->K_is_A) {  // un-negated K from gdml_assemble_K: A = -K + lam I on the lower triangle (analytic.py:65,82)
    hipLaunchKernelGGL(negate_shift_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, ctx->K, n,
                       ctx->K_ld, lam);
    ctx->launch_counter++;
  }
  int inf = 0;
  GDML_TRY(chol_factor_device(ctx, ctx->K, n, ctx->K_ld, &inf, ctx->K_rhs_row ? n + 1 : n));
  GDML_TRY(phase_end(ctx, "factor"));
  if (info) *info = inf;
  ctx->K_lam = lam;
  if (inf != 0) {
    ctx->K_factored = false;
    ctx->K_destroyed = true;
    return gdml_fail(ctx, GDML_ERR_NOT_PD,
                     "%d-th leading minor of the array is not positive definite", inf);
  }
  ctx->K_factored = true;
  return GDML_OK;
}

__global__ void __launch_bounds__(256) scale_kernel(double* __restrict__ x, int64_t n, double s) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) x[t] *= s;
}
__global__ void __launch_bounds__(256) axpy_kernel(double* __restrict__ y, const double* __restrict__ x,
                                                   int64_t n, double a) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) y[t] += a * x[t];
}
// r = y - (-(Kx - lam x))... helper: r = y + kv  where kv = K x - lam x  (A x = -(K x - lam x))
__global__ void __launch_bounds__(256) resid_kernel(const double* __restrict__ y,
                                                    const double* __restrict__ kv, int64_t n,
                                                    double* __restrict__ r) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) r[t] = y[t] + kv[t];
}

int operator_model_from_trainset(gdml_ctx* ctx, double sig);

extern "C" int gdml_chol_solve(gdml_ctx* ctx, const double* y, int64_t n, int n_refine,
                               double* alphas_out) {
  if (!ctx || !alphas_out) return GDML_ERR_INVALID;
  if (!ctx->K || !ctx->K_factored)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_chol_solve: no Cholesky factor resident");
  if (!y && !ctx->K_rhs_row)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_chol_solve(y = NULL) needs gdml_chol_set_rhs before the factorisation");
  if (n != ctx->K_rows) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_chol_solve: n mismatch");
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  void* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, &buf, 6 * n * 8));
  double* dx = (double*)buf;   // solution
  double* dy = dx + n;         // right-hand side (kept)
  double* db = dy + n;         // work copy of a right-hand side (destroyed by the solve)
  double* dz = db + n;         // forward-substitution result
  double* dr = dz + n;         // refinement correction
  double* dkv = dr + n;        // K x - lam x
  int rc = GDML_OK;
  hipError_t e;
  if (y) {
    e = hipMemcpyAsync(dy, y, n * 8, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(db, dy, n * 8, hipMemcpyDeviceToDevice, ctx->stream);
  } else {  // forward substitution already done by the factorisation: z is row n of the factor buffer
    e = hipMemcpyAsync(dy, ctx->d_rhs, n * 8, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(dz, ctx->K + n * ctx->K_ld, n * 8, hipMemcpyDeviceToDevice, ctx->stream);
  }
  if (e != hipSuccess) rc = gdml_fail(ctx, GDML_ERR_HIP, "copy: %s", hipGetErrorString(e));
  if (rc == GDML_OK) {
    phase_begin(ctx);
    rc = y ? chol_solve_device(ctx, ctx->K, n, ctx->K_ld, db, dz, dx)
           : chol_bwd_device(ctx, ctx->K, n, ctx->K_ld, dz, dx);
  }
  if (rc == GDML_OK && n_refine > 0) rc = operator_model_from_trainset(ctx, ctx->K_sig);
  for (int it = 0; rc == GDML_OK && it < n_refine; ++it) {
    // r = y - A x,  A x = -(K x - lam x)  =>  r = y + (K x - lam x)
    rc = matvec_device(ctx, ctx->K_lam, ctx->K_use_E, dx, n, dkv);
    if (rc != GDML_OK) break;
    hipLaunchKernelGGL(resid_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, dy, dkv, n, db);
    rc = chol_solve_device(ctx, ctx->K, n, ctx->K_ld, db, dz, dr);
    if (rc != GDML_OK) break;
    hipLaunchKernelGGL(axpy_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, dx, dr, n, 1.0);
  }
  if (rc == GDML_OK) {
    hipLaunchKernelGGL(scale_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, dx, n, -1.0);
    rc = phase_end(ctx, "solve");
  }
  if (rc == GDML_OK) {
    e = hipMemcpyAsync(alphas_out, dx, n * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = gdml_fail(ctx, GDML_ERR_HIP, "D2H: %s", hipGetErrorString(e));
  }
  int rc2 = ctx_free(ctx, buf);
  return rc != GDML_OK ? rc : rc2;
}
