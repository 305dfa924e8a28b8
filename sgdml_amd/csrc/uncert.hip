// Posterior force covariance of the Gaussian process behind an sGDML model (no counterpart in the reference, whose solve
// runs in SciPy on the host and discards the factor).
//
// Conventions: K is the un-negated matrix of gdml_assemble_K, A = -K + lam I = L L^T the factored system
// matrix resident in ctx->K (lower triangle, row-major, pitch K_ld), n = 3N M.  For a query geometry q
//   Kx_q  (3N x n)   cross-kernel rows: block j = the 3N x 3N block of train.py:97-232 for row point q (un-permuted) and
//                    column point j (permuted);  k_qq (3N x 3N) the same with i = j = q
//   Z_q   = (-Kx_q) L^-T                                   (tall_trsm of chol_solve.hip, right-looking: few rows, long factor)
//   Sig_q = (-k_qq) - Z_q Z_q^T                            (block_gram.hip + cov_reduce_kernel)
// in the units of the normalised labels; the host multiplies by std^2 (and its calibration factor).
//
// cross_rows_kernel, with x, g the descriptor / compressed Jacobian of q and X, G those of column point j, pi = pi_p,
// s(a, b) = -1 if a > b else +1 (the sign of atom a's entry in the Jacobian row of the pair {a, b}, desc.py:422-471):
//   d_p[AB]   = x[AB] - X[pi A, pi B]            n_p = sqrt5 |d_p|      b_p = 5 exp(-n_p / sig) / (3 sig^4)
//   w_p[A,:]  = sum_B s(A,B) g[AB,:] d_p[AB]                       (= J_q^T d_p)
//   u_p[piA,:]= sum_B s(piA,piB) G[piA piB,:] d_p[AB]              (= (J_j^p)^T d_p)
//   T_p[(A,.),(a,.)] = J_q^T J_j^p: for a = pi A   sum_B s(A,B) s(piA,piB) g[AB,:] (x) G[piA piB,:]   (N - 1 terms)
//                                   otherwise      s(A,B) s(a,piA) g[AB,:] (x) G[piA a,:],  B = pi^-1 a   (one term)
//   block = sum_p [ 5 b_p w_p (x) u_p - (sig^2 + sig n_p) b_p T_p ]
// One workgroup per (query, column point); the permutations go through LDS in groups (w, u, the diagonal blocks of T and
// the pair sums of |d|^2 per atom), every output element is summed over a group in registers by the one thread that owns it.
#include "common.h"

#define UC_LDS_DOUBLES 6000  // per workgroup of the cross kernel (48 KB: two workgroups per CU keep their LDS)

struct CrossArgs {
  const double* xq;     // (B,D)   query descriptors
  const double* gq;     // (B,D,3) query compressed Jacobians
  const double* xt;     // (M,D)   training descriptors
  const double* gt;     // (M,D,3)
  const int32_t* perm;  // (P,N)
  const int32_t* pinv;  // (P,N)
  double* rows;         // (B 3N) x ld: sgn * Kx, pad columns [n, ld) zeroed
  double* kqq;          // (B,3N,3N):   sgn * k_qq
  double* gws;          // per-workgroup workspace in global memory when a permutation's vectors do not fit LDS, else null
  int64_t ld, M, items;
  int B, N, D, P, PG, WS;
  double sig, sgn;
};

__global__ void __launch_bounds__(256) cross_rows_kernel(CrossArgs a) {
  extern __shared__ double uc_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, n3 = 3 * N, D = a.D;
  double* const ws = a.gws ? a.gws + (int64_t)blockIdx.x * a.WS : uc_lds;
  const double sq5 = 2.23606797749978969641;
  const double sig = a.sig, base_div = 3.0 * sig * sig * sig * sig;
  for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int q = (int)(item / (a.M + 1));
    const int64_t j = item - (int64_t)q * (a.M + 1);
    const bool self = j == a.M;
    const double* __restrict__ xq = a.xq + (int64_t)q * D;
    const double* __restrict__ gq = a.gq + (int64_t)q * D * 3;
    const double* __restrict__ xj = self ? xq : a.xt + j * D;
    const double* __restrict__ gj = self ? gq : a.gt + j * D * 3;
    double* const out = self ? a.kqq + (int64_t)q * n3 * n3 : a.rows + (int64_t)q * n3 * a.ld + j * n3;
    const int64_t out_ld = self ? n3 : a.ld;
    if (self) {  // pad columns of this query's rows (the solve and the Gram kernel read whole 16-column groups)
      const int64_t n = a.M * n3, npad = a.ld - n;
      for (int64_t e = tid; e < npad * n3; e += 256) a.rows[((int64_t)q * n3 + e / npad) * a.ld + n + e % npad] = 0.0;
      if (!a.kqq) continue;  // k_qq not asked for (the same for the whole workgroup)
    }
    for (int p0 = 0; p0 < a.P; p0 += a.PG) {
      const int pg = a.P - p0 < a.PG ? a.P - p0 : a.PG;
      __syncthreads();  // the previous group's (item's) vectors are no longer read
      // ---- per (permutation, row atom A): w_p[A], u_p[pi A], diagonal block of T_p, sum_B d_p[AB]^2
      for (int t = wave; t < pg * N; t += 4) {
        const int pl = t / N, A = t - pl * N;
        const int32_t* __restrict__ pi = a.perm + (int64_t)(p0 + pl) * N;
        const int piA = pi[A];
        double w0 = 0, w1 = 0, w2 = 0, u0 = 0, u1 = 0, u2 = 0, nn = 0;
        double t00 = 0, t01 = 0, t02 = 0, t10 = 0, t11 = 0, t12 = 0, t20 = 0, t21 = 0, t22 = 0;
        for (int Bq = lane; Bq < N; Bq += 64) {
          if (Bq == A) continue;
          const int piB = pi[Bq];
          const int kq = pair_idx(A, Bq), kj = pair_idx(piA, piB);
          const double d = xq[kq] - xj[kj];
          const double sa = A > Bq ? -1.0 : 1.0, sp = piA > piB ? -1.0 : 1.0;
          const double g0 = sa * gq[3 * kq], g1 = sa * gq[3 * kq + 1], g2 = sa * gq[3 * kq + 2];
          const double h0 = sp * gj[3 * kj], h1 = sp * gj[3 * kj + 1], h2 = sp * gj[3 * kj + 2];
          w0 += g0 * d; w1 += g1 * d; w2 += g2 * d;
          u0 += h0 * d; u1 += h1 * d; u2 += h2 * d;
          nn += d * d;
          t00 += g0 * h0; t01 += g0 * h1; t02 += g0 * h2;
          t10 += g1 * h0; t11 += g1 * h1; t12 += g1 * h2;
          t20 += g2 * h0; t21 += g2 * h1; t22 += g2 * h2;
        }
        w0 = wave_sum(w0); w1 = wave_sum(w1); w2 = wave_sum(w2);
        u0 = wave_sum(u0); u1 = wave_sum(u1); u2 = wave_sum(u2);
        nn = wave_sum(nn);
        t00 = wave_sum(t00); t01 = wave_sum(t01); t02 = wave_sum(t02);
        t10 = wave_sum(t10); t11 = wave_sum(t11); t12 = wave_sum(t12);
        t20 = wave_sum(t20); t21 = wave_sum(t21); t22 = wave_sum(t22);
        if (lane == 0) {
          double* v = ws + (int64_t)pl * a.WS;
          double* W = v + 3 * A;
          double* U = v + n3 + 3 * piA;
          double* T = v + 2 * n3 + 9 * A;
          W[0] = w0; W[1] = w1; W[2] = w2;
          U[0] = u0; U[1] = u1; U[2] = u2;
          T[0] = t00; T[1] = t01; T[2] = t02; T[3] = t10; T[4] = t11; T[5] = t12; T[6] = t20; T[7] = t21; T[8] = t22;
          v[15 * N + A] = nn;
        }
      }
      __syncthreads();
      // ---- per permutation: |d_p|^2 (every pair was counted from both of its atoms), the two coefficients
      for (int pl = wave; pl < pg; pl += 4) {
        double* v = ws + (int64_t)pl * a.WS;
        double s = 0.0;
        for (int A = lane; A < N; A += 64) s += v[15 * N + A];
        s = wave_sum(s);
        if (lane == 0) {
          const double nrm = sq5 * sqrt(0.5 * s);
          const double b = exp(-nrm / sig) / base_div * 5.0;
          v[16 * N] = 5.0 * b;
          v[16 * N + 1] = (sig * sig + sig * nrm) * b;
        }
      }
      __syncthreads();
      // ---- the block's elements, each summed over the group by its one owner
      for (int e = tid; e < n3 * n3; e += 256) {
        const int r = e / n3, c = e - r * n3;
        const int A = r / 3, ax = r - 3 * A, ac = c / 3, axc = c - 3 * ac;
        double acc = 0.0;
        for (int pl = 0; pl < pg; ++pl) {
          const double* v = ws + (int64_t)pl * a.WS;
          const int64_t po = (int64_t)(p0 + pl) * N;
          const int piA = a.perm[po + A];
          double t;
          if (ac == piA) {
            t = v[2 * n3 + 9 * A + 3 * ax + axc];
          } else {
            const int Bq = a.pinv[po + ac];
            const double sa = A > Bq ? -1.0 : 1.0, sp = ac > piA ? -1.0 : 1.0;
            t = sa * gq[3 * pair_idx(A, Bq) + ax] * (sp * gj[3 * pair_idx(piA, ac) + axc]);
          }
          acc += v[16 * N] * v[r] * v[n3 + c] - v[16 * N + 1] * t;
        }
        double* o = out + (int64_t)r * out_ld + c;
        *o = p0 == 0 ? a.sgn * acc : *o + a.sgn * acc;
      }
    }
  }
}

// sgn * Kx of bc device-resident queries against the M column points (xt, gt) into `rows` (pitch ld) and sgn * k_qq into
// `kqq` (null: k_qq is not computed, the item only zeroes the pad columns); permutations and molecule size are those of the resident training set, the launch is timed as `tname`
int cross_rows_launch(gdml_ctx* ctx, const double* xt, const double* gt, int64_t M, const double* xq, const double* gq, int bc,
                      double* rows, int64_t ld, double* kqq, double sgn, double sig, const char* tname) {
  const TrainSet& ts = ctx->ts;
  CrossArgs a;
  a.xq = xq; a.gq = gq; a.xt = xt; a.gt = gt; a.perm = ts.perm; a.pinv = ts.pinv;
  a.rows = rows; a.kqq = kqq; a.gws = nullptr;
  a.ld = ld; a.M = M; a.items = (int64_t)bc * (M + 1);
  a.B = bc; a.N = ts.N; a.D = ts.D; a.P = ts.P;
  a.WS = 16 * ts.N + 2;
  a.sig = sig; a.sgn = sgn;
  const bool in_lds = a.WS <= UC_LDS_DOUBLES && !ctx_opt_i(ctx, "predict.cov_global", 0);
  a.PG = in_lds ? UC_LDS_DOUBLES / a.WS : 1;
  if (a.PG > ts.P) a.PG = ts.P;
  int64_t grid = a.items;
  size_t lds = 0;
  if (in_lds) {
    lds = (size_t)a.PG * a.WS * 8;
    if (grid > ((int64_t)1 << 22)) grid = (int64_t)1 << 22;
  } else {  // a few resident workgroups per CU walk the items: the workspace stays small
    if (grid > 4 * (int64_t)ctx->num_cus) grid = 4 * (int64_t)ctx->num_cus;
    void* p = nullptr;
    GDML_TRY(ctx_alloc(ctx, &p, grid * a.WS * 8));
    a.gws = (double*)p;
  }
  const int slot = ktime_begin(ctx);
  hipLaunchKernelGGL(cross_rows_kernel, dim3((unsigned)grid), dim3(256), lds, ctx->stream, a);
  ctx->launch_counter++;
  // algorithmic work: bytes written
  ktime_end(ctx, slot, tname, (double)bc * (double)(M + (kqq ? 1 : 0)) * 9.0 * ts.N * (double)ts.N * 8.0);
  hipError_t e = hipGetLastError();
  int rc = e == hipSuccess ? GDML_OK : gdml_fail(ctx, GDML_ERR_HIP, "cross_rows launch: %s", hipGetErrorString(e));
  if (a.gws) {
    const int rc2 = ctx_free(ctx, a.gws);  // (synchronises the stream first)
    if (rc == GDML_OK) rc = rc2;
  }
  return rc;
}

// ---- Gram step ---------------------------------------------------------------------------------------------------------
// Sig_q = (-k_qq) - Z_q Z_q^T: the partial tiles of Z_q Z_q^T come from block_gram_launch (block_gram.hip; a query's rows have
// no zero prefix, so first = 0), cov_reduce_kernel sums them in the order s = 0 .. S - 1.  The diag_only form runs the same
// MFMA sequence for the diagonal tiles, so the marginal variances equal the diagonal of the full covariance bit for bit.
// out = sym(-k_qq) - sum_s partial_s (fixed order).  Full form: both triangles from the lower block pairs; diag_only: (B,3N).
__global__ void __launch_bounds__(256) cov_reduce_kernel(const double* __restrict__ part, const double* __restrict__ nkqq,
                                                         double* __restrict__ out, int n3, int nblk, int npairs, int S,
                                                         int full, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  if (full) {
    const int64_t q = t / ((int64_t)n3 * n3);
    const int e = (int)(t - q * n3 * n3), r = e / n3, c = e - r * n3;
    const int rr = r > c ? r : c, cc = r > c ? c : r;
    const int I = rr >> 6, J = cc >> 6;
    const double* p = part + ((q * npairs + I * (I + 1) / 2 + J) * S) * 4096 + (rr & 63) * 64 + (cc & 63);
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += p[(int64_t)s * 4096];
    const double* k = nkqq + q * n3 * n3;
    out[t] = 0.5 * (k[rr * n3 + cc] + k[cc * n3 + rr]) - acc;
  } else {
    const int64_t q = t / n3;
    const int r = (int)(t - q * n3);
    const double* p = part + ((q * nblk + (r >> 6)) * S) * 64 + (r & 63);
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += p[(int64_t)s * 64];
    const double kd = nkqq[q * n3 * n3 + (int64_t)r * n3 + r];
    out[t] = 0.5 * (kd + kd) - acc;
  }
}

// the reduce for `items` row blocks (one launch, not timed): out (items,3N,3N) with full, else (items,3N)
void cov_reduce_launch(gdml_ctx* ctx, const GramSplit& g, const double* part, const double* nkqq, double* out, int64_t items,
                       int full) {
  const int64_t total = items * (full ? (int64_t)g.n3 * g.n3 : (int64_t)g.n3);
  hipLaunchKernelGGL(cov_reduce_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, part, nkqq, out, g.n3,
                     g.nblk, g.npairs, g.S, full, total);
  ctx->launch_counter++;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int uncert_check_queries(gdml_ctx* ctx, const char* who, const double* R, int64_t B, const double* lat,
                                const double* lat_inv) {
  if (!R) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: R is NULL", who);
  if (B < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: B < 0", who);
  if ((lat == nullptr) != (lat_inv == nullptr))
    return gdml_fail(ctx, GDML_ERR_INVALID, "lattice and inverse must both be given or both NULL");
  return GDML_OK;
}

// Work buffers of one batch chunk
int64_t cov_chunk_doubles(const GramSplit& g, int64_t D, bool gram) {
  const int64_t n3 = g.n3;
  return n3 + 4 * D + 2 * n3 * n3 + (gram ? (int64_t)g.npairs * g.S * 4096 : 0);
}

double* cov_chunk_carve(CovChunk* c, double* ws, const GramSplit& g, int64_t D, int64_t bc, bool gram) {
  const int64_t n3 = g.n3;
  c->R = ws;
  c->xq = c->R + bc * n3;
  c->gq = c->xq + bc * D;
  c->nkqq = c->gq + 3 * bc * D;
  c->out = c->nkqq + bc * n3 * n3;
  c->part = c->out + bc * n3 * n3;
  return c->part + (gram ? bc * (int64_t)g.npairs * g.S * 4096 : 0);
}

extern "C" int gdml_uncert_prepare(gdml_ctx* ctx, double sig, double lam, int* info) {
  if (!ctx) return GDML_ERR_INVALID;
  if (info) *info = 0;
  if (!ctx->ts.x) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_uncert_prepare: call gdml_train_upload first");
  if (comm_active(ctx) && ctx->world > 1)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "gdml_uncert_prepare: the factor of a multi-rank context is distributed");
  ctx->uncert_ready = false;
  GDML_TRY(gdml_assemble_A(ctx, sig, lam, 0, 0));
  GDML_TRY(gdml_chol_factor(ctx, lam, info));
  ctx->uncert_ready = true;
  return GDML_OK;
}

extern "C" int gdml_uncert_release(gdml_ctx* ctx) {
  if (!ctx) return GDML_ERR_INVALID;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ctx->uncert_ready = false;
  GDML_TRY(ctx_slot_release(ctx, SLOT_GRAM_WS));
  GDML_TRY(ctx_slot_release(ctx, SLOT_GRAM_ROWS));
  if (ctx->K) {
    GDML_TRY(ctx_free(ctx, ctx->K));
    ctx->K = nullptr;
    ctx->K_bytes = 0;
    ctx->K_rows = ctx->K_cols = ctx->K_extra = ctx->K_ld = 0;
    ctx->K_factored = false;
    ctx->K_rhs_row = false;
    ctx->precon = nullptr;
    precon_release_aux(ctx);
  }
  return GDML_OK;
}

extern "C" int gdml_uncert_cross(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv,
                                 double* Kx_out, double* kqq_out) {
  if (!ctx) return GDML_ERR_INVALID;
  GDML_TRY(uncert_check_queries(ctx, "gdml_uncert_cross", R, B, lat, lat_inv));
  if (!ctx->ts.x) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_uncert_cross: call gdml_train_upload first");
  if (ctx->K_sig <= 0 && !(ctx->model.sig > 0))
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_uncert_cross: no length scale known (gdml_uncert_prepare or a model upload sets it)");
  if (B == 0) return GDML_OK;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const double sig = ctx->uncert_ready || ctx->K_sig > 0 ? ctx->K_sig : ctx->model.sig;
  const TrainSet& ts = ctx->ts;
  const GramSplit g = gram_split(ts.M * 3 * ts.N, 3 * ts.N);
  const int64_t n3 = g.n3, n = g.n, ld = g.ld;
  int64_t bc_max;
  double *rows, *ws;
  GDML_TRY(gram_workspace(ctx, g, "predict.cov_chunk", B, cov_chunk_doubles(g, ts.D, false), 0, &bc_max, &rows, &ws));
  CovChunk p;
  cov_chunk_carve(&p, ws, g, ts.D, bc_max, false);
  for (int64_t b0 = 0; b0 < B; b0 += bc_max) {
    const int bc = (int)(B - b0 < bc_max ? B - b0 : bc_max);
    HIP_CHECK(ctx, hipMemcpyAsync(p.R, R + b0 * n3, bc * n3 * 8, hipMemcpyHostToDevice, ctx->stream));
    GDML_TRY(desc_device(ctx, p.R, bc, ts.N, lat, lat_inv, p.xq, p.gq));
    GDML_TRY(cross_rows_launch(ctx, ts.x, ts.g, ts.M, p.xq, p.gq, bc, rows, ld, p.nkqq, 1.0, sig, "uncert_cross"));
    if (Kx_out)
      HIP_CHECK(ctx, hipMemcpy2DAsync(Kx_out + b0 * n3 * n, n * 8, rows, ld * 8, n * 8, bc * n3,
                                      hipMemcpyDeviceToHost, ctx->stream));
    if (kqq_out)
      HIP_CHECK(ctx, hipMemcpyAsync(kqq_out + b0 * n3 * n3, p.nkqq, bc * n3 * n3 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GDML_OK;
}

int cov_chunk_step(gdml_ctx* ctx, const GramSplit& g, const CovPath& path, const CovChunk& c, double* rows, double* fixed,
                   const double* R, bool R_on_device, int bc, const double* lat, const double* lat_inv, int full, double* d_out) {
  const TrainSet& ts = ctx->ts;
  const int64_t n3 = g.n3;
  if (!R_on_device) {
    HIP_CHECK(ctx, hipMemcpyAsync(c.R, R, bc * n3 * 8, hipMemcpyHostToDevice, ctx->stream));
    R = c.R;
  }
  GDML_TRY(desc_device(ctx, R, bc, ts.N, lat, lat_inv, c.xq, c.gq));
  GDML_TRY(cross_rows_launch(ctx, ts.x, ts.g, ts.M, c.xq, c.gq, bc, rows, g.ld, c.nkqq, -1.0, ctx->K_sig, path.t_cross));
  // Z = (-Kx) L^-T on whole row tiles (the row buffer holds whole 128-row tiles)
  const int64_t r = (int64_t)bc * n3, r_pad = (r + path.row_pad - 1) / path.row_pad * path.row_pad;
  if (r_pad > r) HIP_CHECK(ctx, hipMemsetAsync(rows + r * g.ld, 0, (r_pad - r) * g.ld * 8, ctx->stream));
  const double work = (double)g.n * (double)g.n * (double)r;
  if (path.solve) {
    GDML_TRY(path.solve(ctx, g, rows, r_pad, work, fixed));
  } else {
    // Right-looking: the rows are few and the factor is long, so every 512-column step updates the whole remaining width in
    // one launch that fills the chip (the left-looking form of the Nystroem build would run 4 tiles deep products per 128 rows)
    const int slot = ktime_begin(ctx);
    GDML_TRY(tall_trsm(ctx, ctx->K, rows, r_pad, g.n, g.ld, 0));
    ktime_end(ctx, slot, path.t_solve, work);
  }
  const int slot = ktime_begin(ctx);
  block_gram_launch(ctx, g, rows, c.part, bc, !full, 0, 0);
  cov_reduce_launch(ctx, g, c.part, c.nkqq, d_out, bc, full);
  ktime_end(ctx, slot, path.t_gram, 2.0 * (double)g.ld * (full ? (double)n3 * n3 : (double)n3) * bc);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? GDML_OK : gdml_fail(ctx, GDML_ERR_HIP, "cov_gram launch: %s", hipGetErrorString(e));
}

int cov_check(gdml_ctx* ctx, const char* who, const double* R, int64_t B, const double* lat, const double* lat_inv,
              const double* cov_out, GramSplit* g_out) {
  GDML_TRY(uncert_check_queries(ctx, who, R, B, lat, lat_inv));
  if (!cov_out) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: cov_out is NULL", who);
  return resident_factor_check(ctx, who, true, g_out);
}

int cov_run(gdml_ctx* ctx, const GramSplit& g, const CovPath& path, const double* R, bool on_device, int64_t B, const double* lat,
            const double* lat_inv, int full, double* cov_out, int64_t ws_fixed) {
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t n3 = g.n3, D = ctx->ts.D, per_out = full ? n3 * n3 : n3;
  int64_t bc_max;
  double *rows, *ws;
  GDML_TRY(gram_workspace(ctx, g, "predict.cov_chunk", B, cov_chunk_doubles(g, D, true), ws_fixed, &bc_max, &rows, &ws));
  CovChunk c;
  cov_chunk_carve(&c, ws + ws_fixed, g, D, bc_max, true);
  phase_begin(ctx);
  for (int64_t b0 = 0; b0 < B; b0 += bc_max) {
    const int bc = (int)(B - b0 < bc_max ? B - b0 : bc_max);
    double* d_out = on_device ? cov_out + b0 * per_out : c.out;
    GDML_TRY(cov_chunk_step(ctx, g, path, c, rows, ws, R + b0 * n3, on_device, bc, lat, lat_inv, full, d_out));
    if (!on_device) {
      HIP_CHECK(ctx, hipMemcpyAsync(cov_out + b0 * per_out, c.out, bc * per_out * 8, hipMemcpyDeviceToHost, ctx->stream));
      HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  return phase_end(ctx, path.phase);
}

static int cov_common(gdml_ctx* ctx, const double* R, bool on_device, int64_t B, const double* lat, const double* lat_inv,
                      int full, double* cov_out) {
  static const CovPath path = {"uncert_cross", "uncert_solve", "uncert_gram", "uncert", 128, nullptr};
  GramSplit g;
  GDML_TRY(cov_check(ctx, "gdml_predict_cov", R, B, lat, lat_inv, cov_out, &g));
  if (B == 0) return GDML_OK;
  return cov_run(ctx, g, path, R, on_device, B, lat, lat_inv, full, cov_out);
}

extern "C" int gdml_predict_cov(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv, int full,
                                double* cov_out) {
  if (!ctx) return GDML_ERR_INVALID;
  return cov_common(ctx, R, false, B, lat, lat_inv, full, cov_out);
}

extern "C" int gdml_predict_cov_dev(gdml_ctx* ctx, const double* R_dev, int64_t B, const double* lat, const double* lat_inv,
                                    int full, double* cov_dev) {
  if (!ctx) return GDML_ERR_INVALID;
  return cov_common(ctx, R_dev, true, B, lat, lat_inv, full, cov_dev);
}
