// Posterior force covariance of a handful of geometries at low latency: the quantity of uncert.hip,
//   Sig_q = (-k_qq) - Z_q Z_q^T,   Z_q = (-Kx_q) L^-T,
// with a forward solve made for r = 3N B <= GDML_COV_FEW_ROWS right-hand-side rows against the resident n x n factor.  The
// cross-kernel, the descriptor kernel and the Gram step are those of uncert.hip / block_gram.hip, unchanged; only tall_trsm is
// replaced on this path.
//
// The solve is right-looking in steps of FEW_W = 256 columns, every launch ordered by the stream alone:
//   few_inv_kernel     once per call: inv(L_bb) of every 64 x 64 diagonal block b (the last one completed by an identity),
//                      forward substitution, one column per thread.  Nothing is cached across calls.
//   few_diag_kernel    per step, one workgroup per 16-row tile of X: the 16 x 256 panel lives in LDS; per 64-column sub-block jb
//                      X_jb <- X_jb inv(L_jb,jb)^T, then X_kb -= X_jb L[kb, jb]^T for the later sub-blocks of the step, all on
//                      v_mfma_f64_16x16x4_f64.  No serial sweep over columns anywhere.
//   few_update_kernel  per step, one workgroup per strip of 64 trailing columns c, for ALL r rows: X[:, c] -= X_step L[c, step]^T.
//                      A wavefront owns 16 columns (16 rows of L, read once, as whole 2 KB rows of the step's width) and every
//                      16-row tile of X in registers; the solved step reaches the four wavefronts through LDS.  L is read exactly
//                      once per call: n^2 / 2 * 8 bytes.
// Rows are padded with zero rows to a multiple of 64; a row tile runs the same MFMA sequence whatever else shares the call (the
// result row of an MFMA depends on its own row of the A operand only), all sums run over k ascending: a geometry's bits depend on
// n and 3N alone.  fp64 throughout, no atomics, no workgroup waits for another.
#include "common.h"

typedef double d4 __attribute__((ext_vector_type(4)));

#define FEW_W 256            // step width
#define FEW_P (FEW_W + 4)    // LDS pitch of the panel
#define FEW_ROWS GDML_COV_FEW_ROWS

struct FewArgs {
  const double* L;    // factor, lower triangle, pitch ld
  double* X;          // r_pad x ld rows, solved in place
  const double* inv;  // ceil(n / 64) inverted diagonal blocks, 64 x 64 row-major each
  int64_t ld, n, c0;  // c0: first column of the step
  int w;              // columns of the step inside the pitch (a multiple of 16)
};

__global__ void __launch_bounds__(64) few_inv_kernel(const double* __restrict__ L, int64_t ld, int64_t n, double* __restrict__ inv) {
  __shared__ double Ls[64 * 64];  // the block; row i is overwritten by row i of the inverse once it has been used
  const int j = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * 64;
  for (int i = 0; i < 64; ++i) {
    double v = i == j ? 1.0 : 0.0;
    if (b0 + i < n && b0 + j < n && j <= i) v = L[(b0 + i) * ld + b0 + j];
    Ls[i * 64 + j] = v;
  }
  __syncthreads();
  for (int i = 0; i < 64; ++i) {  // thread j: column j of the inverse (entries above the diagonal come out as exact zeros)
    double t = i == j ? 1.0 : 0.0;
    for (int k = 0; k < i; ++k) t -= Ls[i * 64 + k] * Ls[k * 64 + j];
    const double d = Ls[i * 64 + i];
    __syncthreads();
    Ls[i * 64 + j] = t / d;
    __syncthreads();
  }
  double* o = inv + (int64_t)blockIdx.x * 4096;
  for (int i = 0; i < 64; ++i) o[i * 64 + j] = Ls[i * 64 + j];
}

// f64 MFMA operands as in block_gram.hip: lane (li = lane & 15, lk = lane >> 4) feeds row / column li and k = 4 lk + step into
// MFMA step `step` on both sides; C/D: col = li, row = lk + 4 r.
// Everything this kernel reads of L and of the inverses does not depend on X, so all of it is requested before the first MFMA
// (16 + 24 d4 per lane; a step has only r / 16 workgroups, occupancy does not matter): the four sub-blocks then wait for LDS only.
// Tile slot (jb, s): the 16-column tile t = wave + 4 s right of sub-block jb, s < 3 - jb.
__global__ void __launch_bounds__(256) few_diag_kernel(FewArgs a) {
  __shared__ __attribute__((aligned(32))) double Xs[16 * FEW_P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int nsb = (a.w + 63) / 64;
  d4 binv[4][4], bl[6][4];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {  // (a sub-block past the step re-reads the first one: never used)
    const double* ib = a.inv + ((a.c0 >> 6) + (jb < nsb ? jb : 0)) * 4096 + (16 * wave + li) * 64 + 4 * lk;
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) binv[jb][kq] = *reinterpret_cast<const d4*>(ib + 16 * kq);
  }
#pragma unroll
  for (int jb = 0; jb < 3; ++jb)
#pragma unroll
    for (int s = 0; s < 3 - jb; ++s) {
      const int t = wave + 4 * s;
      const int64_t row = a.c0 + 64 * (jb + 1) + 16 * t + li;
      // rows of L past n: zero (their columns of X are pad columns and stay zero); a tile past the step reads the inverses instead
      const bool ok = t < (nsb - jb - 1) * 4 && row < a.n;
      const double* lb = ok ? a.L + row * a.ld + a.c0 + 64 * jb + 4 * lk : a.inv + li * 64 + 4 * lk;
#pragma unroll
      for (int kq = 0; kq < 4; ++kq) {
        const d4 v = *reinterpret_cast<const d4*>(lb + 16 * kq);
        bl[(jb == 0 ? 0 : jb == 1 ? 3 : 5) + s][kq] = ok ? -v : (d4){0.0, 0.0, 0.0, 0.0};
      }
    }
  __builtin_amdgcn_sched_barrier(0);
  double* const Xg = a.X + (int64_t)blockIdx.x * 16 * a.ld + a.c0;
  for (int e = tid; e < 16 * FEW_W; e += 256) {
    const int r = e / FEW_W, c = e % FEW_W;
    Xs[r * FEW_P + c] = c < a.w ? Xg[r * a.ld + c] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    if (jb < nsb) {  // (the same for the whole workgroup)
      const double* xa = Xs + li * FEW_P + 64 * jb + 4 * lk;
      {  // X_jb <- X_jb inv^T: wavefront `wave` owns 16 of the 64 columns
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) {
          const d4 av = *reinterpret_cast<const d4*>(xa + 16 * kq);
#pragma unroll
          for (int st = 0; st < 4; ++st) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], binv[jb][kq][st], acc, 0, 0, 0);
        }
        __syncthreads();  // everybody has read the old X_jb
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[(lk + 4 * r) * FEW_P + 64 * jb + 16 * wave + li] = acc[r];
        __syncthreads();
      }
#pragma unroll
      for (int s = 0; s < 3 - jb; ++s) {  // 16-column tiles right of sub-block jb, dealt round robin
        const int t = wave + 4 * s;
        if (t < (nsb - jb - 1) * 4) {
          const int cl = 64 * (jb + 1) + 16 * t;
          d4 acc;
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = Xs[(lk + 4 * r) * FEW_P + cl + li];
#pragma unroll
          for (int kq = 0; kq < 4; ++kq) {
            const d4 av = *reinterpret_cast<const d4*>(xa + 16 * kq);
#pragma unroll
            for (int st = 0; st < 4; ++st)
              acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], bl[(jb == 0 ? 0 : jb == 1 ? 3 : 5) + s][kq][st], acc, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) Xs[(lk + 4 * r) * FEW_P + cl + li] = acc[r];
        }
      }
      __syncthreads();
    }
  }
  for (int e = tid; e < 16 * FEW_W; e += 256) {
    const int r = e / FEW_W, c = e % FEW_W;
    if (c < a.w) Xg[r * a.ld + c] = Xs[r * FEW_P + c];
  }
}

// RT: 16-row tiles of X (r_pad / 16); KL: columns of the step per pass.  A pass stages the r_pad x KL piece of the solved step in
// LDS once per workgroup (every wavefront needs all of it: read per wavefront from L2 it was four times the traffic of L
// itself and the limit of the kernel), its rows of L are requested before the staging and go straight to registers.  The
// step's columns [c0, c0 + FEW_W) lie left of n whenever this kernel runs.
template <int RT, int KL>
__global__ void __launch_bounds__(256) few_update_kernel(FewArgs a) {
  constexpr int P = KL + 4;
  __shared__ __attribute__((aligned(32))) double As[16 * RT * P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t ct = a.c0 + FEW_W + (int64_t)blockIdx.x * 64 + 16 * wave;  // first of this wavefront's 16 columns
  const bool active = ct < a.n;  // (an idle wavefront of the last strip still stages and meets the barriers)
  const int64_t row = ct + li;
  const bool ok = active && row < a.n;
  const double* lb = a.L + (ok ? row : a.n - 1) * a.ld + a.c0 + 4 * lk;
  double* xc = a.X + (int64_t)lk * a.ld + ct + li;
  d4 acc[RT];
  if (active) {
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][r] = xc[(int64_t)(16 * i + 4 * r) * a.ld];
  }
  for (int kc = 0; kc < FEW_W; kc += KL) {
    d4 bv[KL / 16];
#pragma unroll
    for (int kk = 0; kk < KL / 16; ++kk) bv[kk] = *reinterpret_cast<const d4*>(lb + kc + 16 * kk);
    for (int e = tid; e < 16 * RT * (KL / 4); e += 256) {
      const int r = e / (KL / 4), q = e % (KL / 4);
      *reinterpret_cast<d4*>(As + r * P + 4 * q) = *reinterpret_cast<const d4*>(a.X + (int64_t)r * a.ld + a.c0 + kc + 4 * q);
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int kk = 0; kk < KL / 16; ++kk) {
        const d4 b = ok ? -bv[kk] : (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < RT; ++i) {
          const d4 av = *reinterpret_cast<const d4*>(As + (16 * i + li) * P + 16 * kk + 4 * lk);
#pragma unroll
          for (int st = 0; st < 4; ++st) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], b[st], acc[i], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // the piece is not read any more
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) xc[(int64_t)(16 * i + 4 * r) * a.ld] = acc[i][r];
  }
}

// X <- X L^-T for the r_pad (a multiple of 64, at most FEW_ROWS) rows of X against the resident factor; inv: ceil(n / 64) * 4096
// doubles of workspace (the solve of a CovPath)
static int few_solve(gdml_ctx* ctx, const GramSplit& g, double* X, int64_t r_pad, double work, double* inv) {
  const double* L = ctx->K;
  const int64_t n = g.n, ld = g.ld;
  const bool split = ctx_opt_i(ctx, "predict.cov_few_split_timers", 0) != 0;
  int slot = ktime_begin(ctx);
  hipLaunchKernelGGL(few_inv_kernel, dim3((unsigned)ceil_div(n, 64)), dim3(64), 0, ctx->stream, L, ld, n, inv);
  ctx->launch_counter++;
  ktime_end(ctx, slot, "few_inv", (double)n * 64.0 * 64.0 / 3.0);
  FewArgs a;
  a.L = L; a.X = X; a.inv = inv; a.ld = ld; a.n = n;
  const dim3 dgrid((unsigned)(r_pad / 16));
  if (!split) slot = ktime_begin(ctx);
  for (int64_t c0 = 0; c0 < n; c0 += FEW_W) {
    a.c0 = c0;
    a.w = (int)(ld - c0 < FEW_W ? ld - c0 : FEW_W);
    if (split) slot = ktime_begin(ctx);
    hipLaunchKernelGGL(few_diag_kernel, dgrid, dim3(256), 0, ctx->stream, a);
    ctx->launch_counter++;
    if (split) ktime_end(ctx, slot, "few_diag", (double)r_pad * a.w * a.w);
    if (c0 + FEW_W >= n) break;
    const dim3 ugrid((unsigned)ceil_div(n - c0 - FEW_W, 64));
    if (split) slot = ktime_begin(ctx);
    switch (r_pad / 64) {
      case 1: hipLaunchKernelGGL((few_update_kernel<4, 64>), ugrid, dim3(256), 0, ctx->stream, a); break;
      case 2: hipLaunchKernelGGL((few_update_kernel<8, 32>), ugrid, dim3(256), 0, ctx->stream, a); break;
      case 3: hipLaunchKernelGGL((few_update_kernel<12, 16>), ugrid, dim3(256), 0, ctx->stream, a); break;
      default: hipLaunchKernelGGL((few_update_kernel<16, 16>), ugrid, dim3(256), 0, ctx->stream, a); break;
    }
    ctx->launch_counter++;
    if (split) ktime_end(ctx, slot, "few_upd", 2.0 * (double)r_pad * FEW_W * (double)(n - c0 - FEW_W));
  }
  if (!split) ktime_end(ctx, slot, "few_solve", work);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? GDML_OK : gdml_fail(ctx, GDML_ERR_HIP, "few_solve launch: %s", hipGetErrorString(e));
}

static int few_common(gdml_ctx* ctx, const double* R, bool on_device, int64_t B, const double* lat, const double* lat_inv, int full,
                      double* cov_out) {
  static const CovPath path = {"few_cross", "few_solve", "few_gram", "uncert_few", 64, few_solve};
  GramSplit g;
  GDML_TRY(cov_check(ctx, "gdml_predict_cov_few", R, B, lat, lat_inv, cov_out, &g));
  if (B == 0) return GDML_OK;
  int limit = ctx_opt_i(ctx, "predict.cov_few_rows", FEW_ROWS);
  if (limit > FEW_ROWS) limit = FEW_ROWS;
  if (B * g.n3 > limit)  // the batched path itself, with its bits
    return on_device ? gdml_predict_cov_dev(ctx, R, B, lat, lat_inv, full, cov_out)
                     : gdml_predict_cov(ctx, R, B, lat, lat_inv, full, cov_out);
  return cov_run(ctx, g, path, R, on_device, B, lat, lat_inv, full, cov_out, (int64_t)ceil_div(g.n, 64) * 4096);
}

extern "C" int gdml_predict_cov_few(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv, int full,
                                    double* cov_out) {
  if (!ctx) return GDML_ERR_INVALID;
  return few_common(ctx, R, false, B, lat, lat_inv, full, cov_out);
}

extern "C" int gdml_predict_cov_few_dev(gdml_ctx* ctx, const double* R_dev, int64_t B, const double* lat, const double* lat_inv,
                                        int full, double* cov_dev) {
  if (!ctx) return GDML_ERR_INVALID;
  return few_common(ctx, R_dev, true, B, lat, lat_inv, full, cov_dev);
}
