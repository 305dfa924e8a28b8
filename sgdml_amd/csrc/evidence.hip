// Gradient of the model evidence in sig and lam from the resident Cholesky factor (no counterpart in the reference, which
// picks sig from a grid by validation error and never tunes lam).
//
// Conventions: A = -K + lam I = L L^T resident in ctx->K (lower triangle, row-major, pitch K_ld), n = 3N M,
// a = A^-1 y = -alphas, K' = dK/dsig at the factor's own sig.  The entry returns the five sums
//   tr A^-1,   <A^-1, K'> = sum_ij (A^-1)_ij K'_ij,   a^T K' a,   a^T a,   log det A
// from which the caller forms d lml / d sig = 1/2 (<A^-1, K'> - a^T K' a / s^2), d lml / d lam = 1/2 (a^T a / s^2 - tr A^-1).
//
// Three passes, interleaved chunk by chunk over consecutive training points (rows r0 .. r1 of the system):
//   1. Z = L^-T, KEPT: the chunk's rows are seeded and solved by factor_inverse_rows, the step of loo.hip (trailing sub-problem
//      from c0 = the chunk's first column rounded down to the 512-column panel grid, right-looking tall_trsm on whole 128-row
//      tiles) in the chunk row buffer, and the TRUE rows (not the pad rows behind them) are copied into a second n x K_ld
//      buffer that lives for the call.  Row r of Z is zero left of column r; columns left of c0 are never written and never read.
//   2. -A^-1[r0:r1, 0:r1] = -Z[r0:r1, c0:] Z[0:r1, c0:]^T: one launch_gemm_nt_neg into the chunk row buffer.  Rows above the
//      chunk are zero left of their own diagonal, so the product over k >= c0 is exact without a mask.
//   3. evidence_contract_kernel: every lower pair of points (i in the chunk, j <= i) contracts its 3N x 3N tile of -A^-1 with
//      the block K'_ij, which is evaluated on the fly from ts.x, ts.g, ts.tp and never stored.
// No atomics: a partial per pair, a fixed-order sum per row point on the device and a sum over the points in index order on
// the host.  The sums stay apart down to the host (tr A^-1 is of order 1 / lam where the others are of order 10).
#include "common.h"

// ---- contraction ---------------------------------------------------------------------------------------------------------
// For one pair of points (i, j), one permutation p, d = x_i - P_p x_j, r = sqrt(5) |d|, e = exp(-r / sig) the block of K is
//   J_i^T [ f1 d d^T - f2 I ] J_j^p,   f1 = 25 e / (3 sig^4),  f2 = 5 e (sig + r) / (3 sig^3)       (train.py:97-232)
// and that of K' = dK/dsig has f1' = f1 (r - 4 sig) / sig^2, f2' = 5 e (r^2 - 2 sig r - 2 sig^2) / (3 sig^5) in their place.
// With W the pair's tile, u = J_i^T d, v = (J_j^p)^T d:
//   <W, K'_ij>    = sum_p [ f1' u^T W v - f2' sum_q J_i[q,:] W J_j^p[q,:]^T ]
//   a_i^T K'_ij a_j = sum_p [ f1' (d . J_i a_i) (d . J_j^p a_j) - f2' (J_i a_i) . (J_j^p a_j) ]
// Row q of J_i has six non-zeros (compressed Jacobian g: +g[q] at the pair's lower atom, -g[q] at its higher one), so the
// inner sum of the first line is 36 products per descriptor row and permutation.
// One workgroup walks pairs t = blockIdx.x, blockIdx.x + gridDim.x, ... of the chunk; what it writes for a pair does not
// depend on which workgroup got it.  Per permutation: (a) every thread takes descriptor rows q = tid, tid + 256, ...: d[q]
// into dd[q] and dj[tp[q]] (tp is a permutation: no two rows meet), its share of |d|^2 and of the three sums of the second
// line, and its share of the 36-product sum; (b) f1', f2' from the workgroup's |d|^2, then u and v, one component per thread;
// (c) u^T W v over the tile's elements.  TILE_LDS: the tile is staged in LDS (pitch gp, odd); else it is walked in global
// memory (3N > 128: L2 serves the re-reads).  VEC_LDS: the per-pair vectors live in LDS; else in a global slot per workgroup
// (descriptors beyond LDS; option chol.evidence_global forces it for tests).
struct EvidArgs {
  const double* W;       // rows of -A^-1 of the chunk: row (i - j0) 3N + r, column 3N j + c, pitch ld
  const double* x;       // (M,D)
  const double* g;       // (M,D,3)
  const int32_t* tp;     // (P,D)
  const double* alphas;  // (n): a^T K' a is even in a, so the library's sign is used as it is
  double* gscr;          // !VEC_LDS: [workgroup][vlen]
  double* out;           // [(i - j0) (j0 + bc) + j][3]: <W, K'_ij>, a_i^T K'_ij a_j, tr W (i = j only)
  int64_t ld, j0, bc, vlen;
  int N, D, P, n3, gp;
  double sig;
};

// (hi, lo), hi > lo, of descriptor row q = hi (hi - 1) / 2 + lo
__device__ __forceinline__ void evid_pair(int q, int& hi, int& lo) {
  int h = (int)((1.0 + sqrt(8.0 * (double)q + 1.0)) * 0.5);
  while (h * (h - 1) / 2 > q) --h;
  while ((h + 1) * h / 2 <= q) ++h;
  hi = h;
  lo = q - h * (h - 1) / 2;
}

// sum over the workgroup in the order wave 0 .. 3 of the waves' butterfly sums; the same value in every thread
__device__ __forceinline__ double evid_block_sum(double v, double* red, int tid) {
  v = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

template <bool TILE_LDS, bool VEC_LDS>
__global__ void __launch_bounds__(256) evidence_contract_kernel(EvidArgs A) {
  extern __shared__ double evid_lds[];
  const int tid = threadIdx.x, N = A.N, D = A.D, n3 = A.n3;
  double* const vec = VEC_LDS ? evid_lds : A.gscr + (int64_t)blockIdx.x * A.vlen;
  double* const dd = vec;            // D     d[q]
  double* const dj = dd + D;         // D     d[q] at row tp[q]: d against the rows of J_j
  double* const u = dj + D;          // 3N
  double* const v = u + n3;          // 3N
  double* const ai = v + n3;         // 3N
  double* const aj = ai + n3;        // 3N
  double* const red = aj + n3;       // 16 + 4
  double* const Wl = evid_lds + (VEC_LDS ? A.vlen : 0);
  const int64_t cols = A.j0 + A.bc, items = A.bc * cols;
  const double sig = A.sig, sqrt5 = 2.23606797749978969641;
  const double c1 = 25.0 / (3.0 * sig * sig * sig * sig), c2 = 5.0 / (3.0 * sig * sig * sig * sig * sig);
  for (int64_t t = blockIdx.x; t < items; t += gridDim.x) {
    const int64_t il = t / cols, j = t - il * cols, i = A.j0 + il;
    if (j > i) continue;  // the same in every thread
    const double* const Wg = A.W + il * n3 * A.ld + j * n3;
    const double* W;
    int64_t wp;
    if (TILE_LDS) {
      for (int e = tid; e < n3 * n3; e += 256) {
        const int r = e / n3, c = e - r * n3;
        Wl[r * A.gp + c] = Wg[(int64_t)r * A.ld + c];
      }
      W = Wl;
      wp = A.gp;
    } else {
      W = Wg;
      wp = A.ld;
    }
    for (int k = tid; k < n3; k += 256) {
      ai[k] = A.alphas[i * n3 + k];
      aj[k] = A.alphas[j * n3 + k];
    }
    const double* const xi = A.x + i * D;
    const double* const xj = A.x + j * D;
    const double* const gi = A.g + i * 3 * (int64_t)D;
    const double* const gj = A.g + j * 3 * (int64_t)D;
    double acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    __syncthreads();
    for (int p = 0; p < A.P; ++p) {
      const int32_t* const tp = A.tp + (int64_t)p * D;
      // (a)
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, t2 = 0.0;
      for (int q = tid; q < D; q += 256) {
        const int qj = tp[q];
        int hi, lo, hj, lj;
        evid_pair(q, hi, lo);
        evid_pair(qj, hj, lj);
        const double d = xi[q] - xj[qj];
        dd[q] = d;
        dj[qj] = d;
        s0 = __builtin_fma(d, d, s0);
        const double g0 = gi[3 * q], g1 = gi[3 * q + 1], g2 = gi[3 * q + 2];
        const double h0 = gj[3 * qj], h1 = gj[3 * qj + 1], h2 = gj[3 * qj + 2];
        const double jai = g0 * (ai[3 * lo] - ai[3 * hi]) + g1 * (ai[3 * lo + 1] - ai[3 * hi + 1]) + g2 * (ai[3 * lo + 2] - ai[3 * hi + 2]);
        const double jaj = h0 * (aj[3 * lj] - aj[3 * hj]) + h1 * (aj[3 * lj + 1] - aj[3 * hj + 1]) + h2 * (aj[3 * lj + 2] - aj[3 * hj + 2]);
        s1 = __builtin_fma(d, jai, s1);
        s2 = __builtin_fma(d, jaj, s2);
        s3 = __builtin_fma(jai, jaj, s3);
        const double* const wl = W + 3 * lo * wp;
        const double* const wh = W + 3 * hi * wp;
        double c = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double gr = r == 0 ? g0 : r == 1 ? g1 : g2;
          const double* const pl = wl + r * wp;
          const double* const ph = wh + r * wp;
          double rs = 0.0;
#pragma unroll
          for (int cc = 0; cc < 3; ++cc) {
            const double hc = cc == 0 ? h0 : cc == 1 ? h1 : h2;
            rs = __builtin_fma(hc, (pl[3 * lj + cc] - pl[3 * hj + cc]) - (ph[3 * lj + cc] - ph[3 * hj + cc]), rs);
          }
          c = __builtin_fma(gr, rs, c);
        }
        t2 += c;
      }
      s0 = wave_sum(s0);
      s1 = wave_sum(s1);
      s2 = wave_sum(s2);
      s3 = wave_sum(s3);
      if ((tid & 63) == 0) {
        const int w = tid >> 6;
        red[w] = s0;
        red[4 + w] = s1;
        red[8 + w] = s2;
        red[12 + w] = s3;
      }
      __syncthreads();
      // (b)
      const double nrm2 = ((red[0] + red[1]) + red[2]) + red[3];
      const double S1 = ((red[4] + red[5]) + red[6]) + red[7];
      const double S2 = ((red[8] + red[9]) + red[10]) + red[11];
      const double S3 = ((red[12] + red[13]) + red[14]) + red[15];
      const double r = sqrt5 * sqrt(nrm2);
      const double ex = exp(-r / sig);
      const double f1p = c1 * ex * (r - 4.0 * sig) / (sig * sig);
      const double f2p = c2 * ex * (r * r - 2.0 * sig * r - 2.0 * sig * sig);
      acc2 = __builtin_fma(f2p, t2, acc2);
      if (tid == 0) acc3 += f1p * S1 * S2 - f2p * S3;
      for (int k = tid; k < 2 * n3; k += 256) {
        const int which = k >= n3, comp = which ? k - n3 : k;
        const int a = comp / 3, c = comp - 3 * a;
        const double* const gs = which ? gj : gi;
        const double* const ds = which ? dj : dd;
        double s = 0.0;
        for (int b = 0; b < N; ++b) {
          if (b == a) continue;
          const int q = pair_idx(a, b);
          const double gv = gs[3 * q + c];
          s = __builtin_fma(ds[q], a < b ? gv : -gv, s);
        }
        (which ? v : u)[comp] = s;
      }
      __syncthreads();
      // (c)
      double t1 = 0.0;
      for (int e = tid; e < n3 * n3; e += 256) {
        const int rr = e / n3, cc = e - rr * n3;
        t1 = __builtin_fma(u[rr] * v[cc], W[rr * wp + cc], t1);
      }
      acc1 = __builtin_fma(f1p, t1, acc1);
    }
    double tr = 0.0;
    if (i == j)
      for (int k = tid; k < n3; k += 256) tr += W[k * wp + k];
    const double T1 = evid_block_sum(acc1, red + 16, tid);
    const double T2 = evid_block_sum(acc2, red + 16, tid);
    const double TR = evid_block_sum(tr, red + 16, tid);
    if (tid == 0) {
      double* const o = A.out + t * 3;
      o[0] = T1 - T2;
      o[1] = acc3;
      o[2] = TR;
    }
  }
}

// per row point of the chunk: the pairs j = 0 .. i in index order, off-diagonal pairs twice (A^-1 and K' are symmetric)
__global__ void __launch_bounds__(64) evidence_rowsum_kernel(const double* __restrict__ out, double* __restrict__ pts, int64_t j0, int64_t bc) {
  const int64_t il = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (il >= bc) return;
  const int64_t cols = j0 + bc, i = j0 + il;
  const double* o = out + il * cols * 3;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t j = 0; j < i; ++j) {
    s0 += o[3 * j];
    s1 += o[3 * j + 1];
  }
  pts[3 * i] = 2.0 * s0 + o[3 * i];
  pts[3 * i + 1] = 2.0 * s1 + o[3 * i + 1];
  pts[3 * i + 2] = o[3 * i + 2];
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static int evidence_run(gdml_ctx* ctx, const GramSplit& g, double* Z, const double* alphas, double* terms_out) {
  const TrainSet& ts = ctx->ts;
  const int64_t M = ts.M, n3 = g.n3, n = g.n, ld = g.ld;
  const int D = ts.D;
  hipStream_t st = ctx->stream;
  // where the tile and the per-pair vectors live
  const int gp = (int)n3 | 1;
  const int64_t vlen = 2 * (int64_t)D + 4 * n3 + 32, tile = n3 * gp;
  int lds_max = 0;
  if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess || lds_max < 64 * 1024)
    lds_max = 64 * 1024;
  const bool vec_lds = vlen * 8 <= lds_max && ctx_opt_i(ctx, "chol.evidence_global", 0) == 0;
  const bool tile_lds = vec_lds && (vlen + tile) * 8 <= lds_max;
  const size_t lds_bytes = (size_t)((vec_lds ? vlen : 0) + (tile_lds ? tile : 0)) * 8;
  const int64_t grid_max = (int64_t)ctx->num_cus * 4;
  // work buffers: per point of a chunk its pair partials; fixed: coefficients, diag L, per-point sums, the vector slots
  const int64_t fixed = 2 * n + 3 * M + (vec_lds ? 0 : grid_max * vlen) + 16;
  int64_t bc_max;
  double *rows, *ws;
  GDML_TRY(gram_workspace(ctx, g, "chol.evidence_chunk", M, 3 * M, fixed, &bc_max, &rows, &ws));
  double* const d_alphas = ws;
  double* const d_diag = d_alphas + n;
  double* const d_pts = d_diag + n;
  double* const d_gscr = d_pts + 3 * M;
  double* const d_out = d_gscr + (vec_lds ? 0 : grid_max * vlen);
  HIP_CHECK(ctx, hipMemcpyAsync(d_alphas, alphas, n * 8, hipMemcpyHostToDevice, st));
  if (lds_bytes > 64 * 1024) {
    if (tile_lds)
      HIP_CHECK(ctx, hipFuncSetAttribute((const void*)evidence_contract_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    else
      HIP_CHECK(ctx, hipFuncSetAttribute((const void*)evidence_contract_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  }
  EvidArgs a;
  a.x = ts.x; a.g = ts.g; a.tp = ts.tp; a.alphas = d_alphas; a.gscr = d_gscr; a.out = d_out; a.W = rows;
  a.ld = ld; a.vlen = vlen; a.N = ts.N; a.D = D; a.P = ts.P; a.n3 = (int)n3; a.gp = gp; a.sig = ctx->K_sig;
  phase_begin(ctx);
  for (int64_t j0 = 0; j0 < M; j0 += bc_max) {
    const int64_t bc = M - j0 < bc_max ? M - j0 : bc_max;
    const int64_t nrows = bc * n3, first = j0 * n3, c0 = first / 512 * 512, r1 = first + nrows;
    // pass 1: seed and solve in the chunk buffer, and keep the true rows
    GDML_TRY(factor_inverse_rows(ctx, g, rows, j0, bc, "evidence_seed", "evidence_solve", Z));
    // pass 2: rows of -A^-1 up to the chunk's own diagonal blocks, over the chunk buffer
    int slot = ktime_begin(ctx);
    GDML_TRY(launch_gemm_nt_neg(ctx, st, Z + first * ld + c0, ld, Z + c0, ld, rows, ld, nrows, r1, ld - c0));
    ktime_end(ctx, slot, "evidence_inv", 2.0 * (double)nrows * (double)r1 * (double)(ld - c0));
    // pass 3
    a.j0 = j0; a.bc = bc;
    const int64_t items = bc * (j0 + bc);
    const dim3 grid((unsigned)(items < grid_max ? items : grid_max));
    slot = ktime_begin(ctx);
    if (tile_lds)
      hipLaunchKernelGGL((evidence_contract_kernel<true, true>), grid, dim3(256), lds_bytes, st, a);
    else if (vec_lds)
      hipLaunchKernelGGL((evidence_contract_kernel<false, true>), grid, dim3(256), lds_bytes, st, a);
    else
      hipLaunchKernelGGL((evidence_contract_kernel<false, false>), grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(evidence_rowsum_kernel, dim3((unsigned)ceil_div(bc, 64)), dim3(64), 0, st, d_out, d_pts, j0, bc);
    ctx->launch_counter += 2;
    ktime_end(ctx, slot, "evidence_contract", (double)nrows * ((double)first + 0.5 * (double)nrows) * 8.0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gdml_fail(ctx, GDML_ERR_HIP, "gdml_evidence_grad launch: %s", hipGetErrorString(e));
  }
  GDML_TRY(phase_end(ctx, "evidence"));
  GDML_TRY(factor_logdet(ctx, g, d_diag, &terms_out[4]));
  std::vector<double> pts((size_t)(3 * M));
  HIP_CHECK(ctx, hipMemcpyAsync(pts.data(), d_pts, 3 * M * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipStreamSynchronize(st));
  double tr = 0.0, ik = 0.0, aka = 0.0, aa = 0.0;
  for (int64_t i = 0; i < M; ++i) {  // the tiles hold -A^-1
    ik -= pts[3 * i];
    aka += pts[3 * i + 1];
    tr -= pts[3 * i + 2];
  }
  for (int64_t i = 0; i < n; ++i) aa += alphas[i] * alphas[i];
  terms_out[0] = tr;
  terms_out[1] = ik;
  terms_out[2] = aka;
  terms_out[3] = aa;
  return GDML_OK;
}

extern "C" int gdml_evidence_grad(gdml_ctx* ctx, const double* alphas, int64_t n, double* terms_out, int* info) {
  if (!ctx) return GDML_ERR_INVALID;
  if (info) *info = 0;
  if (!alphas || !terms_out) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_evidence_grad: alphas or terms_out is NULL");
  if (ctx->world > 1)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "gdml_evidence_grad: the factor of a multi-rank context is distributed");
  GramSplit g;
  GDML_TRY(resident_factor_check(ctx, "gdml_evidence_grad", false, &g));
  const int64_t M = ctx->ts.M, n3 = g.n3;
  if (n != M * n3)
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_evidence_grad: n (%lld) is not 3N M = %lld", (long long)n, (long long)(M * n3));
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // the second matrix: as large as the factor.  Usable memory: what gdml_mem_info reports, or option chol.evidence_mem_budget (tests)
  const int64_t need = n * g.ld * 8;
  int64_t free_b = 0;
  GDML_TRY(gdml_mem_info(ctx, nullptr, &free_b, nullptr));
  const double budget = ctx_opt(ctx, "chol.evidence_mem_budget", 0.0);
  if (budget > 0.0) free_b = (int64_t)budget;
  double* Z = nullptr;
  if (need > free_b || ctx_alloc(ctx, (void**)&Z, need) != GDML_OK)
    return gdml_fail(ctx, GDML_ERR_OOM, "gdml_evidence_grad: the rows of L^-T need %lld bytes beside the factor, %lld are free",
                     (long long)need, (long long)free_b);
  const int rc = evidence_run(ctx, g, Z, alphas, terms_out);
  const std::string msg = ctx->err;
  const int rf = ctx_free(ctx, Z);  // waits for the stream first
  if (rc != GDML_OK) {
    ctx->err = msg;
    return rc;
  }
  return rf;
}
