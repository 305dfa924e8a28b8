// Greedy selection of training points from a candidate pool by joint information gain (no counterpart in the reference,
// which draws its training set from the energy histogram before any model exists).
//
// Conventions: A = -K + lam I = L L^T resident in ctx->K (lower triangle, row-major, pitch K_ld), n = 3N M,
// n3 = 3N, the pool holds B candidates (m_pool = n3 B rows).  For candidate q
//   W_q    = (-Kx_q) L^-T                                  (cross_rows_kernel of uncert.hip, tall_trsm of chol_solve.hip)
//   Sig_q  = (-k_qq) - W_q W_q^T                           (block_gram.hip + cov_reduce_kernel: the bits of gdml_predict_cov)
//   gain_q = log det(Sig_q / lam + I) = 2 sum_i log G_ii - n3 log lam,   G G^T = Sig_q + lam I     (select_score_kernel)
// Step t picks q* = argmax gain (ties: the lowest pool index; on the host) and conditions the pool on it:
//   C   = -k(pool, q*) - W W_q*^T - sum_{s<t} V_s V_s[q*]^T     (m_pool x n3: cross_rows_kernel with the pool as queries and q*
//                                                                as the one column point -- the pool is queried against the
//                                                                point, nothing is transposed; select_column_kernel;
//                                                                select_combine_kernel)
//   V_t = C G^-T                                               (select_trsm_kernel)
//   Sig_q <- Sig_q - V_t[q] V_t[q]^T                           (select_downdate_kernel)
// which is a block-pivoted Cholesky of the pool's joint posterior covariance plus lam I: the V_t are its block columns.
// Every sum runs in a fixed order and every output element has one owner: repeated calls give identical bits.  Stage A goes
// through the pool in chunks exactly as gdml_predict_cov does (the k splits depend on n alone, the solve runs on whole
// 128-row tiles), so a candidate's initial gain depends neither on its place in the pool nor on the chunk length.
#include "common.h"

#include <math.h>

typedef double d4 __attribute__((ext_vector_type(4)));

#define SEL_LDS_MAX_N3 128

// ---- score -----------------------------------------------------------------------------------------------------------------
// One workgroup per candidate: G G^T = Sig_q + lam I in place (the right-looking walk of loo_block_kernel: every element is
// updated in the order k = 0, 1, ...), gain = 2 sum_i log G_ii - n3 log lam summed by one thread in index order.  LDS form:
// (n3 + 1) x gp doubles (gp odd: a column walk meets every bank), 130 KB at n3 = 128; GLOBAL form above that: the same walk on
// a scratch slot per candidate.  With Gout the lower triangle of G is stored as well (the picked candidate's factor).
struct ScoreArgs {
  const double* Sig;   // [p][n3 x n3], lower triangle read
  double* gscr;        // GLOBAL form: [p][(n3 + 1) x gp]
  double* gain;        // (B): entry q0 + p
  int* flags;          // (B): set to 1 on a non-positive pivot
  const int* picked;   // (B) or null: candidates that are skipped
  double* Gout;        // n3 x n3 or null
  int64_t q0;
  int n3, gp;
  double lam, n3_log_lam;
};

template <bool LDS>
__global__ void __launch_bounds__(256) select_score_kernel(ScoreArgs a) {
  extern __shared__ double sel_lds[];
  const int tid = threadIdx.x, n3 = a.n3, gp = a.gp;
  const int64_t p = blockIdx.x, q = a.q0 + p;
  if (a.picked && a.picked[q]) return;
  double* const G = LDS ? sel_lds : a.gscr + p * (int64_t)(n3 + 1) * gp;
  double* const v = G + (int64_t)n3 * gp;
  const double* __restrict__ S = a.Sig + p * (int64_t)n3 * n3;
  for (int e = tid; e < n3 * n3; e += 256) {
    const int r = e / n3, c = e - r * n3;
    if (c > r) continue;
    G[(int64_t)r * gp + c] = S[e] + (r == c ? a.lam : 0.0);
  }
  __syncthreads();
  for (int k = 0; k < n3; ++k) {
    const double d = G[(int64_t)k * gp + k];
    if (!(d > 0.0)) {  // (also NaN) the same value in every thread: the workgroup leaves together
      if (tid == 0) a.flags[q] = 1;
      return;
    }
    const double rk = sqrt(d);
    for (int i = k + 1 + tid; i < n3; i += 256) G[(int64_t)i * gp + k] /= rk;
    __syncthreads();
    if (tid == 0) G[(int64_t)k * gp + k] = rk;  // not read again before the logarithms
    const int m = n3 - k - 1;
    for (int e = tid; e < m * m; e += 256) {
      const int ii = e / m, cc = e - ii * m;
      if (cc > ii) continue;
      const int i = k + 1 + ii, c = k + 1 + cc;
      G[(int64_t)i * gp + c] = __builtin_fma(-G[(int64_t)i * gp + k], G[(int64_t)c * gp + k], G[(int64_t)i * gp + c]);
    }
    __syncthreads();
  }
  for (int i = tid; i < n3; i += 256) v[i] = log(G[(int64_t)i * gp + i]);
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < n3; ++i) s += v[i];
    a.gain[q] = 2.0 * s - a.n3_log_lam;
  }
  if (a.Gout)
    for (int e = tid; e < n3 * n3; e += 256) {
      const int r = e / n3, c = e - r * n3;
      a.Gout[e] = c <= r ? G[(int64_t)r * gp + c] : 0.0;
    }
}

// ---- column ----------------------------------------------------------------------------------------------------------------
// W W_q*^T on the fp64 MFMA pipe: the hot kernel of a step.  The m_pool x n3 output is cut into
// 64 x 64 blocks (4 x 4 tiles of v_mfma_f64_16x16x4_f64); one WAVEFRONT owns (row block I of the pool's rows, column block J
// of q*'s rows, k split s).  Both operands are rows of W and come straight from global memory as 32-byte runs with the
// operand bijection of block_gram_kernel (lane group lk = lane >> 4 feeds k = 4 lk + step into MFMA step `step` on both
// sides); rows past the end re-read the last row (their results are never read); the pad columns [n, ld) of W are zero, so
// the k loop needs no edge.  The S partial tiles of a block go to scratch, select_combine_kernel sums them in the order
// s = 0 .. S - 1: no atomics.  Every (I, J) unit streams the 64 pool rows of block I, so W is read nblk = ceil(n3 / 64) times
// per step: once for n3 <= 64, twice up to 128 (a wavefront that kept all J blocks of a row block would need nblk x 128
// accumulator registers); the timer counts those bytes.
struct ColumnArgs {
  const double* W;
  double* part;  // [I][J][s][64 x 64]
  int64_t ld, L, units, m_pool, qrow0;
  int n3, nblk, S;
};

__global__ void __launch_bounds__(256) select_column_kernel(ColumnArgs g) {
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= g.units) return;
  const int s = (int)(unit % g.S);
  const int64_t up = unit / g.S;
  const int J = (int)(up % g.nblk);
  const int64_t I = up / g.nblk;
  const int64_t k_beg = (int64_t)s * g.L;
  const int64_t k_end = k_beg + g.L < g.ld ? k_beg + g.L : g.ld;
  const double* pa[4];
  const double* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int64_t ra = I * 64 + 16 * i + li;
    int rb = J * 64 + 16 * i + li;
    ra = ra < g.m_pool ? ra : g.m_pool - 1;
    rb = rb < g.n3 ? rb : g.n3 - 1;
    pa[i] = g.W + ra * g.ld + 4 * lk;
    pb[i] = g.W + (g.qrow0 + rb) * g.ld + 4 * lk;
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
  double* o = g.part + ((I * g.nblk + J) * g.S + s) * 4096;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(16 * i + lk + 4 * r) * 64 + 16 * j + li] = acc[i][j][r];
}

// ---- the small kernels of a step: every element has one owner ------------------------------------------------------------------
// C[r][c] = Vt[r][c] (= -k(pool, q*), written by the cross kernel) - sum_s partial_s - sum_{u<t} V_u[r] . V_u[q* rows c], in place:
// the partials in the order s = 0 .. S - 1, then the earlier steps in the order u = 0 .. t - 1, k = 0 .. n3 - 1, one fused
// multiply-add each.
struct CombineArgs {
  const double* part;
  const double* V;  // [u][m_pool x ldc]
  double* Vt;
  int64_t m_pool, qrow0, total;
  int n3, ldc, nblk, S, t;
};

__global__ void __launch_bounds__(256) select_combine_kernel(CombineArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const int64_t r = e / a.n3;
  const int c = (int)(e - r * a.n3);
  const double* __restrict__ p = a.part + (((r >> 6) * a.nblk + (c >> 6)) * a.S) * 4096 + (r & 63) * 64 + (c & 63);
  double acc = 0.0;
  for (int s = 0; s < a.S; ++s) acc += p[(int64_t)s * 4096];
  for (int u = 0; u < a.t; ++u) {
    const double* __restrict__ vr = a.V + ((int64_t)u * a.m_pool + r) * a.ldc;
    const double* __restrict__ vc = a.V + ((int64_t)u * a.m_pool + a.qrow0 + c) * a.ldc;
    for (int k = 0; k < a.n3; ++k) acc = __builtin_fma(vr[k], vc[k], acc);
  }
  a.Vt[r * a.ldc + c] -= acc;
}

// V_t = C G^-T in place: one thread per row, forward substitution in the order j = 0, 1, ..., k = 0 .. j - 1
__global__ void __launch_bounds__(64) select_trsm_kernel(double* __restrict__ Vt, const double* __restrict__ G, int64_t m_pool, int n3,
                                                         int ldc) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= m_pool) return;
  double* row = Vt + r * ldc;
  for (int j = 0; j < n3; ++j) {
    const double* __restrict__ gj = G + (int64_t)j * n3;
    double s = row[j];
    for (int k = 0; k < j; ++k) s = __builtin_fma(-row[k], gj[k], s);
    row[j] = s / gj[j];
  }
}

// Sig_q <- Sig_q - V_t[q] V_t[q]^T on the lower triangle (the only part the score kernel reads) of every remaining candidate
__global__ void __launch_bounds__(256) select_downdate_kernel(double* __restrict__ Sig, const double* __restrict__ Vt,
                                                             const int* __restrict__ picked, int n3, int ldc) {
  const int64_t q = blockIdx.x;
  if (picked[q]) return;
  double* S = Sig + q * (int64_t)n3 * n3;
  const double* __restrict__ V = Vt + q * (int64_t)n3 * ldc;
  for (int e = threadIdx.x; e < n3 * n3; e += 256) {
    const int r = e / n3, c = e - r * n3;
    if (c > r) continue;
    const double* __restrict__ vr = V + (int64_t)r * ldc;
    const double* __restrict__ vc = V + (int64_t)c * ldc;
    double acc = 0.0;
    for (int k = 0; k < n3; ++k) acc = __builtin_fma(vr[k], vc[k], acc);
    S[e] -= acc;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// doubles the joint sweep retains for a pool of B candidates and n_select > 1 picks (W, Sig, descriptors, the block columns V,
// the partial tiles of the column, G, scratch of the GLOBAL score form, gains / flags)
static int64_t select_retained_doubles(const GramSplit& g, int64_t D, int64_t B, int64_t n_select, bool lds) {
  const int64_t n3 = g.n3, m = B * n3, ldc = round16(n3), gp = n3 | 1;
  const int64_t nv = n_select > 1 ? n_select - 1 : 0;
  return pad_rows128(m) * g.ld + B * (n3 * n3 + 4 * D) + nv * m * ldc + (m + 63) / 64 * g.nblk * g.S * 4096 + n3 * n3 +
         (lds ? 0 : (B + 1) * (n3 + 1) * gp) + 3 * (B + 2) + 16;
}

static void score_launch(gdml_ctx* ctx, const ScoreArgs& a, int64_t count, bool lds, size_t lds_bytes) {
  if (lds)
    hipLaunchKernelGGL(select_score_kernel<true>, dim3((unsigned)count), dim3(256), lds_bytes, ctx->stream, a);
  else
    hipLaunchKernelGGL(select_score_kernel<false>, dim3((unsigned)count), dim3(256), 0, ctx->stream, a);
  ctx->launch_counter++;
}

extern "C" int gdml_select_points(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv,
                                  int64_t n_select, double min_gain, int64_t* idx_out, double* gain_out, double* gain0_out,
                                  int64_t* n_selected_out, int* info) {
  if (!ctx) return GDML_ERR_INVALID;
  if (info) *info = 0;
  if (!R) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_select_points: R is NULL");
  if (B < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_select_points: B < 0");
  if (n_select < 0 || n_select > B)
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_select_points: n_select %lld is not in [0, B = %lld]", (long long)n_select, (long long)B);
  if ((lat == nullptr) != (lat_inv == nullptr))
    return gdml_fail(ctx, GDML_ERR_INVALID, "lattice and inverse must both be given or both NULL");
  if (!gain0_out || !n_selected_out) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_select_points: gain0_out or n_selected_out is NULL");
  if (n_select > 0 && (!idx_out || !gain_out)) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_select_points: idx_out or gain_out is NULL");
  if (min_gain != min_gain) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_select_points: min_gain is NaN");
  *n_selected_out = 0;
  if (comm_active(ctx) && ctx->world > 1)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "gdml_select_points: the factor of a multi-rank context is distributed");
  GramSplit g;
  GDML_TRY(resident_factor_check(ctx, "gdml_select_points", true, &g));
  const TrainSet& ts = ctx->ts;
  if (B == 0) return GDML_OK;
  if (B * 2 > INT32_MAX) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_select_points: a pool of %lld candidates exceeds the cross kernel's range", (long long)B);
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t n3 = g.n3, D = ts.D, m_pool = B * n3, ldc = round16(n3);
  const int gp = (int)(n3 | 1);
  const bool lds = n3 <= SEL_LDS_MAX_N3;
  const bool joint = n_select > 1;  // a single pick conditions nothing: the streamed gains and an argmax are all it needs
  const size_t lds_bytes = lds ? (size_t)(n3 + 1) * gp * 8 : 0;
  const double lam = ctx->K_lam, sig = ctx->K_sig;
  const int64_t gscr_item = lds ? 0 : (n3 + 1) * gp;

  // ---- the retained buffers of the joint sweep; with n_select <= 1 only the gains are kept and the chunks stream
  double *Wb = nullptr, *ws = nullptr;
  auto drop = [&](int rc) {
    (void)hipStreamSynchronize(st);
    if (ws) (void)ctx_free(ctx, ws);
    if (Wb) (void)ctx_free(ctx, Wb);
    if (rc != GDML_OK) {  // on an error nothing of this call stays allocated
      (void)ctx_slot_release(ctx, SLOT_GRAM_WS);
      (void)ctx_slot_release(ctx, SLOT_GRAM_ROWS);
    }
    return rc;
  };

  const int64_t small_A = cov_chunk_doubles(g, D, true) + gscr_item;  // doubles per candidate of a chunk
  if (joint) {
    // budget: option chol.select_mem_budget (bytes; tests), else 90 % of what is free plus the two Gram slots, which are carved anew
    size_t mem_free = 0, mem_total = 0;
    DROP_HIP(hipMemGetInfo(&mem_free, &mem_total));
    double budget = ctx_opt(ctx, "chol.select_mem_budget", 0.0);
    if (!(budget > 0.0))
      budget = 0.9 * (double)((int64_t)mem_free + ctx->slot_bytes[SLOT_GRAM_WS] + ctx->slot_bytes[SLOT_GRAM_ROWS]);
    const double stage_a = 8.0 * (double)(pad_rows128(n3) * g.ld + small_A);  // a chunk of one candidate
    auto need = [&](int64_t b) { return 8.0 * (double)select_retained_doubles(g, D, b, n_select, lds) + stage_a; };
    if (need(B) > budget) {
      int64_t lo = 0, hi = B;  // need(lo) fits (or lo = 0), need(hi) does not
      while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (need(mid) <= budget) lo = mid; else hi = mid;
      }
      if (lo < n_select) lo = 0;  // a pool smaller than the number of picks is no use
      return drop(gdml_fail(ctx, GDML_ERR_OOM,
                            "gdml_select_points: the retained rows of %lld candidates need %.0f MB, the budget is %.0f MB; "
                            "largest pool that fits: %lld",
                            (long long)B, need(B) / 1048576.0, budget / 1048576.0, (long long)lo));
    }
    DROP_TRY(ctx_slot_release(ctx, SLOT_GRAM_WS));
    DROP_TRY(ctx_slot_release(ctx, SLOT_GRAM_ROWS));
    DROP_TRY(ctx_alloc(ctx, (void**)&Wb, pad_rows128(m_pool) * g.ld * 8));
  }
  const int64_t nv = n_select > 1 ? n_select - 1 : 0;
  const int64_t nrb = (m_pool + 63) / 64;
  const int64_t ws_doubles = joint ? select_retained_doubles(g, D, B, n_select, lds) - pad_rows128(m_pool) * g.ld : 3 * (B + 2) + 16;
  DROP_TRY(ctx_alloc(ctx, (void**)&ws, ws_doubles * 8));
  double* const d_gain = ws;                                   // (B + 1): the last entry takes the pivot launch's gain
  int* const d_flags = (int*)(d_gain + B + 2);                 // (B)
  int* const d_picked = (int*)(d_gain + B + 2 + (B + 2) / 2 + 1);  // (B)
  double* const Sig = d_gain + 3 * (B + 2) + 16 - 0;           // joint only from here on
  double* const xq_all = Sig + (joint ? B * n3 * n3 : 0);
  double* const gq_all = xq_all + (joint ? B * D : 0);
  double* const Vb = gq_all + (joint ? 3 * B * D : 0);
  double* const cpart = Vb + nv * m_pool * ldc;
  double* const Gf = cpart + (joint ? nrb * g.nblk * g.S * 4096 : 0);
  double* const gscr_B = Gf + (joint ? n3 * n3 : 0);
  DROP_HIP(hipMemsetAsync(d_gain, 0, (3 * (B + 2) + 16) * 8, st));

  if (lds_bytes > 64 * 1024)
    DROP_HIP(hipFuncSetAttribute((const void*)select_score_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  ScoreArgs sa;
  sa.flags = d_flags; sa.gain = d_gain; sa.n3 = (int)n3; sa.gp = gp; sa.lam = lam; sa.n3_log_lam = (double)n3 * log(lam);

  // ---- stage A: W, Sig^(0) and the initial gains, chunk by chunk (the sequence of gdml_predict_cov)
  int64_t bcA = 0;
  double *rowsA = nullptr, *wsA = nullptr;
  DROP_TRY(gram_workspace(ctx, g, "chol.select_chunk", B, small_A, 0, &bcA, &rowsA, &wsA));
  static const CovPath path = {"select_cross", "select_solve", "select_gram", "select", 128, nullptr};
  CovChunk a;
  double* const a_gscr = cov_chunk_carve(&a, wsA, g, D, bcA, true);
  phase_begin(ctx);
  for (int64_t b0 = 0; b0 < B; b0 += bcA) {
    const int bc = (int)(B - b0 < bcA ? B - b0 : bcA);
    const int64_t rows = (int64_t)bc * n3;
    DROP_TRY(cov_chunk_step(ctx, g, path, a, rowsA, nullptr, R + b0 * n3, false, bc, lat, lat_inv, 1, a.out));
    sa.Sig = a.out; sa.gscr = a_gscr; sa.picked = nullptr; sa.Gout = nullptr; sa.q0 = b0;
    const int slot = ktime_begin(ctx);
    score_launch(ctx, sa, bc, lds, lds_bytes);
    ktime_end(ctx, slot, "select_score", (double)bc * (double)n3 * n3 * n3 / 3.0);
    DROP_HIP(hipGetLastError());
    if (joint) {
      DROP_HIP(hipMemcpyAsync(Wb + b0 * n3 * g.ld, rowsA, rows * g.ld * 8, hipMemcpyDeviceToDevice, st));
      DROP_HIP(hipMemcpyAsync(Sig + b0 * n3 * n3, a.out, rows * n3 * 8, hipMemcpyDeviceToDevice, st));
      DROP_HIP(hipMemcpyAsync(xq_all + b0 * D, a.xq, bc * D * 8, hipMemcpyDeviceToDevice, st));
      DROP_HIP(hipMemcpyAsync(gq_all + 3 * b0 * D, a.gq, bc * D * 24, hipMemcpyDeviceToDevice, st));
    }
  }
  if (joint && pad_rows128(m_pool) > m_pool)
    DROP_HIP(hipMemsetAsync(Wb + m_pool * g.ld, 0, (pad_rows128(m_pool) - m_pool) * g.ld * 8, st));

  // ---- stage B: pick, condition, score again
  std::vector<double> gain((size_t)B);
  std::vector<int> flags((size_t)B), picked((size_t)B, 0);
  static const int one = 1;
  int64_t k = 0;
  for (int64_t t = 0; t == 0 || t < n_select; ++t) {
    if (t > 0) {
      sa.Sig = Sig; sa.gscr = gscr_B; sa.picked = d_picked; sa.Gout = nullptr; sa.q0 = 0;
      const int slot = ktime_begin(ctx);
      score_launch(ctx, sa, B, lds, lds_bytes);
      ktime_end(ctx, slot, "select_score", (double)(B - t) * (double)n3 * n3 * n3 / 3.0);
      DROP_HIP(hipGetLastError());
    }
    DROP_HIP(hipMemcpyAsync(gain.data(), d_gain, B * 8, hipMemcpyDeviceToHost, st));
    DROP_HIP(hipMemcpyAsync(flags.data(), d_flags, B * sizeof(int), hipMemcpyDeviceToHost, st));
    DROP_HIP(hipStreamSynchronize(st));
    for (int64_t q = 0; q < B; ++q)
      if (flags[q] && !picked[q]) {
        if (info) *info = (int)(q + 1);
        return drop(gdml_fail(ctx, GDML_ERR_NOT_PD,
                              "gdml_select_points: the posterior covariance of candidate %lld plus lam I is not positive definite (step %lld)",
                              (long long)q, (long long)t));
      }
    if (t == 0) memcpy(gain0_out, gain.data(), (size_t)B * 8);
    if (t >= n_select) break;
    int64_t best = -1;
    for (int64_t q = 0; q < B; ++q)  // ties: the lowest pool index
      if (!picked[q] && (best < 0 || gain[q] > gain[best])) best = q;
    if (best < 0 || gain[best] < min_gain) break;
    idx_out[k] = best;
    gain_out[k] = gain[best];
    ++k;
    picked[best] = 1;
    if (t + 1 >= n_select) break;
    // the picked candidate's block column V_t
    double* const Vt = Vb + t * m_pool * ldc;
    const int64_t qrow0 = best * n3;
    DROP_TRY(cross_rows_launch(ctx, xq_all + best * D, gq_all + 3 * best * D, 1, xq_all, gq_all, (int)B, Vt, ldc, nullptr, -1.0, sig,
                              "select_cross"));
    int slot = ktime_begin(ctx);
    ColumnArgs ca;
    ca.W = Wb; ca.part = cpart; ca.ld = g.ld; ca.L = g.L; ca.m_pool = m_pool; ca.qrow0 = qrow0;
    ca.n3 = (int)n3; ca.nblk = g.nblk; ca.S = g.S; ca.units = nrb * g.nblk * g.S;
    hipLaunchKernelGGL(select_column_kernel, dim3((unsigned)ceil_div(ca.units, 4)), dim3(256), 0, st, ca);
    ctx->launch_counter++;
    ktime_end(ctx, slot, "select_column", (double)m_pool * (double)g.ld * 8.0 * g.nblk);  // bytes of W read, nblk times
    DROP_HIP(hipGetLastError());
    // G of the picked candidate: the score kernel on its Sig once more, the factor stored
    sa.Sig = Sig + best * n3 * n3; sa.gscr = gscr_B; sa.picked = nullptr; sa.Gout = Gf; sa.q0 = B;
    slot = ktime_begin(ctx);
    score_launch(ctx, sa, 1, lds, lds_bytes);
    ktime_end(ctx, slot, "select_score", (double)n3 * n3 * n3 / 3.0);
    DROP_HIP(hipGetLastError());
    DROP_HIP(hipMemcpyAsync(d_picked + best, &one, sizeof(int), hipMemcpyHostToDevice, st));
    slot = ktime_begin(ctx);
    CombineArgs cb;
    cb.part = cpart; cb.V = Vb; cb.Vt = Vt; cb.m_pool = m_pool; cb.qrow0 = qrow0; cb.total = m_pool * n3;
    cb.n3 = (int)n3; cb.ldc = (int)ldc; cb.nblk = g.nblk; cb.S = g.S; cb.t = (int)t;
    hipLaunchKernelGGL(select_combine_kernel, dim3((unsigned)ceil_div(cb.total, 256)), dim3(256), 0, st, cb);
    hipLaunchKernelGGL(select_trsm_kernel, dim3((unsigned)ceil_div(m_pool, 64)), dim3(64), 0, st, Vt, Gf, m_pool, (int)n3, (int)ldc);
    hipLaunchKernelGGL(select_downdate_kernel, dim3((unsigned)B), dim3(256), 0, st, Sig, Vt, d_picked, (int)n3, (int)ldc);
    ctx->launch_counter += 3;
    ktime_end(ctx, slot, "select_update", (double)m_pool * (double)n3 * (2.0 * n3 * (t + 1) + (double)n3));
    DROP_HIP(hipGetLastError());
  }
  DROP_TRY(phase_end(ctx, path.phase));
  *n_selected_out = k;
  return drop(GDML_OK);
}
