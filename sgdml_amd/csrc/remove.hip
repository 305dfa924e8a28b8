// Removing training points from the resident Cholesky factor without factoring again (no counterpart in the reference, which
// retrains from nothing).  The inverse of extend.hip.
//
// Conventions: A = -K + lam I = L L^T resident in ctx->K (lower triangle, row-major, pitch K_ld = n rounded up
// to 16), n = 3N M.  Removing b points deletes their m = 3N b rows and columns from A.  With L_c = L[kept, kept] (lower
// triangular: the kept points keep their order) and V = L[kept, removed] (n' x m, zero above each removed point's position),
//   A_kept = L_c L_c^T + V V^T = [L_c V] [L_c V]^T,
// so any orthogonal Q with [L_c V] Q = [L' 0], L' lower triangular, gives the factor of A_kept: a rank-m POSITIVE update.  Q is
// built block column by block column (64 columns): a Householder LQ of the 64 x (64 + w) block [L_kk V_k] (remove_panel_kernel;
// reflector i = e_i + [0; v_i] touches diagonal element i and the V part only, because L_kk is triangular), kept as the WY pair
// (U, T), Q_k = I - [I; U^T] T [I, U], and applied to the rows below on the fp64 MFMA pipe (remove_apply_kernel).
// V goes through in column slices of at most RM_W columns (the LDS of the two kernels; option chol.remove_chunk caps the points
// per slice): a sweep's Q mixes the columns of L with the columns of ITS slice only, the other slices' columns are not
// touched by it, and [L' V_rest] [L' V_rest]^T = A_kept holds after every sweep -- the slices are independent and run one
// after another, highest columns first (their sweeps start furthest right).
// Everything new lives in buffers of its own until the commit (as in extend.hip): a failure leaves the context as it was.
#include <algorithm>

#include "common.h"

typedef double d4 __attribute__((ext_vector_type(4)));

#define RM_W 128  // widest slice of V (columns): 64 x (RM_W + 4) doubles of reflectors beside two 64 x 64 blocks in LDS

// ---- compaction: L[kept, kept] into the new buffer, L[kept, removed] into the side buffer ------------------------------------
// dst row r: columns 0 .. r from the kept columns of the old row, zeros above the diagonal up to the 64-column grid of the
// diagonal blocks and on to the 512-column panel grid (the guarantees of extend_copy_lower_kernel), written as 32-byte groups.
// A kept column right of a removed point moves left by a multiple of 3N, in general no multiple of 4: a group whose four
// sources lie in one point at a 32-byte aligned address is loaded as one group, any other element by element.
// V row r: column j of slice g (w columns, padded with zeros to wp) at g wp + j.
// A workgroup takes rows r and n1 - 1 - r together: every workgroup moves about the same number of bytes.
struct RemoveCompactArgs {
  const double* src;
  double* dst;
  double* V;
  const int32_t* kept_old;  // [M1] old index of kept point p
  const int32_t* rem_old;   // [b]  old index of removed point t (ascending)
  int64_t lds, ldd, ldv, n1;
  int n3, M1, m, w, wp;
};

__global__ void __launch_bounds__(256) remove_compact_kernel(RemoveCompactArgs a) {
  const int64_t half = (a.n1 + 1) / 2;
  const int n3 = a.n3;
  for (int64_t i = blockIdx.x; i < half; i += gridDim.x) {
    for (int k = 0; k < 2; ++k) {
      const int64_t r = k == 0 ? i : a.n1 - 1 - i;
      if (k == 1 && r == i) break;
      const int pr = (int)(r / n3);
      const int64_t ro = (int64_t)a.kept_old[pr] * n3 + (r - (int64_t)pr * n3);
      const double* __restrict__ s = a.src + ro * a.lds;
      d4* __restrict__ d = reinterpret_cast<d4*>(a.dst + r * a.ldd);
      int64_t c_zero = (r / 512 + 1) * 512;
      if (c_zero > a.ldd) c_zero = a.ldd;
      for (int64_t v = threadIdx.x; v < c_zero / 4; v += 256) {
        const int64_t c = 4 * v;
        d4 o = (d4){0.0, 0.0, 0.0, 0.0};
        if (c <= r) {
          int p = (int)(c / n3), e = (int)(c - (int64_t)p * n3);
          int64_t co = (int64_t)a.kept_old[p] * n3 + e;
          if (e + 3 < n3 && c + 3 <= r && (co & 3) == 0) {
            o = *reinterpret_cast<const d4*>(s + co);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (c + q <= r) o[q] = s[co];
              if (++e == n3) {
                e = 0;
                ++p;
                co = p < a.M1 ? (int64_t)a.kept_old[p] * n3 : 0;
              } else {
                ++co;
              }
            }
          }
        }
        d[v] = o;
      }
      double* __restrict__ vr = a.V + r * a.ldv;
      for (int64_t j = threadIdx.x; j < a.ldv; j += 256) {
        const int g = (int)(j / a.wp), p = (int)(j - (int64_t)g * a.wp);
        const int64_t jj = (int64_t)g * a.w + p;
        double val = 0.0;
        if (p < a.w && jj < a.m) {
          const int t = (int)(jj / n3);
          const int64_t co = (int64_t)a.rem_old[t] * n3 + (jj - (int64_t)t * n3);
          if (co < ro) val = s[co];
        }
        vr[j] = val;
      }
    }
  }
}

// ---- panel: Householder LQ of [L_kk V_k], one workgroup ------------------------------------------------------------------
// Row i of the block is [.. alpha ..| x]: reflector i maps (alpha, x) to (beta, 0), beta = -sign(alpha) sqrt(alpha^2 + |x|^2),
// tau = (beta - alpha) / beta, v = x / (alpha - beta) (LAPACK's dlarfg), and is applied to the rows below it in the block.
// x = 0 exactly: the identity (tau = 0).  Column i of the new factor is negated as a whole where beta < 0 (sgn; the apply
// kernel does the same to the rows below), so the diagonal stays positive.  A diagonal entry that is not finite or zero, or
// a row of V that is not finite, sets *flag to the 1-based column (the first one wins: one workgroup, launches in order).
// Out: the new L_kk, zeros in this block's rows of V, and for the apply kernel U (64 x wp, row i = v_i), T (64 x 64 upper
// triangular, LAPACK's forward columnwise larft: T[0:i, i] = -tau_i T[0:i, 0:i] (U U^T)[0:i, i]) and sgn.
// Every sum runs in a fixed order (strided partial sums, butterfly over the lanes): no atomics.
struct RemovePanelArgs {
  double* L;
  double* V;
  double *U, *T, *sgn;
  int* flag;
  int64_t ld, ldv, k;
  int wk, voff, wp, below;
};

__global__ void __launch_bounds__(256) remove_panel_kernel(RemovePanelArgs a) {
  extern __shared__ __attribute__((aligned(16))) double rm_lds[];
  const int pv = a.wp + 4;  // pitch = 4 (mod 16): the 4 lanes of a row and the 16 rows of a wavefront spread over the banks
  double* Ls = rm_lds;        // 64 x 65
  double* Ts = Ls + 64 * 65;  // 64 x 65: U U^T strictly below the diagonal, T on and above it
  double* Vs = Ts + 64 * 65;  // 64 x pv
  double* tau = Vs + 64 * pv;
  double* sg = tau + 64;
  const int tid = threadIdx.x, wk = a.wk, wp = a.wp;
  for (int e = tid; e < 4096; e += 256) {
    const int r = e >> 6, c = e & 63;
    Ls[r * 65 + c] = (r < wk && c <= r) ? a.L[(a.k + r) * a.ld + a.k + c] : 0.0;
    Ts[r * 65 + c] = 0.0;
  }
  for (int e = tid; e < 64 * wp; e += 256) {
    const int r = e / wp, p = e - r * wp;
    Vs[r * pv + p] = r < wk ? a.V[(a.k + r) * a.ldv + a.voff + p] : 0.0;
  }
  if (tid < 64) {
    tau[tid] = 0.0;
    sg[tid] = 1.0;
  }
  __syncthreads();
  const int rr = tid >> 2, rq = tid & 3;
  for (int i = 0; i < wk; ++i) {
    if (tid < 64) {
      double* __restrict__ vi = Vs + i * pv;
      double s = 0.0;
      for (int p = tid; p < wp; p += 64) s = __builtin_fma(vi[p], vi[p], s);
      s = wave_sum(s);
      const double alpha = Ls[i * 65 + i];
      double beta = alpha, t = 0.0, inv = 0.0;
      if (s > 0.0) {
        const double nrm = sqrt(__builtin_fma(alpha, alpha, s));
        beta = alpha > 0.0 ? -nrm : nrm;
        t = (beta - alpha) / beta;
        inv = 1.0 / (alpha - beta);
      }
      for (int p = tid; p < wp; p += 64) vi[p] *= inv;
      if (tid == 0) {
        Ls[i * 65 + i] = beta;
        tau[i] = t;
        sg[i] = beta < 0.0 ? -1.0 : 1.0;
        const bool ok = s >= 0.0 && fabs(beta) > 0.0 && fabs(beta) <= 1.79769313486231570815e308;
        if (!ok && *a.flag == 0) *a.flag = (int)(a.k + i + 1);
      }
    }
    __syncthreads();
    const double t = tau[i];
    if (t != 0.0 && rr > i && rr < wk) {  // (the 4 lanes of a row take the branch together)
      const double* __restrict__ vi = Vs + i * pv;
      double* __restrict__ vr = Vs + rr * pv;
      double s = 0.0;
      for (int p = rq; p < wp; p += 4) s = __builtin_fma(vr[p], vi[p], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      const double tw = t * (Ls[rr * 65 + i] + s);
      for (int p = rq; p < wp; p += 4) vr[p] = __builtin_fma(-tw, vi[p], vr[p]);
      if (rq == 0) Ls[rr * 65 + i] -= tw;
    }
    __syncthreads();
  }
  // the new diagonal block (zeros above the diagonal stay) and this block's rows of V
  for (int e = tid; e < 4096; e += 256) {
    const int r = e >> 6, c = e & 63;
    if (r < wk && c <= r) a.L[(a.k + r) * a.ld + a.k + c] = sg[c] * Ls[r * 65 + c];
  }
  for (int e = tid; e < 64 * wp; e += 256) {
    const int r = e / wp, p = e - r * wp;
    if (r < wk) a.V[(a.k + r) * a.ldv + a.voff + p] = 0.0;
  }
  if (!a.below) return;
  for (int e = tid; e < 4096; e += 256) {
    const int i = e >> 6, c = e & 63;
    if (c < i) {
      const double* __restrict__ vi = Vs + i * pv;
      const double* __restrict__ vc = Vs + c * pv;
      double s = 0.0;
      for (int p = 0; p < wp; ++p) s = __builtin_fma(vi[p], vc[p], s);
      Ts[i * 65 + c] = s;
    }
  }
  __syncthreads();
  for (int i = 0; i < 64; ++i) {  // row rr of T belongs to the 4 lanes of rr
    if (i == rr) {
      if (rq == 0) Ts[rr * 65 + rr] = tau[rr];
    } else if (i > rr) {
      double s = 0.0;
      for (int c = rr + rq; c < i; c += 4) s = __builtin_fma(Ts[rr * 65 + c], Ts[i * 65 + c], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      if (rq == 0) Ts[rr * 65 + i] = -tau[i] * s;
    }
    __syncthreads();
  }
  for (int e = tid; e < 64 * wp; e += 256) {
    const int r = e / wp, p = e - r * wp;
    a.U[e] = Vs[r * pv + p];
  }
  for (int e = tid; e < 4096; e += 256) {
    const int r = e >> 6, c = e & 63;
    a.T[e] = c >= r ? Ts[r * 65 + c] : 0.0;
  }
  if (tid < 64) a.sgn[tid] = sg[tid];
}

// ---- apply: [L_bk V_b] <- [L_bk V_b] Q_k for the rows below the block ------------------------------------------------------
// X = [X1 X2] (64 and wp columns of a row):  W = X1 + X2 U^T,  Z = W T,  X1' = (X1 - Z) sgn,  X2' = X2 - Z U.
// A wavefront owns 16 rows and keeps them in registers from the load to the store.  All three products run TRANSPOSED on
// v_mfma_f64_16x16x4_f64 (W^T = X1^T + U X2^T, Z^T = T^T W^T, X2'^T = X2^T - U^T Z^T): the rows are then the B-side index
// (lane & 15) throughout, and with the A-side rows fed in the order pi(a) = 4 (a & 3) + (a >> 2) a lane's four results of a
// 16 x 16 tile, A-side rows (lane >> 4) + 4 r, are the columns 4 (lane >> 4) + r of its row -- the 32-byte group it loaded.
// So X1 and X2 are the C operands as loaded, W and Z are B operands as they come out of the MFMA, and nothing is staged.
// U, T and sgn sit in LDS (pitch = 4 mod 16 doubles); a workgroup walks over row tiles of 64.  Rows past n1 re-read row n1 - 1
// and store nothing.  T is upper triangular: Z's 16-column tile ct sums over the tiles kt <= ct of W only.
struct RemoveApplyArgs {
  double* L;
  double* V;
  const double *U, *T, *sgn;
  int64_t ld, ldv, k, r0, n1;
  int voff, wp;
};

__global__ void __launch_bounds__(256) remove_apply_kernel(RemoveApplyArgs a) {
  extern __shared__ __attribute__((aligned(16))) double rm_lds[];
  const int wp = a.wp, pu = wp + 4, nt = wp / 16;
  double* Us = rm_lds;         // 64 x pu
  double* Ts = Us + 64 * pu;   // 64 x 68
  double* sg = Ts + 64 * 68;   // 64
  const int tid = threadIdx.x;
  for (int e = tid; e < 64 * wp; e += 256) {
    const int r = e / wp, p = e - r * wp;
    Us[r * pu + p] = a.U[e];
  }
  for (int e = tid; e < 4096; e += 256) Ts[(e >> 6) * 68 + (e & 63)] = a.T[e];
  if (tid < 64) sg[tid] = a.sgn[tid];
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int pi = 4 * (li & 3) + (li >> 2);
  const int64_t ntiles = (a.n1 - a.r0 + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row = a.r0 + tile * 64 + wv * 16 + li;
    const bool live = row < a.n1;
    const int64_t rr = live ? row : a.n1 - 1;
    double* const pl = a.L + rr * a.ld + a.k + 4 * lk;
    double* const px = a.V + rr * a.ldv + a.voff + 4 * lk;
    d4 x1[4], x2[RM_W / 16], w[4], z[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) x1[ct] = *reinterpret_cast<const d4*>(pl + 16 * ct);
#pragma unroll
    for (int t = 0; t < RM_W / 16; ++t)
      if (t < nt) x2[t] = *reinterpret_cast<const d4*>(px + 16 * t);
    // W^T = X1^T + U X2^T
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      d4 acc = x1[ct];
      const double* ua = Us + (16 * ct + pi) * pu + 4 * lk;
#pragma unroll
      for (int t = 0; t < RM_W / 16; ++t)
        if (t < nt) {
          const d4 u = *reinterpret_cast<const d4*>(ua + 16 * t);
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(u[s], x2[t][s], acc, 0, 0, 0);
        }
      w[ct] = acc;
    }
    // Z^T = T^T W^T
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kt = 0; kt <= ct; ++kt)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ts[(16 * kt + 4 * lk + s) * 68 + 16 * ct + pi], w[kt][s], acc, 0, 0, 0);
      z[ct] = acc;
    }
    // X1' = (X1 - Z) sgn
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      d4 o;
#pragma unroll
      for (int s = 0; s < 4; ++s) o[s] = (x1[ct][s] - z[ct][s]) * sg[16 * ct + 4 * lk + s];
      if (live) *reinterpret_cast<d4*>(pl + 16 * ct) = o;
      z[ct] = -z[ct];
    }
    // X2'^T = X2^T - U^T Z^T
#pragma unroll
    for (int t = 0; t < RM_W / 16; ++t)
      if (t < nt) {
        d4 acc = x2[t];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int s = 0; s < 4; ++s)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Us[(16 * kt + 4 * lk + s) * pu + 16 * t + pi], z[kt][s], acc, 0, 0, 0);
        if (live) *reinterpret_cast<d4*>(px + 16 * t) = acc;
      }
  }
}

extern "C" int gdml_factor_remove(gdml_ctx* ctx, const int64_t* idx, int64_t b, int* info) {
  if (!ctx) return GDML_ERR_INVALID;
  if (info) *info = 0;
  if (b < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_factor_remove: b < 0");
  if (b > 0 && !idx) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_factor_remove: idx is NULL");
  if (comm_active(ctx) && ctx->world > 1)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "gdml_factor_remove: the factor of a multi-rank context is distributed");
  GramSplit g0;
  GDML_TRY(resident_factor_check(ctx, "gdml_factor_remove", true, &g0));
  TrainSet& ts = ctx->ts;
  const int64_t M0 = ts.M, n3 = g0.n3, D = ts.D, ld0 = g0.ld;
  if (b == 0) return GDML_OK;
  if (b >= M0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_factor_remove: %lld of %lld points: nothing would be left", (long long)b, (long long)M0);
  std::vector<char> gone((size_t)M0, 0);
  for (int64_t i = 0; i < b; ++i) {
    if (idx[i] < 0 || idx[i] >= M0)
      return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_factor_remove: index %lld is outside [0, %lld)", (long long)idx[i], (long long)M0);
    if (gone[(size_t)idx[i]]) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_factor_remove: index %lld occurs twice", (long long)idx[i]);
    gone[(size_t)idx[i]] = 1;
  }
  const int64_t M1 = M0 - b, n1 = M1 * n3, ld1 = round16(n1), m = b * n3;
  std::vector<int32_t> map((size_t)M0);  // [0, M1): old index of kept point p; [M1, M0): removed points, ascending
  {
    int64_t pk = 0, pr = M1;
    for (int64_t i = 0; i < M0; ++i) map[(size_t)(gone[(size_t)i] ? pr++ : pk++)] = (int32_t)i;
  }
  // slices of V: at most chol.remove_chunk points and RM_W columns each, padded to a multiple of 16 columns
  int64_t chunk = ctx_opt_i(ctx, "chol.remove_chunk", 64);
  if (chunk < 1) chunk = 1;
  int64_t w = chunk * n3 < RM_W ? chunk * n3 : RM_W;
  if (w > m) w = m;
  const int64_t wp = round16(w), nsl = (m + w - 1) / w, ldv = nsl * wp;

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

  // the matrix with 127 pad rows behind it (gdml_factor_extend solves its new rows there on whole 128-row tiles)
  const int64_t Kn_bytes = (n1 + 127) * ld1 * 8;
  DROP_TRY(ctx_alloc(ctx, (void**)&Kn, Kn_bytes));
  DROP_TRY(ctx_alloc(ctx, (void**)&x1, M1 * D * 8));
  DROP_TRY(ctx_alloc(ctx, (void**)&g1, M1 * D * 24));
  // work buffer: V (n1 x ldv) | U (64 x wp) | T (64 x 64) | sgn (64) | the point map (M0 int32)
  const int64_t ws_doubles = n1 * ldv + 64 * wp + 4096 + 64 + (M0 + 1) / 2;
  DROP_TRY(ctx_alloc(ctx, (void**)&ws, ws_doubles * 8));
  double* const V = ws;
  double* const Ub = V + n1 * ldv;
  double* const Tb = Ub + 64 * wp;
  double* const sgb = Tb + 4096;
  int32_t* const d_map = reinterpret_cast<int32_t*>(sgb + 64);
  const int lds_panel = (int)((2 * 64 * 65 + 64 * (wp + 4) + 128) * 8);
  const int lds_apply = (int)((64 * (wp + 4) + 64 * 68 + 64) * 8);
  DROP_HIP(hipFuncSetAttribute((const void*)remove_panel_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_panel));
  DROP_HIP(hipFuncSetAttribute((const void*)remove_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_apply));

  phase_begin(ctx);
  DROP_HIP(hipMemcpyAsync(d_map, map.data(), M0 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  DROP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), st));
  DROP_HIP(hipMemsetAsync(Kn + n1 * ld1, 0, 127 * ld1 * 8, st));
  // the kept points' descriptors and Jacobians, one copy per run of consecutive kept points
  for (int64_t p = 0; p < M1;) {
    int64_t q = p + 1;
    while (q < M1 && map[(size_t)q] == map[(size_t)q - 1] + 1) ++q;
    const int64_t o = map[(size_t)p];
    DROP_HIP(hipMemcpyAsync(x1 + p * D, ts.x + o * D, (q - p) * D * 8, hipMemcpyDeviceToDevice, st));
    DROP_HIP(hipMemcpyAsync(g1 + p * D * 3, ts.g + o * D * 3, (q - p) * D * 24, hipMemcpyDeviceToDevice, st));
    p = q;
  }
  int slot = ktime_begin(ctx);
  {
    RemoveCompactArgs a;
    a.src = ctx->K; a.dst = Kn; a.V = V; a.kept_old = d_map; a.rem_old = d_map + M1;
    a.lds = ld0; a.ldd = ld1; a.ldv = ldv; a.n1 = n1;
    a.n3 = (int)n3; a.M1 = (int)M1; a.m = (int)m; a.w = (int)w; a.wp = (int)wp;
    int64_t grid = (n1 + 1) / 2;
    if (grid > 64 * (int64_t)ctx->num_cus) grid = 64 * (int64_t)ctx->num_cus;
    hipLaunchKernelGGL(remove_compact_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
    ctx->launch_counter++;
  }
  ktime_end(ctx, slot, "remove_compact", ((double)n1 * (double)(n1 + 1) + 2.0 * (double)n1 * (double)ldv) * 8.0);  // bytes read + written
  DROP_HIP(hipGetLastError());

  for (int64_t g = nsl - 1; g >= 0; --g) {
    // rows above the first kept column behind the slice's first removed point are zero in the slice
    const int64_t t0 = g * w / n3, cstart = ((int64_t)map[(size_t)(M1 + t0)] - t0) * n3;
    if (cstart >= n1) continue;  // only kept points in front of it: its columns of V are zero, the rows are simply cut off
    for (int64_t k = cstart / 64 * 64; k < n1; k += 64) {
      const int64_t wk = n1 - k < 64 ? n1 - k : 64, below = n1 - (k + wk);
      slot = ktime_begin(ctx);
      RemovePanelArgs pa;
      pa.L = Kn; pa.V = V; pa.U = Ub; pa.T = Tb; pa.sgn = sgb; pa.flag = ctx->d_info;
      pa.ld = ld1; pa.ldv = ldv; pa.k = k; pa.wk = (int)wk; pa.voff = (int)(g * wp); pa.wp = (int)wp; pa.below = below > 0;
      hipLaunchKernelGGL(remove_panel_kernel, dim3(1), dim3(256), (size_t)lds_panel, st, pa);
      ctx->launch_counter++;
      ktime_end(ctx, slot, "remove_panel", 2.0 * (double)wk * (double)wk * (double)wp + (double)wk * (double)wk * (double)(wp + 22));
      if (below > 0) {
        slot = ktime_begin(ctx);
        RemoveApplyArgs aa;
        aa.L = Kn; aa.V = V; aa.U = Ub; aa.T = Tb; aa.sgn = sgb;
        aa.ld = ld1; aa.ldv = ldv; aa.k = k; aa.r0 = k + wk; aa.n1 = n1; aa.voff = (int)(g * wp); aa.wp = (int)wp;
        int64_t grid = (below + 63) / 64;
        if (grid > ctx->num_cus) grid = ctx->num_cus;
        hipLaunchKernelGGL(remove_apply_kernel, dim3((unsigned)grid), dim3(256), (size_t)lds_apply, st, aa);
        ctx->launch_counter++;
        ktime_end(ctx, slot, "remove_apply", (double)below * (256.0 * (double)wp + 5120.0));  // two 64 x wp products, the triangle of T
      }
    }
    DROP_HIP(hipGetLastError());
    if (ctx->profiling) DROP_TRY(ktime_collect(ctx));  // (a sweep is up to 2000 timed launches: their events go back to the pool)
  }
  int flag = 0;
  DROP_HIP(hipMemcpyAsync(&flag, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, st));
  DROP_TRY(phase_end(ctx, "remove"));
  DROP_HIP(hipStreamSynchronize(st));
  if (flag != 0) {
    if (info) *info = flag;
    return drop(gdml_fail(ctx, GDML_ERR_NOT_PD, "gdml_factor_remove: column %d of the reduced factor has no positive finite diagonal entry", flag));
  }

  // ---- commit
  (void)ctx_free(ctx, ws);
  factor_commit(ctx, Kn, Kn_bytes, n1, ld1, x1, g1, M1);
  return GDML_OK;
}
