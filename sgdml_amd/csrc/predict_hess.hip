// Analytic Hessians (force constants) of the sGDML energy on gfx950: H' = d^2 E' / dR^2 of the unscaled predictor.
// The reference has no counterpart (its users take finite differences of predict()).
//
// Symbols as in predict.hip.  Query descriptor x (D = N (N - 1) / 2 entries), pair k = (i_k > j_k), x_k = 1/|r_k|,
// g_k = r_k x_k^3 (desc_kernel), J_x the D x 3N Jacobian (dx_k/dr_i = -g_k, dx_k/dr_j = +g_k).  Per table row rho = (m, p):
//   d = x - X_rho, n = sqrt5 |d|, b = 5/(3 sig^3) exp(-n/sig), a = d . v_rho, e_rho = aE (0 without energy constraints)
//   grad^2_x E' = sum_rho [ gam d d^T + s (v d^T + d v^T) ] + tau I
//     s = -(5/sig) b,  gam = 25 a b / (sig^2 n) + (5/sig) e_rho b   (first term 0 at n = 0, where d = 0 as well)
//     tau = sum_rho [ -(5/sig) a b - e_rho b (n + sig) ]
// With u = J_x^T d and w = J_x^T v (3N each):
//   H' = sum_rho [ gam u u^T + s (w u^T + u w^T) ] + tau J_x^T J_x - sum_k F_x[k] grad^2_R x_k,
// grad^2_R x_k = [[Q, -Q], [-Q, Q]] on the atom pair (i_k, j_k), Q = 3 g g^T / x - x^3 I3.
//
// Pipeline of hess_device (all fp64, no atomics: every sum runs in a fixed order, so a call is bit-reproducible):
//   hess_proj_kernel<KT>  one workgroup per (query, group of RG rows of a chunk; later chunks add onto the first chunk's
//                         group partials): per row the coefficient pass (|d|^2 and a as
//                         block reductions, then b, gam, s), the partials of E', tau and F_x (F_x in registers, KT = D/256
//                         entries per thread; KT = 0: in the group's partial row in memory), and the two projections
//                         u, w -> the panels U, W (rows of the chunk x ld, ld = 3N padded to 64), gam and s per row.
//                         d (and v while 2 D doubles fit) sit in LDS for the projection's gathers.
//   hess_rank2_kernel     one workgroup per (lower 64 x 64 tile of H, query, row split): H_tile += [gam u + s w | s u]^T [u | w]
//                         over the split's rows, K = 2 x 16 rows per LDS stage, 4 x 4 accumulators per thread.  The split's
//                         partial H lives in the workspace and is added to chunk after chunk (the table rows are processed
//                         in chunks so that U and W stay bounded).
//   hess_fx_kernel        per query: the group partials of F_x, E', tau summed in order; F = J_x^T F_x.
//   hess_epilogue_kernel  per (16-row block of H, query): split partials summed in order, + tau J_x^T J_x - sum F_x grad^2 x
//                         (both block-sparse), the lower triangle mirrored; H written (B, 3N, 3N) row-major, both triangles.
// Which projection variant serves a call, the slices, chunks, groups and splits, and the workspace: hess_plan.h.
#include "common.h"
#include "hess_plan.h"

namespace {

struct HessProjArgs {
  const double* xq;   // (bs, D)
  const double* gq;   // (bs, D, 3)
  const double* xp;   // (MP, D)
  const double* jap;  // (MP, D)
  const double* aE;   // (MP) or null
  int D, N, n3, ld, RG, bs, v_lds;
  double sig;
  int64_t r0, nr, nr_cap;
  double* U;          // (bs, nr_cap, ld)
  double* W;
  double* cs;         // (bs, nr_cap, 2): gam, s
  double* part_F;     // (G, bs, D)
  double* part_ET;    // (G, bs, 2): E', tau
};

template <int KT>
__global__ void __launch_bounds__(256) hess_proj_kernel(HessProjArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q = blockIdx.y;
  const int64_t lg = blockIdx.x, gg = lg;
  const bool acc = A.r0 > 0;  // later chunks add onto the group partials of the earlier ones
  const int64_t rl0 = lg * A.RG;
  const int64_t rl1 = (rl0 + A.RG < A.nr) ? rl0 + A.RG : A.nr;
  const int D = A.D, N = A.N;
  double* sd = lds;
  double* sv = lds + D;
  const double* xq = A.xq + (int64_t)q * D;
  const double* gq = A.gq + (int64_t)q * 3 * D;
  double* pF = A.part_F + (gg * A.bs + q) * D;
  const double sig = A.sig;
  const double sqrt5 = 2.23606797749978969641;
  const double fact = 5.0 / (3.0 * sig * sig * sig);
  const double dscale = 5.0 / sig;
  constexpr int KR = KT > 0 ? KT : 1;
  double xr[KR], fx[KR];
  if constexpr (KT > 0) {
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const int k = tid + 256 * t;
      xr[t] = k < D ? xq[k] : 0.0;
      fx[t] = 0.0;
    }
  } else if (!acc) {
    for (int k = tid; k < D; k += 256) pF[k] = 0.0;
  }
  double eacc = 0.0, tacc = 0.0;
  for (int64_t rl = rl0; rl < rl1; ++rl) {
    const int64_t r = A.r0 + rl;
    const double* X = A.xp + r * D;
    const double* V = A.jap + r * D;
    const double* vs = A.v_lds ? sv : V;
    double ps = 0.0, pa = 0.0;
    if constexpr (KT > 0) {
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        const int k = tid + 256 * t;
        if (k < D) {
          const double d = xr[t] - X[k], v = V[k];
          sd[k] = d;
          if (A.v_lds) sv[k] = v;
          ps += d * d;
          pa += d * v;
        }
      }
    } else {
      for (int k = tid; k < D; k += 256) {
        const double d = xq[k] - X[k], v = V[k];
        sd[k] = d;
        if (A.v_lds) sv[k] = v;
        ps += d * d;
        pa += d * v;
      }
    }
    ps = wave_sum(ps);
    pa = wave_sum(pa);
    if (lane == 0) {
      red[0][wv] = ps;
      red[1][wv] = pa;
    }
    __syncthreads();
    const double s2 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const double a = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const double ae = A.aE ? A.aE[r] : 0.0;
    const double nn = sqrt5 * sqrt(s2);
    const double ex = exp(-nn / sig);
    const double b = fact * ex;
    const double nps = nn + sig;
    const double c1 = dscale * a * b + ae * b * nps;  // F_x += c1 d + c2 v
    const double c2 = -b * nps;
    const double gam = (nn > 0.0 ? 25.0 * a * b / (sig * sig * nn) : 0.0) + dscale * ae * b;
    const double sc = -dscale * b;
    eacc += a * b * nps + ae * (1.0 + nn / sig + nn * nn / (3.0 * sig * sig)) * ex;
    tacc += -dscale * a * b - ae * b * nps;
    if constexpr (KT > 0) {
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        const int k = tid + 256 * t;
        if (k < D) fx[t] += c1 * sd[k] + c2 * vs[k];
      }
    } else {
      for (int k = tid; k < D; k += 256) pF[k] += c1 * sd[k] + c2 * vs[k];
    }
    double* Ur = A.U + ((int64_t)q * A.nr_cap + rl) * A.ld;
    double* Wr = A.W + ((int64_t)q * A.nr_cap + rl) * A.ld;
    for (int col = tid; col < A.ld; col += 256) {
      double u = 0.0, w = 0.0;
      if (col < A.n3) {
        const int at = col / 3, c = col - 3 * at;
        for (int m = 0; m < N; ++m) {
          if (m == at) continue;
          const int k = pair_idx(at, m);
          const double gv = gq[k * 3 + c];
          const double gs = at < m ? gv : -gv;
          u += gs * sd[k];
          w += gs * vs[k];
        }
      }
      Ur[col] = u;
      Wr[col] = w;
    }
    if (tid == 0) {
      A.cs[((int64_t)q * A.nr_cap + rl) * 2] = gam;
      A.cs[((int64_t)q * A.nr_cap + rl) * 2 + 1] = sc;
    }
    __syncthreads();  // sd, sv and red are rewritten by the next row
  }
  if constexpr (KT > 0) {
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const int k = tid + 256 * t;
      if (k < D) pF[k] = acc ? pF[k] + fx[t] : fx[t];
    }
  }
  if (tid == 0) {
    double* pe = A.part_ET + (gg * A.bs + q) * 2;
    pe[0] = acc ? pe[0] + eacc : eacc;
    pe[1] = acc ? pe[1] + tacc : tacc;
  }
}

// Small descriptors (D <= 512): one wavefront per row group, four groups per workgroup, so that four table rows are in
// flight per workgroup without block barriers.  Per lane KPL = D / 64 descriptor entries (x in registers, d and v in the
// wavefront's LDS rows); reductions are cross-lane shuffles.  Same outputs as hess_proj_kernel, group = wavefront.
template <int KPL>
__global__ void __launch_bounds__(256) hess_proj_wave_kernel(HessProjArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q = blockIdx.y;
  const int64_t lg = (int64_t)blockIdx.x * 4 + wv, gg = lg;
  const bool acc = A.r0 > 0;
  const int64_t rl0 = lg * A.RG;
  if (rl0 >= A.nr) return;  // no block barriers below: a wavefront without rows may leave
  const int64_t rl1 = (rl0 + A.RG < A.nr) ? rl0 + A.RG : A.nr;
  const int D = A.D, N = A.N;
  double* sd = lds + (size_t)wv * 2 * D;
  double* sv = sd + D;
  const double* xq = A.xq + (int64_t)q * D;
  const double* gq = A.gq + (int64_t)q * 3 * D;
  const double sig = A.sig;
  const double sqrt5 = 2.23606797749978969641;
  const double fact = 5.0 / (3.0 * sig * sig * sig);
  const double dscale = 5.0 / sig;
  double xr[KPL], fx[KPL];
#pragma unroll
  for (int t = 0; t < KPL; ++t) {
    const int k = lane + 64 * t;
    xr[t] = k < D ? xq[k] : 0.0;
    fx[t] = 0.0;
  }
  double eacc = 0.0, tacc = 0.0;
  for (int64_t rl = rl0; rl < rl1; ++rl) {
    const int64_t r = A.r0 + rl;
    const double* X = A.xp + r * D;
    const double* V = A.jap + r * D;
    double ps = 0.0, pa = 0.0;
#pragma unroll
    for (int t = 0; t < KPL; ++t) {
      const int k = lane + 64 * t;
      if (k < D) {
        const double d = xr[t] - X[k], v = V[k];
        sd[k] = d;
        sv[k] = v;
        ps += d * d;
        pa += d * v;
      }
    }
    const double s2 = wave_sum(ps);
    const double a = wave_sum(pa);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const double ae = A.aE ? A.aE[r] : 0.0;
    const double nn = sqrt5 * sqrt(s2);
    const double ex = exp(-nn / sig);
    const double b = fact * ex;
    const double nps = nn + sig;
    const double c1 = dscale * a * b + ae * b * nps;
    const double c2 = -b * nps;
    const double gam = (nn > 0.0 ? 25.0 * a * b / (sig * sig * nn) : 0.0) + dscale * ae * b;
    const double sc = -dscale * b;
    eacc += a * b * nps + ae * (1.0 + nn / sig + nn * nn / (3.0 * sig * sig)) * ex;
    tacc += -dscale * a * b - ae * b * nps;
#pragma unroll
    for (int t = 0; t < KPL; ++t) {
      const int k = lane + 64 * t;
      if (k < D) fx[t] += c1 * sd[k] + c2 * sv[k];
    }
    double* Ur = A.U + ((int64_t)q * A.nr_cap + rl) * A.ld;
    double* Wr = A.W + ((int64_t)q * A.nr_cap + rl) * A.ld;
    for (int col = lane; col < A.ld; col += 64) {
      double u = 0.0, w = 0.0;
      if (col < A.n3) {
        const int at = col / 3, c = col - 3 * at;
        for (int m = 0; m < N; ++m) {
          if (m == at) continue;
          const int k = pair_idx(at, m);
          const double gv = gq[k * 3 + c];
          const double gs = at < m ? gv : -gv;
          u += gs * sd[k];
          w += gs * sv[k];
        }
      }
      Ur[col] = u;
      Wr[col] = w;
    }
    if (lane == 0) {
      A.cs[((int64_t)q * A.nr_cap + rl) * 2] = gam;
      A.cs[((int64_t)q * A.nr_cap + rl) * 2 + 1] = sc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // sd / sv are rewritten by the next row
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  double* pF = A.part_F + (gg * A.bs + q) * D;
#pragma unroll
  for (int t = 0; t < KPL; ++t) {
    const int k = lane + 64 * t;
    if (k < D) pF[k] = acc ? pF[k] + fx[t] : fx[t];
  }
  if (lane == 0) {
    double* pe = A.part_ET + (gg * A.bs + q) * 2;
    pe[0] = acc ? pe[0] + eacc : eacc;
    pe[1] = acc ? pe[1] + tacc : tacc;
  }
}

struct HessRank2Args {
  const double* U;
  const double* W;
  const double* cs;
  int64_t nr, nr_cap, rps;
  int ld, bs, accumulate;
  double* Hp;  // (JS, bs, ld, ld)
};

// lower tile pair p -> (bi >= bj)
__device__ __forceinline__ void tile_pair(int p, int& bi, int& bj) {
  int i = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while (i * (i + 1) / 2 > p) --i;
  while ((i + 1) * (i + 2) / 2 <= p) ++i;
  bi = i;
  bj = p - i * (i + 1) / 2;
}

__global__ void __launch_bounds__(256) hess_rank2_kernel(HessRank2Args A) {
  __shared__ double la1[HK][HT], la2[HK][HT], lb1[HK][HT], lb2[HK][HT];
  int bi, bj;
  tile_pair(blockIdx.x, bi, bj);
  const int q = blockIdx.y, js = blockIdx.z;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int I0 = bi * HT, J0 = bj * HT;
  const int64_t k0 = (int64_t)js * A.rps;
  const int64_t k1 = (k0 + A.rps < A.nr) ? k0 + A.rps : A.nr;
  const double* Uq = A.U + (int64_t)q * A.nr_cap * A.ld;
  const double* Wq = A.W + (int64_t)q * A.nr_cap * A.ld;
  const double* cq = A.cs + (int64_t)q * A.nr_cap * 2;
  double acc[4][4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = 0.0;
  for (int64_t kk = k0; kk < k1; kk += HK) {
#pragma unroll
    for (int e0 = 0; e0 < HK * HT; e0 += 256) {
      const int e = e0 + tid, r = e / HT, c = e - r * HT;
      const int64_t rr = kk + r;
      double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
      if (rr < k1) {
        const double* u = Uq + rr * A.ld;
        const double* w = Wq + rr * A.ld;
        const double gm = cq[rr * 2], s = cq[rr * 2 + 1];
        const double ui = u[I0 + c], wi = w[I0 + c];
        a1 = gm * ui + s * wi;
        a2 = s * ui;
        b1 = u[J0 + c];
        b2 = w[J0 + c];
      }
      la1[r][c] = a1;
      la2[r][c] = a2;
      lb1[r][c] = b1;
      lb2[r][c] = b2;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < HK; ++r) {
      double x1[4], x2[4], y1[4], y2[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        x1[t] = la1[r][ty + 16 * t];
        x2[t] = la2[r][ty + 16 * t];
        y1[t] = lb1[r][tx + 16 * t];
        y2[t] = lb2[r][tx + 16 * t];
      }
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = fma(x2[ii], y2[jj], fma(x1[ii], y1[jj], acc[ii][jj]));
    }
    __syncthreads();
  }
  double* H = A.Hp + ((int64_t)js * A.bs + q) * A.ld * A.ld;
#pragma unroll
  for (int ii = 0; ii < 4; ++ii)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int64_t o = (int64_t)(I0 + ty + 16 * ii) * A.ld + (J0 + tx + 16 * jj);
      H[o] = A.accumulate ? H[o] + acc[ii][jj] : acc[ii][jj];
    }
}

// per query: F_x, E', tau from the group partials (fixed order); F = J_x^T F_x
__global__ void __launch_bounds__(256) hess_fx_kernel(const double* __restrict__ part_F, const double* __restrict__ part_ET,
                                                      int64_t G, int bs, int N, int D, const double* __restrict__ gq,
                                                      double* fx, double* __restrict__ tau, double* __restrict__ E_out,
                                                      double* __restrict__ F_out) {
  const int q = blockIdx.x, tid = threadIdx.x;
  double* f = fx + (int64_t)q * D;
  for (int k = tid; k < D; k += 256) f[k] = sum_in_order8(G, [&](int64_t g) { return part_F[(g * bs + q) * D + k]; });
  if (tid == 0) {
    double e = 0.0, t = 0.0;
    for (int64_t g = 0; g < G; ++g) {
      e += part_ET[(g * bs + q) * 2];
      t += part_ET[(g * bs + q) * 2 + 1];
    }
    tau[q] = t;
    if (E_out) E_out[q] = e;
  }
  __syncthreads();  // f is read across the workgroup below
  if (!F_out) return;
  const double* g = gq + (int64_t)q * 3 * D;
  for (int t = tid; t < 3 * N; t += 256) {
    const int a = t / 3, al = t - 3 * a;
    double s = 0.0;
    for (int m = 0; m < N; ++m) {
      if (m == a) continue;
      const int k = pair_idx(a, m);
      const double v = g[k * 3 + al] * f[k];
      s += (a < m) ? v : -v;
    }
    F_out[(int64_t)q * 3 * N + t] = s;
  }
}

__global__ void __launch_bounds__(256) hess_epilogue_kernel(const double* __restrict__ Hp, int JS, int bs, int ld, int N,
                                                            int D, const double* __restrict__ xq,
                                                            const double* __restrict__ gq, const double* __restrict__ fx,
                                                            const double* __restrict__ tau, double* __restrict__ H_out) {
  const int bi = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  const int n3 = 3 * N, I0 = bi * HE;
  const int rows = (n3 - I0 < HE) ? n3 - I0 : HE;
  const double* x = xq + (int64_t)q * D;
  const double* g = gq + (int64_t)q * 3 * D;
  const double* f = fx + (int64_t)q * D;
  const double tq = tau[q];
  double* H = H_out + (int64_t)q * n3 * n3;
  for (int e = tid; e < rows * n3; e += 256) {
    const int il = e / n3, j = e - il * n3, i = I0 + il;
    if (j > i) continue;
    const double s = sum_in_order8(JS, [&](int js) { return Hp[(((int64_t)js * bs + q) * ld + i) * ld + j]; });
    const int a = i / 3, c = i - 3 * a, bb = j / 3, c2 = j - 3 * bb;
    double extra = 0.0;
    if (a == bb) {
      for (int m = 0; m < N; ++m) {
        if (m == a) continue;
        const int k = pair_idx(a, m);
        const double gc = g[k * 3 + c], gd = g[k * 3 + c2], xk = x[k];
        const double Q = 3.0 * gc * gd / xk - (c == c2 ? xk * xk * xk : 0.0);
        extra += tq * gc * gd - f[k] * Q;
      }
    } else {
      const int k = pair_idx(a, bb);
      const double gc = g[k * 3 + c], gd = g[k * 3 + c2], xk = x[k];
      const double Q = 3.0 * gc * gd / xk - (c == c2 ? xk * xk * xk : 0.0);
      extra = -tq * gc * gd + f[k] * Q;
    }
    const double v = s + extra;
    H[(int64_t)i * n3 + j] = v;
    H[(int64_t)j * n3 + i] = v;
  }
}

}  // namespace

// the projection kernel of a plan: one pointer for hipFuncSetAttribute and for the launches; null for a selector no kernel has
typedef void (*HessProjFn)(HessProjArgs);
static HessProjFn hess_proj_fn(const HessPlan& p) {
  if (p.variant == HESS_WAVE) {  // D <= 512: KPL <= 8
    switch (p.sel) {
      case 1: return hess_proj_wave_kernel<1>;
      case 2: return hess_proj_wave_kernel<2>;
      case 4: return hess_proj_wave_kernel<4>;
      case 8: return hess_proj_wave_kernel<8>;
    }
  } else {  // D > 512 (KT >= 4), or forced KT = 0
    switch (p.sel) {
      case 0: return hess_proj_kernel<0>;
      case 4: return hess_proj_kernel<4>;
      case 8: return hess_proj_kernel<8>;
      case 16: return hess_proj_kernel<16>;
      case 32: return hess_proj_kernel<32>;
      case 48: return hess_proj_kernel<48>;
    }
  }
  return nullptr;
}

// Plan (hess_plan.h) -> workspace -> per batch slice: per row chunk projection and rank-2 update, then F_x and the epilogue.
int hess_device(gdml_ctx* ctx, const double* d_xq, const double* d_gq, int64_t B, double* d_E, double* d_F, double* d_H) {
  Model& md = ctx->model;
  if (!md.xp) return gdml_fail(ctx, GDML_ERR_STATE, "hessian: no model resident");
  if (B == 0) return GDML_OK;
  const int N = md.N, D = md.D, n3 = 3 * N;
  const int64_t MP = md.M * md.P;
  HessPlanIn in;
  in.N = N; in.MP = MP; in.B = B;
  in.generic = ctx_opt_i(ctx, "predict.hess_generic", 0);
  in.chunk_rows = ctx_opt_i(ctx, "predict.hess_chunk_rows", 0);
  const HessPlan p = hess_plan(in);
  if (!p.supported)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "hessian: N = %d beyond the LDS row of the projection (N <= 197)", N);

  double* ws;
  GDML_TRY(ctx_slot(ctx, SLOT_PREDICT_WS, p.ws_bytes, &ws));
  const struct { double *U, *W, *cs, *part_F, *part_ET, *Hp, *fx, *tau; } w = {
      ws, ws + p.oW, ws + p.oCS, ws + p.oPF, ws + p.oPE, ws + p.oHp, ws + p.oFX, ws + p.oTau};

  const HessProjFn proj = hess_proj_fn(p);
  if (!proj)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, p.variant == HESS_WAVE ? "hessian: bad lane tile %d" : "hessian: bad register tile %d",
                     p.sel);
  if (p.lds_bytes > 64 * 1024)
    HIP_CHECK(ctx, hipFuncSetAttribute((const void*)proj, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));

  for (int64_t b0 = 0; b0 < B; b0 += p.Bs) {
    const int bs = p.slice(b0);
    const double* xq = d_xq + b0 * D;
    const double* gq = d_gq + b0 * 3 * D;
    const int slot = ktime_begin(ctx);
    for (int64_t r0 = 0; r0 < MP; r0 += p.nr_cap) {
      const HessChunk c = p.chunk(r0);
      HessProjArgs P;
      P.xq = xq; P.gq = gq; P.xp = md.xp; P.jap = md.jap; P.aE = md.has_aE ? md.aE : nullptr;
      P.D = D; P.N = N; P.n3 = n3; P.ld = p.ld; P.RG = p.RG; P.bs = bs; P.v_lds = p.v_lds; P.sig = md.sig;
      P.r0 = r0; P.nr = c.nr; P.nr_cap = p.nr_cap;
      P.U = w.U; P.W = w.W; P.cs = w.cs; P.part_F = w.part_F; P.part_ET = w.part_ET;
      hipLaunchKernelGGL(proj, dim3(c.grid_x, (unsigned)bs), dim3(256), p.lds_bytes, ctx->stream, P);
      HessRank2Args R2;
      R2.U = w.U; R2.W = w.W; R2.cs = w.cs; R2.nr = c.nr; R2.nr_cap = p.nr_cap; R2.rps = c.rps;
      R2.ld = p.ld; R2.bs = bs; R2.accumulate = c.accumulate; R2.Hp = w.Hp;
      hipLaunchKernelGGL(hess_rank2_kernel, dim3((unsigned)p.n_tp, (unsigned)bs, (unsigned)p.JS), dim3(256), 0, ctx->stream, R2);
      ctx->launch_counter += 2;
    }
    hipLaunchKernelGGL(hess_fx_kernel, dim3((unsigned)bs), dim3(256), 0, ctx->stream, w.part_F, w.part_ET, p.G, bs, N, D, gq, w.fx,
                       w.tau, d_E ? d_E + b0 : nullptr, d_F ? d_F + b0 * n3 : nullptr);
    hipLaunchKernelGGL(hess_epilogue_kernel, dim3((unsigned)((n3 + HE - 1) / HE), (unsigned)bs), dim3(256), 0, ctx->stream, w.Hp,
                       (int)p.JS, bs, p.ld, N, D, xq, gq, w.fx, w.tau, d_H + b0 * n3 * (int64_t)n3);
    ctx->launch_counter += 2;
    // algorithmic work per Hessian and table row: rank-2 update 36 N^2, projections 24 D, coefficients and F_x 9 D
    ktime_end(ctx, slot, "hessian", (double)bs * (double)MP * (36.0 * N * (double)N + 33.0 * D));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gdml_fail(ctx, GDML_ERR_HIP, "hessian launch: %s", hipGetErrorString(e));
  }
  return GDML_OK;
}

static int hess_common(gdml_ctx* ctx, const double* R, bool on_device, int64_t B, const double* lat, const double* lat_inv,
                       double* E_out, double* F_out, double* H_out) {
  Model& md = ctx->model;
  if (!md.xp) return gdml_fail(ctx, GDML_ERR_STATE, "gdml_predict_hessian: upload a model first");
  if (!R) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_predict_hessian: R is NULL (no training-set mode)");
  if (!H_out) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_predict_hessian: H_out is NULL");
  if ((lat == nullptr) != (lat_inv == nullptr))
    return gdml_fail(ctx, GDML_ERR_INVALID, "lattice and inverse must both be given or both NULL");
  if (B < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_predict_hessian: B < 0");
  if (B == 0) return GDML_OK;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int N = md.N, D = md.D;
  const int64_t n3 = 3 * (int64_t)N;
  const int64_t nR = B * n3, nx = B * (int64_t)D, ng = 3 * nx, nout = on_device ? 0 : B + nR + B * n3 * n3;
  double* buf;
  GDML_TRY(ctx_scratch(ctx, (nR + nx + ng + nout) * 8, &buf));
  double* d_R = buf;
  double* dx = d_R + nR;
  double* dg = dx + nx;
  double *d_E = E_out, *d_F = F_out, *d_H = H_out;
  if (!on_device) {
    d_E = dg + ng;
    d_F = d_E + B;
    d_H = d_F + nR;
    HIP_CHECK(ctx, hipMemcpyAsync(d_R, R, nR * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  phase_begin(ctx);
  GDML_TRY(desc_device(ctx, on_device ? R : d_R, B, N, lat, lat_inv, dx, dg));
  GDML_TRY(hess_device(ctx, dx, dg, B, (E_out || !on_device) ? d_E : nullptr, (F_out || !on_device) ? d_F : nullptr, d_H));
  GDML_TRY(phase_end(ctx, "hessian"));
  if (!on_device) {
    if (E_out) HIP_CHECK(ctx, hipMemcpyAsync(E_out, d_E, B * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (F_out) HIP_CHECK(ctx, hipMemcpyAsync(F_out, d_F, nR * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipMemcpyAsync(H_out, d_H, B * n3 * n3 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GDML_OK;
}

extern "C" int gdml_predict_hessian(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv,
                                    double* E_out, double* F_out, double* H_out) {
  if (!ctx) return GDML_ERR_INVALID;
  return hess_common(ctx, R, false, B, lat, lat_inv, E_out, F_out, H_out);
}

extern "C" int gdml_predict_hessian_dev(gdml_ctx* ctx, const double* R_dev, int64_t B, const double* lat,
                                        const double* lat_inv, double* E_dev, double* F_dev, double* H_dev) {
  if (!ctx) return GDML_ERR_INVALID;
  return hess_common(ctx, R_dev, true, B, lat, lat_inv, E_dev, F_dev, H_dev);
}
