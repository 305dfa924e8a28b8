// ------------------------------------------------------------------------------------------
// Harmonic vibrational analysis (gdml_vib_run) and the spectrum of a slice of geometries under it, which eigenvector following
// (gdml_ef_run, ef.hip) runs as it is.  The contract; include/gdml_hip.h and tests/_vib_ref.py state the same.
//   Per chunk of geometries, everything on the device (spectrum_slice):
//   a. H' of the chunk (gdml_predict_hessian_dev), E', F unscaled
//   b. vib_project_kernel, one workgroup per geometry, in place on H':
//        D_ij = h_scale sym(H')_ij / (sqrt m_i sqrt m_j)
//        rigid candidates in mass-weighted coordinates, in this order: translations sqrt(m_i) e_c, c = x, y, z (project >= 1);
//        rotations sqrt(m_i) (e_c x (r_i - r_cm)), c = x, y, z (project = 2); modified Gram-Schmidt in that order, a candidate
//        whose remainder has a squared norm below 1e-10 of its own (or that is zero) is dropped -> Q (n_rigid rows)
//        Y = D Q, S = sym(Q^T Y), Z = Y - Q S / 2:   P D P = D - Q Z^T - Z Q^T   (P = I - Q Q^T)
//        D_s = P D P + Lambda Q Q^T,  Lambda = 2 |P D P|_F (1 if that is 0): the rigid modes are exact eigenvectors at Lambda,
//        every vibration has |lambda| <= |P D P|_2 < Lambda
//      every sum in a fixed order (per-thread partial sums in index order, then the 256-slot tree; wavefront sums by the xor
//      butterfly); the upper triangle is computed and mirrored, so D_s is symmetric bit for bit.  No atomics.
//   c. the eigensolver on D_s (sym_eig.hip: eigenvalues ascending, signed eigenvectors as rows), the eigenvectors over D_s in place
//   d. vib_finish_kernel: the last n_rigid eigenvalues (those at Lambda) become exactly 0, n_neg counts the others below
//      -tau, tau = 3N eps |D_s|_F
// The chunk length, the eigensolver's plan and the layout of a chunk's workspace are sym_eig_plan.h's.
// ------------------------------------------------------------------------------------------
#include <float.h>
#include <math.h>

#include "vib.h"

namespace {

constexpr int VIB_MAX_RIGID = 6;

struct VibProjArgs {
  double* H;           // (B, n3, n3): H' in, D_s out
  const double* R;     // (B, n3)
  const double* mass;  // (N)
  double* info;        // (B, 4) out: n_rigid, Lambda, |D_s|_F, |P D P|_F
  double h_scale;
  int N, n3, project;
};

// dynamic LDS: Q [6][n3] | Z [6][n3] | sw [n3] | red [256] | S [36]
static inline size_t vib_proj_lds(int n3) { return (size_t)(13 * n3 + 256 + 36) * 8; }

__global__ void __launch_bounds__(256) vib_project_kernel(VibProjArgs A) {
  extern __shared__ __attribute__((aligned(8))) unsigned char vib_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = A.N, n3 = A.n3;
  double* Q = reinterpret_cast<double*>(vib_raw);
  double* Z = Q + VIB_MAX_RIGID * n3;
  double* sw = Z + VIB_MAX_RIGID * n3;
  double (*red)[256] = reinterpret_cast<double (*)[256]>(sw + n3);
  double* Sm = sw + n3 + 256;
  double* Hq = A.H + (int64_t)blockIdx.x * n3 * n3;
  const double* r = A.R + (int64_t)blockIdx.x * n3;

  for (int i = tid; i < n3; i += 256) sw[i] = sqrt(A.mass[i / 3]);
  for (int e = tid; e < VIB_MAX_RIGID * n3; e += 256) Q[e] = 0.0;
  __syncthreads();
  // D = h_scale sym(H') / (sqrt m_i sqrt m_j), upper triangle computed, mirrored
  for (int e = tid; e < n3 * n3; e += 256) {
    const int i = e / n3, j = e - i * n3;
    if (j < i) continue;
    const double d = A.h_scale * (0.5 * (Hq[i * n3 + j] + Hq[j * n3 + i])) / (sw[i] * sw[j]);
    Hq[i * n3 + j] = d;
    Hq[j * n3 + i] = d;
  }
  __threadfence_block();
  __syncthreads();

  // rigid basis: candidates in a fixed order, modified Gram-Schmidt, rank rule
  int k = 0;
  double cm[3] = {0.0, 0.0, 0.0};
  if (A.project == 2) {
    double pm = 0.0, px = 0.0, py = 0.0, pz = 0.0;
    for (int a = tid; a < N; a += 256) {
      const double m = A.mass[a];
      pm += m; px += m * r[3 * a]; py += m * r[3 * a + 1]; pz += m * r[3 * a + 2];
    }
    const double mt = vib_sum(red, tid, pm);
    cm[0] = vib_sum(red, tid, px) / mt;
    cm[1] = vib_sum(red, tid, py) / mt;
    cm[2] = vib_sum(red, tid, pz) / mt;
  }
  const int n_cand = A.project == 2 ? 6 : A.project == 1 ? 3 : 0;
  for (int cand = 0; cand < n_cand; ++cand) {
    double* v = Q + k * n3;
    const int c = cand % 3;
    double p2 = 0.0;
    for (int i = tid; i < n3; i += 256) {
      const int a = i / 3, x = i - 3 * a;
      double val;
      if (cand < 3) {
        val = x == c ? sw[i] : 0.0;
      } else {
        // (e_c x d)[x], d = r_a - r_cm: component x = c vanishes, x = c + 1 gets -d[c + 2], x = c + 2 gets d[c + 1] (mod 3)
        const int x1 = (c + 1) % 3, x2 = (c + 2) % 3;
        val = x == x1 ? -(r[3 * a + x2] - cm[x2]) : x == x2 ? (r[3 * a + x1] - cm[x1]) : 0.0;
        val *= sw[i];
      }
      v[i] = val;
      p2 += val * val;
    }
    const double orig2 = vib_sum(red, tid, p2);
    for (int b = 0; b < k; ++b) {
      const double* q = Q + b * n3;
      double pd = 0.0;
      for (int i = tid; i < n3; i += 256) pd += q[i] * v[i];
      const double dot = vib_sum(red, tid, pd);
      for (int i = tid; i < n3; i += 256) v[i] -= dot * q[i];
    }
    p2 = 0.0;
    for (int i = tid; i < n3; i += 256) p2 += v[i] * v[i];
    const double rem2 = vib_sum(red, tid, p2);
    const bool keep = orig2 > 0.0 && rem2 >= 1e-10 * orig2;
    const double nrm = sqrt(rem2);
    for (int i = tid; i < n3; i += 256) v[i] = keep ? v[i] / nrm : 0.0;
    if (keep) ++k;
    __syncthreads();
  }

  // Y = D Q (into Z), one wavefront per row of D
  for (int i = wave; i < n3; i += 4) {
    double acc[VIB_MAX_RIGID] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < n3; j += 64) {
      const double d = Hq[i * n3 + j];
#pragma unroll
      for (int a = 0; a < VIB_MAX_RIGID; ++a) acc[a] += d * Q[a * n3 + j];
    }
#pragma unroll
    for (int a = 0; a < VIB_MAX_RIGID; ++a) {
      const double s = wave_sum(acc[a]);
      if (lane == 0) Z[a * n3 + i] = s;
    }
  }
  __syncthreads();
  // S = Q^T Y, one thread per entry, in index order
  if (tid < VIB_MAX_RIGID * VIB_MAX_RIGID) {
    const int a = tid / VIB_MAX_RIGID, b = tid - a * VIB_MAX_RIGID;
    double s = 0.0;
    for (int i = 0; i < n3; ++i) s += Q[a * n3 + i] * Z[b * n3 + i];
    Sm[tid] = s;
  }
  __syncthreads();
  // Z = Y - Q sym(S) / 2
  for (int i = tid; i < n3; i += 256) {
    double y[VIB_MAX_RIGID], q[VIB_MAX_RIGID];
#pragma unroll
    for (int a = 0; a < VIB_MAX_RIGID; ++a) { y[a] = Z[a * n3 + i]; q[a] = Q[a * n3 + i]; }
#pragma unroll
    for (int a = 0; a < VIB_MAX_RIGID; ++a) {
      double t = 0.0;
#pragma unroll
      for (int b = 0; b < VIB_MAX_RIGID; ++b) t += (0.5 * (Sm[a * VIB_MAX_RIGID + b] + Sm[b * VIB_MAX_RIGID + a])) * q[b];
      Z[a * n3 + i] = y[a] - 0.5 * t;
    }
  }
  __syncthreads();
  // P D P = D - Q Z^T - Z Q^T and its Frobenius norm
  double p2 = 0.0;
  for (int e = tid; e < n3 * n3; e += 256) {
    const int i = e / n3, j = e - i * n3;
    if (j < i) continue;
    double t = 0.0;
#pragma unroll
    for (int a = 0; a < VIB_MAX_RIGID; ++a) t += Q[a * n3 + i] * Z[a * n3 + j] + Z[a * n3 + i] * Q[a * n3 + j];
    const double x = Hq[i * n3 + j] - t;
    Hq[i * n3 + j] = x;
    Hq[j * n3 + i] = x;
    p2 += (i == j ? 1.0 : 2.0) * (x * x);
  }
  const double n_pdp = sqrt(vib_sum(red, tid, p2));
  double lambda = 0.0, n_ds = n_pdp;
  if (k > 0) {
    lambda = n_pdp > 0.0 ? 2.0 * n_pdp : 1.0;
    __threadfence_block();
    __syncthreads();
    // D_s = P D P + Lambda Q Q^T and its Frobenius norm
    p2 = 0.0;
    for (int e = tid; e < n3 * n3; e += 256) {
      const int i = e / n3, j = e - i * n3;
      if (j < i) continue;
      double t = 0.0;
#pragma unroll
      for (int a = 0; a < VIB_MAX_RIGID; ++a) t += Q[a * n3 + i] * Q[a * n3 + j];
      const double x = Hq[i * n3 + j] + lambda * t;
      Hq[i * n3 + j] = x;
      Hq[j * n3 + i] = x;
      p2 += (i == j ? 1.0 : 2.0) * (x * x);
    }
    n_ds = sqrt(vib_sum(red, tid, p2));
  }
  if (tid == 0) {
    double* o = A.info + (int64_t)blockIdx.x * 4;
    o[0] = (double)k; o[1] = lambda; o[2] = n_ds; o[3] = n_pdp;
  }
}

// one thread per geometry: rigid eigenvalues (the last n_rigid, at Lambda) to exactly 0, imaginary modes counted
__global__ void __launch_bounds__(256) vib_finish_kernel(double* w, const double* info, int64_t B, int n3, int64_t* n_rigid,
                                                         int64_t* n_neg) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int k = (int)info[4 * b];
  const double tau = (double)n3 * DBL_EPSILON * info[4 * b + 2];
  double* wb = w + b * n3;
  int64_t neg = 0;
  for (int e = 0; e < n3 - k; ++e) neg += wb[e] < -tau;
  for (int e = n3 - k; e < n3; ++e) wb[e] = 0.0;
  n_rigid[b] = k;
  n_neg[b] = neg;
}

int vib_check(gdml_ctx* ctx, const gdml_vib_params* p, const double* R, const double* masses, const double* w2,
              const int64_t* n_rigid, const int64_t* n_neg) {
  const char* fn = "gdml_vib_run";
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: params is NULL", fn);
  GDML_TRY(traj_check_shape(ctx, fn, p->B, p->N));
  GDML_TRY(spectrum_check_projection(ctx, fn, p->project, p->lat, p->lat_inv));
  if (!isfinite(p->h_scale) || !(p->h_scale > 0.0))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: h_scale must be positive and finite", fn);
  if (!masses) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: masses is NULL", fn);
  GDML_TRY(spectrum_check_atoms(ctx, fn, p->N));
  for (int a = 0; a < p->N; ++a)
    if (!(masses[a] > 0.0) || !isfinite(masses[a]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: mass of atom %d must be positive and finite", fn, a);
  if (!R || !w2 || !n_rigid || !n_neg) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: R, w2, n_rigid or n_neg is NULL", fn);
  return spectrum_check_finite(ctx, fn, p->N, p->B, R, nullptr);
}

}  // namespace

int spectrum_check_projection(gdml_ctx* ctx, const char* fn, int project, const double* lat, const double* lat_inv) {
  if (project < 0 || project > 2) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: project must be 0, 1 or 2", fn);
  GDML_TRY(traj_check_lattice(ctx, fn, lat, lat_inv));
  if (project == 2 && lat)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: project = 2 with a lattice (rotations are no symmetry of a periodic cell)", fn);
  return GDML_OK;
}

int spectrum_check_atoms(gdml_ctx* ctx, const char* fn, int N) {
  if (N > VIB_MAX_ATOMS)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "%s: N = %d beyond the Hessian's limit (N <= %d)", fn, N, VIB_MAX_ATOMS);
  return GDML_OK;
}

int spectrum_check_finite(gdml_ctx* ctx, const char* fn, int N, int64_t B, const double* R, const double* t) {
  const int64_t n3 = 3 * (int64_t)N;
  for (int64_t i = 0; i < B * n3; ++i) {
    if (!isfinite(R[i]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: coordinate %lld of geometry %lld is not finite", fn, (long long)(i % n3),
                       (long long)(i / n3));
    if (t && !isfinite(t[i]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: follow vector entry %lld of geometry %lld is not finite", fn,
                       (long long)(i % n3), (long long)(i / n3));
  }
  return GDML_OK;
}

int spectrum_slice(gdml_ctx* ctx, const SymEigPlan& plan, const Spectrum& S, const SpectrumIn& in, const double* d_R, int64_t bc) {
  const int n3 = 3 * in.N;
  hipStream_t st = ctx->stream;
  GDML_TRY(gdml_predict_hessian_dev(ctx, d_R, bc, in.lat, in.lat_inv, S.E, S.F, S.H));
  VibProjArgs A;
  A.H = S.H; A.R = d_R; A.mass = S.mass; A.info = S.info; A.h_scale = in.h_scale; A.N = in.N; A.n3 = n3; A.project = in.project;
  const size_t proj_lds = vib_proj_lds(n3);
  if (proj_lds > 48 * 1024)
    HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(vib_project_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)proj_lds));
  const int ks = ktime_begin(ctx);
  hipLaunchKernelGGL(vib_project_kernel, dim3((unsigned)bc), dim3(256), proj_lds, st, A);
  ktime_end(ctx, ks, "vib_project", (double)bc);
  HIP_CHECK(ctx, hipGetLastError());
  SymEigPlan pc = plan;
  if (pc.grid > bc) pc.grid = bc;
  HIP_CHECK(ctx, sym_eig_rows_launch(ctx, pc, S.H, bc, n3, S.w, S.H, S.sweeps, S.work));
  hipLaunchKernelGGL(vib_finish_kernel, dim3((unsigned)ceil_div(bc, 256)), dim3(256), 0, st, S.w, S.info, bc, n3, S.n_rigid, S.n_neg);
  HIP_CHECK(ctx, hipGetLastError());
  ctx->launch_counter += 2;
  return GDML_OK;
}

extern "C" int gdml_vib_run(gdml_ctx* ctx, const gdml_vib_params* p, const double* R, const double* masses, double* w2,
                            double* modes, int64_t* n_rigid, int64_t* n_neg, double* E, double* F, int64_t* sweeps) {
  GDML_TRY(vib_check(ctx, p, R, masses, w2, n_rigid, n_neg));
  bool run;
  GDML_TRY(traj_prelude(ctx, "gdml_vib_run", p->N, p->B, nullptr, &run));
  if (!run) return GDML_OK;
  const int64_t B = p->B;
  const int N = p->N, n3 = 3 * N;
  const int64_t nn = (int64_t)n3 * n3;

  const int64_t chunk = spectrum_slice_len(ctx->num_cus, B, n3, (int64_t)ctx_opt(ctx, "predict.vib_chunk", 0.0));
  const SymEigPlan plan = sym_eig_plan(ctx->num_cus, chunk, n3, true);
  const SpectrumWs ws = spectrum_ws(chunk, N, plan.work_doubles, true);
  double* buf;
  GDML_TRY(ctx_slot(ctx, SLOT_VIB_WS, ws.total * 8, &buf));
  const Spectrum S = spectrum_carve(buf, ws);
  const SpectrumIn in = {N, p->project, p->h_scale, p->lat, p->lat_inv};

  hipStream_t st = ctx->stream;
  HIP_CHECK(ctx, hipMemcpyAsync(S.mass, masses, (size_t)N * 8, hipMemcpyHostToDevice, st));
  std::vector<int64_t> h_sw((size_t)chunk);
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t bc = B - b0 < chunk ? B - b0 : chunk;
    HIP_CHECK(ctx, hipMemcpyAsync(S.R, R + b0 * n3, (size_t)(bc * n3) * 8, hipMemcpyHostToDevice, st));
    GDML_TRY(spectrum_slice(ctx, plan, S, in, S.R, bc));
    HIP_CHECK(ctx, hipMemcpyAsync(h_sw.data(), S.sweeps, (size_t)bc * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipMemcpyAsync(w2 + b0 * n3, S.w, (size_t)(bc * n3) * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipMemcpyAsync(n_rigid + b0, S.n_rigid, (size_t)bc * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipMemcpyAsync(n_neg + b0, S.n_neg, (size_t)bc * 8, hipMemcpyDeviceToHost, st));
    if (E) HIP_CHECK(ctx, hipMemcpyAsync(E + b0, S.E, (size_t)bc * 8, hipMemcpyDeviceToHost, st));
    if (F) HIP_CHECK(ctx, hipMemcpyAsync(F + b0 * n3, S.F, (size_t)(bc * n3) * 8, hipMemcpyDeviceToHost, st));
    if (modes) HIP_CHECK(ctx, hipMemcpyAsync(modes + b0 * nn, S.H, (size_t)(bc * nn) * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (sweeps) memcpy(sweeps + b0, h_sw.data(), (size_t)bc * 8);
    GDML_TRY(sym_eig_check_sweeps(ctx, "gdml_vib_run", h_sw.data(), bc, b0));
  }
  return GDML_OK;
}
