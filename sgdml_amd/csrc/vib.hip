// ------------------------------------------------------------------------------------------
// Harmonic vibrational analysis (gdml_vib_run) and the batched symmetric eigensolver under it (gdml_sym_eig, gdml_sym_eig_dev).
// The contract; include/gdml_hip.h and tests/_vib_ref.py state the same.
//   Eigensolver: one workgroup per matrix, the Jacobi sweeps, storage routes and stopping rule of sym_eig.h (the loop the
//   symmetry search runs, perm_match.hip).  Eigenvalues ascending (ties: the lower Jacobi column first), V[k][:] the unit
//   eigenvector of w[k] as a ROW, its component of largest magnitude positive (lowest index on ties).  sweeps[m] = sweeps
//   made, SYM_EIG_MAX_SWEEPS + 1 when the matrix is still above the threshold after the cap (the entries turn that into an error).
//   Vibrations, per chunk of geometries, everything on the device:
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
//   c. sym_eig_full_kernel on D_s, the eigenvectors over D_s in place
//   d. vib_finish_kernel: the last n_rigid eigenvalues (those at Lambda) become exactly 0, n_neg counts the others below
//      -tau, tau = 3N eps |D_s|_F
// Eigenvector following (gdml_ef_run) lies beside them because it runs b, c and d as they are, once per evaluation, with unit
// masses and h_scale = f_scale, and adds ONE kernel, ef_step_kernel: the step in the eigenbasis, the trust radius, the mode
// tracking and the per-geometry convergence (the contract: include/gdml_hip.h; tests/_ef_ref.py states the same).  Its driver
// is gdml_relax_run's general route: plain launches queued back to back, traj.h's chunk loop, one synchronisation per chunk.
// ------------------------------------------------------------------------------------------
#include <float.h>
#include <math.h>

#include "common.h"
#include "sym_eig.h"
#include "traj.h"

namespace {

constexpr int VIB_MAX_ATOMS = 197;               // the Hessian's own limit
constexpr int SYM_EIG_MAX_N = 3 * VIB_MAX_ATOMS;
constexpr int64_t VIB_CHUNK_BYTES = 256ll << 20;
constexpr int VIB_MAX_RIGID = 6;

struct SymEigFullArgs {
  const double* A;   // (M, N, N)
  double* w;         // (M, N) out
  double* V;         // (M, N, N) out, row k = eigenvector k; may be A itself (a matrix is read whole before its rows are
                     // written); null: eigenvalues only
  int64_t* sweeps;   // (M) out
  double* work;      // gridDim.x x 2 x N x NP doubles unless both working matrices are in LDS
  int64_t M;
  int N, NP;
  int a_in_lds, v_in_lds;
};

__global__ void __launch_bounds__(256) sym_eig_full_kernel(SymEigFullArgs S) {
  extern __shared__ __attribute__((aligned(8))) unsigned char eig_raw[];
  const int N = S.N, NP = S.NP, tid = threadIdx.x;
  const SymEigWork w = sym_eig_carve(eig_raw, N, NP, S.a_in_lds, S.v_in_lds, S.work + (int64_t)blockIdx.x * 2 * N * NP);
  double* A = w.A;
  double* V = w.V;

  for (int64_t mat = blockIdx.x; mat < S.M; mat += gridDim.x) {
    const double* G = S.A + mat * N * N;
    for (int e = tid; e < N * N; e += 256) {
      const int r = e / N, c = e - r * N;
      A[r * NP + c] = 0.5 * (G[e] + G[c * N + r]);
      V[r * NP + c] = (r == c) ? 1.0 : 0.0;
    }
    __threadfence_block();
    __syncthreads();
    int sweeps = sym_eig_sweeps(w, N, NP, tid);
    if (sweeps == SYM_EIG_MAX_SWEEPS) {  // the cap: the loop has not tested what the last sweep left
      double off, dia;
      sym_eig_mass(A, N, NP, w.red, tid, &off, &dia);
      if (!sym_eig_converged(off, dia)) sweeps = SYM_EIG_MAX_SWEEPS + 1;
    }
    if (tid == 0) S.sweeps[mat] = sweeps;
    // ascending eigenvalues (ties: lower column first); column i of V becomes row rank(i), largest component positive
    double* O = S.V ? S.V + mat * N * N : nullptr;
    for (int i = tid; i < N; i += 256) {
      const double li = A[i * NP + i];
      int rank = 0;
      for (int j = 0; j < N; ++j) {
        const double lj = A[j * NP + j];
        rank += (lj < li) || (lj == li && j < i);
      }
      S.w[mat * N + rank] = li;
      if (!O) continue;
      double best = -1.0, sgn = 1.0;
      for (int a = 0; a < N; ++a) {
        const double v = V[a * NP + i];
        if (fabs(v) > best) { best = fabs(v); sgn = v < 0.0 ? -1.0 : 1.0; }
      }
      for (int a = 0; a < N; ++a) O[rank * N + a] = sgn * V[a * NP + i];
    }
    __threadfence_block();
    __syncthreads();
  }
}

// sum of one value per thread by the 256-slot tree, the same on every thread
__device__ __forceinline__ double vib_sum(double (*red)[256], int tid, double v) {
  red[0][tid] = v;
  __syncthreads();
  block_tree_sum<1>(red, tid);
  const double s = red[0][0];
  __syncthreads();
  return s;
}

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

// ---- eigenvector following ----------------------------------------------------------------------------------------------------
struct EfConst {
  int n3, order, has_t;
  double f_scale, fmax, trust_min, trust_max;
};
struct EfState {  // per geometry, in device memory: the optimiser's state, the end-of-run outputs and status
  double *R, *tvec, *trust, *E_prev, *dE_pred;
  int64_t* flags;   // bit 0: a previous step exists, bit 1: that step was clipped
  double *F, *E, *w, *mode;
  int64_t *n_rigid, *n_neg;
  int64_t* status;  // (B,2) as gdml_relax_run's
  int64_t* bad;
};
struct EfEval {  // this evaluation's results for one slice of geometries
  const double *V, *w, *Ft, *Et;  // eigenvectors as rows (bc,n3,n3), spectrum after vib_finish_kernel (bc,n3), F', E'
  const int64_t *sweeps, *n_rigid, *n_neg;
};
struct EfSlot {  // where this evaluation goes in the chunk buffers
  double *E, *fat;  // (B) rows of the history
  double* wf;       // (B) row: eigenvalue of the followed mode
  int64_t* kf;      // (B) row: its index
  double* R;        // (B,3N) frame; null when this is no recording evaluation
};

// dynamic LDS: g [n3] | gt [n3] | s [n3] (the overlaps v_i . t until the followed mode is chosen) | red [256] | followed index
// (no static LDS beside it: statics precede the dynamic region and would shift its base off the doubles' alignment)
static inline size_t ef_step_lds(int n3) { return (size_t)(3 * n3 + 256 + 1) * 8; }

// One evaluation of geometry b0 + blockIdx.x once its F', E', spectrum and eigenvectors are known.  One workgroup per geometry;
// it writes nothing another workgroup reads.  Sums over modes: per-thread partial sums in index order, then the 256-slot tree;
// row . vector products: one wavefront per row, lanes stride the columns, the xor butterfly; the back-projection sums over the
// modes in ascending order, one coordinate per thread.
__global__ void __launch_bounds__(256) ef_step_kernel(EfConst C, EfState S, EfEval Ev, EfSlot sl, int64_t b0, int64_t t,
                                                      int last) {
  extern __shared__ __attribute__((aligned(8))) unsigned char ef_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n3 = C.n3;
  const int64_t ql = blockIdx.x, q = b0 + ql;
  if (S.status[2 * q] >= 0) return;  // frozen by an earlier launch: never written again
  double* g = reinterpret_cast<double*>(ef_raw);
  double* gt = g + n3;
  double* s = gt + n3;
  double (*red)[256] = reinterpret_cast<double (*)[256]>(s + n3);
  int* s_k = reinterpret_cast<int*>(s + n3 + 256);
  const int64_t o = q * n3;
  double* r = S.R + o;
  double* tv = C.has_t ? S.tvec + o : nullptr;
  const double* fp = Ev.Ft + ql * n3;
  const double* wq = Ev.w + ql * n3;
  const double* Vq = Ev.V + ql * n3 * (int64_t)n3;
  const double e = Ev.Et[ql];
  const int n_rigid = (int)Ev.n_rigid[ql], nv = n3 - n_rigid;

  // a. gradient, finiteness, this evaluation's outputs
  int nf = 0;
  for (int k = tid; k < n3; k += 256) {
    const double f = fp[k], wk = wq[k];
    g[k] = -C.f_scale * f;
    nf |= !(isfinite(r[k]) && isfinite(f) && isfinite(wk));
    S.F[o + k] = f;
    S.w[o + k] = wk;
    if (sl.R) sl.R[o + k] = r[k];
  }
  nf = __syncthreads_or(nf);
  double fa = 0.0;
  for (int a = tid; 3 * a < n3; a += 256) {
    const double g0 = g[3 * a], g1 = g[3 * a + 1], g2 = g[3 * a + 2];
    const double nrm = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
    fa = nrm > fa ? nrm : fa;
  }
  red[0][tid] = fa;
  __syncthreads();
  block_tree_sum<0, 1>(red, tid);
  const double f_atom = red[0][0];  // (the maximum skips a NaN)
  __syncthreads();
  const bool bad_now = nf || !isfinite(e) || Ev.sweeps[ql] > SYM_EIG_MAX_SWEEPS;

  // c. gradient in the eigenbasis, and the overlaps with the follow vector
  for (int i = wave; i < nv; i += 4) {
    const double* v = Vq + (int64_t)i * n3;
    double ag = 0.0, at = 0.0;
    for (int j = lane; j < n3; j += 64) {
      const double vj = v[j];
      ag += vj * g[j];
      if (tv) at += vj * tv[j];
    }
    ag = wave_sum(ag);
    at = wave_sum(at);
    if (lane == 0) { gt[i] = ag; s[i] = at; }
  }
  __syncthreads();
  // d. the followed mode: the largest |v_i . t|, the lowest index on ties
  if (tid == 0) {
    int k = 0;
    if (C.order == 1 && tv) {
      double best = -1.0;
      for (int i = 0; i < nv; ++i) {
        const double a = fabs(s[i]);
        if (a > best) { best = a; k = i; }
      }
    }
    *s_k = k;
  }
  __syncthreads();
  const int kfol = *s_k;
  for (int j = tid; j < n3; j += 256) S.mode[o + j] = C.order == 1 ? Vq[(int64_t)kfol * n3 + j] : 0.0;
  if (tid == 0) {
    S.E[q] = e;
    S.n_rigid[q] = n_rigid;
    S.n_neg[q] = Ev.n_neg[ql];
    sl.wf[q] = nv > 0 ? wq[kfol] : 0.0;
    sl.kf[q] = kfol;
    sl.E[q] = e;
    sl.fat[q] = f_atom;
    if (bad_now && S.bad[q] < 0) S.bad[q] = t;
  }
  const bool conv = !bad_now && f_atom < C.fmax;
  if (conv || last) {  // frozen from here on: the state stays what this evaluation found
    if (tid == 0) {
      S.status[2 * q] = conv ? 1 : 0;
      S.status[2 * q + 1] = t;
    }
    return;
  }

  // b. trust radius from the last step's predicted and actual change of the energy
  double trust = S.trust[q];
  const int64_t fl = S.flags[q];
  if (fl & 1) {
    const double dEp = S.dE_pred[q], Ep = S.E_prev[q];
    if (fabs(dEp) > 1e-8 * fmax(fabs(e), fabs(Ep)) * C.f_scale) {
      const double rho = C.f_scale * (e - Ep) / dEp;
      if (rho < 0.25 || rho > 1.75) trust = fmax(0.5 * trust, C.trust_min);
      else if (rho > 0.75 && rho < 1.25 && (fl & 2)) trust = fmin(2.0 * trust, C.trust_max);
    }
  }
  // e. the rational-function step of every mode in closed form
  double p2 = 0.0;
  for (int i = tid; i < nv; i += 256) {
    const double wi = wq[i], gi = gt[i];
    const double d = fabs(wi) + sqrt(wi * wi + 4.0 * (gi * gi));
    double si = d > 0.0 ? -2.0 * gi / d : 0.0;
    if (C.order == 1 && i == kfol) si = -si;
    s[i] = si;
    p2 += si * si;
  }
  // f. trust radius
  const double s_nrm = sqrt(vib_sum(red, tid, p2));
  const bool clip = s_nrm > trust;
  const double scale = trust / s_nrm;
  // g. predicted change, new positions, follow vector
  double pe = 0.0;
  for (int i = tid; i < nv; i += 256) {
    double si = s[i];
    if (clip) si = si * scale;
    s[i] = si;
    pe += gt[i] * si + 0.5 * wq[i] * (si * si);
  }
  const double dE = vib_sum(red, tid, pe);
  for (int j = tid; j < n3; j += 256) {
    double acc = 0.0;
    for (int i = 0; i < nv; ++i) acc += s[i] * Vq[(int64_t)i * n3 + j];
    r[j] = r[j] + acc;
    if (tv && C.order == 1) tv[j] = Vq[(int64_t)kfol * n3 + j];
  }
  if (tid == 0) {
    S.trust[q] = trust;
    S.E_prev[q] = e;
    S.dE_pred[q] = dE;
    S.flags[q] = 1 | (clip ? 2 : 0);
  }
}

// the eigensolver's plan for this file: the device-memory route keeps one workgroup per compute unit (its work matrices are
// 16 N^2 bytes per workgroup)
SymEigPlan full_plan(const gdml_ctx* ctx, int64_t M, int N) {
  SymEigPlan p = sym_eig_plan(ctx->num_cus, M, N);
  if (!p.a_in_lds && p.grid > ctx->num_cus) p.grid = ctx->num_cus;
  return p;
}
int64_t full_work_doubles(const SymEigPlan& p, int N) { return p.v_in_lds ? 0 : p.grid * 2 * (int64_t)N * p.NP; }

// geometries per chunk of gdml_vib_run and per slice of gdml_ef_run: Hessians, spectra and the eigensolver's work matrices
// under VIB_CHUNK_BYTES, whole slices of the Hessian's 64 when there are several
// (a matrix beyond LDS brings its workgroup's two work matrices; beyond one workgroup per compute unit that over-counts)
int64_t vib_chunk_len(const gdml_ctx* ctx, int64_t B, int n3) {
  const int64_t nn = (int64_t)n3 * n3;
  const SymEigPlan p1 = full_plan(ctx, 1, n3);
  const int64_t per = (nn + 3 * (int64_t)n3 + 8 + full_work_doubles(p1, n3)) * 8;
  int64_t chunk = VIB_CHUNK_BYTES / per;
  if (chunk > 64) chunk = chunk / 64 * 64;
  const int64_t opt = (int64_t)ctx_opt(ctx, "predict.vib_chunk", 0.0);
  if (opt > 0) chunk = opt;
  if (chunk < 1) chunk = 1;
  if (chunk > B) chunk = B;
  return chunk;
}

// queues the eigen-kernel for M matrices on the device; work: full_work_doubles(p, N) doubles
int launch_sym_eig_full(gdml_ctx* ctx, const SymEigPlan& p, const double* d_A, int64_t M, int N, double* d_w, double* d_V,
                        int64_t* d_sweeps, double* work) {
  SymEigFullArgs e;
  e.A = d_A; e.w = d_w; e.V = d_V; e.sweeps = d_sweeps; e.work = work; e.M = M; e.N = N;
  e.NP = p.NP; e.a_in_lds = p.a_in_lds; e.v_in_lds = p.v_in_lds;
  if (p.lds > 48 * 1024)
    HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(sym_eig_full_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
  const int es = ktime_begin(ctx);
  hipLaunchKernelGGL(sym_eig_full_kernel, dim3((unsigned)p.grid), dim3(256), p.lds, ctx->stream, e);
  ktime_end(ctx, es, "sym_eig_full", (double)M);
  ctx->launch_counter++;
  HIP_CHECK(ctx, hipGetLastError());
  return GDML_OK;
}

// the first matrix the cap stopped above the threshold becomes the call's error
int check_sweeps(gdml_ctx* ctx, const char* fn, const int64_t* sweeps, int64_t M, int64_t m0) {
  for (int64_t m = 0; m < M; ++m)
    if (sweeps[m] > SYM_EIG_MAX_SWEEPS)
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: matrix %lld is still above the threshold after %d Jacobi sweeps (not finite?)",
                       fn, (long long)(m0 + m), SYM_EIG_MAX_SWEEPS);
  return GDML_OK;
}

int sym_eig_check(gdml_ctx* ctx, const char* fn, const double* A, int64_t M, int n, const double* w) {
  if (M < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: M < 0", fn);
  if (n < 1 || n > SYM_EIG_MAX_N) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: n = %d outside 1 .. %d", fn, n, SYM_EIG_MAX_N);
  if (!A || !w) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: A or w is NULL", fn);
  if (M > 0 && M >= ((int64_t)1 << 62) / ((int64_t)n * n)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: M n n >= 2^62", fn);
  if (!ctx) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: ctx is NULL", fn);
  return GDML_OK;
}

int sym_eig_common(gdml_ctx* ctx, const char* fn, const double* A, bool on_device, int64_t M, int n, double* w, double* V,
                   int64_t* sweeps) {
  GDML_TRY(sym_eig_check(ctx, fn, A, M, n, w));
  if (M == 0) return GDML_OK;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t nn = (int64_t)n * n;
  const SymEigPlan p = full_plan(ctx, M, n);
  const int64_t n_work = full_work_doubles(p, n);
  // host entry: the matrices (the eigenvectors over them), the eigenvalues; both: the sweeps when the caller has no room
  const int64_t n_own = on_device ? (sweeps ? 0 : M) : M * nn + M * n + M;
  double* buf;
  GDML_TRY(ctx_slot(ctx, SLOT_VIB_WS, (n_work + n_own) * 8, &buf));
  double* work = buf;
  const double* d_A = A;
  double *d_w = w, *d_V = V;
  int64_t* d_sw = sweeps;
  hipStream_t st = ctx->stream;
  if (!on_device) {
    double* own = buf + n_work;
    HIP_CHECK(ctx, hipMemcpyAsync(own, A, (size_t)(M * nn) * 8, hipMemcpyHostToDevice, st));
    d_A = own;
    d_V = V ? own : nullptr;
    d_w = own + M * nn;
    d_sw = (int64_t*)(d_w + M * n);
  } else if (!sweeps) {
    d_sw = (int64_t*)(buf + n_work);
  }
  GDML_TRY(launch_sym_eig_full(ctx, p, d_A, M, n, d_w, d_V, d_sw, work));
  std::vector<int64_t> h_sw;
  int64_t* sw_host = sweeps;
  if (on_device || !sweeps) {
    h_sw.resize((size_t)M);
    sw_host = h_sw.data();
  }
  HIP_CHECK(ctx, hipMemcpyAsync(sw_host, d_sw, (size_t)M * 8, hipMemcpyDeviceToHost, st));
  if (!on_device) {
    HIP_CHECK(ctx, hipMemcpyAsync(w, d_w, (size_t)(M * n) * 8, hipMemcpyDeviceToHost, st));
    if (V) HIP_CHECK(ctx, hipMemcpyAsync(V, d_V, (size_t)(M * nn) * 8, hipMemcpyDeviceToHost, st));
  }
  HIP_CHECK(ctx, hipStreamSynchronize(st));
  return check_sweeps(ctx, fn, sw_host, M, 0);
}

int vib_check(gdml_ctx* ctx, const gdml_vib_params* p, const double* R, const double* masses, const double* w2,
              const int64_t* n_rigid, const int64_t* n_neg) {
  const char* fn = "gdml_vib_run";
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: params is NULL", fn);
  GDML_TRY(traj_check_shape(ctx, fn, p->B, p->N));
  if (p->project < 0 || p->project > 2) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: project must be 0, 1 or 2", fn);
  GDML_TRY(traj_check_lattice(ctx, fn, p->lat, p->lat_inv));
  if (p->project == 2 && p->lat)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: project = 2 with a lattice (rotations are no symmetry of a periodic cell)", fn);
  if (!isfinite(p->h_scale) || !(p->h_scale > 0.0))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: h_scale must be positive and finite", fn);
  if (!masses) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: masses is NULL", fn);
  if (p->N > VIB_MAX_ATOMS)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "%s: N = %d beyond the Hessian's limit (N <= %d)", fn, p->N, VIB_MAX_ATOMS);
  for (int a = 0; a < p->N; ++a)
    if (!(masses[a] > 0.0) || !isfinite(masses[a]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: mass of atom %d must be positive and finite", fn, a);
  if (!R || !w2 || !n_rigid || !n_neg) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: R, w2, n_rigid or n_neg is NULL", fn);
  const int64_t nR = p->B * 3 * (int64_t)p->N;
  for (int64_t i = 0; i < nR; ++i)
    if (!isfinite(R[i]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: coordinate %lld of geometry %lld is not finite", fn,
                       (long long)(i % (3 * p->N)), (long long)(i / (3 * p->N)));
  return GDML_OK;
}

int ef_check(gdml_ctx* ctx, const gdml_ef_params* p, const double* R, const double* trust, const double* E_prev,
             const double* dE_pred, const int64_t* flags, const double* t, int64_t max_steps, int64_t record_every,
             const double* R_rec, const void* const* out, int n_out) {
  const char* fn = "gdml_ef_run";
  if (!p) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: params is NULL", fn);
  if (max_steps < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: max_steps < 0", fn);
  if (record_every < 0 || (R_rec && record_every < 1))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: record_every < 0, or < 1 with R_rec", fn);
  GDML_TRY(traj_check_shape(ctx, fn, p->B, p->N));
  if (!isfinite(p->f_scale) || !(p->f_scale > 0.0))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: f_scale must be positive and finite", fn);
  if (!(p->fmax > 0.0) || !isfinite(p->fmax)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: fmax must be positive and finite", fn);
  if (p->order != 0 && p->order != 1) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: order must be 0 (minimum) or 1 (saddle)", fn);
  if (!(p->trust_min > 0.0) || !isfinite(p->trust_min))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: trust_min must be positive and finite", fn);
  if (!(p->trust_max >= p->trust_min) || !isfinite(p->trust_max))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: trust_max must be finite and at least trust_min", fn);
  if (p->project < 0 || p->project > 2) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: project must be 0, 1 or 2", fn);
  GDML_TRY(traj_check_lattice(ctx, fn, p->lat, p->lat_inv));
  if (p->project == 2 && p->lat)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: project = 2 with a lattice (rotations are no symmetry of a periodic cell)", fn);
  if (t && p->order == 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: a follow vector with order = 0", fn);
  if (!R || !trust || !E_prev || !dE_pred || !flags)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: a state array (R, trust, E_prev, dE_pred, flags) is NULL", fn);
  for (int i = 0; i < n_out; ++i)
    if (!out[i])
      return gdml_fail(ctx, GDML_ERR_INVALID,
                       "%s: an output array (E_hist, fmax_hist, w_follow_hist, E_end, F_end, w_end, n_rigid, n_neg, mode_end, "
                       "status) is NULL", fn);
  if (p->N > VIB_MAX_ATOMS)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "%s: N = %d beyond the Hessian's limit (N <= %d)", fn, p->N, VIB_MAX_ATOMS);
  const int64_t n3 = 3 * (int64_t)p->N;
  for (int64_t b = 0; b < p->B; ++b) {
    if (!(trust[b] >= p->trust_min && trust[b] <= p->trust_max))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: trust of geometry %lld outside [trust_min, trust_max]", fn, (long long)b);
    if (flags[b] < 0 || flags[b] > 3) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: flags of geometry %lld outside 0 .. 3", fn, (long long)b);
    if ((flags[b] & 1) && !(isfinite(E_prev[b]) && isfinite(dE_pred[b])))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: E_prev or dE_pred of geometry %lld is not finite", fn, (long long)b);
  }
  for (int64_t i = 0; i < p->B * n3; ++i) {
    if (!isfinite(R[i]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: coordinate %lld of geometry %lld is not finite", fn, (long long)(i % n3),
                       (long long)(i / n3));
    if (t && !isfinite(t[i]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: follow vector entry %lld of geometry %lld is not finite", fn,
                       (long long)(i % n3), (long long)(i / n3));
  }
  return GDML_OK;
}

}  // namespace

extern "C" int gdml_sym_eig(gdml_ctx* ctx, const double* A, int64_t M, int n, double* w, double* V, int64_t* sweeps) {
  return sym_eig_common(ctx, "gdml_sym_eig", A, false, M, n, w, V, sweeps);
}

extern "C" int gdml_sym_eig_dev(gdml_ctx* ctx, const double* A_dev, int64_t M, int n, double* w_dev, double* V_dev,
                                int64_t* sweeps_dev) {
  return sym_eig_common(ctx, "gdml_sym_eig_dev", A_dev, true, M, n, w_dev, V_dev, sweeps_dev);
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

  const int64_t chunk = vib_chunk_len(ctx, B, n3);
  const SymEigPlan plan = full_plan(ctx, chunk, n3);
  const int64_t n_work = full_work_doubles(plan, n3);

  // one carve: work matrices | H (D_s, modes) | R | F | w | info | E | mass | sweeps, n_rigid, n_neg
  double* buf;
  GDML_TRY(ctx_slot(ctx, SLOT_VIB_WS, (n_work + chunk * (nn + 3 * n3 + 4 + 1 + 3) + N) * 8, &buf));
  double* work = buf;
  double* d_H = work + n_work;
  double* d_R = d_H + chunk * nn;
  double* d_F = d_R + chunk * n3;
  double* d_w = d_F + chunk * n3;
  double* d_info = d_w + chunk * n3;
  double* d_E = d_info + chunk * 4;
  double* d_mass = d_E + chunk;
  int64_t* d_sw = (int64_t*)(d_mass + N);
  int64_t* d_nr = d_sw + chunk;
  int64_t* d_nn = d_nr + chunk;

  hipStream_t st = ctx->stream;
  HIP_CHECK(ctx, hipMemcpyAsync(d_mass, masses, (size_t)N * 8, hipMemcpyHostToDevice, st));
  const size_t proj_lds = vib_proj_lds(n3);
  if (proj_lds > 48 * 1024)
    HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(vib_project_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)proj_lds));
  std::vector<int64_t> h_sw((size_t)chunk);
  for (int64_t b0 = 0; b0 < B; b0 += chunk) {
    const int64_t bc = B - b0 < chunk ? B - b0 : chunk;
    HIP_CHECK(ctx, hipMemcpyAsync(d_R, R + b0 * n3, (size_t)(bc * n3) * 8, hipMemcpyHostToDevice, st));
    GDML_TRY(gdml_predict_hessian_dev(ctx, d_R, bc, p->lat, p->lat_inv, d_E, d_F, d_H));
    VibProjArgs A;
    A.H = d_H; A.R = d_R; A.mass = d_mass; A.info = d_info; A.h_scale = p->h_scale; A.N = N; A.n3 = n3; A.project = p->project;
    int ks = ktime_begin(ctx);
    hipLaunchKernelGGL(vib_project_kernel, dim3((unsigned)bc), dim3(256), proj_lds, st, A);
    ktime_end(ctx, ks, "vib_project", (double)bc);
    HIP_CHECK(ctx, hipGetLastError());
    SymEigPlan pc = plan;
    if (pc.grid > bc) pc.grid = bc;
    GDML_TRY(launch_sym_eig_full(ctx, pc, d_H, bc, n3, d_w, d_H, d_sw, work));
    hipLaunchKernelGGL(vib_finish_kernel, dim3((unsigned)ceil_div(bc, 256)), dim3(256), 0, st, d_w, d_info, bc, n3, d_nr, d_nn);
    HIP_CHECK(ctx, hipGetLastError());
    ctx->launch_counter += 2;
    HIP_CHECK(ctx, hipMemcpyAsync(h_sw.data(), d_sw, (size_t)bc * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipMemcpyAsync(w2 + b0 * n3, d_w, (size_t)(bc * n3) * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipMemcpyAsync(n_rigid + b0, d_nr, (size_t)bc * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipMemcpyAsync(n_neg + b0, d_nn, (size_t)bc * 8, hipMemcpyDeviceToHost, st));
    if (E) HIP_CHECK(ctx, hipMemcpyAsync(E + b0, d_E, (size_t)bc * 8, hipMemcpyDeviceToHost, st));
    if (F) HIP_CHECK(ctx, hipMemcpyAsync(F + b0 * n3, d_F, (size_t)(bc * n3) * 8, hipMemcpyDeviceToHost, st));
    if (modes) HIP_CHECK(ctx, hipMemcpyAsync(modes + b0 * nn, d_H, (size_t)(bc * nn) * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (sweeps) memcpy(sweeps + b0, h_sw.data(), (size_t)bc * 8);
    GDML_TRY(check_sweeps(ctx, "gdml_vib_run", h_sw.data(), bc, b0));
  }
  return GDML_OK;
}

extern "C" int gdml_ef_run(gdml_ctx* ctx, const gdml_ef_params* p, double* R, double* trust, double* E_prev, double* dE_pred,
                           int64_t* flags, double* t_follow, int64_t max_steps, int64_t record_every, double* R_rec,
                           double* E_hist, double* fmax_hist, double* w_follow_hist, int64_t* k_follow_hist, double* E_end,
                           double* F_end, double* w_end, int64_t* n_rigid, int64_t* n_neg, double* mode_end, int64_t* status,
                           int64_t* first_bad_step) {
  const void* outs[] = {E_hist, fmax_hist, w_follow_hist, E_end, F_end, w_end, n_rigid, n_neg, mode_end, status};
  GDML_TRY(ef_check(ctx, p, R, trust, E_prev, dE_pred, flags, t_follow, max_steps, record_every, R_rec, outs, 10));
  bool run;
  GDML_TRY(traj_prelude(ctx, "gdml_ef_run", p->N, p->B, first_bad_step, &run));
  if (!run) return GDML_OK;
  const int64_t B = p->B;
  const int N = p->N, n3 = 3 * N;
  const int64_t nn = (int64_t)n3 * n3, nc = B * n3;
  // evaluations per chunk, and frames of R per chunk where they are recorded: gdml_relax_run's
  FrozenRun fr = {B, max_steps, record_every, traj_frozen_chunk_steps(ctx, max_steps), 4,
                  {E_hist, fmax_hist, w_follow_hist, k_follow_hist}};
  Recorder rec;
  const int f_R = rec.add(R_rec, nc);
  rec.size(ctx, fr.chunk_steps);
  // geometries per slice of an evaluation: gdml_vib_run's chunk
  const int64_t slice = vib_chunk_len(ctx, B, n3);
  const SymEigPlan plan = full_plan(ctx, slice, n3);
  const int64_t n_work = full_work_doubles(plan, n3);

  // one carve.  Per slice: work matrices | H (D_s, eigenvectors) | F' | w | info | E' | unit masses | sweeps, n_rigid, n_neg.
  // Per run: R | t | F_end | w_end | mode_end | E_end | trust | E_prev | dE_pred | flags, n_rigid, n_neg | status, bad, a chunk of
  // the history (E, f_atom, w_follow, k_follow) | a chunk of frames
  const int64_t n_slice = n_work + slice * (nn + 2 * n3 + 4 + 1 + 3) + N;
  const int64_t n_run = 5 * nc + 7 * B + fr.words() + rec.len();
  double* buf;
  GDML_TRY(ctx_slot(ctx, SLOT_EF_WS, (n_slice + n_run) * 8, &buf));
  double* work = buf;
  double* d_H = work + n_work;
  double* d_Ft = d_H + slice * nn;
  double* d_w = d_Ft + slice * n3;
  double* d_info = d_w + slice * n3;
  double* d_Et = d_info + slice * 4;
  double* d_mass = d_Et + slice;
  int64_t* d_sw = (int64_t*)(d_mass + N);
  int64_t* d_nr = d_sw + slice;
  int64_t* d_nn = d_nr + slice;
  EfState S;
  S.R = (double*)(d_nn + slice);
  S.tvec = S.R + nc;
  S.F = S.tvec + nc;
  S.w = S.F + nc;
  S.mode = S.w + nc;
  S.E = S.mode + nc;
  S.trust = S.E + B;
  S.E_prev = S.trust + B;
  S.dE_pred = S.E_prev + B;
  S.flags = (int64_t*)(S.dE_pred + B);
  S.n_rigid = S.flags + B;
  S.n_neg = S.n_rigid + B;
  rec.carve(fr.carve((double*)(S.n_neg + B)));
  S.status = fr.status();
  S.bad = fr.bad();

  hipStream_t st = ctx->stream;
  const std::vector<double> ones((size_t)N, 1.0);
  HIP_CHECK(ctx, hipMemcpyAsync(d_mass, ones.data(), (size_t)N * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.R, R, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  if (t_follow) HIP_CHECK(ctx, hipMemcpyAsync(S.tvec, t_follow, (size_t)nc * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.trust, trust, (size_t)B * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.E_prev, E_prev, (size_t)B * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.dE_pred, dE_pred, (size_t)B * 8, hipMemcpyHostToDevice, st));
  HIP_CHECK(ctx, hipMemcpyAsync(S.flags, flags, (size_t)B * 8, hipMemcpyHostToDevice, st));
  // the caller's arrays are pageable: the copies above have to be through before they may change
  HIP_CHECK(ctx, hipStreamSynchronize(st));

  EfConst C;
  C.n3 = n3; C.order = p->order; C.has_t = t_follow != nullptr;
  C.f_scale = p->f_scale; C.fmax = p->fmax; C.trust_min = p->trust_min; C.trust_max = p->trust_max;
  const size_t proj_lds = vib_proj_lds(n3);
  if (proj_lds > 48 * 1024)
    HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(vib_project_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)proj_lds));

  GDML_TRY(traj_run_until_frozen(ctx, rec, R_rec != nullptr, fr, [&](int64_t te, int64_t row, int64_t frame, int last) {
    const EfSlot sl = {fr.row(0, row), fr.row(1, row), fr.row(2, row), (int64_t*)fr.row(3, row),
                       frame >= 0 ? rec.slot(f_R, frame) : nullptr};
    // the timer of the previous Hessian is dropped unread: reading it would wait for it on the host
    ctx->phase_pending.clear();
    for (int64_t b0 = 0; b0 < B; b0 += slice) {
      const int64_t bc = B - b0 < slice ? B - b0 : slice;
      GDML_TRY(gdml_predict_hessian_dev(ctx, S.R + b0 * n3, bc, p->lat, p->lat_inv, d_Et, d_Ft, d_H));
      VibProjArgs A;
      A.H = d_H; A.R = S.R + b0 * n3; A.mass = d_mass; A.info = d_info; A.h_scale = p->f_scale; A.N = N; A.n3 = n3;
      A.project = p->project;
      hipLaunchKernelGGL(vib_project_kernel, dim3((unsigned)bc), dim3(256), proj_lds, st, A);
      HIP_CHECK(ctx, hipGetLastError());
      SymEigPlan pc = plan;
      if (pc.grid > bc) pc.grid = bc;
      GDML_TRY(launch_sym_eig_full(ctx, pc, d_H, bc, n3, d_w, d_H, d_sw, work));
      hipLaunchKernelGGL(vib_finish_kernel, dim3((unsigned)ceil_div(bc, 256)), dim3(256), 0, st, d_w, d_info, bc, n3, d_nr, d_nn);
      const EfEval Ev = {d_H, d_w, d_Ft, d_Et, d_sw, d_nr, d_nn};
      hipLaunchKernelGGL(ef_step_kernel, dim3((unsigned)bc), dim3(256), ef_step_lds(n3), st, C, S, Ev, sl, b0, te, last);
      HIP_CHECK(ctx, hipGetLastError());
      ctx->launch_counter += 3;
    }
    return (int)GDML_OK;
  }));
  HIP_CHECK(ctx, hipMemcpyAsync(R, S.R, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  if (t_follow) HIP_CHECK(ctx, hipMemcpyAsync(t_follow, S.tvec, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(trust, S.trust, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(E_prev, S.E_prev, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(dE_pred, S.dE_pred, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(flags, S.flags, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(E_end, S.E, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(F_end, S.F, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(w_end, S.w, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(mode_end, S.mode, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(n_rigid, S.n_rigid, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipMemcpyAsync(n_neg, S.n_neg, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(ctx, hipStreamSynchronize(st));
  // a frozen geometry repeats its last history values and its end positions up to the last evaluation made (the launches
  // behind its freeze wrote nothing for it)
  const TrajFrames frames = {R_rec, R, n3};
  fr.finish(status, first_bad_step, &frames, 1);
  return GDML_OK;
}
