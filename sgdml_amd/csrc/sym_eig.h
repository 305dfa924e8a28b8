// The batched cyclic Jacobi eigensolver's device parts: the carving of a workgroup's LDS, the off-diagonal mass and the sweep
// loop itself, which the one kernel template of sym_eig.hip runs under either of its output policies; and what the other files
// call of sym_eig.hip.  The launch plan (storage route, LDS bytes, grid, work matrices) is sym_eig_plan.h's.
// One workgroup of 256 threads per matrix, round-robin ordering: a step rotates N/2 disjoint index pairs at once (angles from
// the current matrix, then all row updates, then all column updates -- disjoint rotations commute), N - 1 steps visit every
// pair once.  The working matrix A and the accumulated rotations V live in LDS when both fit (N <= 100), only A when it alone
// fits (N <= 141), both in device memory above that.
#pragma once
#include "common.h"
#include "sym_eig_plan.h"

constexpr int SYM_EIG_MAX_SWEEPS = 30;

// ---- sym_eig.hip, for vib.hip -------------------------------------------------------------------------------------------------
// Queues the eigen-kernel (eigenvalues ascending, signed eigenvectors as rows, sweeps) for M matrices on the device, p.grid
// workgroups; work: p.work_doubles doubles.  d_V may be d_A, or null.  Counts the launch; does not synchronise.
hipError_t sym_eig_rows_launch(gdml_ctx* ctx, const SymEigPlan& p, const double* d_A, int64_t M, int N, double* d_w, double* d_V,
                               int64_t* d_sweeps, double* work);
// the first matrix (numbered from m0) the cap stopped above the threshold becomes the call's error
int sym_eig_check_sweeps(gdml_ctx* ctx, const char* fn, const int64_t* sweeps, int64_t M, int64_t m0);

// a workgroup's pieces: cs [npairs][2], pq [npairs][2], red [8] in LDS; A and V in LDS or in the workgroup's 2 x N x NP
// doubles of device memory gw
struct SymEigWork {
  double* cs;
  int* pq;
  double* red;
  double *A, *V;
};

__device__ __forceinline__ SymEigWork sym_eig_carve(unsigned char* raw, int N, int NP, int a_in_lds, int v_in_lds, double* gw) {
  const int ne = (N + 1) & ~1, npairs = ne / 2;
  SymEigWork w;
  double* lds = reinterpret_cast<double*>(raw);
  w.cs = lds;
  w.pq = reinterpret_cast<int*>(w.cs + 2 * npairs);
  w.red = reinterpret_cast<double*>(w.pq + 2 * npairs + (npairs & 1) * 2);
  double* next = w.red + 8;
  w.A = a_in_lds ? next : gw;
  if (a_in_lds) next += N * NP;
  w.V = v_in_lds ? next : gw + N * NP;
  return w;
}

// off-diagonal and diagonal mass of A (sums of squares), the same on every thread.  Called by all 256 threads.
__device__ __forceinline__ void sym_eig_mass(const double* A, int N, int NP, double* red, int tid, double* off_out,
                                             double* dia_out) {
  double off = 0.0, dia = 0.0;
  for (int e = tid; e < N * N; e += 256) {
    const int r = e / N, c = e - r * N;
    const double a = A[r * NP + c];
    if (r == c) dia += a * a; else off += a * a;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { off += __shfl_xor(off, o, 64); dia += __shfl_xor(dia, o, 64); }
  if ((tid & 63) == 0) { red[2 * (tid >> 6)] = off; red[2 * (tid >> 6) + 1] = dia; }
  __syncthreads();
  off = red[0] + red[2] + red[4] + red[6];
  dia = red[1] + red[3] + red[5] + red[7];
  __syncthreads();
  *off_out = off;
  *dia_out = dia;
}

// converged when the off-diagonal mass is below 1e-30 of the whole -- eigenvectors to a few ulp for separated eigenvalues
__device__ __forceinline__ bool sym_eig_converged(double off, double dia) { return off <= 1e-30 * (dia + off); }

// The sweeps: A (symmetric, both triangles) becomes diagonal, V (the identity on entry) collects the rotations, so that
// column i of V is the eigenvector of A[i][i].  Called by all 256 threads behind a barrier after their writes of A and V;
// returns the sweeps made (0 .. SYM_EIG_MAX_SWEEPS; at the cap the stopping rule has not been tested again).
__device__ __forceinline__ int sym_eig_sweeps(const SymEigWork& w, int N, int NP, int tid) {
  double* A = w.A;
  double* V = w.V;
  double* cs = w.cs;
  int* pq = w.pq;
  const int ne = (N + 1) & ~1, npairs = ne / 2, m = ne - 1;
  int sweep = 0;
  for (; sweep < SYM_EIG_MAX_SWEEPS; ++sweep) {
    // off-diagonal mass against the diagonal's
    double off, dia;
    sym_eig_mass(A, N, NP, w.red, tid, &off, &dia);
    if (sym_eig_converged(off, dia)) break;
    for (int step = 0; step < m; ++step) {
      if (tid < npairs) {
        int p, q;
        if (tid == 0) { p = step % m; q = m; }
        else { p = (step + tid) % m; q = (step + m - tid) % m; }
        if (p > q) { const int t = p; p = q; q = t; }
        double c = 1.0, s = 0.0;
        if (q < N) {
          const double apq = A[p * NP + q];
          if (apq != 0.0) {
            const double tau = (A[q * NP + q] - A[p * NP + p]) / (2.0 * apq);
            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            s = t * c;
          }
        } else {
          q = -1;  // the padding index of an odd N: no rotation
        }
        cs[2 * tid] = c; cs[2 * tid + 1] = s;
        pq[2 * tid] = p; pq[2 * tid + 1] = q;
      }
      __syncthreads();
      // rows p, q of A:  A <- J^T A
      for (int e = tid; e < npairs * N; e += 256) {
        const int k = e / N, j = e - k * N;
        const int p = pq[2 * k], q = pq[2 * k + 1];
        if (q < 0) continue;
        const double c = cs[2 * k], s = cs[2 * k + 1];
        const double ap = A[p * NP + j], aq = A[q * NP + j];
        A[p * NP + j] = c * ap - s * aq;
        A[q * NP + j] = s * ap + c * aq;
      }
      __threadfence_block();
      __syncthreads();
      // columns p, q of A and of V:  A <- A J,  V <- V J
      for (int e = tid; e < npairs * N; e += 256) {
        const int k = e / N, i = e - k * N;
        const int p = pq[2 * k], q = pq[2 * k + 1];
        if (q < 0) continue;
        const double c = cs[2 * k], s = cs[2 * k + 1];
        const double ap = A[i * NP + p], aq = A[i * NP + q];
        A[i * NP + p] = c * ap - s * aq;
        A[i * NP + q] = s * ap + c * aq;
        const double vp = V[i * NP + p], vq = V[i * NP + q];
        V[i * NP + p] = c * vp - s * vq;
        V[i * NP + q] = s * vp + c * vq;
      }
      __threadfence_block();
      __syncthreads();
      // (the rotated pair's off-diagonal entry is zero up to rounding: make it exactly symmetric-zero)
      if (tid < npairs && pq[2 * tid + 1] >= 0) {
        A[pq[2 * tid] * NP + pq[2 * tid + 1]] = 0.0;
        A[pq[2 * tid + 1] * NP + pq[2 * tid]] = 0.0;
      }
      __syncthreads();
    }
  }
  return sweep;
}
