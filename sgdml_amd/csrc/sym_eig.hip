// ------------------------------------------------------------------------------------------
// The batched symmetric eigensolver: ONE kernel template, ONE launcher, and the entries gdml_sym_eig, gdml_sym_eig_dev (full
// spectrum; harmonic vibrations and eigenvector following run the same launch, vib.hip) and gdml_sym_eig_absv (what the
// symmetry search consumes; gdml_perm_match in perm_match.hip calls sym_eig_absv_dev).
// One workgroup per matrix, grid-stride over the batch: the symmetrised matrix into A, the identity into V, the Jacobi sweeps,
// storage routes and stopping rule of sym_eig.h under the plan of sym_eig_plan.h.  What follows the sweeps is the output policy:
//   EigRows   eigenvalues ascending (ties: the lower Jacobi column first), V[k][:] the unit eigenvector of w[k] as a ROW, its
//             component of largest magnitude positive (lowest index on ties).  sweeps[m] = sweeps made, SYM_EIG_MAX_SWEEPS + 1
//             when the matrix is still above the threshold after the cap (the entries turn that into an error).  The contract;
//             include/gdml_hip.h and tests/_vib_ref.py state the same.
//   EigAbsCols  |V| with columns by decreasing eigenvalue (ties: the lower index first), as [a][k] and transposed as [k][a]: the
//             form the matching consumes (only |V| enters, perm.py:66-70, so the sign convention is immaterial; the reference:
//             numpy.linalg.eig per geometry, perm.py:183-187; the host form here: one batched LAPACK eigh -- 4.5 s for 1000
//             geometries of 100 atoms, more than the matching itself).
// ------------------------------------------------------------------------------------------
#include <math.h>

#include "sym_eig.h"

namespace {

// The output policies: what the kernel writes, under which name it is timed, and which eigenvalue comes first.  Their write-out
// is spelled out in the kernel under `if constexpr`: behind a member function, however it is inlined, the compiler schedules the
// kernel differently and the full solver measured 1.6 ... 3.7 % slower (profiles/eig_split_resources.txt).
struct EigRows {
  static constexpr const char* name = "sym_eig_full";
  static constexpr bool rows = true;
  double* w;        // (M, N) out
  double* V;        // (M, N, N) out, row k = eigenvector k; may be the input itself (a matrix is read whole before its rows are
                    // written); null: eigenvalues only
  int64_t* sweeps;  // (M) out
  __device__ static bool before(double lj, double li) { return lj < li; }
};

struct EigAbsCols {
  static constexpr const char* name = "sym_eig";
  static constexpr bool rows = false;
  double* absv;   // (M, N, N) out: [a][k]
  double* absvT;  // (M, N, N) out: [k][a]
  __device__ static bool before(double lj, double li) { return lj > li; }
};

template <class Out>
struct SymEigArgs {
  const double* A;  // (M, N, N)
  Out out;
  double* work;     // gridDim.x x 2 x N x NP doubles (only the parts that do not fit in LDS are used)
  int64_t M;
  int N, NP;
  int a_in_lds, v_in_lds;
};

template <class Out>
__global__ void __launch_bounds__(256) sym_eig_kernel(SymEigArgs<Out> S) {
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
    double *O, *OT;
    if constexpr (Out::rows) {
      if (sweeps == SYM_EIG_MAX_SWEEPS) {  // the cap: the loop has not tested what the last sweep left
        double off, dia;
        sym_eig_mass(A, N, NP, w.red, tid, &off, &dia);
        if (!sym_eig_converged(off, dia)) sweeps = SYM_EIG_MAX_SWEEPS + 1;
      }
      if (tid == 0) S.out.sweeps[mat] = sweeps;
      O = S.out.V ? S.out.V + mat * N * N : nullptr;
    } else {
      O = S.out.absv + mat * N * N;
      OT = S.out.absvT + mat * N * N;
    }
    // the policy's order of the eigenvalues (ties: lower column first); column i of V goes out at its rank
    for (int i = tid; i < N; i += 256) {
      const double li = A[i * NP + i];
      int rank = 0;
      for (int j = 0; j < N; ++j) {
        const double lj = A[j * NP + j];
        rank += Out::before(lj, li) || (lj == li && j < i);
      }
      if constexpr (Out::rows) {  // as row `rank`, largest component positive
        S.out.w[mat * N + rank] = li;
        if (!O) continue;
        double best = -1.0, sgn = 1.0;
        for (int a = 0; a < N; ++a) {
          const double v = V[a * NP + i];
          if (fabs(v) > best) { best = fabs(v); sgn = v < 0.0 ? -1.0 : 1.0; }
        }
        for (int a = 0; a < N; ++a) O[rank * N + a] = sgn * V[a * NP + i];
      } else {  // absolute values as column `rank`, and transposed
        for (int a = 0; a < N; ++a) {
          const double av = fabs(V[a * NP + i]);
          O[a * N + rank] = av;
          OT[rank * N + a] = av;
        }
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}

// queues the eigen-kernel for M matrices on the device under the policy's name; work: p.work_doubles doubles
template <class Out>
hipError_t launch_sym_eig(gdml_ctx* ctx, const SymEigPlan& p, const double* d_A, int64_t M, int N, const Out& out, double* work) {
  SymEigArgs<Out> e;
  e.A = d_A; e.out = out; e.work = work; e.M = M; e.N = N;
  e.NP = p.NP; e.a_in_lds = p.a_in_lds; e.v_in_lds = p.v_in_lds;
  if (p.lds > 48 * 1024) {
    const hipError_t se = hipFuncSetAttribute(reinterpret_cast<const void*>(sym_eig_kernel<Out>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    if (se != hipSuccess) return se;
  }
  const int es = ktime_begin(ctx);
  hipLaunchKernelGGL(sym_eig_kernel<Out>, dim3((unsigned)p.grid), dim3(256), p.lds, ctx->stream, e);
  ktime_end(ctx, es, Out::name, (double)M);
  ctx->launch_counter++;
  return hipGetLastError();
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
  const SymEigPlan p = sym_eig_plan(ctx->num_cus, M, n, true);
  const int64_t n_work = p.work_doubles;
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
  HIP_CHECK(ctx, sym_eig_rows_launch(ctx, p, d_A, M, n, d_w, d_V, d_sw, work));
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
  return sym_eig_check_sweeps(ctx, fn, sw_host, M, 0);
}

}  // namespace

hipError_t sym_eig_rows_launch(gdml_ctx* ctx, const SymEigPlan& p, const double* d_A, int64_t M, int N, double* d_w, double* d_V,
                               int64_t* d_sweeps, double* work) {
  return launch_sym_eig(ctx, p, d_A, M, N, EigRows{d_w, d_V, d_sweeps}, work);
}

int sym_eig_check_sweeps(gdml_ctx* ctx, const char* fn, const int64_t* sweeps, int64_t M, int64_t m0) {
  for (int64_t m = 0; m < M; ++m)
    if (sweeps[m] > SYM_EIG_MAX_SWEEPS)
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: matrix %lld is still above the threshold after %d Jacobi sweeps (not finite?)",
                       fn, (long long)(m0 + m), SYM_EIG_MAX_SWEEPS);
  return GDML_OK;
}

// |V| (columns by decreasing eigenvalue) of M symmetric N x N matrices already on the device; d_v [a][k], d_vT [k][a].  No
// slot is reserved for the search's work matrices: they are allocated here (none when both matrices live in LDS, N <= 100)
// and released behind the synchronisation, which also brings a failure of the kernel back under this function's message.
int sym_eig_absv_dev(gdml_ctx* ctx, const double* d_adj, double* d_v, double* d_vT, int64_t M, int N) {
  const SymEigPlan p = sym_eig_plan(ctx->num_cus, M, N, false);
  double* d_w = nullptr;
  if (p.work_doubles > 0) GDML_TRY(ctx_alloc(ctx, (void**)&d_w, p.work_doubles * 8));
  hipError_t se = launch_sym_eig(ctx, p, d_adj, M, N, EigAbsCols{d_v, d_vT}, d_w);
  if (se == hipSuccess) se = hipStreamSynchronize(ctx->stream);
  if (d_w) ctx_free(ctx, d_w);
  if (se != hipSuccess) return gdml_fail(ctx, GDML_ERR_HIP, "eigenvector kernel of the symmetry search: %s", hipGetErrorString(se));
  return GDML_OK;
}

extern "C" int gdml_sym_eig(gdml_ctx* ctx, const double* A, int64_t M, int n, double* w, double* V, int64_t* sweeps) {
  return sym_eig_common(ctx, "gdml_sym_eig", A, false, M, n, w, V, sweeps);
}

extern "C" int gdml_sym_eig_dev(gdml_ctx* ctx, const double* A_dev, int64_t M, int n, double* w_dev, double* V_dev,
                                int64_t* sweeps_dev) {
  return sym_eig_common(ctx, "gdml_sym_eig_dev", A_dev, true, M, n, w_dev, V_dev, sweeps_dev);
}

// |eigenvectors| of M symmetric N x N matrices, columns by decreasing eigenvalue (what gdml_perm_match computes when it is not
// handed any): for tests and for callers that want them on the host.
extern "C" int gdml_sym_eig_absv(gdml_ctx* ctx, const double* adj, int64_t M, int N, double* absv_out) {
  if (!ctx) return GDML_ERR_INVALID;
  if (!adj || !absv_out || M < 0 || N < 1 || N > GDML_MAX_ATOMS)
    return gdml_fail(ctx, GDML_ERR_INVALID, "gdml_sym_eig_absv: bad arguments (M=%lld N=%d)", (long long)M, N);
  if (M == 0) return GDML_OK;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t bytes = M * (int64_t)N * N * 8;
  double *d_a = nullptr, *d_v = nullptr, *d_t = nullptr;
  int rc = ctx_alloc(ctx, (void**)&d_a, bytes);
  if (rc == GDML_OK) rc = ctx_alloc(ctx, (void**)&d_v, bytes);
  if (rc == GDML_OK) rc = ctx_alloc(ctx, (void**)&d_t, bytes);
  if (rc == GDML_OK && hipMemcpyAsync(d_a, adj, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    rc = gdml_fail(ctx, GDML_ERR_HIP, "gdml_sym_eig_absv: upload failed");
  if (rc == GDML_OK) rc = sym_eig_absv_dev(ctx, d_a, d_v, d_t, M, N);
  if (rc == GDML_OK && (hipMemcpyAsync(absv_out, d_v, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                        hipStreamSynchronize(ctx->stream) != hipSuccess))
    rc = gdml_fail(ctx, GDML_ERR_HIP, "gdml_sym_eig_absv: download failed");
  ctx_free(ctx, d_a); ctx_free(ctx, d_v); ctx_free(ctx, d_t);
  return rc;
}
