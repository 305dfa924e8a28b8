// Application of the Nystroem preconditioner on the device: P v = (X X^T v - v) / lam in the form that is resident -- the
// stored fp64 factor (the reference's operator, iterative.py:83-142), the fp32 factor with its Gram correction T0, or
// matrix-free.  The factor, T0 and Z are built by nystroem.hip; grids, template selectors and the workspace of the two stored
// forms are decided by precon_apply_plan (precon_plan.h).
#include <math.h>

#include "common.h"
#include "precon_plan.h"

typedef double d2 __attribute__((ext_vector_type(2)));

// t_part[rc][c] = sum_{r in chunk rc} X[r][c] v[r].  HBM bound (X is read once per call): a thread owns two adjacent
// columns (16-byte loads; rows are padded to a multiple of 16 doubles, so the pair of an odd last column stays inside the
// row) and keeps eight rows in flight.
// the factor is streamed (25 GB per pass against 256 MB of Infinity Cache): NT = non-temporal loads
template <bool NT>
__device__ __forceinline__ d2 ld_stream(const d2* p) {
  return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool NT>
__global__ void __launch_bounds__(256) gemv_t_part_kernel(const double* __restrict__ X, int64_t ld,
                                                          int64_t n, int64_t m,
                                                          const double* __restrict__ v, int rows_per,
                                                          double* __restrict__ part) {
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t r1 = (r0 + rows_per < n) ? r0 + rows_per : n;
  if (c >= m) return;
  const double* col = X + c;
  d2 s = {0.0, 0.0};
  int64_t r = r0;
  for (; r + 8 <= r1; r += 8) {
    d2 x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = ld_stream<NT>(reinterpret_cast<const d2*>(col + (r + u) * ld));
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double vr = v[r + u];
      s.x += x[u].x * vr;
      s.y += x[u].y * vr;
    }
  }
  for (; r < r1; ++r) {
    const d2 x = *reinterpret_cast<const d2*>(col + r * ld);
    const double vr = v[r];
    s.x += x.x * vr;
    s.y += x.y * vr;
  }
  part[(int64_t)blockIdx.y * m + c] = s.x;
  if (c + 1 < m) part[(int64_t)blockIdx.y * m + c + 1] = s.y;
}
__global__ void __launch_bounds__(256) reduce_parts_kernel(const double* __restrict__ part, int64_t m,
                                                           int nparts, double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += part[(int64_t)p * m + c];
  out[c] = s;
}
// out[r] = (sum_c X[r][c] t[c] - v[r]) * inv_lam  (PRECON; otherwise the plain product sum_c X[r][c] t[c]).  One wavefront
// per row, 16-byte loads, four of them in flight per lane.
template <bool NT, bool PRECON = true>
__global__ void __launch_bounds__(256) gemv_n_precon_kernel(const double* __restrict__ X, int64_t ld,
                                                            int64_t n, int64_t m,
                                                            const double* __restrict__ t,
                                                            const double* __restrict__ v, double inv_lam,
                                                            double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const double* row = X + r * ld;
  const int64_t m2 = m & ~(int64_t)1;  // even part: pairs; an odd last column is added by lane 0
  double s0 = 0.0, s1 = 0.0;
  int64_t c = 2 * lane;
  for (; c + 3 * 128 < m2; c += 4 * 128) {
    d2 x[4], tt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      x[u] = ld_stream<NT>(reinterpret_cast<const d2*>(row + c + 128 * u));
      tt[u] = *reinterpret_cast<const d2*>(t + c + 128 * u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      s0 += x[u].x * tt[u].x;
      s1 += x[u].y * tt[u].y;
    }
  }
  for (; c < m2; c += 128) {
    const d2 x = *reinterpret_cast<const d2*>(row + c);
    const d2 tt = *reinterpret_cast<const d2*>(t + c);
    s0 += x.x * tt.x;
    s1 += x.y * tt.y;
  }
  if (lane == 0 && m2 < m) s0 += row[m2] * t[m2];
  const double s = wave_sum(s0 + s1);
  if (lane == 0) out[r] = PRECON ? (s - v[r]) * inv_lam : s;
}

// ---- matrix-free form of the preconditioner (pcg.precon_form): K_mn v is the kernel mat-vec followed by a gather of the
// inducing entries, K_nm t a scatter of t into an n-vector followed by the mat-vec (K is symmetric)
__global__ void __launch_bounds__(256) gather_idx_kernel(const double* __restrict__ s, const int64_t* __restrict__ idx,
                                                         int64_t m, double* __restrict__ t) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < m) t[q] = s[idx[q]];
}
__global__ void __launch_bounds__(256) scatter_idx_kernel(const double* __restrict__ t, const int64_t* __restrict__ idx,
                                                          int64_t m, double* __restrict__ e) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < m) e[idx[q]] = t[q];
}
__global__ void __launch_bounds__(256) precon_finish_kernel(const double* __restrict__ w, const double* __restrict__ v,
                                                            double inv_lam, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (w[i] - v[i]) * inv_lam;
}

typedef float f4 __attribute__((ext_vector_type(4)));
// t_part[rc][c] = sum_{r in chunk rc} X32[r][c] v[r]: a thread owns four adjacent columns (16-byte loads); products and
// sums in fp64 (the fp32 values are exact doubles).  The sums are COMPENSATED (Kahan): what the operator needs from
// X32^T v on the dominant subspace is 1 - lam / (sigma + lam) ~ 1 - 1e-12, and a plain chain of rows_per additions loses
// eps sqrt(rows_per) of that (profiles/r05_f32_diag.txt: 1.4e-2 of the top direction's action against 1.8e-3 for a blocked
// CPU sum, the difference between a 300-iteration plateau and none); the kernel is HBM bound, the four extra additions
// per element are free.
struct KahanSum {
  double s = 0.0, c = 0.0;
  __device__ __forceinline__ void add_prod(double x, double v) {
    const double y = __builtin_fma(x, v, -c);
    const double t = s + y;
    c = (t - s) - y;
    s = t;
  }
  __device__ __forceinline__ void add(double x) {
    const double y = x - c;
    const double t = s + y;
    c = (t - s) - y;
    s = t;
  }
};
template <bool NT>
__global__ void __launch_bounds__(256) gemv_t_part_f32_kernel(const float* __restrict__ X, int64_t ld, int64_t n, int64_t m,
                                                              const double* __restrict__ v, int rows_per,
                                                              double* __restrict__ part) {
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t r1 = (r0 + rows_per < n) ? r0 + rows_per : n;
  if (c >= m) return;
  const float* col = X + c;
  KahanSum s0, s1, s2, s3;
  int64_t r = r0;
  for (; r + 8 <= r1; r += 8) {
    f4 x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const f4* p = reinterpret_cast<const f4*>(col + (r + u) * ld);
      x[u] = NT ? __builtin_nontemporal_load(p) : *p;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double vr = v[r + u];
      s0.add_prod((double)x[u].x, vr);
      s1.add_prod((double)x[u].y, vr);
      s2.add_prod((double)x[u].z, vr);
      s3.add_prod((double)x[u].w, vr);
    }
  }
  for (; r < r1; ++r) {
    const f4 x = *reinterpret_cast<const f4*>(col + r * ld);
    const double vr = v[r];
    s0.add_prod((double)x.x, vr);
    s1.add_prod((double)x.y, vr);
    s2.add_prod((double)x.z, vr);
    s3.add_prod((double)x.w, vr);
  }
  double* o = part + (int64_t)blockIdx.y * m + c;
  o[0] = s0.s;
  if (c + 1 < m) o[1] = s1.s;
  if (c + 2 < m) o[2] = s2.s;
  if (c + 3 < m) o[3] = s3.s;
}
__global__ void __launch_bounds__(256) reduce_parts_kahan_kernel(const double* __restrict__ part, int64_t m, int nparts,
                                                                 double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  KahanSum s;
  for (int p = 0; p < nparts; ++p) s.add(part[(int64_t)p * m + c]);
  out[c] = s.s;
}
// out[r] = (sum_c X32[r][c] t[c] - v[r]) * inv_lam.  A wavefront owns RW consecutive rows: a row of X32 is half as long
// as the fp64 vector t it is multiplied with, so with one row per wavefront the t reads (from L2) would be twice the X32
// reads (from HBM); t is loaded once per RW rows.  t is padded with zeros up to a multiple of 4, X32's pad columns are zero.
template <bool NT, int RW>
__global__ void __launch_bounds__(256) gemv_n_precon_f32_kernel(const float* __restrict__ X, int64_t ld, int64_t n, int64_t m,
                                                                const double* __restrict__ t, const double* __restrict__ v,
                                                                double inv_lam, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RW;
  if (r0 >= n) return;
  const float* row[RW];
#pragma unroll
  for (int k = 0; k < RW; ++k) row[k] = X + ((r0 + k < n) ? r0 + k : n - 1) * ld;
  const int64_t m4 = (m + 3) & ~(int64_t)3;
  double s[RW];
#pragma unroll
  for (int k = 0; k < RW; ++k) s[k] = 0.0;
  int64_t c = 4 * lane;
  for (; c + 256 < m4; c += 512) {
    f4 x[2][RW];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int k = 0; k < RW; ++k) {
        const f4* p = reinterpret_cast<const f4*>(row[k] + c + 256 * u);
        x[u][k] = NT ? __builtin_nontemporal_load(p) : *p;
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const d2 ta = *reinterpret_cast<const d2*>(t + c + 256 * u);
      const d2 tb = *reinterpret_cast<const d2*>(t + c + 256 * u + 2);
#pragma unroll
      for (int k = 0; k < RW; ++k)
        s[k] += ((double)x[u][k].x * ta.x + (double)x[u][k].y * ta.y) + ((double)x[u][k].z * tb.x + (double)x[u][k].w * tb.y);
    }
  }
  for (; c < m4; c += 256) {
    const d2 ta = *reinterpret_cast<const d2*>(t + c);
    const d2 tb = *reinterpret_cast<const d2*>(t + c + 2);
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      const f4 x = *reinterpret_cast<const f4*>(row[k] + c);
      s[k] += ((double)x.x * ta.x + (double)x.y * ta.y) + ((double)x.z * tb.x + (double)x.w * tb.y);
    }
  }
#pragma unroll
  for (int k = 0; k < RW; ++k) {
    const double sk = wave_sum(s[k]);
    if (lane == 0 && r0 + k < n) out[r0 + k] = (sk - v[r0 + k]) * inv_lam;
  }
}

// Matrix-free form: d_out = (K_nm Z Z^T K_mn d_v - d_v)/lam.  The n x m factor X = K_nm Z is never read: K_mn v is the
// kernel mat-vec followed by a gather of the m inducing entries, K_nm t a scatter into an n-vector followed by the
// mat-vec -- 2 x 10 M^2 P D flops and 16 m^2 bytes per application instead of 16 n m bytes (at configs[2]: 2 x 1.0 ms +
// 0.3 ms against 7.8 ms).  Sharded: the mat-vecs are query-sharded and all-gather their result; Z is replicated.
static int precon_apply_mf(gdml_ctx* ctx, double lam, const double* d_v, double* d_out) {
  const int64_t m = ctx->precon_m, n = ctx->precon_n, ld = ctx->K_ld;
  if (!ctx->precon_Z || !ctx->precon_idx) return gdml_fail(ctx, GDML_ERR_STATE, "matrix-free preconditioner not resident");
  if (ctx->world > 1 && ctx->precon_use_E)
    return gdml_fail(ctx, GDML_ERR_UNSUPPORTED, "matrix-free preconditioner: not with sharded energy constraints");
  Model& md = ctx->model;
  if (!md.xp || md.M != ctx->ts.M || md.N != ctx->ts.N || md.P != ctx->ts.P || md.sig != ctx->precon_sig)
    GDML_TRY(operator_model_from_trainset(ctx, ctx->precon_sig));
  int64_t n_pad = n;
  if (ctx->world > 1) {
    int64_t p0, p1, per;
    shard_points(ctx, ctx->ts.M, &p0, &p1, &per);
    n_pad = per * 3 * ctx->ts.N * ctx->world;
    if (n_pad < n) n_pad = n;
  }
  n_pad = (n_pad + 31) / 32 * 32;
  const int64_t m_pad = (m + 31) / 32 * 32;
  const int rows_per = 512;
  const int nparts = (int)((m + rows_per - 1) / rows_per);
  double* buf;
  GDML_TRY(ctx_slot(ctx, SLOT_PRECON_MF, (2 * n_pad + 2 * m_pad + (int64_t)nparts * m_pad) * 8, &buf));
  double* s = buf;            // K v, later K e
  double* e = s + n_pad;      // scattered m-vector
  double* t1 = e + n_pad;
  double* t2 = t1 + m_pad;
  double* part = t2 + m_pad;
  hipStream_t st = ctx->stream;
  const double* Z = ctx->precon_Z;
  GDML_TRY(matvec_device(ctx, 0.0, ctx->precon_use_E, d_v, n, s));
  hipLaunchKernelGGL(gather_idx_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, s, ctx->precon_idx, m, t1);
  hipLaunchKernelGGL(gemv_t_part_kernel<false>, dim3(ceil_div(m, 512), nparts), dim3(256), 0, st, Z, ld, m, m, t1, rows_per,
                     part);
  hipLaunchKernelGGL(reduce_parts_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, part, m, nparts, t2);
  hipLaunchKernelGGL((gemv_n_precon_kernel<false, false>), dim3(ceil_div(m, 4)), dim3(256), 0, st, Z, ld, m, m, t2,
                     (const double*)nullptr, 1.0, t1);
  HIP_CHECK(ctx, hipMemsetAsync(e, 0, n_pad * 8, st));
  hipLaunchKernelGGL(scatter_idx_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, t1, ctx->precon_idx, m, e);
  GDML_TRY(matvec_device(ctx, 0.0, ctx->precon_use_E, e, n, s));
  hipLaunchKernelGGL(precon_finish_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, s, d_v, 1.0 / lam, n, d_out);
  ctx->launch_counter += 7;
  HIP_CHECK(ctx, hipGetLastError());
  return GDML_OK;
}

// ---- one launcher per GEMV kernel: grid and template instantiation (nt, rw) come from the plan
static void launch_gemv_t(gdml_ctx* ctx, const PreconApplyPlan& p, const double* X, int64_t ld, int64_t n, int64_t m,
                          const double* v, double* part) {
  auto* k = p.nt ? gemv_t_part_kernel<true> : gemv_t_part_kernel<false>;
  hipLaunchKernelGGL(k, dim3(p.col_blocks, p.nparts), dim3(256), 0, ctx->stream, X, ld, n, m, v, p.rows_per, part);
}
static void launch_gemv_n(gdml_ctx* ctx, const PreconApplyPlan& p, const double* X, int64_t ld, int64_t n, int64_t m,
                          const double* t, const double* v, double inv_lam, double* out) {
  auto* k = p.nt ? gemv_n_precon_kernel<true> : gemv_n_precon_kernel<false>;
  hipLaunchKernelGGL(k, dim3(p.row_blocks), dim3(256), 0, ctx->stream, X, ld, n, m, t, v, inv_lam, out);
}
static void launch_gemv_t_f32(gdml_ctx* ctx, const PreconApplyPlan& p, const float* X, int64_t ld, int64_t n, int64_t m,
                              const double* v, double* part) {
  auto* k = p.nt ? gemv_t_part_f32_kernel<true> : gemv_t_part_f32_kernel<false>;
  hipLaunchKernelGGL(k, dim3(p.col_blocks, p.nparts), dim3(256), 0, ctx->stream, X, ld, n, m, v, p.rows_per, part);
}
static void launch_gemv_n_f32(gdml_ctx* ctx, const PreconApplyPlan& p, const float* X, int64_t ld, int64_t n, int64_t m,
                              const double* t, const double* v, double inv_lam, double* out) {
  auto* k = p.nt ? gemv_n_precon_f32_kernel<true, 1> : gemv_n_precon_f32_kernel<false, 1>;
  switch (p.rw) {
    case 4: k = p.nt ? gemv_n_precon_f32_kernel<true, 4> : gemv_n_precon_f32_kernel<false, 4>; break;
    case 2: k = p.nt ? gemv_n_precon_f32_kernel<true, 2> : gemv_n_precon_f32_kernel<false, 2>; break;
  }
  hipLaunchKernelGGL(k, dim3(p.row_blocks), dim3(256), 0, ctx->stream, X, ld, n, m, t, v, inv_lam, out);
}

// d_out = (X X^T d_v - d_v)/lam on replicated (padded) device vectors; X row-sharded.  Form 3: (X32 T0 X32^T v - v)/lam, the two
// passes read n_loc x m x 4 bytes each; T0 (m x m, fp64, replicated) in between
int precon_apply_device(gdml_ctx* ctx, double lam, const double* d_v, double* d_out) {
  if (!ctx->precon) return gdml_fail(ctx, GDML_ERR_STATE, "no preconditioner resident");
  if (ctx->precon_form == 1) return precon_apply_mf(ctx, lam, d_v, d_out);
  const ShardGeo sg = shard_geo(ctx);
  const int64_t n_loc = sg.n_loc, m = ctx->precon_m, ld = ctx->K_ld;
  const bool f32 = ctx->precon_form == 3;
  if (f32 && (!ctx->precon_X32 || !ctx->precon_T0)) return gdml_fail(ctx, GDML_ERR_STATE, "fp32 preconditioner not resident");
  const PreconOpts opts = {ctx_opt_i(ctx, "pcg.gemv_plain", 0), ctx_opt_i(ctx, "pcg.f32_rows_per", 1024), ctx_opt_i(ctx, "pcg.f32_rw", 4)};
  const PreconApplyPlan p = precon_apply_plan(ctx->precon_form, n_loc, m, ld, opts);
  double* part;
  GDML_TRY(ctx_slot(ctx, SLOT_PRECON_GEMV, p.ws_bytes, &part));
  double* t = part + p.o_t;
  double* u = part + p.o_u;
  const double *v = d_v + sg.row0, inv_lam = 1.0 / lam;
  const int slot = ktime_begin(ctx);
  if (n_loc > 0) {
    if (f32)
      launch_gemv_t_f32(ctx, p, ctx->precon_X32, ctx->precon_X32_ld, n_loc, m, v, part);
    else
      launch_gemv_t(ctx, p, ctx->precon, ld, n_loc, m, v, part);
    hipLaunchKernelGGL(f32 ? reduce_parts_kahan_kernel : reduce_parts_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, ctx->stream,
                       part, m, p.nparts, t);
  } else {
    HIP_CHECK(ctx, hipMemsetAsync(t, 0, m * 8, ctx->stream));
  }
  GDML_TRY(comm_allreduce_sum(ctx, t, m));
  if (f32) {
    HIP_CHECK(ctx, hipMemsetAsync(u, 0, p.n_u * 8, ctx->stream));  // pad entries [m, m4) stay zero
    hipLaunchKernelGGL((gemv_n_precon_kernel<false, false>), dim3(ceil_div(m, 4)), dim3(256), 0, ctx->stream, ctx->precon_T0,
                       ld, m, m, t, (const double*)nullptr, 1.0, u);
  }
  if (n_loc > 0) {
    if (f32)
      launch_gemv_n_f32(ctx, p, ctx->precon_X32, ctx->precon_X32_ld, n_loc, m, u, v, inv_lam, d_out + sg.row0);
    else
      launch_gemv_n(ctx, p, ctx->precon, ld, n_loc, m, t, v, inv_lam, d_out + sg.row0);
  }
  ktime_end(ctx, slot, "precon_gemv", p.work);
  ctx->launch_counter += p.launches;
  HIP_CHECK(ctx, hipGetLastError());
  return comm_allgather_inplace(ctx, d_out, sg.chunk);
}

extern "C" int gdml_precon_apply(gdml_ctx* ctx, double lam, const double* v, int64_t n, double* out) {
  if (!ctx || !v || !out) return GDML_ERR_INVALID;
  if (!ctx->precon || n != ctx->precon_n)
    return gdml_fail(ctx, GDML_ERR_STATE, "gdml_precon_apply: no matching preconditioner resident");
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const ShardGeo sg = shard_geo(ctx);
  void* buf = nullptr;
  GDML_TRY(ctx_alloc(ctx, &buf, 2 * sg.n_pad * 8));
  double* dv = (double*)buf;
  double* dout = dv + sg.n_pad;
  int rc = GDML_OK;
  hipError_t e = hipMemsetAsync(dv, 0, 2 * sg.n_pad * 8, ctx->stream);
  if (e != hipSuccess) rc = gdml_fail(ctx, GDML_ERR_HIP, "memset: %s", hipGetErrorString(e));
  if (rc == GDML_OK) rc = vec_upload(ctx, sg, v, dv);
  if (rc == GDML_OK) rc = precon_apply_device(ctx, lam, dv, dout);
  if (rc == GDML_OK) rc = vec_download(ctx, sg, dout, out);
  int rc2 = ctx_free(ctx, buf);
  return rc != GDML_OK ? rc : rc2;
}
