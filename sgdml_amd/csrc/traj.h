// What the on-device trajectory entries (gdml_md_run in md.hip, gdml_pimd_run in pimd.hip, gdml_relax_run in relax.hip,
// gdml_neb_run in neb.hip, gdml_cell_relax_run in cellrelax.hip, gdml_ef_run in ef.hip) share:
// the counter-based noise, the fixed reduction tree, the argument checks and prelude, the recorder of a chunk of frames and
// the chunk loop of the two MD entries, and the chunk loop of the four entries whose replicas freeze on their own
// (gdml_relax_run, gdml_neb_run, gdml_cell_relax_run, gdml_ef_run), whose host-only part is traj_host.h's.
#pragma once
#include <math.h>

#include <vector>

#include "common.h"
#include "traj_host.h"

// ---- Philox4x32-10 (Salmon et al., SC'11), key = (seed lo, seed hi), counter = (step lo, step hi, replica, block) -------------
struct Philox4 {
  uint32_t v[4];
};

__host__ __device__ static inline Philox4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                                        uint32_t c3) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Philox4 o;
  o.v[0] = c0;
  o.v[1] = c1;
  o.v[2] = c2;
  o.v[3] = c3;
  return o;
}

// standard normal of coordinate `coord` of replica `rep` at absolute step `step`: block = coord / 4, the block's outputs
// (x0, x1) and (x2, x3) are two Box-Muller pairs, u = (x + 0.5) 2^-32 in (0, 1)
__device__ static inline double md_normal(uint64_t seed, uint64_t step, uint32_t rep, int64_t coord) {
  const Philox4 o = philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32), rep,
                                  (uint32_t)(coord >> 2));
  const int j = (int)(coord & 3);
  const double u0 = ((double)o.v[j & 2] + 0.5) * 2.3283064365386963e-10;
  const double u1 = ((double)o.v[(j & 2) + 1] + 0.5) * 2.3283064365386963e-10;
  const double rad = sqrt(-2.0 * log(u0));
  const double ang = 6.283185307179586 * u1;
  return (j & 1) ? rad * sin(ang) : rad * cos(ang);
}

// The 256-slot tree of every per-replica sum: rows [0, NSUM) of red are summed, rows [NSUM, NSUM + NMAX) reduced to their
// maximum, results in slot 0 of each row.  Called by all 256 threads after a barrier behind their writes to red; every thread
// may read the results when it returns.
template <int NSUM, int NMAX = 0>
__device__ __forceinline__ void block_tree_sum(double (*red)[256], int tid) {
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int c = 0; c < NSUM; ++c) red[c][tid] += red[c][tid + s];
#pragma unroll
      for (int c = NSUM; c < NSUM + NMAX; ++c) red[c][tid] = red[c][tid + s] > red[c][tid] ? red[c][tid + s] : red[c][tid];
    }
    __syncthreads();
  }
}

static __global__ void __launch_bounds__(256) traj_fill_i64_kernel(int64_t* p, int64_t n, int64_t v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---- argument checks: fn is the entry's name, the prefix of every message; ctx may be NULL (the message then goes where
// gdml_ctx_create's goes).  Each entry calls them in the order in which it has always tested its arguments. ------------------
static inline int traj_check_shape(gdml_ctx* ctx, const char* fn, int64_t B, int N) {
  if (B < 0 || B > 0x7fffffffLL) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: B out of range", fn);
  if (N < 1 || N > GDML_MAX_ATOMS) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: N out of range", fn);
  return GDML_OK;
}
static inline int traj_check_f_scale(gdml_ctx* ctx, const char* fn, double f_scale) {
  if (!isfinite(f_scale)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: f_scale is not finite", fn);
  return GDML_OK;
}
static inline int traj_check_lattice(gdml_ctx* ctx, const char* fn, const double* lat, const double* lat_inv) {
  if ((lat == nullptr) != (lat_inv == nullptr))
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: lattice and inverse must both be given or both NULL", fn);
  return GDML_OK;
}
// the two MD entries: head (params, n_steps, record_every), integrator (dt, f_scale, mass, lattice, thermostat; the second
// thermostat's name differs) and tail (step0, R, V)
static inline int traj_check_md_head(gdml_ctx* ctx, const char* fn, const void* params, int64_t n_steps, int64_t record_every) {
  if (!params) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: params is NULL", fn);
  if (n_steps < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: n_steps < 0", fn);
  if (record_every < 1) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: record_every < 1", fn);
  return GDML_OK;
}
static inline int traj_check_md_integrator(gdml_ctx* ctx, const char* fn, int N, double dt, double f_scale, const double* mass,
                                           const double* lat, const double* lat_inv, int thermostat, const char* thermostat_1) {
  if (!(dt > 0.0) || !isfinite(dt)) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: dt must be positive and finite", fn);
  GDML_TRY(traj_check_f_scale(ctx, fn, f_scale));
  if (!mass) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: mass is NULL", fn);
  for (int a = 0; a < N; ++a)
    if (!(mass[a] > 0.0) || !isfinite(mass[a]))
      return gdml_fail(ctx, GDML_ERR_INVALID, "%s: mass of atom %d must be positive and finite", fn, a);
  GDML_TRY(traj_check_lattice(ctx, fn, lat, lat_inv));
  if (thermostat != 0 && thermostat != 1)
    return gdml_fail(ctx, GDML_ERR_INVALID, "%s: thermostat must be 0 (none) or 1 (%s)", fn, thermostat_1);
  return GDML_OK;
}
static inline int traj_check_md_tail(gdml_ctx* ctx, const char* fn, int64_t step0, const double* R, const double* V) {
  if (step0 < 0) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: step0 < 0", fn);
  if (!R || !V) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: R or V is NULL", fn);
  return GDML_OK;
}

// What follows the checks in every entry: context, model, N match, first_bad_step filled with -1, device.  *run = false: B = 0,
// nothing to do.
static inline int traj_prelude(gdml_ctx* ctx, const char* fn, int N, int64_t B, int64_t* first_bad_step, bool* run) {
  *run = false;
  if (!ctx) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: ctx is NULL", fn);
  const Model& md = ctx->model;
  if (!md.xp) return gdml_fail(ctx, GDML_ERR_STATE, "%s: upload a model first", fn);
  if (md.N != N) return gdml_fail(ctx, GDML_ERR_INVALID, "%s: N = %d but the model has %d atoms", fn, N, md.N);
  if (first_bad_step)
    for (int64_t b = 0; b < B; ++b) first_bad_step[b] = -1;
  if (B == 0) return GDML_OK;
  HIP_CHECK(ctx, hipSetDevice(ctx->device));
  *run = true;
  return GDML_OK;
}

// most bytes of frames, and most steps, queued between two synchronisations
static constexpr int64_t MD_CHUNK_BYTES = 64ll << 20;
static constexpr int64_t MD_CHUNK_STEPS = 4096;

// The frames of one chunk in device memory, field by field, and their way to the caller's arrays.
struct Recorder {
  struct Field {
    double* host;  // the caller's (frames, len) array; null: not wanted
    int64_t len;   // doubles per frame
    bool always;   // the kernels write it whether wanted or not: it has device space without a host array
    double* dev;   // chunk base (null: no device space)
  };
  Field f[6];
  int n = 0;
  int64_t frames = 0;  // frames of a chunk
  int64_t done = 0;    // frames flushed so far

  int add(double* host, int64_t len, bool always = false) {
    f[n] = Field{host, len, always, nullptr};
    return n++;
  }
  int64_t frame_len() const {
    int64_t s = 0;
    for (int i = 0; i < n; ++i)
      if (f[i].host || f[i].always) s += f[i].len;
    return s;
  }
  // frames per chunk: MD_CHUNK_BYTES of them, option predict.md_chunk_frames where smaller, at least one, at most `most`
  // (0: nothing will be recorded)
  void size(const gdml_ctx* ctx, int64_t most) {
    frames = 0;
    if (frame_len() == 0) return;
    frames = MD_CHUNK_BYTES / (frame_len() * 8);
    const int64_t opt = (int64_t)ctx_opt(ctx, "predict.md_chunk_frames", 0.0);
    if (opt > 0 && opt < frames) frames = opt;
    if (frames < 1) frames = 1;
    if (frames > most) frames = most;
  }
  int64_t len() const { return frames * frame_len(); }  // doubles of the chunk
  double* carve(double* p) {                            // the fields side by side from p; returns the end
    for (int i = 0; i < n; ++i)
      if (f[i].host || f[i].always) {
        f[i].dev = p;
        p += frames * f[i].len;
      }
    return p;
  }
  double* slot(int i, int64_t frame) const { return f[i].dev ? f[i].dev + frame * f[i].len : nullptr; }
  hipError_t flush(hipStream_t st, int64_t in_chunk) {  // the chunk's first in_chunk frames behind those flushed before
    for (int i = 0; i < n; ++i)
      if (f[i].host) {
        const hipError_t e =
            hipMemcpyAsync(f[i].host + done * f[i].len, f[i].dev, (size_t)(in_chunk * f[i].len) * 8, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return e;
      }
    done += in_chunk;
    return hipSuccess;
  }
};

// The chunk loop of gdml_md_run and gdml_pimd_run: enqueue(t, frame) queues step t = 0 .. n_steps - 1 on ctx->stream; frame is
// the chunk slot that step t + 1's state goes to, or -1 when it is not recorded.  Per chunk (bounded in frames and in queued
// steps): flush, the bad flags (d_bad, B of them) into h_bad, ONE synchronisation; a flag set ends the run (the caller reads
// first_bad_step; frames up to that chunk are written).
template <class Enqueue>
static int traj_run_chunks(gdml_ctx* ctx, Recorder& rec, int64_t n_steps, int64_t record_every, const int64_t* d_bad,
                           std::vector<int64_t>& h_bad, Enqueue&& enqueue) {
  hipStream_t st = ctx->stream;
  int64_t t = 0;
  while (t < n_steps) {
    int64_t in_chunk = 0, steps = 0;
    while (t < n_steps && steps < MD_CHUNK_STEPS && (rec.frames == 0 || in_chunk < rec.frames)) {
      const bool record = (t + 1) % record_every == 0;
      GDML_TRY(enqueue(t, record ? in_chunk : (int64_t)-1));
      if (record) ++in_chunk;
      ++t;
      ++steps;
    }
    HIP_CHECK(ctx, hipGetLastError());
    if (in_chunk > 0) HIP_CHECK(ctx, rec.flush(st, in_chunk));
    HIP_CHECK(ctx, hipMemcpyAsync(h_bad.data(), d_bad, h_bad.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipStreamSynchronize(st));
    bool any_bad = false;
    for (const int64_t b : h_bad) any_bad |= b >= 0;
    if (any_bad) break;
  }
  return GDML_OK;
}

// A run of one of the four entries whose replicas (geometries, bands) freeze on their own.  Device layout, side by side so that
// ONE copy per chunk brings all of it to the host: status (B,2) | bad (B) | history 0 .. n_hist - 1, (chunk_steps,B) each.  A
// history is 8-byte words (doubles, or int64 as gdml_ef_run's k_follow_hist); its rows go on into hist[h] (max_steps + 1, B).
struct FrozenRun {
  int64_t B, max_steps, record_every, chunk_steps;
  int n_hist;
  void* hist[4];             // the caller's arrays; null: not wanted
  int64_t* d_flags;          // device base (carve)
  std::vector<int64_t> h_out;  // the last chunk as read back: h_out.data() = status, + 2 B = bad
  int64_t t;                 // evaluations queued

  int64_t words() const { return 3 * B + n_hist * chunk_steps * B; }
  double* carve(double* p) {  // takes words() from p; returns the end
    d_flags = (int64_t*)p;
    return p + words();
  }
  int64_t* status() const { return d_flags; }
  int64_t* bad() const { return d_flags + 2 * B; }
  double* row(int h, int64_t r) const { return (double*)(d_flags + 3 * B + (h * chunk_steps + r) * B); }
  // behind the run: status and first_bad_step (may be null) for the caller, then what frozen replicas repeat
  void finish(int64_t* status_out, int64_t* first_bad_step, const TrajFrames* fr, int n_fr) {
    memcpy(status_out, h_out.data(), (size_t)(2 * B) * 8);
    if (first_bad_step) memcpy(first_bad_step, h_out.data() + 2 * B, (size_t)B * 8);
    traj_repeat_frozen(h_out.data(), B, t, record_every, hist, n_hist, fr, n_fr);
  }
};

// evaluations per chunk of such a run: option predict.relax_chunk_steps, at least one, at most all max_steps + 1
static inline int64_t traj_frozen_chunk_steps(const gdml_ctx* ctx, int64_t max_steps) {
  const int64_t c = (int64_t)ctx_opt(ctx, "predict.relax_chunk_steps", 32.0);
  return std::min(std::max(c, (int64_t)1), max_steps + 1);
}

// The chunk loop of such a run: status and bad start at -1; enqueue(t, row, frame, last) queues evaluation t = 0 .. max_steps on
// ctx->stream; row = its row in the chunk's histories (run.row(h, row)), frame = the chunk slot of its recorded frame or -1,
// last = (t == max_steps).  Per chunk (traj_next_chunk): flush, the ONE copy, ONE synchronisation.  Ends when no status word
// says active (-1), a bad flag is set or the budget is used up.
template <class Enqueue>
static int traj_run_until_frozen(gdml_ctx* ctx, Recorder& rec, bool record, FrozenRun& run, Enqueue&& enqueue) {
  hipStream_t st = ctx->stream;
  traj_fill_i64_kernel<<<ceil_div(3 * run.B, 256), 256, 0, st>>>(run.d_flags, 3 * run.B, -1);
  run.h_out.assign((size_t)run.words(), -1);
  run.t = 0;
  for (bool go = true; go && run.t <= run.max_steps;) {
    const TrajChunk c = traj_next_chunk(run.t, run.max_steps, run.chunk_steps, record, run.record_every, rec.frames);
    for (int64_t t = c.t0; t < c.t1; ++t) GDML_TRY(enqueue(t, c.row(t), c.frame(t), (int)(t == run.max_steps)));
    run.t = c.t1;
    HIP_CHECK(ctx, hipGetLastError());
    if (c.frames > 0) HIP_CHECK(ctx, rec.flush(st, c.frames));
    HIP_CHECK(ctx, hipMemcpyAsync(run.h_out.data(), run.d_flags, (size_t)run.words() * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(ctx, hipStreamSynchronize(st));
    go = traj_take_chunk(c, run.h_out.data(), run.B, run.chunk_steps, run.hist, run.n_hist);
  }
  return GDML_OK;
}
