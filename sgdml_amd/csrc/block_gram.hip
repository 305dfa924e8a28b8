// Z Z^T of tall row blocks on the fp64 MFMA pipe, and the chunking of such blocks: the part that the posterior covariance
// (uncert.hip: Z_q = (-Kx_q) L^-T, one block per query) and the leave-one-out pass (loo.hip: Z_j = E_j^T L^-T, one block per
// training point) share.  An ITEM is one block of n3 = 3N consecutive rows of the row buffer (pitch ld).
#include "common.h"

typedef double d4 __attribute__((ext_vector_type(4)));

// The one place the k splits are planned: S and L depend on n alone, never on how the items were cut into chunks -- the
// chunk invariance of both callers and "the variances are the diagonal of the full covariance" rest on that.
GramSplit gram_split(int64_t n, int n3) {
  GramSplit g;
  g.n = n; g.n3 = n3;
  g.ld = round16(n);
  g.nblk = (n3 + 63) / 64;
  g.npairs = g.nblk * (g.nblk + 1) / 2;
  g.S = (int)((n + 1023) / 1024);
  if (g.S > 32) g.S = 32;
  if (g.S < 1) g.S = 1;
  g.L = round16((g.ld + g.S - 1) / g.S);
  g.S = (int)((g.ld + g.L - 1) / g.L);  // no empty split
  return g;
}

// Chunk of the items and its two buffers: the option's cap, the item count, then halved while the row buffer (with up to 127
// pad rows) and the workspace exceed 90 % of free memory plus the two slots already held.
int gram_workspace(gdml_ctx* ctx, const GramSplit& g, const char* chunk_opt, int64_t items, int64_t ws_per_item, int64_t ws_fixed,
                   int64_t* chunk, double** rows, double** ws) {
  int64_t bc = ctx_opt_i(ctx, chunk_opt, 64);  // 64 items: 2 GB of rows at n = 63 000
  if (bc < 1) bc = 1;
  if (bc > items) bc = items;
  size_t f = 0, t = 0;
  HIP_CHECK(ctx, hipMemGetInfo(&f, &t));
  const int64_t have = (int64_t)f + ctx->slot_bytes[SLOT_GRAM_WS] + ctx->slot_bytes[SLOT_GRAM_ROWS];
  while (bc > 1 && (bc * (g.n3 * g.ld + ws_per_item) + 127 * g.ld + ws_fixed) * 8 > have / 10 * 9) bc = (bc + 1) / 2;
  *chunk = bc;
  GDML_TRY(ctx_slot(ctx, SLOT_GRAM_ROWS, pad_rows128(bc * g.n3) * g.ld * 8, rows));
  return ctx_slot(ctx, SLOT_GRAM_WS, (ws_fixed + bc * ws_per_item) * 8, ws);
}

// The n3 x n3 output is cut into 64 x 64 blocks (4 x 4 MFMA tiles of v_mfma_f64_16x16x4_f64); one WAVEFRONT owns (item, lower
// block pair (I, J), k split s): both operands are rows of Z and come straight from global memory as 32-byte runs (lane group
// g = lane >> 4 feeds k = 4 g + step into MFMA step `step`, the same bijection on both sides -- as in the panel solve of
// chol.hip), rows past n3 re-read row n3 - 1 (their results are never read).  The pad columns [n, ld) of Z are zero, so the
// k loop needs no edge.  The S partial tiles of a block go to scratch and the caller sums them in the order s = 0 .. S - 1:
// no atomics, bit-reproducible.  DIAG runs the SAME MFMA sequence for the diagonal tiles (it only leaves the others out).
// An item whose rows are zero left of column `first` skips the splits wholly left of it (the tile is not written: the caller
// does not read it) and starts the first split it keeps at `first` rounded down to 16; first = 0 changes nothing.
// The rows may lie in a wider buffer (pitch > ld: extend.hip sums over the first ld columns of rows of the factor).
struct BlockGramArgs {
  const double* Z;
  double* part;  // full: [item][pair][s][64 x 64]; DIAG: [item][block][s][64]
  int64_t ld, pitch, L, units, first0, first_stride;
  int n3, nblk, npairs, S;
};

template <bool DIAG>
__global__ void __launch_bounds__(256) block_gram_kernel(BlockGramArgs g) {
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= g.units) return;
  const int s = (int)(unit % g.S);
  const int64_t up = unit / g.S;
  const int pr = (int)(up % g.npairs);
  const int64_t q = up / g.npairs;
  const int64_t first = g.first0 + q * g.first_stride;
  int64_t k_beg = (int64_t)s * g.L;
  const int64_t k_end = k_beg + g.L < g.ld ? k_beg + g.L : g.ld;
  if (k_end <= first) return;
  if (k_beg < first) k_beg = first / 16 * 16;
  int I, J;
  if (DIAG) {
    I = J = pr;
  } else {
    I = (int)((sqrt(8.0 * (double)pr + 1.0) - 1.0) * 0.5);
    while (I * (I + 1) / 2 > pr) --I;
    while ((I + 1) * (I + 2) / 2 <= pr) ++I;
    J = pr - I * (I + 1) / 2;
  }
  const double* pa[4];
  const double* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int ra = I * 64 + 16 * i + li, rb = J * 64 + 16 * i + li;
    ra = ra < g.n3 ? ra : g.n3 - 1;
    rb = rb < g.n3 ? rb : g.n3 - 1;
    pa[i] = g.Z + (q * g.n3 + ra) * g.pitch + 4 * lk;
    pb[i] = g.Z + (q * g.n3 + rb) * g.pitch + 4 * lk;
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
    for (int i = 0; i < 4; ++i) bv[i] = DIAG ? av[i] : *reinterpret_cast<const d4*>(pb[i] + k0);
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (!DIAG || i == j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i][st], bv[j][st], acc[i][j], 0, 0, 0);
  }
  // f64 MFMA C/D layout: col = lane & 15, row = (lane >> 4) + 4 r
  if (DIAG) {
    double* o = g.part + ((q * g.nblk + I) * g.S + s) * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (li == lk + 4 * r) o[16 * i + li] = acc[i][i][r];
  } else {
    double* o = g.part + ((q * g.npairs + pr) * g.S + s) * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(16 * i + lk + 4 * r) * 64 + 16 * j + li] = acc[i][j][r];
  }
}

void block_gram_launch(gdml_ctx* ctx, const GramSplit& s, const double* Z, double* part, int64_t items, bool diag, int64_t first0,
                       int64_t first_stride, int64_t pitch) {
  BlockGramArgs g;
  g.Z = Z; g.part = part; g.ld = s.ld; g.pitch = pitch > 0 ? pitch : s.ld; g.L = s.L; g.first0 = first0; g.first_stride = first_stride;
  g.n3 = s.n3; g.nblk = s.nblk; g.S = s.S;
  g.npairs = diag ? s.nblk : s.npairs;
  g.units = items * g.npairs * g.S;
  const dim3 grid((unsigned)ceil_div(g.units, 4));
  if (diag)
    hipLaunchKernelGGL(block_gram_kernel<true>, grid, dim3(256), 0, ctx->stream, g);
  else
    hipLaunchKernelGGL(block_gram_kernel<false>, grid, dim3(256), 0, ctx->stream, g);
  ctx->launch_counter++;
}
