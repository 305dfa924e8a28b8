// Host-side plan of the analytic Hessian (hess_device, predict_hess.hip): which projection kernel serves a call, with which
// template selector and LDS, how the batch is sliced, the table rows chunked, grouped and split, and how the workspace is laid
// out.  Plain C++ with no HIP include and no gdml_ctx, so that the decision is a value one can print and test without a GPU
// (tests/hess_plan_driver.cpp, tests/test_hess_plan_cpu.py).
//
// DISPATCH.  D = N (N - 1) / 2 descriptor entries.  D <= 512 (N <= 32): hess_proj_wave_kernel<KPL> (one wavefront per row
// group, KPL = D / 64 rounded up to 1, 2, 4, 8); otherwise hess_proj_kernel<KT>, KT = ceil(D / 256) >= 3 rounded up to 4, 8,
// 16, 32, 48 (N <= 157); above that, or with option predict.hess_generic = 1 (which also skips the wavefront variant), the
// KT = 0 variant.  d must fit the LDS (D <= 19456, N <= 197): larger molecules are GDML_ERR_UNSUPPORTED.  v sits in LDS
// beside d while 2 D doubles fit (always for the wavefront variant, whose four wavefronts hold a d and a v row each).
// Departure from one fused fp64-MFMA kernel with J_x in LDS: projection and rank-2 update are separate passes through
// bounded panels, which keeps every N, P, lattice and energy-constraint case on one deterministic path; the rank-2 update
// is VALU.  The projection pass is the measured bottleneck and the first thing to move onto the MFMA pipe.
// WORKSPACE (one ctx_slot): batches go through in slices of at most 64 queries and the table rows in chunks sized to
// ~256 MiB of panels (option predict.hess_chunk_rows caps the chunk, tests).  Segments, in doubles and in this order:
//   U, W     (Bs, nr_cap, ld) each   the projected panels of a chunk
//   cs       (Bs, nr_cap, 2)         gam, s per row
//   part_F   (G, Bs, D)              group partials of F_x
//   part_ET  (G, Bs, 2)              group partials of E', tau
//   Hp       (JS, Bs, ld, ld)        split partials of H
//   fx, tau  (Bs, D), (Bs)           F_x and tau per query
#pragma once
#include <stddef.h>
#include <stdint.h>

// tile constants of the kernels (predict_hess.hip), which the plan has to respect
constexpr int HT = 64;  // H tile edge (rank2 / epilogue)
constexpr int HK = 16;  // table rows per LDS stage of the rank-2 kernel
constexpr int HE = 16;  // H rows per workgroup of the epilogue
constexpr int64_t HESS_PANEL_BYTES = 256ll << 20;
constexpr int64_t HESS_LDS_MAX = 152 * 1024;

enum HessVariant { HESS_WAVE = 0, HESS_BLOCK = 1 };

struct HessPlanIn {
  int N;
  int64_t MP, B;       // table rows, queries (both >= 1)
  int generic;         // option predict.hess_generic
  int64_t chunk_rows;  // option predict.hess_chunk_rows (0: no cap)
};

// one chunk of table rows, [r0, r0 + nr)
struct HessChunk {
  int64_t nr, groups;  // rows; row groups of RG (the last may be short)
  unsigned grid_x;     // of the projection: a workgroup per group, or per four groups (wave)
  int64_t rps;         // rows per split of the rank-2 update
  int accumulate;      // later chunks add onto the partials of the first
};

struct HessPlan {
  bool supported;  // false: nothing below is set
  HessVariant variant;
  int sel;  // template selector: KPL (wave), KT (block)
  int v_lds;
  size_t lds_bytes;  // dynamic LDS of the projection
  int D, n3, nb, ld, n_tp;  // nb tiles of HT along 3N, ld = nb HT, n_tp lower tile pairs
  int64_t MP, B;
  int64_t Bs;  // queries per batch slice
  int RG;      // rows per projection group (a workgroup, or a wavefront of the wave variant)
  int64_t nr_cap, G, JS;  // rows per chunk (a multiple of RG), groups of the first chunk, rank-2 splits
  int64_t nU, nCS, nPF, nPE, nHp, nFX, nTau;  // workspace segments in doubles (U and W: nU each)
  int64_t oW, oCS, oPF, oPE, oHp, oFX, oTau;  // where each begins, in doubles (U at 0)
  int64_t ws_bytes;

  HessChunk chunk(int64_t r0) const {
    HessChunk c;
    c.nr = MP - r0 < nr_cap ? MP - r0 : nr_cap;
    c.groups = (c.nr + RG - 1) / RG;
    c.grid_x = (unsigned)(variant == HESS_WAVE ? (c.groups + 3) / 4 : c.groups);
    c.rps = (c.nr + JS - 1) / JS;
    c.accumulate = r0 > 0;
    return c;
  }
  int slice(int64_t b0) const { return (int)(B - b0 < Bs ? B - b0 : Bs); }
};

inline HessPlan hess_plan(const HessPlanIn& in) {
  HessPlan p = {};
  const int N = in.N, D = N * (N - 1) / 2, n3 = 3 * N;
  const int64_t MP = in.MP, B = in.B;
  p.supported = (int64_t)D * 8 <= HESS_LDS_MAX;
  if (!p.supported) return p;
  p.D = D; p.n3 = n3; p.MP = MP; p.B = B;
  const int nb = (n3 + HT - 1) / HT, ld = nb * HT, n_tp = nb * (nb + 1) / 2;
  p.nb = nb; p.ld = ld; p.n_tp = n_tp;
  int kt = (D + 255) / 256;
  int KT = 1;
  while (KT < kt) KT <<= 1;
  if (KT == 64 && kt <= 48) KT = 48;
  if (kt > 48 || in.generic) KT = 0;
  // wavefront-per-row-group projection for small descriptors (D <= 512; at D = 861 it ran at half the block variant's rate)
  int KPL = 1;
  while (KPL * 64 < D) KPL <<= 1;
  const bool wave = D <= 512 && !in.generic;
  p.variant = wave ? HESS_WAVE : HESS_BLOCK;
  p.sel = wave ? KPL : KT;
  p.v_lds = wave || (int64_t)2 * D * 8 <= HESS_LDS_MAX;
  p.lds_bytes = wave ? (size_t)8 * D * 8 : (size_t)(p.v_lds ? 2 : 1) * D * 8;

  // batch slice (bounded partial-H workspace), rows per projection group, row chunk, rank-2 splits
  int64_t Bs = B < 64 ? B : 64;
  // never fires: ld <= 640 (N <= 197), and 64 slices of 640 x 640 doubles are 200 MiB.  Kept for a larger HT or LDS row.
  while (Bs > 1 && Bs * (int64_t)ld * ld * 8 > HESS_PANEL_BYTES) Bs >>= 1;
  int64_t nr_cap = HESS_PANEL_BYTES / (Bs * ((int64_t)ld * 16 + 16));
  if (in.chunk_rows > 0 && in.chunk_rows < nr_cap) nr_cap = in.chunk_rows;
  if (nr_cap > MP) nr_cap = MP;
  int RG = 256;  // enough groups per chunk to fill the chip
  while (RG > (wave ? 4 : 8) && ((nr_cap + RG - 1) / RG) * Bs < 4096) RG >>= 1;
  nr_cap = (nr_cap + RG - 1) / RG * RG;  // a multiple of RG: every chunk but the last has full groups
  // groups of the first (largest) chunk; later chunks add their group partials of F_x, E', tau onto these
  const int64_t G = ((MP < nr_cap ? MP : nr_cap) + RG - 1) / RG;
  int64_t JS = (1024 + n_tp * Bs - 1) / (n_tp * Bs);
  const int64_t js_max = nr_cap / 64 > 1 ? nr_cap / 64 : 1;
  if (JS > js_max) JS = js_max;
  if (JS < 1) JS = 1;
  p.Bs = Bs; p.RG = RG; p.nr_cap = nr_cap; p.G = G; p.JS = JS;

  p.nU = Bs * nr_cap * ld;
  p.nCS = Bs * nr_cap * 2;
  p.nPF = G * Bs * D;
  p.nPE = G * Bs * 2;
  p.nHp = JS * Bs * (int64_t)ld * ld;
  p.nFX = Bs * (int64_t)D;
  p.nTau = Bs;
  p.oW = p.nU;
  p.oCS = p.oW + p.nU;
  p.oPF = p.oCS + p.nCS;
  p.oPE = p.oPF + p.nPF;
  p.oHp = p.oPE + p.nPE;
  p.oFX = p.oHp + p.nHp;
  p.oTau = p.oFX + p.nFX;
  p.ws_bytes = (p.oTau + p.nTau) * 8;
  return p;
}
