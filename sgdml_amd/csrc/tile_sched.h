// Tile schedule of the lower (SYRK-shaped) trailing updates: which workgroup of a launch computes which 128 x 128 C tile.
//
// Two enumerations, both plain functions that compile for the host too (tests/tile_balance_driver.cpp runs the decode
// for every block index of a launch):
//   tile_decode_super   the 8 x 8 super-tile enumeration (block b -> XCD b % 8, super tile s -> XCD s % 8, 64 block slots
//                       per super tile whatever it holds).  Rectangular, cyclic and overwrite launches, and every launch
//                       with gemm.balance = 0.
//   tile_decode_bal     balanced: every XCD gets the same number of tiles (+- 1) and no workgroup is empty except the
//                       padding of the grid to a multiple of 8.  Per XCD the sequence is
//                         [head tiles (table)] [full super tiles, 64 slots each (analytic)] [tail tiles (table)]
//                       Full super tiles (64 tiles, strictly below the super diagonal, whole super rows) stay whole and on
//                       one XCD, in ROUNDS of 8 (one per XCD).  Everything else -- diagonal super tiles, the ragged last
//                       super row, the < 8 full super tiles that do not fill a round -- is a list of single tiles in the
//                       old order, dealt in contiguous runs.  With the first-column-first form the tiles of super column 0
//                       that are not in a round form the head, everything else the tail.
// The schedule of an outer step (one list, one or two launches) is built on the host by tile_sched_build.
#pragma once
#include <array>
#include <math.h>
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__)
#define TS_HD __host__ __device__ __forceinline__
#else
#define TS_HD inline
#endif

// t = I (I + 1) / 2 + J, 0 <= J <= I
TS_HD void ts_tri(int64_t t, int64_t* I, int64_t* J) {
  int64_t i = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (i * (i + 1) / 2 > t) --i;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  *I = i;
  *J = t - i * (i + 1) / 2;
}

// ---- super-tile enumeration -------------------------------------------------------------------------------------
// block b (second problem's blocks already taken off) -> tile; false: the block has no tile.  Super tiles [s_begin, n_super).
TS_HD bool tile_decode_super(int64_t b, int lower, int col0_first, int tiles_m, int tiles_n, int super_n, int64_t s_begin,
                             int64_t n_super, int64_t* ti_out, int64_t* tj_out) {
  const int64_t xcd = b & 7, loc = b >> 3;
  const int64_t s = s_begin + (loc >> 6) * 8 + xcd;
  const int within = (int)(loc & 63);
  if (s >= n_super) return false;
  int64_t SI = 0, SJ = 0;
  if (lower) {
    int64_t sr = s, shift = 0;
    const int64_t sm = (tiles_m + 7) / 8;
    if (col0_first) {  // column SJ = 0 (all SI) first, then the lower triangle of the remaining sm - 1 super rows
      if (s < sm) { SI = s; SJ = 0; sr = -1; }
      else { sr = s - sm; shift = 1; }
    }
    if (sr >= 0) {
      ts_tri(sr, &SI, &SJ);
      SI += shift; SJ += shift;
    }
  } else {
    SI = s / super_n;
    SJ = s - SI * super_n;
  }
  const int64_t ti = SI * 8 + (within >> 3), tj = SJ * 8 + (within & 7);
  if (ti >= tiles_m || tj >= tiles_n) return false;
  if (lower && tj > ti) return false;
  *ti_out = ti; *tj_out = tj;
  return true;
}

// ---- balanced enumeration ---------------------------------------------------------------------------------------
struct TileLaunch {         // what the workgroups of one launch decode from (kernel argument)
  const uint32_t* table;    // [8][stride]: XCD x's head tiles, then its tail tiles; entry = ti | tj << 16
  int stride;
  int r0, r1;               // rounds [r0, r1) of the full-super-tile list
  int nh;                   // col0_first: the first nh full super tiles of the list are (SI = 1 .. nh, SJ = 0)
  int col0_first;
  uint64_t hn[2], tn[2];    // head / tail tiles per XCD, 16 bits each (XCD x: word x >> 2, bits 16 (x & 3) ...)
};

TS_HD int ts_unpack(const uint64_t (&w)[2], int x) { return (int)((w[x >> 2] >> (16 * (x & 3))) & 0xffff); }

// f-th full super tile of the list
TS_HD void ts_full_super(int64_t f, int col0_first, int nh, int64_t* SI, int64_t* SJ) {
  if (col0_first) {
    if (f < nh) { *SI = f + 1; *SJ = 0; return; }
    ts_tri(f - nh, SI, SJ);  // super rows 2 .., super columns 1 .. SI - 1
    *SI += 2; *SJ += 1;
  } else {
    ts_tri(f, SI, SJ);       // super rows 1 .., super columns 0 .. SI - 1
    *SI += 1;
  }
}

// block b -> tile: ONE table load at most, and its address depends on kernel arguments only
TS_HD bool tile_decode_bal(const TileLaunch& L, int64_t b, int64_t* ti, int64_t* tj) {
  const int x = (int)(b & 7);
  const int64_t pos = b >> 3;
  const int hn = ts_unpack(L.hn, x);
  const int64_t q = pos - hn, full_slots = (int64_t)(L.r1 - L.r0) * 64;
  if (q >= 0 && q < full_slots) {
    int64_t SI, SJ;
    ts_full_super(((int64_t)L.r0 + (q >> 6)) * 8 + x, L.col0_first, L.nh, &SI, &SJ);
    *ti = SI * 8 + ((q & 63) >> 3);
    *tj = SJ * 8 + (q & 7);
    return true;
  }
  int64_t e = pos;  // head entry
  if (q >= 0) {
    e = q - full_slots;  // tail entry
    if (e >= ts_unpack(L.tn, x)) return false;
    e += hn;
  }
  uint32_t v = L.table[(int64_t)x * L.stride + e];
#if defined(__HIP_DEVICE_COMPILE__)
  v = __builtin_amdgcn_readfirstlane(v);  // workgroup-uniform: the tile's corner stays in scalar registers
#endif
  *ti = v & 0xffff;
  *tj = v >> 16;
  return true;
}

// second problem (M2 x N2, tiles above the diagonal of its leading N2 x N2 block skipped), compact form: the
// tn2 (tn2 + 1) / 2 lower tiles of the leading block row by row, then the rows below; needs ceil(M2 / GT) >= tn2
TS_HD void tile_decode_second(int64_t b, int tn2, int64_t* ti, int64_t* tj) {
  const int64_t nlow = (int64_t)tn2 * (tn2 + 1) / 2;
  if (b < nlow) { ts_tri(b, ti, tj); return; }
  const int64_t r = b - nlow;
  *ti = tn2 + r / tn2;
  *tj = r % tn2;
}

// ---- host scheduler (no HIP calls) ------------------------------------------------------------------------------

struct TileSched {
  bool ok = false;               // false: shape outside the balanced form (the launch keeps the super-tile enumeration)
  int n_launch = 1;
  TileLaunch L[2] = {};          // L[l].table is left null: the caller points it at its copy of table[l]
  std::vector<uint32_t> table[2];
  int64_t blocks[2] = {0, 0};    // grid of the tile list (multiple of 8)
  double base_last[8] = {};      // the other work the list was dealt around (tile_sched_build's argument)
  int64_t tiles[2] = {0, 0};
  // tiles per launch by kind, for the flop count: off-diagonal / diagonal, above / in the last tile row
  int64_t off_int[2] = {0, 0}, off_last[2] = {0, 0}, diag_int[2] = {0, 0}, diag_last[2] = {0, 0};
};

namespace ts_detail {
struct Deal { std::vector<uint32_t> t[8]; };

// tiles (in order) -> contiguous runs per XCD so that prior[x] + run[x] are equal (+- 1); the XCDs that take the extra
// tile are those that already hold it, then those with the least other work (base)
inline void deal(const std::vector<uint32_t>& tiles, const int64_t prior[8], const double base[8], Deal* d) {
  int64_t total = (int64_t)tiles.size();
  for (int x = 0; x < 8; ++x) total += prior[x];
  const int64_t q = total / 8;
  int rem = (int)(total % 8);
  int64_t want[8];
  bool extra[8] = {};
  for (int x = 0; x < 8; ++x)
    if (prior[x] > q && rem > 0) { extra[x] = true; --rem; }
  while (rem > 0) {
    int best = -1;
    for (int x = 0; x < 8; ++x)
      if (!extra[x] && (best < 0 || base[x] < base[best])) best = x;
    extra[best] = true; --rem;
  }
  int64_t given = 0;
  for (int x = 0; x < 8; ++x) {
    want[x] = q + (extra[x] ? 1 : 0) - prior[x];
    if (want[x] < 0) want[x] = 0;
  }
  for (int x = 0; x < 8; ++x) {
    int64_t w = want[x];
    if (x == 7 || w > (int64_t)tiles.size() - given) w = (int64_t)tiles.size() - given;  // (prior more than 1 apart: the rest)
    d->t[x].assign(tiles.begin() + given, tiles.begin() + given + w);
    given += w;
  }
}
}  // namespace ts_detail

// Lower update of tiles_m x tiles_n tiles (tiles_n <= tiles_m), one tile list in n_launch (1 or 2) launches.
//   col0_first  super column 0 (all rows) is enumerated first and lies in the first launch
//   base_last   other work (in tiles) the XCDs of the LAST launch already carry, by the XCD label b & 7 of the list's own
//               block index b (the second problem's blocks that lead the launch)
// Two launches are cut so that the first holds about half the tiles: the head and whole rounds only.
inline void tile_sched_build(int tiles_m, int tiles_n, bool col0_first, int n_launch, const double base_last[8], TileSched* S) {
  *S = TileSched();
  S->n_launch = n_launch;
  for (int x = 0; x < 8 && base_last; ++x) S->base_last[x] = base_last[x];
  const int sm = (tiles_m + 7) / 8, fm = tiles_m / 8;
  if (tiles_m < 1 || tiles_n < 1 || tiles_n > tiles_m || tiles_m > 0xffff || (n_launch != 1 && n_launch != 2)) return;
  if (fm >= 2 && (fm - 1) * 8 > tiles_n) return;  // a "full" super tile would be cut by the column bound
  const int nh = col0_first ? (fm > 1 ? fm - 1 : 0) : 0;
  const int64_t F = (int64_t)fm * (fm - 1) / 2, R = F / 8;
  // single tiles in the old order: super column 0 first (col0_first), then row by row
  std::vector<uint32_t> head, tail;
  int64_t f = 0, total = R * 512;
  auto visit = [&](int SI, int SJ) {
    const bool full = SI < fm && SJ < SI;
    if (full && f++ < R * 8) return;
    std::vector<uint32_t>& v = (col0_first && SJ == 0) ? head : tail;
    for (int r = 0; r < 8; ++r)
      for (int c = 0; c < 8; ++c) {
        const int ti = SI * 8 + r, tj = SJ * 8 + c;
        if (ti < tiles_m && tj < tiles_n && tj <= ti) { v.push_back((uint32_t)ti | ((uint32_t)tj << 16)); ++total; }
      }
  };
  if (col0_first) {
    // the full super tiles of column 0 lead the list of full ones, so the head must be visited in that order too
    for (int SI = 1; SI < fm; ++SI) visit(SI, 0);
    std::vector<uint32_t> rest;
    rest.swap(head);
    visit(0, 0);
    head.insert(head.end(), rest.begin(), rest.end());
    for (int SI = fm > 1 ? fm : 1; SI < sm; ++SI) visit(SI, 0);
    for (int SI = 1; SI < sm; ++SI)
      for (int SJ = 1; SJ <= SI; ++SJ) visit(SI, SJ);
  } else {
    for (int SI = 0; SI < sm; ++SI)
      for (int SJ = 0; SJ <= SI; ++SJ) visit(SI, SJ);
  }
  int64_t r_cut = R;
  if (n_launch == 2) {
    r_cut = (int64_t)floor(((double)total * 0.5 - (double)head.size()) / 512.0 + 0.5);
    const int64_t need = (((int64_t)nh < R * 8 ? (int64_t)nh : R * 8) + 7) / 8;  // rounds that hold column 0's full super tiles
    if (r_cut < need) r_cut = need;
    if (r_cut > R) r_cut = R;
  }
  const int64_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const double nobase[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  ts_detail::Deal dh, dt, dl;
  ts_detail::deal(head, zero, nobase, &dh);
  // The tail's tiles of the last tile row are dealt on their own and lead each XCD's tail: when the update's row count is
  // no multiple of the tile they take the guarded tile body, which is slower, and one contiguous run would hand all of
  // them to the last XCD, at the very end of the launch.
  std::vector<uint32_t> tail_last, tail_rest;
  for (uint32_t v : tail) ((int)(v & 0xffff) == tiles_m - 1 ? tail_last : tail_rest).push_back(v);
  int64_t prior[8];
  for (int x = 0; x < 8; ++x) prior[x] = (n_launch == 1) ? (int64_t)dh.t[x].size() : 0;
  ts_detail::deal(tail_last, prior, nobase, &dl);
  for (int x = 0; x < 8; ++x) prior[x] += (int64_t)dl.t[x].size();
  ts_detail::deal(tail_rest, prior, base_last ? base_last : nobase, &dt);
  for (int x = 0; x < 8; ++x) dt.t[x].insert(dt.t[x].begin(), dl.t[x].begin(), dl.t[x].end());
  const int last = n_launch - 1;
  for (int l = 0; l < n_launch; ++l) {
    TileLaunch& L = S->L[l];
    L.table = nullptr;
    L.r0 = (l == 0) ? 0 : (int)r_cut;
    L.r1 = (l == last) ? (int)R : (int)r_cut;
    L.nh = nh;
    L.col0_first = col0_first ? 1 : 0;
    int64_t per[8], mx = 0, cnt_max = 0;
    for (int x = 0; x < 8; ++x) {
      const int64_t h = (l == 0) ? (int64_t)dh.t[x].size() : 0, t = (l == last) ? (int64_t)dt.t[x].size() : 0;
      if (h > 0xffff || t > 0xffff) return;
      L.hn[x >> 2] |= (uint64_t)h << (16 * (x & 3));
      L.tn[x >> 2] |= (uint64_t)t << (16 * (x & 3));
      per[x] = h + t;
      if (per[x] > mx) mx = per[x];
      const int64_t c = per[x] + (int64_t)(L.r1 - L.r0) * 64;
      if (c > cnt_max) cnt_max = c;
    }
    L.stride = (int)mx;
    S->table[l].assign((size_t)(8 * mx), 0);
    for (int x = 0; x < 8; ++x) {
      size_t o = (size_t)x * (size_t)mx;
      if (l == 0) for (uint32_t v : dh.t[x]) S->table[l][o++] = v;
      if (l == last) for (uint32_t v : dt.t[x]) S->table[l][o++] = v;
    }
    S->blocks[l] = 8 * cnt_max;
    // tiles by kind
    auto count = [&](int64_t ti, int64_t tj) {
      const bool lastrow = ti == tiles_m - 1;
      ++S->tiles[l];
      if (ti == tj) ++(lastrow ? S->diag_last[l] : S->diag_int[l]);
      else ++(lastrow ? S->off_last[l] : S->off_int[l]);
    };
    for (int x = 0; x < 8; ++x) {
      if (l == 0) for (uint32_t v : dh.t[x]) count(v & 0xffff, v >> 16);
      if (l == last) for (uint32_t v : dt.t[x]) count(v & 0xffff, v >> 16);
    }
    for (int64_t ff = (int64_t)L.r0 * 8; ff < (int64_t)L.r1 * 8; ++ff) {
      int64_t SI, SJ;
      ts_full_super(ff, L.col0_first, L.nh, &SI, &SJ);
      for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 8; ++c) count(SI * 8 + r, SJ * 8 + c);
    }
  }
  S->ok = true;
}

// algorithmic flops of launch l: lower update of order M (last tile row: M - (tiles_m - 1) gt rows), depth K.  A launch
// that does not end the list counts the tiles it holds, the last one takes the rest of M (M + 1) K (the same count, plus
// the one-row diagonal tile that a carried right-hand-side row has no column for).
inline double tile_sched_counted_flops(const TileSched& S, int l, int64_t M, int64_t K, int tiles_m, int gt) {
  const double rl = (double)(M - (int64_t)(tiles_m - 1) * gt), g = (double)gt;
  return (double)K * (2.0 * g * g * (double)S.off_int[l] + 2.0 * rl * g * (double)S.off_last[l] +
                      g * (g + 1.0) * (double)S.diag_int[l] + rl * (rl + 1.0) * (double)S.diag_last[l]);
}
inline double tile_sched_flops(const TileSched& S, int l, int64_t M, int64_t K, int tiles_m, int gt) {
  if (l < S.n_launch - 1) return tile_sched_counted_flops(S, l, M, K, tiles_m, gt);
  double before = 0.0;
  for (int i = 0; i < l; ++i) before += tile_sched_counted_flops(S, i, M, K, tiles_m, gt);
  return (double)M * (double)(M + 1) * (double)K - before;
}

// ---- the factorisation's launch plan (host only) and the composed launches of the deep schedule (chol.deep) ------
// chol_plan_build states the schedule as a list of operations, each fused launch with its full description (PlanLowerLaunch
// one-level, PlanSegLaunch composed); chol_factor_device (chol.hip) runs that list and derives nothing of its own.  With
// chol.deep = 0 the list is the one-level schedule: panel pairs, fused single panels, tail.  With chol.deep = W
// the columns form blocks [0, NB + W), [NB + W, NB + 2 W), ...  Inside block b the K = 2 NB update of an outer step covers
// only the tile columns of block b (near band); the tiles right of it receive the whole block in ONE pass of depth W (far
// pass) that has no launch of its own: its tiles ride in the launches of block b + 1's outer steps, as further SEGMENTS
// of those launches (own A, B, C, M, N, K).  A launch is then a per-XCD table of (segment, ti, tj) entries; a full 8 x 8 super
// tile stays whole on one XCD, single tiles are dealt in contiguous runs so that the XCDs carry the same cost.  The last
// tile row, when it is ragged, takes the guarded tile body, which rounds C - (A B^T) instead of accumulating into -C: it
// stays in the near band of every step, so that the factor is bit for bit the one-level factor.
// The deep regime ends at the first outer step whose trailing matrix is shorter than chol.deep_min_rows (or whose successor
// is no panel pair any more): that step's two launches carry whatever is pending, then the one-level schedule goes on.
#define TS_SEG_TI(v) ((int64_t)((v) & 0x3fffu))
#define TS_SEG_TJ(v) ((int64_t)(((v) >> 14) & 0x3fffu))
#define TS_SEG_ID(v) ((int)(((v) >> 28) & 7u))
#define TS_SEG_COUNTED(v) ((v) >> 31)

struct CholPlanOpts {
  int64_t NB = 512, OB = 1024, outer_min_rows = 16384, fused_min_rows = 12288, deep = 0, deep_min_rows = 26624;
};
struct PlanSeg {      // C[origin:, origin:] -= A[origin:, a_col0 : a_col0 + K] (same rows of the matrix)^T, M x N
  int64_t origin = 0, a_col0 = 0, M = 0, N = 0, K = 0;
  int kind = 0;       // 0 near band, 1 far pass, 2 second problem (columns of panel b updated by panel a)
};
struct PlanSegLaunch {
  PlanSeg seg[3];
  std::vector<uint32_t> xcd[8];  // ti | tj << 14 | segment << 28 | counted << 31, tile indices relative to the segment's origin
  int64_t diag0 = 0;             // first row of the diagonal block workgroup 0 factors
  int diag_nbw = 0, counted = 0;
  int64_t tiles = 0, far_tiles = 0;
  double flops = 0.0, far_flops = 0.0, cost = 0.0;
};
// One-level fused launch (OP_PAIR1, OP_PAIR2, OP_FUSED): launch `launch` of the n_launch (1 or 2) that share the tile list of
// the lower update upd; workgroup 0 factors the diagonal block at diag0 meanwhile.  A lower update without a diagonal block
// (the public launch_gemm_nt_sub, lower) is the same description with only upd set.
struct PlanLowerLaunch {
  PlanSeg upd;                   // kind 0
  int col0_first = 0;            // super column 0 (the outer panel's own columns) leads the list and lies in launch 0
  int launch = 0, n_launch = 1;
  PlanSeg second;                // kind 2 (M = 0: none): led by the list's LAST launch, as workgroups in front of its tiles
  int carries_second = 0;        // this launch carries it (0: a later one will; the list is dealt around it all the same)
  int64_t diag0 = 0;             // first row of the diagonal block
  int diag_nbw = 0;              // its width / 64 (0: no block)
  int counted = 0;               // its tiles are in this launch (the leading tiles of upd, or of second where carried) and
                                 // count themselves: their number (0: the block is complete before the launch)
};
enum { OP_PANEL = 0, OP_RECT, OP_PAIR1, OP_PAIR2, OP_FUSED, OP_TRSM, OP_TAIL, OP_SEG };
struct CholOp {
  int kind = 0;
  int64_t k0 = 0, nb = 0;   // finished panel: columns [k0, k0 + nb)
  int64_t t0 = 0, nb2 = 0;  // next panel (OP_TRSM: the diagonal block and its width)
  int seg = -1;             // OP_SEG: index into CholPlan::segs
  int lower = -1;           // OP_PAIR1, OP_PAIR2, OP_FUSED: index into CholPlan::lowers
  int ready_target = 0;     // launches with counted tiles: what the tile counter, which is never reset, shows when they are all in
};
struct CholPlan {
  std::vector<CholOp> ops;
  std::vector<PlanSegLaunch> segs;
  std::vector<PlanLowerLaunch> lowers;
  int64_t NB = 0, OB = 0, deep = 0, deep_end = 0;  // deep_end: first column of the step that leaves the deep regime (0: never entered)
};

// ---- what a PlanLowerLaunch means for the launcher (chol.hip) and for tests/tile_balance_driver.cpp
inline PlanLowerLaunch plan_lower_plain(int64_t M, int64_t N, int64_t K) {
  PlanLowerLaunch L;
  L.upd.M = M; L.upd.N = N; L.upd.K = K;
  return L;
}
// workgroups of a second problem in front of a launch; *compact: each of them holds a tile (tile_decode_second)
inline int plan_second_blocks(int64_t M2, int64_t N2, bool* compact) {
  const int64_t tm2 = (M2 + 127) / 128, tn2 = (N2 + 127) / 128;
  *compact = tm2 >= tn2;
  return (int)(tm2 * tn2 - (*compact ? tn2 * (tn2 - 1) / 2 : 0));
}
// everything the balanced list depends on: tiles_m, tiles_n, col0_first, n_launch, and of a (compact) second problem its
// workgroups and the two depths
inline std::array<int64_t, 7> plan_lower_key(const PlanLowerLaunch& L) {
  bool compact = false;
  const int lead2 = (L.second.M > 0 && L.second.N > 0) ? plan_second_blocks(L.second.M, L.second.N, &compact) : 0;
  const bool has2 = compact && lead2 > 0;
  return {(L.upd.M + 127) / 128, (L.upd.N + 127) / 128, L.col0_first ? 1 : 0, L.n_launch, has2 ? lead2 : 0, has2 ? L.second.K : 0,
          has2 ? L.upd.K : 0};
}
// the balanced list (all its launches); !S->ok: the shape has none and keeps the super-tile enumeration
inline void plan_lower_sched(const PlanLowerLaunch& L, TileSched* S) {
  const std::array<int64_t, 7> k = plan_lower_key(L);
  // the second problem's block q sits lead2 - q blocks in front of the list's block 0: XCD label (q - lead2) mod 8
  const int lead2 = (int)k[4];
  double base[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int q = 0; q < lead2; ++q) base[((q - lead2) % 8 + 8) % 8] += (double)k[5] / (double)k[6];
  tile_sched_build((int)k[0], (int)k[1], k[2] != 0, (int)k[3], base, S);
}
// super-tile enumeration: the super tiles [*s_begin, *n_super) of this launch.  Two launches cut the list in the middle, but
// not inside super column 0.
inline void plan_lower_range(const PlanLowerLaunch& L, int64_t* s_begin, int64_t* n_super) {
  const int64_t sm = ((L.upd.M + 127) / 128 + 7) / 8, n_all = sm * (sm + 1) / 2;
  const int64_t s_split = n_all / 2 < sm ? sm : n_all / 2;
  *s_begin = (L.n_launch == 2 && L.launch == 1) ? s_split : 0;
  *n_super = (L.n_launch == 2 && L.launch == 0) ? s_split : n_all;
}

namespace cp_detail {
const int GT_ = 128;
const int64_t TURNOVER = 66;  // tile turnover in units of k: 0.885 of the peak at K = 1024 and 0.927 at K = 4096
// one tile (v = ti | tj << 14) or one full 8 x 8 super tile (v = its first tile): no storage of its own
struct Unit {
  uint32_t v = 0;
  int64_t K = 0;
  uint8_t seg = 0, kind = 0;
  bool full = false, ragged = false, first = false;
  int tiles() const { return full ? 64 : 1; }
  int64_t cost() const { return (int64_t)tiles() * (K + TURNOVER); }
  uint32_t tile(int i) const { return full ? v + (uint32_t)(i >> 3) + ((uint32_t)(i & 7) << 14) : v; }
};
// the lower tiles of an M x N problem that pred accepts, super row by super row; 64 accepted tiles of one super tile form
// one unit, everything else (and every super tile that reaches into a ragged last tile row) single tiles
// (only super columns [tj_lo / 8, ceil(tj_hi / 8)) are visited, and the last super row over all its columns when last_row is
// set: pred still decides, the range only spares the visit of super tiles it would reject anyway)
template <class Pred>
inline void gen_units(int seg, const PlanSeg& s, Pred pred, bool first, std::vector<Unit>* out, int tj_lo = 0, int tj_hi = 1 << 30,
                      bool last_row = false) {
  const int tiles_m = (int)((s.M + GT_ - 1) / GT_), tiles_n = (int)((s.N + GT_ - 1) / GT_);
  const bool ragged = (s.M % GT_) != 0 || (s.N % GT_) != 0;
  const int sm = (tiles_m + 7) / 8;
  Unit u;
  u.seg = (uint8_t)seg; u.kind = (uint8_t)s.kind; u.K = s.K; u.first = first;
  const int sj_lo = tj_lo / 8, sj_hi = tj_hi > (1 << 29) ? (1 << 29) : (tj_hi + 7) / 8;
  for (int SI = 0; SI < sm; ++SI)
    for (int SJ = 0; SJ <= SI; ++SJ) {
      if ((SJ < sj_lo || SJ >= sj_hi) && !(last_row && SI == sm - 1)) continue;
      uint32_t got[64];
      int ng = 0;
      for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 8; ++c) {
          const int ti = SI * 8 + r, tj = SJ * 8 + c;
          if (ti < tiles_m && tj < tiles_n && tj <= ti && pred(ti, tj)) got[ng++] = (uint32_t)ti | ((uint32_t)tj << 14);
        }
      if (ng == 64 && !(ragged && SI * 8 + 7 == tiles_m - 1)) {
        u.full = true; u.ragged = false; u.v = got[0];
        out->push_back(u);
        continue;
      }
      for (int i = 0; i < ng; ++i) {
        u.full = false; u.v = got[i];
        u.ragged = ragged && (int)TS_SEG_TI(got[i]) == tiles_m - 1;
        out->push_back(u);
      }
    }
}
inline int64_t units_cost(const std::vector<Unit>& v, size_t from = 0) {
  int64_t c = 0;
  for (size_t i = from; i < v.size(); ++i) c += v[i].cost();
  return c;
}
// Classes in the order of an XCD's list: 0 first-column tiles (the counted ones lead), 1 far pass, 2 ragged last row (guarded
// body, not at the very end), 3 near full super tiles, 4 the rest.  Long tiles ahead of short ones: the launch ends on
// short tiles (with the far tiles behind the near ones 12 of the 15 ms the schedule gains are lost, profiles/chol_deep.txt).
inline void deal_launch(const std::vector<Unit>& units, int counted_seg, int counted_rows, PlanSegLaunch* L) {
  std::vector<Unit> cls[5];
  for (const Unit& u : units) cls[u.first ? 0 : (u.kind == 1 ? 1 : (u.ragged ? 2 : (u.full ? 3 : 4)))].push_back(u);
  int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto put = [&](int x, const Unit& u) {
    const PlanSeg& s = L->seg[u.seg];
    for (int i = 0; i < u.tiles(); ++i) {
      const uint32_t v = u.tile(i);
      const int64_t ti = TS_SEG_TI(v), tj = TS_SEG_TJ(v);
      const bool cnt = u.seg == counted_seg && ti < counted_rows && tj < counted_rows;
      L->xcd[x].push_back(v | ((uint32_t)u.seg << 28) | (cnt ? 0x80000000u : 0u));
      const double r = (double)(s.M - ti * GT_ < GT_ ? s.M - ti * GT_ : GT_), c = (double)(s.N - tj * GT_ < GT_ ? s.N - tj * GT_ : GT_);
      const double fl = (double)s.K * ((ti == tj && s.kind != 2) ? r * (r + 1.0) : 2.0 * r * c);
      L->flops += fl; ++L->tiles;
      if (s.kind == 1) { L->far_flops += fl; ++L->far_tiles; }
    }
    load[x] += u.cost();
  };
  std::vector<Unit> fulls, singles;
  for (int c = 0; c < 5; ++c) {
    // full super tiles in rounds of eight, one per XCD (least loaded first); the < 8 that fill no round become single
    // tiles, and the single tiles are dealt in contiguous runs that even out what the XCDs carry so far
    fulls.clear(); singles.clear();
    size_t n_full = 0, nf = 0;
    for (const Unit& u : cls[c]) n_full += u.full ? 1 : 0;
    const size_t keep = n_full - n_full % 8;
    for (const Unit& u : cls[c]) {
      if (u.full && nf++ < keep) { fulls.push_back(u); continue; }
      Unit w = u;
      w.full = false;
      for (int i = 0; i < u.tiles(); ++i) { w.v = u.tile(i); singles.push_back(w); }
    }
    auto deal_full = [&]() {
      for (const Unit& u : fulls) {
        int best = 0;
        for (int x = 1; x < 8; ++x) if (load[x] < load[best]) best = x;
        put(best, u);
      }
    };
    if (c != 0) deal_full();
    int64_t tot = 0;
    for (const Unit& u : singles) tot += u.cost();
    for (int x = 0; x < 8; ++x) tot += load[x];
    const double mean = (double)tot / 8.0;
    size_t i = 0;
    for (int x = 0; x < 8; ++x) {
      double want = mean - (double)load[x];
      while (i < singles.size() && (x == 7 || want >= 0.5 * (double)singles[i].cost())) {
        want -= (double)singles[i].cost();
        put(x, singles[i++]);
      }
    }
    if (c == 0) deal_full();
  }
  int64_t mx = 0;
  for (int x = 0; x < 8; ++x) if (load[x] > mx) mx = load[x];
  L->cost = (double)mx;
}
}  // namespace cp_detail

// 32-bit words of a composed launch's device table: [8][stride], stride = the longest XCD list, padded to 64 words
inline size_t plan_launch_stride(const PlanSegLaunch& L) {
  size_t mx = 0;
  for (int x = 0; x < 8; ++x) mx = L.xcd[x].size() > mx ? L.xcd[x].size() : mx;
  return mx;
}
inline size_t plan_launch_words(const PlanSegLaunch& L) { return (8 * plan_launch_stride(L) + 63) & ~(size_t)63; }

inline void chol_plan_build(int64_t n, int64_t n_rows, CholPlanOpts o, CholPlan* P) {
  using namespace cp_detail;
  *P = CholPlan();
  if (n_rows < n) n_rows = n;
  // The options are clamped here and nowhere else.
  int64_t NB = o.NB;
  if (NB < 64 || NB % 64 || NB > 512) NB = 512;  // the diagonal-block role and the row-local solve hold at most 8 x 64 columns
  // a fused launch needs a trailing matrix to ride in: with 0 the last panel of a matrix with a carried right-hand-side row
  // (n - t1 = 0, n_rows - t1 = 1) asked for a fused launch with an empty update, which the launcher skips together with its
  // diagonal-block workgroup -- the block was never factored
  int64_t min_rows = o.fused_min_rows < 1 ? 1 : o.fused_min_rows;
  // pairs count finished 128 x 128 tiles of the diagonal block, so they need NB % 128 == 0: other NB run single panels
  int64_t OB = o.OB;
  if (OB != 2 * NB || NB % GT_ != 0) OB = NB;
  P->NB = NB; P->OB = OB;
  auto width_at = [&](int64_t c0) -> int64_t {
    const int64_t left = n - (c0 + OB);
    const int64_t w = (OB > NB && left > 0 && left >= o.outer_min_rows) ? OB : NB;
    return (n - c0 < w) ? n - c0 : w;
  };
  auto fuse_at = [&](int64_t t0) {
    const int64_t nb2 = width_at(t0), t1 = t0 + nb2;
    return (nb2 % 64 == 0) && (n - t1 >= min_rows) && (n_rows - t1 > 0);
  };
  auto paired = [&](int64_t t0) { return t0 < n && OB == 2 * NB && width_at(t0) == 2 * NB && fuse_at(t0); };
  // deep regime: outer steps t0 = NB, NB + OB, ... < X are composed, the step at X carries what is pending and leaves
  int64_t W = (OB == 2 * NB) ? o.deep : 0;
  if (W > 0) W -= W % OB;
  int64_t X = NB;
  if (W >= OB && n_rows / GT_ < 0x3ff0) {
    while (paired(X) && paired(X + OB) && n - X >= o.deep_min_rows) X += OB;
  }
  const bool has_deep = X > NB;
  P->deep = has_deep ? W : 0;
  P->deep_end = has_deep ? X : 0;
  const int OBt = (int)(OB / GT_), NBt = (int)(NB / GT_);
  const int block_tiles = NBt * (NBt + 1) / 2;
  auto op = [&](int kind, int64_t k0, int64_t nb, int64_t t0, int64_t nb2, int seg = -1) {
    CholOp c;
    c.kind = kind; c.k0 = k0; c.nb = nb; c.t0 = t0; c.nb2 = nb2; c.seg = seg;
    P->ops.push_back(c);
  };
  // ---- state of the deep regime
  int64_t S = 0, E = NB + W;        // current block
  PlanSeg pool_seg;                 // the pending pass
  std::vector<Unit> pool;           // its tiles not yet dealt, in order
  size_t pool_at = 0;
  int64_t span_cost = 0;
  int span_left = 0;
  auto near_seg = [&](int64_t t0, int64_t k0, int64_t nb) {
    PlanSeg s;
    s.origin = t0; s.a_col0 = k0; s.M = n_rows - t0; s.N = n - t0; s.K = nb; s.kind = 0;
    return s;
  };
  auto second_seg = [&](int64_t t0) {
    PlanSeg s;
    s.origin = t0 + NB; s.a_col0 = t0; s.M = n_rows - (t0 + NB); s.N = NB; s.K = NB; s.kind = 2;
    return s;
  };
  auto near_bound = [&](int64_t t0, int64_t blockS, int64_t blockE) -> int { return (t0 == blockS && blockS > 0) ? 0 : (int)((blockE - t0) / GT_); };
  auto near_pred = [&](const PlanSeg& s, int bound) {
    const int tiles_m = (int)((s.M + GT_ - 1) / GT_);
    const bool ragged = (s.M % GT_) != 0 || (s.N % GT_) != 0;
    return [=](int ti, int tj) { return tj < bound || (ragged && ti == tiles_m - 1); };
  };
  auto far_pred = [&](const PlanSeg& s) {
    const int tiles_m = (int)((s.M + GT_ - 1) / GT_);
    const bool ragged = (s.M % GT_) != 0 || (s.N % GT_) != 0;
    return [=](int ti, int tj) { return !(ragged && ti == tiles_m - 1); };
  };
  auto step_fixed_cost = [&](int64_t t0, int64_t nb, int64_t blockS, int64_t blockE) {
    std::vector<Unit> u;
    const PlanSeg s = near_seg(t0, t0 - nb, nb), s2 = second_seg(t0);
    const int bound = near_bound(t0, blockS, blockE);
    gen_units(0, s, near_pred(s, bound), false, &u, 0, bound, true);
    gen_units(2, s2, [](int, int) { return true; }, true, &u, 0, NBt);
    return units_cost(u);
  };

  int ready = 0;  // the tile counter so far
  auto counted_op = [&](int tiles) { P->ops.back().ready_target = (ready += tiles); };
  // one-level fused launches: the pair of an outer step (one tile list of everything right of the finished panel, first
  // columns first, cut in two; the second leads with the K = NB update of b's columns by panel a) and the single fused one
  auto lower_op = [&](int kind, int64_t k0, int64_t nb, int64_t t0, int64_t nb2) {
    PlanLowerLaunch L;
    const bool pair = kind != OP_FUSED;
    L.upd = near_seg(pair ? t0 : t0 + nb2, k0, nb);
    if (pair) { L.col0_first = 1; L.n_launch = 2; L.launch = L.carries_second = (kind == OP_PAIR2) ? 1 : 0; L.second = second_seg(t0); }
    L.diag0 = t0 + L.launch * NB; L.diag_nbw = (int)((pair ? NB : nb2) / 64);
    L.counted = pair ? block_tiles : 0;
    P->lowers.push_back(L);
    op(kind, k0, nb, t0, nb2);
    P->ops.back().lower = (int)P->lowers.size() - 1;
    if (L.counted) counted_op(L.counted);
  };

  int64_t k0 = 0, nb = (n < NB) ? n : NB;
  op(OP_PANEL, 0, 0, 0, nb);
  for (;;) {
    const int64_t t0 = k0 + nb;
    if (t0 >= n) break;
    const int64_t nb2 = width_at(t0), t1 = t0 + nb2;
    const bool fuse = fuse_at(t0);
    if (fuse && nb2 == 2 * NB && has_deep && t0 <= X) {
      const int64_t ta = t0 + NB;
      int must = 0;  // tile columns of the pending pass that the first launch must hold
      if (t0 == E) {  // block boundary: block [S, E) becomes the pending far pass, its tiles ride in the next block's steps
        pool_seg = PlanSeg();
        pool_seg.origin = E; pool_seg.a_col0 = S; pool_seg.M = n_rows - E; pool_seg.N = n - E; pool_seg.K = E - S; pool_seg.kind = 1;
        S = E; E = S + W;
        int m = 0;
        int64_t fixed = 0;
        for (int64_t t = t0; t < E && (t < X || t == t0); t += OB) { ++m; fixed += step_fixed_cost(t, t == t0 ? nb : OB, S, E); }
        must = (m > 1) ? (int)(W / GT_) : OBt;
        pool.clear(); pool_at = 0;
        const auto fp = far_pred(pool_seg);
        gen_units(1, pool_seg, [&](int ti, int tj) { return fp(ti, tj) && tj < OBt; }, true, &pool, 0, OBt);
        gen_units(1, pool_seg, [&](int ti, int tj) { return fp(ti, tj) && tj >= OBt && tj < must; }, false, &pool, OBt, must);
        gen_units(1, pool_seg, [&](int ti, int tj) { return fp(ti, tj) && tj >= must; }, false, &pool, must);
        span_cost = fixed + units_cost(pool);
        span_left = 2 * m;
      } else if (t0 == X) {  // leaving inside block [S, E): the block's finished panels [S, X) go to the tiles right of E now
        pool.clear(); pool_at = 0;
        pool_seg = PlanSeg();
        if (E < n) {
          pool_seg.origin = E; pool_seg.a_col0 = S; pool_seg.M = n_rows - E; pool_seg.N = n - E; pool_seg.K = X - S; pool_seg.kind = 1;
          gen_units(1, pool_seg, far_pred(pool_seg), false, &pool);
        }
        span_cost = step_fixed_cost(t0, nb, S, E) + units_cost(pool);
        span_left = 2;
      } else if (span_left == 0) {
        span_cost = step_fixed_cost(t0, nb, S, E);
        span_left = 2;
      }
      const PlanSeg ns = near_seg(t0, k0, nb);
      const int bound = near_bound(t0, S, E);
      const auto np_ = near_pred(ns, bound);
      std::vector<Unit> rest;  // near tiles right of the first columns: either launch of the step
      size_t rest_at = 0;
      for (int l = 0; l < 2; ++l) {
        PlanSegLaunch L;
        L.seg[0] = ns;
        L.seg[1] = pool_seg;
        if (l == 1) L.seg[2] = second_seg(t0);
        std::vector<Unit> u;
        if (l == 0) {
          gen_units(0, ns, [&](int ti, int tj) { return np_(ti, tj) && tj < OBt; }, true, &u, 0, OBt);
          while (pool_at < pool.size() && must > 0 && (int)TS_SEG_TJ(pool[pool_at].v) < must) u.push_back(pool[pool_at++]);
          rest.clear(); rest_at = 0;
          gen_units(0, ns, [&](int ti, int tj) { return np_(ti, tj) && tj >= OBt; }, false, &rest, OBt, bound, true);
        } else {
          gen_units(2, L.seg[2], [](int, int) { return true; }, true, &u, 0, NBt);
        }
        int64_t cost = units_cost(u);
        const int64_t target = span_cost / span_left;
        if (l == 0) {
          while (rest_at < rest.size() && cost + rest[rest_at].cost() / 2 <= target) { cost += rest[rest_at].cost(); u.push_back(rest[rest_at++]); }
        } else {
          while (rest_at < rest.size()) { cost += rest[rest_at].cost(); u.push_back(rest[rest_at++]); }
        }
        while (pool_at < pool.size() && (span_left == 1 || cost + pool[pool_at].cost() / 2 <= target)) {
          cost += pool[pool_at].cost();
          u.push_back(pool[pool_at++]);
        }
        span_cost -= cost;
        --span_left;
        L.diag0 = (l == 0) ? t0 : ta;
        L.diag_nbw = (int)(NB / 64);
        L.counted = block_tiles;
        const bool counted_in_pool = (l == 0) && bound == 0;  // at a block boundary the diagonal block's tiles are far tiles
        deal_launch(u, l == 1 ? 2 : (counted_in_pool ? 1 : 0), NBt, &L);
        P->segs.push_back(std::move(L));
        op(OP_SEG, k0, nb, t0, nb2, (int)P->segs.size() - 1);
        counted_op(block_tiles);
        op(OP_TRSM, 0, 0, l == 0 ? t0 : ta, NB);
      }
    } else if (fuse && nb2 == 2 * NB) {
      lower_op(OP_PAIR1, k0, nb, t0, nb2);
      op(OP_TRSM, 0, 0, t0, NB);
      lower_op(OP_PAIR2, k0, nb, t0, nb2);
      op(OP_TRSM, 0, 0, t0 + NB, NB);
    } else {
      op(OP_RECT, k0, nb, t0, nb2);
      if (fuse) {
        lower_op(OP_FUSED, k0, nb, t0, nb2);
        op(OP_TRSM, 0, 0, t0, nb2);
      } else if (t1 < n) {
        op(OP_TAIL, k0, nb, t0, nb2);
      } else {
        op(OP_PANEL, 0, 0, t0, nb2);
      }
    }
    k0 = t0;
    nb = nb2;
  }
}
