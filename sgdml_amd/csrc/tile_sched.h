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
