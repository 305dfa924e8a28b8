// The host-only part of the chunk loop of the entries whose replicas freeze on their own (traj.h: traj_run_until_frozen):
// which evaluations make up a chunk, and what a frozen replica repeats behind its freeze.  No HIP header is included, so
// tests/traj_frozen_driver.cpp compiles this with the host compiler alone.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>

// One chunk: evaluations [t0, t1), evaluation t at history row t - t0.  With `record` the evaluations with
// t % record_every == 0 are frames; the chunk holds `frames` of them, in order from slot 0.
struct TrajChunk {
  int64_t t0, t1, frames;
  int64_t record_every;  // 0: nothing is recorded
  int64_t row(int64_t t) const { return t - t0; }
  int64_t frame(int64_t t) const {  // the chunk slot of evaluation t's frame, or -1
    if (record_every == 0 || t % record_every != 0) return -1;
    return t / record_every - (t0 + record_every - 1) / record_every;
  }
};

// The chunk that starts at evaluation t of 0 .. max_steps: at most chunk_steps evaluations and, where frames are recorded, at
// most max_frames (>= 1) of them.
static inline TrajChunk traj_next_chunk(int64_t t, int64_t max_steps, int64_t chunk_steps, bool record, int64_t record_every,
                                        int64_t max_frames) {
  TrajChunk c = {t, t, 0, record ? record_every : 0};
  for (; c.t1 <= max_steps && c.t1 - t < chunk_steps; ++c.t1) {
    const bool on = record && c.t1 % record_every == 0;
    if (on && c.frames == max_frames) break;
    c.frames += on;
  }
  return c;
}

// A chunk as read back, h_out = status (B,2) | bad (B) | history 0 .. n_hist - 1, (chunk_steps,B) words each: the rows of chunk c
// go on into hist[h] ((max_steps + 1, B); null: not wanted).  Returns whether the run goes on: a status word still says
// active (-1) and no bad flag is set.
static inline bool traj_take_chunk(const TrajChunk& c, const int64_t* h_out, int64_t B, int64_t chunk_steps, void* const* hist,
                                   int n_hist) {
  for (int h = 0; h < n_hist; ++h)
    if (hist[h]) memcpy((char*)hist[h] + c.t0 * B * 8, h_out + 3 * B + h * chunk_steps * B, (size_t)((c.t1 - c.t0) * B) * 8);
  bool active = false, any_bad = false;
  for (int64_t b = 0; b < B; ++b) {
    active |= h_out[(size_t)(2 * b)] < 0;
    any_bad |= h_out[(size_t)(2 * B + b)] >= 0;
  }
  return active && !any_bad;
}

// A frame field of such a run: the caller's (frames, B, len) array (null: not wanted) and the end state (B, len) that a
// frozen replica repeats in it.
struct TrajFrames {
  double* rec;
  const double* end;
  int64_t len;  // 8-byte words per replica
};

// After such a run: a frozen replica repeats its last value in each of the n_hist histories (arrays (max_steps + 1, B) of
// 8-byte words, doubles or int64; null: not wanted) and its end state in each frame field, up to the last evaluation any
// replica made (the launches behind its freeze wrote nothing for it).  h_flags: status (B,2) as read back; t: evaluations
// queued.  Returns the number of evaluations made.
static inline int64_t traj_repeat_frozen(const int64_t* h_flags, int64_t B, int64_t t, int64_t record_every, void* const* hist,
                                         int n_hist, const TrajFrames* fr, int n_fr) {
  int64_t n_made = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t e = h_flags[(size_t)(2 * b + 1)];
    n_made = std::max(n_made, e < 0 ? t : e + 1);
  }
  for (int64_t b = 0; b < B; ++b) {
    const int64_t e = h_flags[(size_t)(2 * b + 1)];
    if (e < 0) continue;
    for (int64_t u = e + 1; u < n_made; ++u) {
      for (int h = 0; h < n_hist; ++h)
        if (hist[h]) memcpy((char*)hist[h] + (u * B + b) * 8, (const char*)hist[h] + (e * B + b) * 8, 8);
      if (record_every > 0 && u % record_every == 0)
        for (int f = 0; f < n_fr; ++f)
          if (fr[f].rec)
            memcpy(fr[f].rec + ((u / record_every) * B + b) * fr[f].len, fr[f].end + b * fr[f].len, (size_t)fr[f].len * 8);
    }
  }
  return n_made;
}
