// Stand-alone run of the host-only part of the run-until-frozen chunk loop (sgdml_amd/csrc/traj_host.h) against a simulated
// device.  Built and run by test_traj_frozen_cpu.py (host compiler, -fsanitize=address,undefined).  Reads one case per line,
//   B max_steps chunk_steps record_every max_frames n_hist e_0 .. e_{B-1}
// (record_every 0: nothing recorded; e_b: the evaluation at which replica b converges, -1: never), runs the loop of
// traj_run_until_frozen with the kernels replaced by plain stores into a chunk buffer of the device's layout, and prints
//   CASE, one CHUNK t0 t1 frames line per chunk followed by an EV t row frame line per evaluation, END t n_made,
//   H h u v_0 .. v_{B-1} for every history h and row u < n_made, F f j w_0 .. for every frame field f and frame j of n_made.
// Values are integers (doubles hold them exactly): history h of replica b at evaluation t is ((h + 1) 1000 + t) 10 + b, word k
// of its frame 500000 + (10 t + b) 10 + k; history 3 is int64 as gdml_ef_run's k_follow_hist.  What no store reached is -1.
#include "../sgdml_amd/csrc/traj_host.h"

#include <cstdio>
#include <vector>

static const int64_t FRAME_LEN[2] = {3, 2};

static void put(void* base, int64_t i, int h, int64_t v) {  // word i of history h
  const double d = (double)v;
  memcpy((char*)base + i * 8, h == 3 ? (const void*)&v : (const void*)&d, 8);
}
static long long get(const void* base, int64_t i, int h) {
  int64_t v;
  double d;
  memcpy(&v, (const char*)base + i * 8, 8);
  memcpy(&d, (const char*)base + i * 8, 8);
  return h == 3 ? (long long)v : (long long)d;
}

int main() {
  long long B, max_steps, chunk_steps, record_every, max_frames, n_hist;
  while (std::scanf("%lld %lld %lld %lld %lld %lld", &B, &max_steps, &chunk_steps, &record_every, &max_frames, &n_hist) == 6) {
    std::vector<long long> e((size_t)B);
    for (auto& x : e)
      if (std::scanf("%lld", &x) != 1) return 2;
    const bool record = record_every > 0;
    const int64_t n_eval = max_steps + 1, n_rec = record ? max_steps / record_every + 1 : 0;
    // the caller's arrays
    std::vector<std::vector<int64_t>> hist_mem((size_t)n_hist, std::vector<int64_t>((size_t)(n_eval * B)));
    void* hist[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int h = 0; h < n_hist; ++h) {
      hist[h] = hist_mem[(size_t)h].data();
      for (int64_t i = 0; i < n_eval * B; ++i) put(hist[h], i, h, -1);
    }
    std::vector<double> rec[2], end[2];
    TrajFrames fr[2];
    for (int f = 0; f < 2; ++f) {
      rec[f].assign((size_t)(n_rec * B * FRAME_LEN[f]), -1.0);
      end[f].assign((size_t)(B * FRAME_LEN[f]), -1.0);
      fr[f] = TrajFrames{record ? rec[f].data() : nullptr, end[f].data(), FRAME_LEN[f]};
    }
    // the device: status (B,2) | bad (B) | histories (chunk_steps,B), never cleared between chunks
    std::vector<int64_t> dev((size_t)(3 * B + n_hist * chunk_steps * B), -1);
    for (int h = 0; h < n_hist; ++h)
      for (int64_t i = 0; i < chunk_steps * B; ++i) put(dev.data() + 3 * B + h * chunk_steps * B, i, h, -1);

    std::printf("CASE\n");
    int64_t t = 0, frames_done = 0;
    for (bool go = true; go && t <= max_steps;) {
      const TrajChunk c = traj_next_chunk(t, max_steps, chunk_steps, record, record_every, max_frames);
      std::printf("CHUNK %lld %lld %lld\n", (long long)c.t0, (long long)c.t1, (long long)c.frames);
      for (int64_t te = c.t0; te < c.t1; ++te) {
        const int64_t row = c.row(te), frame = c.frame(te);
        std::printf("EV %lld %lld %lld\n", (long long)te, (long long)row, (long long)frame);
        for (int64_t b = 0; b < B; ++b) {
          if (dev[(size_t)(2 * b)] >= 0) continue;  // frozen by an earlier evaluation: never written again
          for (int h = 0; h < n_hist; ++h)
            put(dev.data() + 3 * B + h * chunk_steps * B, row * B + b, h, ((h + 1) * 1000 + te) * 10 + b);
          for (int f = 0; f < 2; ++f)
            for (int64_t k = 0; k < FRAME_LEN[f]; ++k) {
              const double w = (double)(500000 + (10 * te + b) * 10 + k);
              end[f][(size_t)(b * FRAME_LEN[f] + k)] = w;
              if (frame >= 0) rec[f][(size_t)(((frames_done + frame) * B + b) * FRAME_LEN[f] + k)] = w;  // (the recorder's flush)
            }
          if (te == e[(size_t)b] || te == max_steps) {
            dev[(size_t)(2 * b)] = te == e[(size_t)b] ? 1 : 0;
            dev[(size_t)(2 * b + 1)] = te;
          }
        }
      }
      t = c.t1;
      frames_done += c.frames;
      go = traj_take_chunk(c, dev.data(), B, chunk_steps, hist, (int)n_hist);
    }
    const int64_t n_made = traj_repeat_frozen(dev.data(), B, t, record_every, hist, (int)n_hist, fr, 2);
    std::printf("END %lld %lld\n", (long long)t, (long long)n_made);
    for (int h = 0; h < n_hist; ++h)
      for (int64_t u = 0; u < n_made; ++u) {
        std::printf("H %d %lld", h, (long long)u);
        for (int64_t b = 0; b < B; ++b) std::printf(" %lld", get(hist[h], u * B + b, h));
        std::printf("\n");
      }
    const int64_t n_fr = record ? (n_made + record_every - 1) / record_every : 0;
    for (int f = 0; f < 2; ++f)
      for (int64_t j = 0; j < n_fr; ++j) {
        std::printf("F %d %lld", f, (long long)j);
        for (int64_t i = 0; i < B * FRAME_LEN[f]; ++i) std::printf(" %lld", (long long)rec[f][(size_t)(j * B * FRAME_LEN[f] + i)]);
        std::printf("\n");
      }
  }
  return 0;
}
