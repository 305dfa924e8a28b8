// Stand-alone printer of the batched predictor's plan (sgdml_amd/csrc/predict_plan.h).  Built and run by
// test_predict_plan_cpu.py (host compiler, -fsanitize=address,undefined).  Reads one input per line from standard input,
//   N MP B num_cus want_virial wave_only mfma mfma_wide fill
// and prints the input followed by every field of the plan, one line per input.
#include "../sgdml_amd/csrc/predict_plan.h"

#include <cstdio>

int main() {
  static const char* const names[] = {"WAVE", "BIG", "BULK", "MFMA", "WIDE"};
  long long N, MP, B, ncu, virial, wave_only, mfma, wide, fill;
  while (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld", &N, &MP, &B, &ncu, &virial, &wave_only, &mfma, &wide, &fill) == 9) {
    PredPlanIn in;
    in.N = (int)N;
    in.D = (int)(N * (N - 1) / 2);
    in.MP = MP;
    in.B = B;
    in.num_cus = (int)ncu;
    in.want_virial = virial != 0;
    in.wave_only = (int)wave_only;
    in.mfma = (int)mfma;
    in.mfma_wide = (int)wide;
    in.fill = (int)fill;
    const PredPlan p = predict_plan(in);
    std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld : route %s sel %d QB %d grid_x %u grid_y %u block %u JS %d rps %lld lds %zu ws %lld stats %lld "
                "epi_lds_row %d epi_virial %d epi_JS %d epi_lds %zu\n",
                N, MP, B, ncu, virial, wave_only, mfma, wide, fill, names[p.route], p.sel, p.QB, p.grid_x, p.grid_y, p.block, p.JS,
                (long long)p.rows_per_split, p.lds_bytes, (long long)p.ws_bytes, (long long)p.stats_bytes, (int)p.epi_lds_row,
                (int)p.epi_virial, p.epi_JS, p.epi_lds_bytes);
  }
  return 0;
}
