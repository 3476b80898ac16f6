// ntt_choose_host.cpp -- starks_amd/csrc/knobs.hpp's choice of the NTT pass kernel (shk_ntt_choose_cell) and its table of existing
// instantiations (shk_ntt_cell_exists) on the host, for tests/test_ntt_passes_host.py.  Plain g++, no HIP.
//   ntt_choose_host exists          one line "form tile_log log_R" per existing cell
//   ntt_choose_host radices         one line "log_n r1 r2 ..." per log_n 0 .. 32: shk_choose_radices under the environment
//   ntt_choose_host choose < Q      one answer "form tile_log xcd" per query line
//        "K tile_log tile_forced tile_log_big f0 f1 f2 f3 xcd_swz narrow_tiles  log_R last total log_n log_S pass_index"  (knobs given)
//        "E log_R last total log_n log_S pass_index"                                  (knobs parsed from the environment)
#include <stdio.h>
#include <string.h>

#include "knobs.hpp"

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "exists")) {
    for (int form = 0; form <= 1; ++form)
      for (int tl = 0; tl <= 16; ++tl)
        for (int r = 0; r <= 16; ++r)
          if (shk_ntt_cell_exists(form, tl, r)) printf("%d %d %d\n", form, tl, r);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "radices")) {
    for (int lg = 0; lg <= 32; ++lg) {
      int r[4] = {0, 0, 0, 0};
      const int m = shk_choose_radices(lg, r);
      printf("%d", lg);
      for (int i = 0; i < m; ++i) printf(" %d", r[i]);
      printf("\n");
    }
    return 0;
  }
  if (argc != 2 || strcmp(argv[1], "choose")) return 2;
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    ShkKnobs kn;
    int log_R, last;
    unsigned long long total;
    unsigned log_n, log_S, pi;
    if (line[0] == 'K') {
      int forced;
      if (sscanf(line + 1, "%d %d %d %d %d %d %d %d %ld %d %d %llu %u %u %u", &kn.tile_log, &forced, &kn.tile_log_big, &kn.tile_logs[0],
                 &kn.tile_logs[1], &kn.tile_logs[2], &kn.tile_logs[3], &kn.xcd_swz, &kn.narrow_tiles, &log_R, &last, &total, &log_n,
                 &log_S, &pi) != 15)
        return 2;
      kn.tile_forced = forced != 0;
    } else if (line[0] == 'E') {
      if (sscanf(line + 1, "%d %d %llu %u %u %u", &log_R, &last, &total, &log_n, &log_S, &pi) != 6) return 2;
      kn = shk_knobs();
    } else {
      return 2;
    }
    const ShkNttCell c = shk_ntt_choose_cell(kn, log_R, last != 0, ShkNttPassShape{total, log_n, log_S, pi});
    printf("%d %d %d\n", c.form, c.tile_log, (int)c.xcd);
  }
  return 0;
}
