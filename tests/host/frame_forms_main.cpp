// A stand-alone driver of the scanMatching driver's form decision (tloam_amd/csrc/tl_forms.hpp: decide_forms), meant to be compiled
// for the host alone with -fsanitize=address,undefined and run on a machine without a GPU (tests/test_frame_forms_host.py does).
// No HIP in here, and no other header of the project.
// Reads one FormsIn per line from stdin -- 34 integers in the order of the struct's fields -- and prints one line of forms for each:
//   set prepare solve finish finish_rides loop qbin_ride
#include <stdio.h>

#include "../../tloam_amd/csrc/tl_forms.hpp"

int main() {
  static const char* const kSet[] = {"COMPACT", "DIRECT"};
  static const char* const kPrepare[] = {"NONE", "IN_SOLVE", "SMALL", "TILES", "FULL"};
  static const char* const kSolve[] = {"PERSISTENT", "FUSED_LARGE", "SHARDED_MBOX", "SHARDED_COLLECTIVE", "SMALL_STEP", "SWEEP_REDUCE"};
  static const char* const kFinish[] = {"DIRECT", "SMALL", "LARGE", "SHARDED"};
  static const char* const kRides[] = {"NO", "ON_SEARCH_SMALL", "ON_SEARCH_LARGE", "IN_SOLVE"};
  static const char* const kLoop[] = {"DEVICE", "HOST"};
  for (;;) {
    tl::FormsIn in;
    int got = scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &in.nranks, &in.loopback, &in.mailbox, &in.device_cus, &in.no_persistent_solve,
                    &in.no_direct_set, &in.no_device_loop, &in.no_build_reuse, &in.fused_large, &in.no_qbin_ride, &in.factor_num,
                    &in.max_iterations);
    if (got == EOF) return 0;
    if (got != 12) return 2;
    for (int k = 0; k < 4; ++k) got += scanf("%lld", &in.maxnum[k]);
    for (int k = 0; k < 4; ++k) got += scanf("%lld", &in.n_src[k]);
    for (int k = 0; k < 4; ++k) got += scanf("%lld", &in.n_tgt[k]);
    for (int k = 0; k < 4; ++k) got += scanf("%d", &in.has_grid[k]);
    got += scanf("%d %d", &in.k3_grid, &in.k3_single);
    for (int k = 0; k < 4; ++k) got += scanf("%lld", &in.seg_cap[k]);
    if (got != 34) return 2;
    const tl::FrameForms f = tl::decide_forms(in);
    printf("%s %s %s %s %s %s %d\n", kSet[(int)f.set], kPrepare[(int)f.prepare], kSolve[(int)f.solve], kFinish[(int)f.finish],
           kRides[(int)f.finish_rides], kLoop[(int)f.loop], f.qbin_ride ? 1 : 0);
  }
}
