// A stand-alone driver of the search grids' plan (tloam_amd/csrc/tl_grid_plan.hpp: plan_grids, grid_reservation), meant to be
// compiled for the host alone with -fsanitize=address,undefined and run on a machine without a GPU (tests/test_grid_plan_host.py
// does).  No HIP in here, and no other header of the project.
// Reads one case per line from stdin -- device_cus, single pass allowed, sparse_ok, then per kind: n, radius, lo[3], hi[3] (doubles
// in C99 hexadecimal), then the capacities of cell_start, cell_cnt and cell_cnt32 -- and prints one line for each:
//   scan tiles elem_bytes tgt_total cell_total n_tab | per kind: n tgt_off cell inv_cell org[3] dim[3] ncell cell_base start_base
//   | per buffer, in GridReservation's order: elements zeroed
#include <stdio.h>

#include "../../tloam_amd/csrc/tl_grid_plan.hpp"

int main() {
  static const char* const kScan[] = {"NONE", "SMALL", "TILES", "SINGLE_PASS", "GENERIC"};
  for (;;) {
    tl::GridPlanIn in;
    int allowed = 0, sparse = 0;
    int got = scanf("%d %d %d", &in.device_cus, &allowed, &sparse);
    if (got == EOF) return 0;
    if (got != 3) return 2;
    in.single_pass_allowed = allowed != 0;
    in.sparse_ok = sparse != 0;
    for (int k = 0; k < tl::kGridKinds; ++k) {
      got += scanf("%lld %la", &in.n[k], &in.radius[k]);
      for (int a = 0; a < 3; ++a) got += scanf("%la", &in.lo[k][a]);
      for (int a = 0; a < 3; ++a) got += scanf("%la", &in.hi[k][a]);
    }
    tl::GridCaps cap;
    got += scanf("%zu %zu %zu", &cap.cell_start, &cap.cell_cnt, &cap.cell_cnt32);
    if (got != 3 + 8 * tl::kGridKinds + 3) return 2;
    const tl::GridPlan p = tl::plan_grids(in);
    printf("%s %d %d %lld %lld %lld", kScan[(int)p.scan], p.tiles, p.elem_bytes, p.tgt_total, p.cell_total, p.n_tab);
    for (int k = 0; k < tl::kGridKinds; ++k) {
      const tl::GridPlan::Kind& g = p.k[k];
      printf(" | %d %d %a %a %a %a %a %d %d %d %lld %lld %lld", g.n, g.tgt_off, g.cell, g.inv_cell, g.org[0], g.org[1], g.org[2], g.dim[0],
             g.dim[1], g.dim[2], g.ncell, g.cell_base, g.start_base);
    }
    const tl::GridReservation r = tl::grid_reservation(p, cap);
    const tl::GridWant* const w[] = {&r.gp,       &r.cell_of_pt, &r.rank_of_pt, &r.cell_start, &r.cell_cnt32, &r.cell_scan32,
                                     &r.totals32, &r.cell_cnt,   &r.scan1p,     &r.cell_scan,  &r.scan_tmp};
    printf(" |");
    for (const tl::GridWant* x : w) printf(" %zu %d", x->n, x->zeroed ? 1 : 0);
    printf("\n");
  }
}
