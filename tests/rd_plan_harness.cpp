// rd_plan_harness.cpp -- csrc/rd_launch_plan.h as a program (tests/test_rd_plan.py builds it with the host compiler under the sanitizers): reads one request a line from
// stdin and answers one line each.
//   launch  <context> <n_frames ctu_begin ctu_end cabac_in cabac_out tile_begin tile_count session_frame>  ->  <workspace blocks>\t<what hevcdl_last_rd_launch reports>
//   reserve <context>                                                                                      ->  <workspace blocks hevcdl_reserve_workspace asks for>
// <context>: n_cus max_frames bit_depth tools exec_flags wavefront tile_columns tile_rows ctus_x ctus_y waves[narrow wide tools bd10]
#include <stdio.h>
#include <string.h>
#include "rd_launch_plan.h"

static bool read_context(RdPlanContext &c)
{
  return scanf("%d %d %d %u %d %d %d %d %d %d %d %d %d %d", &c.n_cus, &c.max_frames, &c.bit_depth, &c.tools, &c.exec_flags, &c.wavefront, &c.tile_columns, &c.tile_rows,
               &c.ctus_x, &c.ctus_y, &c.waves[RD_NARROW], &c.waves[RD_WIDE], &c.waves[RD_TOOLS], &c.waves[RD_BD10]) == 14;
}

int main()
{
  char verb[16];
  while (scanf("%15s", verb) == 1) {
    RdPlanContext c;
    if (!read_context(c)) { printf("rd plan harness: bad context\n"); return 2; }
    if (!strcmp(verb, "reserve")) { printf("%zu\n", rd_largest_scratch_blocks(c)); continue; }
    RdLaunchArgs a; int cabac_in = 0, cabac_out = 0;
    if (strcmp(verb, "launch") || scanf("%d %d %d %d %d %d %d %d", &a.n_frames, &a.ctu_begin, &a.ctu_end, &cabac_in, &cabac_out, &a.tile_begin, &a.tile_count, &a.session_frame) != 8) {
      printf("rd plan harness: bad request\n"); return 2;
    }
    a.cabac_in = cabac_in != 0; a.cabac_out = cabac_out != 0;
    const RdLaunchPlan p = rd_launch_plan(c, a);
    if (p.status) { printf("0\tstatus %d\n", (int)p.status); continue; }
    char report[160];
    rd_launch_report(p, report, sizeof report);
    printf("%zu\t%s\n", p.scratch_blocks(), report);
  }
  return 0;
}
