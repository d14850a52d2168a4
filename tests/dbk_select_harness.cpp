// Stand-alone harness for csrc/dbk_select.h (the host side of DeblockingFilterMetric 1: thresholds, the edges that count, the metric-to-offset lines of
// TEncGOP.cpp:3270-3283), built by tests/test_dbk_select.py with -fsanitize=address,undefined.
//   dbk_select_harness CASES.txt          lines "width height bit_depth qp col_sum row_sum" -> lines "thr1 thr2 edges_x edges_y offset"
//   dbk_select_harness walk CASES.txt     lines "pps_beta pps_tc available disabled beta tc" + 49 table entries -> lines "override disabled beta tc | the new state"
//                                         (the walk of DeblockingFilterMetric 2; the table is an exact-size heap block, so an entry read outside it is caught)
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>
#include "dbk_select.h"

int main(int argc, char **argv)
{
  if (argc == 3 && std::string(argv[1]) == "walk") {
    FILE *g = fopen(argv[2], "r");
    if (!g) { printf("cannot read %s\n", argv[2]); return 2; }
    int pb, pt, m = 0; hevcdl_dbk_walk_state st;
    while (fscanf(g, "%d %d %d %d %d %d", &pb, &pt, &st.available, &st.disabled, &st.beta_offset_div2, &st.tc_offset_div2) == 6) {
      std::vector<uint64_t> table(49);
      for (uint64_t &v : table) if (fscanf(g, "%" SCNu64, &v) != 1) { printf("short table\n"); return 2; }
      const hevcdl_dbk_walk_result r = hevcdl_dbk_walk(table.data(), pb, pt, &st);
      printf("%d %d %d %d %d %d %d %d\n", r.override_flag, r.disabled, r.beta_offset_div2, r.tc_offset_div2, st.available, st.disabled, st.beta_offset_div2, st.tc_offset_div2);
      m++;
    }
    fclose(g);
    return m ? 0 : 2;
  }
  if (argc != 2) { printf("usage: dbk_select_harness [walk] CASES.txt\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
  int w, h, bd, qp; uint64_t cs, rs; int n = 0;
  while (fscanf(f, "%d %d %d %d %" SCNu64 " %" SCNu64, &w, &h, &bd, &qp, &cs, &rs) == 6) {
    int t1, t2;
    hevcdl_dbk_metric_thresholds(qp, bd, &t1, &t2);
    printf("%d %d %d %d %d\n", t1, t2, hevcdl_dbk_metric_edges(w), hevcdl_dbk_metric_edges(h), hevcdl_dbk_metric_offset(w, h, bd, cs, rs));
    n++;
  }
  fclose(f);
  return n ? 0 : 2;
}
