// Stand-alone harness for csrc/frame_qp.h (a QP per picture: the rule, the dQP-file reader, the grouping, the lambda family with a modifier, the refusals), built by
// tests/test_frame_qp.py with -fsanitize=address,undefined.  Every table is an exact-size heap block, so an entry read or written outside it is caught.
//   frame_qp_harness qps CASES.txt       lines "n base_qp intra_qp_offset bit_depth qpif frame_skip ratio" (qpif -1: absent) -> lines of n QPs
//   frame_qp_harness file N DQPFILE      the offsets of N POCs, all 7 before the file is read -> "status" and a line of N offsets
//   frame_qp_harness group CASES.txt     lines "n qp0 .. qp(n-1)" -> "runs contiguous", the permutation, its inverse, then per run "qp first count"
//   frame_qp_harness family CASES.txt    lines "qp bit_depth modifier-bits" -> "qp qp_chroma lambda sqrt_lambda chroma_weight lambda_chroma err_scale x 8 sbh x 2" (doubles as 64-bit patterns)
//   frame_qp_harness keys CASES.txt      lines "bit_depth delta_qp_rd deblocking_metric modifier-bits n qp0 .." -> lines "status|sentence"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "frame_qp.h"

static uint64_t bits_of(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static double double_of(uint64_t u) { double v; memcpy(&v, &u, 8); return v; }

int main(int argc, char **argv)
{
  if (argc < 3) { printf("usage: frame_qp_harness qps|group|family|keys CASES.txt | file N DQPFILE\n"); return 2; }
  const std::string mode = argv[1];
  if (mode == "file") {
    if (argc != 4) return 2;
    const int n = atoi(argv[2]);
    std::vector<int> dqp((size_t)n, 7);
    const int st = hevcdl_dqp_read_file(argv[3], dqp.data(), n);
    printf("%d\n", st);
    for (int i = 0; i < n; i++) printf("%s%d", i ? " " : "", dqp[(size_t)i]);
    printf("\n");
    return 0;
  }
  FILE *f = fopen(argv[2], "r");
  if (!f) { printf("cannot read %s\n", argv[2]); return 2; }
  int done = 0;
  if (mode == "qps") {
    int n, base, off, bd, qpif, skip, ratio;
    while (fscanf(f, "%d %d %d %d %d %d %d", &n, &base, &off, &bd, &qpif, &skip, &ratio) == 7) {
      std::vector<int> dqp((size_t)n);
      hevcdl_dqp_increment(dqp.data(), n, qpif >= 0, (unsigned)(qpif >= 0 ? qpif : 0), (unsigned)skip, (unsigned)ratio);
      for (int i = 0; i < n; i++) printf("%s%d", i ? " " : "", hevcdl_frame_qp_of(base, dqp[(size_t)i], off, bd));
      printf("\n");
      done++;
    }
  } else if (mode == "group") {
    int n;
    while (fscanf(f, "%d", &n) == 1) {
      std::vector<int> qp((size_t)n), perm((size_t)n), inv((size_t)n);
      for (int i = 0; i < n; i++) if (fscanf(f, "%d", &qp[(size_t)i]) != 1) { printf("short case\n"); return 2; }
      std::vector<hevcdl_qp_run> runs((size_t)(n < 52 ? n : 52)), cruns((size_t)(n < 52 ? n : 52));
      const int n_runs = hevcdl_frame_qp_group(qp.data(), n, perm.data(), runs.data(), nullptr);
      const int cont = n_runs < 0 ? -1 : hevcdl_frame_qp_contiguous_runs(qp.data(), n, cruns.data());
      printf("%d %d\n", n_runs, n == 0 ? 1 : (cont > 0));
      if (n_runs >= 0) {
        hevcdl_frame_qp_inverse(perm.data(), n, inv.data());
        for (int i = 0; i < n; i++) printf("%s%d", i ? " " : "", perm[(size_t)i]);
        printf("\n");
        for (int i = 0; i < n; i++) printf("%s%d", i ? " " : "", inv[(size_t)i]);
        printf("\n");
        for (int r = 0; r < n_runs; r++) printf("%d %d %d\n", runs[(size_t)r].qp, runs[(size_t)r].first, runs[(size_t)r].count);
        for (int r = 0; r < cont; r++) { // the no-copy runs cover the list in picture order
          const hevcdl_qp_run &c = cruns[(size_t)r];
          for (int i = c.first; i < c.first + c.count; i++) if (qp[(size_t)i] != c.qp) { printf("contiguous run mismatch\n"); return 3; }
        }
      }
      done++;
    }
  } else if (mode == "family") {
    int qp, bd; uint64_t mb;
    while (fscanf(f, "%d %d %" SCNu64, &qp, &bd, &mb) == 3) {
      hevcdl_qp_rd_candidate c;
      hevcdl_frame_qp_family(qp, bd, double_of(mb), &c);
      printf("%d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, c.qp, c.qp_chroma, bits_of(c.lambda), bits_of(c.sqrt_lambda), bits_of(c.chroma_weight), bits_of(c.lambda_chroma));
      for (int ch = 0; ch < 2; ch++) for (int l = 0; l < 4; l++) printf(" %" PRIu64, bits_of(c.err_scale[ch][l]));
      printf(" %" PRId64 " %" PRId64 "\n", c.sbh_rd_factor[0], c.sbh_rd_factor[1]);
      done++;
    }
  } else if (mode == "keys") {
    hevcdl_config c; memset(&c, 0, sizeof c);
    uint64_t mb; int n;
    while (fscanf(f, "%d %d %d %" SCNu64 " %d", &c.bit_depth, &c.delta_qp_rd, &c.deblocking_metric, &mb, &n) == 5) {
      std::vector<int> qp((size_t)n);
      for (int i = 0; i < n; i++) if (fscanf(f, "%d", &qp[(size_t)i]) != 1) { printf("short case\n"); return 2; }
      const char *why = "";
      const int st = (int)hevcdl_frame_qp_keys(&c, n ? qp.data() : nullptr, n, double_of(mb), &why);
      printf("%d|%s\n", st, why);
      done++;
    }
  } else { printf("unknown mode %s\n", mode.c_str()); return 2; }
  fclose(f);
  return done ? 0 : 2;
}
