// Stand-alone harness for csrc/qp_rd.h (the host side of DeltaQpRD: candidate offsets, clipped QPs, the lambda family, the candidate table, the pick rule of
// TEncSlice.cpp:646-652, the refusals), built by tests/test_deltaqprd.py with -fsanitize=address,undefined.
//   deltaqprd_harness table CASES.txt     lines "qp n bit_depth" -> per case "count frame_lambda-bits", then per candidate one line
//                                         "offset qp qp_chroma lambda sqrt_lambda chroma_weight lambda_chroma err_scale x 8 sbh x 2" (doubles as 64-bit patterns);
//                                         a refused case prints "-1 0".  The table is an exact-size heap block, so an entry written outside it is caught.
//   deltaqprd_harness pick CASES.txt      lines "n frame_lambda-bits" + n pairs "bits dist" -> lines "index" (exact-size heap blocks again)
//   deltaqprd_harness keys CASES.txt      lines "qp bit_depth delta_qp_rd slice_mode slice_segment_mode deblocking_metric" -> lines "status|sentence"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "qp_rd.h"

static uint64_t bits_of(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

int main(int argc, char **argv)
{
  if (argc != 3) { printf("usage: deltaqprd_harness table|pick|keys CASES.txt\n"); return 2; }
  const std::string mode = argv[1];
  FILE *f = fopen(argv[2], "r");
  if (!f) { printf("cannot read %s\n", argv[2]); return 2; }
  int done = 0;
  if (mode == "table") {
    int qp, n, bd;
    while (fscanf(f, "%d %d %d", &qp, &n, &bd) == 3) {
      std::vector<hevcdl_qp_rd_candidate> cand((size_t)(n >= 0 && n <= HEVCDL_QP_RD_MAX_N ? 2 * n + 1 : 1));
      double fl = 0;
      const int count = hevcdl_qp_rd_table(qp, n, bd, cand.data(), &fl);
      printf("%d %" PRIu64 "\n", count, count < 0 ? (uint64_t)0 : bits_of(fl));
      for (int i = 0; i < count; i++) {
        const hevcdl_qp_rd_candidate &c = cand[(size_t)i];
        printf("%d %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, c.offset, c.qp, c.qp_chroma, bits_of(c.lambda), bits_of(c.sqrt_lambda), bits_of(c.chroma_weight), bits_of(c.lambda_chroma));
        for (int ch = 0; ch < 2; ch++) for (int l = 0; l < 4; l++) printf(" %" PRIu64, bits_of(c.err_scale[ch][l]));
        printf(" %" PRId64 " %" PRId64 "\n", c.sbh_rd_factor[0], c.sbh_rd_factor[1]);
        if (c.offset != hevcdl_qp_rd_offset(i) || c.qp != hevcdl_qp_rd_clip_qp(qp + c.offset, bd)) { printf("offset / clip mismatch\n"); return 3; }
      }
      done++;
    }
  } else if (mode == "pick") {
    int n; uint64_t lam_bits;
    while (fscanf(f, "%d %" SCNu64, &n, &lam_bits) == 2) {
      std::vector<uint64_t> bits((size_t)n), dist((size_t)n);
      for (int i = 0; i < n; i++) if (fscanf(f, "%" SCNu64 " %" SCNu64, &bits[(size_t)i], &dist[(size_t)i]) != 2) { printf("short case\n"); return 2; }
      double lam; memcpy(&lam, &lam_bits, 8);
      printf("%d\n", hevcdl_qp_rd_pick(bits.data(), dist.data(), n, lam));
      done++;
    }
  } else if (mode == "keys") {
    hevcdl_config c; memset(&c, 0, sizeof c);
    while (fscanf(f, "%d %d %d %d %d %d", &c.qp, &c.bit_depth, &c.delta_qp_rd, &c.slice_mode, &c.slice_segment_mode, &c.deblocking_metric) == 6) {
      const char *why = "";
      const int st = (int)hevcdl_qp_rd_keys(&c, &why);
      printf("%d|%s\n", st, why);
      done++;
    }
  } else { printf("unknown mode %s\n", mode.c_str()); return 2; }
  fclose(f);
  return done ? 0 : 2;
}
