// slices_harness.cpp -- the host side of slices as a program (tests/test_slices.py builds it with the host compiler under the sanitizers, together with
// csrc/hevcdl_bitstream.cpp).  One request a line on stdin, one answer a line.
//   plan  <n_cus> <waves narrow wide tools bd10> <width height max_frames slice_mode slice_argument tile_rows h0 .. h20> <n_frames>
//         csrc/slice_grid.h + csrc/rd_launch_plan.h: the launch of n_frames whole frames on the context of that configuration (tile_rows > 1: one tile column with the
//         explicit row heights h*)  ->  <workspace blocks>\t<what hevcdl_last_rd_launch reports>, or "status <n>\t<reason>" when the slice keys are refused
//   write <width height qp slice_mode slice_argument lf_across_slices tile_columns tile_rows n_frames seed>
//         the writer on synthetic records: every picture through hevcdl_write_access_unit_slices into an allocation of exactly its length, and through
//         hevcdl_code_slice_data_host_slices + hevcdl_write_access_unit_from_slice_data_slices; the two must agree, the canaries between the regions must stand and
//         hevcdl_access_unit_bound_slices must hold  ->  "ok <slice NAL units of the last picture> <bytes>"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "hevcdl.h"
#include "entropy_coder.h"
#include "rd_launch_plan.h"
#include "slice_grid.h"

static int plan()
{
  int n_cus, waves[RD_BUILDS], w, h, max_frames, mode, arg, rows, n_frames;
  hevcdl_config cfg; memset(&cfg, 0, sizeof cfg);
  if (scanf("%d %d %d %d %d %d %d %d %d %d %d", &n_cus, &waves[0], &waves[1], &waves[2], &waves[3], &w, &h, &max_frames, &mode, &arg, &rows) != 11) return 2;
  for (int i = 0; i < 21; i++) if (scanf("%d", &cfg.tile_row_height[i]) != 1) return 2;
  if (scanf("%d", &n_frames) != 1) return 2;
  cfg.struct_size = sizeof cfg; cfg.width = w; cfg.height = h; cfg.bit_depth = 8; cfg.tools = HEVCDL_TOOLS_REFERENCE; cfg.max_frames = max_frames;
  cfg.tile_columns = 1; cfg.tile_rows = rows; cfg.tile_uniform_spacing = rows > 1 ? 0 : 1; cfg.lf_across_tiles = 1; cfg.lf_across_slices = 1;
  cfg.slice_mode = mode; cfg.slice_argument = arg;
  hevcdl_config grid; const char *why = "";
  const hevcdl_status st = hevcdl_slice_grid(&cfg, &grid, &why);
  if (st != HEVCDL_OK) { printf("status %d\t%s\n", (int)st, why); return 0; }
  const RdPlanContext pc = rd_plan_context_of(grid, n_cus, waves);
  RdLaunchArgs a; a.n_frames = n_frames;
  const RdLaunchPlan p = rd_launch_plan(pc, a);
  if (p.status) { printf("status %d\tplan\n", (int)p.status); return 0; }
  char report[160];
  rd_launch_report(p, report, sizeof report);
  printf("%zu\t%s\t%d x %d rows", p.scratch_blocks(), report, grid.tile_columns, grid.tile_rows);
  for (int i = 0; i < grid.tile_rows - 1; i++) printf(" %d", grid.tile_row_height[i]);
  printf("\n");
  return 0;
}

// records of a plausible shape -- 64x64 .. 8x8 CUs, any luma mode, a few levels in a CU's first luma block; the coder reads any record safely, so their validity as a
// picture is not what this program checks (the fixtures of tests/test_slices.py are the reference's own records)
static void synth_records(std::vector<hevcdl_ctu_record> &recs, int ctus_x, int ctus_y, int w, int h, uint32_t seed)
{
  uint32_t s = seed * 2654435761u + 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  for (size_t a = 0; a < recs.size(); a++) {
    hevcdl_ctu_record &r = recs[a]; memset(&r, 0, sizeof r);
    const int cx = (int)(a % (size_t)(ctus_x * ctus_y)) % ctus_x, cy = (int)(a % (size_t)(ctus_x * ctus_y)) / ctus_x;
    const bool inside = (cx + 1) * 64 <= w && (cy + 1) * 64 <= h;
    const int depth = inside ? (int)(rnd() % 4) : 3;       // a CTU that crosses the picture's edge: 8x8 CUs, inside it at any picture size that is a multiple of 8
    for (int z = 0; z < 256; z++) { r.depth[z] = (uint8_t)depth; r.part_size[z] = 0; r.chroma_dir[z] = 36; }
    const int nparts = 256 >> (2 * depth);
    for (int z0 = 0; z0 < 256; z0 += nparts) {
      const int dir = (int)(rnd() % 35), trd = depth == 0 ? 1 : 0;      // a 64x64 CU holds four 32x32 transform blocks
      const bool coded = rnd() % 3 != 0;
      for (int z = z0; z < z0 + nparts; z++) { r.luma_dir[z] = (uint8_t)dir; r.tr_idx[z] = (uint8_t)trd; }
      if (coded) { // levels in the first transform block of the CU: its cbf at the block's depth, and at depth 0 of a 64x64 CU for the whole quadrant
        const int tparts = depth == 0 ? 64 : nparts;
        for (int z = z0; z < z0 + tparts; z++) r.cbf[0][z] = (uint8_t)((1 << trd) | (trd ? 1 : 0));
        r.coeff_y[16 * z0] = (int16_t)(1 + rnd() % 40); r.coeff_y[16 * z0 + 1] = (int16_t)-(int)(rnd() % 3);
      }
    }
  }
}

static int count_slice_nals(const std::vector<uint8_t> &au)
{
  int n = 0;
  for (size_t i = 0; i + 3 < au.size(); i++) if (au[i] == 0 && au[i + 1] == 0 && au[i + 2] == 1) { const int type = (au[i + 3] >> 1) & 63; if (type <= 21) n++; }
  return n;
}

static int write()
{
  int w, h, qp, mode, arg, lf, tc, tr, n_frames; unsigned seed;
  if (scanf("%d %d %d %d %d %d %d %d %d %u", &w, &h, &qp, &mode, &arg, &lf, &tc, &tr, &n_frames, &seed) != 10) return 2;
  hevcdl_stream_config cfg;
  if (hevcdl_stream_config_default(&cfg, w, h, qp) != HEVCDL_OK) { printf("bad size\n"); return 0; }
  cfg.tile_columns = tc; cfg.tile_rows = tr;
  const hevcdl_slice_layout layout = { mode, arg, lf };
  const int ctus_x = (w + 63) >> 6, ctus_y = (h + 63) >> 6; const size_t ctus = (size_t)ctus_x * ctus_y;
  std::vector<hevcdl_ctu_record> recs(ctus * n_frames);
  synth_records(recs, ctus_x, ctus_y, w, h, seed);
  int n_sub = 0; size_t pic_bytes = 0;
  const hevcdl_status ls = hevcdl_slice_data_layout_slices(&cfg, &layout, 0, &n_sub, &pic_bytes, nullptr, nullptr);
  if (ls != HEVCDL_OK) { printf("status %d\n", (int)ls); return 0; }
  std::vector<uint32_t> off(n_sub), cap(n_sub), sizes((size_t)n_sub * n_frames), ovf((size_t)n_sub * n_frames);
  hevcdl_slice_data_layout_slices(&cfg, &layout, 0, &n_sub, &pic_bytes, off.data(), cap.data());
  std::vector<uint8_t> out(pic_bytes * n_frames, 0xA5);
  if (hevcdl_code_slice_data_host_slices(&cfg, &layout, recs.data(), nullptr, n_frames, 0, out.data(), out.size(), sizes.data(), ovf.data()) != HEVCDL_OK) { printf("coder status\n"); return 1; }
  int nals = 0; size_t total = 0;
  for (int fr = 0; fr < n_frames; fr++) {
    std::vector<uint8_t> packed;
    for (int k = 0; k < n_sub; k++) {
      const uint8_t *p = out.data() + pic_bytes * fr + off[k], *gap = p + cap[k];
      for (int i = 0; i < hevcdl_ec::EC_REGION_GAP; i++) if (gap[i] != 0xA5) { printf("canary of sub-stream %d.%d\n", fr, k); return 1; }
      if (ovf[(size_t)fr * n_sub + k]) { printf("sub-stream %d.%d overflowed\n", fr, k); return 1; }
      packed.insert(packed.end(), p, p + sizes[(size_t)fr * n_sub + k]);
    }
    packed.push_back(0);
    size_t na = 0, nb = 0, nc = 0; uint8_t none = 0;
    if (hevcdl_write_access_unit_slices(&cfg, &layout, fr, recs.data() + ctus * fr, nullptr, nullptr, &none, 0, &na) != HEVCDL_ERR_INVALID_ARG || na == 0) { printf("picture %d: no length from a call without room\n", fr); return 1; }
    if (na > hevcdl_access_unit_bound_slices(w, h, &layout)) { printf("picture %d: %zu bytes exceed the bound\n", fr, na); return 1; }
    std::vector<uint8_t> a(na), b(na);      // exactly the access unit's length: a store past it is a sanitizer report
    if (hevcdl_write_access_unit_slices(&cfg, &layout, fr, recs.data() + ctus * fr, nullptr, nullptr, a.data(), a.size(), &nb) != HEVCDL_OK || nb != na) { printf("picture %d: writer status\n", fr); return 1; }
    if (hevcdl_write_access_unit_from_slice_data_slices(&cfg, &layout, fr, packed.data(), sizes.data() + (size_t)fr * n_sub, n_sub, nullptr, b.data(), b.size(), &nc) != HEVCDL_OK || nc != na) { printf("picture %d: assembly status\n", fr); return 1; }
    if (memcmp(a.data(), b.data(), na) != 0) { printf("picture %d: the two ways to an access unit differ\n", fr); return 1; }
    nals = count_slice_nals(a); total += na;
  }
  printf("ok %d %zu\n", nals, total);
  return 0;
}

int main()
{
  char verb[16];
  while (scanf("%15s", verb) == 1) {
    const int rc = !strcmp(verb, "plan") ? plan() : (!strcmp(verb, "write") ? write() : 2);
    if (rc == 2) { printf("slices harness: bad request\n"); return 2; }
    if (rc) return rc;
  }
  return 0;
}
