// segments_harness.cpp -- the host side of dependent slice segments as a program (tests/test_segments.py builds it with the host compiler under the sanitizers, together
// with csrc/hevcdl_bitstream.cpp).  One request a line on stdin, one answer a line.  A <layout> is
//   <width height qp wavefront tile_columns tile_rows slice_mode slice_argument segment_mode segment_argument>
//   plan    <n_cus> <waves narrow wide tools bd10> <max_frames> <layout> <n_frames>
//           csrc/slice_grid.h + csrc/rd_launch_plan.h: the launch of n_frames whole frames on the context of that configuration  ->
//           <workspace blocks>\t<what hevcdl_last_rd_launch reports>\t<segment keys left in the grid>, or "status <n>\t<reason>" when the keys are refused
//   records <file of hevcdl_ctu_record> <file to write> <layout> <n_frames>
//           the pictures of the file (a fixture's records; no SAO) through hevcdl_write_access_unit_segments into an allocation of exactly the access unit's length, and
//           through hevcdl_code_slice_data_host_segments + hevcdl_write_access_unit_from_slice_data_segments; the two must agree, the canaries between the regions must
//           stand and hevcdl_access_unit_bound_segments must hold; the access units go to the second file  ->  "ok <slice NAL units of the last picture> <bytes>"
//   synth   <layout> <n_frames> <seed> <garbage>
//           the same on synthetic records -- garbage 0: records of a plausible shape; 1: random bytes (the coder must read any record safely; the bound is then not
//           asked for: it is a bound for pictures)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "hevcdl.h"
#include "entropy_coder.h"
#include "rd_launch_plan.h"
#include "slice_grid.h"

struct Layout { int w, h, qp, wpp, tc, tr; hevcdl_slice_layout slices; hevcdl_segment_layout segments; };
static bool read_layout(Layout &l)
{
  l.slices.lf_across_slices = 1;
  return scanf("%d %d %d %d %d %d %d %d %d %d", &l.w, &l.h, &l.qp, &l.wpp, &l.tc, &l.tr, &l.slices.mode, &l.slices.argument, &l.segments.mode, &l.segments.argument) == 10;
}

static int plan()
{
  int n_cus, waves[RD_BUILDS], max_frames, n_frames; Layout l;
  if (scanf("%d %d %d %d %d %d", &n_cus, &waves[0], &waves[1], &waves[2], &waves[3], &max_frames) != 6 || !read_layout(l) || scanf("%d", &n_frames) != 1) return 2;
  hevcdl_config cfg; memset(&cfg, 0, sizeof cfg);
  cfg.struct_size = sizeof cfg; cfg.width = l.w; cfg.height = l.h; cfg.qp = l.qp; cfg.bit_depth = 8; cfg.tools = HEVCDL_TOOLS_REFERENCE; cfg.max_frames = max_frames;
  cfg.tile_columns = l.tc; cfg.tile_rows = l.tr; cfg.tile_uniform_spacing = 1; cfg.lf_across_tiles = 1; cfg.lf_across_slices = 1; cfg.wavefront = l.wpp; cfg.lf_offset_in_pps = 1;
  cfg.slice_mode = l.slices.mode; cfg.slice_argument = l.slices.argument; cfg.slice_segment_mode = l.segments.mode; cfg.slice_segment_argument = l.segments.argument;
  hevcdl_config grid; const char *why = "";
  const hevcdl_status st = hevcdl_slice_grid(&cfg, &grid, &why);
  if (st != HEVCDL_OK) { printf("status %d\t%s\n", (int)st, why); return 0; }
  const RdPlanContext pc = rd_plan_context_of(grid, n_cus, waves);
  RdLaunchArgs a; a.n_frames = n_frames;
  const RdLaunchPlan p = rd_launch_plan(pc, a);
  if (p.status) { printf("status %d\tplan\n", (int)p.status); return 0; }
  char report[160];
  rd_launch_report(p, report, sizeof report);
  printf("%zu\t%s\t%d %d\n", p.scratch_blocks(), report, grid.slice_segment_mode, grid.slice_segment_argument);
  return 0;
}

// records of a plausible shape -- 64x64 .. 8x8 CUs, any luma mode, a few levels in a CU's first luma block
static void synth_records(std::vector<hevcdl_ctu_record> &recs, int ctus_x, int ctus_y, int w, int h, uint32_t seed, int garbage)
{
  uint32_t s = seed * 2654435761u + 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  if (garbage) { uint8_t *b = (uint8_t *)recs.data(); for (size_t i = 0; i < recs.size() * sizeof(hevcdl_ctu_record); i++) b[i] = (uint8_t)rnd(); return; }
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
      if (coded) {
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

// every picture of recs both ways; the access units are appended to *all when it is there
static int write_pictures(const Layout &l, const std::vector<hevcdl_ctu_record> &recs, int n_frames, bool check_bound, std::vector<uint8_t> *all)
{
  hevcdl_stream_config cfg;
  if (hevcdl_stream_config_default(&cfg, l.w, l.h, l.qp) != HEVCDL_OK) { printf("bad size\n"); return 0; }
  cfg.tile_columns = l.tc; cfg.tile_rows = l.tr; cfg.wavefront = l.wpp;
  const hevcdl_slice_layout *sl = l.slices.mode ? &l.slices : nullptr;
  const hevcdl_segment_layout *sg = &l.segments;
  const size_t ctus = (size_t)((l.w + 63) >> 6) * ((l.h + 63) >> 6);
  int n_sub = 0; size_t pic_bytes = 0;
  const hevcdl_status ls = hevcdl_slice_data_layout_segments(&cfg, sl, sg, 0, &n_sub, &pic_bytes, nullptr, nullptr);
  if (ls != HEVCDL_OK) { printf("status %d\n", (int)ls); return 0; }
  std::vector<uint32_t> off(n_sub), cap(n_sub), sizes((size_t)n_sub * n_frames), ovf((size_t)n_sub * n_frames);
  hevcdl_slice_data_layout_segments(&cfg, sl, sg, 0, &n_sub, &pic_bytes, off.data(), cap.data());
  std::vector<uint8_t> out(pic_bytes * n_frames, 0xA5);
  if (hevcdl_code_slice_data_host_segments(&cfg, sl, sg, recs.data(), nullptr, n_frames, 0, out.data(), out.size(), sizes.data(), ovf.data()) != HEVCDL_OK) { printf("coder status\n"); return 1; }
  int nals = 0; size_t total = 0;
  for (int fr = 0; fr < n_frames; fr++) {
    std::vector<uint8_t> packed; bool fits = true;
    for (int k = 0; k < n_sub; k++) {
      const uint8_t *p = out.data() + pic_bytes * fr + off[k], *gap = p + cap[k];
      for (int i = 0; i < hevcdl_ec::EC_REGION_GAP; i++) if (gap[i] != 0xA5) { printf("canary of sub-stream %d.%d\n", fr, k); return 1; }
      if (ovf[(size_t)fr * n_sub + k]) { // (random bytes may code to more than a region holds: the writer, which codes with all the room it needs, is then run alone)
        if (check_bound) { printf("sub-stream %d.%d overflowed\n", fr, k); return 1; }
        fits = false; continue;
      }
      packed.insert(packed.end(), p, p + sizes[(size_t)fr * n_sub + k]);
    }
    packed.push_back(0);
    size_t na = 0, nb = 0, nc = 0; uint8_t none = 0;
    if (hevcdl_write_access_unit_segments(&cfg, sl, sg, fr, recs.data() + ctus * fr, nullptr, nullptr, &none, 0, &na) != HEVCDL_ERR_INVALID_ARG || na == 0) { printf("picture %d: no length from a call without room\n", fr); return 1; }
    if (check_bound && na > hevcdl_access_unit_bound_segments(l.w, l.h, sl, sg)) { printf("picture %d: %zu bytes exceed the bound\n", fr, na); return 1; }
    std::vector<uint8_t> a(na), b(na);      // exactly the access unit's length: a store past it is a sanitizer report
    if (hevcdl_write_access_unit_segments(&cfg, sl, sg, fr, recs.data() + ctus * fr, nullptr, nullptr, a.data(), a.size(), &nb) != HEVCDL_OK || nb != na) { printf("picture %d: writer status\n", fr); return 1; }
    if (fits && hevcdl_write_access_unit_from_slice_data_segments(&cfg, sl, sg, fr, packed.data(), sizes.data() + (size_t)fr * n_sub, n_sub, nullptr, b.data(), b.size(), &nc) != HEVCDL_OK || nc != na) { printf("picture %d: assembly status\n", fr); return 1; }
    if (fits && memcmp(a.data(), b.data(), na) != 0) { printf("picture %d: the two ways to an access unit differ\n", fr); return 1; }
    if (all) all->insert(all->end(), a.begin(), a.end());
    nals = count_slice_nals(a); total += na;
  }
  printf("ok %d %zu\n", nals, total);
  return 0;
}

static int records()
{
  char in[512], outp[512]; Layout l; int n_frames;
  if (scanf("%511s %511s", in, outp) != 2 || !read_layout(l) || scanf("%d", &n_frames) != 1 || n_frames < 1 || l.w <= 0 || l.h <= 0) return 2;
  const size_t ctus = (size_t)((l.w + 63) >> 6) * ((l.h + 63) >> 6);
  std::vector<hevcdl_ctu_record> recs(ctus * n_frames);
  FILE *f = fopen(in, "rb");
  if (!f || fread(recs.data(), sizeof(hevcdl_ctu_record), recs.size(), f) != recs.size()) { printf("cannot read %s\n", in); if (f) fclose(f); return 1; }
  fclose(f);
  std::vector<uint8_t> all;
  const int rc = write_pictures(l, recs, n_frames, true, &all);
  if (rc) return rc;
  f = fopen(outp, "wb");
  if (!f || fwrite(all.data(), 1, all.size(), f) != all.size()) { if (f) fclose(f); return 1; }
  fclose(f);
  return 0;
}

static int synth()
{
  Layout l; int n_frames, garbage; unsigned seed;
  if (!read_layout(l) || scanf("%d %u %d", &n_frames, &seed, &garbage) != 3 || n_frames < 1 || l.w <= 0 || l.h <= 0) return 2;
  const int ctus_x = (l.w + 63) >> 6, ctus_y = (l.h + 63) >> 6;
  std::vector<hevcdl_ctu_record> recs((size_t)ctus_x * ctus_y * n_frames);
  synth_records(recs, ctus_x, ctus_y, l.w, l.h, seed, garbage);
  return write_pictures(l, recs, n_frames, !garbage, nullptr);
}

int main()
{
  char verb[16];
  while (scanf("%15s", verb) == 1) {
    const int rc = !strcmp(verb, "plan") ? plan() : (!strcmp(verb, "records") ? records() : (!strcmp(verb, "synth") ? synth() : 2));
    if (rc == 2) { printf("segments harness: bad request\n"); return 2; }
    if (rc) return rc;
  }
  return 0;
}
