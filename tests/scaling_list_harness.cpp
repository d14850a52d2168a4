// tests/scaling_list_harness.cpp -- TEST INFRASTRUCTURE.  The scaling-list forms of the stream parser (csrc/hevcdl_parse.cpp: hevcdl_parse_stream_sl), of the shared slice-data
// decoder's entry (hevcdl_parse_stream_core_sl) and of the reconstruction (csrc/recon_core.h, instantiated here with RcPicSl on one "lane") as a stand-alone program.
// tests/test_scaling_lists.py builds it with the host compiler and -fsanitize=address,undefined and runs it over the sclist_* fixtures, the flip corpus and synthetic
// extremes; tools/scaling_list_mutants.py builds it from sources with one line changed and expects it to fail.
// Every buffer is an exact-size heap block: a byte read behind a stream, or a record, map entry or factor touched outside its array, is a sanitizer report.
// Dump: int64 stream bytes, int64 picture bytes (0: none; otherwise the reference decoder's pictures of a filters-off stream), int64 mode (0: must parse, and reconstruct to
// the pictures; 1: as 0, then every single-bit flip and every truncation must give the same status from parser and core, a flip that parses a factor block without zeros and
// a reconstruction that runs); the stream; the pictures.  The argument "extremes" runs the synthetic records instead of a dump.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#include "recon_core.h"

using namespace hevcdl_rc;

static const unsigned ACCEPT = HEVCDL_ACCEPT_CU_QP | HEVCDL_ACCEPT_SCALING_LISTS;

struct Parsed {
  hevcdl_status st; hevcdl_stream_config cfg; hevcdl_slice_layout sl; hevcdl_segment_layout sg; hevcdl_qp_info qi; int n; size_t ctus;
  std::unique_ptr<hevcdl_scaling_info> si;
  std::unique_ptr<hevcdl_ctu_record[]> recs; std::unique_ptr<hevcdl_sao_blk[]> sao; std::unique_ptr<int8_t[]> map;
};
typedef hevcdl_status (*ParseFn)(const uint8_t *, size_t, unsigned, hevcdl_stream_config *, hevcdl_slice_layout *, hevcdl_segment_layout *, hevcdl_parsed_picture *, int, int *,
                                 hevcdl_ctu_record *, hevcdl_sao_blk *, size_t, hevcdl_qp_info *, int8_t *, hevcdl_scaling_info *);

static void parse(ParseFn fn, const uint8_t *s, size_t n, Parsed &p)
{
  memset(&p.cfg, 0, sizeof p.cfg); p.cfg.struct_size = sizeof p.cfg; p.n = 0; p.ctus = 0;
  p.si.reset(new hevcdl_scaling_info);
  p.st = hevcdl_parse_stream_sl(s, n, ACCEPT, &p.cfg, &p.sl, &p.sg, nullptr, 0, &p.n, nullptr, nullptr, 0, &p.qi, nullptr, p.si.get());
  if (p.st != HEVCDL_OK) return;
  p.ctus = (size_t)(((p.cfg.width + 63) >> 6) * ((p.cfg.height + 63) >> 6));
  const size_t all = p.ctus * (size_t)p.n;
  p.recs.reset(new hevcdl_ctu_record[all]); p.sao.reset(new hevcdl_sao_blk[all]); p.map.reset(new int8_t[all * 256]);
  std::vector<hevcdl_parsed_picture> pics((size_t)p.n);
  p.st = fn(s, n, ACCEPT, &p.cfg, &p.sl, &p.sg, pics.data(), p.n, &p.n, p.recs.get(), p.sao.get(), all, &p.qi, p.map.get(), p.si.get());
}

// the filters-off pictures of records, map and factors: what hevcdl_reconstruct_frames_sl_host does, from recon_core.h.  The factors go into a block of their exact size
static bool reconstruct(const hevcdl_stream_config &c, const hevcdl_slice_layout &sl, const hevcdl_qp_info &qi, const hevcdl_scaling_info &si, const hevcdl_ctu_record *recs,
                        const int8_t *map, int n, size_t ctus, std::vector<unsigned char> &out)
{
  RcPicSl pic; memset(&pic, 0, sizeof pic);
  pic.W = c.width; pic.H = c.height; pic.ctus_x = (c.width + 63) >> 6; pic.ctus_y = (c.height + 63) >> 6; pic.bit_depth = c.bit_depth; pic.qp = c.qp;
  pic.strong = (c.tools & HEVCDL_TOOL_STRONG_INTRA) != 0; pic.cb_off = qi.cb_qp_offset; pic.cr_off = qi.cr_qp_offset;
  std::unique_ptr<uint8_t[]> factor(new uint8_t[HEVCDL_SCALING_FACTOR_BYTES]);
  memcpy(factor.get(), si.factor, HEVCDL_SCALING_FACTOR_BYTES);
  pic.factor = factor.get();
  int col_bd[21], row_bd[23];
  if (hevcdl_tile_bounds(pic.ctus_x, c.tile_columns, c.tile_uniform_spacing != 0, c.tile_column_width, 1, col_bd) ||
      hevcdl_tile_bounds(pic.ctus_y, c.tile_rows, c.tile_uniform_spacing != 0, c.tile_row_height, 1, row_bd)) return false;
  std::vector<uint32_t> unit(ctus);
  for (int y = 0; y < pic.ctus_y; y++) for (int x = 0; x < pic.ctus_x; x++) {
    int tx = 0, ty = 0;
    while (tx + 1 < c.tile_columns && x >= col_bd[tx + 1]) tx++;
    while (ty + 1 < c.tile_rows && y >= row_bd[ty + 1]) ty++;
    const int tile = ty * c.tile_columns + tx, slice = sl.mode == 1 ? y / (sl.argument / pic.ctus_x) : (sl.mode == 3 ? tile / sl.argument : 0);
    unit[(size_t)y * pic.ctus_x + x] = (uint32_t)slice * 1024u + (uint32_t)tile;
  }
  pic.unit = unit.data();
  const size_t fb = (size_t)c.width * c.height * 3 / 2 * (c.bit_depth > 8 ? 2 : 1);
  out.assign(fb * (size_t)n, 0);
  std::unique_ptr<RcWork> w(new RcWork);
  for (int f = 0; f < n; f++) {
    pic.recs = recs + (size_t)f * ctus; pic.out = out.data() + (size_t)f * fb; pic.qp_map = map + (size_t)f * ctus * 256;
    for (int cy = 0; cy < pic.ctus_y; cy++) for (int cx = 0; cx < pic.ctus_x; cx++) {
      if (c.bit_depth == 8) rc_ctu<uint8_t>(pic, *w, 0, 1, cx, cy); else rc_ctu<uint16_t>(pic, *w, 0, 1, cx, cy);
    }
  }
  return true;
}

// the same status from the parser and from the core; behind a success the same bytes, no factor of 0, and (deep) a reconstruction that runs
static bool same(const uint8_t *s, size_t n, const char *path, const char *what, size_t at, bool deep)
{
  Parsed a, b;
  parse(hevcdl_parse_stream_sl, s, n, a);
  parse(hevcdl_parse_stream_core_sl, s, n, b);
  if (a.st != b.st) { printf("scaling_list harness: %s: %s %zu: parser %d, core %d\n", path, what, at, (int)a.st, (int)b.st); return false; }
  if (a.st != HEVCDL_OK) return true;
  const size_t all = a.ctus * (size_t)a.n;
  if (memcmp(a.recs.get(), b.recs.get(), all * sizeof(hevcdl_ctu_record)) || memcmp(a.sao.get(), b.sao.get(), all * sizeof(hevcdl_sao_blk)) || memcmp(a.map.get(), b.map.get(), all * 256) ||
      memcmp(a.si.get(), b.si.get(), sizeof(hevcdl_scaling_info))) {
    printf("scaling_list harness: %s: %s %zu: parser and core differ in records, SAO blocks, the QP map or the factors\n", path, what, at); return false;
  }
  for (int i = 0; i < HEVCDL_SCALING_FACTOR_BYTES; i++) if (!a.si->factor[i]) { printf("scaling_list harness: %s: %s %zu: factor %d is 0\n", path, what, at, i); return false; }
  if (deep) {
    std::vector<unsigned char> got;
    if (!reconstruct(a.cfg, a.sl, a.qi, *a.si, a.recs.get(), a.map.get(), a.n, a.ctus, got)) { printf("scaling_list harness: %s: %s %zu: no tile grid\n", path, what, at); return false; }
  }
  return true;
}

static int run(const char *path)
{
  FILE *f = fopen(path, "rb");
  if (!f) { printf("scaling_list harness: cannot open %s\n", path); return 1; }
  int64_t head[3];
  if (fread(head, sizeof head, 1, f) != 1 || head[0] < 0 || head[1] < 0) { fclose(f); printf("scaling_list harness: %s: short dump\n", path); return 1; }
  std::unique_ptr<uint8_t[]> stream(new uint8_t[(size_t)head[0]]);
  std::vector<unsigned char> want((size_t)head[1]);
  if (fread(stream.get(), 1, (size_t)head[0], f) != (size_t)head[0] || (head[1] && fread(want.data(), 1, want.size(), f) != want.size())) { fclose(f); printf("scaling_list harness: %s: short dump\n", path); return 1; }
  fclose(f);
  const size_t n = (size_t)head[0];
  { // without the switch: refused, by both, also where cu_qp alone is accepted
    hevcdl_stream_config cfg; memset(&cfg, 0, sizeof cfg); cfg.struct_size = sizeof cfg; int k = 0;
    if (hevcdl_parse_stream(stream.get(), n, &cfg, nullptr, nullptr, nullptr, 0, &k, nullptr, nullptr, 0) != HEVCDL_ERR_UNSUPPORTED ||
        hevcdl_parse_stream_core(stream.get(), n, &cfg, nullptr, nullptr, nullptr, 0, &k, nullptr, nullptr, 0) != HEVCDL_ERR_UNSUPPORTED ||
        hevcdl_parse_stream_qp(stream.get(), n, HEVCDL_ACCEPT_CU_QP, &cfg, nullptr, nullptr, nullptr, 0, &k, nullptr, nullptr, 0, nullptr, nullptr) != HEVCDL_ERR_UNSUPPORTED) {
      printf("scaling_list harness: %s: accepted without the switch\n", path); return 1;
    }
  }
  Parsed p;
  parse(hevcdl_parse_stream_core_sl, stream.get(), n, p);
  if (p.st != HEVCDL_OK) { printf("scaling_list harness: %s: status %d: %s\n", path, (int)p.st, hevcdl_parse_error()); return 1; }
  if (!p.si->enabled) { printf("scaling_list harness: %s: a stream without scaling lists\n", path); return 1; }
  if (!same(stream.get(), n, path, "stream", 0, false)) return 1;
  if (!want.empty()) {
    std::vector<unsigned char> got;
    if (!reconstruct(p.cfg, p.sl, p.qi, *p.si, p.recs.get(), p.map.get(), p.n, p.ctus, got) || got.size() != want.size() || memcmp(got.data(), want.data(), got.size())) {
      printf("scaling_list harness: %s: the reconstruction differs from the reference decoder's pictures\n", path); return 1;
    }
  }
  if (head[2] == 1) {
    for (size_t bit = 0; bit < n * 8; bit++) {
      stream[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      const bool ok = same(stream.get(), n, path, "flip", bit, true);
      stream[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      if (!ok) return 1;
    }
    for (size_t cut = 0; cut < n; cut++) { // a copy of its own size: the parser may not read behind the cut
      std::unique_ptr<uint8_t[]> part(new uint8_t[cut ? cut : 1]);
      memcpy(part.get(), stream.get(), cut);
      if (!same(part.get(), cut, path, "truncation", cut, false)) return 1;
    }
    printf("%s: %zu flips and %zu truncations agree\n", path, n * 8, n);
  }
  return 0;
}

// Synthetic records of one 64x64 CTU: levels of +-32767 everywhere, factors of 1 and 255 side by side, at QP 51 and at the lowest QpY of the bit depth; `small` 0: four 32x32
// luma blocks with their 16x16 chroma blocks, 1: 4x4 blocks, every other one transform-skipped.  Every output sample must be a sample; the sanitizer watches the arithmetic.
static int extremes()
{
  int failed = 0;
  for (int bd = 8; bd <= 10; bd += 2) for (int hi = 0; hi < 2; hi++) for (int small = 0; small < 2; small++) {
    std::unique_ptr<hevcdl_ctu_record[]> rec(new hevcdl_ctu_record[1]);
    memset(rec.get(), 0, sizeof(hevcdl_ctu_record));
    hevcdl_ctu_record &r = rec[0];
    for (int z = 0; z < 256; z++) {
      r.depth[z] = small ? 3 : 0; r.tr_idx[z] = 1; r.luma_dir[z] = (uint8_t)(small && (z & 4) ? 26 : 1); r.chroma_dir[z] = 1;      // (one mode per CU: DC, or vertical for every other 8x8 CU)
      for (int c = 0; c < 3; c++) { r.cbf[c][z] = 3; r.tskip[c][z] = (uint8_t)(small && ((z >> 2) & 1)); }
    }
    for (int i = 0; i < 4096; i++) r.coeff_y[i] = (int16_t)(((i * 7) & 8) ? 32767 : -32767);
    for (int i = 0; i < 1024; i++) { r.coeff_cb[i] = (int16_t)((i & 1) ? -32767 : 32767); r.coeff_cr[i] = (int16_t)((i & 2) ? 32767 : -32767); }
    hevcdl_stream_config c; hevcdl_stream_config_default(&c, 64, 64, 26);
    c.bit_depth = bd;
    hevcdl_slice_layout sl = { 0, 0, 1 }; hevcdl_qp_info qi = { 0, 0, hi ? 12 : -12, hi ? 12 : -12 };
    std::unique_ptr<hevcdl_scaling_info> si(new hevcdl_scaling_info);
    si->enabled = si->data_present = 1;
    for (int i = 0; i < HEVCDL_SCALING_FACTOR_BYTES; i++) si->factor[i] = (uint8_t)(((i ^ (i >> 3)) & 1) ? 255 : 1);
    std::unique_ptr<int8_t[]> map(new int8_t[256]);
    memset(map.get(), hi ? 51 : -6 * (bd - 8), 256);
    if (hevcdl_validate_records(&c, rec.get(), 1) != HEVCDL_OK) { printf("scaling_list harness: extremes: the synthetic records are refused: %s\n", hevcdl_parse_error()); return 1; }
    std::vector<unsigned char> got;
    if (!reconstruct(c, sl, qi, *si, rec.get(), map.get(), 1, 1, got)) { failed++; continue; }
    const int pmax = (1 << bd) - 1; int lo = 0, hi_n = 0;
    for (size_t i = 0; i < (size_t)64 * 64 * 3 / 2; i++) {
      const int v = bd == 8 ? got[i] : (got[2 * i] | (got[2 * i + 1] << 8));
      if (v > pmax) failed++;
      lo += v == 0; hi_n += v == pmax;
    }
    printf("extremes: %d bits, QpY %d, %s blocks: %d samples at 0, %d at %d\n", bd, hi ? 51 : -6 * (bd - 8), small ? "4x4" : "32x32", lo, hi_n, pmax);
  }
  return failed;
}

int main(int argc, char **argv)
{
  int failed = 0;
  for (int i = 1; i < argc; i++) failed += strcmp(argv[i], "extremes") ? run(argv[i]) : (extremes() != 0);
  printf("scaling_list harness: %d dumps, %d failed\n", argc - 1, failed);
  return failed ? 1 : 0;
}
