// tests/cu_qp_harness.cpp -- TEST INFRASTRUCTURE.  The QP-map forms of the stream parser (csrc/hevcdl_parse.cpp), of the shared slice-data decoder
// (csrc/slice_decode_core.h through hevcdl_parse_stream_core_qp) and of the reconstruction (csrc/recon_core.h, instantiated here with RcPicQp on one "lane") as a
// stand-alone program.  tests/test_cu_qp.py builds it with the host compiler and -fsanitize=address,undefined and runs it over the cuqp_* fixtures and damaged streams;
// tools/cu_qp_mutants.py builds it from sources with one line changed and expects it to fail.
// Every buffer is an exact-size heap block: a byte read behind a stream, or a record, SAO block or map entry written behind its array, is a sanitizer report.
// Dump: int64 stream bytes, int64 picture bytes (0: none; otherwise the reference decoder's pictures of a filters-off stream), int64 mode (0: must parse; 1: every
// single-bit flip and every truncation must give the same status from parser and core; 2: the stream as it is must give the same status from both, whatever it is);
// the stream; the pictures.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#include "recon_core.h"

using namespace hevcdl_rc;

struct Parsed {
  hevcdl_status st; hevcdl_stream_config cfg; hevcdl_slice_layout sl; hevcdl_segment_layout sg; hevcdl_qp_info qi; int n; size_t ctus;
  std::unique_ptr<hevcdl_ctu_record[]> recs; std::unique_ptr<hevcdl_sao_blk[]> sao; std::unique_ptr<int8_t[]> map;
};
typedef hevcdl_status (*ParseFn)(const uint8_t *, size_t, unsigned, hevcdl_stream_config *, hevcdl_slice_layout *, hevcdl_segment_layout *, hevcdl_parsed_picture *, int, int *,
                                 hevcdl_ctu_record *, hevcdl_sao_blk *, size_t, hevcdl_qp_info *, int8_t *);

static void parse(ParseFn fn, const uint8_t *s, size_t n, Parsed &p)
{
  memset(&p.cfg, 0, sizeof p.cfg); p.cfg.struct_size = sizeof p.cfg; p.n = 0; p.ctus = 0;
  p.st = hevcdl_parse_stream_qp(s, n, HEVCDL_ACCEPT_CU_QP, &p.cfg, &p.sl, &p.sg, nullptr, 0, &p.n, nullptr, nullptr, 0, &p.qi, nullptr);
  if (p.st != HEVCDL_OK) return;
  p.ctus = (size_t)(((p.cfg.width + 63) >> 6) * ((p.cfg.height + 63) >> 6));
  const size_t all = p.ctus * (size_t)p.n;
  p.recs.reset(new hevcdl_ctu_record[all]); p.sao.reset(new hevcdl_sao_blk[all]); p.map.reset(new int8_t[all * 256]);
  std::vector<hevcdl_parsed_picture> pics((size_t)p.n);
  p.st = fn(s, n, HEVCDL_ACCEPT_CU_QP, &p.cfg, &p.sl, &p.sg, pics.data(), p.n, &p.n, p.recs.get(), p.sao.get(), all, &p.qi, p.map.get());
}

// the filters-off pictures of the core's records and map: what hevcdl_reconstruct_frames_qp_host does, from recon_core.h
static bool reconstruct(const Parsed &p, std::vector<unsigned char> &out)
{
  RcPicQp pic; memset(&pic, 0, sizeof pic);
  const hevcdl_stream_config &c = p.cfg;
  pic.W = c.width; pic.H = c.height; pic.ctus_x = (c.width + 63) >> 6; pic.ctus_y = (c.height + 63) >> 6; pic.bit_depth = c.bit_depth; pic.qp = c.qp;
  pic.strong = (c.tools & HEVCDL_TOOL_STRONG_INTRA) != 0; pic.cb_off = p.qi.cb_qp_offset; pic.cr_off = p.qi.cr_qp_offset;
  int col_bd[21], row_bd[23];
  if (hevcdl_tile_bounds(pic.ctus_x, c.tile_columns, c.tile_uniform_spacing != 0, c.tile_column_width, 1, col_bd) ||
      hevcdl_tile_bounds(pic.ctus_y, c.tile_rows, c.tile_uniform_spacing != 0, c.tile_row_height, 1, row_bd)) return false;
  std::vector<uint32_t> unit(p.ctus);
  for (int y = 0; y < pic.ctus_y; y++) for (int x = 0; x < pic.ctus_x; x++) {
    int tx = 0, ty = 0;
    while (tx + 1 < c.tile_columns && x >= col_bd[tx + 1]) tx++;
    while (ty + 1 < c.tile_rows && y >= row_bd[ty + 1]) ty++;
    const int tile = ty * c.tile_columns + tx, slice = p.sl.mode == 1 ? y / (p.sl.argument / pic.ctus_x) : (p.sl.mode == 3 ? tile / p.sl.argument : 0);
    unit[(size_t)y * pic.ctus_x + x] = (uint32_t)slice * 1024u + (uint32_t)tile;
  }
  pic.unit = unit.data();
  const size_t fb = (size_t)c.width * c.height * 3 / 2 * (c.bit_depth > 8 ? 2 : 1);
  out.assign(fb * (size_t)p.n, 0);
  std::unique_ptr<RcWork> w(new RcWork);
  for (int f = 0; f < p.n; f++) {
    pic.recs = p.recs.get() + (size_t)f * p.ctus; pic.out = out.data() + (size_t)f * fb; pic.qp_map = p.map.get() + (size_t)f * p.ctus * 256;
    for (int cy = 0; cy < pic.ctus_y; cy++) for (int cx = 0; cx < pic.ctus_x; cx++) {
      if (c.bit_depth == 8) rc_ctu<uint8_t>(pic, *w, 0, 1, cx, cy); else rc_ctu<uint16_t>(pic, *w, 0, 1, cx, cy);
    }
  }
  return true;
}

// the same status from the parser and from the core; behind a success the same bytes
static bool same(const uint8_t *s, size_t n, const char *path, const char *what, size_t at)
{
  Parsed a, b;
  parse(hevcdl_parse_stream_qp, s, n, a);
  parse(hevcdl_parse_stream_core_qp, s, n, b);
  if (a.st != b.st) { printf("cu_qp harness: %s: %s %zu: parser %d, core %d\n", path, what, at, (int)a.st, (int)b.st); return false; }
  if (a.st != HEVCDL_OK) return true;
  const size_t all = a.ctus * (size_t)a.n;
  if (memcmp(a.recs.get(), b.recs.get(), all * sizeof(hevcdl_ctu_record)) || memcmp(a.sao.get(), b.sao.get(), all * sizeof(hevcdl_sao_blk)) || memcmp(a.map.get(), b.map.get(), all * 256)) {
    printf("cu_qp harness: %s: %s %zu: parser and core differ in records, SAO blocks or the QP map\n", path, what, at); return false;
  }
  return true;
}

static int run(const char *path)
{
  FILE *f = fopen(path, "rb");
  if (!f) { printf("cu_qp harness: cannot open %s\n", path); return 1; }
  int64_t head[3];
  if (fread(head, sizeof head, 1, f) != 1 || head[0] < 0 || head[1] < 0) { fclose(f); printf("cu_qp harness: %s: short dump\n", path); return 1; }
  std::unique_ptr<uint8_t[]> stream(new uint8_t[(size_t)head[0]]);
  std::vector<unsigned char> want((size_t)head[1]);
  if (fread(stream.get(), 1, (size_t)head[0], f) != (size_t)head[0] || (head[1] && fread(want.data(), 1, want.size(), f) != want.size())) { fclose(f); printf("cu_qp harness: %s: short dump\n", path); return 1; }
  fclose(f);
  const size_t n = (size_t)head[0];
  if (head[2] == 2) return same(stream.get(), n, path, "stream", 0) ? 0 : 1;
  { // without the switch: refused, by both
    hevcdl_stream_config cfg; memset(&cfg, 0, sizeof cfg); cfg.struct_size = sizeof cfg; int k = 0;
    if (hevcdl_parse_stream(stream.get(), n, &cfg, nullptr, nullptr, nullptr, 0, &k, nullptr, nullptr, 0) != HEVCDL_ERR_UNSUPPORTED ||
        hevcdl_parse_stream_core(stream.get(), n, &cfg, nullptr, nullptr, nullptr, 0, &k, nullptr, nullptr, 0) != HEVCDL_ERR_UNSUPPORTED) { printf("cu_qp harness: %s: accepted without the switch\n", path); return 1; }
  }
  Parsed p;
  parse(hevcdl_parse_stream_core_qp, stream.get(), n, p);
  if (p.st != HEVCDL_OK) { printf("cu_qp harness: %s: status %d: %s\n", path, (int)p.st, hevcdl_parse_error()); return 1; }
  if (!same(stream.get(), n, path, "stream", 0)) return 1;
  if (!want.empty()) {
    std::vector<unsigned char> got;
    if (!reconstruct(p, got) || got.size() != want.size() || memcmp(got.data(), want.data(), got.size())) { printf("cu_qp harness: %s: the reconstruction differs from the reference decoder's pictures\n", path); return 1; }
  }
  if (head[2] == 1) {
    for (size_t bit = 0; bit < n * 8; bit++) {
      stream[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      const bool ok = same(stream.get(), n, path, "flip", bit);
      stream[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      if (!ok) return 1;
    }
    for (size_t cut = 0; cut < n; cut++) { // a copy of its own size: the parser may not read behind the cut
      std::unique_ptr<uint8_t[]> part(new uint8_t[cut ? cut : 1]);
      memcpy(part.get(), stream.get(), cut);
      if (!same(part.get(), cut, path, "truncation", cut)) return 1;
    }
    printf("%s: %zu flips and %zu truncations agree\n", path, n * 8, n);
  }
  return 0;
}

int main(int argc, char **argv)
{
  int failed = 0;
  for (int i = 1; i < argc; i++) failed += run(argv[i]);
  printf("cu_qp harness: %d dumps, %d failed\n", argc - 1, failed);
  return failed ? 1 : 0;
}
