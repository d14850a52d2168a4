// tests/decode_harness.cpp -- TEST INFRASTRUCTURE.  The stream parser (csrc/hevcdl_parse.cpp) as a stand-alone program, built by tests/test_decode.py with the host
// compiler and -fsanitize=address,undefined.  Every dump is a stream in an exact-size heap block (a read one byte past its end is a sanitizer report), optionally the
// records the stream was coded from, and a switch that runs every single-bit flip of the stream through the parser with hevcdl_validate_records behind each flip that
// parses.  Dump: int64 stream bytes, int64 record bytes, int64 flips; the stream; the records.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "hevcdl.h"

static int ctus_of(int w, int h) { return ((w + 63) >> 6) * ((h + 63) >> 6); }
static int z_of(int x4, int y4)
{
  int z = 0;
  for (int b = 0; b < 4; b++) z |= ((x4 >> b) & 1) << (2 * b) | ((y4 >> b) & 1) << (2 * b + 1);
  return z;
}

struct Parsed { hevcdl_status st; hevcdl_stream_config cfg; int n; std::vector<hevcdl_ctu_record> recs; std::vector<hevcdl_sao_blk> sao; std::vector<hevcdl_parsed_picture> pics; };

static void parse(const uint8_t *s, size_t n, Parsed &p)
{
  memset(&p.cfg, 0, sizeof p.cfg); p.cfg.struct_size = sizeof p.cfg; p.n = 0;
  p.st = hevcdl_parse_stream(s, n, &p.cfg, nullptr, nullptr, nullptr, 0, &p.n, nullptr, nullptr, 0);
  if (p.st != HEVCDL_OK) return;
  const size_t ctus = (size_t)ctus_of(p.cfg.width, p.cfg.height) * (size_t)p.n;
  p.recs.resize(ctus); p.sao.resize(ctus); p.pics.resize((size_t)p.n);      // exact sizes: a CTU written past the end is a report
  hevcdl_slice_layout sl; hevcdl_segment_layout sg;
  p.st = hevcdl_parse_stream(s, n, &p.cfg, &sl, &sg, p.pics.data(), p.n, &p.n, p.recs.data(), p.sao.data(), ctus);
}

static int run(const char *path)
{
  FILE *f = fopen(path, "rb");
  if (!f) { printf("decode harness: cannot open %s\n", path); return 1; }
  int64_t head[3];
  if (fread(head, sizeof head, 1, f) != 1 || head[0] < 0 || head[1] < 0) { fclose(f); printf("decode harness: %s: short dump\n", path); return 1; }
  std::unique_ptr<uint8_t[]> stream(new uint8_t[(size_t)head[0]]);
  std::vector<uint8_t> want((size_t)head[1]);
  if (fread(stream.get(), 1, (size_t)head[0], f) != (size_t)head[0] || (head[1] && fread(want.data(), 1, want.size(), f) != want.size())) { fclose(f); printf("decode harness: %s: short dump\n", path); return 1; }
  fclose(f);
  Parsed p;
  parse(stream.get(), (size_t)head[0], p);
  if (p.st != HEVCDL_OK) { printf("decode harness: %s: status %d: %s\n", path, (int)p.st, hevcdl_parse_error()); return 1; }
  if (hevcdl_validate_records(&p.cfg, p.recs.data(), p.n) != HEVCDL_OK) { printf("decode harness: %s: the parser's records do not validate: %s\n", path, hevcdl_parse_error()); return 1; }
  if (!want.empty()) {
    if (want.size() != p.recs.size() * sizeof(hevcdl_ctu_record)) { printf("decode harness: %s: %zu record bytes, the stream has %zu\n", path, want.size(), p.recs.size() * sizeof(hevcdl_ctu_record)); return 1; }
    const hevcdl_ctu_record *w = (const hevcdl_ctu_record *)want.data();
    const int cx = (p.cfg.width + 63) >> 6, ctus = ctus_of(p.cfg.width, p.cfg.height);
    for (size_t i = 0; i < p.recs.size(); i++) {
      const hevcdl_ctu_record &a = p.recs[i], &b = w[i];
      if (memcmp(a.coeff_y, b.coeff_y, sizeof a.coeff_y) || memcmp(a.coeff_cb, b.coeff_cb, sizeof a.coeff_cb) || memcmp(a.coeff_cr, b.coeff_cr, sizeof a.coeff_cr)) { printf("decode harness: %s: levels of CTU %zu differ\n", path, i); return 1; }
      const int x0 = ((int)(i % (size_t)ctus) % cx) * 64, y0 = ((int)(i % (size_t)ctus) / cx) * 64;
      for (int y4 = 0; y4 < 16; y4++) for (int x4 = 0; x4 < 16; x4++) {
        if (x0 + 4 * x4 >= p.cfg.width || y0 + 4 * y4 >= p.cfg.height) continue;
        const int z = z_of(x4, y4);
        if (a.depth[z] != b.depth[z] || a.part_size[z] != b.part_size[z] || a.luma_dir[z] != b.luma_dir[z] || a.chroma_dir[z] != b.chroma_dir[z] || a.tr_idx[z] != b.tr_idx[z] ||
            a.cbf[0][z] != b.cbf[0][z] || a.cbf[1][z] != b.cbf[1][z] || a.cbf[2][z] != b.cbf[2][z]) { printf("decode harness: %s: CTU %zu differs at partition %d\n", path, i, z); return 1; }
      }
    }
  }
  if (head[2]) {
    long ok = 0, refused = 0;
    for (size_t bit = 0; bit < (size_t)head[0] * 8; bit++) {
      stream[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      Parsed q;
      parse(stream.get(), (size_t)head[0], q);
      stream[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      if (q.st != HEVCDL_OK) { refused++; if (!hevcdl_parse_error()[0]) { printf("decode harness: %s: flip %zu refused without a sentence\n", path, bit); return 1; } continue; }
      ok++;
      if (hevcdl_validate_records(&q.cfg, q.recs.data(), q.n) != HEVCDL_OK) { printf("decode harness: %s: flip %zu parses to records that do not validate: %s\n", path, bit, hevcdl_parse_error()); return 1; }
    }
    printf("%s: %ld flips refused, %ld parsed\n", path, refused, ok);
  }
  return 0;
}

int main(int argc, char **argv)
{
  int failed = 0;
  for (int i = 1; i < argc; i++) failed += run(argv[i]);
  printf("decode harness: %d dumps, %d failed\n", argc - 1, failed);
  return failed ? 1 : 0;
}
