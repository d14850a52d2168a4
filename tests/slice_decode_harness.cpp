// tests/slice_decode_harness.cpp -- TEST INFRASTRUCTURE.  The shared slice-data decoder (csrc/slice_decode_core.h behind hevcdl_parse_stream_core) held against the
// parser (hevcdl_parse_stream) as a stand-alone program, built by tests/test_parse_core.py with the host compiler and -fsanitize=address,undefined.  Every dump is a
// stream in an exact-size heap block, parsed by both into exact-size blocks: status, picture infos, configuration, layouts, records and SAO blocks must be equal, byte for
// byte.  With the dump's switch every single-bit flip of the stream goes through both: equal status; where both still parse, equal records and SAO blocks; where both
// name a CTU, the same CTU.  Dump: int64 stream bytes, int64 flips; the stream.  The same program, built with a mutated copy of the core in front of the include path, is
// the mutation check: a dump whose comparison fails is a fixture that catches the mutant.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "hevcdl.h"

typedef hevcdl_status (*ParseFn)(const uint8_t *, size_t, hevcdl_stream_config *, hevcdl_slice_layout *, hevcdl_segment_layout *, hevcdl_parsed_picture *, int, int *, hevcdl_ctu_record *,
                                 hevcdl_sao_blk *, size_t);
static int ctus_of(int w, int h) { return ((w + 63) >> 6) * ((h + 63) >> 6); }

struct Parsed {
  hevcdl_status st; hevcdl_stream_config cfg; hevcdl_slice_layout sl; hevcdl_segment_layout sg; int n; std::string why;
  std::unique_ptr<hevcdl_ctu_record[]> recs; std::unique_ptr<hevcdl_sao_blk[]> sao; std::unique_ptr<hevcdl_parsed_picture[]> pics; size_t ctus;
};

static void parse(ParseFn fn, const uint8_t *s, size_t n, Parsed &p)
{
  memset(&p.cfg, 0, sizeof p.cfg); p.cfg.struct_size = sizeof p.cfg; p.n = 0; p.ctus = 0; memset(&p.sl, 0, sizeof p.sl); memset(&p.sg, 0, sizeof p.sg);
  p.st = fn(s, n, &p.cfg, nullptr, nullptr, nullptr, 0, &p.n, nullptr, nullptr, 0);
  if (p.st == HEVCDL_OK) {
    p.ctus = (size_t)ctus_of(p.cfg.width, p.cfg.height) * (size_t)p.n;
    p.recs.reset(new hevcdl_ctu_record[p.ctus]); p.sao.reset(new hevcdl_sao_blk[p.ctus]); p.pics.reset(new hevcdl_parsed_picture[(size_t)p.n]);      // exact sizes: a CTU written past the end is a report
    memset(p.recs.get(), 0xa5, sizeof(hevcdl_ctu_record) * p.ctus); memset(p.sao.get(), 0xa5, sizeof(hevcdl_sao_blk) * p.ctus);                        // what a decoder leaves unwritten shows
    p.st = fn(s, n, &p.cfg, &p.sl, &p.sg, p.pics.get(), p.n, &p.n, p.recs.get(), p.sao.get(), p.ctus);
  }
  p.why = hevcdl_parse_error();
}

// the CTU a sentence names ("CTU 17"), -1: none
static long ctu_named(const std::string &s)
{
  for (size_t at = s.find("CTU "); at != std::string::npos; at = s.find("CTU ", at + 1))
    if (at + 4 < s.size() && s[at + 4] >= '0' && s[at + 4] <= '9') return strtol(s.c_str() + at + 4, nullptr, 10);
  return -1;
}

// "" where the two agree
static std::string compare(const uint8_t *s, size_t n)
{
  Parsed a, b;
  parse(hevcdl_parse_stream, s, n, a);
  parse(hevcdl_parse_stream_core, s, n, b);
  if (a.st != b.st) return "status " + std::to_string((int)a.st) + " (" + a.why + ") against " + std::to_string((int)b.st) + " (" + b.why + ")";
  if (a.st != HEVCDL_OK) {
    if (b.why.empty()) return "refused without a sentence";
    const long ca = ctu_named(a.why), cb = ctu_named(b.why);
    if (ca >= 0 && cb >= 0 && ca != cb) return "the parser names CTU " + std::to_string(ca) + " (" + a.why + "), the core CTU " + std::to_string(cb) + " (" + b.why + ")";
    return "";
  }
  if (a.n != b.n || memcmp(&a.cfg, &b.cfg, sizeof a.cfg) || memcmp(&a.sl, &b.sl, sizeof a.sl) || memcmp(&a.sg, &b.sg, sizeof a.sg)) return "picture count, configuration or layouts differ";
  if (memcmp(a.pics.get(), b.pics.get(), sizeof(hevcdl_parsed_picture) * (size_t)a.n)) return "picture infos differ";
  for (size_t i = 0; i < a.ctus; i++) {
    if (memcmp(&a.recs[i], &b.recs[i], sizeof(hevcdl_ctu_record))) return "the record of CTU " + std::to_string(i) + " differs";
    if (memcmp(&a.sao[i], &b.sao[i], sizeof(hevcdl_sao_blk))) return "the SAO block of CTU " + std::to_string(i) + " differs";
  }
  if (hevcdl_validate_records(&b.cfg, b.recs.get(), b.n) != HEVCDL_OK) return std::string("the core's records do not validate: ") + hevcdl_parse_error();
  return "";
}

static int run(const char *path)
{
  FILE *f = fopen(path, "rb");
  if (!f) { printf("slice decode harness: %s: cannot open\n", path); return 1; }
  int64_t head[2];
  if (fread(head, sizeof head, 1, f) != 1 || head[0] < 0) { fclose(f); printf("slice decode harness: %s: short dump\n", path); return 1; }
  std::unique_ptr<uint8_t[]> stream(new uint8_t[(size_t)head[0]]);
  if (fread(stream.get(), 1, (size_t)head[0], f) != (size_t)head[0]) { fclose(f); printf("slice decode harness: %s: short dump\n", path); return 1; }
  fclose(f);
  std::string why = compare(stream.get(), (size_t)head[0]);
  if (!why.empty()) { printf("slice decode harness: %s: %s\n", path, why.c_str()); return 1; }
  if (head[1]) {
    for (size_t bit = 0; bit < (size_t)head[0] * 8; bit++) {
      stream[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      why = compare(stream.get(), (size_t)head[0]);
      stream[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
      if (!why.empty()) { printf("slice decode harness: %s: flip %zu: %s\n", path, bit, why.c_str()); return 1; }
    }
    printf("%s: %zu flips agree\n", path, (size_t)head[0] * 8);
  }
  return 0;
}

int main(int argc, char **argv)
{
  int failed = 0;
  for (int i = 1; i < argc; i++) failed += run(argv[i]);
  printf("slice decode harness: %d dumps, %d failed\n", argc - 1, failed);
  return failed ? 1 : 0;
}
