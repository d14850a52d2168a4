// report_harness.cpp -- csrc/picture_hash_core.h under AddressSanitizer / UndefinedBehaviorSanitizer on the CPU (tests/test_report.py builds and runs it; it is never
// loaded into Python and never runs on a GPU).
//
// Every argument is a dump: int32 width, height, bit depth, chunk bytes; the 16 bytes of the plane's MD5 as hashlib computed it; the plane's bytes.  The plane is copied
// into a heap block of exactly its size, so that a read past either end is a sanitizer report.  MD5 is compared with the dump's digest, CRC and checksum with the
// reference's serial loops restated below (TComPicYuvMD5.cpp:89-165).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "picture_hash_core.h"

static unsigned crc_serial(const uint8_t *p, size_t n)
{
  unsigned crc = 0xffff;
  for (size_t i = 0; i < n; i++) for (int b = 0; b < 8; b++) { const unsigned msb = (crc >> 15) & 1, bit = (p[i] >> (7 - b)) & 1; crc = (((crc << 1) + bit) & 0xffff) ^ (msb * 0x1021); }
  for (int b = 0; b < 16; b++) { const unsigned msb = (crc >> 15) & 1; crc = ((crc << 1) & 0xffff) ^ (msb * 0x1021); }
  return crc;
}

static uint32_t checksum_serial(const uint8_t *p, int w, int h, int sb)
{
  uint32_t sum = 0;
  for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
    const unsigned mask = ((unsigned)x & 0xff) ^ ((unsigned)y & 0xff) ^ ((unsigned)x >> 8) ^ ((unsigned)y >> 8);
    for (int k = 0; k < sb; k++) sum += (p[((size_t)y * w + x) * sb + k] ^ mask) & 0xff;
  }
  return sum;
}

int main(int argc, char **argv)
{
  int failed = 0;
  for (int a = 1; a < argc; a++) {
    FILE *f = fopen(argv[a], "rb");
    int32_t hdr[4]; uint8_t want_md5[16];
    if (!f || fread(hdr, sizeof hdr, 1, f) != 1 || fread(want_md5, 16, 1, f) != 1) { printf("report harness: cannot read %s\n", argv[a]); if (f) fclose(f); failed++; continue; }
    const int w = hdr[0], h = hdr[1], bd = hdr[2], sb = bd > 8 ? 2 : 1;
    const uint64_t chunk = hdr[3] > 0 ? (uint64_t)hdr[3] : HEVCDL_REPORT_CHUNK_BYTES;
    const size_t n = (size_t)w * h * sb;
    uint8_t *plane = (uint8_t *)malloc(n);                                // exactly the plane: no slack on either side
    const bool ok_read = plane && fread(plane, 1, n, f) == n;
    fclose(f);
    if (!ok_read) { printf("report harness: short dump %s\n", argv[a]); free(plane); failed++; continue; }
    uint8_t dg[16];
    bool ok = true;
    memset(dg, 0, sizeof dg);
    ok = hevcdl_ph::plane_hash_chunked(plane, (uint32_t)w, (uint32_t)h, sb, 1, chunk, dg) == 16 && memcmp(dg, want_md5, 16) == 0;
    if (!ok) printf("report harness: MD5 differs for %s\n", argv[a]);
    const unsigned crc = crc_serial(plane, n);
    if (hevcdl_ph::plane_hash_chunked(plane, (uint32_t)w, (uint32_t)h, sb, 2, chunk, dg) != 2 || dg[0] != (crc >> 8) || dg[1] != (crc & 0xff)) { printf("report harness: CRC differs for %s\n", argv[a]); ok = false; }
    { // the partials as an array, folded by crc_fold: the device's form
      const size_t chunks = hevcdl_ph::report_chunks(n, chunk);
      std::vector<uint32_t> part(chunks);
      for (size_t k = 0; k < chunks; k++) { const uint64_t at = k * chunk, end = at + chunk < n ? at + chunk : n; part[k] = hevcdl_ph::crc_bytes(0, plane + at, (size_t)(end - at)); }
      if (hevcdl_ph::crc_fold(part.data(), chunks, n, chunk) != crc) { printf("report harness: folded CRC differs for %s\n", argv[a]); ok = false; }
    }
    const uint32_t sum = checksum_serial(plane, w, h, sb);
    if (hevcdl_ph::plane_hash_chunked(plane, (uint32_t)w, (uint32_t)h, sb, 3, chunk, dg) != 4 || dg[0] != (sum >> 24) || dg[1] != ((sum >> 16) & 0xff) || dg[2] != ((sum >> 8) & 0xff) || dg[3] != (sum & 0xff)) {
      printf("report harness: checksum differs for %s\n", argv[a]); ok = false;
    }
    free(plane);
    if (!ok) failed++;
  }
  printf("report harness: %d dumps, %d failed\n", argc - 1, failed);
  return failed ? 1 : 0;
}
