// Sanitizer harness of the shared entropy coder (csrc/entropy_coder.h): tests/test_entropy.py compiles this file together with csrc/hevcdl_bitstream.cpp with the host
// compiler and -fsanitize=address,undefined, and runs it on dumped inputs.  The index arithmetic of the device kernel is this source: a wild index shows up here as a
// sanitizer report.  Sanitizers stay on host code.
//
// A dump: hevcdl_stream_config, then int32 { n_frames, has_sao, capacity_per_ctu, mode }, the records, the SAO parameters.  Every dump: lengths within the capacity or the
// overflow word set, the canaries between the regions intact; every picture through hevcdl_write_access_unit (which codes into a first-pass region and, past it, once
// more) into an allocation of exactly its length, and, where no region overflowed, equal to hevcdl_code_slice_data_host + hevcdl_write_access_unit_from_slice_data.
// mode 0 (fixtures, synthetic corpus): no region may overflow; mode 1: overflow and garbage records.  The regions of a dump share one buffer, so a store past a region
// shows in the canary gap behind it (AddressSanitizer does not see it); the first picture of a dump with a single sub-stream (no tiles, no wavefront) is coded once
// more into an allocation of exactly its capacity, where such a store is also an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "hevcdl.h"
#include "entropy_coder.h"

static int run(const char *path)
{
  FILE *f = fopen(path, "rb");
  if (!f) { printf("%s: cannot open\n", path); return 2; }
  hevcdl_stream_config cfg; int32_t hd[4];
  if (fread(&cfg, sizeof cfg, 1, f) != 1 || fread(hd, sizeof hd, 1, f) != 1) { fclose(f); printf("%s: short header\n", path); return 2; }
  const int n_frames = hd[0], has_sao = hd[1], cpc = hd[2], mode = hd[3];
  const size_t ctus = (size_t)((cfg.width + 63) >> 6) * ((cfg.height + 63) >> 6);
  std::vector<hevcdl_ctu_record> recs(ctus * n_frames);
  std::vector<hevcdl_sao_blk> sao(has_sao ? ctus * n_frames : 0);
  bool ok = fread(recs.data(), sizeof(hevcdl_ctu_record), recs.size(), f) == recs.size();
  if (has_sao) ok = ok && fread(sao.data(), sizeof(hevcdl_sao_blk), sao.size(), f) == sao.size();
  fclose(f);
  if (!ok) { printf("%s: short body\n", path); return 2; }
  int n_sub = 0; size_t pic_bytes = 0;
  if (hevcdl_slice_data_layout(&cfg, cpc, &n_sub, &pic_bytes, nullptr, nullptr) != HEVCDL_OK) { printf("%s: layout\n", path); return 2; }
  std::vector<uint32_t> off(n_sub), cap(n_sub), sizes((size_t)n_sub * n_frames), ovf((size_t)n_sub * n_frames);
  hevcdl_slice_data_layout(&cfg, cpc, &n_sub, &pic_bytes, off.data(), cap.data());
  std::vector<uint8_t> out(pic_bytes * n_frames, 0xA5);
  if (hevcdl_code_slice_data_host(&cfg, recs.data(), has_sao ? sao.data() : nullptr, n_frames, cpc, out.data(), out.size(), sizes.data(), ovf.data()) != HEVCDL_OK) { printf("%s: coder status\n", path); return 1; }
  for (int fr = 0; fr < n_frames; fr++) for (int k = 0; k < n_sub; k++) {
    const uint8_t *gap = out.data() + pic_bytes * fr + off[k] + cap[k];
    for (int i = 0; i < hevcdl_ec::EC_REGION_GAP; i++) if (gap[i] != 0xA5) { printf("%s: canary of sub-stream %d.%d\n", path, fr, k); return 1; }
    const uint32_t sz = sizes[(size_t)fr * n_sub + k], ov = ovf[(size_t)fr * n_sub + k];
    if ((sz > cap[k]) != (ov != 0)) { printf("%s: length %u capacity %u overflow %u\n", path, sz, cap[k], ov); return 1; }
  }
  { // every picture of every dump through hevcdl_write_access_unit, into an allocation of exactly the access unit's length (learnt from a first call, whose buffer is
    // too small on purpose); where no region overflowed above, the two ways to an access unit must agree
    std::vector<uint8_t> b((size_t)ctus * (hevcdl_ec::EC_DEFAULT_CAPACITY_PER_CTU + 128) * 2 + 65536), packed;
    for (int fr = 0; fr < n_frames; fr++) {
      const hevcdl_ctu_record *r = recs.data() + ctus * fr; const hevcdl_sao_blk *sp = has_sao ? sao.data() + ctus * fr : nullptr;
      size_t na = 0, nb = 0; uint8_t none = 0; bool fits = true;
      if (hevcdl_write_access_unit(&cfg, fr, r, sp, &none, 0, &na) != HEVCDL_ERR_INVALID_ARG || na == 0) { printf("%s: picture %d: no length from a call without room\n", path, fr); return 1; }
      std::vector<uint8_t> a(na);
      if (hevcdl_write_access_unit(&cfg, fr, r, sp, a.data(), a.size(), &nb) != HEVCDL_OK || nb != na) { printf("%s: picture %d: writer status\n", path, fr); return 1; }
      packed.clear();
      for (int k = 0; k < n_sub; k++) {
        const size_t i = (size_t)fr * n_sub + k; const uint8_t *p = out.data() + pic_bytes * fr + off[k];
        if (ovf[i]) { fits = false; break; }
        packed.insert(packed.end(), p, p + sizes[i]);
      }
      if (!fits) { if (mode == 0) { printf("%s: picture %d overflowed its region\n", path, fr); return 1; } continue; }
      packed.push_back(0);
      if (hevcdl_write_access_unit_from_slice_data(&cfg, fr, packed.data(), sizes.data() + (size_t)fr * n_sub, n_sub, b.data(), b.size(), &nb) != HEVCDL_OK) { printf("%s: picture %d: assembly status\n", path, fr); return 1; }
      if (na != nb || memcmp(a.data(), b.data(), na) != 0) { printf("%s: picture %d: hevcdl_write_access_unit differs from the assembled slice data\n", path, fr); return 1; }
    }
  }
  // the first picture of a single-sub-stream dump once more, into an allocation of exactly its capacity: a store past the region is a heap-buffer-overflow report
  {
    using namespace hevcdl_ec;
    const EcTables &t = ec_tables();
    if (!cfg.wavefront && n_sub == 1) { const int k = 0;
      std::vector<uint8_t> region(cap[k]); uint8_t ctx[EC_SYNC_BYTES]; uint16_t absb[16];
      EcCoder s; memset(&s, 0, sizeof s); s.t = &t; s.ctx = ctx; s.absb = absb; s.out = region.data(); s.cap = cap[k];
      EcPic p; p.recs = recs.data(); p.sao = has_sao ? sao.data() : nullptr; p.W = cfg.width; p.H = cfg.height; p.ctus_x = (p.W + 63) >> 6; p.ctus_y = (p.H + 63) >> 6; p.ctus = p.ctus_x * p.ctus_y;
      p.tools = cfg.tools; p.max_sao_offset = (1 << ((cfg.bit_depth < 10 ? cfg.bit_depth : 10) - 5)) - 1;
      p.tx0 = 0; p.ty0 = 0;
      ec_init_contexts(ctx, &t, cfg.qp);
      ec_code_substream(s, p, 0, p.ctus_x, 0, p.ctus_y);
      if (s.pos != sizes[k]) { printf("%s: second run differs\n", path); return 1; }
    }
  }
  return 0;
}

int main(int argc, char **argv)
{
  int bad = 0;
  for (int i = 1; i < argc; i++) bad += run(argv[i]) != 0;
  printf("entropy harness: %d dumps, %d failed\n", argc - 1, bad);
  return bad ? 1 : 0;
}
