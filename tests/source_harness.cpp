// source_harness.cpp -- csrc/source_core.h under AddressSanitizer / UndefinedBehaviorSanitizer on the CPU (tests/test_source.py builds and runs it; it is never loaded
// into Python and never runs on a GPU).
//
// For every size and depth case below the source picture, the coded picture and the output picture each sit in a heap block of exactly their size, so that a read or a
// write past either end is a sanitizer report.  load_pictures / store_pictures are compared with the reference's procedure restated here in its own order: pad the
// columns, then the rows, then scale the whole padded plane (TVideoIOYuv.cpp:363-381, 70-95); crop, then scale (:755-830).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "source_core.h"

static int scale_ref(int v, int from, int to)
{
  const int shift = to - from;
  if (shift > 0) return v << shift;
  if (shift < 0) { const int s = -shift, r = (v + (1 << (s - 1))) >> s, hi = (1 << to) - 1; return r < 0 ? 0 : (r > hi ? hi : r); }
  return v;
}

static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <typename T> static T *exact(size_t n) { T *p = (T *)malloc(n * sizeof(T)); if (!p) { printf("source harness: out of memory\n"); exit(2); } return p; }

// one case: source sw x sh at in_bd -> coded cw x ch at bd -> window at out_bd, n pictures
template <typename IN, typename PEL, typename OUT> static bool run_case(int sw, int sh, int cw, int ch, int in_bd, int bd, int out_bd, int n)
{
  using namespace hevcdl_src;
  const size_t ss = picture_samples(sw, sh), cs = picture_samples(cw, ch);
  IN *src = exact<IN>(ss * n); PEL *coded = exact<PEL>(cs * n); OUT *out = exact<OUT>(ss * n);
  const int top = (1 << in_bd) - 1;
  for (size_t i = 0; i < ss * n; i++) {                                  // both rails, the rounding midpoints of every down-shift, anything else
    const uint32_t r = rnd();
    int v = (int)(r % (uint32_t)(top + 1));
    if ((r >> 12) % 4 == 0) v = (r >> 14) & 1 ? top - (int)((r >> 15) % 4) : (int)((r >> 15) % 4);
    if ((r >> 12) % 4 == 1 && in_bd > bd) v = (v & ~((1 << (in_bd - bd)) - 1)) | (1 << (in_bd - bd - 1));
    src[i] = (IN)(v > top ? top : v);
  }
  load_pictures<IN, PEL>(src, sw, sh, coded, cw, ch, n, in_bd, bd);
  bool ok = true;
  for (int i = 0; i < n && ok; i++) for (int c = 0; c < 3 && ok; c++) {
    const int pw = plane_width(cw, c), ph = plane_height(ch, c), qw = plane_width(sw, c), qh = plane_height(sh, c);
    std::vector<int> pad((size_t)pw * ph);
    const IN *sp = src + ss * i + plane_offset(sw, sh, c);
    for (int y = 0; y < qh; y++) { for (int x = 0; x < qw; x++) pad[(size_t)y * pw + x] = sp[(size_t)y * qw + x]; for (int x = qw; x < pw; x++) pad[(size_t)y * pw + x] = pad[(size_t)y * pw + qw - 1]; }
    for (int y = qh; y < ph; y++) for (int x = 0; x < pw; x++) pad[(size_t)y * pw + x] = pad[(size_t)(y - 1) * pw + x];
    const PEL *cp = coded + cs * i + plane_offset(cw, ch, c);
    for (size_t k = 0; k < (size_t)pw * ph; k++) if ((int)cp[k] != scale_ref(pad[k], in_bd, bd)) { ok = false; break; }
  }
  if (!ok) printf("source harness: load differs for %dx%d -> %dx%d, %d -> %d bits\n", sw, sh, cw, ch, in_bd, bd);
  for (size_t i = 0; i < cs * n; i++) coded[i] = (PEL)(rnd() % (1u << bd));      // any coded picture: the store direction on its own
  store_pictures<PEL, OUT>(coded, cw, ch, out, sw, sh, n, bd, out_bd);
  bool ok2 = true;
  for (int i = 0; i < n && ok2; i++) for (int c = 0; c < 3 && ok2; c++) {
    const int pw = plane_width(cw, c), qw = plane_width(sw, c), qh = plane_height(sh, c);
    const PEL *cp = coded + cs * i + plane_offset(cw, ch, c);
    const OUT *op = out + ss * i + plane_offset(sw, sh, c);
    for (int y = 0; y < qh && ok2; y++) for (int x = 0; x < qw; x++) if ((int)op[(size_t)y * qw + x] != scale_ref(cp[(size_t)y * pw + x], bd, out_bd)) { ok2 = false; break; }
  }
  if (!ok2) printf("source harness: store differs for %dx%d <- %dx%d, %d -> %d bits\n", sw, sh, cw, ch, bd, out_bd);
  free(src); free(coded); free(out);
  return ok && ok2;
}

static bool dispatch(int sw, int sh, int cw, int ch, int in_bd, int bd, int out_bd, int n)
{
  const int k = (in_bd > 8 ? 4 : 0) | (bd > 8 ? 2 : 0) | (out_bd > 8 ? 1 : 0);
  switch (k) {
  case 0: return run_case<uint8_t, uint8_t, uint8_t>(sw, sh, cw, ch, in_bd, bd, out_bd, n);
  case 1: return run_case<uint8_t, uint8_t, uint16_t>(sw, sh, cw, ch, in_bd, bd, out_bd, n);
  case 2: return run_case<uint8_t, uint16_t, uint8_t>(sw, sh, cw, ch, in_bd, bd, out_bd, n);
  case 3: return run_case<uint8_t, uint16_t, uint16_t>(sw, sh, cw, ch, in_bd, bd, out_bd, n);
  case 4: return run_case<uint16_t, uint8_t, uint8_t>(sw, sh, cw, ch, in_bd, bd, out_bd, n);
  case 5: return run_case<uint16_t, uint8_t, uint16_t>(sw, sh, cw, ch, in_bd, bd, out_bd, n);
  case 6: return run_case<uint16_t, uint16_t, uint8_t>(sw, sh, cw, ch, in_bd, bd, out_bd, n);
  default: return run_case<uint16_t, uint16_t, uint16_t>(sw, sh, cw, ch, in_bd, bd, out_bd, n);
  }
}

int main()
{
  // source size -> coded size: no padding, ConformanceWindowMode 1, and a padding above 8 (rows of replicated rows)
  const int sizes[][4] = { { 2, 2, 2, 2 }, { 2, 2, 8, 8 }, { 6, 10, 8, 16 }, { 66, 42, 72, 48 }, { 70, 2, 72, 8 }, { 60, 60, 64, 72 }, { 64, 64, 64, 64 } };
  const int in_depths[] = { 8, 10, 12 }, depths[] = { 8, 10 };
  int cases = 0, failed = 0;
  for (const auto &s : sizes) for (int in_bd : in_depths) for (int bd : depths) for (int out_bd : in_depths) {
    cases++;
    if (!dispatch(s[0], s[1], s[2], s[3], in_bd, bd, out_bd, 2)) failed++;
  }
  printf("source harness: %d cases, %d failed\n", cases, failed);
  return failed ? 1 : 0;
}
