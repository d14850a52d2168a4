// source_format_harness.cpp -- the file-layout functions of csrc/source_core.h (4:0:0 / 4:2:2 / 4:4:4 files, swapped chroma planes, a window with an origin) under
// AddressSanitizer / UndefinedBehaviorSanitizer on the CPU (tests/test_source_formats.py builds and runs it; it is never loaded into Python and never runs on a GPU).
//
// The source picture, the coded picture and the output picture each sit in a heap block of exactly their size, so that a read or a write past either end -- an odd
// source row or column read by mistake, a window origin applied twice -- is a sanitizer report.  load_pictures_fmt / store_pictures_fmt are compared with a serial
// restatement in the reference's own order (TVideoIOYuv.cpp readPlane :249-384: read a file row, pick, replicate columns, then rows; write :811-826: offset, then rows).
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

static uint32_t rng_state = 2468;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <typename T> static T *exact(size_t n) { T *p = (T *)malloc(n ? n * sizeof(T) : 1); if (!p) { printf("source format harness: out of memory\n"); exit(2); } return p; }

static size_t file_samples(int sw, int sh, int f) { return (size_t)sw * sh + (f == 400 ? 0 : 2 * (size_t)(f == 444 ? sw : sw / 2) * (f == 420 ? sh / 2 : sh)); }

// one load case: a file of sw x sh in format f (Cr first when swap) at in_bd -> coded cw x ch at bd
template <typename IN, typename PEL> static bool load_case(int sw, int sh, int cw, int ch, int f, int swap, int in_bd, int bd, int n)
{
  using namespace hevcdl_src;
  const size_t ss = file_samples(sw, sh, f), cs = picture_samples(cw, ch);
  if (ss != picture_samples_fmt(sw, sh, f)) { printf("source format harness: picture_samples_fmt(%d, %d, %d)\n", sw, sh, f); return false; }
  IN *src = exact<IN>(ss * n); PEL *coded = exact<PEL>(cs * n);
  const int top = (1 << in_bd) - 1;
  for (size_t i = 0; i < ss * n; i++) { const uint32_t r = rnd(); int v = (int)(r % (uint32_t)(top + 1)); if ((r >> 12) % 4 == 0) v = (r >> 14) & 1 ? top - (int)((r >> 15) % 4) : (int)((r >> 15) % 4); src[i] = (IN)v; }
  load_pictures_fmt<IN, PEL>(src, sw, sh, f, swap, coded, cw, ch, n, in_bd, bd);
  bool ok = true;
  const int fw = f == 444 ? sw : sw / 2, fh = f == 420 ? sh / 2 : sh;      // the file's chroma plane
  for (int i = 0; i < n && ok; i++) for (int c = 0; c < 3 && ok; c++) {
    const int pw = c ? cw / 2 : cw, ph = c ? ch / 2 : ch, qw = c ? sw / 2 : sw, qh = c ? sh / 2 : sh;      // destination plane; the part of it the file covers
    std::vector<int> pad((size_t)pw * ph);
    if (c && f == 400) { for (auto &v : pad) v = 1 << (in_bd - 1); }
    else {
      const int fc = (c && swap) ? 3 - c : c, rw = c ? fw : sw, stepx = c ? fw / qw : 1, stepy = c ? fh / qh : 1;
      const IN *sp = src + ss * i + (fc == 0 ? 0 : (size_t)sw * sh + (fc == 2 ? (size_t)fw * fh : 0));
      for (int y = 0; y < qh; y++) {
        const IN *row = sp + (size_t)(y * stepy) * rw;                                          // read a file row
        for (int x = 0; x < qw; x++) pad[(size_t)y * pw + x] = row[x * stepx];                    // pick
        for (int x = qw; x < pw; x++) pad[(size_t)y * pw + x] = pad[(size_t)y * pw + qw - 1];     // replicate columns
      }
      for (int y = qh; y < ph; y++) for (int x = 0; x < pw; x++) pad[(size_t)y * pw + x] = pad[(size_t)(y - 1) * pw + x];      // replicate rows
    }
    const PEL *cp = coded + cs * i + plane_offset(cw, ch, c);
    for (size_t k = 0; k < (size_t)pw * ph; k++) if ((int)cp[k] != scale_ref(pad[k], in_bd, bd)) { ok = false; break; }
  }
  if (!ok) printf("source format harness: load differs for %dx%d (%d%s) -> %dx%d, %d -> %d bits\n", sw, sh, f, swap ? ", swapped" : "", cw, ch, in_bd, bd);
  free(src); free(coded);
  return ok;
}

// one store case: the window (l, r, t, b) of a coded cw x ch picture at bd -> output at out_bd
template <typename PEL, typename OUT> static bool store_case(int cw, int ch, int l, int r, int t, int b, int swap, int bd, int out_bd, int n)
{
  using namespace hevcdl_src;
  if (!window_fits(cw, ch, l, r, t, b)) { printf("source format harness: window_fits\n"); return false; }
  const int ww = cw - l - r, wh = ch - t - b;
  const size_t cs = picture_samples(cw, ch), ws = picture_samples(ww, wh);
  PEL *coded = exact<PEL>(cs * n); OUT *out = exact<OUT>(ws * n);
  for (size_t i = 0; i < cs * n; i++) coded[i] = (PEL)(rnd() % (1u << bd));
  store_pictures_fmt<PEL, OUT>(coded, cw, ch, out, ww, wh, l, t, swap, n, bd, out_bd);
  bool ok = true;
  for (int i = 0; i < n && ok; i++) for (int c = 0; c < 3 && ok; c++) {
    const int cs_ = c ? 1 : 0, pw = cw >> cs_, qw = ww >> cs_, qh = wh >> cs_, sc = (c && swap) ? 3 - c : c;
    const PEL *cp = coded + cs * i + plane_offset(cw, ch, sc) + (size_t)(l >> cs_) + (size_t)(t >> cs_) * pw;      // write :811-826
    const OUT *op = out + ws * i + plane_offset(ww, wh, c);
    for (int y = 0; y < qh && ok; y++) for (int x = 0; x < qw; x++) if ((int)op[(size_t)y * qw + x] != scale_ref(cp[(size_t)y * pw + x], bd, out_bd)) { ok = false; break; }
  }
  if (!ok) printf("source format harness: store differs for window (%d, %d, %d, %d) of %dx%d%s, %d -> %d bits\n", l, r, t, b, cw, ch, swap ? ", swapped" : "", bd, out_bd);
  free(coded); free(out);
  return ok;
}

static bool load_dispatch(int sw, int sh, int cw, int ch, int f, int swap, int in_bd, int bd, int n)
{
  if (in_bd > 8) return bd > 8 ? load_case<uint16_t, uint16_t>(sw, sh, cw, ch, f, swap, in_bd, bd, n) : load_case<uint16_t, uint8_t>(sw, sh, cw, ch, f, swap, in_bd, bd, n);
  return bd > 8 ? load_case<uint8_t, uint16_t>(sw, sh, cw, ch, f, swap, in_bd, bd, n) : load_case<uint8_t, uint8_t>(sw, sh, cw, ch, f, swap, in_bd, bd, n);
}
static bool store_dispatch(int cw, int ch, const int *w, int swap, int bd, int out_bd, int n)
{
  if (bd > 8) return out_bd > 8 ? store_case<uint16_t, uint16_t>(cw, ch, w[0], w[1], w[2], w[3], swap, bd, out_bd, n) : store_case<uint16_t, uint8_t>(cw, ch, w[0], w[1], w[2], w[3], swap, bd, out_bd, n);
  return out_bd > 8 ? store_case<uint8_t, uint16_t>(cw, ch, w[0], w[1], w[2], w[3], swap, bd, out_bd, n) : store_case<uint8_t, uint8_t>(cw, ch, w[0], w[1], w[2], w[3], swap, bd, out_bd, n);
}

int main()
{
  // source size -> coded size: the smallest picture (coded chroma 4 x 4), odd chroma widths (5, 33), no padding, ConformanceWindowMode 1, a padding above 8
  const int sizes[][4] = { { 8, 8, 8, 8 }, { 2, 2, 8, 8 }, { 10, 8, 16, 8 }, { 6, 10, 8, 16 }, { 66, 42, 72, 48 }, { 70, 2, 72, 8 }, { 60, 60, 64, 72 }, { 64, 64, 64, 64 } };
  const int formats[] = { 400, 420, 422, 444 }, in_depths[] = { 8, 10, 16 }, depths[] = { 8, 10 };
  int cases = 0, failed = 0;
  for (const auto &s : sizes) for (int f : formats) for (int swap = 0; swap < (f == 400 ? 1 : 2); swap++) for (int in_bd : in_depths) for (int bd : depths) {
    cases++;
    if (!load_dispatch(s[0], s[1], s[2], s[3], f, swap, in_bd, bd, 2)) failed++;
  }
  // windows: none, the issue's three on 72 x 40 (one two samples wide), one row high, the smallest picture
  const int windows[][6] = { { 72, 40, 0, 0, 0, 0 }, { 72, 40, 2, 0, 0, 2 }, { 72, 40, 4, 2, 6, 8 }, { 72, 40, 62, 0, 0, 38 }, { 72, 40, 0, 70, 38, 0 }, { 8, 8, 2, 2, 2, 2 }, { 8, 8, 6, 0, 0, 6 } };
  for (const auto &w : windows) for (int swap = 0; swap < 2; swap++) for (int bd : depths) for (int out_bd : in_depths) {
    cases++;
    if (!store_dispatch(w[0], w[1], w + 2, swap, bd, out_bd, 2)) failed++;
  }
  printf("source format harness: %d cases, %d failed\n", cases, failed);
  return failed ? 1 : 0;
}
