// source_core.h -- source pictures of any (even) size and bit depth <-> the codec's own format, as ONE source for the host and the device.
//
// Plain inline functions over raw pointers: what the reference does at its file boundary (TVideoIOYuv.cpp: readPlane :363-381 extends the right and lower edges,
// scalePlane :70-95 changes the bit depth, write :755-830 crops to the conformance window and scales to the output depth), restated per sample so that a plane can be
// split over threads: hevcdl_source_load_kernel / hevcdl_source_store_kernel (source_kernel.hip) and hevcdl_load_source_host / hevcdl_store_output_host (hevcdl_bitstream.cpp)
// are the two instantiations.
//
// A picture is three planes (Y, Cb, Cr; 4:2:0) back to back, each row-major without a pitch; samples of a depth above 8 bits are two bytes, little endian.
//   source format   planes of source_width x source_height (chroma: halved), input_bit_depth
//   coded format    planes of width x height (the context's size, multiples of 8), the context's bit depth
//   output format   planes of the window = the coded picture minus the right and lower padding = the source size, output_bit_depth
// Load: coded(x, y) = scale(source(min(x, sw - 1), min(y, sh - 1)), input -> internal).  The reference pads first (a column past the source width takes the row's last
// source sample, then a row past the source height takes the row above over the full padded width) and scales afterwards; scaling is a per-sample map, so the order does
// not matter, and replicating rows of replicated columns is the clamp of both coordinates: the one expression above gives the reference's values.
// Store: output(x, y) = scale(coded(x, y), internal -> output) for (x, y) inside the window.
// Construction rules (as picture_hash_core.h): no allocation, no std:: containers, no inline assembly; every loop bound is an argument.
#ifndef HEVCDL_SOURCE_CORE_H
#define HEVCDL_SOURCE_CORE_H
#include <stddef.h>
#include <stdint.h>

#ifndef SRC_FN
#ifdef __HIPCC__
#define SRC_FN __host__ __device__ inline
#else
#define SRC_FN inline
#endif
#endif

namespace hevcdl_src {

// scalePlane for one sample (no Rec.709 clip): up by a left shift; down by a rounding right shift clipped to the target depth; equal depths copy
SRC_FN int32_t scale_sample(int32_t v, int from_depth, int to_depth)
{
  const int shift = to_depth - from_depth;
  if (shift > 0) return v << shift;
  if (shift < 0) {
    const int s = -shift;
    const int32_t r = (v + (1 << (s - 1))) >> s, hi = (1 << to_depth) - 1;
    return r < 0 ? 0 : (r > hi ? hi : r);
  }
  return v;
}

// a source format against a coded size: even source size of at least 2, padding (coded - source) non-negative and even, depths 8 .. 16
SRC_FN bool format_fits(int sw, int sh, int in_depth, int out_depth, int cw, int ch)
{
  return sw >= 2 && sh >= 2 && !(sw & 1) && !(sh & 1) && cw >= sw && ch >= sh && !((cw - sw) & 1) && !((ch - sh) & 1) && in_depth >= 8 && in_depth <= 16 && out_depth >= 8 && out_depth <= 16;
}

// plane c (0 Y, 1 Cb, 2 Cr) of a 4:2:0 picture of w x h luma samples: its size and its first sample in the packed picture
SRC_FN int plane_width(int w, int c) { return c ? w >> 1 : w; }
SRC_FN int plane_height(int h, int c) { return c ? h >> 1 : h; }
SRC_FN size_t plane_offset(int w, int h, int c) { return c == 0 ? 0 : (size_t)w * h + (c == 2 ? (size_t)(w >> 1) * (h >> 1) : 0); }
SRC_FN size_t picture_samples(int w, int h) { return (size_t)w * h + 2 * ((size_t)(w >> 1) * (h >> 1)); }

// columns [x0, x1) of row y of one coded plane (cw wide) from a source plane of sw x sh samples
template <typename IN, typename PEL>
SRC_FN void load_row(const IN *src, int sw, int sh, PEL *dst, int cw, int y, int x0, int x1, int in_depth, int internal_depth)
{
  const IN *s = src + (size_t)(y < sh ? y : sh - 1) * sw;
  PEL *d = dst + (size_t)y * cw;
  for (int x = x0; x < x1; x++) d[x] = (PEL)scale_sample((int32_t)s[x < sw ? x : sw - 1], in_depth, internal_depth);
}

// columns [x0, x1) of row y of one window plane (ww wide) from the coded plane (cw wide)
template <typename PEL, typename OUT>
SRC_FN void store_row(const PEL *coded, int cw, OUT *dst, int ww, int y, int x0, int x1, int internal_depth, int out_depth)
{
  const PEL *s = coded + (size_t)y * cw;
  OUT *d = dst + (size_t)y * ww;
  for (int x = x0; x < x1; x++) d[x] = (OUT)scale_sample((int32_t)s[x], internal_depth, out_depth);
}

// whole pictures, serially: the host's form
template <typename IN, typename PEL>
SRC_FN void load_pictures(const IN *src, int sw, int sh, PEL *dst, int cw, int ch, int n, int in_depth, int internal_depth)
{
  const size_t ss = picture_samples(sw, sh), cs = picture_samples(cw, ch);
  for (int i = 0; i < n; i++) for (int c = 0; c < 3; c++) {
    const IN *sp = src + ss * i + plane_offset(sw, sh, c);
    PEL *dp = dst + cs * i + plane_offset(cw, ch, c);
    const int pw = plane_width(cw, c), ph = plane_height(ch, c);
    for (int y = 0; y < ph; y++) load_row<IN, PEL>(sp, plane_width(sw, c), plane_height(sh, c), dp, pw, y, 0, pw, in_depth, internal_depth);
  }
}
template <typename PEL, typename OUT>
SRC_FN void store_pictures(const PEL *coded, int cw, int ch, OUT *dst, int ww, int wh, int n, int internal_depth, int out_depth)
{
  const size_t cs = picture_samples(cw, ch), ws = picture_samples(ww, wh);
  for (int i = 0; i < n; i++) for (int c = 0; c < 3; c++) {
    const PEL *sp = coded + cs * i + plane_offset(cw, ch, c);
    OUT *dp = dst + ws * i + plane_offset(ww, wh, c);
    const int pw = plane_width(ww, c), ph = plane_height(wh, c);
    for (int y = 0; y < ph; y++) store_row<PEL, OUT>(sp, plane_width(cw, c), dp, pw, y, 0, pw, internal_depth, out_depth);
  }
}

}  // namespace hevcdl_src
#endif
