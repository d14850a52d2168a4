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
//
// The FILE's layout (the coded picture stays 4:2:0, Y Cb Cr): a source picture may be 4:0:0, 4:2:2 or 4:4:4, may store Cr before Cb, and the output may be a window with
// an explicit origin (ConformanceWindowMode 3).  All of it is one description per plane, `plane_ref` -- where the plane starts in the packed picture, its row pitch, a
// horizontal and a vertical source step of 1 or 2 (as shifts), the clamp limits in DESTINATION coordinates, or "constant" -- and one row function over it:
//   coded_c(x, y) = scale(file_c(min(x, sw/2 - 1) << (1 - csx), min(y, sh/2 - 1) << (1 - csy)))      csx, csy = 1, 1 (4:2:0); 1, 0 (4:2:2); 0, 0 (4:4:4)
// readPlane :249-384 reads a file row, keeps every (1 << shift)-th sample of it, replicates the last KEPT sample into the padding columns and the last kept row into the
// padding rows: the nearest (top-left) sample, no filter, and the clamp acts on the destination coordinate (a padded 4:4:4 file replicates file column sw - 2, not sw - 1).
// A 4:0:0 file has no chroma planes: both coded chroma planes are scale(1 << (input depth - 1)) (:280-293, then scalePlane).  With YCbCrtoYCrCb (ColourSpaceConvert
// :981-1041) coded plane 1 is the file's plane 2 and the other way round; the output file gets them back in the file's order unless the caller keeps the internal one.
// A window with an origin: output_c(x, y) = scale(coded_c(x + (left >> cs), y + (top >> cs))) (write :811-826), cs = 1 for chroma.
// load_row / store_row / load_pictures / store_pictures below are the 4:2:0, unpermuted, origin-less forms and stay what they were; the *_fmt functions hold the rest.
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

// ---- the file's layout: chroma format, plane order, window origin -----------------------------------------------------------------------------------------------------
enum { FMT_400 = 400, FMT_420 = 420, FMT_422 = 422, FMT_444 = 444 };

SRC_FN int chroma_format_id(int f) { return f == 0 ? FMT_420 : f; }      // 0 = 4:2:0 (the ABI's default)
SRC_FN bool chroma_format_known(int f) { return f == 0 || f == FMT_400 || f == FMT_420 || f == FMT_422 || f == FMT_444; }
// log2 of the luma : chroma ratio of a file format, horizontally and vertically
SRC_FN int chroma_shift_x(int f) { return chroma_format_id(f) == FMT_444 ? 0 : 1; }
SRC_FN int chroma_shift_y(int f) { return chroma_format_id(f) == FMT_420 ? 1 : 0; }
// samples of one packed picture of w x h luma samples in file format f: Y, then both chroma planes at the file's own chroma size (4:0:0: none)
SRC_FN size_t chroma_plane_samples(int w, int h, int f) { return chroma_format_id(f) == FMT_400 ? 0 : (size_t)(w >> chroma_shift_x(f)) * (h >> chroma_shift_y(f)); }
SRC_FN size_t picture_samples_fmt(int w, int h, int f) { return (size_t)w * h + 2 * chroma_plane_samples(w, h, f); }

// a window inside a coded picture: even offsets, something left of the picture
SRC_FN bool window_fits(int w, int h, int left, int right, int top, int bottom)
{
  return left >= 0 && right >= 0 && top >= 0 && bottom >= 0 && !((left | right | top | bottom) & 1) && (long long)left + right < w && (long long)top + bottom < h;
}

// where one destination plane takes its samples from
struct plane_ref {
  size_t offset;          // first sample read (the window's origin included), from the picture's first sample
  int pitch;              // samples between two source rows
  int lim_w, lim_h;       // the clamp: destination column x reads min(x, lim_w - 1) << sx, row y reads min(y, lim_h - 1) << sy
  int sx, sy;             // source step as a shift: 0 (every sample) or 1 (every second sample / row: the even ones)
  int constant;           // 1: no source plane; every sample is `value` (at the source's depth)
  int32_t value;
};

// coded plane c (0 Y, 1 Cb, 2 Cr) of a 4:2:0 picture from a file picture of sw x sh luma samples in format f; swap: the file stores Cr before Cb
SRC_FN plane_ref load_plane_ref(int sw, int sh, int f, int swap, int c, int in_depth)
{
  plane_ref r; r.offset = 0; r.pitch = sw; r.lim_w = sw; r.lim_h = sh; r.sx = r.sy = 0; r.constant = 0; r.value = 0;
  if (c == 0) return r;
  r.lim_w = sw >> 1; r.lim_h = sh >> 1;
  if (chroma_format_id(f) == FMT_400) { r.constant = 1; r.value = (int32_t)1 << (in_depth - 1); r.pitch = 0; return r; }
  const int fc = swap ? 3 - c : c;
  r.pitch = sw >> chroma_shift_x(f); r.sx = 1 - chroma_shift_x(f); r.sy = 1 - chroma_shift_y(f);
  r.offset = (size_t)sw * sh + (fc == 2 ? chroma_plane_samples(sw, sh, f) : 0);
  return r;
}
// output plane c of a window of ww x wh luma samples at (left, top) of a coded 4:2:0 picture of cw x ch; swap: the output stores coded plane 2 before coded plane 1
SRC_FN plane_ref store_plane_ref(int cw, int ch, int ww, int wh, int left, int top, int swap, int c)
{
  const int sc = (c && swap) ? 3 - c : c, cs = c ? 1 : 0;
  plane_ref r; r.pitch = plane_width(cw, c); r.lim_w = plane_width(ww, c); r.lim_h = plane_height(wh, c); r.sx = r.sy = 0; r.constant = 0; r.value = 0;
  r.offset = plane_offset(cw, ch, sc) + (size_t)(top >> cs) * r.pitch + (size_t)(left >> cs);
  return r;
}

// columns [x0, x1) of row y of one destination plane (dw wide) from the plane `r` describes inside the picture at `pic`
template <typename S, typename D>
SRC_FN void convert_row_fmt(const S *pic, const plane_ref &r, D *dst, int dw, int y, int x0, int x1, int from_depth, int to_depth)
{
  D *d = dst + (size_t)y * dw;
  if (r.constant) { const D v = (D)scale_sample(r.value, from_depth, to_depth); for (int x = x0; x < x1; x++) d[x] = v; return; }
  const S *s = pic + r.offset + ((size_t)(y < r.lim_h ? y : r.lim_h - 1) << r.sy) * r.pitch;
  for (int x = x0; x < x1; x++) d[x] = (D)scale_sample((int32_t)s[(size_t)(x < r.lim_w ? x : r.lim_w - 1) << r.sx], from_depth, to_depth);
}

// whole pictures, serially
template <typename IN, typename PEL>
SRC_FN void load_pictures_fmt(const IN *src, int sw, int sh, int f, int swap, PEL *dst, int cw, int ch, int n, int in_depth, int internal_depth)
{
  const size_t ss = picture_samples_fmt(sw, sh, f), cs = picture_samples(cw, ch);
  for (int i = 0; i < n; i++) for (int c = 0; c < 3; c++) {
    const plane_ref r = load_plane_ref(sw, sh, f, swap, c, in_depth);
    PEL *dp = dst + cs * i + plane_offset(cw, ch, c);
    const int pw = plane_width(cw, c), ph = plane_height(ch, c);
    for (int y = 0; y < ph; y++) convert_row_fmt<IN, PEL>(src + ss * i, r, dp, pw, y, 0, pw, in_depth, internal_depth);
  }
}
template <typename PEL, typename OUT>
SRC_FN void store_pictures_fmt(const PEL *coded, int cw, int ch, OUT *dst, int ww, int wh, int left, int top, int swap, int n, int internal_depth, int out_depth)
{
  const size_t cs = picture_samples(cw, ch), ws = picture_samples(ww, wh);
  for (int i = 0; i < n; i++) for (int c = 0; c < 3; c++) {
    const plane_ref r = store_plane_ref(cw, ch, ww, wh, left, top, swap, c);
    OUT *dp = dst + ws * i + plane_offset(ww, wh, c);
    const int pw = plane_width(ww, c), ph = plane_height(wh, c);
    for (int y = 0; y < ph; y++) convert_row_fmt<PEL, OUT>(coded + cs * i, r, dp, pw, y, 0, pw, internal_depth, out_depth);
  }
}

}  // namespace hevcdl_src
#endif
