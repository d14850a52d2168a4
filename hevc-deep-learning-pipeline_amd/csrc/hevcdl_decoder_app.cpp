// hevcdl_decoder_app.cpp -- bin/TAppDecoderHevcdl: the command-line decoder over the C ABI, with the reference decoder's option names.
//   TAppDecoderHevcdl -b str.bin [-o rec.yuv] [-d depth] [--device n] [--batch n] [--DeviceParse 0|1]
// -b the stream, -o the reconstruction file (the conformance window of every picture, planar 4:2:0), -d the file's bit depth (0, the default: the stream's own; samples
// above 8 bits are two bytes, little endian; converted as the reference's file writer does: up by a left shift, down by a rounding right shift and a clip).  One line per
// picture: POC, QP and the verdict of the decoded picture hash -- the device's digest against the stream's SEI.  Exit status: 0; 1 when a digest does not match; 2 for
// anything else (options, the file, a stream the decoder refuses: its sentence is printed).  --DeviceParse 1: the slice data is decoded on the device
// (hevcdl_enable_device_parse); the pictures, the lines and the exit status are the same.
// Host C++: the stream is parsed and the pictures are rebuilt by hevcdl_decode_stream; nothing here touches a sample but the window and the depth of the file.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "hevcdl.h"

static void write_plane(FILE *f, const unsigned char *pic, size_t plane_off, int stride, int x0, int y0, int w, int h, int bd, int out_bd)
{
  std::vector<unsigned char> row((size_t)w * (out_bd > 8 ? 2 : 1));
  for (int y = 0; y < h; y++) {
    for (int x = 0; x < w; x++) {
      const size_t i = plane_off + (size_t)(y0 + y) * stride + (size_t)(x0 + x);
      int v = bd > 8 ? (int)((const uint16_t *)pic)[i] : (int)pic[i];
      if (out_bd > bd) v <<= out_bd - bd;
      else if (out_bd < bd) { v = (v + (1 << (bd - out_bd - 1))) >> (bd - out_bd); const int mx = (1 << out_bd) - 1; if (v > mx) v = mx; }
      if (out_bd > 8) { row[2 * (size_t)x] = (unsigned char)(v & 255); row[2 * (size_t)x + 1] = (unsigned char)(v >> 8); } else row[(size_t)x] = (unsigned char)v;
    }
    fwrite(row.data(), 1, row.size(), f);
  }
}

int main(int argc, char **argv)
{
  std::string in, out;
  int depth = 0, device = 0, batch = 64, device_parse = 0;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto value = [&](const char *name) -> const char * { if (i + 1 >= argc) { fprintf(stderr, "Error: %s needs a value\n", name); exit(2); } return argv[++i]; };
    if (a == "-b" || a == "--BitstreamFile") in = value("-b");
    else if (a == "-o" || a == "--ReconFile") out = value("-o");
    else if (a == "-d" || a == "--OutputBitDepth") depth = atoi(value("-d"));
    else if (a == "--device") device = atoi(value("--device"));
    else if (a == "--batch") batch = atoi(value("--batch"));
    else if (a == "--DeviceParse") device_parse = atoi(value("--DeviceParse"));
    else { fprintf(stderr, "Error: unknown option '%s'\nusage: TAppDecoderHevcdl -b str.bin [-o rec.yuv] [-d depth] [--device n] [--batch n] [--DeviceParse 0|1]\n", a.c_str()); return 2; }
  }
  if (in.empty()) { fprintf(stderr, "Error: no bitstream file (-b)\n"); return 2; }
  if (depth != 0 && (depth < 8 || depth > 16)) { fprintf(stderr, "Error: -d is 0 or 8 .. 16\n"); return 2; }
  if (batch < 1) batch = 1;
  std::vector<uint8_t> stream;
  {
    FILE *f = fopen(in.c_str(), "rb");
    if (!f) { fprintf(stderr, "Error: cannot open '%s'\n", in.c_str()); return 2; }
    unsigned char buf[1 << 16]; size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) stream.insert(stream.end(), buf, buf + got);
    fclose(f);
  }
  hevcdl_stream_config sc; memset(&sc, 0, sizeof sc); sc.struct_size = sizeof sc;
  hevcdl_slice_layout sl = { 0, 0, 1 }; hevcdl_segment_layout sg = { 0, 0 };
  int n = 0;
  // a QP per CU, PPS chroma QP offsets and scaling lists are always accepted here (hevcdl_enable_cu_qp, hevcdl_enable_scaling_lists below); the picture line shows the slice QP
  hevcdl_status st = hevcdl_parse_stream_sl(stream.data(), stream.size(), HEVCDL_ACCEPT_CU_QP | HEVCDL_ACCEPT_SCALING_LISTS, &sc, &sl, &sg, nullptr, 0, &n, nullptr, nullptr, 0, nullptr, nullptr, nullptr);
  if (st != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_parse_error(), (int)st); return 2; }
  hevcdl_config cfg;
  if (hevcdl_config_from_stream(&sc, &sl, n < batch ? n : batch, device, &cfg) != HEVCDL_OK) { fprintf(stderr, "Error: no context configuration for this stream\n"); return 2; }
  std::vector<float> weights(HEVCDL_WEIGHT_FLOATS, 0.0f);      // the label CNN does not run in a decoder: a context wants a blob of the right size, its values are never read
  hevcdl_ctx *ctx = nullptr;
  st = hevcdl_create(&cfg, weights.data(), weights.size(), &ctx);
  if (st != HEVCDL_OK) { fprintf(stderr, "Error: hevcdl_create: status %d %s\n", (int)st, hevcdl_create_error()); return 2; }
  if ((st = hevcdl_enable_cu_qp(ctx, 1)) != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(ctx), (int)st); hevcdl_destroy(ctx); return 2; }
  if ((st = hevcdl_enable_scaling_lists(ctx, 1)) != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(ctx), (int)st); hevcdl_destroy(ctx); return 2; }
  if (device_parse && (st = hevcdl_enable_device_parse(ctx, 1)) != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(ctx), (int)st); hevcdl_destroy(ctx); return 2; }
  const size_t fb = hevcdl_frame_bytes_bd(sc.width, sc.height, sc.bit_depth);
  std::vector<unsigned char> pictures(fb * (size_t)n);
  std::vector<hevcdl_parsed_picture> info((size_t)n); std::vector<int32_t> ok((size_t)n);
  st = hevcdl_decode_stream(ctx, stream.data(), stream.size(), pictures.data(), n, &n, info.data(), ok.data());
  if (st != HEVCDL_OK) { fprintf(stderr, "Error: %s (status %d)\n", hevcdl_last_error(ctx), (int)st); hevcdl_destroy(ctx); return 2; }
  hevcdl_destroy(ctx);
  const int out_bd = depth ? depth : sc.bit_depth;
  FILE *fo = nullptr;
  if (!out.empty() && !(fo = fopen(out.c_str(), "wb"))) { fprintf(stderr, "Error: cannot write '%s'\n", out.c_str()); return 2; }
  static const char *const names[4] = { "", "MD5", "CRC", "Checksum" };
  int mismatches = 0;
  const int w = sc.width, h = sc.height, ww = w - sc.conf_win_left - sc.conf_win_right, wh = h - sc.conf_win_top - sc.conf_win_bottom;
  for (int i = 0; i < n; i++) {
    const hevcdl_parsed_picture &p = info[(size_t)i];
    printf("POC %4d ( I-SLICE, QP %2d ) ", p.nal_type == 21 ? p.poc : 0, p.qp);
    if (ok[(size_t)i] < 0) printf("[no decoded picture hash]\n");
    else {
      printf("[%s:", names[p.hash_method & 3]);
      for (int k = 0; k < 3 * p.hash_plane_bytes; k++) printf("%s%02x", k && k % p.hash_plane_bytes == 0 ? "," : "", p.digest[k]);
      printf(",(%s)]\n", ok[(size_t)i] ? "OK" : "***ERROR***");
      mismatches += !ok[(size_t)i];
    }
    if (fo) {
      const unsigned char *pic = pictures.data() + (size_t)i * fb;
      const size_t ysz = (size_t)w * h;
      write_plane(fo, pic, 0, w, sc.conf_win_left, sc.conf_win_top, ww, wh, sc.bit_depth, out_bd);
      write_plane(fo, pic, ysz, w / 2, sc.conf_win_left / 2, sc.conf_win_top / 2, ww / 2, wh / 2, sc.bit_depth, out_bd);
      write_plane(fo, pic, ysz + ysz / 4, w / 2, sc.conf_win_left / 2, sc.conf_win_top / 2, ww / 2, wh / 2, sc.bit_depth, out_bd);
    }
  }
  if (fo) fclose(fo);
  printf("%d pictures decoded, %d hash mismatches\n", n, mismatches);
  return mismatches ? 1 : 0;
}
