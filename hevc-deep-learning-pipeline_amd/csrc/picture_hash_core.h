// picture_hash_core.h -- the three decoded-picture hashes (SEIDecodedPictureHash 1 MD5, 2 CRC, 3 checksum) as ONE source for the host and the device.
//
// Plain inline functions over raw pointers and POD state: what hevcdl_picture_hash (hevcdl_bitstream.cpp; the reference: TComPicYuvMD5.cpp:88-180) computes serially,
// restated so that a plane can be split over threads: hevcdl_report_*_kernel (report_kernel.hip) and hevcdl_plane_hash_host (hevcdl_bitstream.cpp) are the two
// instantiations.  hevcdl_picture_hash stays the independent yardstick: tests/test_report.py holds the two against each other, and against hashlib.
//
// A plane is hashed as the bytes of its samples in raster order, low byte first: one byte a sample at 8 bits, two above -- on a little-endian machine the plane as it lies
// in memory.  Everything here is exact integer arithmetic; nothing depends on how a plane was split.
//   MD5        one serial chain per plane (md5_block / md5_tail); RFC 1321.
//   CRC        the reference's bit-serial loop, crc = ((crc << 1) + bit) ^ (msb ? 0x1021 : 0) from 0xffff over the n message bits and 16 zero bits behind them, is
//              linear over GF(2):  digest = (0xffff x^n + M(x)) x^16 mod P,  P = x^16 + x^12 + x^5 + 1 (0x11021).
//              A plane is cut into chunks; chunk k's partial is M_k(x) mod P (the same loop from 0, no flush: leading zero bits do not change it), and
//              M(x) mod P = xor_k partial_k x^(bits behind chunk k) mod P.  x^m mod P by square-and-multiply over a 16-bit carry-less multiplication (crc_mulmod).
//   checksum   sum mod 2^32 of (byte ^ mask(x, y)) & 0xff over every byte of every sample, mask = (x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8); the high byte of a
//              sample above 8 bits takes the same mask.  A chunk's partial is the sum over its bytes; the fold is a 32-bit sum.
// Construction rules (as entropy_coder.h): no allocation, no std:: containers, no function pointers, no inline assembly; every loop bound is an argument.
#ifndef HEVCDL_PICTURE_HASH_CORE_H
#define HEVCDL_PICTURE_HASH_CORE_H
#include <stddef.h>
#include <stdint.h>

#ifndef PH_FN
#ifdef __HIPCC__
#define PH_FN __host__ __device__ inline
#else
#define PH_FN inline
#endif
#endif

#define HEVCDL_REPORT_CHUNK_BYTES 16384      // default chunk of the CRC / checksum partials: a multiple of 16; 507 chunks in a 2160p luma plane of 8-bit samples

namespace hevcdl_ph {

enum { PH_PIECE = 16 };                    // bytes a device lane reads at a time

// ---- MD5 ---------------------------------------------------------------------------------------------------------------------------------
struct Md5State { uint32_t a, b, c, d; };

PH_FN void md5_init(Md5State *s) { s->a = 0x67452301u; s->b = 0xefcdab89u; s->c = 0x98badcfeu; s->d = 0x10325476u; }

PH_FN uint32_t md5_rotl(uint32_t v, int n) { return (v << n) | (v >> (32 - n)); }

#define PH_MD5_STEP(f, a, b, c, d, x, t, s) (a) += f((b), (c), (d)) + (x) + (uint32_t)(t); (a) = md5_rotl((a), (s)); (a) += (b);
#define PH_MD5_F(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define PH_MD5_G(x, y, z) ((y) ^ ((z) & ((x) ^ (y))))
#define PH_MD5_H(x, y, z) ((x) ^ (y) ^ (z))
#define PH_MD5_I(x, y, z) ((y) ^ ((x) | ~(z)))

// one 64-byte block, given as its sixteen little-endian words
PH_FN void md5_block(Md5State *s, const uint32_t w[16])
{
  uint32_t a = s->a, b = s->b, c = s->c, d = s->d;
  PH_MD5_STEP(PH_MD5_F, a, b, c, d, w[0], 0xd76aa478u, 7)   PH_MD5_STEP(PH_MD5_F, d, a, b, c, w[1], 0xe8c7b756u, 12)
  PH_MD5_STEP(PH_MD5_F, c, d, a, b, w[2], 0x242070dbu, 17)  PH_MD5_STEP(PH_MD5_F, b, c, d, a, w[3], 0xc1bdceeeu, 22)
  PH_MD5_STEP(PH_MD5_F, a, b, c, d, w[4], 0xf57c0fafu, 7)   PH_MD5_STEP(PH_MD5_F, d, a, b, c, w[5], 0x4787c62au, 12)
  PH_MD5_STEP(PH_MD5_F, c, d, a, b, w[6], 0xa8304613u, 17)  PH_MD5_STEP(PH_MD5_F, b, c, d, a, w[7], 0xfd469501u, 22)
  PH_MD5_STEP(PH_MD5_F, a, b, c, d, w[8], 0x698098d8u, 7)   PH_MD5_STEP(PH_MD5_F, d, a, b, c, w[9], 0x8b44f7afu, 12)
  PH_MD5_STEP(PH_MD5_F, c, d, a, b, w[10], 0xffff5bb1u, 17) PH_MD5_STEP(PH_MD5_F, b, c, d, a, w[11], 0x895cd7beu, 22)
  PH_MD5_STEP(PH_MD5_F, a, b, c, d, w[12], 0x6b901122u, 7)  PH_MD5_STEP(PH_MD5_F, d, a, b, c, w[13], 0xfd987193u, 12)
  PH_MD5_STEP(PH_MD5_F, c, d, a, b, w[14], 0xa679438eu, 17) PH_MD5_STEP(PH_MD5_F, b, c, d, a, w[15], 0x49b40821u, 22)
  PH_MD5_STEP(PH_MD5_G, a, b, c, d, w[1], 0xf61e2562u, 5)   PH_MD5_STEP(PH_MD5_G, d, a, b, c, w[6], 0xc040b340u, 9)
  PH_MD5_STEP(PH_MD5_G, c, d, a, b, w[11], 0x265e5a51u, 14) PH_MD5_STEP(PH_MD5_G, b, c, d, a, w[0], 0xe9b6c7aau, 20)
  PH_MD5_STEP(PH_MD5_G, a, b, c, d, w[5], 0xd62f105du, 5)   PH_MD5_STEP(PH_MD5_G, d, a, b, c, w[10], 0x02441453u, 9)
  PH_MD5_STEP(PH_MD5_G, c, d, a, b, w[15], 0xd8a1e681u, 14) PH_MD5_STEP(PH_MD5_G, b, c, d, a, w[4], 0xe7d3fbc8u, 20)
  PH_MD5_STEP(PH_MD5_G, a, b, c, d, w[9], 0x21e1cde6u, 5)   PH_MD5_STEP(PH_MD5_G, d, a, b, c, w[14], 0xc33707d6u, 9)
  PH_MD5_STEP(PH_MD5_G, c, d, a, b, w[3], 0xf4d50d87u, 14)  PH_MD5_STEP(PH_MD5_G, b, c, d, a, w[8], 0x455a14edu, 20)
  PH_MD5_STEP(PH_MD5_G, a, b, c, d, w[13], 0xa9e3e905u, 5)  PH_MD5_STEP(PH_MD5_G, d, a, b, c, w[2], 0xfcefa3f8u, 9)
  PH_MD5_STEP(PH_MD5_G, c, d, a, b, w[7], 0x676f02d9u, 14)  PH_MD5_STEP(PH_MD5_G, b, c, d, a, w[12], 0x8d2a4c8au, 20)
  PH_MD5_STEP(PH_MD5_H, a, b, c, d, w[5], 0xfffa3942u, 4)   PH_MD5_STEP(PH_MD5_H, d, a, b, c, w[8], 0x8771f681u, 11)
  PH_MD5_STEP(PH_MD5_H, c, d, a, b, w[11], 0x6d9d6122u, 16) PH_MD5_STEP(PH_MD5_H, b, c, d, a, w[14], 0xfde5380cu, 23)
  PH_MD5_STEP(PH_MD5_H, a, b, c, d, w[1], 0xa4beea44u, 4)   PH_MD5_STEP(PH_MD5_H, d, a, b, c, w[4], 0x4bdecfa9u, 11)
  PH_MD5_STEP(PH_MD5_H, c, d, a, b, w[7], 0xf6bb4b60u, 16)  PH_MD5_STEP(PH_MD5_H, b, c, d, a, w[10], 0xbebfbc70u, 23)
  PH_MD5_STEP(PH_MD5_H, a, b, c, d, w[13], 0x289b7ec6u, 4)  PH_MD5_STEP(PH_MD5_H, d, a, b, c, w[0], 0xeaa127fau, 11)
  PH_MD5_STEP(PH_MD5_H, c, d, a, b, w[3], 0xd4ef3085u, 16)  PH_MD5_STEP(PH_MD5_H, b, c, d, a, w[6], 0x04881d05u, 23)
  PH_MD5_STEP(PH_MD5_H, a, b, c, d, w[9], 0xd9d4d039u, 4)   PH_MD5_STEP(PH_MD5_H, d, a, b, c, w[12], 0xe6db99e5u, 11)
  PH_MD5_STEP(PH_MD5_H, c, d, a, b, w[15], 0x1fa27cf8u, 16) PH_MD5_STEP(PH_MD5_H, b, c, d, a, w[2], 0xc4ac5665u, 23)
  PH_MD5_STEP(PH_MD5_I, a, b, c, d, w[0], 0xf4292244u, 6)   PH_MD5_STEP(PH_MD5_I, d, a, b, c, w[7], 0x432aff97u, 10)
  PH_MD5_STEP(PH_MD5_I, c, d, a, b, w[14], 0xab9423a7u, 15) PH_MD5_STEP(PH_MD5_I, b, c, d, a, w[5], 0xfc93a039u, 21)
  PH_MD5_STEP(PH_MD5_I, a, b, c, d, w[12], 0x655b59c3u, 6)  PH_MD5_STEP(PH_MD5_I, d, a, b, c, w[3], 0x8f0ccc92u, 10)
  PH_MD5_STEP(PH_MD5_I, c, d, a, b, w[10], 0xffeff47du, 15) PH_MD5_STEP(PH_MD5_I, b, c, d, a, w[1], 0x85845dd1u, 21)
  PH_MD5_STEP(PH_MD5_I, a, b, c, d, w[8], 0x6fa87e4fu, 6)   PH_MD5_STEP(PH_MD5_I, d, a, b, c, w[15], 0xfe2ce6e0u, 10)
  PH_MD5_STEP(PH_MD5_I, c, d, a, b, w[6], 0xa3014314u, 15)  PH_MD5_STEP(PH_MD5_I, b, c, d, a, w[13], 0x4e0811a1u, 21)
  PH_MD5_STEP(PH_MD5_I, a, b, c, d, w[4], 0xf7537e82u, 6)   PH_MD5_STEP(PH_MD5_I, d, a, b, c, w[11], 0xbd3af235u, 10)
  PH_MD5_STEP(PH_MD5_I, c, d, a, b, w[2], 0x2ad7d2bbu, 15)  PH_MD5_STEP(PH_MD5_I, b, c, d, a, w[9], 0xeb86d391u, 21)
  s->a += a; s->b += b; s->c += c; s->d += d;
}

// sixteen words from 64 bytes of any alignment
PH_FN void md5_words(const uint8_t *p, uint32_t w[16])
{
  for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
}

// The end of a chain: the `tail` (0 .. 63) bytes behind the last whole block, then the padding -- 0x80, zeros up to 56 (mod 64), the message length in bits as 64 bits,
// low byte first: one block for tails of 0 .. 55 bytes, two for 56 .. 63 -- and the digest, a b c d low byte first.  total_bytes: the whole message.
PH_FN void md5_tail(Md5State *s, const uint8_t *tail_bytes, int tail, uint64_t total_bytes, uint8_t digest[16])
{
  const uint64_t bits = total_bytes * 8;
  const int blocks = tail < 56 ? 1 : 2;
  for (int b = 0; b < blocks; b++) {
    uint32_t w[16];
    for (int i = 0; i < 16; i++) {
      uint32_t v = 0;
      for (int k = 0; k < 4; k++) {
        const int at = 64 * b + 4 * i + k;              // byte position behind the last whole block
        uint32_t byte = 0;
        if (at < tail) byte = tail_bytes[at];
        else if (at == tail) byte = 0x80;
        else if (at >= 64 * blocks - 8) byte = (uint32_t)(bits >> (8 * (at - (64 * blocks - 8)))) & 0xff;
        v |= byte << (8 * k);
      }
      w[i] = v;
    }
    md5_block(s, w);
  }
  const uint32_t st[4] = { s->a, s->b, s->c, s->d };
  for (int i = 0; i < 16; i++) digest[i] = (uint8_t)(st[i >> 2] >> (8 * (i & 3)));
}

// the whole chain over n bytes (the host's form; the device kernel walks the blocks itself, with the next block's words requested ahead)
PH_FN void md5_bytes(const uint8_t *p, uint64_t n, uint8_t digest[16])
{
  Md5State s; md5_init(&s);
  const uint64_t whole = n / 64;
  for (uint64_t b = 0; b < whole; b++) { uint32_t w[16]; md5_words(p + 64 * b, w); md5_block(&s, w); }
  md5_tail(&s, p + 64 * whole, (int)(n - 64 * whole), n, digest);
}

// ---- CRC ---------------------------------------------------------------------------------------------------------------------------------
// the reference's loop over one byte, most significant bit first: crc <- (crc x^8 + byte) mod P
PH_FN uint32_t crc_feed(uint32_t crc, uint32_t byte)
{
  for (int b = 0; b < 8; b++) { const uint32_t msb = (crc >> 15) & 1, bit = (byte >> (7 - b)) & 1; crc = (((crc << 1) + bit) & 0xffff) ^ (msb * 0x1021); }
  return crc;
}
// M(x) mod P of n bytes, from `crc` (0 for a partial)
PH_FN uint32_t crc_bytes(uint32_t crc, const uint8_t *p, size_t n) { for (size_t i = 0; i < n; i++) crc = crc_feed(crc, p[i]); return crc; }

// a b mod P, both below 2^16
PH_FN uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
  uint32_t r = 0;
  for (int i = 15; i >= 0; i--) {
    const uint32_t msb = (r >> 15) & 1;
    r = ((r << 1) & 0xffff) ^ (msb * 0x1021);          // r x mod P
    if ((b >> i) & 1) r ^= a;
  }
  return r;
}
// x^m mod P
PH_FN uint32_t crc_xpow(uint64_t m)
{
  uint32_t r = 1, sq = 2;                               // x^0, x^1
  for (int i = 0; i < 64; i++) {
    if ((m >> i) & 1) r = crc_mulmod(r, sq);
    if ((m >> i) <= 1) break;
    sq = crc_mulmod(sq, sq);
  }
  return r;
}
// Partials in chunk order -> digest: chunk k covers bytes [k chunk_bytes, min((k + 1) chunk_bytes, plane_bytes)).
// The sum  0xffff x^n ^ xor_k partial_k x^(bits behind chunk k)  is taken by Horner's rule from the first chunk on: m <- m x^(bits of chunk k) ^ partial_k, starting from the
// initial value 0xffff -- one multiplication a chunk, the power of x computed once for the whole chunks and once for the last, shorter one.
PH_FN uint32_t crc_fold(const uint32_t *partials, size_t n_chunks, uint64_t plane_bytes, uint64_t chunk_bytes)
{
  const uint32_t xc = crc_xpow(chunk_bytes * 8);
  uint32_t m = 0xffff;
  for (size_t k = 0; k < n_chunks; k++) {
    const uint64_t at = k * chunk_bytes;
    const uint32_t xk = at + chunk_bytes <= plane_bytes ? xc : crc_xpow((plane_bytes - at) * 8);
    m = crc_mulmod(m, xk) ^ (partials[k] & 0xffff);
  }
  return crc_mulmod(m, crc_xpow(16));                   // the 16 flush bits
}

// ---- checksum ----------------------------------------------------------------------------------------------------------------------------
PH_FN uint32_t checksum_mask(uint32_t x, uint32_t y) { return ((x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)) & 0xff; }
// sum over bytes [first, first + n) of a plane `width` samples wide with sample_bytes bytes a sample
PH_FN uint32_t checksum_bytes(const uint8_t *plane, uint64_t first, size_t n, uint32_t width, int sample_bytes)
{
  uint64_t s = first / (uint32_t)sample_bytes;
  uint32_t y = (uint32_t)(s / width), x = (uint32_t)(s - (uint64_t)y * width), sub = (uint32_t)(first - s * (uint32_t)sample_bytes), sum = 0;
  for (size_t i = 0; i < n; i++) {
    sum += (plane[first + i] ^ checksum_mask(x, y)) & 0xff;
    if (++sub == (uint32_t)sample_bytes) { sub = 0; if (++x == width) { x = 0; y++; } }
  }
  return sum;
}

PH_FN size_t report_chunks(uint64_t plane_bytes, uint64_t chunk_bytes) { return (size_t)((plane_bytes + chunk_bytes - 1) / chunk_bytes); }

// One plane by the chunked forms, serially (the CPU instantiation): method 1 MD5 (16 digest bytes), 2 CRC (2), 3 checksum (4).  Returns the digest's length.
PH_FN int plane_hash_chunked(const uint8_t *plane, uint32_t width, uint32_t height, int sample_bytes, int method, uint64_t chunk_bytes, uint8_t digest[16])
{
  const uint64_t n = (uint64_t)width * height * (uint32_t)sample_bytes;
  if (method == 1) { md5_bytes(plane, n, digest); return 16; }
  const size_t chunks = report_chunks(n, chunk_bytes);
  if (method == 2) {
    // the fold of crc_fold, with every partial made where it is used (no array of partials: no allocation here)
    const uint32_t xc = crc_xpow(chunk_bytes * 8);
    uint32_t m = 0xffff;
    for (size_t k = 0; k < chunks; k++) {
      const uint64_t at = k * chunk_bytes, end = at + chunk_bytes < n ? at + chunk_bytes : n;
      m = crc_mulmod(m, end - at == chunk_bytes ? xc : crc_xpow((end - at) * 8)) ^ crc_bytes(0, plane + at, (size_t)(end - at));
    }
    m = crc_mulmod(m, crc_xpow(16));
    digest[0] = (uint8_t)(m >> 8); digest[1] = (uint8_t)m;
    return 2;
  }
  uint32_t sum = 0;
  for (size_t k = 0; k < chunks; k++) {
    const uint64_t at = k * chunk_bytes, end = at + chunk_bytes < n ? at + chunk_bytes : n;
    sum += checksum_bytes(plane, at, (size_t)(end - at), width, sample_bytes);
  }
  for (int k = 0; k < 4; k++) digest[k] = (uint8_t)(sum >> (24 - 8 * k));
  return 4;
}

}  // namespace hevcdl_ph
#endif
