"""Planes and pictures for the picture report's tests (tests/test_report.py on the CPU, tests/test_report_gpu.py on the device): the shapes that reach every MD5 padding
length, every chunk boundary of the CRC / checksum partials and the x >> 8 / y >> 8 terms of the checksum mask, each filled with random, all-zero and all-maximal samples."""
import zlib

import numpy as np

CHUNK = 16384                                   # hevcdl_report_chunk_bytes(): checked by test_report.py
MD5_WIDTHS = (1, 55, 56, 57, 63, 64, 65, 119, 120, 128, 129)      # bytes of a w x 1 plane at 8 bits: tails on both sides of the 56-byte padding limit and of a block
CRC_CHUNKS = (1, 2, 3, 64, 0)                   # 0: the default
CHECKSUM_SHAPES = ((300, 2), (2, 300), (260, 260))      # (width, height): x >> 8 alone, y >> 8 alone, both
PICTURES = ((8, 8), (16, 8), (72, 40), (520, 8), (8, 520))
FILLS = ("random", "zero", "max")


def dtype_of(bit_depth):
    return np.uint8 if bit_depth == 8 else np.dtype("<u2")


def fill(shape, bit_depth, how, seed):
    if how == "zero":
        return np.zeros(shape, dtype_of(bit_depth))
    if how == "max":
        return np.full(shape, (1 << bit_depth) - 1, dtype_of(bit_depth))
    return np.random.default_rng(seed).integers(0, 1 << bit_depth, shape).astype(dtype_of(bit_depth))


def _planes(shapes):
    """shapes: (tag, width, height, bit depth) -> [(id, plane [height][width], bit depth)], one per fill."""
    out = []
    for tag, w, h, bd in shapes:
        for how in FILLS:
            name = "%s-%dx%d-b%d-%s" % (tag, w, h, bd, how)
            out.append((name, fill((h, w), bd, how, zlib.crc32(name.encode())), bd))      # seeded by the id: planes of equal id are equal
    return out


def md5_planes():
    shapes = [("tail", w, 1, 8) for w in MD5_WIDTHS]
    shapes += [("tail", w // 2, 1, bd) for bd in (10, 16) for w in MD5_WIDTHS if w % 2 == 0]      # the same byte lengths where they are even
    shapes += [("odd", 3, 5, 8), ("odd", 7, 9, 8), ("odd", 3, 5, 10), ("odd", 7, 9, 10)]
    return _planes(shapes)


def crc_lengths(chunk_bytes):
    c = chunk_bytes or CHUNK
    return [n for n in (c - 1, c, c + 1, 2 * c + 3, 1) if n > 0]


def crc_planes(chunk_bytes):
    """Planes of the byte lengths chunk - 1, chunk, chunk + 1, 2 chunk + 3 and 1 at 8 bits; at 10 bits the even ones of them, and the odd ones plus one byte."""
    shapes = [("len", n, 1, 8) for n in crc_lengths(chunk_bytes)]
    shapes += [("len", (n + 1) // 2, 1, 10) for n in sorted(set(crc_lengths(chunk_bytes)))]
    return _planes(shapes)


def checksum_planes():
    return _planes([("pos", w, h, bd) for (w, h) in CHECKSUM_SHAPES for bd in (8, 10)])


def edge_planes():
    """1 x 1, and one byte less than a chunk (the sanitizer harness and the device tests)."""
    return _planes([("edge", 1, 1, 8), ("edge", 1, 1, 10), ("edge", CHUNK - 1, 1, 8)])


def all_planes():
    """Every plane of the CPU file once (the CRC planes of every chunk size; planes of equal id are the same plane)."""
    seen, out = set(), []
    for case in md5_planes() + [c for cb in CRC_CHUNKS for c in crc_planes(cb)] + checksum_planes() + edge_planes():
        if case[0] not in seen:
            seen.add(case[0]); out.append(case)
    return out


def picture(width, height, bit_depth, seed, n=1):
    """n random packed planar 4:2:0 pictures [n, width * height * 3 / 2]."""
    return np.random.default_rng(seed).integers(0, 1 << bit_depth, (n, width * height * 3 // 2)).astype(dtype_of(bit_depth))


def picture_planes(pic, width, height):
    ysz = width * height
    return [pic[:ysz].reshape(height, width), pic[ysz:ysz + ysz // 4].reshape(height // 2, width // 2), pic[ysz + ysz // 4:].reshape(height // 2, width // 2)]
