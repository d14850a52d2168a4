"""The shared picture-hash source (csrc/picture_hash_core.h) on the CPU: hevcdl_plane_hash_host against hashlib.md5, against the reference's CRC and checksum loops restated
below, against the host's hevcdl_picture_hash and against the digests in the reference's streams (golden fixtures); the same under AddressSanitizer /
UndefinedBehaviorSanitizer; the CLI key.  No GPU."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import report_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- the reference's loops, restated (TComPicYuvMD5.cpp:89-165): the yardstick of the CRC and checksum tests ----
def crc_ref(plane, bit_depth):
    crc = 0xffff
    for v in plane.reshape(-1).tolist():
        for byte in ((v & 0xff,) if bit_depth == 8 else (v & 0xff, v >> 8)):
            for b in range(8):
                crc = (((crc << 1) + ((byte >> (7 - b)) & 1)) & 0xffff) ^ (0x1021 if crc & 0x8000 else 0)
    for b in range(16):
        crc = ((crc << 1) & 0xffff) ^ (0x1021 if crc & 0x8000 else 0)
    return bytes([crc >> 8, crc & 0xff])


def checksum_ref(plane, bit_depth):
    total = 0
    for y, row in enumerate(plane.tolist()):
        for x, v in enumerate(row):
            mask = (x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)
            total += ((v & 0xff) ^ mask) + (((v >> 8) ^ mask) if bit_depth > 8 else 0)
    return (total & 0xffffffff).to_bytes(4, "big")


def test_default_chunk():
    import hevcdl_amd
    assert hevcdl_amd.load_library().hevcdl_report_chunk_bytes() == rc.CHUNK and rc.CHUNK % 16 == 0


@pytest.mark.parametrize("case", rc.md5_planes(), ids=lambda c: c[0])
def test_md5_tails(case):
    """Every padding length: tails of 0 .. 55 bytes take one padding block, 56 .. 63 two."""
    import hevcdl_amd
    _, plane, bd = case
    assert hevcdl_amd.plane_hash_host(plane, bd, 1) == hashlib.md5(plane.tobytes()).digest()


@pytest.mark.parametrize("chunk", rc.CRC_CHUNKS)
def test_crc_chunking(chunk):
    """Planes that end one byte before, on and one byte behind a chunk boundary, of two chunks and a rest, and of one byte: the folded partials == the serial loop."""
    import hevcdl_amd
    for name, plane, bd in rc.crc_planes(chunk):
        assert hevcdl_amd.plane_hash_host(plane, bd, 2, chunk) == crc_ref(plane, bd), name
        assert hevcdl_amd.plane_hash_host(plane, bd, 3, chunk) == checksum_ref(plane, bd), name


@pytest.mark.parametrize("case", rc.checksum_planes(), ids=lambda c: c[0])
def test_checksum_positions(case):
    import hevcdl_amd
    _, plane, bd = case
    for chunk in (0, 64, 3):
        assert hevcdl_amd.plane_hash_host(plane, bd, 3, chunk) == checksum_ref(plane, bd)
    assert hevcdl_amd.plane_hash_host(plane, bd, 2) == crc_ref(plane, bd)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", rc.PICTURES, ids=lambda s: "%dx%d" % s)
def test_whole_pictures_against_the_host_hash(size, bd):
    import hevcdl_amd
    w, h = size
    pic = rc.picture(w, h, bd, seed=w * 7 + h + bd)[0]
    for method in (1, 2, 3):
        ours = b"".join(hevcdl_amd.plane_hash_host(p, bd, method) for p in rc.picture_planes(pic, w, h))
        assert ours == hevcdl_amd.picture_hash(w, h, pic, bd, method)


def _new_digests(w, h, pic, bd, method):
    import hevcdl_amd
    return b"".join(hevcdl_amd.plane_hash_host(p, bd, method) for p in rc.picture_planes(pic, w, h))


@pytest.mark.parametrize("key,method,bd", [("crc", 2, 8), ("sum", 3, 8), ("crc10", 2, 10), ("sum10", 3, 10)])
def test_fixture_streams_crc_and_checksum(key, method, bd):
    """The comparison tests/test_bitstream.py makes with the host hash: access units + hevcdl_write_hash_sei of the NEW digests of the reference's final pictures == the
    reference's stream of its SEIDecodedPictureHash 2 / 3 run."""
    import hevcdl_amd
    f = np.load(os.path.join(GOLD, "stream_c192_q32.npz"))
    w, h, qp, nf = int(f["width"]), int(f["height"]), int(f["qp"]), f["records"].shape[0]
    recs = np.frombuffer((f["records"] if bd == 8 else f["records10"]).tobytes(), dtype=hevcdl_amd.REC_DTYPE).reshape(nf, -1)
    pics = np.frombuffer(f["recon_" + key].tobytes(), rc.dtype_of(bd)).reshape(nf, w * h * 3 // 2)
    ours = b"".join(hevcdl_amd.write_access_unit(w, h, qp, poc, recs[poc], bit_depth=bd) + hevcdl_amd.hash_sei(method, _new_digests(w, h, pics[poc], bd, method)) for poc in range(nf))
    assert ours == f["bitstream_" + key].tobytes()


@pytest.mark.parametrize("name", ["c192_q32_r2", "w200_q30_b10"])
def test_fixture_streams_md5(name):
    """The reference's default-configuration runs carry an MD5 SEI behind every access unit: the SEI of the new digests of picture k is in the stream, the last picture's
    ends it, and the k-th occurrence order is the picture order."""
    import hevcdl_amd
    f = np.load(os.path.join(GOLD, "rd_%s.npz" % name))
    w, h, nf = int(f["width"]), int(f["height"]), f["yuv"].shape[0]
    bd = int(f["bit_depth"]) if "bit_depth" in f.files else 8
    pics = np.frombuffer(f["recon_filtered"].tobytes(), rc.dtype_of(bd)).reshape(nf, w * h * 3 // 2)
    stream = f["bitstream"].tobytes()
    at = -1
    for poc in range(nf):
        sei = hevcdl_amd.hash_sei(1, _new_digests(w, h, pics[poc], bd, 1))
        assert sei == hevcdl_amd.picture_hash_sei(w, h, pics[poc], bd)
        nxt = stream.find(sei, at + 1)
        assert nxt > at
        at = nxt
    assert stream.endswith(sei)


def test_entry_points_reject_bad_arguments():
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    p, dg = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
    assert lib.hevcdl_plane_hash_host(p.ctypes.data, 4, 4, 8, 0, 0, dg.ctypes.data) == 1       # no such method
    assert lib.hevcdl_plane_hash_host(p.ctypes.data, 4, 4, 8, 4, 0, dg.ctypes.data) == 1
    assert lib.hevcdl_plane_hash_host(p.ctypes.data, 0, 4, 8, 1, 0, dg.ctypes.data) == 1
    assert lib.hevcdl_plane_hash_host(p.ctypes.data, 4, 4, 7, 1, 0, dg.ctypes.data) == 2       # bit depths 8 .. 16
    assert lib.hevcdl_plane_hash_host(None, 4, 4, 8, 1, 0, dg.ctypes.data) == 1
    assert hevcdl_amd.REPORT_DTYPE.itemsize == 80 and hevcdl_amd.REPORT_DTYPE.fields["digest"][1] == 24 and hevcdl_amd.REPORT_DTYPE.fields["method"][1] == 72


def test_sanitizer_harness(tmp_path):
    """tests/report_harness.cpp + csrc/picture_hash_core.h built with the host compiler and -fsanitize=address,undefined -static-libasan: the tail, chunk and position cases
    above and the 1 x 1 / chunk - 1 planes, each in a heap block of exactly its size, without a sanitizer report and equal to the harness's serial loops."""
    import hevcdl_amd
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host g++")
    csrc = os.path.join(hevcdl_amd.PKG_DIR, "csrc")
    exe = str(tmp_path / "report_harness")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-I" + csrc, os.path.join(ROOT, "tests", "report_harness.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("the host compiler has no static AddressSanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    dumps = []

    def dump(name, plane, bd, chunk):
        dumps.append(str(tmp_path / ("%s_c%d.bin" % (name, chunk))))
        with open(dumps[-1], "wb") as f:
            f.write(np.array([plane.shape[1], plane.shape[0], bd, chunk], np.int32).tobytes() + hashlib.md5(plane.tobytes()).digest() + plane.tobytes())
    for name, plane, bd in rc.md5_planes() + rc.checksum_planes() + rc.edge_planes():
        dump(name, plane, bd, 0)
    for name, plane, bd in rc.checksum_planes()[:3] + rc.edge_planes():
        dump(name, plane, bd, 3)
    for chunk in rc.CRC_CHUNKS:
        for name, plane, bd in rc.crc_planes(chunk):
            dump(name, plane, bd, chunk)
    r = subprocess.run([exe] + dumps, capture_output=True, text=True)
    # only a binary that the loader or the sanitizer's start-up refused (before main) is a reason to skip; a harness that dies in any other way fails the test
    startup = ("ASan runtime does not come first", "Shadow memory range interleaves", "ReserveShadowMemoryRange failed", "error while loading shared libraries")
    if r.returncode != 0 and "report harness:" not in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and any(m in r.stderr for m in startup):
        pytest.skip("the sanitizer build cannot start here: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200])
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    assert "%d dumps, 0 failed" % len(dumps) in r.stdout


CFG = ["-i", "in.yuv", "-wdt", "192", "-hgt", "128", "-q", "32"]


def test_cli_key_is_parsed_and_range_checked(tmp_path):
    """--DeviceReport: 0 or 1; anything else is rejected by name (the no-GPU form of tests/test_app_cli.py: --PrintConfig stops behind the option checks)."""
    import json
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    r = subprocess.run([app] + CFG + ["--DeviceReport=2", "--PrintConfig"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "DeviceReport" in " ".join(json.loads(r.stdout)["errors"])
    for extra in (["--DeviceReport=1"], ["--DeviceReport=0"], ["--DeviceReport=1", "--DeviceEntropy=1", "--SEIDecodedPictureHash=2"]):
        r = subprocess.run([app] + CFG + extra + ["--PrintConfig"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and json.loads(r.stdout)["errors"] == [], r.stdout + r.stderr
