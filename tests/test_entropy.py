"""The entropy coder (csrc/entropy_coder.h) on the CPU: hevcdl_code_slice_data_host + hevcdl_write_access_unit_from_slice_data against the reference's streams
(golden fixtures), against the streams recorded from the former host writer (tests/golden/entropy_host_writer_digests.json) and against hevcdl_write_access_unit, the
other way from the same coder to an access unit, byte for byte; the capacity guard; garbage records; the same under AddressSanitizer / UndefinedBehaviorSanitizer.
No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import entropy_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("path", ec.CASES, ids=lambda p: os.path.basename(p)[3:-4])
def test_fixture_streams_without_sao(path):
    """56 reference runs (8 / 10 bit, tiles, wavefront, every tool switch, 8x8 and strip pictures): slice data by the shared coder + the access unit around it == the
    reference encoder's stream."""
    import hevcdl_amd
    cfg, recs, want = ec.fixture_case(path)
    coded = hevcdl_amd.code_slice_data(cfg, recs)
    ec.check_guard(coded)
    assert ec.assemble(cfg, coded) == want


@pytest.mark.parametrize("name", ec.SAO_CASES)
def test_fixture_streams_with_sao(name, oracle_built):
    import hevcdl_amd
    cfg, recs, sao = ec.sao_case(name)
    stream = ec.assemble(cfg, hevcdl_amd.code_slice_data(cfg, recs, sao))
    ec.assert_recorded_stream("sao_" + name, cfg, recs, sao, stream)
    assert stream == ec.host_writer_stream(cfg, recs, sao)


def test_pictures_of_maximal_levels_fit_the_default_capacity():
    """Checked with hevcdl_write_access_unit, which has no capacity of its own: the slice data of the all-+-32767 pictures stays below (CTUs x default capacity per
    CTU); the old per-CTU figure (hevcdl_access_unit_bound / CTUs = 12 288) does not hold for them, which is why the default is the derived 40 960
    (csrc/entropy_coder.h)."""
    import hevcdl_amd
    worst = 0.0
    for name, cfg, recs, sao in ec.fuzz_corpus()[:6]:
        n = len(ec.host_writer_stream(cfg, recs, sao))
        print(name, "access unit", n, "bytes,", n / recs.shape[1], "per CTU")
        worst = max(worst, n / recs.shape[1])
        assert n <= recs.shape[1] * 40960
    assert worst > 12288      # the figure the first design took from hevcdl_access_unit_bound is not a bound


def test_fuzz_against_the_host_writer():
    """At least 200 seeded synthetic pictures (valid records no encode produces) and the directed ones: the coder's sub-streams, assembled, are the stream recorded
    from the host writer, and hevcdl_write_access_unit (its own sub-stream regions, the second pass after an overflow, its own assembly) gives the same bytes."""
    import hevcdl_amd
    corpus = ec.fuzz_corpus()
    assert len(corpus) >= 200
    for name, cfg, recs, sao in corpus + ec.directed_pictures():
        coded = hevcdl_amd.code_slice_data(cfg, recs, sao)
        ec.check_guard(coded)
        stream = ec.assemble(cfg, coded)
        ec.assert_recorded_stream(name, cfg, recs, sao, stream)
        assert stream == ec.host_writer_stream(cfg, recs, sao), name


FIRST_PASS_PER_CTU = 4096      # HOST_FIRST_PASS_PER_CTU of csrc/hevcdl_bitstream.cpp: the room hevcdl_write_access_unit gives a picture's slice data before it knows better


def test_write_access_unit_codes_a_sub_stream_that_overflowed_once_more():
    """hevcdl_write_access_unit itself through its second pass.  The all-+-32767 corpus pictures of 72x72, 136x200 and 200x136 (one sub-stream each; 23 KB per whole
    CTU, 7 to 13 KB per CTU of the picture, against the 4 KB of the first pass) give the recorded streams; pictures of the same kind with two tiles and with three wavefront rows overflow in a sub-stream that has others in front
    of it (the coded ones move to the larger buffer, a wavefront row starts again from the contexts it started from) and give what the default regions give."""
    import hevcdl_amd
    for name, cfg, recs, sao in ec.fuzz_corpus()[3:6]:
        stream = ec.host_writer_stream(cfg, recs, sao)
        print(name, len(stream), "bytes,", recs.shape[1], "CTUs")
        assert len(stream) > recs.shape[1] * FIRST_PASS_PER_CTU + 4096, name      # more than the first pass holds (+ 64 bytes, + parameter sets and slice header)
        ec.assert_recorded_stream(name, cfg, recs, sao, stream)
    rng = np.random.default_rng(5)
    room = 12 * FIRST_PASS_PER_CTU + 64                                 # 136 x 200: 3 x 4 CTUs
    for kw in ({"tiles": (1, 2)}, {"wavefront": True}):
        cfg = hevcdl_amd.stream_config(136, 200, 30, **kw)
        recs = ec.synth_records(rng, 136, 200, 0)[None]
        coded = hevcdl_amd.code_slice_data(cfg, recs)
        n = [int(v) for v in coded[1][0]]
        print(kw, "sub-streams of", n, "bytes; first pass", room)
        if "tiles" in kw:      # tile 0 does not fit; tile 1 does not fit what its six CTUs are given behind it
            assert len(n) == 2 and n[0] > room and n[1] > 6 * FIRST_PASS_PER_CTU + 64
        else:                  # row 0 fits, row 1 does not fit what is left, row 2 does not fit what rows 2 and 3 are given behind row 1, row 3 fits
            assert len(n) == 4 and n[0] <= room < n[0] + n[1] and n[2] > 6 * FIRST_PASS_PER_CTU + 64 and n[3] <= 3 * FIRST_PASS_PER_CTU + 64
        assert ec.host_writer_stream(cfg, recs) == ec.assemble(cfg, coded)


@pytest.mark.parametrize("name", ["c192_q32_r2", "t576_q27_2x3", "w200_q27_r2"])
def test_overflow_is_flagged_and_nothing_is_written_past_the_region(name):
    import hevcdl_amd
    cfg, recs, _ = ec.fixture_case(os.path.join(ec.GOLD, "rd_%s.npz" % name))
    full = hevcdl_amd.code_slice_data(cfg, recs)
    small = hevcdl_amd.code_slice_data(cfg, recs, capacity_per_ctu=16)
    ec.check_guard(small)
    buf, sizes, ovf, off, cap = small
    assert ovf.any() and np.array_equal(sizes, full[1])                 # the reported length is the true length
    for poc in range(buf.shape[0]):
        for k in range(len(off)):                                        # what was stored is the head of the true sub-stream
            n = min(int(sizes[poc, k]), int(cap[k]))
            assert np.array_equal(buf[poc, off[k]:off[k] + n], full[0][poc, full[3][k]:full[3][k] + n])


@pytest.mark.parametrize("layout", ["plain", "wavefront", "tiles", "sao10"])
def test_garbage_records_stay_inside_the_guard(layout):
    """200 CTUs of seeded random bytes (depth 7, tr_idx 9, luma_dir 200, part_size 5, ...): the call returns, lengths are within the capacity or the overflow word is set,
    the canaries are intact."""
    import hevcdl_amd
    w, h = 640, 1280      # 10 x 20 CTUs
    cfg = hevcdl_amd.stream_config(w, h, 30, sao=layout == "sao10", tiles=(2, 3) if layout == "tiles" else (1, 1), bit_depth=10 if layout == "sao10" else 8, wavefront=layout == "wavefront")
    recs = ec.garbage_records(7, 200)[None]
    sao = ec.garbage_sao(8, 200)[None] if layout == "sao10" else None
    for cpc in (0, 64):
        ec.check_guard(hevcdl_amd.code_slice_data(cfg, recs, sao, capacity_per_ctu=cpc))


def test_entry_points_reject_bad_arguments():
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    cfg = hevcdl_amd.stream_config(64, 64, 32)
    n, nb = ctypes.c_int(0), ctypes.c_size_t(0)
    assert lib.hevcdl_slice_data_layout(ctypes.byref(cfg), 18, ctypes.byref(n), ctypes.byref(nb), None, None) == 1      # not a multiple of 4
    assert lib.hevcdl_slice_data_layout(ctypes.byref(cfg), 0, ctypes.byref(n), ctypes.byref(nb), None, None) == 0 and (n.value, nb.value) == (1, 40960 + 64 + 64)
    rec = np.zeros(1, hevcdl_amd.REC_DTYPE); buf = np.zeros(64, np.uint8); sz = np.zeros(1, np.uint32); ov = np.zeros(1, np.uint32)
    assert lib.hevcdl_code_slice_data_host(ctypes.byref(cfg), rec.ctypes.data, None, 1, 0, buf.ctypes.data, 64, sz.ctypes.data, ov.ctypes.data) == 1      # buffer smaller than the layout
    out = np.zeros(256, np.uint8); m = ctypes.c_size_t(0)
    assert lib.hevcdl_write_access_unit_from_slice_data(ctypes.byref(cfg), 0, buf.ctypes.data, sz.ctypes.data, 2, out.ctypes.data, 256, ctypes.byref(m)) == 1      # one sub-stream expected


def _dump(path, cfg, recs, sao, cpc, mode):
    with open(path, "wb") as f:
        f.write(bytes(cfg))
        f.write(np.array([recs.shape[0], 0 if sao is None else 1, cpc, mode], np.int32).tobytes())
        f.write(np.ascontiguousarray(recs).tobytes())
        if sao is not None:
            f.write(np.ascontiguousarray(sao).tobytes())


def test_sanitizer_harness(tmp_path):
    """tests/entropy_harness.cpp + csrc/hevcdl_bitstream.cpp built with the host compiler and -fsanitize=address,undefined -static-libasan: fixtures, the synthetic
    corpus, overflow and garbage records run without a sanitizer report and with the same checks as above, each picture also through hevcdl_write_access_unit."""
    import hevcdl_amd
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host g++")
    csrc = os.path.join(hevcdl_amd.PKG_DIR, "csrc")
    exe = str(tmp_path / "entropy_harness")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "entropy_harness.cpp"), os.path.join(csrc, "hevcdl_bitstream.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("the host compiler has no static AddressSanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    dumps = []
    for i, path in enumerate(ec.CASES):
        cfg, recs, _ = ec.fixture_case(path)
        dumps.append(str(tmp_path / ("fx%02d.bin" % i))); _dump(dumps[-1], cfg, recs, None, 0, 0)
        if i % 8 == 0:
            dumps.append(str(tmp_path / ("ov%02d.bin" % i))); _dump(dumps[-1], cfg, recs, None, 16, 1)
    for name, cfg, recs, sao in ec.fuzz_corpus():
        dumps.append(str(tmp_path / (name + ".bin"))); _dump(dumps[-1], cfg, recs, sao, 0, 0)
    for j, (tiles, wpp, bd) in enumerate([((1, 1), False, 8), ((1, 1), True, 8), ((2, 3), False, 8), ((1, 1), False, 10)]):
        cfg = hevcdl_amd.stream_config(640, 1280, 30, sao=bd == 10, tiles=tiles, bit_depth=bd, wavefront=wpp)
        for cpc in (0, 64):
            dumps.append(str(tmp_path / ("gb%d_%d.bin" % (j, cpc)))); _dump(dumps[-1], cfg, ec.garbage_records(7 + j, 200)[None], ec.garbage_sao(8, 200)[None] if bd == 10 else None, cpc, 1)
    r = subprocess.run([exe] + dumps, capture_output=True, text=True)
    # only a binary that the loader or the sanitizer's start-up refused (before main: a preloaded library, no room for the shadow memory) is a reason to skip; a
    # harness that dies in any other way fails the test
    startup = ("ASan runtime does not come first", "Shadow memory range interleaves", "ReserveShadowMemoryRange failed", "error while loading shared libraries")
    if r.returncode != 0 and "entropy harness:" not in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and any(m in r.stderr for m in startup):
        pytest.skip("the sanitizer build cannot start here: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200])
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    assert "%d dumps, 0 failed" % len(dumps) in r.stdout
