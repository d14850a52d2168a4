"""The shared slice-data decoder on the CPU (csrc/slice_decode_core.h behind hevcdl_parse_stream_core) against the parser (hevcdl_parse_stream, csrc/hevcdl_parse.cpp):
every reference-encoder stream under tests/golden, the shared coder's output on the synthetic corpora, damaged streams, a sanitizer harness and a mutation check.
Every comparison is exact: status, integer syntax, raw bytes.  No GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import entropy_cases as ec
from conftest import GOLD
from test_decode import ALL_STREAMS, FLIP_STREAMS, _join, _nals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUNCATED = [("rd_w200_q27_r2", "bitstream"), ("slices_r128_a2", "bitstream"), ("segments_t512x128_s2_a1", "bitstream"), ("stream_c192_q32", "bitstream_ps0")]      # the streams test_decode.py cuts


def _parse(stream, engine, **kw):
    """-> (status, ParsedStream or None, sentence)"""
    import hevcdl_amd
    try:
        return 0, hevcdl_amd.parse_stream(stream, engine=engine, **kw), ""
    except hevcdl_amd.HevcdlError as e:
        return e.status, None, str(e)


def ctu_named(sentence):
    m = re.search(r"CTU (\d+)", sentence)
    return None if m is None else int(m.group(1))


def assert_same_parse(a, b, what):
    """Two ParsedStream: picture infos, stream configuration and layouts equal; records and SAO blocks the same bytes."""
    assert bytes(a.cfg) == bytes(b.cfg), (what, "configuration")
    for x, y in ((a.slices, b.slices), (a.segments, b.segments)):
        assert (x is None) == (y is None) and (x is None or bytes(x) == bytes(y)), (what, "layouts")
    assert len(a.pictures) == len(b.pictures) and all(bytes(p) == bytes(q) for p, q in zip(a.pictures, b.pictures)), (what, "picture infos")
    assert a.records.shape == b.records.shape and a.records.tobytes() == b.records.tobytes(), (what, "records")
    assert a.sao.shape == b.sao.shape and a.sao.tobytes() == b.sao.tobytes(), (what, "SAO blocks")


def compare(stream, what, engine="core", **kw):
    """The stream through the parser and through `engine`: the same status; where both parse, the same output; where both name a CTU, the same CTU.  -> the status"""
    sa, a, wa = _parse(stream, "host")
    sb, b, wb = _parse(stream, engine, **kw)
    assert sa == sb, (what, sa, wa, sb, wb)
    if sa == 0:
        assert_same_parse(a, b, what)
    else:
        ca, cb = ctu_named(wa), ctu_named(wb)
        assert wb and (ca is None or cb is None or ca == cb), (what, wa, wb)
    return sa


def test_core_equals_the_parser_on_every_reference_stream():
    """All 215 reference-encoder streams under tests/golden, by test_decode.py's enumeration."""
    assert len(ALL_STREAMS) == 215
    done = 0
    for fam, name, key, _ in ALL_STREAMS:
        assert compare(np.load(os.path.join(GOLD, name + ".npz"))[key].tobytes(), (name, key)) == 0, (name, key)
        done += 1
    assert done == 215


def test_core_equals_the_parser_on_the_coder_corpora():
    """entropy_cases.fuzz_corpus() and layout_corpus() coded by the shared coder -- the streams that say +32768 behind a hidden sign included: refused by both, status 1."""
    refused = parsed = 0

    def conforming(recs):
        out = recs.copy()
        for k in ("coeff_y", "coeff_cb", "coeff_cr"):
            out[k][out[k] == -32768] = -32767
        return out
    for name, cfg, recs, sao in ec.fuzz_corpus():
        st = compare(ec.host_writer_stream(cfg, recs, sao), name)
        assert st in (0, 1), name
        refused, parsed = refused + (st == 1), parsed + (st == 0)
        if st == 1:      # (test_decode.py: -32768 behind a hidden sign; with -32767 in its place the picture conforms)
            assert compare(ec.host_writer_stream(cfg, conforming(recs), sao), name) == 0, name
    for name, cfg, recs, sao, lay in ec.layout_corpus():
        st = compare(ec.write_layout_access_units(cfg, recs, sao, lay)[0], name)
        assert st in (0, 1), name
        refused, parsed = refused + (st == 1), parsed + (st == 0)
        if st == 1:
            assert compare(ec.write_layout_access_units(cfg, conforming(recs), sao, lay)[0], name) == 0, name
    assert refused > 0 and parsed > 0


@pytest.mark.parametrize("name,key", TRUNCATED)
def test_core_equals_the_parser_on_truncated_streams(name, key):
    """The stream cut at every NAL boundary, and every slice NAL unit cut one byte short and in its middle."""
    stream = np.load(os.path.join(GOLD, name + ".npz"))[key].tobytes()
    nals = _nals(stream)
    errors = 0
    for k in range(1, len(nals)):
        errors += compare(_join(nals[:k]), (name, "cut in front of NAL", k)) != 0
        if (nals[k][1][0] >> 1) & 63 < 32:
            for cut in (len(nals[k][1]) - 1, len(nals[k][1]) // 2):
                assert compare(_join(nals[:k]) + b"\0\0\1" + nals[k][1][:cut], (name, "NAL", k, "cut at", cut)) != 0
    assert errors >= 3


@pytest.mark.parametrize("name,key", FLIP_STREAMS)
def test_core_equals_the_parser_on_every_single_bit_flip(name, key):
    """Every single bit of the three small streams test_decode.py flips: the status is the parser's; where both fail inside slice data the CTU named is the same; where
    both still parse the records are the same."""
    stream = np.load(os.path.join(GOLD, name + ".npz"))[key].tobytes()
    data = bytearray(stream)
    ok = refused = 0
    for bit in range(len(stream) * 8):
        data[bit >> 3] ^= 0x80 >> (bit & 7)
        st = compare(bytes(data), (name, "bit", bit))
        data[bit >> 3] ^= 0x80 >> (bit & 7)
        ok, refused = ok + (st == 0), refused + (st != 0)
    print("%s: %d flips, %d refused by both, %d parsed by both" % (name, len(stream) * 8, refused, ok))
    assert ok > 0 and refused > 0


def damaged_three():
    """Three damaged streams the parser refuses INSIDE slice data, naming the CTU: a sub-stream cut short, a flipped bit inside slice data, an entry point moved by one.
    -> [(what, stream, the CTU the parser names)].  (tests/test_parse_gpu.py sends exactly these to the kernel.)"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import hevc_parse as hp
    from test_decode import _flip
    out = []

    def load(name):
        stream = np.load(os.path.join(GOLD, name + ".npz"))["bitstream"].tobytes()
        nals = _nals(stream)
        return nals, next(i for i, (_, n) in enumerate(nals) if (n[0] >> 1) & 63 < 32)      # ... and its first slice NAL unit
    nals, k = load("slices_r128_a2")
    k += 1                                                                # the second (and last) slice of the first picture: every slice of the layout is there
    assert (nals[k][1][0] >> 1) & 63 < 32 and not nals[k][1][2] & 0x80
    out.append(("a sub-stream cut short", _join(nals[:k]) + b"\0\0\1" + nals[k][1][:len(nals[k][1]) // 2]))
    nals, k = load("dbksel_inpps0_72x72_q32_dis")
    for bit in range(4 * (len(nals[k][1]) - 2), 4 * (len(nals[k][1]) - 2) + 64):      # from the middle of the NAL unit on: the first flip the parser answers with a CTU
        flipped = _join(nals[:k] + [(nals[k][0], _flip(nals[k][1], bit))] + nals[k + 1:])
        st, _, why = _parse(flipped, "host")
        if st == 1 and ctu_named(why) is not None:
            out.append(("a flipped bit inside slice data", flipped))
            break
    nals, k = load("rd_t512_q32_2x2")
    sps, pps = hp.parse_sps(next(n for _, n in nals if (n[0] >> 1) & 63 == 33)), hp.parse_pps(next(n for _, n in nals if (n[0] >> 1) & 63 == 34))
    hdr, _ = hp.parse_slice_header(nals[k][1], sps, pps)
    assert len(hdr["entry_points"]) == 3
    lsb = hdr["entry_point_bit_pos"] - 16 + hdr["offset_len_minus1"]                 # the last bit of the first entry_point_offset_minus1
    out.append(("an entry point moved by one", _join(nals[:k] + [(nals[k][0], _flip(nals[k][1], lsb))] + nals[k + 1:])))
    assert len(out) == 3
    res = []
    for what, stream in out:
        st, _, why = _parse(stream, "host")
        assert st == 1 and ctu_named(why) is not None, (what, st, why)
        res.append((what, stream, ctu_named(why)))
    return res


def test_core_equals_the_parser_on_the_three_damaged_streams_of_the_gpu_test():
    for what, stream, ctu in damaged_three():
        st, _, why = _parse(stream, "core")
        assert st == 1 and ctu_named(why) == ctu, (what, why)


# ---- the stand-alone harness: sanitizers, and the mutation check ----------------------------------------------------------------------------------------------
def _build_harness(exe, sanitize, csrc=None):
    """tests/slice_decode_harness.cpp + csrc/hevcdl_parse.cpp + csrc/hevcdl_bitstream.cpp by the host compiler; csrc: a scratch copy of the directory (one with a mutated
    slice_decode_core.h).  -> the compiler's CompletedProcess"""
    import hevcdl_amd
    csrc = csrc or os.path.join(hevcdl_amd.PKG_DIR, "csrc")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"] if sanitize else []
    cmd = [shutil.which("g++"), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + flags + \
          ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "slice_decode_harness.cpp"), os.path.join(csrc, "hevcdl_parse.cpp"), os.path.join(csrc, "hevcdl_bitstream.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True)


def _dumps(tmp, flips):
    out = []
    for i, (fam, name, key, _) in enumerate(ALL_STREAMS):
        s = np.load(os.path.join(GOLD, name + ".npz"))[key]
        path = os.path.join(str(tmp), "s%03d.bin" % i)
        with open(path, "wb") as f:
            f.write(np.array([len(s), 1 if flips and (name, key) in FLIP_STREAMS else 0], np.int64).tobytes() + s.tobytes())
        out.append(path)
    return out


def test_sanitizer_harness(tmp_path):
    """The harness with -fsanitize=address,undefined -static-libasan, run as a program: the 215 fixtures and the flip corpus through the parser and the core, streams and
    outputs in exact-size heap blocks.  It finishes clean.  (Nothing is loaded into Python under a sanitizer.)"""
    if not shutil.which("g++"):
        pytest.skip("no host g++")
    exe = str(tmp_path / "slice_decode_harness")
    r = _build_harness(exe, True)
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("the host compiler has no static AddressSanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    dumps = _dumps(tmp_path, True)
    for i, (_, stream, _) in enumerate(damaged_three()):      # ... and the three damaged streams the GPU test sends to the kernel
        dumps.append(str(tmp_path / ("d%d.bin" % i)))
        with open(dumps[-1], "wb") as f:
            f.write(np.array([len(stream), 0], np.int64).tobytes() + stream)
    r = subprocess.run([exe] + dumps, capture_output=True, text=True)
    startup = ("ASan runtime does not come first", "Shadow memory range interleaves", "ReserveShadowMemoryRange failed", "error while loading shared libraries")
    if r.returncode != 0 and "slice decode harness:" not in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and any(m in r.stderr for m in startup):
        pytest.skip("the sanitizer build cannot start here: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200])
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    assert "%d dumps, 0 failed" % len(dumps) in r.stdout and r.stdout.count("flips agree") == len(FLIP_STREAMS)


# one-line mutants of csrc/slice_decode_core.h: (what, the line's text, its replacement)
MUTANTS = [
    ("a wrong context increment for the split flag", "if (sd_available(s, x, y - 1)) inc += sd_depth_at(s, x, y - 1) > depth;", "if (sd_available(s, x, y - 1)) inc += sd_depth_at(s, x, y - 1) >= depth;"),
    ("the candidate-list sort dropped", "if (c0 > c1) { tmp = c0; c0 = c1; c1 = tmp; } if (c0 > c2) { tmp = c0; c0 = c2; c2 = tmp; } if (c1 > c2) { tmp = c1; c1 = c2; c2 = tmp; }", "(void)tmp;"),
    ("the wavefront take-over one CTU late", "if (g.wpp && cx == u.cx0 + 1) {", "if (g.wpp && cx == u.cx0 + 2) {"),
    ("the Rice parameter update off by one", "if (a > (3 << go_rice)) go_rice", "if (a >= (3 << go_rice)) go_rice"),
]


def run_mutants(tmp):
    """Every mutant applied to a scratch copy of the core, built as the harness (without the sanitizers: a mutant is wrong, not unsafe) and run over the 215 fixtures.
    -> {what: [fixtures whose comparison with the parser failed]}"""
    import hevcdl_amd
    csrc = os.path.join(hevcdl_amd.PKG_DIR, "csrc")
    text = open(os.path.join(csrc, "slice_decode_core.h")).read()
    dumps = _dumps(tmp, False)
    caught = {}
    for i, (what, old, new) in enumerate(MUTANTS):
        assert text.count(old) == 1, what
        d = os.path.join(str(tmp), "mutant%d" % i)
        os.makedirs(d)
        for name in os.listdir(csrc):      # the headers and the two host sources: a quoted include is looked for beside the file that includes it
            if name.endswith(".h") or name in ("hevcdl_parse.cpp", "hevcdl_bitstream.cpp"):
                shutil.copy(os.path.join(csrc, name), d)
        with open(os.path.join(d, "slice_decode_core.h"), "w") as f:
            f.write(text.replace(old, new))
        exe = os.path.join(d, "harness")
        r = _build_harness(exe, False, csrc=d)
        assert r.returncode == 0, (what, r.stderr[-2000:])
        r = subprocess.run([exe] + dumps, capture_output=True, text=True)
        failed = [int(m.group(1)) for m in re.finditer(r"slice decode harness: \S*s(\d+)\.bin: ", r.stdout)]
        caught[what] = ["%s:%s" % (ALL_STREAMS[k][1], ALL_STREAMS[k][2]) for k in failed]
    return caught


def test_the_fixtures_catch_every_mutant(tmp_path):
    """The comparison of the first test, run by the harness against four wrong cores, fails for each of them on at least one fixture (profiles/parse_core_mutants.txt
    records which: `python tests/test_parse_core.py` rewrites it)."""
    if not shutil.which("g++"):
        pytest.skip("no host g++")
    caught = run_mutants(tmp_path)
    assert len(caught) >= 4
    for what, fixtures in caught.items():
        assert fixtures, what


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        caught = run_mutants(tmp)
    with open(os.path.join(ROOT, "profiles", "parse_core_mutants.txt"), "w") as f:
        f.write("One-line mutants of csrc/slice_decode_core.h against hevcdl_parse_stream on the 215 reference streams of tests/golden\n")
        f.write("(tests/test_parse_core.py::test_the_fixtures_catch_every_mutant; rewritten by `python tests/test_parse_core.py`).\n")
        for what, old, new in MUTANTS:
            f.write("\n%s\n  - %s\n  + %s\n  caught by %d of %d fixtures: %s\n" % (what, old, new, len(caught[what]), len(ALL_STREAMS), ", ".join(caught[what])))
