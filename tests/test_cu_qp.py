"""A QP per CU on the CPU: the cuqp_* fixtures -- reference-encoder streams with cu_qp_delta_enabled_flag (RateControl, AdaptiveQP, MaxDeltaQP) or PPS
chroma QP offsets, each with the reference decoder's pictures (tools/gen_cu_qp_fixtures.py) -- through hevcdl_parse_stream_qp, the shared decoder
(hevcdl_parse_stream_core_qp) and the host form of the QP-map reconstruction.  Every comparison is exact.  No GPU."""
import ctypes
import functools
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import entropy_cases as ec
from conftest import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ["act_b10_q2", "act_d0_r12", "act_d0_r6", "act_d2_q50", "aq_d0", "aq_d2", "aq_d3_q22", "aq_d3_q45", "b10_off", "chroma_off", "maxdqp", "rc_lcu", "rc_pic", "slices", "tiles", "wpp"]
RUNS = ("nolf", "dbk", "full")
# Table 8-12
TC = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24])
Z = np.array([[ec._z_of(x, y) for x in range(16)] for y in range(16)])


@functools.lru_cache(maxsize=None)
def fixture(name):
    return np.load(os.path.join(GOLD, "cuqp_%s.npz" % name))


@functools.lru_cache(maxsize=None)
def parsed(name, run, engine="host"):
    import hevcdl_amd
    return hevcdl_amd.parse_stream(fixture(name)["stream_" + run].tobytes(), cu_qp=True, engine=engine)


def test_the_fixture_set():
    """Sixteen fixtures, each below 1 MiB, none with a key that the constant-QP families of tests/test_decode.py would pick up; the table's sizes and keys."""
    files = sorted(glob.glob(os.path.join(GOLD, "cuqp_*.npz")))
    assert [os.path.basename(p)[5:-4] for p in files] == NAMES
    for p in files:
        f = np.load(p)
        assert os.path.getsize(p) < 1 << 20 and not any(k.startswith("bitstream") for k in f.files)
        assert all("stream_" + r in f.files and "picture_" + r in f.files for r in RUNS)
    assert (int(fixture("aq_d3_q22")["width"]), int(fixture("aq_d3_q22")["height"])) == (136, 72) and int(fixture("b10_off")["bit_depth"]) == 10


@pytest.mark.parametrize("name", NAMES)
def test_without_the_switch_every_stream_is_refused_as_ever(name):
    """The parser, the core and the Python entry without cu_qp: HEVCDL_ERR_UNSUPPORTED with the sentence of the parent commit."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    sentence = "chroma QP offsets are outside this decoder" if name == "chroma_off" else "cu_qp_delta_enabled_flag is outside this decoder"
    for run in RUNS:
        s = fixture(name)["stream_" + run].tobytes()
        for engine in ("host", "core"):
            with pytest.raises(hevcdl_amd.HevcdlError) as e:
                hevcdl_amd.parse_stream(s, engine=engine)
            assert e.value.status == 2 and sentence in str(e.value)
        buf = np.frombuffer(s, np.uint8)
        cfg = hevcdl_amd.StreamConfig()
        cfg.struct_size = ctypes.sizeof(cfg)
        n = ctypes.c_int(0)
        for fn in (lib.hevcdl_parse_stream, lib.hevcdl_parse_stream_core):
            assert fn(buf.ctypes.data, buf.size, ctypes.byref(cfg), None, None, None, 0, ctypes.byref(n), None, None, 0) == 2 and lib.hevcdl_parse_error().decode() == sentence
        # accept 0 through the new entry point is the old one
        assert lib.hevcdl_parse_stream_qp(buf.ctypes.data, buf.size, 0, ctypes.byref(cfg), None, None, None, 0, ctypes.byref(n), None, None, 0, None, None) == 2
        assert lib.hevcdl_parse_error().decode() == sentence


@pytest.mark.parametrize("name", NAMES)
def test_parser_and_core_agree_byte_for_byte(name):
    """hevcdl_parse_stream_qp == hevcdl_parse_stream_core_qp: QP map, records, SAO blocks, the PPS fields; the map is 0 outside the picture and every partition inside it
    is filled (QpY 0 occurs in no 8-bit fixture: their slice QPs are 12 and more and the ranges are 12 at the most)."""
    f = fixture(name)
    w, h, bd = int(f["width"]), int(f["height"]), int(f["bit_depth"])
    cx, cy = (w + 63) // 64, (h + 63) // 64
    for run in RUNS:
        a, b = parsed(name, run), parsed(name, run, "core")
        assert a.qp_map.tobytes() == b.qp_map.tobytes() and a.records.tobytes() == b.records.tobytes() and a.sao.tobytes() == b.sao.tobytes()
        assert [getattr(a.qp_info, k) for k, _ in a.qp_info._fields_] == [getattr(b.qp_info, k) for k, _ in b.qp_info._fields_]
        grid = a.qp_map.reshape(-1, cy, cx, 256)[:, :, :, Z].transpose(0, 1, 3, 2, 4).reshape(-1, cy * 16, cx * 16)
        assert not grid[:, h // 4:, :].any() and not grid[:, :, w // 4:].any()
        inside = grid[:, :h // 4, :w // 4]
        assert inside.min() >= -6 * (bd - 8) and inside.max() <= 51
        if bd == 8:
            assert inside.min() > 0
        if not a.qp_info.cu_qp_delta_enabled:
            assert name == "chroma_off" and (inside == np.array(a.qps)[:, None, None]).all()
    assert (parsed("chroma_off", "nolf").qp_info.cb_qp_offset, parsed("chroma_off", "nolf").qp_info.cr_qp_offset) == (3, -4)
    assert (parsed("b10_off", "nolf").qp_info.cb_qp_offset, parsed("b10_off", "nolf").qp_info.cr_qp_offset) == (-2, 5)
    assert [parsed(n, "nolf").qp_info.diff_cu_qp_delta_depth for n in ("aq_d0", "maxdqp", "aq_d2", "aq_d3_q22")] == [0, 1, 2, 3]


@pytest.mark.parametrize("name", NAMES)
def test_host_reconstruction_gives_the_reference_decoders_picture(name):
    """hevcdl_reconstruct_frames_qp_host (csrc/recon_core.h instantiated with the QP map) over every filters-off stream: the reference decoder's pictures, exactly."""
    import hevcdl_amd
    p = parsed(name, "nolf")
    got = hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info)
    assert np.array_equal(got, fixture(name)["picture_nolf"])


def test_constant_qp_reconstruction_is_not_what_these_streams_need():
    """The constant-QP form over the same records misses the picture where the QP varies: the map is what the comparison above rests on."""
    import hevcdl_amd
    for name in ("aq_d2", "chroma_off"):
        p = parsed(name, "nolf")
        assert not np.array_equal(hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qps=p.qps), fixture(name)["picture_nolf"])


@pytest.mark.parametrize("name", NAMES)
def test_slice_qps_are_the_reference_logs(name):
    for run in RUNS:
        assert parsed(name, run).qps == [int(q) for q in fixture(name)["slice_qps_" + run]]
    if name in ("rc_pic", "rc_lcu"):
        assert len(set(parsed(name, "full").qps)) > 1                    # rate control: the slice QP differs per picture


def test_tally_conditions_over_the_whole_set():
    """What the fixtures reach of the QP syntax and of 8.6.1 (hevcdl_parse_qp_tally, summed over every stream): every counter, suffixes of several bins, both signs, a
    group with a delta behind one without in the same CTU; and QpY below 0 (the 10-bit activity case at QP 2)."""
    import hevcdl_amd
    total = dict.fromkeys(hevcdl_amd.QP_TALLY_FIELDS, 0)
    for name in NAMES:
        for run in RUNS:
            hevcdl_amd.parse_stream(fixture(name)["stream_" + run].tobytes(), cu_qp=True)
            t = hevcdl_amd.parse_qp_tally()
            for k in total:
                total[k] = max(total[k], t[k]) if k == "max_abs_delta" else total[k] + t[k]
    print(total)
    assert all(v >= 1 for v in total.values()), total
    assert total["max_abs_delta"] >= 7 and total["suffixes_of_several_bins"] >= 1 and total["deltas_positive"] >= 1 and total["deltas_negative"] >= 1
    assert total["coded_behind_uncoded_in_ctu"] >= 1 and total["groups_without_delta"] >= 1
    assert parsed("act_b10_q2", "nolf").qp_map.min() < 0


def _grid(p, w, h):
    """(QpY, TU size) per 4x4 partition of every picture in raster order [pictures, h / 4, w / 4]."""
    cx, cy = (w + 63) // 64, (h + 63) // 64
    def g(a):
        return a.reshape(-1, cy, cx, 256)[:, :, :, Z].transpose(0, 1, 3, 2, 4).reshape(-1, cy * 16, cx * 16)[:, :h // 4, :w // 4]
    return g(p.qp_map).astype(np.int32), 64 >> (g(p.records["depth"]).astype(np.int32) + g(p.records["tr_idx"]))


def test_deblocking_coverage_of_the_deblock_only_fixtures():
    """Computed from map + records: over the deblock-only streams there are luma edges with QpP != QpQ and an odd sum (the + 1 of qPL matters), edges whose tC at qPL is
    neither side's, and chroma edges where the tC of Cb and of Cr differ."""
    odd = mid = cbcr = 0
    for name in NAMES:
        f, p = fixture(name), parsed(name, "dbk")
        w, h = int(f["width"]), int(f["height"])
        qp, tu = _grid(p, w, h)
        for dirn in (0, 1):
            q, t = (qp, tu) if dirn == 0 else (qp.transpose(0, 2, 1), tu.transpose(0, 2, 1))
            pos = np.arange(q.shape[2]) * 4
            edge = (pos[None, None, :] % 8 == 0) & (pos[None, None, :] > 0) & (pos[None, None, :] % t == 0)      # the 8x8 grid, a TU boundary of the Q side
            qq, qpp = q[:, :, 1:], q[:, :, :-1]
            e = edge[:, :, 1:]
            qpl = (qq + qpp + 1) >> 1
            odd += int((e & (qq != qpp) & ((qq + qpp) % 2 == 1)).sum())
            tc = lambda v: TC[np.clip(v + 2 + 2 * p.pictures[0].dbk.tc_offset_div2, 0, 53)]
            mid += int((e & (tc(qpl) != tc(qq)) & (tc(qpl) != tc(qpp))).sum())
            ce = e & (pos[None, None, 1:] % 16 == 0)
            qc = lambda off: np.where(qpl + off < 30, qpl + off, np.where(qpl + off >= 43, qpl + off - 6, np.array([29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37])[np.clip(qpl + off - 30, 0, 13)]))
            cbcr += int((ce & (tc(qc(p.qp_info.cb_qp_offset)) != tc(qc(p.qp_info.cr_qp_offset)))).sum())
    print(odd, mid, cbcr)
    assert odd >= 1 and mid >= 1 and cbcr >= 1


# (fixture, run, bit) -> the CTU both name: single-bit flips of a header byte found by a scan of the fixture (every later context starts from another state)
OUT_OF_RANGE = [("act_d0_r12", "nolf", 743, 5), ("maxdqp", "dbk", 748, 1)]


@pytest.mark.parametrize("name,run,bit,ctu", OUT_OF_RANGE)
def test_a_delta_out_of_range_is_a_damaged_stream_with_its_ctu(name, run, bit, ctu):
    import hevcdl_amd
    s = bytearray(fixture(name)["stream_" + run].tobytes())
    s[bit >> 3] ^= 0x80 >> (bit & 7)
    for engine, where in (("host", "CTU %d: " % ctu), ("core", "picture 0, CTU %d: " % ctu)):
        with pytest.raises(hevcdl_amd.HevcdlError) as e:
            hevcdl_amd.parse_stream(bytes(s), cu_qp=True, engine=engine)
        assert e.value.status == 1 and where + "CuQpDeltaVal outside its range" in str(e.value)


def _pps_flag_bit(stream):
    """Bit position, in the stream, of pps_slice_chroma_qp_offsets_present_flag of the first PPS (no emulation prevention byte lies in front of it in these streams)."""
    i = stream.index(b"\x00\x00\x01\x44\x01") + 5
    bits = "".join("{:08b}".format(b) for b in stream[i:i + 16])
    p = 0
    def u(n):
        nonlocal p
        v = int(bits[p:p + n], 2); p += n
        return v
    def ue():
        z = 0
        while u(1) == 0:
            z += 1
        return (1 << z) - 1 + (u(z) if z else 0)
    ue(); ue(); u(5); u(1); u(1); ue(); ue(); ue(); u(1); u(1)
    if u(1):
        ue()
    ue(); ue()
    return i * 8 + p


def test_slice_level_chroma_offsets_stay_refused():
    import hevcdl_amd
    for name in ("chroma_off", "aq_d2"):
        s = bytearray(fixture(name)["stream_nolf"].tobytes())
        bit = _pps_flag_bit(bytes(s))
        assert not s[bit >> 3] & (0x80 >> (bit & 7))
        s[bit >> 3] |= 0x80 >> (bit & 7)
        for engine in ("host", "core"):
            with pytest.raises(hevcdl_amd.HevcdlError) as e:
                hevcdl_amd.parse_stream(bytes(s), cu_qp=True, engine=engine)
            assert e.value.status == 2 and "slice-level chroma QP offsets are outside this decoder" in str(e.value)


FLIP_STREAMS = [("aq_d3_q45", "full"), ("maxdqp", "dbk")]


@pytest.mark.parametrize("name,run", FLIP_STREAMS)
def test_flips_and_truncations_give_one_status(name, run):
    """Every single-bit flip and every truncation of two small streams: the parser and the core answer with the same status, and where both parse, with the same bytes."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    s = fixture(name)["stream_" + run].tobytes()
    p = parsed(name, run)
    n, ctus = len(p.pictures), p.records.shape[1]

    def both(data):
        out = []
        for fn in (lib.hevcdl_parse_stream_qp, lib.hevcdl_parse_stream_core_qp):
            buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
            cfg = hevcdl_amd.StreamConfig()
            cfg.struct_size = ctypes.sizeof(cfg)
            cnt, info = ctypes.c_int(0), hevcdl_amd.QpInfo()
            recs, sao, qm = np.zeros((n, ctus), hevcdl_amd.REC_DTYPE), np.zeros((n, ctus, 3), hevcdl_amd.SAO_DTYPE), np.zeros((n, ctus, 256), np.int8)
            pics = (hevcdl_amd.ParsedPicture * n)()
            st = fn(buf.ctypes.data, len(data), 1, ctypes.byref(cfg), None, None, pics, n, ctypes.byref(cnt), recs.ctypes.data, sao.ctypes.data, n * ctus, ctypes.byref(info), qm.ctypes.data)
            out.append((st, (recs.tobytes(), sao.tobytes(), qm.tobytes()) if st == 0 else None))
        return out
    statuses = {0: 0, 1: 0, 2: 0}
    b = bytearray(s)
    for bit in range(len(s) * 8):
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        x, y = both(bytes(b))
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        assert x == y, ("flip", bit, x[0], y[0])
        statuses[x[0]] += 1
    for cut in range(len(s)):
        x, y = both(s[:cut])
        assert x == y, ("truncation", cut, x[0], y[0])
    print(name, run, statuses)
    assert statuses[0] > 0 and statuses[1] > 0


def test_sanitizer_harness(tmp_path):
    """tests/cu_qp_harness.cpp + csrc/hevcdl_parse.cpp + csrc/hevcdl_bitstream.cpp + csrc/recon_core.h built with the host compiler and -fsanitize=address,undefined
    -static-libasan and run as a program: every fixture stream through the parser, the core and the host reconstruction in exact-size heap blocks, the two damaged streams,
    and the flips and truncations of the smallest stream."""
    import cu_qp_mutants as cm
    if not shutil.which("g++"):
        pytest.skip("no host g++")
    exe = str(tmp_path / "cu_qp_harness")
    r = cm.build_harness(cm.CSRC, exe, flags=("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"))
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("the host compiler has no static AddressSanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    dumps = cm.write_dumps(str(tmp_path))
    for k, (name, run, bit, _) in enumerate(OUT_OF_RANGE):
        s = bytearray(fixture(name)["stream_" + run].tobytes())
        s[bit >> 3] ^= 0x80 >> (bit & 7)
        dumps.append(str(tmp_path / ("damaged%d.bin" % k)))
        open(dumps[-1], "wb").write(np.array([len(s), 0, 2], np.int64).tobytes() + bytes(s))
    s = fixture("aq_d3_q45")["stream_full"].tobytes()
    dumps.append(str(tmp_path / "flips.bin"))
    open(dumps[-1], "wb").write(np.array([len(s), 0, 1], np.int64).tobytes() + s)
    r = subprocess.run([exe] + dumps, capture_output=True, text=True)
    startup = ("ASan runtime does not come first", "Shadow memory range interleaves", "ReserveShadowMemoryRange failed", "error while loading shared libraries")
    if r.returncode != 0 and "cu_qp harness:" not in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and any(m in r.stderr for m in startup):
        pytest.skip("the sanitizer build cannot start here: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200])
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    assert "%d dumps, 0 failed" % len(dumps) in r.stdout and "flips and" in r.stdout


def test_four_one_line_mutants_are_caught():
    """tools/cu_qp_mutants.py: qPY_PRED from the left only, no qPY_PREV reset at a wavefront row, the parent's chroma cbf ignored for 4x4 blocks, Cr dequantised with the Cb
    offset -- each makes the harness fail on at least one fixture stream, and the source as it is on none (the counts: profiles/cu_qp_mutants.txt)."""
    import cu_qp_mutants as cm
    if not shutil.which("g++"):
        pytest.skip("no host g++")
    res = cm.run_mutants()
    print(res)
    assert res["unchanged"][0] == 0 and set(res) == {"unchanged"} | set(cm.MUTANTS)
    for name in cm.MUTANTS:
        assert res[name][0] >= 1, name


def test_a_constant_qp_stream_parses_the_same_with_the_switch_on():
    """An existing fixture through the _qp entry points with the switch on: the same records and SAO blocks, the PPS fields all 0, the map the slice QP inside the picture."""
    import hevcdl_amd
    f = np.load(os.path.join(GOLD, "rd_w200_q27_r2.npz"))
    s = f["bitstream"].tobytes()
    a = hevcdl_amd.parse_stream(s)
    for engine in ("host", "core"):
        b = hevcdl_amd.parse_stream(s, cu_qp=True, engine=engine)
        assert a.records.tobytes() == b.records.tobytes() and a.sao.tobytes() == b.sao.tobytes() and a.qps == b.qps
        assert [getattr(b.qp_info, k) for k, _ in b.qp_info._fields_] == [0, 0, 0, 0]
        vals = set(np.unique(b.qp_map).tolist())
        assert vals == {0, 27}                                               # 200 x 136: partitions outside the picture stay 0
