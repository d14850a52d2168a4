"""Scaling lists on the CPU: the sclist_* fixtures -- reference-encoder streams with scaling_list_enabled_flag (ScalingList 1: the default lists;
ScalingList 2: a list file written from a seed), each with the reference decoder's pictures (tools/gen_scaling_list_fixtures.py) -- through hevcdl_parse_stream_sl, the
shared decoder's entry (hevcdl_parse_stream_core_sl) and the host form of the scaling-list reconstruction.  Every comparison is exact.  No GPU."""
import ctypes
import functools
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ["cuqp", "default", "edge_q45", "file_pred", "file_rand", "file_steep_b10", "one_ctu", "tiles", "tskip", "wpp"]
RUNS = ("nolf", "dbk", "full")
SENTENCE = "scaling lists are outside this decoder"
ACCEPT_BOTH = 3
# Table 7-5 is 16 everywhere; Table 7-6, the intra list (matrixId 0 .. 2), by its index i in the up-right diagonal scan
TABLE_7_6_INTRA = [16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 17, 16, 17, 16, 17, 18, 17, 18, 18, 17, 18, 21, 19, 20, 21, 20, 19, 21, 24, 22, 22, 24,
                   24, 22, 22, 24, 25, 25, 27, 30, 27, 25, 25, 29, 31, 35, 35, 31, 29, 36, 41, 44, 41, 36, 47, 54, 54, 47, 65, 70, 65, 88, 88, 115]


@functools.lru_cache(maxsize=None)
def fixture(name):
    return np.load(os.path.join(GOLD, "sclist_%s.npz" % name))


@functools.lru_cache(maxsize=None)
def parsed(name, run, engine="host"):
    import hevcdl_amd
    return hevcdl_amd.parse_stream(fixture(name)["stream_" + run].tobytes(), cu_qp=True, scaling_lists=True, engine=engine)


def diag_scan(n):
    """6.5.3: the up-right diagonal scan of an n x n block -> [(x, y)] by scan index."""
    out, x, y = [], 0, 0
    while len(out) < n * n:
        while y >= 0:
            if x < n and y < n:
                out.append((x, y))
            y -= 1
            x += 1
        y, x = x, 0
    return out


def block_from_raster_lists(f):
    """7.4.5 from the arrays a fixture stores (the list file's, raster order): Y 4 8 16 32, Cb 4 8 16, Cr 4 8 16; 16x16 and 32x32 repeat their 8x8 list by 2 and 4, DC at [0]."""
    out = []
    for c in range(3):
        out += [f["lists4"][c].ravel(), f["lists8"][c].ravel()]
        b = np.kron(f["lists16"][c].reshape(8, 8), np.ones((2, 2), np.uint8))
        b[0, 0] = f["dc16"][c]
        out.append(b.ravel())
        if c == 0:
            b = np.kron(f["lists32"][0].reshape(8, 8), np.ones((4, 4), np.uint8))
            b[0, 0] = f["dc32"][0]
            out.append(b.ravel())
    return np.concatenate(out).astype(np.uint8)


def default_block():
    """The same from Tables 7-5 / 7-6 as the standard prints them (by scan index), through the diagonal scan; every DC 16."""
    l8 = np.zeros((8, 8), np.uint8)
    for i, (x, y) in enumerate(diag_scan(8)):
        l8[y, x] = TABLE_7_6_INTRA[i]
    out = []
    for c in range(3):
        out += [np.full(16, 16, np.uint8), l8.ravel(), np.kron(l8, np.ones((2, 2), np.uint8)).ravel()]
        if c == 0:
            out.append(np.kron(l8, np.ones((4, 4), np.uint8)).ravel())
    return np.concatenate(out)


def test_the_fixture_set():
    """Ten fixtures (the tiles_wpp case is two files, one stream each way), each below 1 MiB, none with a key the constant-QP families of tests/test_decode.py would pick up."""
    files = sorted(glob.glob(os.path.join(GOLD, "sclist_*.npz")))
    assert [os.path.basename(p)[7:-4] for p in files] == NAMES
    for p in files:
        f = np.load(p)
        assert os.path.getsize(p) < 1 << 20 and not any(k.startswith("bitstream") for k in f.files)
        assert all("stream_" + r in f.files and "picture_" + r in f.files for r in RUNS)
    assert (int(fixture("edge_q45")["width"]), int(fixture("edge_q45")["height"])) == (136, 72) and int(fixture("file_steep_b10")["bit_depth"]) == 10
    assert (int(fixture("one_ctu")["width"]), int(fixture("one_ctu")["height"]), int(fixture("one_ctu")["n_frames"])) == (64, 64, 1)


def _c_parse(fn, s, *tail):
    import hevcdl_amd
    buf = np.frombuffer(s, np.uint8)
    cfg = hevcdl_amd.StreamConfig()
    cfg.struct_size = ctypes.sizeof(cfg)
    n = ctypes.c_int(0)
    st = fn(buf.ctypes.data, buf.size, *tail[:1], ctypes.byref(cfg), None, None, None, 0, ctypes.byref(n), None, None, 0, *tail[1:]) if tail else \
        fn(buf.ctypes.data, buf.size, ctypes.byref(cfg), None, None, None, 0, ctypes.byref(n), None, None, 0)
    return st, hevcdl_amd.load_library().hevcdl_parse_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_without_the_bit_every_stream_is_refused_as_ever(name):
    """The parser, the core and the Python entry without scaling_lists -- with and without cu_qp --: HEVCDL_ERR_UNSUPPORTED with the sentence of the parent commit."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    for run in RUNS:
        s = fixture(name)["stream_" + run].tobytes()
        for engine in ("host", "core"):
            for cu_qp in (False, True):
                with pytest.raises(hevcdl_amd.HevcdlError) as e:
                    hevcdl_amd.parse_stream(s, engine=engine, cu_qp=cu_qp)
                assert e.value.status == 2 and SENTENCE in str(e.value)
        for fn in (lib.hevcdl_parse_stream, lib.hevcdl_parse_stream_core):
            assert _c_parse(fn, s) == (2, SENTENCE)
        for fn in (lib.hevcdl_parse_stream_qp, lib.hevcdl_parse_stream_core_qp):
            assert _c_parse(fn, s, 1, None, None) == (2, SENTENCE)
        # accept 0 / cu_qp alone through the new entry points is the old ones
        for fn in (lib.hevcdl_parse_stream_sl, lib.hevcdl_parse_stream_core_sl):
            for accept in (0, 1):
                assert _c_parse(fn, s, accept, None, None, None) == (2, SENTENCE)


def test_lists_with_cu_qp_need_both_bits():
    """The cuqp case with HEVCDL_ACCEPT_SCALING_LISTS alone: refused with the sentence of cu_qp_delta_enabled_flag."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    s = fixture("cuqp")["stream_nolf"].tobytes()
    for fn in (lib.hevcdl_parse_stream_sl, lib.hevcdl_parse_stream_core_sl):
        assert _c_parse(fn, s, 2, None, None, None) == (2, "cu_qp_delta_enabled_flag is outside this decoder")
        assert _c_parse(fn, s, ACCEPT_BOTH, None, None, None)[0] == 0
    for engine in ("host", "core"):
        with pytest.raises(hevcdl_amd.HevcdlError) as e:
            hevcdl_amd.parse_stream(s, scaling_lists=True, engine=engine)
        assert e.value.status == 2 and "cu_qp_delta_enabled_flag is outside this decoder" in str(e.value)
    p = parsed("cuqp", "nolf")
    assert p.qp_info.cu_qp_delta_enabled == 1 and (p.qp_info.cb_qp_offset, p.qp_info.cr_qp_offset) == (3, -4) and len(np.unique(p.qp_map)) > 2


# ---- bits of a parameter set ---------------------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self, data):
        self.b = "".join("{:08b}".format(x) for x in data)
        self.p = 0

    def u(self, n):
        v = int(self.b[self.p:self.p + n], 2) if n else 0
        self.p += n
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + self.u(z)

    def se(self):
        k = self.ue()
        return (k + 1) >> 1 if k & 1 else -(k >> 1)


def ue_bits(v):
    return "0" * ((v + 1).bit_length() - 1) + "{:b}".format(v + 1)


def se_bits(v):
    return ue_bits(2 * v - 1 if v > 0 else -2 * v)


def nal_of(stream, nal_type):
    """-> (first byte behind the two header bytes, end) of the first NAL unit of that type, and its RBSP bytes (emulation prevention removed)."""
    i = stream.index(b"\x00\x00\x01" + bytes([nal_type << 1, 1])) + 5
    j = stream.index(b"\x00\x00\x01", i)
    while stream[j - 1] == 0:
        j -= 1
    raw, out, zeros = stream[i:j], bytearray(), 0
    for x in raw:
        if zeros >= 2 and x == 3:
            zeros = 0
            continue
        out.append(x)
        zeros = zeros + 1 if x == 0 else 0
    return i, j, bytes(out)


def escape(rbsp):
    out, zeros = bytearray(), 0
    for x in rbsp:
        if zeros >= 2 and x <= 3:
            out.append(3)
            zeros = 0
        out.append(x)
        zeros = zeros + 1 if x == 0 else 0
    return bytes(out)


def sps_elements(rbsp):
    """The syntax elements of scaling_list_data() of an SPS -> (bit string of the RBSP, [(name, sizeId, matrixId, index, first bit, bits, value)])."""
    r = Bits(rbsp)
    r.u(8); r.u(88); r.u(8)
    r.ue(); r.ue(); r.ue(); r.ue()
    if r.u(1):
        r.ue(); r.ue(); r.ue(); r.ue()
    r.ue(); r.ue(); r.ue()
    r.u(1); r.ue(); r.ue(); r.ue()
    for _ in range(6):
        r.ue()
    els = []

    def take(name, size_id, m, i, fn):
        at = r.p
        v = fn()
        els.append((name, size_id, m, i, at, r.p - at, v))
        return v
    assert take("enabled", -1, -1, 0, lambda: r.u(1)) == 1
    if take("present", -1, -1, 0, lambda: r.u(1)):
        for size_id in range(4):
            for m in range(0, 6, 3 if size_id == 3 else 1):
                if not take("pred_mode", size_id, m, 0, lambda: r.u(1)):
                    take("delta_id", size_id, m, 0, r.ue)
                    continue
                if size_id > 1:
                    take("dc", size_id, m, 0, r.se)
                for i in range(16 if size_id == 0 else 64):
                    take("coef", size_id, m, i, r.se)
    return r.b, els


def with_sps_bits(stream, bits):
    """The stream with the RBSP of its SPS replaced by `bits` (padded with zeros to a byte)."""
    i, j, _ = nal_of(stream, 33)
    bits += "0" * (-len(bits) % 8)
    return stream[:i] + escape(bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8))) + stream[j:]


def reencoded(stream, pick, new_bits):
    """The stream with one syntax element of its SPS's scaling lists coded anew: pick(elements) -> the element."""
    _, _, rbsp = nal_of(stream, 33)
    bits, els = sps_elements(rbsp)
    e = pick(els)
    return with_sps_bits(stream, bits[:e[4]] + new_bits + bits[e[4] + e[5]:])


def test_the_sps_walker_reads_what_the_parser_reads():
    """The test's own walk over scaling_list_data() ends at the same place as a valid SPS: re-encoding an element with its own value gives the same stream."""
    for name in ("file_rand", "file_pred", "one_ctu"):
        s = fixture(name)["stream_nolf"].tobytes()
        _, _, rbsp = nal_of(s, 33)
        bits, els = sps_elements(rbsp)
        assert with_sps_bits(s, bits) == s
        assert {e[0] for e in els} >= {"pred_mode", "coef", "dc"}
    els = sps_elements(nal_of(fixture("file_pred")["stream_nolf"].tobytes(), 33)[2])[1]
    deltas = [(e[1], e[2], e[6]) for e in els if e[0] == "delta_id"]
    assert any(d[2] == 0 for d in deltas) and any(d[2] > 0 for d in deltas) and (3, 3, 1) in deltas      # the default, an earlier list, and the step of 3 at 32x32


@pytest.mark.parametrize("name", NAMES)
def test_the_factor_block(name):
    """hevcdl_scaling_info.factor == the block a numpy restatement derives from the list arrays of the fixture (default: from Tables 7-5 / 7-6), from parser and core."""
    f = fixture(name)
    want = default_block() if name == "default" else block_from_raster_lists(f)
    assert want.size == 2032
    for run in RUNS:
        for engine in ("host", "core"):
            p = parsed(name, run, engine)
            assert p.scaling.enabled == 1 and p.scaling.data_present == (0 if name == "default" else 1)
            assert np.array_equal(p.scaling_factors, want), (name, run, engine)
    if name == "file_rand":      # every list distinct, every DC other than its list's first entry
        assert len({f[k][m].tobytes() for k in ("lists8", "lists16") for m in range(6)}) == 12 and all(f["dc16"][m] != f["lists16"][m][0] for m in range(6)) and f["dc32"][0] != f["lists32"][0][0]


def test_a_stream_without_lists_has_factors_of_16_and_the_records_it_always_had():
    """A constant-QP stream of the existing fixtures through the _sl entry points: enabled 0, 2032 factors of 16, and the record bytes of hevcdl_parse_stream."""
    import hevcdl_amd
    s = np.load(os.path.join(GOLD, "rd_w200_q27_r2.npz"))["bitstream"].tobytes()
    a = hevcdl_amd.parse_stream(s)
    for engine in ("host", "core"):
        b = hevcdl_amd.parse_stream(s, scaling_lists=True, engine=engine)
        assert a.records.tobytes() == b.records.tobytes() and a.sao.tobytes() == b.sao.tobytes() and a.qps == b.qps
        assert (b.scaling.enabled, b.scaling.data_present) == (0, 0) and (b.scaling_factors == 16).all() and b.scaling_factors.size == 2032
        assert set(np.unique(b.qp_map).tolist()) == {0, 27}


@pytest.mark.parametrize("name", NAMES)
def test_parser_and_core_give_the_same_records(name):
    for run in RUNS:
        a, b = parsed(name, run), parsed(name, run, "core")
        assert a.records.tobytes() == b.records.tobytes() and a.sao.tobytes() == b.sao.tobytes() and a.qp_map.tobytes() == b.qp_map.tobytes()
        assert a.qps == b.qps == [int(q) for q in fixture(name)["slice_qps_" + run]]


@pytest.mark.parametrize("name", NAMES)
def test_host_reconstruction_gives_the_reference_decoders_picture(name):
    """hevcdl_reconstruct_frames_sl_host (csrc/recon_core.h instantiated with the factors) over every filters-off stream: the reference decoder's pictures, exactly; the
    flat reconstruction (hevcdl_reconstruct_frames_qp_host) of the same records and QP map is NOT that picture -- the lists are what the comparison rests on."""
    import hevcdl_amd
    p = parsed(name, "nolf")
    assert (p.scaling_factors != 16).any()
    got = hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info, scaling=p.scaling)
    assert np.array_equal(got, fixture(name)["picture_nolf"])
    flat = hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info)
    assert not np.array_equal(flat, fixture(name)["picture_nolf"])


def test_factors_of_16_give_the_flat_reconstruction():
    import hevcdl_amd
    p = parsed("one_ctu", "nolf")
    flat = hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info)
    assert np.array_equal(hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info, scaling=hevcdl_amd.scaling_info(np.full(2032, 16))), flat)
    with pytest.raises(hevcdl_amd.HevcdlError) as e:
        hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info, scaling=hevcdl_amd.scaling_info(np.zeros(2032)))
    assert e.value.status == 1 and "scaling factor 0 is 0" in str(e.value)


def test_coverage_conditions_over_the_whole_set():
    """tools/scaling_list_cover.py summed over every filters-off stream: non-zero levels at a non-16 factor in all seven plane kinds, DC levels under a DC factor of their own
    at 16x16 and 32x32 luma and 16x16 chroma, transform-skipped luma and chroma blocks under non-flat factors.  The 16-bit clip is NOT reached by any reference stream (the
    encoder quantises with the same factors, so a dequantised value is about the transform coefficient it came from: DESIGN.md 5n); the synthetic extremes reach it."""
    import scaling_list_cover as slc
    total = dict.fromkeys(slc.FIELDS, 0)
    for name in NAMES:
        c = slc.coverage(parsed(name, "nolf"))
        for k in total:
            total[k] += c[k]
    print(total)
    assert all(total[k] >= 1 for k in slc.FIELDS if k != "clip"), total
    assert total["clip"] == 0
    ts = slc.coverage(parsed("tskip", "nolf"))
    assert ts["ts_luma"] >= 1 and ts["ts_chroma"] >= 1
    assert slc.coverage(parsed("one_ctu", "nolf"))["nz_Y32"] >= 1


def test_the_pps_flag_stays_refused():
    """pps_scaling_list_data_present_flag set in a fixture's PPS: refused with the sentence as ever, with the bit too (the reference encoder never sets it)."""
    import hevcdl_amd
    for name in ("file_rand", "default"):
        s = fixture(name)["stream_nolf"].tobytes()
        i, j, rbsp = nal_of(s, 34)
        r = Bits(rbsp)
        r.ue(); r.ue(); r.u(5); r.u(1); r.u(1); r.ue(); r.ue(); r.se(); r.u(1); r.u(1)
        if r.u(1):
            r.ue()
        r.se(); r.se(); r.u(4)
        tiles = r.u(1); r.u(1)
        assert not tiles
        r.u(1)
        if r.u(1):
            r.u(1)
            if not r.u(1):
                r.se(); r.se()
        assert r.b[r.p] == "0"
        bits = r.b[:r.p] + "1" + r.b[r.p + 1:]
        t = s[:i] + escape(bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8))) + s[j:]
        for engine in ("host", "core"):
            for sl in (False, True):
                with pytest.raises(hevcdl_amd.HevcdlError) as e:
                    hevcdl_amd.parse_stream(t, cu_qp=True, scaling_lists=sl, engine=engine)
                assert e.value.status == 2 and SENTENCE in str(e.value)


def first(name, **kw):
    return lambda els: next(e for e in els if e[0] == name and all(e[{"size_id": 1, "m": 2, "i": 3}[k]] == v for k, v in kw.items()))


DAMAGE = [
    # (fixture, the element, its new coding, the sentence)
    ("file_pred", first("delta_id", size_id=0, m=1), ue_bits(2), "scaling_list_pred_matrix_id_delta 2 of list 1 of size 0"),
    ("file_pred", first("delta_id", size_id=3, m=3), ue_bits(2), "scaling_list_pred_matrix_id_delta 2 of list 3 of size 3"),
    ("file_rand", first("dc", size_id=2, m=0), se_bits(248), "scaling_list_dc_coef_minus8 248 of list 0 of size 2"),
    ("file_rand", first("dc", size_id=3, m=0), se_bits(-8), "scaling_list_dc_coef_minus8 -8 of list 0 of size 3"),
    ("file_rand", first("coef", size_id=1, m=2, i=5), se_bits(128), "scaling_list_delta_coef 128 of list 2 of size 1"),
    ("file_rand", first("coef", size_id=0, m=0, i=3), se_bits(-129), "scaling_list_delta_coef -129 of list 0 of size 0"),
    ("file_rand", first("coef", size_id=0, m=0, i=0), se_bits(-8), "entry 0 of scaling list 0 of size 0 is 0"),
]


@pytest.mark.parametrize("name,pick,new,sentence", DAMAGE, ids=[d[3].split(" of ")[0].replace(" ", "_") + "_%d" % k for k, d in enumerate(DAMAGE)])
def test_a_damaged_list_is_invalid_with_a_sentence(name, pick, new, sentence):
    import hevcdl_amd
    t = reencoded(fixture(name)["stream_nolf"].tobytes(), pick, new)
    for engine in ("host", "core"):
        with pytest.raises(hevcdl_amd.HevcdlError) as e:
            hevcdl_amd.parse_stream(t, cu_qp=True, scaling_lists=True, engine=engine)
        assert e.value.status == 1 and sentence in str(e.value)


def test_an_sps_that_ends_inside_its_lists_is_invalid():
    import hevcdl_amd
    for name in ("file_rand", "one_ctu"):
        s = fixture(name)["stream_nolf"].tobytes()
        _, _, rbsp = nal_of(s, 33)
        bits, els = sps_elements(rbsp)
        for e in (els[2], els[len(els) // 2], els[-40]):
            cut = ((e[4] + 7) // 8) * 8      # whole bytes: the SPS ends at or just behind the start of the element, inside the list data
            for engine in ("host", "core"):
                with pytest.raises(hevcdl_amd.HevcdlError) as err:
                    hevcdl_amd.parse_stream(with_sps_bits(s, bits[:cut]), cu_qp=True, scaling_lists=True, engine=engine)
                assert err.value.status == 1 and "the SPS ends inside its scaling lists" in str(err.value)


@pytest.mark.parametrize("name", ["file_rand", "one_ctu"])
def test_flips_and_truncations_of_the_sps_give_a_status(name):
    """Every single-bit flip and every truncation of the SPS: a status (0, 1 or 2), never a crash; a flip that still parses gives a factor block without zeros."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    full = fixture(name)["stream_nolf"].tobytes()
    s = full[:full.index(b"\x00\x00\x01", nal_of(full, 34)[1]) + 400]      # parameter sets and the start of the first picture: the headers are what is parsed here
    i, j, _ = nal_of(s, 33)
    cfg, n, qi, si = hevcdl_amd.StreamConfig(), ctypes.c_int(0), hevcdl_amd.QpInfo(), hevcdl_amd.ScalingInfo()

    def status(data):
        buf = np.frombuffer(data, np.uint8)
        cfg.struct_size = ctypes.sizeof(cfg)
        return lib.hevcdl_parse_stream_sl(buf.ctypes.data, buf.size, ACCEPT_BOTH, ctypes.byref(cfg), None, None, None, 0, ctypes.byref(n), None, None, 0, ctypes.byref(qi), None, ctypes.byref(si))
    assert status(s) == 0
    seen = {0: 0, 1: 0, 2: 0}
    b = bytearray(s)
    for bit in range(i * 8, j * 8):
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        st = status(bytes(b))
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        assert st in (0, 1, 2)
        seen[st] += 1
        if st == 0 and si.enabled:
            assert min(si.factor) > 0, bit
    for cut in range(i, j):
        assert status(s[:cut] + s[j:]) in (0, 1, 2)
    print(name, seen)
    assert seen[0] > 0 and seen[1] > 0


def _skip_unless_sanitizer_starts(r, tag):
    startup = ("ASan runtime does not come first", "Shadow memory range interleaves", "ReserveShadowMemoryRange failed", "error while loading shared libraries")
    if r.returncode != 0 and tag not in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and any(m in r.stderr for m in startup):
        pytest.skip("the sanitizer build cannot start here: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200])


def test_sanitizer_harness(tmp_path):
    """tests/scaling_list_harness.cpp + csrc/hevcdl_parse.cpp + csrc/hevcdl_bitstream.cpp + csrc/recon_core.h built with the host compiler and
    -fsanitize=address,undefined -static-libasan and run as a program: every fixture stream through the parser, the core and the host reconstruction in exact-size heap
    blocks, every flip and truncation of the smallest stream (a flip that parses is reconstructed too), and the synthetic extremes (levels of +-32767 under factors of 1 and
    255 at QP 51 and at the lowest QP of each bit depth)."""
    import scaling_list_mutants as sm
    if not shutil.which("g++"):
        pytest.skip("no host g++")
    exe = str(tmp_path / "scaling_list_harness")
    r = sm.build_harness(sm.CSRC, exe, flags=("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"))
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("the host compiler has no static AddressSanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    dumps = sm.write_dumps(str(tmp_path), runs=RUNS, mode_of=lambda name, run: 1 if (name, run) == ("one_ctu", "nolf") else 0)
    r = subprocess.run([exe] + dumps + ["extremes"], capture_output=True, text=True)
    _skip_unless_sanitizer_starts(r, "scaling_list harness:")
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    assert "%d dumps, 0 failed" % (len(dumps) + 1) in r.stdout and "flips and" in r.stdout and r.stdout.count("extremes: ") == 8


def test_five_one_line_mutants_are_caught():
    """tools/scaling_list_mutants.py: the DC entry not applied, row and column swapped in the replication, refMatrixId off by one, transform-skipped blocks left flat, the
    chroma planes swapped -- each makes the harness fail on at least one fixture stream, and the source as it is on none (the counts: profiles/scaling_list_mutants.txt)."""
    import scaling_list_mutants as sm
    if not shutil.which("g++"):
        pytest.skip("no host g++")
    res = sm.run_mutants()
    print(res)
    assert res["unchanged"][0] == 0 and set(res) == {"unchanged"} | set(sm.MUTANTS) and len(sm.MUTANTS) == 5
    for name in sm.MUTANTS:
        assert res[name][0] >= 1, name
