"""Dependent slice segments on the host (no GPU): SliceSegmentMode 1 over the CTU rows of a wavefront picture, SliceSegmentMode 3 over tiles.  The fixtures are runs of
the reference encoder (tools/gen_segment_fixtures.py); the writer -- one NAL unit per segment with a short dependent header, the shared slice-data coder ending a
sub-stream as a segment's last -- must give the reference's streams byte for byte, and nothing but the stream may change."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import rd_plan_cases
import segments_cases as sg
import slices_cases as sc
from conftest import GOLD, ROOT

REF_DEC = os.path.join(ROOT, "oracle", "_ref", "TAppDecoder_ref")
IDS = dict(ids=sg.case_id)


@pytest.fixture(scope="module")
def lib():
    import hevcdl_amd
    return hevcdl_amd.load_library()


_filter_cache = {}


def filtered(c):
    """(deblocked pictures, SAO parameters, final pictures) of the oracle's in-loop filters on the fixture's records and unfiltered reconstruction: computed once a
    fixture and shared.  Segments do not exist for the filters: the oracle runs the picture as the run without the keys would."""
    if c.name not in _filter_cache:
        import ref_tools
        dbk = ref_tools.run_deblock(c.prefilter(), c.w, c.h, c.qp, c.records(ref_tools.REC_DTYPE), bit_depth=c.bd, tiles=c.tiles, lf_across_tiles=True)
        dbk = np.asarray(dbk, np.uint8).reshape(c.nf, c.fs)
        params, pic = ref_tools.run_sao(c.yuv, dbk, c.w, c.h, c.qp, tiles=c.tiles, bit_depth=c.bd, lf_across_tiles=True)
        _filter_cache[c.name] = (dbk, params, np.asarray(pic, np.uint8).reshape(c.nf, c.fs))
    return _filter_cache[c.name]


def stream_cfg(c, sao):
    import hevcdl_amd
    return hevcdl_amd.stream_config(c.w, c.h, c.qp, sao=sao, tiles=c.tiles, bit_depth=c.bd, tools=c.tools, wavefront=c.wavefront)


def library_streams(c):
    """[(access units written by hevcdl_write_access_unit_segments, the reference's stream)] with SAO and without."""
    import hevcdl_amd
    _, params, _ = filtered(c)
    recs = c.records(hevcdl_amd.REC_DTYPE)
    out = []
    for sao, want in ((True, c.stream), (False, c.stream_nosao)):
        aus = [hevcdl_amd.write_access_unit(c.w, c.h, c.qp, poc, recs[poc], sao=params[poc].view(hevcdl_amd.SAO_DTYPE) if sao else None, tiles=c.tiles, bit_depth=c.bd,
                                            tools=c.tools, wavefront=c.wavefront, slices=c.slices, segments=c.segments) for poc in range(c.nf)]
        out.append((aus, want))
    return out


def test_the_fixture_set_is_the_generators():
    assert {sg.case_id(p) for p in sg.CASES} == sg.EXPECTED
    biggest_slices_fixture = max(os.path.getsize(p) for p in sc.CASES)
    for p in sg.CASES:
        assert os.path.getsize(p) <= biggest_slices_fixture, p


@pytest.mark.parametrize("path", sg.CASES, **IDS)
def test_fixtures_satisfy_the_generators_assertions(path):
    """Two pictures (an IDR and a CRA header); the NAL units of every access unit, their types and which are dependent; the stream is not as long as the run without the
    keys; the pictures put together from the deltas are pictures."""
    c = sg.Case(path)
    assert c.nf == 2 and len(c.dependent) > 1 and c.dependent[0] == 0 and sum(c.dependent) >= 1
    for s in (c.stream, c.stream_nosao):
        nals = sg.slice_nals(s)
        assert [[t for t, _, _ in au] for au in nals] == [[19] * len(c.dependent), [21] * len(c.dependent)]
        assert [[d for _, _, d in au] for au in nals] == [c.dependent] * c.nf
        assert [[f for _, f, _ in au] for au in nals] == [[1] + [0] * (len(c.dependent) - 1)] * c.nf
    assert len(c.stream) > int(c.f["base_stream_bytes"])
    assert c.final.shape == c.deblocked.shape == c.prefilter().shape == (c.nf, c.fs)
    assert len([l for l in c.f["stdout"] if str(l).startswith("POC")]) == c.nf


@pytest.mark.parametrize("path", sg.CASES, **IDS)
def test_writer_gives_both_reference_streams(oracle_built, path):
    """Records and SAO parameters (the oracle's on the fixture's records: its deblocked and final pictures are the reference's) through hevcdl_write_access_unit_segments:
    the reference's stream with SAO and the one of the --SAO=0 run, byte for byte, hash SEI included; the bound holds; the log's bit counts are the access units without
    the SEI."""
    import hevcdl_amd
    c = sg.Case(path)
    dbk, params, final = filtered(c)
    assert np.array_equal(dbk, c.deblocked) and np.array_equal(final, c.final)
    bound = hevcdl_amd.load_library().hevcdl_access_unit_bound_segments(c.w, c.h, hevcdl_amd._layout_ptr(hevcdl_amd.slice_layout(c.slices)),
                                                                       ctypes.byref(hevcdl_amd.segment_layout(c.segments)))
    (aus, want), (aus0, want0) = library_streams(c)
    assert all(len(au) <= bound for au in aus + aus0)
    assert b"".join(aus) == sg.strip_sei(want)
    assert b"".join(aus0) == sg.strip_sei(want0)
    assert [au + hevcdl_amd.picture_hash_sei(c.w, c.h, final[poc], c.bd) for poc, au in enumerate(aus)] == sg.access_units(want)
    assert [au + hevcdl_amd.picture_hash_sei(c.w, c.h, dbk[poc], c.bd) for poc, au in enumerate(aus0)] == sg.access_units(want0)
    bits = [int(str(l).split(")")[1].split("bits")[0]) for l in c.f["stdout"] if str(l).startswith("POC")]
    assert bits == [8 * len(au) for au in aus]      # all NAL units but the SEI (TEncGOP.cpp:2422-2448)


@pytest.mark.parametrize("path", sg.CASES, **IDS)
def test_nal_units_of_the_written_access_units(oracle_built, path):
    """What the library writes has the fixture's NAL units: VPS, SPS, PPS, then one slice NAL unit per segment of the fixture's type, dependent where the fixture's are,
    the zero_byte on the VPS alone."""
    c = sg.Case(path)
    for aus, want in library_streams(c):
        for poc, au in enumerate(aus):
            nals = sg.split_annexb(au)
            assert [(n[0] >> 1) & 63 for _, n in nals] == [32, 33, 34] + [19 if poc == 0 else 21] * len(c.dependent)
            assert [s for s, _ in nals] == [4, 4, 4] + [3] * len(c.dependent)      # parameter sets carry the zero_byte as ever; of the slice NAL units none follows them without
        assert [[d for _, _, d in au] for au in sg.slice_nals(b"".join(aus))] == [c.dependent] * c.nf


@pytest.mark.parametrize("path", sg.CASES, **IDS)
def test_slice_data_coded_apart_gives_the_same_streams(oracle_built, path):
    """hevcdl_code_slice_data_host_segments + hevcdl_write_access_unit_from_slice_data_segments: the sub-streams are the rows / tiles of the stream without segments, the
    regions are untouched outside, and only the sub-streams that end a segment differ from those coded without the keys."""
    import hevcdl_amd
    c = sg.Case(path)
    _, params, _ = filtered(c)
    layout = hevcdl_amd.slice_layout(c.slices)
    recs = c.records(hevcdl_amd.REC_DTYPE)
    for sao, want in ((True, c.stream), (False, c.stream_nosao)):
        cfg = stream_cfg(c, sao)
        sp = params.view(hevcdl_amd.SAO_DTYPE) if sao else None
        buf, sizes, ovf, off, cap = hevcdl_amd.code_slice_data(cfg, recs, sp, layout=layout, segments=c.segments)
        assert sizes.shape == (c.nf, c.cy if c.wavefront else c.tiles[0] * c.tiles[1]) and not ovf.any()
        for k in range(sizes.shape[1]):      # nothing but the regions is written
            assert (buf[:, int(off[k]) + int(cap[k]):int(off[k]) + int(cap[k]) + 64] == hevcdl_amd.CANARY).all()
        aus = [hevcdl_amd.write_access_unit_from_slice_data(cfg, poc, hevcdl_amd.pack_slice_data(buf[poc], sizes[poc], off), sizes[poc], layout=layout, segments=c.segments)
               for poc in range(c.nf)]
        assert b"".join(aus) == sg.strip_sei(want)
        # without the keys: the same regions, and the same bytes in every sub-stream that does not end a segment
        buf1, sizes1, _, off1, cap1 = hevcdl_amd.code_slice_data(cfg, recs, sp, layout=layout)
        assert np.array_equal(off, off1) and np.array_equal(cap, cap1)
        changed = c.substreams_ending_a_dependent_border()
        sub = lambda b, s, o, f, k: hevcdl_amd.pack_slice_data(b[f], s[f, k:k + 1], o[k:k + 1])
        for k in range(sizes.shape[1]):
            if k not in changed:
                assert all(sub(buf, sizes, off, f, k) == sub(buf1, sizes1, off1, f, k) for f in range(c.nf)), k
        assert changed and any(sub(buf, sizes, off, f, k) != sub(buf1, sizes1, off1, f, k) for f in range(c.nf) for k in changed)


def test_a_null_layout_and_mode_0_are_the_slices_functions():
    """The _segments entry points with a NULL block and with mode 0 (a stray argument beside it) on every slices_* fixture and on a one-slice picture of the reference
    (tests/golden/rd_c128_q27_r.npz, its run with --SAO=0): the bytes, lengths, regions and bounds of the _slices functions."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    blocks = (None, hevcdl_amd.SegmentLayout(0, 77))
    jobs = []
    for p in sc.CASES:
        c = sc.Case(p)
        cfg = hevcdl_amd.stream_config(c.w, c.h, c.qp, tiles=c.tiles, bit_depth=c.bd, lf_across_tiles=c.lf_tiles, tools=c.tools, lf_offsets=c.offsets, lf_disable=c.lf_disable)
        jobs.append((c.name, cfg, hevcdl_amd.slice_layout(c.slices, c.lf_slices), c.records(hevcdl_amd.REC_DTYPE), c.choice(), None))
    f = np.load(os.path.join(GOLD, "rd_c128_q27_r.npz"))
    w, h, qp, nf = int(f["width"]), int(f["height"]), int(f["qp"]), f["records"].shape[0]
    recs = np.frombuffer(f["records"].tobytes(), dtype=hevcdl_amd.REC_DTYPE).reshape(nf, -1)
    jobs.append(("rd_c128_q27_r", hevcdl_amd.stream_config(w, h, qp), None, recs, None, sc.strip_sei(f["bitstream_nosao"].tobytes())))
    for name, cfg, layout, recs, choice, reference in jobs:
        lp = hevcdl_amd._layout_ptr(layout)
        cp, _keep = hevcdl_amd._choice_ptr(choice)
        cap = lib.hevcdl_access_unit_bound_slices(cfg.width, cfg.height, lp)
        b0, s0, o0, off0, cap0 = hevcdl_amd.code_slice_data(cfg, recs, layout=layout)
        old = b""
        for poc in range(recs.shape[0]):
            buf, n = np.zeros(cap, np.uint8), ctypes.c_size_t(0)
            assert lib.hevcdl_write_access_unit_slices(ctypes.byref(cfg), lp, poc, recs[poc].ctypes.data, None, cp, buf.ctypes.data, cap, ctypes.byref(n)) == 0
            old += buf[:n.value].tobytes()
        assert reference is None or old == reference, name
        for block in blocks:
            bp = ctypes.byref(block) if block is not None else None
            assert lib.hevcdl_access_unit_bound_segments(cfg.width, cfg.height, lp, bp) == cap, name
            new = apart = b""
            b1, s1, o1, off1, cap1 = hevcdl_amd.code_slice_data(cfg, recs, layout=layout, segments=block)
            assert b0.tobytes() == b1.tobytes() and np.array_equal(s0, s1) and np.array_equal(o0, o1) and np.array_equal(off0, off1) and np.array_equal(cap0, cap1), name
            for poc in range(recs.shape[0]):
                buf, n = np.zeros(cap, np.uint8), ctypes.c_size_t(0)
                assert lib.hevcdl_write_access_unit_segments(ctypes.byref(cfg), lp, bp, poc, recs[poc].ctypes.data, None, cp, buf.ctypes.data, cap, ctypes.byref(n)) == 0
                new += buf[:n.value].tobytes()
                data = np.frombuffer(hevcdl_amd.pack_slice_data(b1[poc], s1[poc], off1) + b"\0", np.uint8)
                buf, n = np.zeros(cap, np.uint8), ctypes.c_size_t(0)
                assert lib.hevcdl_write_access_unit_from_slice_data_segments(ctypes.byref(cfg), lp, bp, poc, data.ctypes.data, s1[poc].ctypes.data, int(s1[poc].size), cp, buf.ctypes.data,
                                                                             cap, ctypes.byref(n)) == 0
                apart += buf[:n.value].tobytes()
            assert new == old and apart == old, name


def test_writer_refuses_segment_layouts_it_cannot_write(lib):
    import hevcdl_amd

    def status(cfg, segments, slices=None, ctus=6):
        recs = np.zeros(ctus, hevcdl_amd.REC_DTYPE)
        cap = 1 << 16
        buf, n = np.zeros(cap, np.uint8), ctypes.c_size_t(0)
        return lib.hevcdl_write_access_unit_segments(ctypes.byref(cfg), hevcdl_amd._layout_ptr(hevcdl_amd.slice_layout(slices)), ctypes.byref(hevcdl_amd.SegmentLayout(*segments)), 0,
                                                     recs.ctypes.data, None, None, buf.ctypes.data, cap, ctypes.byref(n))
    wpp = hevcdl_amd.stream_config(192, 128, 32, wavefront=True)            # 3 x 2 CTUs
    plain = hevcdl_amd.stream_config(192, 128, 32)
    assert status(wpp, (1, 3)) == 0 and status(wpp, (1, 6)) == 0 and status(wpp, (1, 300)) == 0 and status(wpp, (0, 5)) == 0
    assert status(wpp, (2, 1500)) == 2                                      # segments by bytes: HEVCDL_ERR_UNSUPPORTED
    for bad in ((1, 0), (1, 2), (1, 4), (1, -3), (3, 1), (4, 1), (-1, 1)):     # not whole rows; SliceSegmentMode 3 without tiles; no mode
        assert status(wpp, bad) == 1, bad
    assert status(plain, (1, 3)) == 1                                       # no wavefront: a row would start in the middle of the coder chain
    assert status(plain, (1, 3), slices=(1, 3)) == 1
    tiled = hevcdl_amd.stream_config(512, 128, 32, tiles=(2, 2))
    assert status(tiled, (3, 1), ctus=16) == 0 and status(tiled, (3, 3), ctus=16) == 0 and status(tiled, (3, 9), ctus=16) == 0 and status(tiled, (3, 1), slices=(3, 2), ctus=16) == 0
    assert status(tiled, (3, 0), ctus=16) == 1 and status(tiled, (1, 8), ctus=16) == 1 and status(tiled, (2, 8), ctus=16) == 2
    thin = hevcdl_amd.stream_config(64, 192, 32, wavefront=True)            # one CTU wide: every CTU a segment
    assert status(thin, (1, 1), ctus=3) == 0 and status(thin, (1, 2), ctus=3) == 0


REFUSALS = [      # (keyword arguments of default_config, status, a word of the reason)
    (dict(segments=(2, 1500), wavefront=True), 2, "SliceSegmentMode 2"),
    (dict(segments=(1, 5)), 2, "the reference's decisions change"),                                       # no wavefront
    (dict(segments=(1, 5)), 2, "needs WaveFrontSynchro"),
    (dict(segments=(1, 3), wavefront=True), 2, "the reference's decisions"),                               # five CTUs wide: 3 is no whole row
    (dict(segments=(1, 7), wavefront=True), 2, "multiple of the picture's width"),
    (dict(segments=(1, 0), wavefront=True), 2, "multiple of the picture's width"),
    (dict(segments=(1, 5), tiles=(1, 2)), 2, "together with tiles"),
    (dict(segments=(1, 5), slices=(1, 5)), 2, "together with slices"),
    (dict(segments=(3, 1)), 1, "needs tiles"),
    (dict(segments=(3, 1), wavefront=True), 1, "needs tiles"),
    (dict(segments=(3, 0), tiles=(1, 2)), 1, "at least 1 tile"),
    (dict(segments=(1, 5), wavefront=True, deblocking_metric=1, lf_offset_in_pps=False), 2, "DeblockingFilterMetric"),
    (dict(segments=(3, 1), tiles=(1, 2), deblocking_metric=2, lf_offset_in_pps=False), 2, "DeblockingFilterMetric"),
    (dict(segments=(4, 1), wavefront=True), 1, "SliceSegmentMode is 0, 1 or 3"),
]


@pytest.mark.parametrize("kw,status,word", REFUSALS, ids=[r[2].replace(" ", "-") + "-%d" % i for i, r in enumerate(REFUSALS)])
def test_create_refuses_with_a_status_and_a_reason(lib, kw, status, word):
    """hevcdl_create checks the segment keys before it looks for a device: the refusals need no GPU."""
    import hevcdl_amd
    cfg = hevcdl_amd.default_config(320, 256, 32, **kw)       # 5 x 4 CTUs
    w = np.zeros(hevcdl_amd.WEIGHT_FLOATS, np.float32)
    h = ctypes.c_void_p()
    assert lib.hevcdl_create(ctypes.byref(cfg), w.ctypes.data, w.size, ctypes.byref(h)) == status
    why = lib.hevcdl_create_error().decode()
    assert why and word in why


def test_create_accepts_what_it_should(lib):
    import hevcdl_amd
    w = np.zeros(hevcdl_amd.WEIGHT_FLOATS, np.float32)

    def create(cfg):
        h = ctypes.c_void_p()
        st = lib.hevcdl_create(ctypes.byref(cfg), w.ctypes.data, w.size, ctypes.byref(h))
        if st == 0:
            lib.hevcdl_destroy(h)
        return st, lib.hevcdl_create_error().decode()
    # what is valid gets past the segment keys: a context (on a GPU), or the loud failure for want of a device -- never a reason
    for cfg in (hevcdl_amd.default_config(320, 256, 32, wavefront=True, segments=(1, 5)), hevcdl_amd.default_config(320, 256, 32, wavefront=True, segments=(1, 15)),
                hevcdl_amd.default_config(64, 192, 32, wavefront=True, segments=(1, 1)), hevcdl_amd.default_config(512, 128, 32, tiles=(2, 2), segments=(3, 3)),
                hevcdl_amd.default_config(512, 128, 32, tiles=(2, 2), slices=(3, 2), segments=(3, 1)), hevcdl_amd.default_config(320, 256, 32, segments=(0, 3))):
        st, why = create(cfg)
        assert st in (0, 3) and why == ""
    tail = hevcdl_amd.default_config(128, 128, 32)             # a zeroed tail is no segments
    assert (tail.slice_segment_mode, tail.slice_segment_argument) == (0, 0)
    assert create(tail)[0] in (0, 3)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/segments_harness.cpp + csrc/hevcdl_bitstream.cpp under the host compiler's sanitizers (a stand-alone program: nothing is loaded into this process)."""
    import hevcdl_amd
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host g++")
    csrc = os.path.join(hevcdl_amd.PKG_DIR, "csrc")
    exe = str(tmp_path_factory.mktemp("segments") / "segments_harness")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "segments_harness.cpp"), os.path.join(csrc, "hevcdl_bitstream.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("the host compiler has no static AddressSanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr

    def ask(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        startup = ("error while loading shared libraries", "ASan runtime does not come first", "Shadow memory range interleaves", "ReserveShadowMemoryRange failed")
        if r.returncode != 0 and not r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and any(m in r.stderr for m in startup):
            pytest.skip("the sanitizer build cannot start here: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200])
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return ask


def layout_words(w, h, qp, wavefront=False, tiles=(1, 1), slices=None, segments=None):
    s, g = slices or (0, 0), segments or (0, 0)
    return "%d %d %d %d %d %d %d %d %d %d" % (w, h, qp, int(wavefront), tiles[0], tiles[1], s[0], s[1], g[0], g[1])


def test_segment_context_plans_like_the_context_without_the_keys(harness):
    """csrc/slice_grid.h hands the launch plan a configuration WITHOUT the segment keys: the plan of a segment context is the plan of the same context without them,
    launch for launch, over the frame counts of tests/rd_plan_cases.py -- at 2160p with wavefront (34 rows) and with tiles, and on the fixture shapes."""
    with open(os.path.join(GOLD, "rd_launch_forms.json")) as f:
        rec = json.load(f)
    waves = " ".join(str(rec["waves"][b]) for b in rd_plan_cases.BUILDS)
    counts = sorted({c["n_frames"] for c in rec["cases"] if c["call"] == "frames"} | {1, 75})
    shapes = [dict(w=3840, h=2160, wavefront=True, segments=(1, 60)), dict(w=3840, h=2160, wavefront=True, segments=(1, 240)), dict(w=3840, h=2160, tiles=(4, 3), segments=(3, 1)),
              dict(w=3840, h=2160, tiles=(4, 3), slices=(3, 4), segments=(3, 3)), dict(w=264, h=136, wavefront=True, segments=(1, 5)), dict(w=64, h=192, wavefront=True, segments=(1, 1)),
              dict(w=512, h=128, tiles=(2, 2), segments=(3, 3))]
    lines = []
    for s in shapes:
        for n in counts:
            head = "plan %d %s %d" % (rec["cus"], waves, max(counts))
            lines.append("%s %s %d" % (head, layout_words(qp=32, **s), n))
            lines.append("%s %s %d" % (head, layout_words(qp=32, **dict(s, segments=None)), n))
    got = harness(lines)
    forms = set()
    for i in range(0, len(got), 2):
        assert got[i] == got[i + 1] and not got[i].startswith("status") and got[i].endswith("\t0 0"), (lines[i], got[i], got[i + 1])
        forms.add(got[i].split("\t")[1].split(" form=")[1].split(" ")[0].split("(")[0])
    assert len(forms) >= 2, forms      # the shapes and counts reach more than one launch form
    # and the refusals arrive through the same function
    head = "plan %d %s 8" % (rec["cus"], waves)
    bad = harness(["%s %s 1" % (head, layout_words(3840, 2160, 32, segments=(1, 60))), "%s %s 1" % (head, layout_words(3840, 2160, 32, wavefront=True, segments=(1, 61))),
                   "%s %s 1" % (head, layout_words(3840, 2160, 32, wavefront=True, segments=(2, 1500)))])
    assert [b.split("\t")[0] for b in bad] == ["status 2"] * 3 and "WaveFrontSynchro" in bad[0] and "multiple" in bad[1] and "SliceSegmentMode 2" in bad[2]


@pytest.mark.parametrize("path", sg.CASES, **IDS)
def test_fixture_records_under_the_sanitizers(harness, path, tmp_path):
    """The host coder and the access-unit assembly over the fixture's records with its segment layout, each access unit in an allocation of exactly its length: no
    sanitizer report, the two ways to an access unit agree, and the bytes are the reference's stream of the --SAO=0 run (the program has no SAO parameters)."""
    import hevcdl_amd
    c = sg.Case(path)
    c.records(hevcdl_amd.REC_DTYPE).tofile(tmp_path / "records.bin")
    got = harness(["records %s %s %s %d" % (tmp_path / "records.bin", tmp_path / "stream.bin", layout_words(c.w, c.h, c.qp, c.wavefront, c.tiles, c.slices, c.segments), c.nf)])
    assert got[0].split()[:2] == ["ok", str(len(c.dependent))]
    assert (tmp_path / "stream.bin").read_bytes() == sg.strip_sei(c.stream_nosao)


def test_synthetic_and_garbage_records_under_the_sanitizers(harness):
    """Shapes the fixtures do not have (a segment a row at 2 x 23 CTUs, 22 x 20 tiles' worth of headers is out of reach of a quick test: 4 x 3 tiles), layouts the writer
    refuses, and records of random bytes: the coder reads any record safely and the writer's allocations hold."""
    got = harness(["synth %s 2 1 0" % layout_words(128, 1472, 30, wavefront=True, segments=(1, 2)), "synth %s 1 2 0" % layout_words(128, 1472, 30, wavefront=True, segments=(1, 6)),
                   "synth %s 1 3 0" % layout_words(1024, 192, 35, tiles=(4, 3), segments=(3, 1)), "synth %s 1 4 0" % layout_words(1024, 192, 35, tiles=(4, 3), slices=(3, 5), segments=(3, 2)),
                   "synth %s 1 5 0" % layout_words(64, 192, 37, wavefront=True, segments=(1, 1)), "synth %s 1 6 0" % layout_words(264, 136, 22, wavefront=True),
                   "synth %s 2 7 1" % layout_words(264, 136, 32, wavefront=True, segments=(1, 5)), "synth %s 1 8 1" % layout_words(512, 128, 32, tiles=(2, 2), segments=(3, 3)),
                   "synth %s 1 9 1" % layout_words(512, 128, 32, tiles=(2, 2), slices=(3, 2), segments=(3, 1)), "synth %s 1 10 1" % layout_words(64, 192, 32, wavefront=True, segments=(1, 1)),
                   "synth %s 1 11 0" % layout_words(264, 136, 32, segments=(1, 5)), "synth %s 1 11 0" % layout_words(264, 136, 32, wavefront=True, segments=(2, 5))])
    # slice NAL units: 23 rows; ceil(23 / 3); 12 tiles; slices of 5 + 5 + 2 tiles in segments of two: 3 + 3 + 1; 3 CTUs; no segments
    assert [g.split()[:2] for g in got[:6]] == [["ok", "23"], ["ok", "8"], ["ok", "12"], ["ok", "7"], ["ok", "3"], ["ok", "1"]]
    assert [g.split()[:2] for g in got[6:10]] == [["ok", "3"], ["ok", "2"], ["ok", "4"], ["ok", "3"]]
    assert got[10:] == ["status 1", "status 2"]


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason="reference decoder build (oracle/_ref) only exists where the reference's sources are")
@pytest.mark.parametrize("path", sg.CASES, **IDS)
def test_reference_decoder_verifies_the_librarys_streams(oracle_built, path, tmp_path):
    """The streams the LIBRARY writes for the fixture (with the hash SEI of the final picture) through the reference decoder: every picture's MD5 verifies and the
    decoded pictures are the fixture's."""
    import hevcdl_amd
    c = sg.Case(path)
    dbk, _, final = filtered(c)
    for (aus, _), pics, name in zip(library_streams(c), (final, dbk), ("sao", "nosao")):
        (tmp_path / (name + ".bin")).write_bytes(b"".join(au + hevcdl_amd.picture_hash_sei(c.w, c.h, pics[poc], c.bd) for poc, au in enumerate(aus)))
        r = subprocess.run([REF_DEC, "-b", name + ".bin", "-o", name + ".yuv"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ERROR" not in r.stdout and r.stdout.count("(OK)") == c.nf, r.stdout[-800:]
        assert np.array_equal(np.fromfile(tmp_path / (name + ".yuv"), np.uint8), pics.reshape(-1))


@pytest.fixture(scope="module")
def app():
    import hevcdl_amd
    return hevcdl_amd.build_app()


def print_config(app, args, cwd):
    r = subprocess.run([app] + args + ["--PrintConfig"], cwd=cwd, capture_output=True, text=True, timeout=600)
    return r.returncode, json.loads(r.stdout)


def test_cli_segment_keys(app, lib, tmp_path):
    """--PrintConfig shows the two keys; the argument is read only beside a mode; what the library refuses is an error with the library's reason."""
    import hevcdl_amd
    cfg = os.path.join(GOLD, "encoder_intra_main.cfg")
    size = ["-wdt", "320", "-hgt", "256", "-i", "in.yuv"]
    rc, c = print_config(app, ["-c", cfg] + size, tmp_path)
    assert rc == 0 and c["errors"] == [] and (c["SliceSegmentMode"], c["SliceSegmentArgument"]) == (0, 0)
    rc, c = print_config(app, ["-c", cfg] + size + ["--SliceSegmentArgument=7"], tmp_path)
    assert rc == 0 and c["errors"] == [] and (c["SliceSegmentMode"], c["SliceSegmentArgument"]) == (0, 0)
    rc, c = print_config(app, ["-c", cfg] + size + ["--WaveFrontSynchro=1", "--SliceSegmentMode=1", "--SliceSegmentArgument=10"], tmp_path)
    assert rc == 0 and c["errors"] == [] and (c["SliceSegmentMode"], c["SliceSegmentArgument"]) == (1, 10)
    tiled = ["-c", cfg, "-wdt", "512", "-hgt", "128", "-i", "in.yuv", "--NumTileColumnsMinus1=1", "--NumTileRowsMinus1=1", "--TileUniformSpacing=1"]
    rc, c = print_config(app, tiled + ["--SliceSegmentMode=3", "--SliceSegmentArgument=3"], tmp_path)
    assert rc == 0 and c["errors"] == [] and (c["SliceSegmentMode"], c["SliceSegmentArgument"], c["tiles"]) == (3, 3, [2, 2])
    rc, c = print_config(app, tiled + ["--SliceMode=3", "--SliceArgument=2", "--SliceSegmentMode=3", "--SliceSegmentArgument=1"], tmp_path)
    assert rc == 0 and c["errors"] == [] and (c["SliceMode"], c["SliceArgument"], c["SliceSegmentMode"], c["SliceSegmentArgument"]) == (3, 2, 3, 1)
    w = np.zeros(hevcdl_amd.WEIGHT_FLOATS, np.float32)
    for extra, kw in ((["--SliceSegmentMode=2", "--SliceSegmentArgument=1500"], dict(segments=(2, 1500))),
                      (["--SliceSegmentMode=1", "--SliceSegmentArgument=5"], dict(segments=(1, 5))),
                      (["--SliceSegmentMode=1", "--SliceSegmentArgument=3", "--WaveFrontSynchro=1"], dict(segments=(1, 3), wavefront=True)),
                      (["--SliceSegmentMode=1", "--SliceSegmentArgument=5", "--NumTileRowsMinus1=1", "--TileUniformSpacing=1"], dict(segments=(1, 5), tiles=(1, 2))),
                      (["--SliceSegmentMode=3", "--SliceSegmentArgument=1"], dict(segments=(3, 1))),
                      (["--SliceSegmentMode=1", "--SliceSegmentArgument=5", "--WaveFrontSynchro=1", "--DeblockingFilterMetric=1", "--LoopFilterOffsetInPPS=0"],
                       dict(segments=(1, 5), wavefront=True, deblocking_metric=1, lf_offset_in_pps=False)),
                      (["--SliceSegmentMode=5"], dict(segments=(5, 0)))):
        rc, c = print_config(app, ["-c", cfg] + size + extra, tmp_path)
        h = ctypes.c_void_p()      # the same reason as hevcdl_create's
        kcfg = hevcdl_amd.default_config(320, 256, 32, **kw)
        assert lib.hevcdl_create(ctypes.byref(kcfg), w.ctypes.data, w.size, ctypes.byref(h)) in (1, 2)
        why = lib.hevcdl_create_error().decode()
        assert rc == 2 and why and why in " ".join(c["errors"]), (extra, c["errors"], why)


def test_python_front_ends_take_and_refuse_segments():
    import inspect
    import hevcdl_amd
    import hevcdl_amd.pipeline as pipeline
    assert "segments" in inspect.signature(pipeline.encode_sequence).parameters and "segments" in inspect.signature(hevcdl_amd.Encoder.__init__).parameters
    assert hevcdl_amd.segment_layout(None) is None and hevcdl_amd.segment_layout((0, 9)) is None
    lay = hevcdl_amd.segment_layout((1, 10))
    assert (lay.mode, lay.argument) == (1, 10) and ctypes.sizeof(lay) == 8
    cfg = hevcdl_amd.default_config(320, 256, 32, wavefront=True, segments=(1, 10))
    assert (cfg.slice_segment_mode, cfg.slice_segment_argument) == (1, 10) and ctypes.sizeof(cfg) == cfg.struct_size
    with pytest.raises(ValueError, match="does not code slice segments"):
        pipeline.encode_sequence_tile_sharded("none.yuv", 512, 128, 32, 1, (2, 2), segments=(3, 1))
