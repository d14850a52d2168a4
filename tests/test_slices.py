"""Slices on the host (no GPU): SliceMode 1 over whole CTU rows, SliceMode 3 over tiles.  The fixtures are runs of the reference encoder (tools/gen_slice_fixtures.py);
the writer -- one slice NAL unit per slice, the shared slice-data coder ending a sub-stream as a slice's last -- must give the reference's streams byte for byte."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import rd_plan_cases
import slices_cases as sc
from conftest import GOLD, ROOT

REF_DEC = os.path.join(ROOT, "oracle", "_ref", "TAppDecoder_ref")
IDS = dict(ids=sc.case_id)


@pytest.fixture(scope="module")
def lib():
    import hevcdl_amd
    return hevcdl_amd.load_library()


_sao_cache = {}


def filtered(c):
    """(SAO parameters or None, final pictures) of the oracle's in-loop filters on the fixture's records and unfiltered reconstruction, on the EQUIVALENT TILE GRID:
    computed once a fixture and shared."""
    if c.name not in _sao_cache:
        import ref_tools
        tiles, lf = c.grid()
        pic = c.prefilter()
        if not c.lf_disable:
            pic = ref_tools.run_deblock(pic, c.w, c.h, c.qp, c.records(ref_tools.REC_DTYPE), bit_depth=c.bd, tiles=tiles, lf_across_tiles=lf, lf_offsets=c.offsets)
        params = None
        if c.sao:
            params, pic = ref_tools.run_sao(c.yuv, pic, c.w, c.h, c.qp, tiles=tiles, bit_depth=c.bd, lf_across_tiles=lf)
        _sao_cache[c.name] = (params, np.asarray(pic, c.dt).reshape(c.nf, c.fs))
    return _sao_cache[c.name]


def stream_cfg(c, sao):
    """The stream configuration of the fixture's run: its own tiles (none for SliceMode 1) -- the slices are the layout's."""
    import hevcdl_amd
    return hevcdl_amd.stream_config(c.w, c.h, c.qp, sao=sao, tiles=c.tiles, bit_depth=c.bd, lf_across_tiles=c.lf_tiles, tools=c.tools, lf_offsets=c.offsets, lf_disable=c.lf_disable)


def test_the_fixture_set_is_the_generators():
    assert {sc.case_id(p) for p in sc.CASES} == sc.EXPECTED
    for p in sc.CASES:
        assert os.path.getsize(p) < 320 * 1024, p      # under the tile fixtures' sizes (rd_t*: up to 385 KB)


@pytest.mark.parametrize("path", sc.CASES, **IDS)
def test_fixtures_satisfy_the_generators_assertions(path):
    """The number of slice NAL units per access unit; another stream than the one-slice run of the same frames; every slice but the first carries its address."""
    c = sc.Case(path)
    units = c.cx * c.cy if c.mode == 1 else c.tiles[0] * c.tiles[1]
    assert c.n_slices == (units + c.arg - 1) // c.arg > 1
    assert sc.slice_nals(c.stream) == [c.n_slices] * c.nf
    one = c.f["bitstream_one_slice"].tobytes()
    assert one != c.stream and sc.slice_nals(one) == [1] * c.nf
    firsts = [n[2] >> 7 for _, n in sc.split_annexb(c.stream) if ((n[0] >> 1) & 63) <= 21]      # first_slice_segment_in_pic_flag
    assert firsts == ([1] + [0] * (c.n_slices - 1)) * c.nf
    assert len([l for l in c.f["stdout"] if str(l).startswith("POC")]) == c.nf


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason="reference decoder build (oracle/_ref) only exists where the reference's sources are")
@pytest.mark.parametrize("path", sc.CASES, **IDS)
def test_reference_decoder_returns_the_reconstruction_file(path, tmp_path):
    c = sc.Case(path)
    (tmp_path / "s.bin").write_bytes(c.stream)
    r = subprocess.run([REF_DEC, "-b", "s.bin", "-o", "dec.yuv"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stdout and r.stdout.count("(OK)") == c.nf, r.stdout[-800:]
    assert np.array_equal(np.fromfile(tmp_path / "dec.yuv", c.dt), c.final.reshape(-1))


@pytest.mark.parametrize("path", sc.CASES, **IDS)
def test_writer_gives_the_reference_stream(oracle_built, path):
    """Records and SAO parameters (the oracle's, on the equivalent tile grid: its final picture is the reference's reconstruction file) through the writer with the slice
    layout: the reference's stream byte for byte, hash SEI included; hevcdl_access_unit_bound_slices is not exceeded."""
    import hevcdl_amd
    c = sc.Case(path)
    params, final = filtered(c)
    assert np.array_equal(final, c.final)
    recs = c.records(hevcdl_amd.REC_DTYPE)
    layout = hevcdl_amd.slice_layout(c.slices, c.lf_slices)
    bound = hevcdl_amd.load_library().hevcdl_access_unit_bound_slices(c.w, c.h, ctypes.byref(layout))
    aus = []
    for poc in range(c.nf):
        au = hevcdl_amd.write_access_unit(c.w, c.h, c.qp, poc, recs[poc], sao=params[poc].view(hevcdl_amd.SAO_DTYPE) if c.sao else None, tiles=c.tiles, bit_depth=c.bd,
                                          lf_across_tiles=c.lf_tiles, tools=c.tools, lf_offsets=c.offsets, lf_disable=c.lf_disable, choice=c.choice(), slices=c.slices,
                                          lf_across_slices=c.lf_slices)
        assert len(au) <= bound
        aus.append(au)
    assert b"".join(aus) == sc.strip_sei(c.stream)
    assert [au + hevcdl_amd.picture_hash_sei(c.w, c.h, final[poc], c.bd) for poc, au in enumerate(aus)] == sc.access_units(c.stream)
    # the picture's bit count of the reference's log is the access unit without the SEI (TEncGOP.cpp:2422-2448)
    bits = [int(str(l).split(")")[1].split("bits")[0]) for l in c.f["stdout"] if str(l).startswith("POC")]
    assert bits == [8 * len(au) for au in aus]


@pytest.mark.parametrize("path", sc.CASES, **IDS)
def test_slice_data_coded_apart_gives_the_same_stream(oracle_built, path):
    """hevcdl_code_slice_data_host_slices + hevcdl_write_access_unit_from_slice_data_slices: in SliceMode 1 one sub-stream per slice, in SliceMode 3 one per tile."""
    import hevcdl_amd
    c = sc.Case(path)
    params, _ = filtered(c)
    cfg = stream_cfg(c, c.sao)
    layout = hevcdl_amd.slice_layout(c.slices, c.lf_slices)
    buf, sizes, ovf, off, cap = hevcdl_amd.code_slice_data(cfg, c.records(hevcdl_amd.REC_DTYPE), params.view(hevcdl_amd.SAO_DTYPE) if c.sao else None, layout=layout)
    assert sizes.shape == (c.nf, c.n_slices if c.mode == 1 else c.tiles[0] * c.tiles[1]) and not ovf.any()
    for k in range(sizes.shape[1]):      # nothing but the regions is written
        assert (buf[:, int(off[k]) + int(cap[k]):int(off[k]) + int(cap[k]) + 64] == hevcdl_amd.CANARY).all()
    aus = [hevcdl_amd.write_access_unit_from_slice_data(cfg, poc, hevcdl_amd.pack_slice_data(buf[poc], sizes[poc], off), sizes[poc], c.choice(), layout=layout) for poc in range(c.nf)]
    assert b"".join(aus) == sc.strip_sei(c.stream)


def test_a_null_layout_and_mode_0_are_the_functions_they_were():
    """A one-slice picture of the reference (tests/golden/rd_c128_q27_r.npz, its run with --SAO=0) through the new entry points with a NULL layout and with a layout of
    mode 0: the reference's stream, which is what the old names give; bound and slice-data layout are the old ones too."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    f = np.load(os.path.join(GOLD, "rd_c128_q27_r.npz"))
    w, h, qp, nf = int(f["width"]), int(f["height"]), int(f["qp"]), f["records"].shape[0]
    recs = np.frombuffer(f["records"].tobytes(), dtype=hevcdl_amd.REC_DTYPE).reshape(nf, -1)
    want = sc.strip_sei(f["bitstream_nosao"].tobytes())
    assert b"".join(hevcdl_amd.write_access_unit(w, h, qp, poc, recs[poc]) for poc in range(nf)) == want and sc.slice_nals(want) == [1] * nf
    cfg = hevcdl_amd.stream_config(w, h, qp)
    cap = lib.hevcdl_access_unit_bound(w, h)
    for layout in (None, hevcdl_amd.SliceLayout(0, 1500, 0)):      # (the default cfg's SliceArgument 1500 and a cleared flag beside SliceMode 0: not looked at)
        lp = ctypes.byref(layout) if layout is not None else None
        got = b""
        for poc in range(nf):
            buf, n = np.zeros(cap, np.uint8), ctypes.c_size_t(0)
            assert lib.hevcdl_write_access_unit_slices(ctypes.byref(cfg), lp, poc, recs[poc].ctypes.data, None, None, buf.ctypes.data, cap, ctypes.byref(n)) == 0
            got += buf[:n.value].tobytes()
        assert got == want
        assert lib.hevcdl_access_unit_bound_slices(w, h, lp) == cap
        b0, s0, o0, _, _ = hevcdl_amd.code_slice_data(cfg, recs)
        b1, s1, o1, _, _ = hevcdl_amd.code_slice_data(cfg, recs, layout=layout)
        assert b0.tobytes() == b1.tobytes() and np.array_equal(s0, s1) and not o0.any() and not o1.any()
        assert b"".join(hevcdl_amd.write_access_unit_from_slice_data(cfg, poc, hevcdl_amd.pack_slice_data(b1[poc], s1[poc], hevcdl_amd.slice_data_layout(cfg)[2]), s1[poc], layout=layout)
                        for poc in range(nf)) == want


def test_writer_refuses_layouts_it_cannot_write(lib):
    import hevcdl_amd
    recs = np.zeros(6, hevcdl_amd.REC_DTYPE)

    def status(cfg, layout):
        cap = 1 << 16
        buf, n = np.zeros(cap, np.uint8), ctypes.c_size_t(0)
        return lib.hevcdl_write_access_unit_slices(ctypes.byref(cfg), ctypes.byref(layout), 0, recs.ctypes.data, None, None, buf.ctypes.data, cap, ctypes.byref(n))
    plain = hevcdl_amd.stream_config(192, 128, 32)                         # 3 x 2 CTUs
    assert status(plain, hevcdl_amd.SliceLayout(1, 3, 1)) == 0
    assert status(plain, hevcdl_amd.SliceLayout(2, 1500, 1)) == 2          # slices by bytes: HEVCDL_ERR_UNSUPPORTED
    for bad in ((1, 0), (1, 2), (1, 4), (3, 1), (4, 1), (-1, 1)):          # no positive multiple of the width; SliceMode 3 without tiles; no mode
        assert status(plain, hevcdl_amd.SliceLayout(bad[0], bad[1], 1)) == 1, bad
    assert status(hevcdl_amd.stream_config(192, 128, 32, wavefront=True), hevcdl_amd.SliceLayout(1, 3, 1)) == 1
    tall = hevcdl_amd.stream_config(64, 64 * 23, 32)                       # 23 rows of one CTU: more than 22 slices
    recs = np.zeros(23, hevcdl_amd.REC_DTYPE)
    assert status(tall, hevcdl_amd.SliceLayout(1, 1, 1)) == 1 and status(tall, hevcdl_amd.SliceLayout(1, 2, 1)) == 0
    recs = np.zeros(16, hevcdl_amd.REC_DTYPE)
    tiled = hevcdl_amd.stream_config(512, 128, 32, tiles=(2, 2))
    assert status(tiled, hevcdl_amd.SliceLayout(3, 3, 1)) == 0 and status(tiled, hevcdl_amd.SliceLayout(3, 0, 1)) == 1 and status(tiled, hevcdl_amd.SliceLayout(1, 8, 1)) == 1


REFUSALS = [      # (keyword arguments of default_config, status, a word of the reason)
    (dict(slices=(2, 1500)), 2, "SliceMode 2"),
    (dict(slices=(1, 0)), 2, "multiple of the picture's width"),
    (dict(slices=(1, 3)), 2, "multiple of the picture's width"),                      # five CTUs wide: 3 is no whole row
    (dict(slices=(1, 5), tiles=(1, 2)), 2, "together with tiles"),
    (dict(slices=(1, 5), wavefront=True), 2, "WaveFrontSynchro"),
    (dict(slices=(3, 1)), 1, "needs tiles"),
    (dict(slices=(3, 0), tiles=(1, 2)), 1, "at least 1 tile"),
    (dict(slices=(1, 5), deblocking_metric=1, lf_offset_in_pps=False), 2, "DeblockingFilterMetric"),
    (dict(slices=(3, 1), tiles=(1, 2), deblocking_metric=2, lf_offset_in_pps=False), 2, "DeblockingFilterMetric"),
    (dict(slices=(3, 2), tiles=(1, 2), lf_across_slices=False), 2, "LFCrossSliceBoundaryFlag 0"),      # borders inside a slice crossed, borders between slices not
    (dict(slices=(4, 1)), 1, "SliceMode is 0, 1 or 3"),
]


@pytest.mark.parametrize("kw,status,word", REFUSALS, ids=[r[2].replace(" ", "-") + "-%d" % i for i, r in enumerate(REFUSALS)])
def test_create_refuses_with_a_status_and_a_reason(lib, kw, status, word):
    """hevcdl_create checks the slice keys before it looks for a device: the refusals need no GPU."""
    import hevcdl_amd
    cfg = hevcdl_amd.default_config(320, 256, 32, **kw)       # 5 x 4 CTUs
    w = np.zeros(hevcdl_amd.WEIGHT_FLOATS, np.float32)
    h = ctypes.c_void_p()
    assert lib.hevcdl_create(ctypes.byref(cfg), w.ctypes.data, w.size, ctypes.byref(h)) == status
    assert word in lib.hevcdl_create_error().decode()


def test_create_refuses_more_than_22_row_slices_and_accepts_what_it_should(lib):
    import hevcdl_amd
    w = np.zeros(hevcdl_amd.WEIGHT_FLOATS, np.float32)

    def create(cfg):
        h = ctypes.c_void_p()
        st = lib.hevcdl_create(ctypes.byref(cfg), w.ctypes.data, w.size, ctypes.byref(h))
        if st == 0:
            lib.hevcdl_destroy(h)
        return st, lib.hevcdl_create_error().decode()
    st, why = create(hevcdl_amd.default_config(64, 64 * 23, 32, slices=(1, 1)))
    assert st == 2 and "at most 22 slices" in why
    # what is valid gets past the slice keys: a context (on a GPU), or the loud failure for want of a device -- never a reason
    for cfg in (hevcdl_amd.default_config(64, 64 * 23, 32, slices=(1, 2)), hevcdl_amd.default_config(128, 128, 32, slices=(1, 2)),
                hevcdl_amd.default_config(512, 128, 32, tiles=(2, 2), slices=(3, 3)), hevcdl_amd.default_config(512, 128, 32, tiles=(2, 2), slices=(3, 1), lf_across_slices=False),
                hevcdl_amd.default_config(320, 256, 32, slices=(0, 1500), lf_across_slices=False)):
        st, why = create(cfg)
        assert st in (0, 3) and why == ""
    tail = hevcdl_amd.default_config(128, 128, 32)             # a zeroed tail is SliceMode 0
    tail.slice_mode = tail.slice_argument = tail.lf_across_slices = 0
    assert create(tail)[0] in (0, 3)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/slices_harness.cpp + csrc/hevcdl_bitstream.cpp under the host compiler's sanitizers (a stand-alone program: nothing is loaded into this process)."""
    import hevcdl_amd
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host g++")
    csrc = os.path.join(hevcdl_amd.PKG_DIR, "csrc")
    exe = str(tmp_path_factory.mktemp("slices") / "slices_harness")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "slices_harness.cpp"), os.path.join(csrc, "hevcdl_bitstream.cpp"), "-o", exe]
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


def test_slice_context_plans_like_the_tile_context_of_its_grid(harness):
    """csrc/slice_grid.h turns the slice keys into the grid hevcdl_create hands to the launch plan; that plan must be the plan of the tile context with the same grid
    (one column, explicit row heights), launch for launch, over the frame counts of tests/rd_plan_cases.py -- at 2160p (34 rows: 17 slices of two rows, 6 of six) and on a
    picture too narrow for tiles."""
    with open(os.path.join(GOLD, "rd_launch_forms.json")) as f:
        rec = json.load(f)
    waves = " ".join(str(rec["waves"][b]) for b in rd_plan_cases.BUILDS)
    counts = sorted({c["n_frames"] for c in rec["cases"] if c["call"] == "frames"} | {1, 75})
    asked, lines = [], []
    for w, h, rows in ((3840, 2160, 2), (3840, 2160, 6), (3840, 2160, 17), (128, 320, 1), (128, 320, 4)):
        cx, cy = (w + 63) // 64, (h + 63) // 64
        heights = [min(rows, cy - r) for r in range(0, cy, rows)]
        pad = lambda v: " ".join(str(x) for x in (list(v) + [0] * 21)[:21])
        for n in counts:
            head = "plan %d %s %d %d %d" % (rec["cus"], waves, w, h, max(counts))
            lines.append("%s 1 %d 1 %s %d" % (head, rows * cx, pad([]), n))                             # the slice context
            lines.append("%s 0 0 %d %s %d" % (head, len(heights), pad(heights[:-1]), n))               # the tile context with the same grid
            asked.append((w, h, rows, n, len(heights)))
    got = harness(lines)
    forms = set()
    for i, (w, h, rows, n, units) in enumerate(asked):
        a, b = got[2 * i], got[2 * i + 1]
        assert a == b and not a.startswith("status"), (w, h, rows, n, a, b)
        assert "units=%d" % (n * units) in a and a.endswith("1 x %d rows%s" % (units, "".join(" %d" % rows for _ in range(units - 1)))), a
        forms.add(a.split("\t")[1].split(" form=")[1].split(" ")[0].split("(")[0])
    assert len(forms) >= 2, forms      # the counts reach more than one launch form
    # and the refusals arrive through the same function
    head = "plan %d %s 3840 2160 8" % (rec["cus"], waves)
    bad = harness(["%s 1 60 1 %s 1" % (head, pad([])), "%s 1 90 1 %s 1" % (head, pad([])), "%s 2 1500 1 %s 1" % (head, pad([]))])
    assert [b.split("\t")[0] for b in bad] == ["status 2"] * 3 and "22 slices" in bad[0] and "multiple" in bad[1] and "SliceMode 2" in bad[2]


def test_writer_on_synthetic_records_under_the_sanitizers(harness):
    """The new writer's paths on synthetic record sets, each access unit in an allocation of exactly its length: no sanitizer report, the two ways to an access unit
    agree, the bound holds, the NAL unit counts are the layouts'."""
    got = harness(["write 128 128 32 1 2 1 1 1 2 1", "write 192 200 27 1 6 0 1 1 2 2", "write 64 192 37 1 1 1 1 1 2 3", "write 512 128 32 3 3 1 2 2 2 4",
                   "write 512 128 32 3 1 0 2 2 1 5", "write 264 136 22 1 5 1 1 1 1 6", "write 128 128 32 0 0 1 1 1 1 7", "write 64 1408 40 1 1 1 1 1 1 8",
                   "write 128 128 32 1 3 1 1 1 1 9", "write 128 128 32 2 100 1 1 1 1 9"])
    assert [g.split()[:2] for g in got[:8]] == [["ok", "2"], ["ok", "2"], ["ok", "3"], ["ok", "2"], ["ok", "4"], ["ok", "3"], ["ok", "1"], ["ok", "22"]]
    assert got[8:] == ["status 1", "status 2"]


@pytest.fixture(scope="module")
def app():
    import hevcdl_amd
    return hevcdl_amd.build_app()


def print_config(app, args, cwd):
    r = subprocess.run([app] + args + ["--PrintConfig"], cwd=cwd, capture_output=True, text=True, timeout=600)
    return r.returncode, json.loads(r.stdout)


def test_cli_slice_keys(app, tmp_path):
    """--PrintConfig shows the three keys; the default cfg (SliceMode 0 beside SliceArgument 1500) still passes and its two other keys stay without effect; what the
    library refuses is an error with its reason."""
    cfg = os.path.join(GOLD, "encoder_intra_main.cfg")
    size = ["-wdt", "320", "-hgt", "256", "-i", "in.yuv"]
    rc, c = print_config(app, ["-c", cfg] + size, tmp_path)
    assert rc == 0 and c["errors"] == [] and (c["SliceMode"], c["SliceArgument"], c["LFCrossSliceBoundaryFlag"]) == (0, 0, 1)
    rc, c = print_config(app, ["-c", cfg] + size + ["--LFCrossSliceBoundaryFlag=0"], tmp_path)
    assert rc == 0 and (c["SliceMode"], c["SliceArgument"], c["LFCrossSliceBoundaryFlag"]) == (0, 0, 1)
    rc, c = print_config(app, ["-c", cfg] + size + ["--SliceMode=1", "--SliceArgument=10", "--LFCrossSliceBoundaryFlag=0"], tmp_path)
    assert rc == 0 and c["errors"] == [] and (c["SliceMode"], c["SliceArgument"], c["LFCrossSliceBoundaryFlag"]) == (1, 10, 0)
    rc, c = print_config(app, ["-c", cfg, "-wdt", "512", "-hgt", "128", "-i", "in.yuv", "--SliceMode=3", "--SliceArgument=3", "--NumTileColumnsMinus1=1", "--NumTileRowsMinus1=1",
                               "--TileUniformSpacing=1"], tmp_path)
    assert rc == 0 and c["errors"] == [] and (c["SliceMode"], c["SliceArgument"], c["tiles"]) == (3, 3, [2, 2])
    for extra, needle in ((["--SliceMode=2"], "SliceMode = 2"), (["--SliceMode=1", "--SliceArgument=0"], "multiple of the picture's width"),
                          (["--SliceMode=1", "--SliceArgument=3"], "multiple of the picture's width"),
                          (["--SliceMode=1", "--SliceArgument=5", "--WaveFrontSynchro=1"], "WaveFrontSynchro"), (["--SliceMode=3", "--SliceArgument=1"], "needs tiles"),
                          (["--SliceMode=1", "--SliceArgument=5", "--DeblockingFilterMetric=1", "--LoopFilterOffsetInPPS=0"], "DeblockingFilterMetric"),
                          (["--SliceMode=5"], "SliceMode = 5")):
        rc, c = print_config(app, ["-c", cfg] + size + extra, tmp_path)
        assert rc == 2 and needle in " ".join(c["errors"]), (extra, c["errors"])


def test_python_front_ends_take_and_refuse_slices():
    import inspect
    import hevcdl_amd
    import hevcdl_amd.pipeline as pipeline
    assert {"slices", "lf_across_slices"} <= set(inspect.signature(pipeline.encode_sequence).parameters)
    assert hevcdl_amd.slice_layout(None) is None and hevcdl_amd.slice_layout((0, 1500)) is None
    lay = hevcdl_amd.slice_layout((1, 10), False)
    assert (lay.mode, lay.argument, lay.lf_across_slices) == (1, 10, 0)
    src = inspect.getsource(pipeline.encode_sequence_tile_sharded)
    assert "does not code slices" in src      # (the refusal itself stands in front of torch.distributed: exercised below)
    with pytest.raises(ValueError, match="does not code slices"):
        pipeline.encode_sequence_tile_sharded("none.yuv", 512, 128, 32, 1, (2, 2), slices=(3, 1))
