"""Slices on the device: a SliceMode 1 context runs its row slices as a unit grid of one column through the decision, deblocking, SAO and entropy kernels; a SliceMode 3
context is the tile context with another stream.  Every picture here is a few CTUs."""
import os
import re
import subprocess

import numpy as np
import pytest

import quality_ref as qr
import slices_cases as sc

pytestmark = pytest.mark.gpu
IDS = dict(ids=sc.case_id)
FIELDS = ["depth", "part_size", "luma_dir", "chroma_dir", "tr_idx", "cbf", "tskip", "bits", "dist", "cost", "coeff_y", "coeff_cb", "coeff_cr"]


def encoder(c, exec_flags=0, **kw):
    import hevcdl_amd
    cfg = hevcdl_amd.default_config(c.w, c.h, c.qp, max_frames=c.nf, tiles=c.tiles, bit_depth=c.bd, lf_across_tiles=c.lf_tiles, tools=c.tools, lf_offsets=c.offsets,
                                    lf_offset_in_pps=c.in_pps, slices=c.slices, lf_across_slices=c.lf_slices, **kw)
    cfg.exec_flags = exec_flags
    return hevcdl_amd.Encoder(c.w, c.h, c.qp, cfg=cfg)


def same_records(got, want):
    return [k for k in FIELDS if not np.array_equal(got[k], want[k])]


# every fixture with the build the launch plan picks, and the 8-bit reference-tools fixtures -- the contexts that have two builds -- once with each forced
BUILDS = [(p, 0) for p in sc.CASES] + [(sc.path_of(n), f) for n in ("r192x200_a6", "c64x192_a1", "t512_a3") for f in (2, 4)]      # HEVCDL_EXEC_RD_WIDE, HEVCDL_EXEC_RD_NARROW


@pytest.mark.parametrize("path,flags", BUILDS, ids=[sc.case_id(p) + {0: "", 2: "-wide", 4: "-narrow"}[f] for p, f in BUILDS])
def test_decisions_are_the_references(path, flags):
    """hevcdl_compress_frames on the slice context: the reference's records and unfiltered reconstruction behind every compressCtu, exactly."""
    import hevcdl_amd
    c = sc.Case(path)
    e = encoder(c, flags)
    try:
        recs, recon, _ = e.compress_frames(c.yuv, c.labels)
        launch = (e.lib.hevcdl_last_rd_launch(e._h) or b"").decode()
    finally:
        e.close()
    assert same_records(recs, c.records(hevcdl_amd.REC_DTYPE)) == []
    assert np.array_equal(recon, c.prefilter())
    want_build = {0: None, 2: "hevcdl_rd_frame_kernel_wide ", 4: "hevcdl_rd_frame_kernel "}[flags]
    assert want_build is None or launch.startswith(want_build), launch
    assert "units=%d" % (c.nf * (c.n_slices if c.mode == 1 else c.tiles[0] * c.tiles[1])) in launch, launch      # every slice (tile) a unit of the launch


def stream_of(c, recs, sao, choices):
    import hevcdl_amd
    return b"".join(hevcdl_amd.write_access_unit(c.w, c.h, c.qp, poc, recs[poc], sao=sao[poc] if c.sao else None, tiles=c.tiles, bit_depth=c.bd, lf_across_tiles=c.lf_tiles,
                                                 tools=c.tools, lf_offsets=c.offsets, lf_disable=c.lf_disable, choice=choices[poc] if not c.in_pps else None, slices=c.slices,
                                                 lf_across_slices=c.lf_slices) for poc in range(c.nf))


@pytest.mark.parametrize("path", sc.CASES, **IDS)
def test_picture_pipeline_gives_the_reconstruction_file_and_the_stream(path):
    """hevcdl_encode_pictures: the reference's reconstruction file, and through the writer its stream; with device entropy on, the slice data of the same call through
    hevcdl_write_access_unit_from_slice_data_slices gives the stream too."""
    import hevcdl_amd
    c = sc.Case(path)
    e = encoder(c)
    try:
        e.enable_device_entropy(True)
        recs, final, sao, _ = e.encode_pictures(c.yuv, c.labels, deblock=not c.lf_disable, sao=c.sao)
        choices = e.get_dbk_choice(0, c.nf)
        data, sizes = e.get_slice_data(0, c.nf)
        fallbacks = e.entropy_info()[0]
        layout = e.slice_layout
    finally:
        e.close()
    assert np.array_equal(final, c.final)
    want = sc.strip_sei(c.stream)
    assert stream_of(c, recs, sao, choices) == want
    assert fallbacks == 0 and sizes.shape == (c.nf, c.n_slices if c.mode == 1 else c.tiles[0] * c.tiles[1])
    scfg = hevcdl_amd.stream_config(c.w, c.h, c.qp, sao=c.sao, tiles=c.tiles, bit_depth=c.bd, lf_across_tiles=c.lf_tiles, tools=c.tools, lf_offsets=c.offsets, lf_disable=c.lf_disable)
    assert (layout.mode, layout.argument, layout.lf_across_slices) == (c.mode, c.arg, int(c.lf_slices))
    got = b"".join(hevcdl_amd.write_access_unit_from_slice_data(scfg, poc, data[poc], sizes[poc], choices[poc] if not c.in_pps else None, layout=layout) for poc in range(c.nf))
    assert got == want


@pytest.mark.parametrize("name", ["r192x200_a6", "t512_a3"])
def test_host_fallback_codes_a_slice_picture(name):
    """A capacity so small that sub-streams overflow their regions: the host codes those pictures with the same coder and the same slice ends; the stream is the same."""
    import hevcdl_amd
    c = sc.Case(sc.path_of(name))
    e = encoder(c)
    try:
        e.set_entropy_capacity(8)
        e.enable_device_entropy(True)
        chunks = e.encode_pictures_stream(c.yuv, c.labels, deblock=True, sao=True)
        choices = e.get_dbk_choice(0, c.nf)
        fallbacks = e.entropy_info()[0]
        layout = e.slice_layout
    finally:
        e.close()
    assert fallbacks >= 1
    scfg = hevcdl_amd.stream_config(c.w, c.h, c.qp, sao=True, tiles=c.tiles, bit_depth=c.bd, lf_across_tiles=c.lf_tiles, tools=c.tools)
    got = b""
    for first, data, sizes, _, _, _ in chunks:
        got += b"".join(hevcdl_amd.write_access_unit_from_slice_data(scfg, first + i, data[i], sizes[i], None, layout=layout) for i in range(len(data)))
    assert got == sc.strip_sei(c.stream)


def test_device_coder_entry_point_with_a_layout():
    """hevcdl_code_slice_data_slices (the kernels on uploaded records) against hevcdl_code_slice_data_host_slices: the same bytes, lengths and untouched gaps, for row
    slices and for slices of tiles."""
    import hevcdl_amd
    for name in ("r264x136_a5_lf0", "t512_a3"):
        c = sc.Case(sc.path_of(name))
        scfg = hevcdl_amd.stream_config(c.w, c.h, c.qp, sao=False, tiles=c.tiles, bit_depth=c.bd, lf_across_tiles=c.lf_tiles, tools=c.tools)
        layout = hevcdl_amd.slice_layout(c.slices, c.lf_slices)
        recs = c.records(hevcdl_amd.REC_DTYPE)
        host = hevcdl_amd.code_slice_data(scfg, recs, layout=layout)
        dev = hevcdl_amd.code_slice_data(scfg, recs, layout=layout, device=0)
        assert np.array_equal(host[1], dev[1]) and not dev[2].any()
        off, cap = dev[3], dev[4]
        for poc in range(c.nf):      # the used bytes (the device rounds a sub-stream's last store up to a dword of zeros: inside its region) and the gaps no coder writes
            assert hevcdl_amd.pack_slice_data(host[0][poc], host[1][poc], off) == hevcdl_amd.pack_slice_data(dev[0][poc], dev[1][poc], off)
            for k in range(len(off)):
                assert (dev[0][poc, int(off[k]) + int(cap[k]):int(off[k]) + int(cap[k]) + 64] == hevcdl_amd.CANARY).all()


def test_row_slices_are_the_tile_rows_on_content_without_a_fixture(oracle_built):
    """Random 256x192 content (4 x 3 CTUs, wide enough for a tile column): the SliceMode 1 context and the tile context with the same grid give identical records,
    reconstruction, SAO parameters and output pictures; lf_across_slices 0 and 1 give different pictures."""
    import hevcdl_amd
    import ref_tools
    w, h, qp, nf = 256, 192, 30, 2
    yuv = ref_tools.synth_yuv(w, h, nf, seed=4242)
    labels = ref_tools.make_labels(w, h, nf, "rand", seed=4242)
    out = {}
    for key, kw in (("slices-lf1", dict(slices=(1, 4), lf_across_slices=True)), ("tiles-lf1", dict(tiles=([4], [1, 1, 1]), lf_across_tiles=True)),
                    ("slices-lf0", dict(slices=(1, 4), lf_across_slices=False)), ("tiles-lf0", dict(tiles=([4], [1, 1, 1]), lf_across_tiles=False))):
        e = hevcdl_amd.Encoder(w, h, qp, max_frames=nf, **kw)
        try:
            pre = e.compress_frames(yuv, labels)
            out[key] = (pre[0], pre[1]) + e.encode_pictures(yuv, labels)[:3]
        finally:
            e.close()
    for lf in ("lf1", "lf0"):
        s, t = out["slices-" + lf], out["tiles-" + lf]
        assert same_records(s[0], t[0]) == [] and np.array_equal(s[1], t[1])                     # compress_frames: records, reconstruction
        assert same_records(s[2], t[2]) == [] and np.array_equal(s[3], t[3]) and s[4].tobytes() == t[4].tobytes()      # the pipeline: records, output pictures, SAO parameters
    assert np.array_equal(out["slices-lf1"][1], out["slices-lf0"][1])                            # the decisions do not depend on the flag
    assert not np.array_equal(out["slices-lf1"][3], out["slices-lf0"][3])                        # the filtered pictures do


def test_per_ctu_session_refuses_a_slice_context():
    import hevcdl_amd
    c = sc.Case(sc.path_of("r128_a2"))
    e = encoder(c)
    try:
        st = e.lib.hevcdl_begin_frames(e._h, np.ascontiguousarray(c.yuv).ctypes.data, 1, None, None)
        why = (e.lib.hevcdl_last_error(e._h) or b"").decode()
    finally:
        e.close()
    assert st == 1 and "slices" in why      # HEVCDL_ERR_INVALID_ARG


def log_of(lines):
    """Picture lines without [ET ...] and the reference build's "nQP <n> ", with their hash text, and the two lines of the summary block."""
    poc = [re.sub(r"nQP -?\d+ ", "", qr.strip_et(l)) + " " + l[l.index("[MD5:"):].strip() for l in lines if l.startswith("POC")]
    i = next(k for k, l in enumerate(lines) if l.startswith("SUMMARY"))
    return poc, [l.rstrip() for l in lines[i + 1:i + 3]]


@pytest.mark.parametrize("name", ["r192x200_a6_lf0", "r128_a2_b10", "r128_a2_inpps0", "t512_a3"])
def test_cli_reproduces_the_reference_run(name, tmp_path):
    """The reference's own keys on the reference's own input: stream, reconstruction file and log lines (the picture's bit count is all its slice NAL units); with
    --DeviceEntropy=1 --DeviceReport=1 the same once more."""
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    c = sc.Case(sc.path_of(name))
    c.yuv.astype(c.dt).tofile(tmp_path / "in.yuv")
    for f in range(c.nf):
        os.makedirs(tmp_path / "pred" / str(f))
        for a in range(c.nctu):
            (tmp_path / "pred" / str(f) / ("ctu%d.txt" % a)).write_text(" ".join(str(int(v)) for v in c.labels[f, a]) + " ")
    base = [app, "-i", "in.yuv", "-wdt", str(c.w), "-hgt", str(c.h), "-q", str(c.qp), "-f", str(c.nf), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=1",
            "--InputBitDepth=%d" % c.bd, "--Profile=%s" % ("main" if c.bd == 8 else "main10")] + [str(k) for k in c.f["keys"]]
    want = log_of([str(l) for l in c.f["stdout"]])
    for tag, extra in (("plain", []), ("device", ["--DeviceEntropy=1", "--DeviceReport=1"])):
        r = subprocess.run(base + ["-b", tag + ".bin", "-o", tag + ".yuv"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert (tmp_path / (tag + ".bin")).read_bytes() == c.stream, tag
        assert (tmp_path / (tag + ".yuv")).read_bytes() == c.f["recon_file"].tobytes(), tag
        assert log_of(r.stdout.splitlines()) == want, tag
