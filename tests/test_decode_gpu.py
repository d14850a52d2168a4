"""The stream parser's output as INPUT of the device on the MI355X: a reference-encoder stream is parsed on the host (csrc/hevcdl_parse.cpp), its records and SAO parameters
are coded again by the device entropy coder (csrc/entropy_kernel.hip) under the layouts the parser named, and the access units around that slice data are the stream's
bytes again.  What the parser hands on is therefore complete and exact for the one device stage that consumes records and SAO parameters as a stream describes them.
Every picture is a few CTUs."""
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu

TIME_LIMIT = 60                                                           # seconds a test; each takes well under one


@pytest.fixture(autouse=True)
def own_time_limit():
    """Every test here runs under its own time limit.  A launch that never returns sits in native code, where no Python-level alarm is served: the watchdog thread of
    faulthandler dumps the stacks and ends the process when the limit passes; a test that returns in time disarms it.  The limit ends the WHOLE pytest process, not the one
    test: the tests behind a hang get no verdict.  On a shared GPU that is meant -- nothing more is started on a device that a kernel has just hung."""
    import faulthandler
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()

# tiny and edge sizes, both extremes of QP, 10 bits, every tool off, tiles, wavefront rows, row slices at 10 bits, wavefront segments, tile segments inside tile slices,
# deblocking parameters in the slice header
CASES = [("rd_e8x8_q32", "bitstream"), ("rd_e64x8_q20", "bitstream"), ("rd_e8x72_q40", "bitstream"), ("rd_e136_q0", "bitstream_nosao"), ("rd_e136_q51", "bitstream"),
         ("rd_e72_q0_b10", "bitstream"), ("rd_k200_q27_all0", "bitstream"), ("rd_t512_q32_2x2", "bitstream"), ("rd_w64_q32_r", "bitstream"), ("rd_w200_q27_r2", "bitstream"),
         ("slices_r128_a2_b10", "bitstream"), ("segments_w264x136_a5", "bitstream"), ("segments_t512x128_s2_a1", "bitstream"), ("dbksel_m1_104x72_q37_off", "bitstream")]


@pytest.mark.parametrize("name,key", CASES, ids=[c[0] for c in CASES])
def test_device_coder_writes_the_parsed_stream_again(name, key):
    import hevcdl_amd
    stream = np.load(os.path.join(GOLD, name + ".npz"))[key].tobytes()
    p = hevcdl_amd.parse_stream(stream)
    assert hevcdl_amd.validate_records(p.cfg, p.records) is None
    out = []
    for i, pic in enumerate(p.pictures):
        cfg = hevcdl_amd.StreamConfig.from_buffer_copy(bytes(p.cfg))
        cfg.qp = pic.qp
        sao = p.sao[i:i + 1] if pic.sao else None
        buf, sizes, ovf, off, cap = hevcdl_amd.code_slice_data(cfg, p.records[i:i + 1], sao, device=0, layout=p.slices, segments=p.segments)
        assert not ovf.any()
        out.append(hevcdl_amd.write_access_unit_from_slice_data(cfg, pic.poc if pic.nal_type == 21 else 0, hevcdl_amd.pack_slice_data(buf[0], sizes[0], off), sizes[0],
                                                                choice=pic.dbk if pic.dbk.override_enabled else None, layout=p.slices, segments=p.segments))
        if pic.hash_method:
            out.append(hevcdl_amd.hash_sei(*p.digest(i)))
    assert b"".join(out) == stream


# the second in-loop filter as a decoder runs it: tiny and edge sizes, 10 bits, tiles with the filters stopping at their borders (lf0) and crossing them, wavefront,
# a 10-bit picture of several tiles, two pictures a call
SAO_CASES = ["rd_e8x8_q32", "rd_e64x8_q20", "rd_e8x72_q40", "rd_e136_q51", "rd_e72_q0_b10", "rd_k200_q27_all0", "rd_t512_q32_2x2", "rd_l576_q32_lf0", "rd_l520_q27_lf0_b10",
             "rd_w200_q27_r2", "rd_x576_q30_2x3"]


@pytest.mark.parametrize("name", SAO_CASES)
def test_sao_with_the_streams_parameters_gives_the_reference_picture(name):
    """hevcdl_sao_apply_frames: the reference's deblocked pictures + the SAO parameters the parser reads out of the reference's stream (merges unresolved, as coded) ->
    the reference's final pictures, byte for byte.  No original and no decision runs: the apply kernels alone."""
    import hevcdl_amd
    from conftest import fixture_tiles, fixture_lf
    f = np.load(os.path.join(GOLD, name + ".npz"))
    w, h, qp, nf = int(f["width"]), int(f["height"]), int(f["qp"]), f["records"].shape[0]
    bd = int(f["bit_depth"]) if "bit_depth" in f.files else 8
    dt = np.uint8 if bd == 8 else np.dtype("<u2")
    fb = w * h * 3 // 2
    dbk = np.frombuffer(f["recon_deblocked"].tobytes(), dt).reshape(nf, fb)
    final = np.frombuffer(f["recon_filtered"].tobytes(), dt).reshape(nf, fb)
    p = hevcdl_amd.parse_stream(f["bitstream"].tobytes())
    assert all(pic.sao for pic in p.pictures)
    e = hevcdl_amd.Encoder(w, h, qp, max_frames=nf, tiles=fixture_tiles(f), bit_depth=bd, lf_across_tiles=fixture_lf(f))
    try:
        out = e.sao_apply_frames(dbk, p.sao)
        assert np.array_equal(out, final)
        # parameters a stream cannot carry are refused before anything is launched
        for field, value in (("mode", 3), ("type", 5), ("aux", 32)):
            bad = p.sao.copy()
            bad["mode"][0, 0, 0] = 1                                      # (the picture's first CTU: no merge)
            bad[field][0, 0, 0] = value
            with pytest.raises(hevcdl_amd.HevcdlError) as err:
                e.sao_apply_frames(dbk, bad)
            assert err.value.status == 1
        bad = np.zeros_like(p.sao)
        bad["mode"][0, 0, 0] = 2                                          # a merge to the left in the picture's first CTU
        with pytest.raises(hevcdl_amd.HevcdlError):
            e.sao_apply_frames(dbk, bad)
        _, rows, _, _, rb = hevcdl_amd.tile_layout(fixture_tiles(f), w, h)
        if rows > 1:                                                      # a merge upwards out of the first CTU of the second tile row: no such flag exists in sao()
            bad = np.zeros_like(p.sao)
            bad["mode"][0, rb[1] * ((w + 63) // 64), 0], bad["type"][0, rb[1] * ((w + 63) // 64), 0] = 2, 1
            with pytest.raises(hevcdl_amd.HevcdlError) as err:
                e.sao_apply_frames(dbk, bad)
            assert err.value.status == 1 and "border" in str(err.value)
    finally:
        e.close()
