"""A QP per CU on the device: the cuqp_* fixtures through hevcdl_slice_decode_kernel with the QP map, the QP-map instantiations of
hevcdl_recon_kernel and hevcdl_deblock_fused_kernel, and whole hevcdl_decode_stream with the switch of the context (hevcdl_enable_cu_qp) against the reference decoder's
pictures.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD
from test_cu_qp import NAMES, RUNS, fixture, parsed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", NAMES)
def test_device_parse_equals_the_parser(name):
    """hevcdl_parse_stream_dev_qp == hevcdl_parse_stream_qp on the three streams of every fixture: records, SAO blocks and the QP map, which the kernel writes."""
    import hevcdl_amd
    for run in RUNS:
        a = parsed(name, run)
        b = hevcdl_amd.parse_stream(fixture(name)["stream_" + run].tobytes(), cu_qp=True, engine="device")
        assert a.qp_map.tobytes() == b.qp_map.tobytes() and a.records.tobytes() == b.records.tobytes() and a.sao.tobytes() == b.sao.tobytes() and a.qps == b.qps


@pytest.mark.parametrize("name,run,bit,ctu", [("act_d0_r12", "nolf", 743, 5), ("maxdqp", "dbk", 748, 1)])
def test_device_parse_names_the_ctu_of_a_delta_out_of_range(name, run, bit, ctu):
    import hevcdl_amd
    s = bytearray(fixture(name)["stream_" + run].tobytes())
    s[bit >> 3] ^= 0x80 >> (bit & 7)
    with pytest.raises(hevcdl_amd.HevcdlError) as e:
        hevcdl_amd.parse_stream(bytes(s), cu_qp=True, engine="device")
    assert e.value.status == 1 and "picture 0, CTU %d: CuQpDeltaVal outside its range" % ctu in str(e.value)


@pytest.mark.parametrize("name", NAMES)
def test_reconstruction_kernel_with_a_map(name):
    """the QP-map instantiation of hevcdl_recon_kernel over every filters-off stream: the reference decoder's pictures, and the launch counted as one of the QP-map instantiation."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    p = parsed(name, "nolf")
    before = lib.hevcdl_recon_qp_launches()
    got = hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info, device=0)
    assert np.array_equal(got, fixture(name)["picture_nolf"]) and lib.hevcdl_recon_qp_launches() == before + 1


@pytest.mark.parametrize("name", NAMES)
def test_deblocking_with_a_qp_per_edge(name):
    """The QP-map instantiation of hevcdl_deblock_fused_kernel, at 8 and at 10 bits: the host reconstruction of every deblock-only stream, filtered on the device with its
    map, its PPS chroma offsets and its pictures' slice-header parameters, is the reference decoder's picture."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    p = parsed(name, "dbk")
    recon = hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info)
    before = lib.hevcdl_deblock_qp_launches()
    with hevcdl_amd.StreamDecoder(fixture(name)["stream_dbk"].tobytes(), batch=len(p.pictures)) as d:
        got = d.deblock_map(recon, p)
    want = fixture(name)["picture_dbk"]
    assert np.array_equal(got, want) and lib.hevcdl_deblock_qp_launches() == before + 1
    if int(fixture(name)["qp"]) >= 22:                                     # (the filter had something to do; at QP 2 beta and tC are 0 and it has not)
        assert not np.array_equal(recon, want)


@pytest.mark.parametrize("device_parse", [False, True], ids=["host_parse", "device_parse"])
@pytest.mark.parametrize("name", NAMES)
def test_whole_decode_of_the_default_cfg_streams(name, device_parse):
    """hevcdl_decode_stream with the switch on, parsed on the host and on the device: the reference decoder's pictures, every digest of the device equal to the SEI's."""
    import hevcdl_amd
    pictures, _, info, verdicts = hevcdl_amd.decode_stream(fixture(name)["stream_full"].tobytes(), device_parse=device_parse, cu_qp=True)
    assert np.array_equal(pictures, fixture(name)["picture_full"]) and verdicts == [True] * len(info)
    assert [p.qp for p in info] == [int(q) for q in fixture(name)["slice_qps_full"]]


def test_a_changed_digest_turns_exactly_its_pictures_verdict():
    import hevcdl_amd
    s = bytearray(fixture("rc_lcu")["stream_full"].tobytes())
    s[-3] ^= 0x55                                                             # inside the last picture's digest
    pictures, _, _, verdicts = hevcdl_amd.decode_stream(bytes(s), cu_qp=True)
    assert verdicts == [True, True, False] and np.array_equal(pictures, fixture("rc_lcu")["picture_full"])


@pytest.mark.parametrize("name", ["aq_d2", "b10_off"], ids=["8bit", "10bit"])
def test_cli_decodes_such_streams(tmp_path, name):
    """bin/TAppDecoderHevcdl enables the switch always: the reference decoder's file, a line a picture with the slice QP and (OK)."""
    import hevcdl_amd
    f = fixture(name)
    (tmp_path / "s.bin").write_bytes(f["stream_full"].tobytes())
    r = subprocess.run([hevcdl_amd.build_decoder_app(), "-b", "s.bin", "-o", "rec.yuv"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("(OK)") == int(f["n_frames"]) and "ERROR" not in r.stdout, (r.stdout[-600:], r.stderr[-600:])
    assert (tmp_path / "rec.yuv").read_bytes() == f["picture_full"].tobytes()
    assert all("QP %2d" % q in r.stdout for q in f["slice_qps_full"])


@pytest.mark.parametrize("name", ["rc_lcu", "rc_pic"])
def test_a_batch_of_pictures_with_different_slice_qps_equals_single_launches(name):
    """The three pictures of a rate-controlled stream (another slice QP each) in one launch per stage, against a launch per picture."""
    import hevcdl_amd
    s = fixture(name)["stream_full"].tobytes()
    assert len(set(int(q) for q in fixture(name)["slice_qps_full"])) == 3
    for device_parse in (False, True):
        whole, _, _, v3 = hevcdl_amd.decode_stream(s, batch=3, device_parse=device_parse, cu_qp=True)
        single, _, _, v1 = hevcdl_amd.decode_stream(s, batch=1, device_parse=device_parse, cu_qp=True)
        assert np.array_equal(whole, single) and np.array_equal(whole, fixture(name)["picture_full"]) and v3 == v1 == [True] * 3


def test_the_switch_is_turned_on_and_off_between_calls_on_one_context():
    """One context: refused while off (status, the parser's sentence, nothing else changed), decoded once on, refused again once off, decoded again -- with host parse and
    with device parse; a constant-QP stream of the same size decodes the same either way."""
    import hevcdl_amd
    s = fixture("aq_d2")["stream_full"].tobytes()
    want = fixture("aq_d2")["picture_full"]
    with hevcdl_amd.StreamDecoder(s, batch=2) as d:
        for device_parse in (False, True):
            d.enable_device_parse(device_parse)
            for on in (False, True, False, True):
                d.enable_cu_qp(on)
                if on:
                    pictures, _, verdicts = d.decode(s)
                    assert np.array_equal(pictures, want) and verdicts == [True, True]
                else:
                    with pytest.raises(hevcdl_amd.HevcdlError) as e:
                        d.decode(s, n=2)
                    assert e.value.status == 2 and "cu_qp_delta_enabled_flag is outside this decoder" in str(e.value)


def test_a_constant_qp_stream_takes_the_same_launches_with_the_switch_on():
    """An existing fixture decoded with the switch off and on: the same pictures and verdicts, the same number of reconstruction launches, none of a QP-map instantiation."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    s = np.load(os.path.join(GOLD, "rd_w200_q27_r2.npz"))["bitstream"].tobytes()
    counts = []
    out = []
    for on in (False, True):
        c0 = (lib.hevcdl_recon_launches(), lib.hevcdl_recon_qp_launches(), lib.hevcdl_deblock_qp_launches(), lib.hevcdl_slice_decode_launches())
        out.append(hevcdl_amd.decode_stream(s, cu_qp=on))
        c1 = (lib.hevcdl_recon_launches(), lib.hevcdl_recon_qp_launches(), lib.hevcdl_deblock_qp_launches(), lib.hevcdl_slice_decode_launches())
        counts.append(tuple(b - a for a, b in zip(c0, c1)))
    assert counts[0] == counts[1] and counts[0][1] == 0 and counts[0][2] == 0 and counts[0][0] >= 1
    assert np.array_equal(out[0][0], out[1][0]) and out[0][3] == out[1][3] and all(v is True for v in out[0][3])
    # and a stream that needs the map does launch them
    c0 = (lib.hevcdl_recon_qp_launches(), lib.hevcdl_deblock_qp_launches())
    hevcdl_amd.decode_stream(fixture("aq_d2")["stream_full"].tobytes(), cu_qp=True)
    assert (lib.hevcdl_recon_qp_launches() - c0[0], lib.hevcdl_deblock_qp_launches() - c0[1]) == (1, 1)
