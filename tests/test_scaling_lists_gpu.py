"""Scaling lists on the device: the scaling-list instantiation of hevcdl_recon_kernel against the reference decoder's pictures and against the host
form, and whole hevcdl_decode_stream with the switch of the context (hevcdl_enable_scaling_lists), with host parse and with device parse.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD
from test_scaling_lists import NAMES, fixture, parsed

pytestmark = pytest.mark.gpu

SENTENCE = "scaling lists are outside this decoder"


@pytest.mark.parametrize("name", ["one_ctu", "edge_q45", "file_rand", "file_steep_b10", "tskip", "cuqp"])
def test_reconstruction_kernel_with_scaling_lists(name):
    """The smallest shapes that hold every TU size, both sample types, a padded edge, transform skip and the QP map: the reference decoder's filters-off pictures, and the
    launch counted as one of the scaling-list instantiation and none of the QP-map one."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    p = parsed(name, "nolf")
    before = (lib.hevcdl_recon_sl_launches(), lib.hevcdl_recon_qp_launches(), lib.hevcdl_recon_launches())
    got = hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info, scaling=p.scaling, device=0)
    after = (lib.hevcdl_recon_sl_launches(), lib.hevcdl_recon_qp_launches(), lib.hevcdl_recon_launches())
    assert np.array_equal(got, fixture(name)["picture_nolf"])
    assert tuple(b - a for a, b in zip(before, after)) == (1, 0, 1)


def extreme_records(small):
    """One 64x64 CTU, levels of +-32767 everywhere: four 32x32 luma blocks with their 16x16 chroma blocks, or (small) 4x4 blocks, every other 8x8 CU transform-skipped."""
    import hevcdl_amd
    r = np.zeros((1, 1), hevcdl_amd.REC_DTYPE)
    z = np.arange(256)
    r["depth"][0, 0] = 3 if small else 0
    r["tr_idx"][0, 0] = 1
    r["luma_dir"][0, 0] = np.where(z & 4, 26, 1) if small else 1
    r["chroma_dir"][0, 0] = 1
    r["cbf"][0, 0] = 3
    r["tskip"][0, 0] = ((z >> 2) & 1) if small else 0
    i = np.arange(4096)
    r["coeff_y"][0, 0] = np.where((i * 7) & 8, 32767, -32767)
    r["coeff_cb"][0, 0] = np.where(i[:1024] & 1, -32767, 32767)
    r["coeff_cr"][0, 0] = np.where(i[:1024] & 2, 32767, -32767)
    return r


@pytest.mark.parametrize("bit_depth", [8, 10])
@pytest.mark.parametrize("high", [False, True], ids=["lowest_qp", "qp51"])
@pytest.mark.parametrize("small", [False, True], ids=["32x32", "4x4"])
def test_kernel_equals_the_host_form_on_synthetic_extremes(bit_depth, high, small):
    """Levels of +-32767 under factors of 1 and 255 side by side, at QpY 51 with chroma offsets of +12 and at the lowest QpY of the bit depth with -12: the 16-bit clip of
    8.6.4.2 is reached whatever the reference reaches (level * 255 * 72 << 10 needs the 64-bit product).  The kernel gives what the host form gives."""
    import hevcdl_amd
    import scaling_list_cover as slc
    cfg = hevcdl_amd.stream_config(64, 64, 26, bit_depth=bit_depth)
    r = extreme_records(small)
    hevcdl_amd.validate_records(cfg, r)
    i = np.arange(2032)
    sc = hevcdl_amd.scaling_info(np.where((i ^ (i >> 3)) & 1, 255, 1))
    qi = hevcdl_amd.QpInfo(0, 0, 12 if high else -12, 12 if high else -12)
    qp_map = np.full((1, 1, 256), 51 if high else -6 * (bit_depth - 8), np.int8)
    host = hevcdl_amd.reconstruct_frames(cfg, r, qp_map=qp_map, qp_info=qi, scaling=sc)
    dev = hevcdl_amd.reconstruct_frames(cfg, r, qp_map=qp_map, qp_info=qi, scaling=sc, device=0)
    assert np.array_equal(host, dev)
    assert host.max() == (1 << bit_depth) - 1 and host.min() == 0

    class P:
        pass
    p = P()
    p.cfg, p.records, p.qp_map, p.qp_info, p.scaling_factors = cfg, r, qp_map, qi, np.frombuffer(bytes(sc.factor), np.uint8)
    if high or bit_depth == 8:
        assert slc.coverage(p)["clip"] >= 1


def test_a_batch_of_pictures_of_different_slice_qps_equals_single_launches():
    """Pictures of five streams of one size and four slice QPs (17, 22, 27, and the per-CU QPs of the cuqp case) under one factor block: one launch over the batch against a
    launch per picture and against the host form."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    ps = [parsed(n, "nolf") for n in ("file_rand", "default", "wpp", "file_pred", "cuqp")]
    assert len({(p.cfg.width, p.cfg.height) for p in ps}) == 1 and len({q for p in ps for q in p.qps}) >= 3
    recs, qmap = np.concatenate([p.records for p in ps]), np.concatenate([p.qp_map for p in ps])
    cfg, sc, qi = ps[0].cfg, ps[0].scaling, ps[-1].qp_info
    before = lib.hevcdl_recon_sl_launches()
    whole = hevcdl_amd.reconstruct_frames(cfg, recs, qp_map=qmap, qp_info=qi, scaling=sc, device=0)
    assert lib.hevcdl_recon_sl_launches() == before + 1
    single = np.concatenate([hevcdl_amd.reconstruct_frames(cfg, recs[k:k + 1], qp_map=qmap[k:k + 1], qp_info=qi, scaling=sc, device=0) for k in range(recs.shape[0])])
    assert np.array_equal(whole, single)
    assert np.array_equal(whole, hevcdl_amd.reconstruct_frames(cfg, recs, qp_map=qmap, qp_info=qi, scaling=sc))


@pytest.mark.parametrize("name", NAMES)
def test_device_parse_entry_point_equals_the_parser(name):
    """hevcdl_parse_stream_dev_sl == hevcdl_parse_stream_sl: records, SAO blocks, the QP map the kernel writes (a constant one for a stream of one QP), the factor block."""
    import hevcdl_amd
    a = parsed(name, "full")
    b = hevcdl_amd.parse_stream(fixture(name)["stream_full"].tobytes(), cu_qp=True, scaling_lists=True, engine="device")
    assert a.qp_map.tobytes() == b.qp_map.tobytes() and a.records.tobytes() == b.records.tobytes() and a.sao.tobytes() == b.sao.tobytes() and a.qps == b.qps
    assert np.array_equal(a.scaling_factors, b.scaling_factors) and b.scaling.enabled == 1


@pytest.mark.parametrize("device_parse", [False, True], ids=["host_parse", "device_parse"])
@pytest.mark.parametrize("name", NAMES)
def test_whole_decode_of_the_default_cfg_streams(name, device_parse):
    """hevcdl_decode_stream with the switch on (and hevcdl_enable_cu_qp where the stream needs it), parsed on the host and on the device: the reference decoder's pictures
    of the default cfg (deblocking and SAO), every digest of the device equal to the SEI's; the deblock-only streams likewise."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    for run in ("full", "dbk"):
        before = (lib.hevcdl_recon_sl_launches(), lib.hevcdl_recon_qp_launches(), lib.hevcdl_deblock_qp_launches())
        pictures, _, info, verdicts = hevcdl_amd.decode_stream(fixture(name)["stream_" + run].tobytes(), device_parse=device_parse, cu_qp=name == "cuqp", scaling_lists=True)
        after = (lib.hevcdl_recon_sl_launches(), lib.hevcdl_recon_qp_launches(), lib.hevcdl_deblock_qp_launches())
        assert np.array_equal(pictures, fixture(name)["picture_" + run]) and verdicts == [True] * len(info)
        assert [p.qp for p in info] == [int(q) for q in fixture(name)["slice_qps_" + run]]
        assert tuple(b - a for a, b in zip(before, after)) == (1, 0, 1 if name == "cuqp" else 0)      # the QP-map deblocking only where the QP varies


def test_a_changed_digest_turns_exactly_its_pictures_verdict():
    import hevcdl_amd
    s = bytearray(fixture("file_rand")["stream_full"].tobytes())
    s[-3] ^= 0x55                                                             # inside the last picture's digest
    pictures, _, _, verdicts = hevcdl_amd.decode_stream(bytes(s), scaling_lists=True)
    assert verdicts == [True, False] and np.array_equal(pictures, fixture("file_rand")["picture_full"])


@pytest.mark.parametrize("name", ["cuqp", "file_steep_b10"], ids=["8bit", "10bit"])
def test_cli_decodes_such_streams(tmp_path, name):
    """bin/TAppDecoderHevcdl enables the switch always: the reference decoder's file, a line a picture with the slice QP and (OK)."""
    import hevcdl_amd
    f = fixture(name)
    (tmp_path / "s.bin").write_bytes(f["stream_full"].tobytes())
    r = subprocess.run([hevcdl_amd.build_decoder_app(), "-b", "s.bin", "-o", "rec.yuv"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("(OK)") == int(f["n_frames"]) and "ERROR" not in r.stdout, (r.stdout[-600:], r.stderr[-600:])
    assert (tmp_path / "rec.yuv").read_bytes() == f["picture_full"].tobytes()
    assert all("QP %2d" % q in r.stdout for q in f["slice_qps_full"])


def test_the_switch_and_the_launch_counter_on_one_context():
    """One context (192x128, 8 bits), host parse and device parse: a stream with lists is refused while the switch is off -- status, the parser's sentence, nothing launched --
    and decoded once it is on; off again it is refused again and the next call is correct.  A flat stream on the enabled context decodes as ever and leaves
    hevcdl_recon_sl_launches where it was.  A stream with lists and cu_qp_delta needs both switches and is refused with the missing one's sentence."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    s, want = fixture("file_rand")["stream_full"].tobytes(), fixture("file_rand")["picture_full"]
    both, want_both = fixture("cuqp")["stream_full"].tobytes(), fixture("cuqp")["picture_full"]
    flat = np.load(os.path.join(GOLD, "cuqp_chroma_off.npz"))      # 192x128, chroma offsets only: with cu_qp on, a stream without lists of this size
    with hevcdl_amd.StreamDecoder(s, batch=2) as d:
        for device_parse in (False, True):
            d.enable_device_parse(device_parse)
            for on in (False, True, False, True):
                d.enable_scaling_lists(on)
                c0 = (lib.hevcdl_recon_launches(), lib.hevcdl_recon_sl_launches())
                if on:
                    pictures, _, verdicts = d.decode(s)
                    assert np.array_equal(pictures, want) and verdicts == [True, True]
                    assert (lib.hevcdl_recon_launches() - c0[0], lib.hevcdl_recon_sl_launches() - c0[1]) == (1, 1)
                else:
                    with pytest.raises(hevcdl_amd.HevcdlError) as e:
                        d.decode(s, n=2)
                    assert e.value.status == 2 and SENTENCE in str(e.value)
                    assert (lib.hevcdl_recon_launches(), lib.hevcdl_recon_sl_launches()) == c0
            # enabled: a stream without lists takes the launches it always took
            d.enable_cu_qp(True)
            c0 = (lib.hevcdl_recon_launches(), lib.hevcdl_recon_sl_launches(), lib.hevcdl_recon_qp_launches())
            pictures, _, verdicts = d.decode(flat["stream_full"].tobytes())
            assert np.array_equal(pictures, flat["picture_full"]) and all(verdicts)
            assert (lib.hevcdl_recon_launches() - c0[0], lib.hevcdl_recon_sl_launches() - c0[1], lib.hevcdl_recon_qp_launches() - c0[2]) == (1, 0, 1)
            # lists and cu_qp_delta: both switches, or the missing one's sentence
            pictures, _, verdicts = d.decode(both)
            assert np.array_equal(pictures, want_both) and verdicts == [True, True]
            for sl_on, qp_on, sentence in ((True, False, "cu_qp_delta_enabled_flag is outside this decoder"), (False, True, SENTENCE)):
                d.enable_scaling_lists(sl_on)
                d.enable_cu_qp(qp_on)
                c0 = lib.hevcdl_recon_launches()
                with pytest.raises(hevcdl_amd.HevcdlError) as e:
                    d.decode(both, n=2)
                assert e.value.status == 2 and sentence in str(e.value) and lib.hevcdl_recon_launches() == c0
            d.enable_cu_qp(False)
            d.enable_scaling_lists(True)
            pictures, _, verdicts = d.decode(s)                      # the next call on the context is correct
            assert np.array_equal(pictures, want) and verdicts == [True, True]


def test_a_constant_qp_stream_takes_the_same_launches_with_the_switch_on():
    """An existing fixture decoded with the switch off and on: the same pictures and verdicts, the same launches, none of the scaling-list or a QP-map instantiation."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    s = np.load(os.path.join(GOLD, "rd_w200_q27_r2.npz"))["bitstream"].tobytes()
    counts, out = [], []
    for on in (False, True):
        c0 = (lib.hevcdl_recon_launches(), lib.hevcdl_recon_sl_launches(), lib.hevcdl_recon_qp_launches(), lib.hevcdl_deblock_qp_launches(), lib.hevcdl_slice_decode_launches())
        out.append(hevcdl_amd.decode_stream(s, scaling_lists=on))
        c1 = (lib.hevcdl_recon_launches(), lib.hevcdl_recon_sl_launches(), lib.hevcdl_recon_qp_launches(), lib.hevcdl_deblock_qp_launches(), lib.hevcdl_slice_decode_launches())
        counts.append(tuple(b - a for a, b in zip(c0, c1)))
    assert counts[0] == counts[1] and counts[0][1:4] == (0, 0, 0) and counts[0][0] >= 1
    assert np.array_equal(out[0][0], out[1][0]) and out[0][3] == out[1][3] and all(v is True for v in out[0][3])
