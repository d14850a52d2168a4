"""The picture report on the device (csrc/report_kernel.hip + the SSE kernel of csrc/quality_kernel.hip): every plane case of tests/test_report.py through the kernels,
hevcdl_picture_report against the host's hevcdl_picture_hash and a numpy SSE, the picture pipeline with nothing but slice data leaving HBM, and the CLI key.  Everything is
exact: there is no tolerance in this file."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import report_cases as rc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("method", [1, 2, 3], ids=["md5", "crc", "checksum"])
def test_planes_equal_the_host_instantiation(method):
    """MD5 tails, chunk boundaries (the default chunk: planes of 16383, 16384, 16385 and 32771 bytes), checksum positions, 1 x 1; random, all-zero and all-maximal samples."""
    import hevcdl_amd
    cases = rc.all_planes()
    assert len(cases) > 150
    for name, plane, bd in cases:
        assert hevcdl_amd.plane_hash(plane, bd, method) == hevcdl_amd.plane_hash_host(plane, bd, method), name


def sse_of(org, pic, w, h):
    d = (org.astype(np.int64) - pic.astype(np.int64)) ** 2
    ysz = w * h
    return [int(d[:ysz].sum()), int(d[ysz:ysz + ysz // 4].sum()), int(d[ysz + ysz // 4:].sum())]


def check_records(recs, org, pics, w, h, bd, method):
    import hevcdl_amd
    for i in range(pics.shape[0]):
        assert (int(recs[i]["method"]), int(recs[i]["plane_bytes"])) == (method, hevcdl_amd.HASH_BYTES.get(method, 0))
        if method:
            assert hevcdl_amd.report_digest(recs[i]) == hevcdl_amd.picture_hash(w, h, pics[i], bd, method), (i, method)
        assert not recs[i]["digest"][3 * int(recs[i]["plane_bytes"]):].any()
        assert recs[i]["sse"].tolist() == (sse_of(org[i], pics[i], w, h) if org is not None else [0, 0, 0]), i


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size,n", [((8, 8), 2), ((16, 8), 1), ((16, 8), 3), ((16, 8), 65), ((16, 8), 130), ((72, 40), 2), ((520, 8), 2), ((8, 520), 2)],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "n%d" % v)
def test_picture_report(size, n, bd):
    """65 pictures cross a wave's 64 lanes in the MD5 kernel, 130 take a third wave."""
    import hevcdl_amd
    w, h = size
    org, pics = rc.picture(w, h, bd, seed=w + h + n, n=n), rc.picture(w, h, bd, seed=w + h + n + 1, n=n)
    if n >= 65:
        pics[1] = pics[0]; pics[64] = pics[0]; org[1] = org[0]; org[64] = org[0]      # the same picture at positions 0, 1 and 64 of the batch
    enc = hevcdl_amd.Encoder(w, h, 32, max_frames=n, bit_depth=bd)
    try:
        for method in (1, 2, 3):
            recs = enc.picture_report(org, pics, method)
            check_records(recs, org, pics, w, h, bd, method)
            if n >= 65:
                assert recs[0].tobytes() == recs[1].tobytes() == recs[64].tobytes()
        check_records(enc.picture_report(None, pics, 2), None, pics, w, h, bd, 2)          # no originals: sse stays 0
        none = enc.picture_report(org, pics, 0)                                            # method 0: the digest stays zero
        check_records(none, org, pics, w, h, bd, 0)
        assert not none["digest"].any()
        out = np.zeros(n, hevcdl_amd.REPORT_DTYPE)
        for bad in (-1, 4):
            assert enc.lib.hevcdl_picture_report(enc._h, org.ctypes.data, pics.ctypes.data, n, bad, out.ctypes.data) == 1
    finally:
        enc.close()


def test_device_entry_point_writes_nothing_but_its_records():
    """hevcdl_picture_report_dev on device buffers: a pattern in front of and behind the records is intact, an output inside the pictures is refused."""
    import torch
    import hevcdl_amd
    w, h, n, bd = 72, 40, 5, 8
    org, pics = rc.picture(w, h, bd, seed=3, n=n), rc.picture(w, h, bd, seed=4, n=n)
    enc = hevcdl_amd.Encoder(w, h, 32, max_frames=n)
    try:
        d_org, d_pic = torch.from_numpy(org).cuda(), torch.from_numpy(pics).cuda()
        guard = 256
        d_out = torch.full((guard + 80 * n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        for method in (1, 2, 3):
            d_out.fill_(0xA5)
            enc.picture_report_dev(d_org.data_ptr(), d_pic.data_ptr(), n, method, d_out.data_ptr() + guard)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert (got[:guard] == 0xA5).all() and (got[guard + 80 * n:] == 0xA5).all()
            check_records(np.frombuffer(got[guard:guard + 80 * n].tobytes(), hevcdl_amd.REPORT_DTYPE), org, pics, w, h, bd, method)
        with pytest.raises(hevcdl_amd.HevcdlError) as err:
            enc.picture_report_dev(d_org.data_ptr(), d_pic.data_ptr(), n, 1, d_pic.data_ptr() + 64)
        assert err.value.status == 1
        assert torch.equal(d_pic.cpu(), torch.from_numpy(pics)) and torch.equal(d_org.cpu(), torch.from_numpy(org))
    finally:
        enc.close()


@pytest.mark.parametrize("name", ["c192_q32_r2", "w200_q30_b10"])
def test_pipeline_reports_without_downloading_pictures(name):
    """encode_pictures_stream(want_pictures=False) with device entropy and the report on: the reports (read inside the callback and after the call) are the SSE and the
    hevcdl_picture_hash of the pictures a second call hands out with want_pictures=True."""
    import hevcdl_amd
    from conftest import fixture_wavefront
    f = np.load(os.path.join(GOLD, "rd_%s.npz" % name))
    w, h, qp, n = int(f["width"]), int(f["height"]), int(f["qp"]), f["yuv"].shape[0]
    bd = int(f["bit_depth"]) if "bit_depth" in f.files else 8
    yuv = f["yuv"].astype(rc.dtype_of(bd))
    enc = hevcdl_amd.Encoder(w, h, qp, max_frames=n, bit_depth=bd, wavefront=fixture_wavefront(f))
    try:
        with pytest.raises(hevcdl_amd.HevcdlError) as err:
            enc.get_picture_report(0, 1)
        assert err.value.status == 1                                   # switch off: HEVCDL_ERR_INVALID_ARG
        enc.enable_device_entropy(True)
        for method in (1, 2, 3):
            enc.enable_picture_report(True, method)
            inside = []
            chunks = enc.encode_pictures_stream(yuv, f["labels"], want_pictures=False, chunk_frames=1, on_chunk_hook=lambda first, count: inside.append(enc.get_picture_report(first, count)))
            assert all(c[4] is None and c[5] is None for c in chunks) and len(chunks) == n      # the callback's pictures_opt is NULL
            recs = enc.get_picture_report(0, n)
            assert np.concatenate(inside).tobytes() == recs.tobytes()
            again = enc.encode_pictures_stream(yuv, f["labels"], want_pictures=True)
            pics = np.concatenate([c[4] for c in again])
            assert [c[1] for c in again][0][:1] == chunks[0][1][:1]                              # the same slice data either way
            check_records(recs, yuv, pics, w, h, bd, method)
            assert pics.tobytes() == f["recon_filtered"].tobytes()                               # and they are the reference's pictures
        enc.enable_picture_report(False)
        with pytest.raises(hevcdl_amd.HevcdlError):
            enc.get_picture_report(0, 1)
        enc.encode_pictures_stream(yuv, f["labels"])                                             # the pipeline runs on without the report
    finally:
        enc.close()


def test_encode_sequence_with_device_report(tmp_path):
    """pipeline.encode_sequence(device_report=True): stream (hash SEI included) and rows of the run without it -- with device entropy and no reconstruction file the batch
    goes through encode_pictures_stream(want_pictures=False)."""
    import ref_tools
    from hevcdl_amd import pipeline
    w, h, n = 200, 136, 3
    ref_tools.synth_yuv(w, h, n, seed=19).tofile(tmp_path / "in.yuv")
    outs = []
    for entropy, report, recon in ((False, False, True), (False, True, True), (True, True, False)):
        b, r = str(tmp_path / ("s%d%d.bin" % (entropy, report))), str(tmp_path / ("s%d%d.yuv" % (entropy, report)))
        _, rows = pipeline.encode_sequence(str(tmp_path / "in.yuv"), w, h, 32, n, b, r if recon else None, hash_sei=True, device_entropy=entropy, device_report=report, log=lambda *a: None)
        outs.append((open(b, "rb").read(), np.asarray(rows).tolist(), open(r, "rb").read() if recon else None))
    assert outs[0][:2] == outs[1][:2] == outs[2][:2] and outs[0][2] == outs[1][2] and len(outs[0][0]) > 500


def _label_files(tmp_path, labels):
    for fr in range(labels.shape[0]):
        os.makedirs(tmp_path / "pred" / str(fr))
        for a in range(labels.shape[1]):
            (tmp_path / "pred" / str(fr) / ("ctu%d.txt" % a)).write_text(" ".join(str(int(v)) for v in labels[fr, a]))


@pytest.mark.parametrize("fixture,method,extra", [("rd_c192_q32_r2", 1, []), ("stream_c192_q32", 2, ["--SAO=0"]), ("stream_c192_q32", 3, ["--SAO=0"]), ("rd_c192_q32_r2", 1, ["--Devices=0,0", "--PrintMSSSIM=1"])],
                         ids=["md5", "crc", "checksum", "md5_devices_msssim"])
def test_cli_device_report_changes_no_output(fixture, method, extra, tmp_path):
    """--DeviceReport=1, alone and with --DeviceEntropy=1: the stream bytes, the reconstruction file and every log line up to [ET (and the digests behind it) are those of
    the run without the key; the stream is the reference's where the fixture holds it."""
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    f = np.load(os.path.join(GOLD, fixture + ".npz"))
    w, h, qp, n = int(f["width"]), int(f["height"]), int(f["qp"]), f["yuv"].shape[0]
    f["yuv"].astype(np.uint8).tofile(tmp_path / "in.yuv")
    _label_files(tmp_path, f["labels"])
    outs = []
    runs = [("plain", []), ("report", ["--DeviceReport=1"]), ("both", ["--DeviceEntropy=1", "--DeviceReport=1"])]
    if extra and extra[0].startswith("--Devices"):
        runs = [runs[0], runs[2]]
    nofile = method != 1                                   # the CRC / checksum cases name no reconstruction file in their last run: that run fetches no picture at all
    for tag, keys in runs:
        files = ["-b", tag + ".bin"] + ([] if nofile and tag == "both" else ["-o", tag + ".yuv"])
        t0 = time.perf_counter()
        r = subprocess.run([app, "-i", "in.yuv", "-wdt", str(w), "-hgt", str(h), "-q", str(qp), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=%d" % method] + files + extra + keys,
                           cwd=tmp_path, capture_output=True, text=True, timeout=300)
        print("%s: %.2f s" % (tag, time.perf_counter() - t0))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        lines = r.stdout.splitlines()
        at = [i for i, ln in enumerate(lines) if ln.startswith("SUMMARY")]
        log = [re.sub(r"\[ET[^\]]*\]", "", ln) for ln in lines if ln.startswith("POC")] + lines[at[0]:at[0] + 4]
        assert sum(ln.startswith("POC") for ln in log) == n and all(("[MD5:", "[CRC:", "[Checksum:")[method - 1] in ln for ln in log[:n])
        outs.append(((tmp_path / (tag + ".bin")).read_bytes(), log, (tmp_path / (tag + ".yuv")).read_bytes() if (tmp_path / (tag + ".yuv")).exists() else None))
    for o in outs[1:]:
        assert o[0] == outs[0][0] and o[1] == outs[0][1] and (o[2] is None or o[2] == outs[0][2])
    assert outs[0][2] is not None and (outs[-1][2] is None) == nofile
    want = {1: "bitstream", 2: "bitstream_crc", 3: "bitstream_sum"}[method]
    assert outs[0][0] == f[want].tobytes()
