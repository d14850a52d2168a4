"""DeltaQpRD on the device: the sum and keep kernels (csrc/qp_rd_kernel.hip) alone on synthetic pictures, the decision stage and the picture pipelines against runs of
the reference encoder with --DeltaQpRD=N (tests/golden/dqr_*.npz, tools/gen_deltaqprd_fixtures.py), the command line and the Python pipeline.  Every picture is a few CTUs."""
import os
import re
import subprocess

import numpy as np
import pytest

import deltaqprd_cases as dc
import quality_ref as qr

pytestmark = pytest.mark.gpu
IDS = dict(ids=dc.case_id)
FIELDS = ["depth", "part_size", "luma_dir", "chroma_dir", "tr_idx", "cbf", "tskip", "bits", "dist", "cost", "coeff_y", "coeff_cb", "coeff_cr"]


def encoder(c, n=None, **kw):
    import hevcdl_amd
    return hevcdl_amd.Encoder(c.w, c.h, c.qp, max_frames=c.nf, tiles=c.tiles, bit_depth=c.bd, tools=c.tools, wavefront=c.wpp, delta_qp_rd=c.n if n is None else n, **kw)


def same_records(got, want):
    return [k for k in FIELDS if not np.array_equal(got[k], want[k])]


@pytest.mark.parametrize("path", dc.CASES, **IDS)
def test_decisions_sums_and_choice_are_the_references(path):
    """hevcdl_compress_frames on a context with the key: the picture sums of every candidate, the index and QP chosen, and the records and unfiltered reconstruction of the
    reference's final pass, exactly; the launch report is that of the context without the key."""
    import hevcdl_amd
    c = dc.Case(path)
    e = encoder(c)
    try:
        recs, recon, stats = e.compress_frames(c.yuv, c.labels)
        rows, qps = e.get_qp_rd(0, c.nf)
        launch = (e.lib.hevcdl_last_rd_launch(e._h) or b"").decode()
        trial_bytes, launches = e.get_qp_rd_info()
    finally:
        e.close()
    k = 2 * c.n + 1
    assert rows["bits"][:, :k].tolist() == c.bits.tolist() and rows["dist"][:, :k].tolist() == c.dist.tolist()
    assert rows["best_idx"].tolist() == c.chosen_idx.tolist() and qps.tolist() == c.chosen_qp.tolist()
    assert same_records(recs, c.records(hevcdl_amd.REC_DTYPE)) == []
    assert np.array_equal(recon, c.prefilter())
    assert launches == k + (k - 1) and trial_bytes >= c.nf * (c.nctu * 15120 + c.fs * (1 if c.bd == 8 else 2))
    plain = encoder(c, n=0)
    try:
        p_recs, p_recon, p_stats = plain.compress_frames(c.yuv, c.labels)
        p_launch = (plain.lib.hevcdl_last_rd_launch(plain._h) or b"").decode()
    finally:
        plain.close()
    assert launch == p_launch and launch                                  # every candidate launch runs the plan of the call without the key
    for f in range(c.nf):                                                 # a picture that kept candidate 0 is the plain context's picture, statistics included
        if c.chosen_idx[f] == 0:
            assert same_records(recs[f], p_recs[f]) == [] and np.array_equal(recon[f], p_recon[f]) and stats[f].tobytes() == p_stats[f].tobytes()
    assert [int(s["est_bits"]) > 0 for s in stats] == [True] * c.nf


def stream_of(c, recs, sao, qps):
    import hevcdl_amd
    return b"".join(hevcdl_amd.write_access_unit(c.w, c.h, int(qps[poc]), poc, recs[poc], sao=sao[poc], tiles=c.tiles, bit_depth=c.bd, tools=c.tools, wavefront=c.wpp)
                    for poc in range(c.nf))


@pytest.mark.parametrize("path", dc.CASES, **IDS)
def test_picture_pipeline_gives_the_references_pictures_and_stream(path):
    """hevcdl_encode_pictures: the deblocked picture (SAO off), the reconstruction file, and the stream -- from the records through the host writer with every picture's own
    QP, and from the slice data the device coded with every picture's own contexts."""
    import hevcdl_amd
    c = dc.Case(path)
    e = encoder(c)
    try:
        _, deblocked, _, _ = e.encode_pictures(c.yuv, c.labels, deblock=True, sao=False)
        e.enable_device_entropy(True)
        recs, final, sao, _ = e.encode_pictures(c.yuv, c.labels, deblock=True, sao=True)
        rows, qps = e.get_qp_rd(0, c.nf)
        data, sizes = e.get_slice_data(0, c.nf)
        fallbacks = e.entropy_info()[0]
    finally:
        e.close()
    assert qps.tolist() == c.chosen_qp.tolist() and rows["best_idx"].tolist() == c.chosen_idx.tolist()
    assert same_records(recs, c.records(hevcdl_amd.REC_DTYPE)) == []
    assert np.array_equal(deblocked, c.deblocked)
    assert np.array_equal(final, c.final)
    want = dc.strip_sei(c.stream)
    assert stream_of(c, recs, sao, qps) == want
    assert fallbacks == 0
    got = b""
    for poc in range(c.nf):
        scfg = hevcdl_amd.stream_config(c.w, c.h, int(qps[poc]), sao=True, tiles=c.tiles, bit_depth=c.bd, tools=c.tools, wavefront=c.wpp)
        got += hevcdl_amd.write_access_unit_from_slice_data(scfg, poc, data[poc], sizes[poc])
    assert got == want


def test_host_fallback_codes_a_picture_with_its_own_qp():
    """A capacity so small that sub-streams overflow their regions: the host codes those pictures, each from the contexts of its own QP."""
    import hevcdl_amd
    c = dc.Case(dc.path_of("c128_q32_n1"))
    e = encoder(c)
    try:
        e.set_entropy_capacity(8)
        e.enable_device_entropy(True)
        e.encode_pictures(c.yuv, c.labels, deblock=True, sao=True)
        _, qps = e.get_qp_rd(0, c.nf)
        data, sizes = e.get_slice_data(0, c.nf)
        fallbacks = e.entropy_info()[0]
    finally:
        e.close()
    assert fallbacks >= 1 and len(set(qps.tolist())) > 1
    got = b""
    for poc in range(c.nf):
        scfg = hevcdl_amd.stream_config(c.w, c.h, int(qps[poc]), sao=True, bit_depth=c.bd, tools=c.tools)
        got += hevcdl_amd.write_access_unit_from_slice_data(scfg, poc, data[poc], sizes[poc])
    assert got == dc.strip_sei(c.stream)


def test_stage_entry_points_take_the_choice():
    """hevcdl_deblock_frames_qp / hevcdl_sao_frames_qp on the reference's unfiltered reconstruction with the reference's choice: its deblocked and final pictures.  Without
    the indices the same entry points filter with the cfg's QP, which is another picture where the choice is not candidate 0."""
    import hevcdl_amd
    c = dc.Case(dc.path_of("c128_q32_n1"))
    recs, pre = c.records(hevcdl_amd.REC_DTYPE), c.prefilter()
    e = encoder(c)
    try:
        dbk = e.deblock_frames_qp(pre, recs, c.chosen_idx)
        _, fin = e.sao_frames_qp(c.yuv, dbk, c.chosen_idx)
        dbk0 = e.deblock_frames(pre, recs)
        _, fin0 = e.sao_frames(c.yuv, c.deblocked)
        with pytest.raises(hevcdl_amd.HevcdlError, match="outside the context's table"):
            e.deblock_frames_qp(pre, recs, np.array([0, 3, 0], np.int32))
    finally:
        e.close()
    assert np.array_equal(dbk, c.deblocked) and np.array_equal(fin, c.final)
    moved = [f for f in range(c.nf) if c.chosen_idx[f] != 0]
    assert moved and all(not np.array_equal(dbk0[f], c.deblocked[f]) or not np.array_equal(fin0[f], c.final[f]) for f in moved)
    assert all(np.array_equal(dbk0[f], c.deblocked[f]) and np.array_equal(fin0[f], c.final[f]) for f in range(c.nf) if f not in moved)


# ---- the kernels alone -------------------------------------------------------------------------------------------------------------------------------------------------
GUARD = 64
CANARY = 0xC7


def guarded(payload_bytes, fill):
    a = np.full(payload_bytes + 2 * GUARD, CANARY, np.uint8)
    a[GUARD:GUARD + payload_bytes] = fill
    return a


@pytest.mark.parametrize("ctus,frame_bytes", [(1, 64 * 64 * 3 // 2), (2, 128 * 64 * 3 // 2), (300, 16)], ids=["one-ctu", "two-ctus", "300-ctus"])
def test_sum_and_keep_kernels_alone(ctus, frame_bytes):
    """Three pictures a launch.  Candidate 0: the sums and the row's start.  Candidate 1 beats it on the middle picture only: that picture's records, reconstruction and
    statistics are the trial set's, its neighbours' and every canary round the three destinations are untouched.  Candidate 2 ties with the best on every picture: nothing
    moves.  Two CTUs carry dist 0xFFFFFFFF and one bits 0xFFFFFFFF: 64-bit sums.  300 CTUs: more than one round of the workgroup's lanes."""
    import hevcdl_amd
    rng = np.random.default_rng(ctus * 7 + frame_bytes)
    n, lam = 3, 4.0
    rec_b, stat_b = ctus * 15120, 40

    def trial(seed, bits, dist):
        r = np.frombuffer(np.random.default_rng(seed).integers(0, 256, n * rec_b, dtype=np.uint8).tobytes(), hevcdl_amd.REC_DTYPE).reshape(n, ctus).copy()
        r["bits"], r["dist"] = bits, dist
        return r
    big = 0xFFFFFFFF
    bits0 = rng.integers(1000, 2000, (n, ctus)).astype(np.uint32)
    dist0 = rng.integers(100000, 200000, (n, ctus)).astype(np.uint32)
    dist0[0, 0] = big
    if ctus > 1:
        dist0[0, ctus - 1] = big
        bits0[2, 1] = big
    rows = np.zeros(n, hevcdl_amd.QP_RD_ROW_DTYPE)
    rows["best_idx"], rows["take"], rows["best_cost"] = 99, 1, -1.0                  # whatever the buffer held: candidate 0 starts the row
    own_recs = trial(1, bits0, dist0)
    hevcdl_amd.qp_rd_step(ctus, frame_bytes, 0, lam, own_recs, None, None, rows, None, None, None, GUARD)
    want_bits0, want_dist0 = bits0.astype(np.uint64).sum(axis=1), dist0.astype(np.uint64).sum(axis=1)
    assert rows["bits"][:, 0].tolist() == want_bits0.tolist() and rows["dist"][:, 0].tolist() == want_dist0.tolist()
    assert want_dist0[0] > 1 << 32 or ctus == 1
    assert rows["best_idx"].tolist() == [0, 0, 0] and rows["take"].tolist() == [0, 0, 0]
    assert rows["best_cost"].tolist() == [float(int(d)) + float(int(b)) * lam for b, d in zip(want_bits0, want_dist0)]
    # candidate 1: one bit fewer on picture 1 (cheaper by lam), one more on pictures 0 and 2
    bits1 = bits0.copy()
    bits1[1, 0] -= 1
    bits1[0, 0] += 1
    bits1[2, 0] += 1
    t_recs = trial(2, bits1, dist0)
    t_pic = rng.integers(0, 256, n * frame_bytes, dtype=np.uint8)
    t_stat = rng.integers(0, 256, n * stat_b, dtype=np.uint8)
    d_rec, d_pic, d_stat = guarded(n * rec_b, np.frombuffer(own_recs.tobytes(), np.uint8)), guarded(n * frame_bytes, 0x11), guarded(n * stat_b, 0x22)
    before = [a.copy() for a in (d_rec, d_pic, d_stat)]
    hevcdl_amd.qp_rd_step(ctus, frame_bytes, 1, lam, t_recs, t_pic, t_stat, rows, d_rec, d_pic, d_stat, GUARD)
    assert rows["best_idx"].tolist() == [0, 1, 0] and rows["take"].tolist() == [0, 1, 0]
    assert rows["bits"][:, 1].tolist() == bits1.astype(np.uint64).sum(axis=1).tolist() and rows["bits"][:, 0].tolist() == want_bits0.tolist()
    for got, was, src, per in ((d_rec, before[0], np.frombuffer(t_recs.tobytes(), np.uint8), rec_b), (d_pic, before[1], t_pic, frame_bytes), (d_stat, before[2], t_stat, stat_b)):
        want = was.copy()
        want[GUARD + per:GUARD + 2 * per] = src[per:2 * per]
        assert np.array_equal(got, want)
        assert (got[:GUARD] == CANARY).all() and (got[-GUARD:] == CANARY).all()
    # candidate 2: the sums of the best of every picture again -- a tie keeps the earlier index, nothing is copied
    bits2 = np.where(np.arange(n)[:, None] == 1, bits1, bits0)
    t2 = trial(3, bits2, dist0)
    after1 = [a.copy() for a in (d_rec, d_pic, d_stat)]
    hevcdl_amd.qp_rd_step(ctus, frame_bytes, 2, lam, t2, t_pic[::-1].copy(), t_stat[::-1].copy(), rows, d_rec, d_pic, d_stat, GUARD)
    assert rows["best_idx"].tolist() == [0, 1, 0] and rows["take"].tolist() == [0, 0, 0]
    assert all(np.array_equal(a, b) for a, b in zip((d_rec, d_pic, d_stat), after1))
    for f in range(n):
        assert hevcdl_amd.qp_rd_pick(rows["bits"][f, :3], rows["dist"][f, :3], lam) == rows["best_idx"][f] == dc.pick(rows["bits"][f, :3], rows["dist"][f, :3], lam)


def test_key_zero_launches_nothing_new_and_allocates_no_trial_set():
    import hevcdl_amd
    c = dc.Case(dc.path_of("c128_q32_n1"))
    e = encoder(c, n=0)
    try:
        e._check(e.lib.hevcdl_reserve_workspace(e._h))
        e.compress_frames(c.yuv, c.labels)
        e.encode_pictures(c.yuv, c.labels)
        assert e.get_qp_rd_info() == (0, 0)
        with pytest.raises(hevcdl_amd.HevcdlError, match="delta_qp_rd"):
            e.get_qp_rd(0, 1)
    finally:
        e.close()
    e = encoder(c)
    try:
        assert e.get_qp_rd_info() == (0, 0)                                # allocated lazily ...
        e._check(e.lib.hevcdl_reserve_workspace(e._h))
        assert e.get_qp_rd_info()[0] > 0 and e.get_qp_rd_info()[1] == 0    # ... or by the reservation
    finally:
        e.close()


def test_session_and_tile_ranges_refuse_the_key():
    import hevcdl_amd
    c = dc.Case(dc.path_of("t512x128_q32_n1"))
    e = encoder(c)
    try:
        st = e.lib.hevcdl_begin_frames(e._h, np.ascontiguousarray(c.yuv).ctypes.data, 1, None, None)
        why = (e.lib.hevcdl_last_error(e._h) or b"").decode()
        assert st == 2 and "per-CTU session" in why and "DeltaQpRD" in why
        st = e.lib.hevcdl_compress_tiles_dev(e._h, None, 1, None, None, None, None, 0, 1, None)
        why = (e.lib.hevcdl_last_error(e._h) or b"").decode()
        assert st == 2 and "DeltaQpRD" in why
    finally:
        e.close()


def log_of(lines):
    """Picture lines without [ET ...] and the reference build's "nQP <n> ", with their hash text, and the two lines of the summary block."""
    poc = [re.sub(r"nQP -?\d+ ", "", qr.strip_et(l)) + " " + l[l.index("[MD5:"):].strip() for l in lines if l.startswith("POC")]
    i = next(k for k, l in enumerate(lines) if l.startswith("SUMMARY"))
    return poc, [l.rstrip() for l in lines[i + 1:i + 3]]


def cli_inputs(c, tmp_path):
    c.yuv.astype(c.dt).tofile(tmp_path / "in.yuv")
    for f in range(c.nf):
        os.makedirs(tmp_path / "pred" / str(f))
        for a in range(c.nctu):
            (tmp_path / "pred" / str(f) / ("ctu%d.txt" % a)).write_text(" ".join(str(int(v)) for v in c.labels[f, a]) + " ")


@pytest.mark.parametrize("name", ["c128_q32_n1", "c128_q30_n1_b10", "w192x128_q32_n1"])
def test_cli_reproduces_the_reference_run(name, tmp_path):
    """The reference's own keys on the reference's own input: stream, reconstruction file and log lines (every picture line with the QP the picture was coded with); with
    --DeviceEntropy=1 --DeviceReport=1 the same once more; and for the first case on two contexts that share device 0, rows gathered."""
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    c = dc.Case(dc.path_of(name))
    cli_inputs(c, tmp_path)
    base = [app, "-i", "in.yuv", "-wdt", str(c.w), "-hgt", str(c.h), "-q", str(c.qp), "-f", str(c.nf), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=1",
            "--InputBitDepth=%d" % c.bd, "--Profile=%s" % ("main" if c.bd == 8 else "main10")] + [str(k) for k in c.f["keys"]]
    want = log_of([str(l) for l in c.f["stdout"]])
    assert ["QP %d )" % q in l for q, l in zip(c.chosen_qp, want[0])] == [True] * c.nf
    runs = [("plain", []), ("device", ["--DeviceEntropy=1", "--DeviceReport=1"])] + ([("shared", ["--Devices=0,0"])] if name == "c128_q32_n1" else [])
    for tag, extra in runs:
        r = subprocess.run(base + ["-b", tag + ".bin", "-o", tag + ".yuv"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert (tmp_path / (tag + ".bin")).read_bytes() == c.stream, tag
        assert (tmp_path / (tag + ".yuv")).read_bytes() == c.f["recon_file"].tobytes(), tag
        assert log_of(r.stdout.splitlines()) == want, tag
        assert tag != "shared" or "Picture rows gathered" in r.stderr


def test_python_pipeline_agrees_with_the_reference_and_so_with_the_cli(tmp_path):
    """pipeline.encode_sequence(delta_qp_rd=N): the stream and reconstruction file test_cli_reproduces_the_reference_run holds the command line to, the rows with the QP
    every picture was coded with; with device entropy and the device report the same."""
    import hevcdl_amd
    from hevcdl_amd import pipeline
    c = dc.Case(dc.path_of("c128_q32_n1"))
    c.yuv.astype(c.dt).tofile(tmp_path / "in.yuv")
    for tag, kw in (("host", {}), ("device", dict(device_entropy=True, device_report=True))):
        lines = []
        summ, rows = pipeline.encode_sequence(str(tmp_path / "in.yuv"), c.w, c.h, c.qp, c.nf, bitstream_path=str(tmp_path / (tag + ".bin")), recon_path=str(tmp_path / (tag + ".yuv")),
                                              hash_sei=True, labels_fn=lambda first, count: c.labels[first:first + count], delta_qp_rd=c.n, log=lines.append, **kw)
        assert (tmp_path / (tag + ".bin")).read_bytes() == c.stream, tag
        assert (tmp_path / (tag + ".yuv")).read_bytes() == c.f["recon_file"].tobytes(), tag
        assert rows.shape == (c.nf, 6) and rows[:, 5].tolist() == c.chosen_qp.tolist()
        assert ["QP %d" % q in l for q, l in zip(c.chosen_qp, [l for l in lines if l.startswith("POC")])] == [True] * c.nf
    with pytest.raises(ValueError, match="tile-sharded path does not search the slice QP"):
        pipeline.encode_sequence_tile_sharded(str(tmp_path / "in.yuv"), c.w, c.h, c.qp, c.nf, (1, 1), delta_qp_rd=1)


def test_two_ranks_give_the_single_process_files_and_log(tmp_path):
    """pipeline.encode_sequence(delta_qp_rd=1) under torch.distributed (tools/encode_sharded.py, two ranks on one GPU, gloo): pictures are independent, so stream,
    reconstruction file and log lines -- every picture's own QP among them, gathered with the rows -- are those of one process, and of the command line on two contexts."""
    import socket
    import sys
    import hevcdl_amd
    c = dc.Case(dc.path_of("c128_q32_n1"))
    c.yuv.astype(c.dt).tofile(tmp_path / "in.yuv")
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "encode_sharded.py")
    common = ["-i", "in.yuv", "-wdt", str(c.w), "-hgt", str(c.h), "-q", str(c.qp), "-f", str(c.nf), "--batch", "2", "--hash", "--delta-qp-rd", "1"]
    r1 = subprocess.run([sys.executable, script] + common + ["-b", "one.bin", "-o", "one.yuv"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                         script] + common + ["-b", "two.bin", "-o", "two.yuv", "--backend", "gloo"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert (tmp_path / "one.bin").read_bytes() == (tmp_path / "two.bin").read_bytes() and (tmp_path / "one.yuv").read_bytes() == (tmp_path / "two.yuv").read_bytes()
    lines = lambda t: [l for l in t.splitlines() if l.startswith("POC") or l.startswith("\t ")]
    assert lines(r1.stdout) == lines(r2.stdout) and len(lines(r1.stdout)) == c.nf + 1
    qps = [int(re.search(r"QP (\d+) \)", l).group(1)) for l in lines(r1.stdout)[:c.nf]]
    assert all(abs(q - c.qp) <= 1 for q in qps) and len(set(qps)) > 1, qps      # the flat picture and the noise picture do not want the same QP
    r3 = subprocess.run([hevcdl_amd.build_app(), "-i", "in.yuv", "-wdt", str(c.w), "-hgt", str(c.h), "-q", str(c.qp), "-f", str(c.nf), "-b", "cli.bin", "-o", "cli.yuv", "-dqr", "1",
                         "--SEIDecodedPictureHash=1", "--Level=6.2", "--Devices=0,0"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, r3.stdout[-1500:] + r3.stderr[-1500:]
    assert (tmp_path / "cli.bin").read_bytes() == (tmp_path / "one.bin").read_bytes() and (tmp_path / "cli.yuv").read_bytes() == (tmp_path / "one.yuv").read_bytes()
    assert [int(re.search(r"QP (\d+) \)", l).group(1)) for l in r3.stdout.splitlines() if l.startswith("POC")] == qps
