"""A QP per picture on the device: the permute kernel (csrc/frame_permute_kernel.hip) alone on synthetic pictures, the grouped decisions and the picture pipelines against
runs of the reference encoder with dQPFile, QPIncrementFrame, IntraQPOffset and the lambda modifiers (tests/golden/fqp_*.npz, tools/gen_frame_qp_fixtures.py), the command
line and the Python pipeline, the permuted path against the no-copy path, and a QP sweep in one context against one context a QP.  Every picture is a few CTUs."""
import os
import re
import subprocess

import numpy as np
import pytest

import frame_qp_cases as fc
import quality_ref as qr

pytestmark = pytest.mark.gpu
IDS = dict(ids=fc.case_id)
FIELDS = ["depth", "part_size", "luma_dir", "chroma_dir", "tr_idx", "cbf", "tskip", "bits", "dist", "cost", "coeff_y", "coeff_cb", "coeff_cr"]


def same_records(got, want):
    return [k for k in FIELDS if not np.array_equal(got[k], want[k])]


def with_keys(c, e):
    """The fixture's keys on a context: the list (only where a key makes one) and the modifier."""
    if c.modifier != 1.0:
        e.set_lambda_modifier(c.modifier)
    if c.qps != [c.qp] * c.nf:
        e.set_frame_qps(c.qps)


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------------------------------------------------
GUARD = 64
CANARY = 0xC7


def guarded(payload_bytes, fill):
    a = np.full(payload_bytes + 2 * GUARD, CANARY, np.uint8)
    a[GUARD:GUARD + payload_bytes] = fill
    return a


def perms_of(n, seed):
    out = [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(seed).permutation(n)]
    return [p.astype(np.int32) for p in out]


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("w,h,bd", [(8, 8, 8), (8, 8, 10), (200, 136, 8), (200, 136, 10)], ids=["8x8", "8x8-b10", "200x136", "200x136-b10"])
def test_permute_kernel_alone(w, h, bd, n):
    """The four ranges of the pipeline in one launch -- source planes, labels (16 bytes a CTU), records (15120 bytes a CTU: more than one chunk at 12 CTUs) and the 40 bytes
    of statistics a picture, whose pictures are 8-byte aligned only -- for the identity, the reversal and a random permutation: the gather equals numpy's, every canary
    round the four destinations is intact, and the scatter of the gathered set restores the input."""
    import hevcdl_amd
    ctus = ((w + 63) // 64) * ((h + 63) // 64)
    sizes = [w * h * 3 // 2 * (1 if bd == 8 else 2), 16 * ctus, 15120 * ctus, 40]
    rng = np.random.default_rng(w + bd + n)
    srcs = [rng.integers(0, 256, n * b, dtype=np.uint8) for b in sizes]
    for perm in perms_of(n, 3 * n + w):
        dsts = [guarded(n * b, 0x5A) for b in sizes]
        hevcdl_amd.frame_permute_step(list(zip(srcs, dsts)), perm, False, GUARD)
        for s, d, b in zip(srcs, dsts, sizes):
            assert (d[:GUARD] == CANARY).all() and (d[-GUARD:] == CANARY).all()
            assert np.array_equal(d[GUARD:-GUARD].reshape(n, b), s.reshape(n, b)[perm])
        back = [guarded(n * b, 0xA5) for b in sizes]
        hevcdl_amd.frame_permute_step([(d[GUARD:-GUARD].copy(), k) for d, k in zip(dsts, back)], perm, True, GUARD)
        for s, k in zip(srcs, back):
            assert (k[:GUARD] == CANARY).all() and (k[-GUARD:] == CANARY).all()
            assert np.array_equal(k[GUARD:-GUARD], s)


def test_permute_kernel_narrow_ranges_and_refusals():
    """Picture sizes that are no multiple of 16: 8-, 4- and 1-byte accesses by one workgroup a picture, more than one round of its lanes (2056 bytes = 257 words of 8);
    one range alone; a guard that is no multiple of 16 (the destination's base is then 1-byte aligned and a 16-byte range goes by bytes).  A list that is no permutation is
    refused before anything runs."""
    import hevcdl_amd
    n = 5
    perm = np.array([3, 0, 4, 1, 2], np.int32)
    rng = np.random.default_rng(77)
    for sizes, guard in (([2056, 36, 37, 16], 64), ([40], 64), ([48, 96], 8), ([32], 3)):
        srcs = [rng.integers(0, 256, n * b, dtype=np.uint8) for b in sizes]
        dsts = [np.full(n * b + 2 * guard, CANARY, np.uint8) for b in sizes]
        hevcdl_amd.frame_permute_step(list(zip(srcs, dsts)), perm, False, guard)
        for s, d, b in zip(srcs, dsts, sizes):
            assert (d[:guard] == CANARY).all() and (d[-guard:] == CANARY).all()
            assert np.array_equal(d[guard:guard + n * b].reshape(n, b), s.reshape(n, b)[perm])
    src, dst = np.zeros(3 * 16, np.uint8), np.zeros(3 * 16 + 2 * GUARD, np.uint8)
    for bad in ([0, 1, 1], [0, 1, 3], [-1, 0, 1]):
        with pytest.raises(hevcdl_amd.HevcdlError):
            hevcdl_amd.frame_permute_step([(src, dst)], np.array(bad, np.int32), False, GUARD)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", fc.CASES, **IDS)
def test_decisions_with_the_list_are_the_references(path):
    """hevcdl_compress_frames with the fixture's list and modifier: the reference's records and unfiltered reconstruction, exactly; one decision launch per distinct QP; the
    permute kernel runs (twice: gather, scatter) exactly where a QP comes back after another."""
    import hevcdl_amd
    c = fc.Case(path)
    e = c.encoder()
    try:
        with_keys(c, e)
        recs, recon, stats = e.compress_frames(c.yuv, c.labels)
        qps = e.get_frame_qps(0, c.nf).tolist()
        set_bytes, rd_launches, permute_launches = e.get_frame_qp_info()
    finally:
        e.close()
    assert qps == c.qps
    assert same_records(recs, c.records(hevcdl_amd.REC_DTYPE)) == []
    assert np.array_equal(recon, c.prefilter)
    assert rd_launches == len(set(c.qps))
    assert permute_launches == (0 if fc.contiguous(c.qps) else 2) and (set_bytes > 0) == (permute_launches > 0)
    assert [int(s["est_bits"]) > 0 for s in stats] == [True] * c.nf


def stream_of(c, recs, sao):
    import hevcdl_amd
    return b"".join(hevcdl_amd.write_access_unit(c.w, c.h, c.qps[poc], poc, recs[poc], sao=sao[poc], **c.writer_kw()) for poc in range(c.nf))


@pytest.mark.parametrize("path", fc.CASES, **IDS)
def test_picture_pipeline_gives_the_references_pictures_and_stream(path):
    """hevcdl_encode_pictures: the deblocked picture (SAO off), the reconstruction file, and the stream -- from the records through the host writer with every picture's own
    QP, and from the slice data the device coded with every picture's own contexts."""
    import hevcdl_amd
    c = fc.Case(path)
    e = c.encoder()
    try:
        with_keys(c, e)
        _, deblocked, _, _ = e.encode_pictures(c.yuv, c.labels, deblock=True, sao=False)
        e.enable_device_entropy(True)
        recs, final, sao, _ = e.encode_pictures(c.yuv, c.labels, deblock=True, sao=True)
        data, sizes = e.get_slice_data(0, c.nf)
        fallbacks = e.entropy_info()[0]
        layout = e.slice_layout
    finally:
        e.close()
    assert same_records(recs, c.records(hevcdl_amd.REC_DTYPE)) == []
    assert np.array_equal(deblocked, c.deblocked)
    assert np.array_equal(final, c.final)
    want = fc.strip_sei(c.stream)
    assert stream_of(c, recs, sao) == want
    assert fallbacks == 0
    got = b""
    for poc in range(c.nf):
        scfg = hevcdl_amd.stream_config(c.w, c.h, c.qps[poc], sao=True, tiles=c.tiles, bit_depth=c.bd, wavefront=c.wpp)
        got += hevcdl_amd.write_access_unit_from_slice_data(scfg, poc, data[poc], sizes[poc], layout=layout)
    assert got == want


def test_host_fallback_codes_a_picture_with_its_own_qp():
    """A capacity so small that sub-streams overflow their regions: the host codes those pictures, each from the contexts of its own QP."""
    import hevcdl_amd
    c = fc.Case(fc.path_of("d192_q32"))
    e = c.encoder()
    try:
        with_keys(c, e)
        e.set_entropy_capacity(8)
        e.enable_device_entropy(True)
        e.encode_pictures(c.yuv, c.labels, deblock=True, sao=True)
        data, sizes = e.get_slice_data(0, c.nf)
        fallbacks = e.entropy_info()[0]
    finally:
        e.close()
    assert fallbacks >= 1
    got = b""
    for poc in range(c.nf):
        got += hevcdl_amd.write_access_unit_from_slice_data(hevcdl_amd.stream_config(c.w, c.h, c.qps[poc], sao=True, bit_depth=c.bd), poc, data[poc], sizes[poc])
    assert got == fc.strip_sei(c.stream)


def log_of(lines):
    """Picture lines without [ET ...] and the reference build's "nQP <n> ", with their hash text, and the two lines of the summary block."""
    poc = [re.sub(r"nQP -?\d+ ", "", qr.strip_et(l)) + " " + l[l.index("[MD5:"):].strip() for l in lines if l.startswith("POC")]
    i = next(k for k, l in enumerate(lines) if l.startswith("SUMMARY"))
    return poc, [l.rstrip() for l in lines[i + 1:i + 3]]


def cli_inputs(c, tmp_path):
    c.file_yuv.astype(c.dt).tofile(tmp_path / "in.yuv")
    if c.dqp_text:
        (tmp_path / "dqp.txt").write_text(c.dqp_text + "\n")
    for f in range(c.nf):
        os.makedirs(tmp_path / "pred" / str(f))
        for a in range(c.nctu):
            (tmp_path / "pred" / str(f) / ("ctu%d.txt" % a)).write_text(" ".join(str(int(v)) for v in c.labels[f, a]) + " ")


@pytest.mark.parametrize("path", fc.CASES, **IDS)
def test_cli_reproduces_the_reference_run(path, tmp_path):
    """The reference's own keys on the reference's own input (FrameSkip frames in front included, the dQP file as it was): stream, reconstruction file and log lines (every
    picture line with the picture's QP); with --DeviceEntropy=1 --DeviceReport=1 the same once more; and for the permuted fixture on two contexts that share device 0, each
    with its slice of the list."""
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    c = fc.Case(path)
    cli_inputs(c, tmp_path)
    base = [app, "-i", "in.yuv", "-wdt", str(c.w), "-hgt", str(c.h), "-q", str(c.qp), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=1",
            "--InputBitDepth=%d" % c.bd, "--Profile=%s" % ("main" if c.bd == 8 else "main10")] + c.keys
    want = log_of([str(l) for l in c.f["stdout"]])
    assert ["QP %d )" % q in l for q, l in zip(c.qps, want[0])] == [True] * c.nf
    runs = [("plain", []), ("device", ["--DeviceEntropy=1", "--DeviceReport=1"])] + ([("shared", ["--Devices=0,0"])] if c.name == "d192_q32" else [])
    for tag, extra in runs:
        r = subprocess.run(base + ["-b", tag + ".bin", "-o", tag + ".yuv"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert (tmp_path / (tag + ".bin")).read_bytes() == c.stream, tag
        assert (tmp_path / (tag + ".yuv")).read_bytes() == c.f["recon_file"].tobytes(), tag
        assert log_of(r.stdout.splitlines()) == want, tag
    if c.qpif is not None:
        assert "QP                                     : %d (incrementing internal QP at source frame %d)" % (c.qp, c.qpif) in r.stdout


def test_python_pipeline_agrees_with_the_reference_and_so_with_the_cli(tmp_path):
    """pipeline.encode_sequence(frame_qps=..., lambda_modifier=...): the stream and reconstruction file test_cli_reproduces_the_reference_run holds the command line to, the
    rows with every picture's QP; with device entropy and the device report the same; in batches of four the batches' slices of the list."""
    import hevcdl_amd
    from hevcdl_amd import pipeline
    for name, batch in (("d192_q32", 256), ("d192_q32", 4), ("o192_q32_lmi", 256)):
        c = fc.Case(fc.path_of(name))
        c.yuv.astype(c.dt).tofile(tmp_path / "in.yuv")
        qps = hevcdl_amd.frame_qp_list(c.qp, c.dqp, c.intra_qp_offset, c.bd).tolist()
        for tag, kw in (("host", {}), ("device", dict(device_entropy=True, device_report=True))):
            lines = []
            summ, rows = pipeline.encode_sequence(str(tmp_path / "in.yuv"), c.w, c.h, c.qp, c.nf, bitstream_path=str(tmp_path / (tag + ".bin")), recon_path=str(tmp_path / (tag + ".yuv")),
                                                  hash_sei=True, labels_fn=lambda first, count: c.labels[first:first + count], frame_qps=qps, lambda_modifier=c.modifier, batch=batch,
                                                  log=lines.append, **kw)
            assert (tmp_path / (tag + ".bin")).read_bytes() == c.stream, (name, tag)
            assert (tmp_path / (tag + ".yuv")).read_bytes() == c.f["recon_file"].tobytes(), (name, tag)
            assert rows.shape == (c.nf, 6) and rows[:, 5].tolist() == c.qps
            assert ["QP %d" % q in l for q, l in zip(c.qps, [l for l in lines if l.startswith("POC")])] == [True] * c.nf


# ---- the two paths, the sweep, the plain call --------------------------------------------------------------------------------------------------------------------------------
def test_permuted_path_equals_the_no_copy_path():
    """Fixture 1's pictures with the list as recorded (a QP comes back: gathered, decided, scattered) and the same pictures sorted by the caller (contiguous runs: offsets
    into the caller's buffers): after un-sorting, records, reconstruction and statistics are the same bytes; both make one decision launch per distinct QP, of the same
    launch form, and only the first touches the sorted sets."""
    import hevcdl_amd
    c = fc.Case(fc.path_of("d192_q32"))
    perm, runs, cont = hevcdl_amd.frame_qp_grouping(c.qps)
    assert not cont
    e = c.encoder()
    try:
        e.profile_enable(True)
        e.set_frame_qps(c.qps)
        recs, recon, stats = e.compress_frames(c.yuv, c.labels)
        info, launch, prof = e.get_frame_qp_info(), e.last_rd_launch(), e.profile_get()
        e.set_frame_qps([c.qps[p] for p in perm])
        s_recs, s_recon, s_stats = e.compress_frames(c.yuv[perm], c.labels[perm])
        s_info, s_launch, s_prof = e.get_frame_qp_info(), e.last_rd_launch(), e.profile_get()
    finally:
        e.close()
    assert recs[perm].tobytes() == s_recs.tobytes() and np.array_equal(recon[perm], s_recon) and stats[perm].tobytes() == s_stats.tobytes()
    assert same_records(recs, c.records(hevcdl_amd.REC_DTYPE)) == []
    assert info[1:] == (3, 2) and s_info[1:] == (3, 0) and info[0] == s_info[0] > 0
    assert prof["rd_launches"] == 3 and s_prof["rd_launches"] == 3            # one launch per distinct QP in both
    assert launch and s_launch and "units=" in launch


def test_a_sweep_in_one_context_equals_a_context_per_qp():
    """Four pictures, each given four times with QPs 22 / 27 / 32 / 37, in one context with the labels computed once -- against four contexts at those QPs."""
    import hevcdl_amd
    import ref_tools
    w, h, qps = 128, 72, [22, 27, 32, 37]
    yuv = ref_tools.synth_yuv(w, h, 4, seed=41)
    want = {}
    for q in qps:
        e = hevcdl_amd.Encoder(w, h, q, max_frames=4)
        try:
            labels = e.predict_depth(yuv)
            want[q] = e.compress_frames(yuv, labels)
        finally:
            e.close()
    e = hevcdl_amd.Encoder(w, h, 30, max_frames=16)
    try:
        labels = e.predict_depth(yuv)                                           # once: the labels do not depend on the QP
        e.set_frame_qps(qps * 4)                                                # picture-major: every QP comes back four times
        recs, recon, stats = e.compress_frames(np.repeat(yuv, 4, axis=0), np.repeat(labels, 4, axis=0))
        info = e.get_frame_qp_info()
    finally:
        e.close()
    assert info[1:] == (4, 2)
    for k, q in enumerate(qps):
        w_recs, w_recon, w_stats = want[q]
        assert recs[k::4].tobytes() == w_recs.tobytes() and np.array_equal(recon[k::4], w_recon) and stats[k::4].tobytes() == w_stats.tobytes(), q
    assert len({want[q][0].tobytes() for q in qps}) == 4


def test_equal_and_cleared_lists_are_the_plain_call():
    """A list of equal QPs is one launch of all the pictures, with the launch form of the plain call and nothing copied; at the context's QP it gives the plain call's
    bytes, at another QP those of a context created with it.  A list past its end and a cleared list fall back to the context's QP."""
    import hevcdl_amd
    c = fc.Case(fc.path_of("d192_q32"))
    outs = {}
    for q in (32, 34):
        e = c.encoder() if q == 32 else hevcdl_amd.Encoder(c.w, c.h, q, max_frames=c.nf)
        try:
            outs[q] = e.compress_frames(c.yuv, c.labels) + (e.last_rd_launch(), e.get_frame_qp_info())
        finally:
            e.close()
    e = c.encoder()
    try:
        def run():
            r = e.compress_frames(c.yuv, c.labels)
            return r + (e.last_rd_launch(), e.get_frame_qp_info())
        e.set_frame_qps([32] * c.nf)
        same = run()
        e.set_frame_qps([34] * c.nf)
        other = run()
        e.set_frame_qps([34] * 2)                                               # pictures past the list take the context's QP
        mixed = run()
        e.set_frame_qps(None)
        cleared = run()
        e.set_lambda_modifier(1.0)
        unit = run()
        with pytest.raises(hevcdl_amd.HevcdlError, match="outside 0 .. 51"):
            e.set_frame_qps([32, 52])
        kept = run()                                                            # a refused list leaves the one before: none
    finally:
        e.close()
    for got, want in ((same, outs[32]), (other, outs[34]), (cleared, outs[32]), (unit, outs[32]), (kept, outs[32])):
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
        assert got[3] == want[3] and got[4] == (0, 1, 0)                        # the launch report of the plain call; one launch, nothing allocated or copied
    assert mixed[0][:2].tobytes() == outs[34][0][:2].tobytes() and mixed[0][2:].tobytes() == outs[32][0][2:].tobytes() and mixed[4] == (0, 2, 0)


def test_session_and_tile_ranges_refuse_the_list():
    import hevcdl_amd
    c = fc.Case(fc.path_of("t512_q32"))
    for setter in (lambda e: e.set_frame_qps(c.qps), lambda e: e.set_lambda_modifier(0.8)):
        e = c.encoder()
        try:
            setter(e)
            st = e.lib.hevcdl_begin_frames(e._h, np.ascontiguousarray(c.yuv).ctypes.data, 1, None, None)
            why = (e.lib.hevcdl_last_error(e._h) or b"").decode()
            assert st == 2 and "per-CTU session" in why and "QP per picture" in why
            st = e.lib.hevcdl_compress_tiles_dev(e._h, None, 1, None, None, None, None, 0, 1, None)
            why = (e.lib.hevcdl_last_error(e._h) or b"").decode()
            assert st == 2 and "compress_tiles" in why and "QP per picture" in why
            e.set_frame_qps(None)
            e.set_lambda_modifier(1.0)
            assert e.lib.hevcdl_compress_tiles_dev(e._h, None, 0, None, None, None, None, 0, 1, None) == 0      # cleared: the call is the call it was
        finally:
            e.close()
    for kw in (dict(delta_qp_rd=1), dict(deblocking_metric=1, lf_offset_in_pps=False)):
        e = hevcdl_amd.Encoder(128, 128, 32, max_frames=2, **kw)
        try:
            for setter in (lambda: e.set_frame_qps([32, 33]), lambda: e.set_lambda_modifier(1.5)):
                with pytest.raises(hevcdl_amd.HevcdlError, match="DeltaQpRD" if "delta_qp_rd" in kw else "DeblockingFilterMetric"):
                    setter()
            e.set_frame_qps(None)
            e.set_lambda_modifier(1.0)
        finally:
            e.close()


def test_reserve_workspace_allocates_the_sorted_sets_only_with_a_list():
    import hevcdl_amd
    c = fc.Case(fc.path_of("d192_q32"))
    e = c.encoder()
    try:
        e.reserve_workspace()
        assert e.get_frame_qp_info()[0] == 0
        e.set_frame_qps(c.qps)
        e.reserve_workspace()
        assert e.get_frame_qp_info()[0] >= c.nf * (c.nctu * 15120 + 2 * c.fs + 16 * c.nctu + 40)
    finally:
        e.close()
