"""Per-picture deblocking parameters on the device: the metric kernel (csrc/dbk_select_kernel.hip) against the Python restatement of
TEncGOP::applyDeblockingFilterMetric (tests/dbk_select_ref.py, itself tied to the reference by tests/test_dbk_select.py), the fused deblocking kernel with a row of
parameters per picture against the oracle, and the picture pipelines and the CLI against runs of the reference encoder (tests/golden/dbksel_*.npz)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dbk_select_ref as ref
import quality_ref as qr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_tools              # noqa: E402

QP = 47      # beta(47) = 56: thr1 = 2, thr2 = 14 at 8 bits; 8 and 56 at 10 bits (both even, so a line's `a` can sit exactly on either)
# 64 x 64: one edge each way; 72 x 72: the edges at 64 are computed by the reference and dropped; 96 x 64: two vertical edges, one horizontal; 264 x 72: more lines than
# one workgroup takes in one step, a width that is no multiple of 32
SIZES = [(64, 64), (72, 72), (96, 64), (264, 72)]


def dt(bd):
    return np.uint8 if bd == 8 else np.dtype("<u2")


def frame_of(luma, bd, seed):
    """A whole frame around a luma plane: the chroma planes are noise the metric must not read into its sums."""
    h, w = luma.shape
    rng = np.random.default_rng(seed)
    return np.concatenate([luma.reshape(-1), rng.integers(0, 1 << bd, w * h // 2)]).astype(dt(bd))


def lumas(w, h, bd, seed):
    """name -> luma plane: noise, ramps, lines whose `a` sits exactly on either threshold (must not count) and one step inside (must), |p0 - q0| at the rails."""
    rng = np.random.default_rng(seed)
    top, s = (1 << bd) - 1, 1 << (bd - 8)
    thr1, thr2 = ref.thresholds(QP, bd)
    y, x = np.mgrid[0:h, 0:w]
    out = {"noise": rng.integers(0, top + 1, (h, w)), "small_noise": top // 2 + rng.integers(-2 * s, 2 * s + 1, (h, w)),
           "ramps": np.clip((x * 3 + y * 2) * s + (x // 32) * 7 * s + (y // 32) * 5 * s + rng.integers(-s, s + 1, (h, w)), 0, top)}
    # second derivatives of exactly k on the p side (p2 p1 p0 = v, v, v + k), flat on the q side: a = 2 k.  Lines cycle through a = thr1, thr1 + 2, thr2 - 2, thr2 around
    # a large step |p0 - q0|; first across the vertical edges, then across the horizontal ones
    ks = [thr1 // 2, thr1 // 2 + 1, thr2 // 2 - 1, thr2 // 2]
    assert [2 * k for k in ks] == [thr1, thr1 + 2, thr2 - 2, thr2]
    for name, transposed in (("thresholds_v", False), ("thresholds_h", True)):
        hh, ww = (w, h) if transposed else (h, w)
        p = np.full((hh, ww), 100 * s, np.int64)
        for c in range(32, ww, 32):
            k = np.array(ks)[np.arange(hh) % 4]
            p[:, c - 1] += k
            p[:, c:c + 16] = 100 * s + k[:, None] + 40 * s + np.arange(hh)[:, None] % 7      # q side flat per line, a step of 40 s + (line mod 7) - nothing
        out[name] = p.T if transposed else p
    rails = np.zeros((h, w), np.int64)
    rails[(x // 32 + y // 32) % 2 == 1] = top
    rails[:, 31::32] -= np.where(rails[:, 31::32] > 0, 2 * s, -2 * s)      # a second derivative inside (thr1, thr2) next to the edge: 2 * 2 s = 4 s
    rails[31::32, :] -= np.where(rails[31::32, :] > 0, 2 * s, -2 * s)
    out["rails"] = np.clip(rails, 0, top)
    return out


def expected(frames, w, h, bd):
    return np.array([ref.metric_sums(f[:w * h].reshape(h, w), QP, bd) for f in frames], np.uint64)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_metric_sums_equal_the_restatement(size, bd):
    import hevcdl_amd
    w, h = size
    planes = lumas(w, h, bd, 7 * w + h + bd)
    frames = np.stack([frame_of(p, bd, i) for i, p in enumerate(planes.values())])
    want = expected(frames, w, h, bd)
    by_name = dict(zip(planes, want.tolist()))
    # the crafted lines: exactly the two inner values of `a` count, so half of the lines of every edge that counts; the restatement must say so before the kernel is asked
    lines_v, lines_h = ((w >> 5) - 1) * h, ((h >> 5) - 1) * w
    s = 1 << (bd - 8)
    for key, lines, size_other in (("thresholds_v", lines_v, h), ("thresholds_h", lines_h, w)):
        k = np.arange(size_other) % 4
        step = 40 * s + np.arange(size_other) % 7
        per_edge = int(step[(k == 1) | (k == 2)].sum())
        assert by_name[key][0 if key.endswith("v") else 1] == per_edge * (lines // size_other), key
    assert by_name["rails"][0] > 0 and by_name["rails"][1] > 0 and by_name["small_noise"] != [0, 0]
    enc = hevcdl_amd.Encoder(w, h, QP, max_frames=len(frames), bit_depth=bd)
    try:
        got = enc.dbk_metric_frames(frames)
        assert got.tolist() == want.tolist(), dict(zip(planes, zip(got.tolist(), want.tolist())))
        # a batch of three unlike frames in another order, and one frame alone: position in the batch and batch size do not matter
        pick = [4, 0, 2]
        assert enc.dbk_metric_frames(frames[pick]).tolist() == want[pick].tolist()
        assert enc.dbk_metric_frames(frames[5:6]).tolist() == want[5:6].tolist()
    finally:
        enc.close()


def test_metric_is_refused_under_64_samples():
    import hevcdl_amd
    enc = hevcdl_amd.Encoder(56, 64, QP, max_frames=1)
    try:
        with pytest.raises(hevcdl_amd.HevcdlError, match="at least 64 luma samples"):
            enc.dbk_metric_frames(np.zeros((1, 56 * 64 * 3 // 2), np.uint8))
    finally:
        enc.close()


@pytest.fixture(scope="module")
def decided():
    """(w, h, qp, bit depth) -> four frames decided by the oracle: records and reconstruction before deblocking."""
    __import__("__graft_entry__").build_oracle()
    out = {}
    for w, h, qp, bd in ((264, 72, 37, 8), (72, 72, 32, 10)):
        yuv = ref_tools.synth_yuv(w, h, 4, seed=w + bd)
        if bd > 8:
            yuv = (yuv.astype(np.uint16) << 2) | (np.arange(yuv.size, dtype=np.uint16).reshape(yuv.shape) & 3)
        labels = ref_tools.make_labels(w, h, 4, "rand", seed=3)
        recs, recon, _ = ref_tools.run_oracle(yuv, w, h, qp, labels, bit_depth=bd)
        out[(w, h, qp, bd)] = (recs, recon)
    return out


@pytest.mark.parametrize("key", [(264, 72, 37, 8), (72, 72, 32, 10)], ids=lambda k: "%dx%d_q%d_b%d" % k)
def test_deblocking_with_parameters_per_picture_equals_the_oracle(decided, key):
    """Three pictures with three different pairs of offsets and one disabled picture, in one launch: every picture is the oracle's with its own offsets; the same in place;
    without the array the launch is the one it was."""
    import torch
    import hevcdl_amd
    w, h, qp, bd = key
    recs, recon = decided[key]
    d = dict(width=w, height=h, qp=qp, bit_depth=bd, tiles=(1, 1), lf_across_tiles=1)
    choices = np.array([(1, 1, 0, 3, -2), (1, 1, 0, -3, 5), (1, 1, 1, 0, 0), (1, 1, 0, 6, 6)], ref.CHOICE)
    want = ref.deblock_with(d, recon, recs, choices)
    assert np.array_equal(want[2], recon[2]) and all(not np.array_equal(want[i], recon[i]) for i in (0, 1, 3))
    assert not np.array_equal(want[0], ref.deblock_with(d, recon[:1], recs[:1], choices[1:2])[0]), "the pairs must matter on this content"
    enc = hevcdl_amd.Encoder(w, h, qp, max_frames=4, bit_depth=bd, lf_offsets=(1, -1))
    try:
        assert np.array_equal(enc.deblock_frames_choice(recon, recs, choices), want)
        assert np.array_equal(enc.deblock_frames_choice(recon[1:3], recs[1:3], choices[1:3]), want[1:3])
        d_rec = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1)).cuda()
        d_pic = torch.from_numpy(np.ascontiguousarray(recon).view(np.uint8).reshape(-1)).cuda()
        enc.deblock_frames_choice_dev(d_pic.data_ptr(), 4, d_rec.data_ptr(), choices, d_pic.data_ptr())      # in == out
        torch.cuda.synchronize()
        assert d_pic.cpu().numpy().tobytes() == want.tobytes()
        # no array: the context's own offsets for every picture, as ever
        plain = ref_tools.run_deblock(recon, w, h, qp, recs, bit_depth=bd, lf_offsets=(1, -1))
        assert np.array_equal(enc.deblock_frames(recon, recs), plain)
        d_pic = torch.from_numpy(np.ascontiguousarray(recon).view(np.uint8).reshape(-1)).cuda()
        d_out = torch.zeros_like(d_pic)
        enc.deblock_frames_choice_dev(d_pic.data_ptr(), 4, d_rec.data_ptr(), None, d_out.data_ptr())
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == plain.astype(dt(bd)).tobytes()
    finally:
        enc.close()


def _encoder(d, n):
    import hevcdl_amd
    return hevcdl_amd.Encoder(d["width"], d["height"], d["qp"], max_frames=n, bit_depth=d["bit_depth"], tiles=d["tiles"], lf_across_tiles=bool(d["lf_across_tiles"]),
                              lf_offsets=d["lf_offsets"], deblocking_metric=d["metric"], lf_offset_in_pps=bool(d["lf_offset_in_pps"]))


@pytest.mark.parametrize("entropy", [False, True], ids=["host_entropy", "device_entropy"])
@pytest.mark.parametrize("name", ref.names())
def test_picture_pipelines_reproduce_the_reference_run(name, entropy):
    """Every fixture through hevcdl_encode_pictures, _chunked and (with device entropy) _stream: the choices are the restatement's, stream and output pictures the
    reference's."""
    import hevcdl_amd
    d = ref.load(name)
    w, h, qp, bd, n = d["width"], d["height"], d["qp"], d["bit_depth"], d["yuv"].shape[0]
    deblock = not d["lf_disable"]
    kw = dict(tiles=d["tiles"], bit_depth=bd, lf_across_tiles=bool(d["lf_across_tiles"]), lf_offsets=d["lf_offsets"], lf_disable=bool(d["lf_disable"]))
    cfg = hevcdl_amd.stream_config(w, h, qp, sao=True, **kw)
    want_stream, want_pics = d["bitstream"].tobytes(), np.frombuffer(d["recon_file"].tobytes(), dt(bd)).reshape(n, -1)
    want_choices = ref.pictures(d)[2]
    enc = _encoder(d, n)
    try:
        if entropy:
            enc.enable_device_entropy(True)

        def stream_of(choices, pics, recs=None, sao=None, slices=None, sizes=None):
            out = []
            for i in range(n):
                if slices is not None:
                    au = hevcdl_amd.write_access_unit_from_slice_data(cfg, i, slices[i], sizes[i], choices[i])
                else:
                    au = hevcdl_amd.write_access_unit(w, h, qp, i, recs[i], sao=sao[i], choice=choices[i], **kw)
                out.append(au + hevcdl_amd.picture_hash_sei(w, h, pics[i], bd))
            return b"".join(out)
        recs, pics, sao, _ = enc.encode_pictures(d["yuv"], d["labels"], deblock=deblock)
        choices = enc.get_dbk_choice(0, n)
        assert choices.tolist() == want_choices.tolist()
        assert np.array_equal(pics, want_pics)
        if entropy:
            slices, sizes = enc.get_slice_data(0, n)
            assert stream_of(choices, pics, slices=slices, sizes=sizes) == want_stream
        else:
            assert stream_of(choices, pics, recs, sao) == want_stream
        enc.dbk_select_reset()      # (DeblockingFilterMetric 2 carries the previous picture's choice across calls: every call below starts the sequence again)
        seen = []
        chunks = enc.encode_pictures_chunked(d["yuv"], d["labels"], deblock=deblock, chunk_frames=2, on_chunk_hook=lambda first, count: seen.append(enc.get_dbk_choice(first, count)))
        assert np.concatenate(seen).tolist() == want_choices.tolist()
        assert np.array_equal(np.concatenate([c[2] for c in chunks]), want_pics)
        assert stream_of(want_choices, want_pics, np.concatenate([c[1] for c in chunks]), np.concatenate([c[3] for c in chunks])) == want_stream
        if entropy:
            enc.dbk_select_reset()
            seen = []
            chunks = enc.encode_pictures_stream(d["yuv"], d["labels"], deblock=deblock, want_pictures=True, chunk_frames=2, on_chunk_hook=lambda first, count: seen.append(enc.get_dbk_choice(first, count)))
            assert np.concatenate(seen).tolist() == want_choices.tolist()
            assert stream_of(want_choices, np.concatenate([c[4] for c in chunks]), slices=sum((c[1] for c in chunks), []), sizes=np.concatenate([c[2] for c in chunks])) == want_stream
        with pytest.raises(hevcdl_amd.HevcdlError):
            enc.get_dbk_choice(0, n + 1)
    finally:
        enc.close()


def trial_case(w, h, bd, tiles, seed):
    """Three unlike pictures with the TU grids of oracle/filter_cases.py (random quadtrees, 4x4 blocks everywhere, 32x32 blocks): originals, and reconstructions that are the
    originals quantised coarsely per 8x8 luma block -- steps on the 8-sample grid of a size the filters react to -- plus a little noise."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import filter_cases as fc
    rng = np.random.default_rng(seed)
    org = ref_tools.synth_yuv(w, h, 3, seed).astype(np.int64)
    recon = org.copy()
    for f in range(3):
        for off, pw, ph in ((0, w, h), (w * h, w // 2, h // 2), (w * h * 5 // 4, w // 2, h // 2)):
            p = recon[f, off:off + pw * ph].reshape(ph, pw)
            bs = 8 if off == 0 else 4      # 8 luma samples = 4 chroma samples
            q = (np.round(p.reshape(ph // bs, bs, pw // bs, bs).mean(axis=(1, 3)) / 6) * 6)
            p[:] = np.repeat(np.repeat(q, bs, axis=0), bs, axis=1) + rng.integers(-1, 2, (ph, pw))
    s = 1 << (bd - 8)
    org, recon = org * s + rng.integers(0, s, org.shape), np.clip(recon, 0, 255) * s + rng.integers(0, s, org.shape)
    recs = np.zeros((3, ((w + 63) // 64) * ((h + 63) // 64)), ref_tools.REC_DTYPE)
    grid = fc.make_records(rng, w, h, 3, "per-frame")
    recs["depth"], recs["tr_idx"] = grid["depth"], grid["tr_idx"]
    return org.astype(dt(bd)), recon.astype(dt(bd)), recs


TRIAL_SHAPES = [(64, 64, (1, 1), True), (72, 40, (1, 1), True), (264, 72, (1, 1), True), (72, 72, (1, 2), False)]      # one rectangle; a picture edge inside it; two rectangles a row; tile rows, filters stopped at the tile border


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("shape", TRIAL_SHAPES, ids=lambda s: "%dx%d_t%dx%d" % (s[0], s[1], s[2][0], s[2][1]))
def test_trial_table_equals_the_restatement(shape, bd):
    """All 49 entries of every picture of a batch of three: 49 whole-picture runs of the oracle's deblocking and numpy's squared error, shifted per sample."""
    import hevcdl_amd
    __import__("__graft_entry__").build_oracle()
    w, h, tiles, lf = shape
    qp = 30
    org, recon, recs = trial_case(w, h, bd, tiles, 31 * w + h + bd)
    d = dict(width=w, height=h, qp=qp, bit_depth=bd, tiles=tiles, lf_across_tiles=int(lf))
    want = np.stack([ref.trial_table(d, org[f], recon[f], recs[f]) for f in range(3)])
    assert all(len(set(want[f].reshape(-1).tolist())) >= 12 for f in range(3)), "the pairs must matter on this content"
    if bd == 10:      # a shift applied to the sum instead of to every sample would give another number
        pic = ref_tools.run_deblock(recon[:1], w, h, qp, recs[:1], bit_depth=bd, tiles=tiles, lf_across_tiles=lf, lf_offsets=(0, 0))[0]
        dd = org[0].astype(np.int64) - pic.astype(np.int64)
        assert int((dd * dd).sum()) >> 4 != int(want[0][3][3])
    enc = hevcdl_amd.Encoder(w, h, qp, max_frames=3, bit_depth=bd, tiles=tiles, lf_across_tiles=lf)
    try:
        got = enc.dbk_trial_frames(org, recon, recs)
        assert got.tolist() == want.tolist()
        assert enc.dbk_trial_frames(org[[2, 0]], recon[[2, 0]], recs[[2, 0]]).tolist() == want[[2, 0]].tolist()      # position in the batch does not matter
    finally:
        enc.close()


def test_mode_2_sequence_cut_into_two_calls_equals_one_call_and_reset_equals_a_fresh_context():
    import hevcdl_amd
    d = ref.load("m2_128x64_q32")
    n = d["yuv"].shape[0]
    want = ref.pictures(d)
    enc = _encoder(d, n)
    try:
        one = enc.encode_pictures(d["yuv"], d["labels"])
        whole = enc.get_dbk_choice(0, n)
        assert whole.tolist() == want[2].tolist() and np.array_equal(one[1], want[5])
        # the state is where the last picture left it: the same pictures again are pictures 4 .. 7 of a sequence, and picture 0's window is no longer the whole range
        again = enc.encode_pictures(d["yuv"][:1], d["labels"][:1])
        cont, _, _ = ref.walk(lambda b, t: ref.trial(d, d["yuv"][0], want[1][0], want[0][0], b, t), want_state(d, want), d["lf_offsets"])
        assert enc.get_dbk_choice(0, 1)[0].tolist() == cont.tolist()
        enc.dbk_select_reset()
        a = enc.encode_pictures(d["yuv"][:1], d["labels"][:1])
        ca = enc.get_dbk_choice(0, 1)
        b = enc.encode_pictures(d["yuv"][1:], d["labels"][1:])
        cb = enc.get_dbk_choice(0, n - 1)
        assert np.concatenate([ca, cb]).tolist() == whole.tolist()
        assert np.array_equal(np.concatenate([a[1], b[1]]), one[1])
        enc.dbk_select_reset()
        enc.encode_pictures(d["yuv"], d["labels"])
        assert enc.get_dbk_choice(0, n).tolist() == whole.tolist()
    finally:
        enc.close()
    fresh = _encoder(d, n)
    try:
        fresh.encode_pictures(d["yuv"], d["labels"])
        assert fresh.get_dbk_choice(0, n).tolist() == whole.tolist()
    finally:
        fresh.close()


def want_state(d, res):
    """The walk's state behind the last picture of fixture d (CPU pipeline results res)."""
    state = [0, 0, 0, 0]
    for f in range(d["yuv"].shape[0]):
        _, state, _ = ref.walk(lambda b, t: ref.trial(d, d["yuv"][f], res[1][f], res[0][f], b, t), state, d["lf_offsets"])
    return state


def test_metric_with_the_filter_off_is_refused_at_the_call():
    import hevcdl_amd
    d = ref.load("m1_64x64_q12")
    enc = _encoder(d, 1)
    try:
        with pytest.raises(hevcdl_amd.HevcdlError, match="both LoopFilterDisable and LoopFilterOffsetInPPS must be 0"):
            enc.encode_pictures(d["yuv"][:1], d["labels"][:1], deblock=False)
    finally:
        enc.close()


def log_of(lines):
    """Picture lines without [ET ...] and the reference build's "nQP <n> ", with their hash text, and the two lines of the summary block."""
    poc = [re.sub(r"nQP -?\d+ ", "", qr.strip_et(l)) + " " + l[l.index("[MD5:"):].strip() for l in lines if l.startswith("POC")]
    i = next(k for k, l in enumerate(lines) if l.startswith("SUMMARY"))
    return poc, [l.rstrip() for l in lines[i + 1:i + 3]]


@pytest.mark.parametrize("name", ref.names())
def test_cli_reproduces_the_reference_run(name, tmp_path):
    """The reference's own keys on the reference's own input: stream and reconstruction file byte for byte, picture lines and summary as the reference printed them; with
    --DeviceEntropy=1 --DeviceReport=1 the same once more; a metric 1 run dealt to two device entries the same again (the metric keeps no state)."""
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    d = ref.load(name)
    n = d["yuv"].shape[0]
    d["yuv"].astype(dt(d["bit_depth"])).tofile(tmp_path / "in.yuv")
    for f in range(n):
        os.makedirs(tmp_path / "pred" / str(f))
        for a in range(d["labels"].shape[1]):
            (tmp_path / "pred" / str(f) / ("ctu%d.txt" % a)).write_text(" ".join(str(int(v)) for v in d["labels"][f, a]) + " ")
    base = [app, "-i", "in.yuv", "-wdt", str(d["width"]), "-hgt", str(d["height"]), "-q", str(d["qp"]), "-f", str(n), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=1",
            "--InputBitDepth=%d" % d["bit_depth"], "--Profile=%s" % ("main" if d["bit_depth"] == 8 else "main10")] + [str(k) for k in d["keys"]]
    want = log_of([str(l) for l in d["stdout"]])
    runs = [("plain", []), ("device", ["--DeviceEntropy=1", "--DeviceReport=1"])] + ([("multi", ["--Devices=0,0"])] if name == "m1_128x64_q45" else [])
    for tag, extra in runs:
        r = subprocess.run(base + ["-b", tag + ".bin", "-o", tag + ".yuv"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert (tmp_path / (tag + ".bin")).read_bytes() == d["bitstream"].tobytes(), tag
        assert (tmp_path / (tag + ".yuv")).read_bytes() == d["recon_file"].tobytes(), tag
        if tag != "multi":
            assert log_of(r.stdout.splitlines()) == want, tag
