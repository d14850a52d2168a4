#!/usr/bin/env python3
"""Writes tests/golden/segments_*.npz: runs of the reference encoder (oracle/_ref, built by build()) with dependent slice segments -- SliceSegmentMode 1 over the CTU
rows of a WaveFrontSynchro picture, SliceSegmentMode 3 over tiles.  Each file holds the frames, the labels (through label files: the CNN plays no part), the
reference's records and unfiltered reconstruction after every compressCtu (oracle/ref_hook.cpp), the deblocked picture (the reconstruction file of the run with
--SAO=0) and the final one (the reconstruction file), both streams (with SAO and with --SAO=0), the picture and summary lines of the log and the keys.  Only data goes
into the files.  To keep them small the two filtered pictures are stored as what each filter changed: deblocked_delta = deblocked - unfiltered and
final_delta = final - deblocked, int16 per sample in the file's plane order (tests/segments_cases.py puts them together again).

The script asserts what it writes, and tests/test_segments.py asserts what can be asserted on the committed files:
  * records, unfiltered reconstruction and reconstruction file EQUAL those of the run without the segment keys -- the feature is syntax only where a segment starts where
    the coder is initialised anyway; the length of that run's stream is kept for the record;
  * the run with --SAO=0 has the same records;
  * the number and the types of the slice NAL units per access unit, and which of them are dependent;
  * the reference decoder, where built, returns the reconstruction file with no hash complaint.
The combination SliceMode 3 + SliceSegmentMode 3 is kept only because this script finds it neutral in the same way (t512x128_s2_a1).

What the library refuses is measured here too (`python tools/gen_segment_fixtures.py --refused`): segments that are not whole rows, and segments without
WaveFrontSynchro, change the reference's records."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hevc_parse   # noqa: E402
import ref_tools    # noqa: E402

TOOLS = ref_tools.TOOLS_REFERENCE


def case(w, h, qp, mode, arg, wpp=False, tiles=(1, 1), slices=None, n=2):
    return dict(w=w, h=h, qp=qp, mode=mode, arg=arg, wpp=wpp, tiles=tiles, slices=slices, n=n)


CASES = {
    "w264x136_a5": case(264, 136, 32, 1, 5, wpp=True),                              # 5 x 3 CTUs, partial last column and row: a row a segment
    "w264x264_a10": case(264, 264, 37, 1, 10, wpp=True),                            # 5 x 5 CTUs: segments of 2 + 2 + 1 rows, an entry point inside a segment (QP 37 keeps the file under the slice fixtures' size)
    "w64x192_a1": case(64, 192, 32, 1, 1, wpp=True),                                # one CTU wide: every CTU a segment, no CTU above-right to take contexts from
    "t512x128_a1": case(512, 128, 32, 3, 1, tiles=(2, 2)),                          # a tile a segment
    "t512x128_a3": case(512, 128, 32, 3, 3, tiles=(2, 2)),                          # segments of 3 + 1 tiles, entry points inside
    "t512x128_s2_a1": case(512, 128, 32, 3, 1, tiles=(2, 2), slices=(3, 2)),        # two slices of two tiles: an independent header in mid-picture, then a dependent one
}


def ref_args(c, segments=True, sao=1):
    a = ["--SAO=%d" % sao] + ref_tools.tool_args(TOOLS)
    if c["wpp"]:
        a += ["--WaveFrontSynchro=1"]
    if c["tiles"] != (1, 1):
        a += ref_tools.tile_args(c["tiles"]) + ["--LFCrossTileBoundaryFlag=1"]
    if c["slices"]:
        a += ["--SliceMode=%d" % c["slices"][0], "--SliceArgument=%d" % c["slices"][1], "--LFCrossSliceBoundaryFlag=1"]
    if segments:
        a += ["--SliceSegmentMode=%d" % c["mode"], "--SliceSegmentArgument=%d" % c["arg"]]
    return a


def slice_nals(stream):
    """Per access unit (one starts at a VPS): [(NAL unit type, dependent_slice_segment_flag)] of its slice NAL units.  The flag follows first_slice_segment_in_pic_flag 0,
    no_output_of_prior_pics_flag and slice_pic_parameter_set_id 0 (one bit) in the streams of this script, all of IRAP pictures with dependent segments enabled."""
    out = []
    for _, n in hevc_parse.split_annexb(stream):
        t = (n[0] >> 1) & 63
        if t == 32:
            out.append([])
        elif t <= 21:
            first = n[2] >> 7
            out[-1].append((t, 0 if first else (n[2] >> 4) & 1))
    return out


def expected_nals(c):
    """[dependent flag] of the segments of one picture."""
    cx, cy = (c["w"] + 63) // 64, (c["h"] + 63) // 64
    units = cy if c["mode"] == 1 else c["tiles"][0] * c["tiles"][1]
    seg = c["arg"] // cx if c["mode"] == 1 else c["arg"]
    per = c["slices"][1] if c["slices"] else units
    flags = []
    for k0 in range(0, units, per):
        k1 = min(k0 + per, units)
        flags += [int(s0 > k0) for s0 in range(k0, k1, seg)]
    return flags


def decode(stream):
    """The reference decoder's reconstruction of `stream` and its log, or (None, None) where it is not built."""
    if not os.path.exists(ref_tools.REF_DEC):
        return None, None
    with tempfile.TemporaryDirectory(prefix="hmdec_") as d:
        open(os.path.join(d, "s.bin"), "wb").write(stream)
        p = subprocess.run([ref_tools.REF_DEC, "-b", "s.bin", "-o", "d.yuv"], cwd=d, capture_output=True, text=True)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return open(os.path.join(d, "d.yuv"), "rb").read(), p.stdout


def unfiltered_frames(dump, w, h, nf):
    """The per-CTU blocks behind every compressCtu as planar frames [nf, w * h * 3 / 2]."""
    cx, nctu = (w + 63) // 64, len(dump) // nf
    frames = np.zeros((nf, w * h * 3 // 2), np.uint8)
    for fr in range(nf):
        Y = np.zeros((h + 64, w + 64), np.uint8); U = np.zeros((h // 2 + 32, w // 2 + 32), np.uint8); V = U.copy()
        for a in range(nctu):
            d = dump[fr * nctu + a]
            x0, y0 = (a % cx) * 64, (a // cx) * 64
            Y[y0:y0 + 64, x0:x0 + 64] = d["rec_y"].reshape(64, 64)
            U[y0 // 2:y0 // 2 + 32, x0 // 2:x0 // 2 + 32] = d["rec_cb"].reshape(32, 32)
            V[y0 // 2:y0 // 2 + 32, x0 // 2:x0 // 2 + 32] = d["rec_cr"].reshape(32, 32)
        frames[fr] = np.concatenate([Y[:h, :w].ravel(), U[:h // 2, :w // 2].ravel(), V[:h // 2, :w // 2].ravel()])
    return frames


def sorted_dump(dump):
    return dump[np.lexsort((dump["addr"], dump["frame"]))]


def run(c, yuv, labels, **kw):
    dump, stdout, stream, recon = ref_tools.run_reference(yuv, c["w"], c["h"], c["qp"], labels, extra_args=ref_args(c, **kw))
    return sorted_dump(dump), stdout, stream, recon


def refused():
    """The measurements behind the library's refusals: where a segment starts in the middle of a coder chain the reference decides differently."""
    for name, c in (("wavefront, 3 CTUs a segment (not whole rows)", case(264, 136, 32, 1, 3, wpp=True)), ("wavefront, 7 CTUs a segment", case(264, 136, 32, 1, 7, wpp=True)),
                    ("no wavefront, a row a segment", case(264, 136, 32, 1, 5))):
        yuv, labels = ref_tools.synth_yuv(c["w"], c["h"], 1, 790), ref_tools.make_labels(c["w"], c["h"], 1, "rand", seed=790)
        dump = run(c, yuv, labels)[0]
        base = run(c, yuv, labels, segments=False)[0]
        differ = [int(a) for a in range(len(dump)) if dump[a:a + 1].tobytes() != base[a:a + 1].tobytes()]
        assert differ, name + ": expected other records than the run without segments"
        print("%s: records differ from CTU %d on (%d of %d CTUs)" % (name, differ[0], len(differ), len(dump)))


def main():
    if not os.path.exists(ref_tools.REF_ENC):
        sys.exit("oracle/_ref/TAppEncoder_ref is missing: run build() first")
    if sys.argv[1:] == ["--refused"]:
        return refused()
    only = sys.argv[1:]
    for name, c in CASES.items():
        if only and name not in only:
            continue
        seed = 800 + sorted(CASES).index(name)
        w, h = c["w"], c["h"]
        yuv, labels = ref_tools.synth_yuv(w, h, c["n"], seed), ref_tools.make_labels(w, h, c["n"], "rand", seed=seed)
        nf, nctu = labels.shape[0], labels.shape[1]
        dump, stdout, stream, recon = run(c, yuv, labels)
        dump0, _, stream0, recon0 = run(c, yuv, labels, sao=0)                     # no SAO: the other stream, and the deblocked picture as a file
        base, _, stream_base, recon_base = run(c, yuv, labels, segments=False)     # the run without the keys
        assert base.tobytes() == dump.tobytes() and recon_base == recon, name + ": the segment keys changed the reference's records or its reconstruction file"
        assert dump0["rec"].tobytes() == dump["rec"].tobytes(), name + ": --SAO=0 changed the records"
        assert stream_base != stream
        want = expected_nals(c)
        for s in (stream, stream0):
            got = slice_nals(s)
            assert [[d for _, d in au] for au in got] == [want] * nf, (name, got)
            assert [[t for t, _ in au] for au in got] == [[19 if poc == 0 else 21] * len(want) for poc in range(nf)], (name, got)
            dec, dec_log = decode(s)
            if dec is not None:
                assert dec == (recon if s is stream else recon0) and "ERROR" not in dec_log and dec_log.count("(OK)") == nf, (name, dec_log[-500:])
        keep = lambda text: np.array([l for l in text.splitlines() if l.startswith("POC") or "SUMMARY" in l or "Total Frames" in l or l.startswith("\t ")])
        unf = unfiltered_frames(dump, w, h, nf).astype(np.int16).ravel()
        dbk, fin = np.frombuffer(recon0, np.uint8).astype(np.int16), np.frombuffer(recon, np.uint8).astype(np.int16)
        out = os.path.join(ROOT, "tests", "golden", "segments_%s.npz" % name)
        np.savez_compressed(out, width=w, height=h, qp=c["qp"], bit_depth=8, seed=seed, segment_mode=c["mode"], segment_argument=c["arg"], wavefront=int(c["wpp"]),
                            tiles=np.array(c["tiles"], np.int32), slices=np.array(c["slices"] or (0, 0), np.int32), tools=TOOLS, dependent=np.array(want, np.int32),
                            yuv=yuv, labels=labels, records=dump["rec"].reshape(nf, nctu),
                            rec_y=dump["rec_y"].reshape(nf, nctu, 4096), rec_cb=dump["rec_cb"].reshape(nf, nctu, 1024), rec_cr=dump["rec_cr"].reshape(nf, nctu, 1024),
                            deblocked_delta=dbk - unf, final_delta=fin - dbk,
                            bitstream=np.frombuffer(stream, np.uint8), bitstream_nosao=np.frombuffer(stream0, np.uint8), base_stream_bytes=len(stream_base),
                            keys=np.array(ref_args(c), dtype=str), stdout=keep(stdout))
        print("%s: seed %d, %d segments a picture %s, stream %d bytes (without the keys: %d), file %d bytes" % (name, seed, len(want), want, len(stream), len(stream_base), os.path.getsize(out)))


if __name__ == "__main__":
    main()
