#!/usr/bin/env python3
"""Writes tests/golden/slices_*.npz: runs of the reference encoder (oracle/_ref, built by build()) with slices -- SliceMode 1 over whole CTU rows, SliceMode 3 over
tiles -- and LFCrossSliceBoundaryFlag.  Each file holds the frames, the labels (through label files: the CNN plays no part), the reference's records and unfiltered
reconstruction after every compressCtu (oracle/ref_hook.cpp), its stream, the bytes of its reconstruction file, the picture and summary lines of its log and the keys.
Only data goes into the files.

The script asserts what it writes, and tests/test_slices.py asserts the same on the committed files:
  * the number of slice NAL units per access unit;
  * the stream differs from the one-slice run of the same frames;
  * the reference decoder, where built, returns the reconstruction file with no hash complaint;
  * for the SliceMode 1 cases that are at least four CTUs wide (a tile column's minimum), records, unfiltered reconstruction and reconstruction file equal those of the run
    with tile rows of full width instead (LFCrossTileBoundaryFlag = LFCrossSliceBoundaryFlag); for the SliceMode 3 cases they equal those of the tiles-only run;
  * on a border that is both a tile and a slice border (SliceMode 3) the in-loop filters cross only when BOTH flags are 1: with a tile a slice, the run with
    LFCrossSliceBoundaryFlag 0 and LFCrossTileBoundaryFlag 1 gives the reconstruction file of the tiles-only run with LFCrossTileBoundaryFlag 0;
  * a tile border INSIDE a slice follows LFCrossTileBoundaryFlag alone: three tiles a slice with the flags 0 and 1 is neither tiles-only run (checked here, not kept: the
    library refuses that combination, its filters have one flag for all tile borders)."""
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


def case(w, h, qp, mode, arg, lf=1, bd=8, tiles=(1, 1), lf_tiles=1, extra=(), tools=TOOLS, sao=1, lf_disable=0, in_pps=1, offsets=(0, 0), wide_twin=False, n=2):
    return dict(w=w, h=h, qp=qp, mode=mode, arg=arg, lf=lf, bd=bd, tiles=tiles, lf_tiles=lf_tiles, extra=list(extra), tools=tools, sao=sao, lf_disable=lf_disable, in_pps=in_pps,
                offsets=offsets, wide_twin=wide_twin, n=n)


CASES = {
    "r128_a2": case(128, 128, 32, 1, 2),                                                       # two CTUs wide: under the tile limit, one row a slice
    "r192x200_a6": case(192, 200, 27, 1, 6),                                                   # 3 x 4 CTUs, partial last row, two rows a slice
    "r192x200_a6_lf0": case(192, 200, 27, 1, 6, lf=0),                                         # ... the filters stop at the slice border
    "c64x192_a1": case(64, 192, 37, 1, 1),                                                     # one CTU column: every CTU a slice
    "r128_a2_b10": case(128, 128, 32, 1, 2, bd=10),
    "r128_a2_off": case(128, 128, 32, 1, 2, sao=0, lf_disable=1),                              # no in-loop filter: the header has no across-slices flag
    "r128_a2_k": case(128, 128, 32, 1, 2, tools=TOOLS & ~(ref_tools.TOOL_RDOQ | ref_tools.TOOL_SIGN_HIDE)),
    "r128_a2_inpps0": case(128, 128, 32, 1, 2, in_pps=0, offsets=(2, -1)),                     # the override repeated in every header
    "r264x136_a5_lf0": case(264, 136, 32, 1, 5, lf=0, wide_twin=True),                         # five CTUs wide, partial column and row: held to the tile-row run
    "t512_a1": case(512, 128, 32, 3, 1, tiles=(2, 2), n=1),                                      # a tile a slice
    "t512_a3": case(512, 128, 32, 3, 3, tiles=(2, 2)),                                         # three tiles with entry points, then one
    "t512_a1_lf0": case(512, 128, 32, 3, 1, lf=0, tiles=(2, 2), n=1),                            # LFCrossSliceBoundaryFlag 0 beside LFCrossTileBoundaryFlag 1: every tile border is a slice border
}


def ref_args(c, slices=True):
    a = ["--SAO=%d" % c["sao"], "--LoopFilterDisable=%d" % c["lf_disable"], "--LoopFilterOffsetInPPS=%d" % c["in_pps"],
         "--LoopFilterBetaOffset_div2=%d" % c["offsets"][0], "--LoopFilterTcOffset_div2=%d" % c["offsets"][1]] + ref_tools.tool_args(c["tools"])
    if c["tiles"] != (1, 1):
        a += ref_tools.tile_args(c["tiles"]) + ["--LFCrossTileBoundaryFlag=%d" % c["lf_tiles"]]
    if slices:
        a += ["--SliceMode=%d" % c["mode"], "--SliceArgument=%d" % c["arg"], "--LFCrossSliceBoundaryFlag=%d" % c["lf"]]
    return a


def unit_grid(c):
    """The tile grid that computes what the case's slices compute: ([widths], [heights]) in CTUs, and the flag that lets the filters cross its borders."""
    cx, cy = (c["w"] + 63) // 64, (c["h"] + 63) // 64
    if c["mode"] == 3:
        return c["tiles"], bool(c["lf_tiles"] and c["lf"])
    rows = c["arg"] // cx
    return ([cx], [min(rows, cy - r) for r in range(0, cy, rows)]), bool(c["lf"])


def slice_nals(stream):
    """Slice NAL units (types 0 .. 21) per access unit: an access unit starts at a VPS."""
    counts = []
    for _, n in hevc_parse.split_annexb(stream):
        t = (n[0] >> 1) & 63
        if t == 32:
            counts.append(0)
        elif t <= 21:
            counts[-1] += 1
    return counts


def expected_slices(c):
    cx, cy = (c["w"] + 63) // 64, (c["h"] + 63) // 64
    units = cx * cy if c["mode"] == 1 else c["tiles"][0] * c["tiles"][1]
    return (units + c["arg"] - 1) // c["arg"]


def decode(stream, n_bytes):
    """The reference decoder's reconstruction of `stream` and its log, or (None, None) where it is not built."""
    if not os.path.exists(ref_tools.REF_DEC):
        return None, None
    with tempfile.TemporaryDirectory(prefix="hmdec_") as d:
        open(os.path.join(d, "s.bin"), "wb").write(stream)
        p = subprocess.run([ref_tools.REF_DEC, "-b", "s.bin", "-o", "d.yuv"], cwd=d, capture_output=True, text=True)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return open(os.path.join(d, "d.yuv"), "rb").read(), p.stdout


def frames_of(c, seed, n=2):
    yuv = ref_tools.synth_yuv(c["w"], c["h"], n, seed)
    if c["bd"] > 8:
        yuv = (yuv.astype(np.uint16) << (c["bd"] - 8)) | np.random.default_rng(seed).integers(0, 1 << (c["bd"] - 8), yuv.shape).astype(np.uint16)
    return yuv, ref_tools.make_labels(c["w"], c["h"], n, "rand", seed=seed)


def sorted_dump(dump):
    return dump[np.lexsort((dump["addr"], dump["frame"]))]


def main():
    if not os.path.exists(ref_tools.REF_ENC):
        sys.exit("oracle/_ref/TAppEncoder_ref is missing: run build() first")
    only = sys.argv[1:]
    for name, c in CASES.items():
        if only and name not in only:
            continue
        seed = 700 + sorted(CASES).index(name)
        w, h, bd = c["w"], c["h"], c["bd"]
        yuv, labels = frames_of(c, seed, c["n"])
        nf, nctu = labels.shape[0], labels.shape[1]
        dump, stdout, stream, recon = ref_tools.run_reference(yuv, w, h, c["qp"], labels, extra_args=ref_args(c), bit_depth=bd)
        dump = sorted_dump(dump)
        assert slice_nals(stream) == [expected_slices(c)] * nf, (name, slice_nals(stream))
        # the one-slice run of the same frames (tiles kept): another stream
        dump1, _, stream1, recon1 = ref_tools.run_reference(yuv, w, h, c["qp"], labels, extra_args=ref_args(c, slices=False), bit_depth=bd)
        assert stream1 != stream and slice_nals(stream1) == [1] * nf
        dec, dec_log = decode(stream, len(recon))
        if dec is not None:
            assert dec == recon and "ERROR" not in dec_log and dec_log.count("(OK)") == nf, (name, dec_log[-500:])
        grid, lf_grid = unit_grid(c)
        if c["mode"] == 3:      # pure syntax: the tiles-only run computes the same, with the flag the two combine to
            twin = dict(c, lf_tiles=int(lf_grid))
            dump_t, _, _, recon_t = ref_tools.run_reference(yuv, w, h, c["qp"], labels, extra_args=ref_args(twin, slices=False), bit_depth=bd)
            assert sorted_dump(dump_t).tobytes() == dump.tobytes() and recon_t == recon, name + ": SliceMode 3 is not the tiles-only run"
            if not c["lf"]:     # ... and it is NOT the run that lets the filters cross (the fixture decides how the two flags combine)
                assert recon1 != recon, name + ": LFCrossSliceBoundaryFlag 0 had no effect on a tile border"
        elif c["wide_twin"]:    # row slices == tile rows of full width
            twin = dict(c, tiles=grid, lf_tiles=int(lf_grid))
            dump_t, _, _, recon_t = ref_tools.run_reference(yuv, w, h, c["qp"], labels, extra_args=ref_args(twin, slices=False), bit_depth=bd)
            assert sorted_dump(dump_t).tobytes() == dump.tobytes() and recon_t == recon, name + ": row slices are not the tile-row run"
        out = os.path.join(ROOT, "tests", "golden", "slices_%s.npz" % name)
        np.savez_compressed(out, width=w, height=h, qp=c["qp"], bit_depth=bd, seed=seed, slice_mode=c["mode"], slice_argument=c["arg"], lf_across_slices=c["lf"],
                            tiles=np.array(c["tiles"], np.int32), lf_across_tiles=c["lf_tiles"], tools=c["tools"], sao=c["sao"], lf_disable=c["lf_disable"],
                            lf_offset_in_pps=c["in_pps"], lf_offsets=np.array(c["offsets"], np.int32), n_slices=expected_slices(c),
                            grid_cols=np.array(grid[0], np.int32) if c["mode"] == 1 else np.zeros(0, np.int32), grid_rows=np.array(grid[1], np.int32) if c["mode"] == 1 else np.zeros(0, np.int32),
                            lf_grid=int(lf_grid), yuv=yuv, labels=labels, records=dump["rec"].reshape(nf, nctu),
                            rec_y=dump["rec_y"].reshape(nf, nctu, 4096), rec_cb=dump["rec_cb"].reshape(nf, nctu, 1024), rec_cr=dump["rec_cr"].reshape(nf, nctu, 1024),
                            bitstream=np.frombuffer(stream, np.uint8), bitstream_one_slice=np.frombuffer(stream1, np.uint8), recon_file=np.frombuffer(recon, np.uint8),
                            keys=np.array(ref_args(c), dtype=str),
                            stdout=np.array([l for l in stdout.splitlines() if l.startswith("POC") or "SUMMARY" in l or "Total Frames" in l or l.startswith("\t ")]))
        if name == "t512_a3":   # the combination the library refuses: borders inside a slice are crossed, borders between slices are not
            mixed = ref_tools.run_reference(yuv, w, h, c["qp"], labels, extra_args=ref_args(dict(c, lf=0)), bit_depth=bd)[3]
            closed = ref_tools.run_reference(yuv, w, h, c["qp"], labels, extra_args=ref_args(dict(c, lf_tiles=0), slices=False), bit_depth=bd)[3]
            assert mixed != recon and mixed != closed, "three tiles a slice, LFCrossSliceBoundaryFlag 0, LFCrossTileBoundaryFlag 1: expected a picture of its own"
        print("%s: seed %d, %d slices a picture, stream %d bytes (one slice: %d), file %d bytes" % (name, seed, expected_slices(c), len(stream), len(stream1), os.path.getsize(out)))


if __name__ == "__main__":
    main()
