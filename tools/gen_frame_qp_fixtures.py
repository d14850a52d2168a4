#!/usr/bin/env python3
"""Writes tests/golden/fqp_*.npz: runs of the reference encoder (oracle/_ref, built by build()) with its per-picture QP keys -- dQPFile, QPIncrementFrame, IntraQPOffset,
LambdaModifierI, LambdaModifier0.  Each file holds the source frames as the reference read them (FrameSkip frames in front included), the labels (through label files: the
CNN plays no part), the keys, the text of the dQP file, the QP of every picture by the rule restated below, the records and the unfiltered reconstruction behind every
compressCtu, the deblocked picture (the reconstruction file of the same run with --SAO=0), the final picture (the reconstruction file), both streams and the log lines.
Only data goes into the files.

The script asserts what it writes, and tests/test_frame_qp.py asserts the same on the committed files:
  * the slice QPs parsed from the stream (oracle/hevc_parse.py) are the rule's, in both runs;
  * fixture d192_q32 ends with three distinct QPs of which none is one contiguous run: otherwise the permuted path is not exercised and the fixture is void."""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hevc_parse   # noqa: E402
import ref_tools    # noqa: E402

DQP = "0 2 0 -1 2 0"


def case(w=192, h=128, qp=32, bd=8, frames=6, dqp=None, qpif=None, frame_skip=0, intra_qp_offset=0, lmi=None, lm0=None, tiles=(1, 1), wpp=0, slices=None):
    return dict(w=w, h=h, qp=qp, bd=bd, frames=frames, dqp=dqp, qpif=qpif, frame_skip=frame_skip, intra_qp_offset=intra_qp_offset, lmi=lmi, lm0=lm0, tiles=tiles, wpp=wpp, slices=slices)


CASES = {
    "d192_q32": case(dqp=DQP),                                          # 1: three QPs, none contiguous: the permuted path
    "i192_q32_s1": case(qpif=3, frame_skip=1),                          # 2: the switch at POC 2; contiguous runs, no copy
    "di192_q32": case(qpif=2, dqp="0 -1 2 0"),                          # 3: the file wins where it has values; four values cover six pictures
    "o192_q32_lmi": case(intra_qp_offset=-2, lmi=1.5, frames=3),        # 4a: IntraQPOffset -2 with LambdaModifierI 1.5
    "o192_q32_lm0": case(lm0=0.8, frames=3),                            # 4b: LambdaModifier0 0.8 alone
    "w192_q32": case(dqp=DQP, wpp=1),                                   # 5a: WaveFrontSynchro 1
    "t512_q32": case(w=512, dqp="0 2 0 -1", frames=4, tiles=(2, 1)),                  # 5b: 2 x 1 tiles (512 wide: the reference asserts tile columns of four CTUs at the least)
    "d192_q32_b10": case(dqp=DQP, bd=10),                               # 6a: ten bits
    "c192_q50": case(qp=50, dqp="1 3"),                                 # 6b: the QP clips at 51
    "s192_q32": case(dqp=DQP, slices=(1, 3)),                           # 7: SliceMode 1, a CTU row a slice
}


def offsets_of(c):
    """TAppEncCfg.cpp:1663-1681 (the increment), :1735-1753 (the file, read afterwards)"""
    n = c["frames"]
    d = [0] * n
    if c["qpif"] is not None:
        sw = (c["qpif"] - c["frame_skip"]) // 1 if c["qpif"] > c["frame_skip"] else 0
        for i in range(sw, n):
            d[i] = 1
    if c["dqp"]:
        for i, v in enumerate(c["dqp"].split()[:n]):
            d[i] = int(v)
    return d


def qps_of(c):
    """TEncTop.cpp:1409-1423, 1449 for an I slice"""
    return [max(-6 * (c["bd"] - 8), min(51, c["qp"] + d + c["intra_qp_offset"])) for d in offsets_of(c)]


def ref_args(c, sao=1):
    a = ["--SAO=%d" % sao, "--WaveFrontSynchro=%d" % c["wpp"], "--FramesToBeEncoded=%d" % c["frames"]]
    if c["frame_skip"]:
        a += ["--FrameSkip=%d" % c["frame_skip"]]
    if c["dqp"]:
        a += ["--dQPFile=dqp.txt"]
    if c["qpif"] is not None:
        a += ["--QPIncrementFrame=%d" % c["qpif"]]
    if c["intra_qp_offset"]:
        a += ["--IntraQPOffset=%d" % c["intra_qp_offset"]]
    if c["lmi"] is not None:
        a += ["--LambdaModifierI=%s" % c["lmi"]]
    if c["lm0"] is not None:
        a += ["--LambdaModifier0=%s" % c["lm0"]]
    if c["tiles"] != (1, 1):
        a += ref_tools.tile_args(c["tiles"])
    if c["slices"]:
        a += ["--SliceMode=%d" % c["slices"][0], "--SliceArgument=%d" % c["slices"][1]]
    return a


def slice_qps(stream):
    """26 + slice_qp_delta of every slice NAL of the stream (init_qp_minus26 is 0)."""
    sps = pps = None
    out = []
    for _, n in hevc_parse.split_annexb(stream):
        t = (n[0] >> 1) & 63
        if t == 33:
            sps = hevc_parse.parse_sps(n)
        elif t == 34:
            pps = hevc_parse.parse_pps(n)
            assert pps["init_qp_m26"] == 0
        elif t <= 21:
            out.append(26 + hevc_parse.parse_slice_header(n, sps, pps)[0]["qp_delta"])
    return out


def prefilter_frames(dump, c, nf, nctu):
    """The reconstruction before the in-loop filters as frames, from the per-CTU blocks behind every compressCtu."""
    w, h, cx = c["w"], c["h"], (c["w"] + 63) // 64
    dt = np.uint8 if c["bd"] == 8 else np.dtype("<u2")
    frames = np.zeros((nf, w * h * 3 // 2), dt)
    for fr in range(nf):
        Y = np.zeros((h + 64, w + 64), dt); U = np.zeros((h // 2 + 32, w // 2 + 32), dt); V = U.copy()
        for a in range(nctu):
            x0, y0 = (a % cx) * 64, (a // cx) * 64
            Y[y0:y0 + 64, x0:x0 + 64] = dump["rec_y"][fr, a].reshape(64, 64)
            U[y0 // 2:y0 // 2 + 32, x0 // 2:x0 // 2 + 32] = dump["rec_cb"][fr, a].reshape(32, 32)
            V[y0 // 2:y0 // 2 + 32, x0 // 2:x0 // 2 + 32] = dump["rec_cr"][fr, a].reshape(32, 32)
        frames[fr] = np.concatenate([Y[:h, :w].ravel(), U[:h // 2, :w // 2].ravel(), V[:h // 2, :w // 2].ravel()])
    return frames


def run(c, yuv, labels, sao):
    d = tempfile.mkdtemp(prefix="fqp_")
    try:
        if c["dqp"]:
            with open(os.path.join(d, "dqp.txt"), "w") as fh:
                fh.write(c["dqp"] + "\n")
        return ref_tools.run_reference(yuv, c["w"], c["h"], c["qp"], labels, extra_args=ref_args(c, sao), keep_dir=d, bit_depth=c["bd"])
    finally:
        shutil.rmtree(d)


def main():
    if not os.path.exists(ref_tools.REF_ENC):
        sys.exit("oracle/_ref/TAppEncoder_ref is missing: run build() first")
    only = sys.argv[1:]
    for name, c in CASES.items():
        if only and name not in only:
            continue
        seed = 1100 + sorted(CASES).index(name)
        w, h, bd, nf, skip = c["w"], c["h"], c["bd"], c["frames"], c["frame_skip"]
        yuv = ref_tools.synth_yuv(w, h, nf + skip, seed)
        if bd > 8:
            yuv = (yuv.astype(np.uint16) << (bd - 8)) | np.random.default_rng(seed).integers(0, 1 << (bd - 8), yuv.shape).astype(np.uint16)
        labels = ref_tools.make_labels(w, h, nf + skip, "rand", seed=seed)
        nctu = labels.shape[1]
        qps = qps_of(c)
        dump, stdout, stream, recon = run(c, yuv, labels, 1)
        assert dump.shape[0] == nf * nctu, (name, dump.shape)
        dump = dump.reshape(nf, nctu)
        dump = np.take_along_axis(dump, np.argsort(dump["addr"], axis=1, kind="stable"), axis=1)      # tiles: the CTUs come in tile scan
        assert (dump["addr"] == np.arange(nctu)[None, :]).all() and (dump["frame"] == np.arange(nf)[:, None]).all()
        _, _, stream0, deblocked = run(c, yuv, labels, 0)
        for s in (stream, stream0):
            got = slice_qps(s)
            per = len(got) // nf
            assert len(got) == per * nf and got == [q for q in qps for _ in range(per)], (name, got, qps)
        if name == "d192_q32":
            starts = [qps[i] for i in range(nf) if i == 0 or qps[i] != qps[i - 1]]      # the QP of every run of the list
            assert len(set(qps)) == 3 and len(starts) > len(set(starts)), qps               # a QP comes back after another: the pictures have to be brought together
        assert len(deblocked) == len(recon)
        out = os.path.join(ROOT, "tests", "golden", "fqp_%s.npz" % name)
        np.savez_compressed(out, width=w, height=h, qp=c["qp"], bit_depth=bd, seed=seed, tiles=np.array(c["tiles"], np.int32), wavefront=c["wpp"], frame_skip=skip,
                            slices=np.array(c["slices"] or (0, 0), np.int32), qp_increment_frame=-1 if c["qpif"] is None else c["qpif"], intra_qp_offset=c["intra_qp_offset"],
                            lambda_modifier_i=-1.0 if c["lmi"] is None else c["lmi"], lambda_modifier_0=-1.0 if c["lm0"] is None else c["lm0"], dqp_text=np.array(c["dqp"] or ""),
                            dqp=np.array(offsets_of(c), np.int32), qps=np.array(qps, np.int32), yuv=yuv, labels=labels[:nf], records=dump["rec"], prefilter=prefilter_frames(dump, c, nf, nctu),
                            bitstream=np.frombuffer(stream, np.uint8), bitstream_nosao=np.frombuffer(stream0, np.uint8), recon_file=np.frombuffer(recon, np.uint8),
                            deblocked_file=np.frombuffer(deblocked, np.uint8), keys=np.array(ref_args(c), dtype=str),
                            stdout=np.array([l for l in stdout.splitlines() if l.startswith("POC") or "SUMMARY" in l or "Total Frames" in l or l.startswith("\t ") or l.startswith("QP  ")]))
        print("%s: seed %d, QPs %s, stream %d bytes, file %d bytes" % (name, seed, qps, len(stream), os.path.getsize(out)))
        assert os.path.getsize(out) < 1 << 20, "a committed file stays below 1 MiB"


if __name__ == "__main__":
    main()
