#!/usr/bin/env python3
"""Writes tests/golden/dqr_*.npz: runs of the reference encoder (oracle/_ref, built by build()) with --DeltaQpRD=N.  oracle/ref_hook.cpp fires after every compressCtu,
so a picture's dump holds 2N+2 passes: the 2N+1 trials of TEncSlice::precompressSlice in candidate order (QP, QP-1, QP+1, ...) and the final compressSlice at the winning
QP.  The script splits them.  Each file holds the frames, the labels (through label files: the CNN plays no part), bits and dist of every CTU of every candidate, the final
pass's records and unfiltered reconstruction, the deblocked picture (the reconstruction file of the same run with --SAO=0: the trials do not see the SAO switch), the
stream, the bytes of the reconstruction file (the final picture), the log lines and the keys.  Only data goes into the files.

The script asserts what it writes, and tests/test_deltaqprd.py asserts the same on the committed files:
  * the final pass equals the winning trial pass, records and reconstruction: this project keeps the winning trial instead of coding the picture again;
  * the QP read from slice_qp_delta (oracle/hevc_parse.py) is the QP of the candidate the pick rule -- restated below from TEncSlice.cpp:646-652 -- gives on the stored sums;
  * across the set at least two different indices win, one of them non-zero, and in at least one fixture two pictures end at different QPs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hevc_parse   # noqa: E402
import ref_tools    # noqa: E402

TOOLS = ref_tools.TOOLS_REFERENCE


def case(w, h, qp, n, bd=8, tiles=(1, 1), wpp=0, tools=TOOLS, content="synth", frames=2):
    return dict(w=w, h=h, qp=qp, n=n, bd=bd, tiles=tiles, wpp=wpp, tools=tools, content=content, frames=frames)


CASES = {
    "c128_q32_n1": case(128, 128, 32, 1, content="unlike", frames=3),          # flat, texture, noise: pictures that want different QPs
    "c192x136_q27_n2": case(192, 136, 27, 2),                                  # five candidates, partial CTU row
    "e64_q51_n1": case(64, 64, 51, 1, frames=1),                               # +1 is coded at QP 51 with the lambda of 52
    "e64_q0_n1": case(64, 64, 0, 1, frames=1),                                 # -1 is coded at QP 0 with the lambda of -1
    "w192x128_q32_n1": case(192, 128, 32, 1, wpp=1),
    "t512x128_q32_n1": case(512, 128, 32, 1, tiles=(2, 2), frames=1),
    "c128_q30_n1_b10": case(128, 128, 30, 1, bd=10),
    "k128_q27_n1": case(128, 128, 27, 1, tools=TOOLS & ~(ref_tools.TOOL_RDOQ | ref_tools.TOOL_SIGN_HIDE)),
}


def offset_of(idx):
    """TEncSlice.cpp:294"""
    return ((idx + 1) >> 1) * (-1 if idx & 1 else 1)


def coded_qp(qp, idx, bd):
    """TEncSlice.cpp:523"""
    return max(-6 * (bd - 8), min(51, qp + offset_of(idx)))


def pick(bits, dist, qp):
    """TEncSlice.cpp:604-653 and TComRdCost.cpp:62-107 (DF_SSE_FRAME) on one picture's sums in candidate order: Python floats are IEEE doubles, every operation rounds once."""
    frame_lambda = 0.68 * 2.0 ** ((qp - 12) / 3.0)
    best, best_idx = 1.7e+308, 0
    for i, (b, d) in enumerate(zip(bits, dist)):
        cost = float(int(d)) + float(int(b)) * frame_lambda
        if cost < best:
            best, best_idx = cost, i
    return best_idx


def ref_args(c, sao=1):
    a = ["--DeltaQpRD=%d" % c["n"], "--SAO=%d" % sao, "--WaveFrontSynchro=%d" % c["wpp"]] + ref_tools.tool_args(c["tools"])
    if c["tiles"] != (1, 1):
        a += ref_tools.tile_args(c["tiles"])
    return a


def frames_of(c, seed):
    w, h, n = c["w"], c["h"], c["frames"]
    yuv = ref_tools.synth_yuv(w, h, n, seed)
    if c["content"] == "unlike":      # picture 0 flat, 1 the synthetic texture, 2 noise
        rng = np.random.default_rng(seed)
        yuv[0] = 90
        yuv[0, :w * h] += (np.arange(w * h) // w // 32).astype(np.uint8)
        yuv[2] = rng.integers(0, 256, yuv.shape[1])
    if c["bd"] > 8:
        yuv = (yuv.astype(np.uint16) << (c["bd"] - 8)) | np.random.default_rng(seed).integers(0, 1 << (c["bd"] - 8), yuv.shape).astype(np.uint16)
    return yuv, ref_tools.make_labels(w, h, n, "rand", seed=seed)


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


def main():
    if not os.path.exists(ref_tools.REF_ENC):
        sys.exit("oracle/_ref/TAppEncoder_ref is missing: run build() first")
    only = sys.argv[1:]
    winners, unlike_qps = set(), False
    for name, c in CASES.items():
        if only and name not in only:
            continue
        seed = 900 + sorted(CASES).index(name)
        w, h, bd, qp, n = c["w"], c["h"], c["bd"], c["qp"], c["n"]
        yuv, labels = frames_of(c, seed)
        nf, nctu, passes = labels.shape[0], labels.shape[1], 2 * n + 2
        dump, stdout, stream, recon = ref_tools.run_reference(yuv, w, h, qp, labels, extra_args=ref_args(c), bit_depth=bd)
        assert dump.shape[0] == nf * passes * nctu, (name, dump.shape)
        dump = dump.reshape(nf, passes, nctu)
        assert (dump["frame"] == np.arange(nf)[:, None, None]).all()
        order = np.argsort(dump["addr"], axis=2, kind="stable")      # tiles: a pass walks the CTUs in tile scan
        dump = np.take_along_axis(dump, order, axis=2)
        assert (dump["addr"] == np.arange(nctu)[None, None, :]).all()
        trials, final = dump[:, :passes - 1], dump[:, passes - 1]
        bits = trials["rec"]["bits"].astype(np.uint64).sum(axis=2)
        dist = trials["rec"]["dist"].astype(np.uint64).sum(axis=2)
        chosen = np.array([pick(bits[f], dist[f], qp) for f in range(nf)], np.int32)
        qps = np.array([coded_qp(qp, int(i), bd) for i in chosen], np.int32)
        assert slice_qps(stream) == qps.tolist(), (name, slice_qps(stream), qps.tolist())
        for f in range(nf):      # the search is deterministic: the final compress is the winning trial again
            win = trials[f, chosen[f]]
            for k in ("rec", "rec_y", "rec_cb", "rec_cr"):
                assert win[k].tobytes() == final[f][k].tobytes(), (name, f, k)
        deblocked = ref_tools.run_reference(yuv, w, h, qp, labels, extra_args=ref_args(c, sao=0), bit_depth=bd)[3]
        assert len(deblocked) == len(recon)
        winners.update(int(i) for i in chosen)
        unlike_qps = unlike_qps or len(set(qps.tolist())) > 1
        out = os.path.join(ROOT, "tests", "golden", "dqr_%s.npz" % name)
        np.savez_compressed(out, width=w, height=h, qp=qp, delta_qp_rd=n, bit_depth=bd, seed=seed, tiles=np.array(c["tiles"], np.int32), wavefront=c["wpp"], tools=c["tools"],
                            yuv=yuv, labels=labels, cand_bits=trials["rec"]["bits"], cand_dist=trials["rec"]["dist"], chosen_idx=chosen, chosen_qp=qps,
                            records=final["rec"], rec_y=final["rec_y"], rec_cb=final["rec_cb"], rec_cr=final["rec_cr"],
                            bitstream=np.frombuffer(stream, np.uint8), recon_file=np.frombuffer(recon, np.uint8), deblocked_file=np.frombuffer(deblocked, np.uint8),
                            keys=np.array(ref_args(c), dtype=str),
                            stdout=np.array([l for l in stdout.splitlines() if l.startswith("POC") or "SUMMARY" in l or "Total Frames" in l or l.startswith("\t ")]))
        print("%s: seed %d, chosen %s -> QP %s, stream %d bytes, file %d bytes" % (name, seed, chosen.tolist(), qps.tolist(), len(stream), os.path.getsize(out)))
    if not only:
        assert len(winners) >= 2 and winners - {0}, "the set must have at least two different winners, one of them not candidate 0: %s" % sorted(winners)
        assert unlike_qps, "no fixture whose pictures end at different QPs"


if __name__ == "__main__":
    main()
