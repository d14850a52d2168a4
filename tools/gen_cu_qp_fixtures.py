#!/usr/bin/env python3
"""tools/gen_cu_qp_fixtures.py -- TEST INFRASTRUCTURE.  Writes tests/golden/cuqp_*.npz: reference-encoder streams whose QP is not constant over the picture
(cu_qp_delta_enabled_flag, PPS chroma QP offsets), each with the reference DECODER's pictures.  Needs oracle/_ref/TAppEncoder_ref and TAppDecoder_ref (build()).

Every case is run three times from the same input -- filters off (parse + reconstruction), deblocking alone, deblocking + SAO -- with --SEIDecodedPictureHash=1; each
run's stream is decoded by the reference decoder, every MD5 must read (OK), and the decoder's pictures are what the fixture stores.  A fixture holds data only: seed and
parameters, labels, the three streams (keys stream_*: NOT bitstream*, the families of tests/test_decode.py are the constant-QP ones), the three picture sets and the slice
QPs of the encoder's log.

Through the new parser (hevcdl_parse_stream_qp) it prints a tally per fixture -- what of the QP syntax and of 8.6.1 the stream reaches -- and writes the table to
profiles/cu_qp_fixtures.txt.  tests/test_cu_qp.py asserts over the whole set what the table shows."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hevcdl_amd      # noqa: E402
import ref_tools       # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
RUNS = {"nolf": ["--LoopFilterDisable=1", "--SAO=0"], "dbk": ["--SAO=0"], "full": []}
AQ = ["--AdaptiveQP=1"]
RC = ["--RateControl=1", "--TargetBitrate=2000000"]

# name: size, pictures, QP, bit depth, content ("synth": ref_tools.synth_yuv, "activity": per-CTU noise), the keys
CASES = {
    "rc_pic": dict(w=192, h=128, n=3, qp=22, bd=8, content="synth", keys=RC + ["--LCULevelRateControl=0"]),
    "rc_lcu": dict(w=192, h=128, n=3, qp=22, bd=8, content="synth", keys=RC + ["--LCULevelRateControl=1"]),
    "aq_d0": dict(w=192, h=128, n=2, qp=27, bd=8, content="synth", keys=AQ + ["--MaxQPAdaptationRange=6", "--MaxCuDQPDepth=0"]),
    "aq_d2": dict(w=192, h=128, n=2, qp=27, bd=8, content="synth", keys=AQ + ["--MaxQPAdaptationRange=6", "--MaxCuDQPDepth=2"]),
    "aq_d3_q22": dict(w=136, h=72, n=2, qp=22, bd=8, content="synth", keys=AQ + ["--MaxQPAdaptationRange=6", "--MaxCuDQPDepth=3"]),
    "aq_d3_q45": dict(w=136, h=72, n=2, qp=45, bd=8, content="synth", keys=AQ + ["--MaxQPAdaptationRange=6", "--MaxCuDQPDepth=3"]),
    "maxdqp": dict(w=128, h=128, n=1, qp=30, bd=8, content="synth", keys=["--MaxDeltaQP=2", "--MaxCuDQPDepth=1"]),
    "chroma_off": dict(w=192, h=128, n=2, qp=32, bd=8, content="synth", keys=["--CbQpOffset=3", "--CrQpOffset=-4"]),
    "wpp": dict(w=192, h=128, n=2, qp=27, bd=8, content="synth", keys=AQ + ["--MaxCuDQPDepth=1", "--WaveFrontSynchro=1"]),
    "tiles": dict(w=512, h=128, n=1, qp=27, bd=8, content="synth", keys=AQ + ["--MaxCuDQPDepth=1"] + ref_tools.tile_args((2, 2))),
    "slices": dict(w=192, h=192, n=1, qp=27, bd=8, content="synth", keys=AQ + ["--MaxCuDQPDepth=1", "--SliceMode=1", "--SliceArgument=3"]),
    "b10_off": dict(w=192, h=128, n=2, qp=27, bd=10, content="synth", keys=AQ + ["--MaxCuDQPDepth=2", "--CbQpOffset=-2", "--CrQpOffset=5"]),
    "act_d0_r6": dict(w=256, h=128, n=2, qp=30, bd=8, content="activity", keys=AQ + ["--MaxCuDQPDepth=0", "--MaxQPAdaptationRange=6"]),
    "act_d0_r12": dict(w=256, h=128, n=2, qp=30, bd=8, content="activity", keys=AQ + ["--MaxCuDQPDepth=0", "--MaxQPAdaptationRange=12"]),
    "act_d2_q50": dict(w=256, h=128, n=2, qp=50, bd=8, content="activity", keys=AQ + ["--MaxQPAdaptationRange=12", "--MaxCuDQPDepth=2"]),
    "act_b10_q2": dict(w=256, h=128, n=1, qp=2, bd=10, content="activity", keys=AQ + ["--MaxQPAdaptationRange=12", "--MaxCuDQPDepth=0"]),
}


def activity_yuv(w, h, n, seed):
    """Every 64x64 luma block Gaussian noise around 128 with its own sigma out of {0.5, 3, 12, 50, 110}, chroma N(128, 6): AdaptiveQP needs activity that differs between CTUs."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        Y = np.zeros((h, w))
        for y in range(0, h, 64):
            for x in range(0, w, 64):
                s = (0.5, 3, 12, 50, 110)[int(rng.integers(0, 5))]
                Y[y:y + 64, x:x + 64] = rng.normal(128, s, Y[y:y + 64, x:x + 64].shape)
        C = rng.normal(128, 6, (2, h // 2, w // 2))
        out.append(np.concatenate([np.clip(np.rint(Y), 0, 255).ravel(), np.clip(np.rint(C), 0, 255).ravel()]).astype(np.uint8))
    return np.stack(out)


def frames_of(c, seed):
    yuv = ref_tools.synth_yuv(c["w"], c["h"], c["n"], seed) if c["content"] == "synth" else activity_yuv(c["w"], c["h"], c["n"], seed)
    if c["bd"] > 8:
        yuv = (yuv.astype(np.uint16) << (c["bd"] - 8)) | np.random.default_rng(seed).integers(0, 1 << (c["bd"] - 8), yuv.shape).astype(np.uint16)
    return yuv, ref_tools.make_labels(c["w"], c["h"], c["n"], "rand", seed=seed)


def decode(stream):
    with tempfile.TemporaryDirectory(prefix="hmdec_") as d:
        open(os.path.join(d, "s.bin"), "wb").write(stream)
        p = subprocess.run([ref_tools.REF_DEC, "-b", "s.bin", "-o", "d.yuv", "-d", "0"], cwd=d, capture_output=True, text=True)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return open(os.path.join(d, "d.yuv"), "rb").read(), p.stdout


def seed_of(name):
    return 900 + sorted(CASES).index(name)


def main():
    if not (os.path.exists(ref_tools.REF_ENC) and os.path.exists(ref_tools.REF_DEC)):
        sys.exit("oracle/_ref/TAppEncoder_ref / TAppDecoder_ref are missing: run build() first")
    only = sys.argv[1:]
    lines = ["%-12s %-5s " % ("fixture", "run") + " ".join(hevcdl_amd.QP_TALLY_FIELDS) + " min_qpy max_qpy"]
    for name, c in CASES.items():
        if only and name not in only:
            continue
        seed = seed_of(name)
        yuv, labels = frames_of(c, seed)
        w, h, bd, n = c["w"], c["h"], c["bd"], c["n"]
        keep = dict(width=w, height=h, qp=c["qp"], bit_depth=bd, seed=seed, n_frames=n, content=c["content"], keys=" ".join(c["keys"]), labels=labels)
        for run, extra in RUNS.items():
            _, log, stream, _ = ref_tools.run_reference(yuv, w, h, c["qp"], labels, extra_args=c["keys"] + extra, bit_depth=bd)
            dec, dec_log = decode(stream)
            assert dec_log.count("(OK)") == n and "ERROR" not in dec_log, (name, run, dec_log[-1500:])
            pic = np.frombuffer(dec, np.uint8 if bd == 8 else "<u2").reshape(n, w * h * 3 // 2)
            qps = [int(q) for q in re.findall(r"POC\s+\d+\s+TId:\s*\d+\s*\(\s*I-SLICE,\s*nQP\s+\d+\s+QP\s+(-?\d+)\s*\)", log)]
            assert len(qps) == n, (name, run, log[-1500:])
            keep["stream_" + run] = np.frombuffer(stream, np.uint8)
            keep["picture_" + run] = pic
            keep["slice_qps_" + run] = np.array(qps, np.int32)
            ps = hevcdl_amd.parse_stream(stream, cu_qp=True)
            t = hevcdl_amd.parse_qp_tally()
            assert ps.qps == qps, (name, run, ps.qps, qps)
            lines.append("%-12s %-5s " % (name, run) + " ".join(str(t[k]) for k in hevcdl_amd.QP_TALLY_FIELDS) + " %d %d" % (ps.qp_map.min(), ps.qp_map.max()))
            print(lines[-1], flush=True)
        out = os.path.join(GOLD, "cuqp_%s.npz" % name)
        np.savez_compressed(out, **keep)
        assert os.path.getsize(out) < 1 << 20, "a committed file stays below 1 MiB"
    if not only:
        with open(os.path.join(ROOT, "profiles", "cu_qp_fixtures.txt"), "w") as f:
            f.write("# tools/gen_cu_qp_fixtures.py: what hevcdl_parse_stream_qp met in every stream of tests/golden/cuqp_*.npz (hevcdl_qp_tally; min / max of the QP map,\n"
                    "# 0 included where a picture has partitions outside it)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
