#!/usr/bin/env python3
"""tools/gen_scaling_list_fixtures.py -- TEST INFRASTRUCTURE.  Writes tests/golden/sclist_*.npz: reference-encoder streams whose SPS enables scaling lists (ScalingList 1: the
default lists, no list data; ScalingList 2: a ScalingListFile this tool writes from a seed), each with the reference DECODER's pictures.  Needs oracle/_ref/TAppEncoder_ref
and TAppDecoder_ref (build()).

Every case is run three times from the same input -- filters off (parse + reconstruction), deblocking alone, the default cfg (deblocking + SAO) -- with
--SEIDecodedPictureHash=1; each run's stream is decoded by the reference decoder, every MD5 must read (OK), and the decoder's pictures are what the fixture stores.  A
fixture holds data only: seed and parameters, labels, the three streams (keys stream_*: NOT bitstream*), the three picture sets, the slice QPs of the encoder's log and, for
ScalingList 2, the lists and DC values that were written to the list file (raster order, as the file holds them): lists4 [6, 16], lists8 / lists16 [6, 64], lists32 [2, 64]
(matrixId 0 and 3), dc16 [6], dc32 [2].  tests/test_scaling_lists.py derives the expected factor block from those arrays.

Through the parser (hevcdl_parse_stream_sl) it prints the coverage of tools/scaling_list_cover.py per fixture and run and writes the table to
profiles/scaling_list_fixtures.txt."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hevcdl_amd                 # noqa: E402
import ref_tools                  # noqa: E402
import scaling_list_cover as slc  # noqa: E402
from gen_cu_qp_fixtures import activity_yuv      # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
RUNS = {"nolf": ["--LoopFilterDisable=1", "--SAO=0"], "dbk": ["--SAO=0"], "full": []}
FILE = ["--ScalingList=2", "--ScalingListFile=scaling_list.txt"]
# Table 7-6 in raster order, as a list file holds it
INTRA8 = [16, 16, 16, 16, 17, 18, 21, 24, 16, 16, 16, 16, 17, 19, 22, 25, 16, 16, 17, 18, 20, 22, 25, 29, 16, 16, 18, 21, 24, 27, 31, 36,
          17, 17, 20, 24, 30, 35, 41, 47, 18, 19, 22, 27, 35, 44, 54, 65, 21, 22, 25, 31, 41, 54, 70, 88, 24, 25, 29, 36, 47, 65, 88, 115]
INTER8 = [16, 16, 16, 16, 17, 18, 20, 24, 16, 16, 16, 17, 18, 20, 24, 25, 16, 16, 17, 18, 20, 24, 25, 28, 16, 17, 18, 20, 24, 25, 28, 33,
          17, 18, 20, 24, 25, 28, 33, 41, 18, 20, 24, 25, 28, 33, 41, 54, 20, 24, 25, 28, 33, 41, 54, 71, 24, 25, 28, 33, 41, 54, 71, 91]
MATRIX = ["LUMA", "CHROMAU", "CHROMAV"]

# name: size, pictures, QP, bit depth, content, labels, lists ("default": ScalingList 1; otherwise the kind of list file), further keys
CASES = {
    "default": dict(w=192, h=128, n=2, qp=22, bd=8, content="synth", lists="default", keys=["--ScalingList=1"]),
    "file_rand": dict(w=192, h=128, n=2, qp=17, bd=8, content="synth", lists="rand", keys=FILE),
    "file_pred": dict(w=192, h=128, n=1, qp=22, bd=8, content="synth", lists="pred", keys=FILE),
    "file_steep_b10": dict(w=192, h=128, n=1, qp=2, bd=10, content="activity", lists="steep", keys=FILE),
    "tskip": dict(w=128, h=128, n=1, qp=27, bd=8, content="sharp", lists="rand", keys=FILE + ["--TransformSkipFast=0"]),
    "cuqp": dict(w=192, h=128, n=2, qp=27, bd=8, content="synth", lists="rand", keys=FILE + ["--AdaptiveQP=1", "--MaxCuDQPDepth=2", "--CbQpOffset=3", "--CrQpOffset=-4"]),
    "tiles": dict(w=512, h=128, n=1, qp=27, bd=8, content="synth", lists="rand", keys=FILE + ref_tools.tile_args((2, 2))),
    "wpp": dict(w=192, h=128, n=1, qp=27, bd=8, content="synth", lists="rand", keys=FILE + ["--WaveFrontSynchro=1"]),
    "edge_q45": dict(w=136, h=72, n=2, qp=45, bd=8, content="synth", lists="rand", keys=FILE),
    "one_ctu": dict(w=64, h=64, n=1, qp=22, bd=8, content="synth", lists="rand", labels=0, keys=FILE),
}


def seed_of(name):
    return 1100 + sorted(CASES).index(name)


def sharp_yuv(w, h, n, seed):
    """Two-level rectangles, one-sample lines and single samples on a flat ground: what transform skip is for."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        planes = []
        for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
            P = np.full((ph, pw), int(rng.integers(60, 200)), np.int32)
            for _ in range(pw * ph // 40):
                x, y = int(rng.integers(0, pw)), int(rng.integers(0, ph))
                kind = int(rng.integers(0, 3))
                v = int(rng.integers(0, 256))
                if kind == 0:
                    P[y:y + int(rng.integers(1, 6)), x:x + int(rng.integers(1, 6))] = v
                elif kind == 1:
                    P[y, x:x + int(rng.integers(2, 12))] = v
                else:
                    P[y, x] = v
            planes.append(P.ravel())
        out.append(np.concatenate(planes).astype(np.uint8))
    return np.stack(out)


def make_lists(kind, seed):
    """-> dict of the arrays a fixture stores; every list in raster order."""
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.integers(1, 256, s).astype(np.int32)
    L = dict(lists4=r(6, 16), lists8=r(6, 64), lists16=r(6, 64), lists32=r(2, 64), dc16=r(6), dc32=r(2))
    if kind == "steep":      # 1 and 255 side by side, every DC the other of the two
        for k, cnt, n in (("lists4", 6, 4), ("lists8", 6, 8), ("lists16", 6, 8), ("lists32", 2, 8)):
            for m in range(cnt):
                y, x = np.mgrid[0:n, 0:n]
                L[k][m] = np.where((x + y + m) & 1, 1, 255).ravel()
        L["dc16"] = np.where(L["lists16"][:, 0] == 1, 255, 1).astype(np.int32)
        L["dc32"] = np.where(L["lists32"][:, 0] == 1, 255, 1).astype(np.int32)
    if kind == "pred":       # lists equal to an earlier one (scaling_list_pred_matrix_id_delta > 0) and to the default (delta 0)
        L["lists4"][1] = L["lists4"][0]; L["lists4"][2] = 16; L["lists4"][4] = L["lists4"][3]
        L["lists8"][2] = L["lists8"][0]; L["lists8"][3] = INTER8; L["lists8"][5] = L["lists8"][4]
        L["lists16"][0] = INTRA8; L["dc16"][0] = 16; L["lists16"][2] = L["lists16"][1]; L["dc16"][2] = L["dc16"][1]
        L["lists32"][1] = L["lists32"][0]; L["dc32"][1] = L["dc32"][0]
    for k, d in (("lists16", "dc16"), ("lists32", "dc32")):      # every DC differs from its list's first entry -- except where a list is to equal the default
        for m in range(len(L[d])):
            if kind != "pred" and L[d][m] == L[k][m][0]:
                L[d][m] = L[d][m] % 255 + 1
    return L


def write_list_file(path, L):
    """The format TComScalingList::xParseScalingList reads: a name line per matrix, the values in raster order, a DC line for 16x16 and 32x32."""
    with open(path, "w") as f:
        for size, key, n in ((4, "lists4", 4), (8, "lists8", 8), (16, "lists16", 8), (32, "lists32", 8)):
            for m in range(6):
                if size == 32 and m % 3:
                    continue
                name = "%s%dX%d_%s" % ("INTRA" if m < 3 else "INTER", size, size, MATRIX[m % 3])
                vals = L[key][m // 3 if size == 32 else m]
                f.write(name + " =\n")
                for y in range(n):
                    f.write("  " + "".join("%3d," % v for v in vals[y * n:(y + 1) * n]) + "\n")
                if size >= 16:
                    f.write(name + "_DC =\n  %3d\n" % (L["dc32"][m // 3] if size == 32 else L["dc16"][m]))
                f.write("\n")


def frames_of(c, seed):
    w, h, n = c["w"], c["h"], c["n"]
    yuv = {"synth": ref_tools.synth_yuv, "activity": activity_yuv, "sharp": sharp_yuv}[c["content"]](w, h, n, seed)
    if c["bd"] > 8:
        yuv = (yuv.astype(np.uint16) << (c["bd"] - 8)) | np.random.default_rng(seed).integers(0, 1 << (c["bd"] - 8), yuv.shape).astype(np.uint16)
    return yuv, ref_tools.make_labels(w, h, n, c.get("labels", "rand"), seed=seed)


def decode(stream):
    with tempfile.TemporaryDirectory(prefix="hmdec_") as d:
        open(os.path.join(d, "s.bin"), "wb").write(stream)
        p = subprocess.run([ref_tools.REF_DEC, "-b", "s.bin", "-o", "d.yuv", "-d", "0"], cwd=d, capture_output=True, text=True)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return open(os.path.join(d, "d.yuv"), "rb").read(), p.stdout


def main():
    if not (os.path.exists(ref_tools.REF_ENC) and os.path.exists(ref_tools.REF_DEC)):
        sys.exit("oracle/_ref/TAppEncoder_ref / TAppDecoder_ref are missing: run build() first")
    only = sys.argv[1:]
    lines = ["%-15s %-5s " % ("fixture", "run") + " ".join(slc.FIELDS)]
    for name, c in CASES.items():
        if only and name not in only:
            continue
        seed = seed_of(name)
        yuv, labels = frames_of(c, seed)
        w, h, bd, n = c["w"], c["h"], c["bd"], c["n"]
        keep = dict(width=w, height=h, qp=c["qp"], bit_depth=bd, seed=seed, n_frames=n, content=c["content"], keys=" ".join(c["keys"]), labels=labels)
        L = None if c["lists"] == "default" else make_lists(c["lists"], seed)
        if L:
            keep.update({k: v.astype(np.uint8) for k, v in L.items()})
        for run, extra in RUNS.items():
            with tempfile.TemporaryDirectory(prefix="hmref_") as d:
                if L:
                    write_list_file(os.path.join(d, "scaling_list.txt"), L)
                _, log, stream, _ = ref_tools.run_reference(yuv, w, h, c["qp"], labels, extra_args=c["keys"] + extra, bit_depth=bd, keep_dir=d)
            dec, dec_log = decode(stream)
            assert dec_log.count("(OK)") == n and "ERROR" not in dec_log, (name, run, dec_log[-1500:])
            pic = np.frombuffer(dec, np.uint8 if bd == 8 else "<u2").reshape(n, w * h * 3 // 2)
            qps = [int(q) for q in re.findall(r"POC\s+\d+\s+TId:\s*\d+\s*\(\s*I-SLICE,\s*nQP\s+\d+\s+QP\s+(-?\d+)\s*\)", log)]
            assert len(qps) == n, (name, run, log[-1500:])
            keep["stream_" + run] = np.frombuffer(stream, np.uint8)
            keep["picture_" + run] = pic
            keep["slice_qps_" + run] = np.array(qps, np.int32)
            ps = hevcdl_amd.parse_stream(stream, cu_qp=True, scaling_lists=True)
            assert ps.qps == qps and ps.scaling.enabled == 1 and ps.scaling.data_present == (0 if L is None else 1), (name, run, ps.qps, qps)
            cov = slc.coverage(ps)
            lines.append("%-15s %-5s " % (name, run) + " ".join(str(cov[k]) for k in slc.FIELDS))
            print(lines[-1], flush=True)
        out = os.path.join(GOLD, "sclist_%s.npz" % name)
        np.savez_compressed(out, **keep)
        assert os.path.getsize(out) < 1 << 20, "a committed file stays below 1 MiB"
    if not only:
        with open(os.path.join(ROOT, "profiles", "scaling_list_fixtures.txt"), "w") as f:
            f.write("# tools/gen_scaling_list_fixtures.py: what the streams of tests/golden/sclist_*.npz reach of the scaling-list dequantisation (tools/scaling_list_cover.py, from the\n"
                    "# parser's records, QP map and factor block).  nz_*: non-zero levels at a factor other than 16; dc_*: non-zero DC levels of 16x16 / 32x32 blocks whose DC factor\n"
                    "# differs from the list's first entry; ts_*: transform-skipped 4x4 blocks with such a level; clip: dequantised values at the 16-bit clip.\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
