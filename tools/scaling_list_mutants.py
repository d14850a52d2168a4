#!/usr/bin/env python3
"""tools/scaling_list_mutants.py -- TEST INFRASTRUCTURE.  Five one-line mutants of the CPU source of the scaling-list path, each built into tests/scaling_list_harness.cpp
(host compiler, no sanitizer) from a copy of csrc/ with that one line changed, and run over the filters-off streams of the sclist_* fixtures: a mutant is CAUGHT when the
harness fails -- the host reconstruction of the parser's records and factors no longer gives the reference decoder's pictures.

tests/test_scaling_lists.py runs run_mutants() and asserts that every mutant is caught and that the unchanged source passes; run as a script this writes the counts to
profiles/scaling_list_mutants.txt."""
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "hevc-deep-learning-pipeline_amd", "csrc")

# name: (file, the line's text, its replacement, what it breaks)
MUTANTS = {
    "dc_not_applied": ("hevcdl_parse.cpp", "      b[0] = (uint8_t)s.dc[size_id][m];\n", "", "the DC entry of 16x16 and 32x32 not applied"),
    "replication_transposed": ("hevcdl_parse.cpp", "b[(y8 * rep + j) * n + x8 * rep + k] = s.list[size_id][m][i];", "b[(x8 * rep + j) * n + y8 * rep + k] = s.list[size_id][m][i];",
                               "row and column swapped in the replication"),
    "ref_matrix_off_by_one": ("hevcdl_parse.cpp", "const int ref = m - (int)delta * step;", "const int ref = m - ((int)delta - 1) * step;", "refMatrixId off by one"),
    "tskip_left_flat": ("recon_core.h", "* rc_coef_scale(p, m, i, scale) +", "* ((tskip && n == 4) ? scale : rc_coef_scale(p, m, i, scale)) +", "transform-skipped blocks left flat"),
    "chroma_planes_swapped": ("recon_core.h", "1360 + (comp - 1) * 336", "1360 + (2 - comp) * 336", "the chroma planes swapped"),
}


def write_dumps(d, runs=("nolf",), mode_of=lambda name, run: 0):
    """One dump per fixture stream (tests/scaling_list_harness.cpp), the filters-off ones with the reference decoder's pictures.  -> [path]"""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLD, "sclist_*.npz"))):
        f = np.load(p)
        name = os.path.basename(p)[7:-4]
        for run in runs:
            s = f["stream_" + run].tobytes()
            pic = f["picture_nolf"].tobytes() if run == "nolf" else b""
            path = os.path.join(d, "%s_%s.bin" % (name, run))
            with open(path, "wb") as fh:
                fh.write(np.array([len(s), len(pic), mode_of(name, run)], np.int64).tobytes() + s + pic)
            out.append(path)
    return out


def build_harness(csrc, exe, flags=("-O1",)):
    cmd = ["g++", "-std=c++17", "-g", "-fno-omit-frame-pointer"] + list(flags) + ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "scaling_list_harness.cpp"),
           os.path.join(csrc, "hevcdl_parse.cpp"), os.path.join(csrc, "hevcdl_bitstream.cpp"), "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True)


def run_mutants():
    """-> {name: (dumps that failed, dumps, what the mutant breaks)}; "unchanged" is the source as it is."""
    res = {}
    with tempfile.TemporaryDirectory(prefix="sclist_mut_") as d:
        dumps = write_dumps(d)
        for name, m in [("unchanged", None)] + list(MUTANTS.items()):
            src = os.path.join(d, "csrc_" + name)
            shutil.copytree(CSRC, src, ignore=shutil.ignore_patterns("*.hip"))
            if m:
                path = os.path.join(src, m[0])
                text = open(path).read()
                assert text.count(m[1]) == 1, "the line of mutant %s occurs %d times in %s" % (name, text.count(m[1]), m[0])
                open(path, "w").write(text.replace(m[1], m[2]))
            exe = os.path.join(d, "h_" + name)
            r = build_harness(src, exe)
            assert r.returncode == 0, r.stderr[-2000:]
            failed = sum(subprocess.run([exe, p], capture_output=True, text=True).returncode != 0 for p in dumps)
            res[name] = (failed, len(dumps), m[3] if m else "the source as it is")
    return res


def main():
    res = run_mutants()
    with open(os.path.join(ROOT, "profiles", "scaling_list_mutants.txt"), "w") as f:
        f.write("# tools/scaling_list_mutants.py: one-line mutants of the CPU source built into tests/scaling_list_harness.cpp and run over the filters-off streams of\n"
                "# tests/golden/sclist_*.npz.  A dump fails when the host reconstruction differs from the reference decoder's pictures.\n")
        for name, (failed, n, what) in res.items():
            line = "%-24s %3d of %d dumps fail   (%s)" % (name, failed, n, what)
            print(line)
            f.write(line + "\n")
    return 0 if res["unchanged"][0] == 0 and all(v[0] > 0 for k, v in res.items() if k != "unchanged") else 1


if __name__ == "__main__":
    sys.exit(main())
