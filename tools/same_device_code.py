"""Is the compiled device code of the decision kernel's builds, and of the decoder's kernels, the same in two source trees?  For a change that must not change code (retiring preprocessor
switches, host-side edits): every build below is compiled device-only for gfx950 from both trees, with build_ext's flags and one -cuid on both sides (hipcc
derives the CUID from the source path otherwise, and it names a symbol), and the two code objects are compared byte for byte.
usage: tools/same_device_code.py BASE_TREE [NEW_TREE]      (BASE_TREE: e.g. `git worktree add DIR HEAD~1`; NEW_TREE: this tree)
One line per build: name, size, sha256 of NEW_TREE's code object, same / DIFFERENT.  Exit status 1 on any difference.  Takes minutes (~85 s per compile)."""
import hashlib, os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hevcdl_amd

RD = ["rd_kernel.hip", "rd_kernel_bd10.hip", "rd_kernel_wide.hip", "rd_kernel_tools.hip"]
BUILDS = ([(s, ()) for s in RD] + [(s, ("HEVCDL_STAGE_TRACE",)) for s in RD] + [(s, ("HEVCDL_LEAF_TEST",)) for s in hevcdl_amd.LEAF_SOURCES] +
          # the instrument builds of tools/phase_profile.py, tools/timeline.py and tools/micro_rd.py
          [("rd_kernel.hip", d) for d in (("HEVCDL_KERNEL_PROF",), ("HEVCDL_KERNEL_PROF", "HEVCDL_PROF_N=64"), ("HEVCDL_KERNEL_PROF", "HEVCDL_PROF_GLUE"),
                                          ("HEVCDL_KERNEL_PROF", "HEVCDL_PROF_N=64", "HEVCDL_PROF_GLUE"), ("HEVCDL_KERNEL_PROF", "HEVCDL_PROF_MASTER"),
                                          ("HEVCDL_KERNEL_DEBUG", "HEVCDL_TIMELINE"), ("HEVCDL_MICRO",), ("HEVCDL_MICRO", "HEVCDL_MICRO_T"),
                                          ("HEVCDL_MICRO", "HEVCDL_MICRO_SMALL", "HEVCDL_NW=12"))] +
          [("hevcdl_api.hip", ()),        # the narrow and clamp kernels beside the host code
           ("recon_kernel.hip", ()), ("slice_decode_kernel.hip", ())])      # the decoder's kernels, each with its host entry points behind it


def compile_one(job):
    tree, src, defines, out = job
    pkg = os.path.join(tree, os.path.basename(hevcdl_amd.PKG_DIR))
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + hevcdl_amd.compile_flags(defines, ("-cuid=same_device_code",), root=tree)
    r = subprocess.run(cmd + ["--cuda-device-only", "-c", os.path.join(pkg, "csrc", src), "-o", out], capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write("%s %s in %s:\n%s\n" % (src, " ".join(defines), tree, r.stderr))
    return r.returncode == 0


def main(base, new=ROOT):
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(tree, src, defines, os.path.join(tmp, "%s%d.o" % (side, i))) for i, (src, defines) in enumerate(BUILDS) for side, tree in (("base", base), ("new", new))]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            ok = list(pool.map(compile_one, jobs))
        different = 0
        for i, (src, defines) in enumerate(BUILDS):
            name = " ".join((src,) + tuple("-D" + d for d in defines))
            if not (ok[2 * i] and ok[2 * i + 1]):
                print("%-75s %8s  %-64s  DIFFERENT (did not compile)" % (name, "-", "-"))
                different += 1
                continue
            a, b = (open(os.path.join(tmp, "%s%d.o" % (side, i)), "rb").read() for side in ("base", "new"))
            print("%-75s %8d  %s  %s" % (name, len(b), hashlib.sha256(b).hexdigest(), "same" if a == b else "DIFFERENT"))
            different += a != b
    return 1 if different else 0


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    sys.exit(main(*[os.path.abspath(p) for p in sys.argv[1:]]))
