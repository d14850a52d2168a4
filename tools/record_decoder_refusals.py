"""Records what the decoder's host code of another tree answers -- statuses and sentences of damaged and refused streams, of every `accept` through every form of
hevcdl_parse_stream, of the order of two refusals, and of bad calls of the reconstruction's entry points -- as tests/golden/decoder_refusals.json: one sha256 and one line
count per group of tests/decoder_refusal_cases.py.  For a change that must not move any of it: record the parent commit, commit the file, and tests/test_decoder_refusals.py
holds the new tree to it.
usage: tools/record_decoder_refusals.py TREE      (TREE: a built tree, e.g. `git worktree add DIR HEAD~1` and its build; the cases and fixtures are this tree's)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(tree):
    sys.path.insert(0, tree)
    import hevcdl_amd                      # TREE's package and library; imported first, so that nothing below loads this tree's
    assert os.path.samefile(hevcdl_amd.ROOT, tree), hevcdl_amd.ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import decoder_refusal_cases as cases
    out = {"recorded_with": "tools/record_decoder_refusals.py", "device_side": {"no such device": cases.digest(cases.no_such_device(hevcdl_amd))}}
    out["groups"] = {name: cases.digest(lines) for name, lines in cases.groups(hevcdl_amd).items()}
    path = os.path.join(ROOT, "tests", "golden", "decoder_refusals.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d groups, %d lines" % (path, len(out["groups"]), sum(g["count"] for g in out["groups"].values())))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
