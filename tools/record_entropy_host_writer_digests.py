"""Record what hevcdl_write_access_unit says for the pictures of tests/entropy_cases.py -- fuzz_corpus(), directed_pictures() and SAO_CASES -- into
tests/golden/entropy_host_writer_digests.json: per picture the SHA-256 of the access units (entropy_cases.host_writer_stream) and the SHA-256 of what went in (stream
configuration, records, SAO parameters), so that a corpus that drifted is told from a coder that changed.  The file is the authority tests/test_entropy.py and
tests/test_entropy_gpu.py hold the entropy coder to, so it is recorded in a checkout of a commit whose coder is trusted, BEFORE a change of the coder, with that checkout's
own library (the header names its HEAD):
    python tools/record_entropy_host_writer_digests.py [OUT.json]
Needs no GPU; the SAO cases build the C oracle.  Takes about a minute."""
import hashlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import entropy_cases as ec


def main(out):
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    entries = {}
    for name, cfg, recs, sao in ec.recorded_pictures():
        stream = ec.host_writer_stream(cfg, recs, sao)
        entries[name] = {"input": ec.input_digest(cfg, recs, sao), "stream": hashlib.sha256(stream).hexdigest(), "bytes": len(stream)}
    with open(out, "w") as f:
        json.dump({"recorded_at": commit, "writer": "hevcdl_write_access_unit", "pictures": entries}, f, indent=1)
        f.write("\n")
    print("%d pictures at %s -> %s" % (len(entries), commit[:7], out))


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "entropy_host_writer_digests.json"))
