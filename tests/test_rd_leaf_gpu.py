"""The leaf routines of the decision kernel (csrc/rd_kernel.hip) one by one against the oracle's leaf entries, in all four builds of the kernel.

lib/libhevcdl_hip_leaf.so (csrc/rd_leaf*.hip + rd_leaf_harness.h, -DHEVCDL_LEAF_TEST: hevcdl_leaf_tu_kernel / hevcdl_leaf_pred_kernel) runs forward transform -> RDOQ or the plain quantiser -> coefficient
bit count -> dequantiser -> inverse transform, and reference filter -> 35 predictions -> rough-mode SATD, on the corpus of oracle/leaf_cases.py, and writes every
intermediate out.  The library defines the product library's kernel names, so a child process per build (oracle/leaf_device.py) loads it, runs everything once
(twice, for the run-to-run test) and saves the outputs; the tests of a build share that one run and the oracle's outputs, computed once per corpus.  Every comparison
is exact: every word of every output, no tolerance, no case skipped.  A failure names the build, the leaf output, the parameters, the case and the first differing
position; `python oracle/leaf_device.py LIB SUFFIX --compare ...` reruns single calls ("Leaf tests of the decision kernel").
HEVCDL_LEAF_LIB names another leaf library to test (a build under investigation)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import leaf_cases
import leaf_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = ["", "_bd10", "_wide", "_tools"]
_oracle_cache = {}


def _oracle(suffix):
    """The corpus of a build and the oracle's outputs for it; builds of one bit depth and tool handling share them."""
    key = leaf_cases.BUILDS[suffix]
    if key not in _oracle_cache:
        import __graft_entry__ as g
        g.build_oracle()
        tu, r2, r3, pr = leaf_device.corpus(suffix)
        tu_all = tu + [c for c, _ in r2] + [c for c, _ in r3]
        _oracle_cache[key] = dict(tu=tu, r2=r2, r3=r3, pr=pr, tu_all=tu_all, tu_ref=[leaf_device.oracle_tu(c) for c in tu_all], pr_ref=[leaf_device.oracle_pred(c) for c in pr])
    return _oracle_cache[key]


@pytest.fixture(scope="module", params=BUILDS, ids=[b or "_default" for b in BUILDS])
def run(request, tmp_path_factory):
    """One child process per build: the whole corpus through the device leaves."""
    import hevcdl_amd
    suffix = request.param
    import time
    t0 = time.time()
    lib = os.environ.get("HEVCDL_LEAF_LIB") or hevcdl_amd.build_leaf_lib()                 # no-op when built by __graft_entry__.build()
    out = str(tmp_path_factory.mktemp("leaf") / ("out%s.npz" % suffix))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "leaf_device.py"), lib, suffix, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "build %r: the device run failed:\n%s%s" % (suffix, r.stdout[-2000:], r.stderr[-3000:])
    t1 = time.time()
    ora = _oracle(suffix)
    f = np.load(out)
    print("leaf run of build %r: child process %.1f s (corpus built at %.1f s, first run done at %.1f s, second at %.1f s), oracle %.1f s" % ((suffix, t1 - t0) + tuple(f["seconds"]) + (time.time() - t1,)))
    tu_dev = leaf_device.unpack({k: f["tu_" + k] for k in leaf_device.TU_KEYS}, ora["tu_ref"], leaf_device.TU_KEYS)
    pr_dev = leaf_device.unpack({k: f["pred_" + k] for k in leaf_device.PRED_KEYS}, ora["pr_ref"], leaf_device.PRED_KEYS)
    return dict(suffix=suffix, ora=ora, tu_dev=tu_dev, pr_dev=pr_dev, digests=(f["digest0"], f["digest1"]), refusals=tuple(int(v) for v in f["refusals"]))


def _check_tu(run, entry):
    ora, n = run["ora"], 0
    for i, c in enumerate(ora["tu"]):
        if c.entry != entry:
            continue
        n += len(c.blocks)
        msg = leaf_device.first_difference(run["suffix"], lambda b, c=c: leaf_cases.describe(c, b), run["tu_dev"][i], ora["tu_ref"][i], leaf_device.TU_KEYS)
        assert msg is None, msg
    return n


def test_tu_chain_from_residuals_equals_the_oracle(run):
    """Entry 0: forward transform (or the transform-skip scaling), quantiser, bit count, dequantiser, inverse transform on the residual corpus: worst-case blocks (all +-M,
    the sign pattern of every basis function), every QP, scan type, cbf context and context set -- coefficients, levels, abs_sum, the fractional bit counter, all
    context bytes, dequantised coefficients and reconstructed residual == hm_oracle_tu_leaf."""
    assert _check_tu(run, 0) > 15000


def test_tu_chain_from_coefficients_equals_the_oracle(run):
    """Entry 1: the quantiser onwards on coefficient blocks no residual reaches: every coefficient +32767 / -32768 (lLevelDouble's 24-bit multiply), single
    coefficients at the ends of each scan, blocks whose every rounded level is exactly 1 / 2 / 3 in whole blocks, alternate groups or one anti-diagonal of groups
    (RDOQ's batch rule), Laplacian magnitudes."""
    assert _check_tu(run, 1) > 8000


def test_dequantiser_and_inverse_transform_equal_the_oracle(run):
    """Entry 2: dequantiser and inverse transform on the level blocks of the reference's traces at every QP, and on +-32767 blocks (the 16-bit clips)."""
    assert _check_tu(run, 2) > 2000


def test_device_leaves_reproduce_the_reference_traces(run):
    """The reference's own TU events (tests/golden/stage_*.npz) through the device leaves, at the fixtures' QP: residual -> coefficients and levels -> dequantised ->
    residual equal what the reference printed.  8-bit builds (the fixtures are 8-bit runs); the 10-bit build has nothing to replay and passes the oracle comparisons."""
    ora = run["ora"]
    if leaf_cases.BUILDS[run["suffix"]][0] != 8:
        assert not ora["r2"] and not ora["r3"]
        return
    at = len(ora["tu"])
    for kind, lst in ((2, ora["r2"]), (3, ora["r3"])):
        assert sum(len(c.blocks) for c, _ in lst) > 3000
        for c, exp in lst:
            dev = run["tu_dev"][at]
            at += 1
            ref = {"coef": exp[:, 1]} if kind == 2 else {"deq": exp[:, 1], "resi": exp[:, 2]}
            msg = leaf_device.first_difference(run["suffix"], lambda b, c=c: "reference trace: " + leaf_cases.describe(c, b), dev, ref, ("coef", "deq", "resi"))
            assert msg is None, msg


def _check_pred(run, key, least):
    ora, n = run["ora"], 0
    for i, c in enumerate(ora["pr"]):
        if key in ora["pr_ref"][i]:
            n += len(c.lines)
            msg = leaf_device.first_difference(run["suffix"], lambda j, c=c: leaf_cases.describe_pred(c, j), run["pr_dev"][i], ora["pr_ref"][i], (key,))
            assert msg is None, msg
    assert n >= least, n


def test_filtered_reference_line_equals_the_oracle(run):
    """filter_refs on luma lines of 4..64: [1 2 1] filter, and strong smoothing at 32x32 on ramps that trip and that just miss its threshold (on and off in the builds
    that read the switch)."""
    _check_pred(run, "fline", 300)


def test_all_35_predictions_equal_the_oracle(run):
    """predict_block of every mode 0..34, luma 4..32 and both chroma components 4..16, each from the line use_filtered_refs selects."""
    _check_pred(run, "pred", 400)


def test_rough_mode_satd_equals_the_oracle(run):
    """rmd_rounds -- rmd_block's second implementation of the 35 predictions, in registers, the horizontal family transposed -- + Hadamard sums against original
    blocks (all 0, all max, the complement of the DC value, random), PU sizes 4..64."""
    _check_pred(run, "satd", 300)


def test_two_runs_give_identical_bytes(run):
    d0, d1 = run["digests"]
    ora = run["ora"]
    assert len(d0) == len(d1) == len(ora["tu_all"]) + len(ora["pr"])
    bad = np.nonzero(d0 != d1)[0]
    what = [leaf_cases.describe(ora["tu_all"][i]) if i < len(ora["tu_all"]) else leaf_cases.describe_pred(ora["pr"][i - len(ora["tu_all"])]) for i in bad[:3]]
    assert not len(bad), "build %r: %d calls gave other bytes in a second launch, e.g. %s" % (run["suffix"], len(bad), what)


def test_runners_refuse_arguments_outside_the_kernels_range(run):
    """A bad test input must not reach a kernel: sizes, components, modes, entries, QPs, context bytes and samples outside the checked ranges are all turned down by
    the host runners (leaf_device.refusals lists them), while the same call with valid arguments runs."""
    refused, tried = run["refusals"]
    assert refused == tried > 20, (refused, tried)


def test_product_library_has_no_leaf_symbols():
    """The harness is test-only: libhevcdl_hip.so exports none of its entry points (and the file holds none of their names)."""
    import hevcdl_amd
    lib = ctypes.CDLL(hevcdl_amd.LIB_PATH)
    for suffix in BUILDS:
        for name in ("hevcdl_leaf_tu_kernel", "hevcdl_leaf_pred_kernel", "hevcdl_leaf_tu_run", "hevcdl_leaf_pred_run", "hevcdl_leaf_info"):
            assert not hasattr(lib, name + suffix), name + suffix
    assert b"hevcdl_leaf" not in open(hevcdl_amd.LIB_PATH, "rb").read()
