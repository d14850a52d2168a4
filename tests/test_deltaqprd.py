"""CPU: DeltaQpRD without a GPU -- the candidate table and the pick rule (csrc/qp_rd.h) through the library and through a stand-alone harness built with the sanitizers,
the fixtures tests/golden/dqr_*.npz (runs of the reference encoder with --DeltaQpRD=N, tools/gen_deltaqprd_fixtures.py) against the rule and against this project's host
writer, the command line's key and every refusal's sentence."""
import ctypes
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import deltaqprd_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = dict(ids=dc.case_id)
FAMILY = ("lambda_", "sqrt_lambda", "chroma_weight", "lambda_chroma", "qp_chroma")


@pytest.fixture(scope="module")
def lib():
    import hevcdl_amd
    hevcdl_amd.build_ext()
    return hevcdl_amd.load_library()


def dbits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def family_of(c):
    return tuple(dbits(getattr(c, k)) if k != "qp_chroma" else c.qp_chroma for k in FAMILY) + tuple(dbits(v) for r in c.err_scale for v in r) + tuple(c.sbh_rd_factor)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("qp", [0, 1, 22, 32, 50, 51])
def test_candidate_table(lib, qp, n, bd):
    """Order 0, -1, +1, ...; the coded QP clipped to 0 .. 51 (8 bits); every in-range candidate carries, bit for bit, what hevcdl_config_default_bd computes for its QP;
    a clipped candidate is coded at the clipped QP with the lambda of the unclipped one; the frame lambda is 0.68 * 2^((qp - 12) / 3)."""
    import hevcdl_amd
    cfg = hevcdl_amd.default_config(64, 64, qp, bit_depth=bd, delta_qp_rd=n)
    if bd == 10 and qp - n < 0:
        out = (hevcdl_amd.QpRdCandidate * hevcdl_amd.QP_RD_MAX_CANDIDATES)()
        cnt, fl = ctypes.c_int(0), ctypes.c_double(0)
        assert lib.hevcdl_qp_rd_candidates(ctypes.byref(cfg), out, len(out), ctypes.byref(cnt), ctypes.byref(fl)) == 2      # HEVCDL_ERR_UNSUPPORTED
        return
    table, fl = hevcdl_amd.qp_rd_candidates(cfg)
    assert len(table) == 2 * n + 1 and dbits(fl) == dbits(dc.frame_lambda(qp))
    assert [c.offset for c in table] == [dc.offset_of(i) for i in range(2 * n + 1)] == [0, -1, 1, -2, 2, -3, 3][:2 * n + 1]
    for i, c in enumerate(table):
        dqp = qp + c.offset
        assert c.qp == dc.coded_qp(qp, i, bd) == min(51, max(0, dqp))
        if 0 <= dqp <= 51:
            assert family_of(c) == family_of(hevcdl_amd.default_config(64, 64, dqp, bit_depth=bd)), (qp, n, bd, i)
        else:      # QP 51 with +1: coded at 51 with the lambda of 52; QP 0 with -1 (8 bits): coded at 0 with the lambda of -1
            at = hevcdl_amd.default_config(64, 64, c.qp, bit_depth=bd)
            assert dbits(c.lambda_) == dbits(0.57 * 2.0 ** ((dqp - 12) / 3.0)) and c.lambda_ != at.lambda_
            assert dbits(c.sqrt_lambda) == dbits(c.lambda_ ** 0.5) and c.qp_chroma == at.qp_chroma and dbits(c.chroma_weight) == dbits(at.chroma_weight)
            assert dbits(c.lambda_chroma) == dbits(c.lambda_ / c.chroma_weight)
            assert [dbits(v) for r in c.err_scale for v in r] == [dbits(v) for r in at.err_scale for v in r]      # the quantiser's tables follow the coded QP
            assert list(c.sbh_rd_factor) != list(at.sbh_rd_factor) or c.qp < 4                                   # ... the sign-hiding factor the lambda too


def test_candidate_table_arguments(lib):
    import hevcdl_amd
    out = (hevcdl_amd.QpRdCandidate * hevcdl_amd.QP_RD_MAX_CANDIDATES)()
    cnt, fl = ctypes.c_int(0), ctypes.c_double(0)
    call = lambda cfg, cap=len(out): lib.hevcdl_qp_rd_candidates(ctypes.byref(cfg), out, cap, ctypes.byref(cnt), ctypes.byref(fl))
    cfg = hevcdl_amd.default_config(64, 64, 30)
    assert call(cfg) == 0 and cnt.value == 1 and out[0].offset == 0 and family_of(out[0]) == family_of(cfg)      # without the key: the one candidate a plain context runs
    cfg.delta_qp_rd = hevcdl_amd.QP_RD_MAX_N
    assert call(cfg) == 0 and cnt.value == hevcdl_amd.QP_RD_MAX_CANDIDATES == 13
    assert call(cfg, 12) == 1                                                                                      # capacity
    cfg.delta_qp_rd = hevcdl_amd.QP_RD_MAX_N + 1
    assert call(cfg) == 1
    cfg.delta_qp_rd = -1
    assert call(cfg) == 1
    assert lib.hevcdl_qp_rd_candidates(None, out, 13, ctypes.byref(cnt), ctypes.byref(fl)) == 1
    assert ctypes.sizeof(hevcdl_amd.QpRdCandidate) == 128 and hevcdl_amd.QP_RD_ROW_DTYPE.itemsize == 224


def directed_sums():
    """name -> (bits, dist, frame lambda, the index the rule must give)"""
    lam = dc.frame_lambda(32)
    out = {
        "tie_keeps_the_earlier": ([100, 100, 100], [5000, 5000, 5000], lam, 0),
        "tie_between_later_ones": ([101, 100, 100], [5000, 5000, 5000], lam, 1),
        "bits_zero": ([0, 0, 10], [700, 699, 0], lam, 2),                      # cost = dist alone; 10 bits * 69.08 = 690.8 < 699
        "all_zero": ([0, 0, 0], [0, 0, 0], lam, 0),
        "above_2_32": ([1 << 33, (1 << 33) - 1, (1 << 33) + 1], [1 << 40, 1 << 40, 1 << 40], 2.0, 1),
        "above_2_32_dist_decides": ([1 << 20] * 3, [(1 << 45) + 3, (1 << 45) + 2, (1 << 45) + 1], 1.0, 2),
        "rounding_makes_a_tie": ([3, 3], [1 << 60, (1 << 60) + 1], 0.25, 0),   # 2^60 + 1 is not a double: both costs round to the same value, the earlier stays
    }
    for k in range(1, 8):      # a winner at every index of 2k - 1 and 2k + 1 candidates, including the last
        for win in (0, k, 2 * k):
            bits = [1000 + 7 * i for i in range(2 * k + 1)]
            bits[win] = 10
            out["winner_%d_of_%d" % (win, 2 * k + 1)] = (bits[:13], [4000] * min(13, 2 * k + 1), lam, win if win < 13 else None)
    return {k: v for k, v in out.items() if v[3] is not None and len(v[0]) <= 13 and v[3] < len(v[0])}


def test_pick_rule_on_directed_sums(lib):
    import hevcdl_amd
    for name, (bits, dist, lam, want) in directed_sums().items():
        assert dc.pick(bits, dist, lam) == want, name                          # the restatement says so ...
        assert hevcdl_amd.qp_rd_pick(bits, dist, lam) == want, name            # ... and the shared source
    assert lib.hevcdl_qp_rd_pick_index(None, None, 3, 1.0) == -1
    a = np.zeros(1, np.uint64)
    assert lib.hevcdl_qp_rd_pick_index(a.ctypes.data, a.ctypes.data, 0, 1.0) == -1


def test_the_fixture_set_is_the_issues():
    assert {dc.case_id(p) for p in dc.CASES} == dc.EXPECTED
    cases = [dc.Case(p) for p in dc.CASES]
    winners = {int(i) for c in cases for i in c.chosen_idx}
    assert len(winners) >= 2 and winners - {0}                                 # at least two different indices win, one of them non-zero
    assert any(len(set(c.chosen_qp.tolist())) > 1 for c in cases)              # two pictures of one fixture end at different QPs
    assert any(c.qp == 51 for c in cases) and any(c.qp == 0 for c in cases) and any(c.bd == 10 for c in cases) and any(c.wpp for c in cases)
    assert any(c.tiles != (1, 1) for c in cases) and any(c.n == 2 for c in cases) and any(c.tools != 0x7f for c in cases)
    assert all(os.path.getsize(p) < 1 << 20 for p in dc.CASES)


@pytest.mark.parametrize("path", dc.CASES, **IDS)
def test_fixture_final_pass_is_the_winning_trial_and_the_rule_gives_the_chosen_qp(lib, path):
    """What the generator asserted, again on the committed file: the final pass's bits and dist are those of the winning trial, CTU by CTU (the generator compared whole
    records and reconstructions); the QP in every slice header is the QP of the candidate the shared rule picks from the stored sums."""
    import hevc_parse
    import hevcdl_amd
    c = dc.Case(path)
    lam = hevcdl_amd.qp_rd_candidates(hevcdl_amd.default_config(c.w, c.h, c.qp, bit_depth=c.bd, delta_qp_rd=c.n))[1]
    assert dbits(lam) == dbits(dc.frame_lambda(c.qp))
    recs = c.records(hevcdl_amd.REC_DTYPE)
    header_qps, sps, pps = [], None, None
    for _, nal in hevc_parse.split_annexb(c.stream):
        t = (nal[0] >> 1) & 63
        if t == 33:
            sps = hevc_parse.parse_sps(nal)
        elif t == 34:
            pps = hevc_parse.parse_pps(nal)
            assert pps["init_qp_m26"] == 0
        elif t <= 21:
            header_qps.append(26 + hevc_parse.parse_slice_header(nal, sps, pps)[0]["qp_delta"])
    for f in range(c.nf):
        idx = hevcdl_amd.qp_rd_pick(c.bits[f], c.dist[f], lam)
        assert idx == dc.pick(c.bits[f], c.dist[f], lam) == c.chosen_idx[f]
        assert dc.coded_qp(c.qp, idx, c.bd) == c.chosen_qp[f] == header_qps[f]
        assert np.array_equal(recs["bits"][f], c.f["cand_bits"][f, idx]) and np.array_equal(recs["dist"][f], c.f["cand_dist"][f, idx])
    assert len(header_qps) == c.nf


@pytest.mark.parametrize("path", dc.CASES, **IDS)
def test_host_writer_reproduces_the_stream_from_records_and_chosen_qps(lib, oracle_built, path):
    """The reference's final records and its chosen QPs, the oracle's SAO decision on the reference's deblocked picture with the chosen QP's lambdas -> this project's
    writer gives the reference's stream byte for byte: slice_qp_delta and the contexts' initialisation follow the picture's QP, no parameter set does."""
    import hevcdl_amd
    import ref_tools
    c = dc.Case(path)
    recs = c.records(hevcdl_amd.REC_DTYPE)
    got = b""
    for poc in range(c.nf):
        sao = sao_of(c, poc, ref_tools)
        got += hevcdl_amd.write_access_unit(c.w, c.h, int(c.chosen_qp[poc]), poc, recs[poc], sao=sao, tiles=c.tiles, bit_depth=c.bd, tools=c.tools, wavefront=c.wpp)
    assert got == dc.strip_sei(c.stream)


def sao_of(c, poc, ref_tools):
    """The SAO parameters of one picture by the oracle (oracle/hm_sao.c) at the picture's QP.  The oracle derives its lambdas from the QP it is given; a clipped candidate's
    lambda is that of the unclipped QP, which the oracle cannot be told: those fixtures (QP 51 + 1, QP 0 - 1) chose an unclipped candidate, asserted here."""
    idx = int(c.chosen_idx[poc])
    assert 0 <= c.qp + dc.offset_of(idx) <= 51
    params, final = ref_tools.run_sao(c.yuv[poc:poc + 1], c.deblocked[poc:poc + 1], c.w, c.h, int(c.chosen_qp[poc]), tiles=c.tiles, bit_depth=c.bd)
    assert np.array_equal(np.asarray(final).reshape(-1), c.final[poc])
    return np.frombuffer(np.ascontiguousarray(params).tobytes(), hevcdl_amd_sao_dtype()).reshape(-1, 3)


def hevcdl_amd_sao_dtype():
    import hevcdl_amd
    return hevcdl_amd.SAO_DTYPE


# ---- refusals: hevcdl_create and the command line, in the same words ----------------------------------------------------------------------------------------------------
REFUSALS = [      # (configuration keywords, command-line keys, status, a piece of the sentence)
    (dict(delta_qp_rd=7), ["--DeltaQpRD=7"], 1, "DeltaQpRD is 0 .. 6"),
    (dict(delta_qp_rd=-1), ["--DeltaQpRD=-1"], 1, "DeltaQpRD is 0 .. 6"),
    (dict(delta_qp_rd=1, slices=(1, 2)), ["-dqr", "1", "--SliceMode=1", "--SliceArgument=2"], 2, "DeltaQpRD together with slices is not supported"),
    (dict(delta_qp_rd=1, tiles=(2, 1), segments=(3, 1)), ["--DeltaQpRD=1", "--NumTileColumnsMinus1=1", "--TileUniformSpacing=1", "--SliceSegmentMode=3", "--SliceSegmentArgument=1"], 2,
     "DeltaQpRD together with slice segments is not supported"),
    (dict(delta_qp_rd=2, deblocking_metric=1, lf_offset_in_pps=False), ["--DeltaQpRD=2", "--DeblockingFilterMetric=1", "--LoopFilterOffsetInPPS=0"], 2, "DeltaQpRD together with DeblockingFilterMetric is not supported"),
    (dict(delta_qp_rd=3, bit_depth=10, qp=2), ["--DeltaQpRD=3", "--InputBitDepth=10", "-q", "2"], 2, "DeltaQpRD at 10 bits needs QP - DeltaQpRD >= 0"),
]


@pytest.mark.parametrize("kw,keys,status,piece", REFUSALS, ids=[r[3][:40].replace(" ", "_") for r in REFUSALS])
def test_create_refuses_with_a_reason(lib, kw, keys, status, piece):
    """hevcdl_create refuses before it looks for a device, so this runs without one; the sentence is in hevcdl_create_error."""
    import hevcdl_amd
    kw = dict(kw)
    w = 512 if "tiles" in kw else 128
    cfg = hevcdl_amd.default_config(w, 128, kw.pop("qp", 32), **kw)
    h, wts = ctypes.c_void_p(), hevcdl_amd.load_weights()
    assert lib.hevcdl_create(ctypes.byref(cfg), wts.ctypes.data, wts.size, ctypes.byref(h)) == status
    assert piece in lib.hevcdl_create_error().decode()


@pytest.fixture(scope="module")
def app():
    import hevcdl_amd
    return hevcdl_amd.build_app()


@pytest.mark.parametrize("kw,keys,status,piece", REFUSALS, ids=[r[3][:40].replace(" ", "_") for r in REFUSALS])
def test_cli_refuses_in_the_same_words(app, tmp_path, kw, keys, status, piece):
    w = 512 if "tiles" in kw else 128
    base = ["-wdt", str(w), "-hgt", "128"] + ([] if "-q" in keys else ["-q", "32"])
    r = subprocess.run([app] + base + keys + ["--PrintConfig"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cfg = json.loads(r.stdout)
    assert r.returncode == 2 and any(piece in e and e.startswith("DeltaQpRD = ") for e in cfg["errors"]), cfg["errors"]
    r = subprocess.run([app, "-i", "none.yuv"] + base + keys, cwd=tmp_path, capture_output=True, text=True, timeout=120)      # ... and without --PrintConfig, before any file is opened
    assert r.returncode == 2 and piece in r.stderr


def test_cli_key_and_its_short_form(app, tmp_path):
    """DeltaQpRD is a used key (the parent refused everything but 0 with "only 0 is implemented"): long form, short form, a cfg file line; tiles and wavefront go with it."""
    for keys, want in ((["--DeltaQpRD=2"], 2), (["-dqr", "3"], 3), (["--DeltaQpRD=0"], 0), ([], 0), (["--DeltaQpRD=1", "--WaveFrontSynchro=1"], 1),
                       (["-dqr", "6", "--NumTileColumnsMinus1=1", "--TileUniformSpacing=1"], 6)):
        r = subprocess.run([app, "-wdt", "512", "-hgt", "128", "-q", "30"] + keys + ["--PrintConfig"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        cfg = json.loads(r.stdout)
        assert r.returncode == 0 and cfg["errors"] == [] and cfg["DeltaQpRD"] == want, (keys, cfg["errors"])
    (tmp_path / "k.cfg").write_text("DeltaQpRD                     : 2           # slice-based multi-QP optimization\nSourceWidth : 128\nSourceHeight : 128\nQP : 32\n")
    r = subprocess.run([app, "-c", "k.cfg", "--PrintConfig"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and json.loads(r.stdout)["DeltaQpRD"] == 2


def test_python_front_ends_refuse(lib):
    import hevcdl_amd
    import hevcdl_amd.pipeline as pipeline
    with pytest.raises(ValueError, match="tile-sharded path does not search the slice QP"):
        pipeline.encode_sequence_tile_sharded("none.yuv", 512, 128, 32, 1, (2, 1), delta_qp_rd=1)
    assert hevcdl_amd.default_config(128, 128, 32).delta_qp_rd == 0 and hevcdl_amd.default_config(128, 128, 32, delta_qp_rd=2).delta_qp_rd == 2


# ---- the shared header under the sanitizers ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/deltaqprd_harness.cpp under AddressSanitizer and UndefinedBehaviorSanitizer (a program of its own: nothing is loaded into python)."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host g++")
    d = tmp_path_factory.mktemp("deltaqprd")
    exe = str(d / "deltaqprd_harness")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "hevc-deep-learning-pipeline_amd", "csrc"), os.path.join(ROOT, "tests", "deltaqprd_harness.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def ask(mode, rows):
        path = d / "cases.txt"
        path.write_text("".join(" ".join(str(int(v)) for v in r) + "\n" for r in rows))
        r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True)
        startup = ("error while loading shared libraries", "ASan runtime does not come first", "Shadow memory range interleaves", "ReserveShadowMemoryRange failed")
        if r.returncode != 0 and not r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and any(m in r.stderr for m in startup):
            pytest.skip("the sanitizer build cannot start here: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200])
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
        return r.stdout.splitlines()
    return ask


def test_table_under_the_sanitizers_equals_the_library(lib, harness):
    import hevcdl_amd
    cases = [(qp, n, bd) for qp in (0, 1, 5, 22, 32, 46, 50, 51) for n in range(0, 7) for bd in (8, 10)] + [(32, 7, 8), (32, -1, 8), (52, 1, 8), (-1, 1, 8), (30, 1, 12)]
    lines = iter(harness("table", cases))
    for qp, n, bd in cases:
        count, fl = (int(v) for v in next(lines).split())
        ok = 0 <= n <= 6 and 0 <= qp <= 51 and bd in (8, 10) and not (bd == 10 and qp - n < 0)
        assert (count == 2 * n + 1) if ok else (count == -1), (qp, n, bd, count)
        if not ok:
            continue
        table, lam = hevcdl_amd.qp_rd_candidates(hevcdl_amd.default_config(64, 64, qp, bit_depth=bd, delta_qp_rd=n))
        assert fl == dbits(lam)
        for c in table:
            v = [int(x) for x in next(lines).split()]
            assert (v[0], v[1]) == (c.offset, c.qp) and (v[3], v[4], v[5], v[6], v[2]) + tuple(v[7:]) == family_of(c), (qp, n, bd, c.offset)


def test_pick_rule_under_the_sanitizers(harness):
    rng = np.random.default_rng(31)
    rows, want = [], []
    for name, (bits, dist, lam, w) in directed_sums().items():
        rows.append([len(bits), dbits(lam)] + [v for p in zip(bits, dist) for v in p])
        want.append(w)
    for _ in range(300):      # random sums, many of them ties or near ties
        n = int(rng.choice([1, 3, 5, 7, 13]))
        lam = dc.frame_lambda(int(rng.integers(0, 52)))
        bits = rng.integers(0, 1 << int(rng.integers(4, 40)), n)
        dist = rng.integers(0, 1 << int(rng.integers(4, 50)), n)
        if rng.integers(0, 2):
            j, k = rng.integers(0, n, 2)
            bits[j], dist[j] = bits[k], dist[k]
        rows.append([n, dbits(lam)] + [int(v) for p in zip(bits, dist) for v in p])
        want.append(dc.pick(bits, dist, lam))
    assert [int(l) for l in harness("pick", rows)] == want


def test_refusals_under_the_sanitizers(harness):
    rows = [(32, 8, 0, 1, 3, 2), (32, 8, 1, 0, 0, 0), (0, 8, 6, 0, 0, 0), (32, 8, 7, 0, 0, 0), (32, 8, 1, 1, 0, 0), (32, 8, 1, 0, 1, 0), (32, 8, 1, 0, 0, 2), (2, 10, 3, 0, 0, 0), (3, 10, 3, 0, 0, 0)]
    got = [l.split("|", 1) for l in harness("keys", rows)]
    assert [int(g[0]) for g in got] == [0, 0, 0, 1, 2, 2, 2, 2, 0]
    assert [bool(g[1]) for g in got] == [False, False, False, True, True, True, True, True, False]
    assert "slices" in got[4][1] and "slice segments" in got[5][1] and "DeblockingFilterMetric" in got[6][1] and "10 bits" in got[7][1]
