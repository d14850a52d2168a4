"""In-loop filters on inputs no encode produces (oracle/filter_cases.py): the C oracle (oracle/hm_deblock.c, oracle/hm_sao.c) against an independent
restatement of H.265 8.7.2 / 8.7.3 (oracle/filter_spec.py), and the conditions the corpus has to meet to be worth running on the kernels
(tests/test_filters_adversarial_gpu.py).  CPU only.

For the rate-distortion choice of the SAO parameters the C oracle is the only yardstick on these inputs: the restatement does not decide, it applies
the oracle's parameters and counts the statistics they must be consistent with."""
import functools

import numpy as np
import pytest

import filter_cases as fc
import filter_spec as fs

MIN_BIN = 64


@functools.lru_cache(None)
def deblock_corpus():
    return list(fc.deblock_cases())


@functools.lru_cache(None)
def sao_corpus():
    return list(fc.sao_cases())


@functools.lru_cache(None)
def oracle_deblocked(i):
    import ref_tools
    c = deblock_corpus()[i]
    recs = np.frombuffer(c["records"].tobytes(), ref_tools.REC_DTYPE).reshape(c["n_frames"], -1)
    return ref_tools.run_deblock(c["planes"], c["w"], c["h"], c["qp"], recs, bit_depth=c["bit_depth"], tiles=c["tiles"], lf_across_tiles=c["lf_across_tiles"], lf_offsets=c["lf_offsets"])


def spec_deblock(c, f, **defects):
    return fs.deblock(c["planes"][f], c["w"], c["h"], c["qp"], c["records"][f]["depth"], c["records"][f]["tr_idx"], c["bit_depth"], c["lf_offsets"], c["tiles"], c["lf_across_tiles"], **defects)


@functools.lru_cache(None)
def oracle_sao(i):
    import ref_tools
    c = sao_corpus()[i]
    return ref_tools.run_sao(c["org"], c["dbk"], c["w"], c["h"], c["qp"], tiles=c["tiles"], bit_depth=c["bit_depth"], lf_across_tiles=c["lf_across_tiles"])


@functools.lru_cache(None)
def spec_stats(i, f, **defects):
    c = sao_corpus()[i]
    return fs.sao_stats(c["org"][f], c["dbk"][f], c["w"], c["h"], c["bit_depth"], c["tiles"], c["lf_across_tiles"], **defects)


def spec_apply(c, params, f, **defects):
    return fs.sao_apply(c["dbk"][f], params[f], c["w"], c["h"], c["bit_depth"], c["tiles"], c["lf_across_tiles"], **defects)


def first_difference(a, b, w, h):
    """(plane, y, x) of the first differing sample of two pictures [w * h * 3 / 2]."""
    i = int(np.flatnonzero(np.asarray(a).astype(np.int64) != np.asarray(b).astype(np.int64))[0])
    if i < w * h:
        return 0, i // w, i % w
    i -= w * h
    plane = 1 + i // (w * h // 4)
    i %= w * h // 4
    return plane, i // (w // 2), i % (w // 2)


def test_corpus_is_deterministic_and_every_group_is_filled():
    again_d, again_s = list(fc.deblock_cases()), list(fc.sao_cases())
    assert [c["name"] for c in again_d] == [c["name"] for c in deblock_corpus()] and [c["name"] for c in again_s] == [c["name"] for c in sao_corpus()]
    for a, b in zip(again_d, deblock_corpus()):
        assert a["planes"].tobytes() == b["planes"].tobytes() and a["records"].tobytes() == b["records"].tobytes(), a["name"]
    for a, b in zip(again_s, sao_corpus()):
        assert a["org"].tobytes() == b["org"].tobytes() and a["dbk"].tobytes() == b["dbk"].tobytes(), a["name"]
    for bd in (8, 10):
        assert {c["group"] for c in deblock_corpus() if c["bit_depth"] == bd} == set(fc.DEBLOCK_GROUPS)
        assert {c["group"] for c in sao_corpus() if c["bit_depth"] == bd} == set(fc.SAO_GROUPS)
        # every QP of the list and every offset pair, at this bit depth
        assert {c["qp"] for c in deblock_corpus() if c["bit_depth"] == bd} >= set(fc.QPS)
        assert {c["lf_offsets"] for c in deblock_corpus() if c["bit_depth"] == bd} >= set(fc.LF_OFFSETS)
    assert len({c["name"] for c in deblock_corpus()}) == len(deblock_corpus()) and len({c["name"] for c in sao_corpus()}) == len(sao_corpus())
    assert any(c["n_frames"] == 3 for c in deblock_corpus()) and any(c["n_frames"] == 3 for c in sao_corpus())


def test_synthesised_records_are_valid_quadtrees():
    """depth 0..3, TUs of 32..4, constant over the CU / TU they describe (so that the grid the filters read is one an encoder could signal)."""
    for c in deblock_corpus():
        for f in range(c["n_frames"]):
            d, t = c["records"][f]["depth"].astype(int), c["records"][f]["tr_idx"].astype(int)
            assert d.max() <= 3 and (64 >> (d + t)).max() <= 32 and (64 >> (d + t)).min() >= 4, c["name"]
            for a in range(d.shape[0]):
                D, T = d[a][fs.Z_OF], t[a][fs.Z_OF]
                ys, xs = np.mgrid[0:16, 0:16]
                cu, tu = 16 >> D, np.maximum(1, 16 >> (D + T))
                assert np.array_equal(D[ys - ys % cu, xs - xs % cu], D) and np.array_equal((D + T)[ys - ys % tu, xs - xs % tu], D + T), (c["name"], a)


def test_oracle_deblock_equals_the_restatement(oracle_built):
    for i, c in enumerate(deblock_corpus()):
        ref = oracle_deblocked(i)
        for f in range(c["n_frames"]):
            out, tally = spec_deblock(c, f)
            if not np.array_equal(out, ref[f].astype(np.int64)):
                p, y, x = first_difference(out, ref[f], c["w"], c["h"])
                pytest.fail("%s frame %d plane %d (y %d, x %d): restatement %d, oracle %d; %s" % (
                    c["name"], f, p, y, x, fs.split_planes(out, c["w"], c["h"])[p][y, x], fs.split_planes(ref[f], c["w"], c["h"])[p][y, x], fs.describe_sample(tally, p, y, x)))


def deblock_tally(bd):
    total = fs.new_tally()
    for c in deblock_corpus():
        if c["bit_depth"] == bd:
            for f in range(c["n_frames"]):
                t = spec_deblock(c, f)[1]
                t.pop("bins")
                fs.add_tally(total, t)
    return total


@pytest.mark.parametrize("bd", [8, 10])
def test_deblock_corpus_reaches_every_branch(bd):
    """Conditions on the corpus, counted by the restatement: per bit depth and per edge direction at least 64 segments in every bin of the luma
    decision (not an edge, d >= beta, strong, normal with each (dEp, dEq), the four lines not all on one side of abs(delta) < 10 * tc, delta clipped
    at +-tc, a strong-filter output clipped at +-2 * tc, a p1 / q1 correction clipped at +-(tc >> 1)), 64 chroma units filtered and 64 clipped,
    64 samples moved by ClipBD at either rail, and the hand-derived 16-bit bound of the kernel's packed luma filter met exactly:
    abs(9 * (q0 - p0) - 3 * (q1 - p1) + 8) = 12 * max + 8 on a line of a segment that takes the normal filter.

    No bin is argued away.  The +-2 * tc clip of the strong filter looks unreachable (flatness < beta >> 3, gap < (5 * tc + 1) >> 1) but is not:
    lines 1 and 2 take no part in the decision, and even on lines 0 / 3 abs(p3 - p0) and abs(p2 - 2 * p1 + p0) leave p1 = a, p2 = 2 * a free."""
    mx = (1 << bd) - 1
    t = deblock_tally(bd)
    print("deblocking tally at %d bits: %s" % (bd, t))
    for d in ("ver", "hor"):
        for k in fs.LUMA_BINS:
            assert t[d][k] >= MIN_BIN, (d, k, t[d][k])
        assert t[d]["clipbd_0"] >= MIN_BIN and t[d]["clipbd_max"] >= MIN_BIN, (d, t[d])
        assert t[d]["max_intermediate"] == 12 * mx + 8 == {8: 3068, 10: 12284}[bd], (d, t[d]["max_intermediate"])
    for k in ("chroma_filtered", "chroma_clipped", "c_clipbd_0", "c_clipbd_max"):
        assert t["chroma"][k] >= MIN_BIN, (k, t["chroma"][k])


def test_oracle_sao_picture_equals_the_restatement_on_the_oracle_parameters(oracle_built):
    for i, c in enumerate(sao_corpus()):
        params, ref = oracle_sao(i)
        for f in range(c["n_frames"]):
            out, _ = spec_apply(c, params, f)
            if not np.array_equal(out, ref[f].astype(np.int64)):
                p, y, x = first_difference(out, ref[f], c["w"], c["h"])
                s = 1 if p == 0 else 2
                a = (y * s // 64) * ((c["w"] + 63) // 64) + x * s // 64
                pytest.fail("%s frame %d plane %d (y %d, x %d) ctu %d: parameters %s" % (c["name"], f, p, y, x, a, params[f, a, p]))


def test_oracle_sao_offsets_are_consistent_with_independent_statistics(oracle_built):
    """Ties the statistics the oracle used to an independent count without restating its rate-distortion chain: sign rules, range, band position,
    and every offset equal to the rounded mean difference of its class or between it and 0."""
    for i, c in enumerate(sao_corpus()):
        params, _ = oracle_sao(i)
        for f in range(c["n_frames"]):
            diff, count = spec_stats(i, f)
            bad = fs.offset_violations(params[f], diff, count, c["bit_depth"])
            assert not bad, (c["name"], f, bad[:4])


@pytest.mark.parametrize("bd", [8, 10])
def test_sao_corpus_reaches_every_choice(oracle_built, bd):
    """Conditions on the corpus: for luma and for chroma the oracle decides off, new with each of the five types, merge-left and merge-above; an offset
    at + and at - the maximum; band positions 0 and 28; at least 64 samples clipped at 0 and at max; and per edge type `packed-max` holds a CTU
    whose statistics in one class are count * (+max) and one with count * (-max), count >= 1024."""
    m, mx = fs.max_offset(bd), (1 << bd) - 1
    seen = {0: set(), 1: set()}
    clip0 = clipmax = 0
    changed = np.zeros((5, 32), np.int64)
    packed = set()
    for i, c in enumerate(sao_corpus()):
        if c["bit_depth"] != bd:
            continue
        params, _ = oracle_sao(i)
        for f in range(c["n_frames"]):
            for comp in range(3):
                P, s = params[f, :, comp], seen[min(comp, 1)]
                s |= {"off"} if (P["mode"] == fs.MODE_OFF).any() else set()
                s |= {"merge%d" % t for t in (0, 1) if ((P["mode"] == fs.MODE_MERGE) & (P["type"] == t)).any()}
                new = P[P["mode"] == fs.MODE_NEW]
                s |= {"new%d" % t for t in np.unique(new["type"])}
                s |= {"+max"} if (new["offset"] == m).any() else set()
                s |= {"-max"} if (new["offset"] == -m).any() else set()
                s |= {"band%d" % a for a in np.unique(new[new["type"] == fs.BO]["aux"])}
            _, t = spec_apply(c, params, f)
            clip0 += t["clip_0"]; clipmax += t["clip_max"]; changed += t["changed"]
            if c["group"] == "packed-max":
                diff, count = spec_stats(i, f)
                for ty in range(4):
                    for sign in (1, -1):
                        if ((count[:, :, ty, :5] >= 1024) & (diff[:, :, ty, :5] == sign * mx * count[:, :, ty, :5])).any():
                            packed.add((ty, sign))
    print("SAO at %d bits: luma %s, chroma %s, clipped at 0 / max: %d / %d, samples changed per (type, class): %s" % (
        bd, sorted(seen[0]), sorted(seen[1]), clip0, clipmax, {ty: changed[ty][changed[ty] > 0].tolist() for ty in range(5)}))
    want = {"off", "merge0", "merge1", "+max", "-max", "band0", "band28"} | {"new%d" % t for t in range(5)}
    for comp in (0, 1):
        assert seen[comp] >= want, (comp, sorted(want - seen[comp]))
    assert clip0 >= MIN_BIN and clipmax >= MIN_BIN, (clip0, clipmax)
    assert packed == {(ty, sign) for ty in range(4) for sign in (1, -1)}, sorted(packed)


@pytest.mark.parametrize("defect", fs.DEFECTS)
def test_a_defective_deblocking_restatement_is_told_from_the_oracle(oracle_built, defect):
    """The yardstick is not vacuous: with one deliberate defect (`<` -> `<=` at 10 * tc; lines 1 / 2 decided from their own dp / dq; ClipBD dropped;
    the edge at the picture border filtered; edges of the 4x4 grid filtered) the restatement disagrees with the oracle on the corpus."""
    differing = []
    for i, c in enumerate(deblock_corpus()):
        out, _ = spec_deblock(c, 0, **{defect: True})
        if not np.array_equal(out, oracle_deblocked(i)[0].astype(np.int64)):
            differing.append(c["name"])
    print("%s: %d of %d cases differ" % (defect, len(differing), len(deblock_corpus())))
    assert differing


def test_defective_sao_restatements_are_told_from_the_oracle(oracle_built):
    """Statistics without the margins next to a right / lower CTU contradict the oracle's offsets; EO_135 and EO_45 exchanged give another picture."""
    margins, diagonals = [], []
    for i, c in enumerate(sao_corpus()):
        params, ref = oracle_sao(i)
        diff, count = spec_stats(i, 0, no_margins=True)
        if fs.offset_violations(params[0], diff, count, c["bit_depth"]):
            margins.append(c["name"])
        if not np.array_equal(spec_apply(c, params, 0, swap_diagonals=True)[0], ref[0].astype(np.int64)):
            diagonals.append(c["name"])
        diff, count = spec_stats(i, 0, swap_diagonals=True)
        if fs.offset_violations(params[0], diff, count, c["bit_depth"]) and c["name"] not in diagonals:
            diagonals.append(c["name"])
    print("no_margins: %d cases, swap_diagonals: %d cases of %d" % (len(margins), len(diagonals), len(sao_corpus())))
    assert margins and diagonals
    assert any(n.startswith("rounding/margins") for n in margins)


def test_deblock_thresholds_of_the_restatement_clamp_at_the_ends_of_the_tables():
    assert fs.thresholds(0, 8, (-6, -6)) == (0, 0, 0) and fs.thresholds(51, 8, (6, 6)) == (64, 24, 24) and fs.thresholds(51, 10, (0, 0)) == (256, 96, 52)
    assert fs.thresholds(17, 8, (0, 0)) == (7, 1, 1) and fs.thresholds(16, 8, (0, 0)) == (6, 1, 1) and fs.thresholds(15, 8, (0, 0)) == (0, 0, 0)
