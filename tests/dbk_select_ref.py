"""TEST INFRASTRUCTURE: the per-picture deblocking parameters of DeblockingFilterMetric 1 and 2, restated on the CPU from the unchanged oracle and numpy.

metric_sums / metric_choice follow TEncGOP::applyDeblockingFilterMetric (TEncGOP.cpp:3185-3302) line by line in Python integers; distortion / trial_table / walk follow
xFindDistortionFrame (:2172-2200) and applyDeblockingFilterParameterSelection (:3304-3421), every trial a whole-picture run of the oracle's deblocking; pictures() runs the whole picture
pipeline of a fixture on the CPU -- oracle decisions, the choice, the oracle's deblocking with the picture's offsets (ref_tools.run_deblock(..., lf_offsets=)), the
oracle's SAO -- so that the writer can be held to the reference's stream and the final pictures to its reconstruction file (tests/test_dbk_select.py).  That ties this
restatement to the reference; the GPU tests then hold the kernels to this restatement."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_tools              # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
BETA = [0] * 16 + [6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60, 62, 64]      # TComLoopFilter.cpp:64-67
CHOICE = np.dtype([("override_enabled", "<i4"), ("override_flag", "<i4"), ("disabled", "<i4"), ("beta_offset_div2", "<i4"), ("tc_offset_div2", "<i4")])      # hevcdl_dbk_choice


def thresholds(qp, bit_depth):
    scale = 1 << (bit_depth - 8)
    return 2 * scale, (BETA[min(max(qp, 0), 51)] * scale) >> 2      # thr1, thr2 (:3208-3211)


def _edge_sad(p2, p1, p0, q0, q1, q2, thr1, thr2):
    a = (np.abs(p2 - 2 * p1 + p0) + np.abs(q0 - 2 * q1 + q2)) << 1
    return int(np.abs(p0 - q0)[(thr1 < a) & (a < thr2)].sum())


def metric_sums(luma, qp, bit_depth):
    """luma [h, w] before deblocking -> (colSADsum, rowSADsum) of :3216-3268: every edge at a multiple of 32 is computed, the first noCol - 1 / noRows - 1 are added."""
    y = np.asarray(luma).astype(np.int64)
    h, w = y.shape
    thr1, thr2 = thresholds(qp, bit_depth)
    no_col, no_rows = w >> 5, h >> 5
    assert no_col > 1 and no_rows > 1
    col = [_edge_sad(y[:, c - 3], y[:, c - 2], y[:, c - 1], y[:, c], y[:, c + 1], y[:, c + 2], thr1, thr2) for c in range(32, w, 32)]
    row = [_edge_sad(y[r - 3], y[r - 2], y[r - 1], y[r], y[r + 1], y[r + 2], thr1, thr2) for r in range(32, h, 32)]
    return sum(col[:no_col - 1]), sum(row[:no_rows - 1])


def metric_offset(w, h, bit_depth, col_sum, row_sum):
    """:3270-3283 -> the offset 2 .. 6 of an override, or 0."""
    c, r = int(col_sum) << 10, int(row_sum) << 10
    c = c // ((w >> 5) - 1) // h
    r = r // ((h >> 5) - 1) // w
    avg = ((c + r) >> 1) >> (bit_depth - 8)
    if avg <= 2048:
        return 0
    return min(max(avg >> 9, 2), 6)


def metric_choice(w, h, bit_depth, col_sum, row_sum, pps_offsets=(0, 0)):
    o = metric_offset(w, h, bit_depth, col_sum, row_sum)
    return np.array([(1, 1, 0, o, o) if o else (1, 0, 0, pps_offsets[0], pps_offsets[1])], CHOICE)[0]


def plain_choice(lf_offset_in_pps, lf_disable, lf_offsets):
    """What every picture carries without the metric (TEncSlice.cpp:388-404)."""
    e = 0 if lf_offset_in_pps else 1
    return np.array([(e, e, 1 if lf_disable else 0, 0 if lf_disable else lf_offsets[0], 0 if lf_disable else lf_offsets[1])], CHOICE)[0]


def distortion(org, pic, bit_depth):
    """xFindDistortionFrame: all three components, (d * d) >> 2 (bd - 8) per sample."""
    d = np.asarray(org).astype(np.int64) - np.asarray(pic).astype(np.int64)
    return int(((d * d) >> (2 * (bit_depth - 8))).sum())


def trial(d, org, recon, recs, b, t):
    """The distortion of ONE picture (org, recon [samples], recs [ctus]) deblocked with slice_beta_offset_div2 b and slice_tc_offset_div2 t."""
    pic = ref_tools.run_deblock(recon[None], d["width"], d["height"], d["qp"], recs[None], bit_depth=d["bit_depth"], tiles=d["tiles"],
                                lf_across_tiles=bool(d["lf_across_tiles"]), lf_offsets=(b, t))[0]
    return distortion(org, pic, d["bit_depth"])


def trial_table(d, org, recon, recs):
    """All 49 entries [b + 3][t + 3] of one picture."""
    return np.array([[trial(d, org, recon, recs, b, t) for t in range(-3, 4)] for b in range(-3, 4)], np.uint64)


def clip3(lo, hi, v):
    return max(lo, min(hi, v))


def walk(dist_of, state, pps_offsets=(0, 0)):
    """:3335-3420 with dist_of(b, t) in the place of restore + loopFilterPic + xFindDistortionFrame, called for exactly the pairs the reference tries.  state = m_DBParam[0]:
    [available, disabled, beta, tc] -> (choice, new state, the pairs tried in order)."""
    U64 = (1 << 64) - 1
    narrow = bool(state[0]) and not state[1]
    max_b = clip3(-3, 3, state[2] + 1) if narrow else 3
    min_b = clip3(-3, 3, state[2] - 1) if narrow else -3
    max_t = clip3(-3, 3, state[3] + 2) if narrow else 3
    min_t = clip3(-3, 3, state[3] - 2) if narrow else -3
    dist_beta_prev, dist_min, disabled_best, beta_best, tc_best, tried = U64, U64, True, 0, 0, []
    b = max_b
    while b >= min_b:
        dist_tc_min = U64
        t = max_t
        while t >= min_t:
            dist = int(dist_of(b, t)); tried.append((b, t))
            if dist < dist_min:
                dist_min, disabled_best, beta_best, tc_best = dist, False, b, t
            if dist < dist_tc_min:
                dist_tc_min = dist
            elif t < -2:
                break
            t -= 1
        if b < -1 and dist_tc_min >= dist_beta_prev:
            break
        dist_beta_prev = dist_tc_min
        b -= 1
    new = [1, int(disabled_best), beta_best, tc_best]
    if disabled_best:
        c = (1, 1, 1, 0, 0)
    elif (beta_best, tc_best) == tuple(pps_offsets):
        c = (1, 0, 0, pps_offsets[0], pps_offsets[1])
    else:
        c = (1, 1, 0, beta_best, tc_best)
    return np.array([c], CHOICE)[0], new, tried


def load(name):
    """A tests/golden/dbksel_<name>.npz as a dict of plain values."""
    z = np.load(os.path.join(GOLD, "dbksel_%s.npz" % name))
    d = {k: z[k] for k in z.files}
    for k in ("width", "height", "qp", "bit_depth", "metric", "lf_offset_in_pps", "lf_disable", "lf_across_tiles"):
        d[k] = int(d[k])
    d["lf_offsets"] = tuple(int(v) for v in d["lf_offsets"])
    d["tiles"] = tuple(int(v) for v in d["tiles"])
    return d


def names():
    return sorted(f[len("dbksel_"):-len(".npz")] for f in os.listdir(GOLD) if f.startswith("dbksel_") and f.endswith(".npz"))


def choices_for(d, recon, recs=None):
    """The choice of every picture of fixture d whose reconstructions before deblocking are recon [n, samples]."""
    w, h, bd = d["width"], d["height"], d["bit_depth"]
    if d["metric"] == 0:
        return np.array([plain_choice(d["lf_offset_in_pps"], d["lf_disable"], d["lf_offsets"])] * recon.shape[0], CHOICE)
    out = []
    state = [0, 0, 0, 0]      # a fixture is a sequence from its first picture
    for f in range(recon.shape[0]):
        if d["metric"] == 1:
            cs, rs = metric_sums(recon[f, :w * h].reshape(h, w), d["qp"], bd)
            out.append(metric_choice(w, h, bd, cs, rs, d["lf_offsets"]))
        else:
            assert d["metric"] == 2 and recs is not None
            c, state, _ = walk(lambda b, t: trial(d, d["yuv"][f], recon[f], recs[f], b, t), state, d["lf_offsets"])
            out.append(c)
    return np.array(out, CHOICE)


def deblock_with(d, recon, recs, choices):
    """The oracle's deblocking, every picture with its own offsets; a disabled picture passes."""
    out = np.array(recon, copy=True)
    for f in range(recon.shape[0]):
        if choices[f]["disabled"]:
            continue
        out[f] = ref_tools.run_deblock(recon[f:f + 1], d["width"], d["height"], d["qp"], recs[f:f + 1], bit_depth=d["bit_depth"], tiles=d["tiles"],
                                       lf_across_tiles=bool(d["lf_across_tiles"]), lf_offsets=(int(choices[f]["beta_offset_div2"]), int(choices[f]["tc_offset_div2"])))[0]
    return out


def pictures(d):
    """The whole picture pipeline of fixture d on the CPU -> (records, reconstruction before deblocking, choices, deblocked, SAO parameters, final pictures)."""
    w, h, bd = d["width"], d["height"], d["bit_depth"]
    recs, recon, _ = ref_tools.run_oracle(d["yuv"], w, h, d["qp"], d["labels"], tiles=d["tiles"], bit_depth=bd)
    choices = choices_for(d, recon, recs)
    dbk = deblock_with(d, recon, recs, choices)
    sao, final = ref_tools.run_sao(d["yuv"], dbk, w, h, d["qp"], tiles=d["tiles"], bit_depth=bd, lf_across_tiles=bool(d["lf_across_tiles"]))
    return recs, recon, choices, dbk, sao, final
