"""oracle/filter_cases.py -- TEST INFRASTRUCTURE, not product code.

Adversarial input corpus of the two in-loop filters: deterministic, seeded, named groups.  Every test that reached the deblocking and the SAO kernels
before fed them what an encode produced (a reconstruction within quantisation error of its source, the TU grid the search chose); these cases are
built for the rest of the input space, where the kernels' packed arithmetic, line pairing, clips and tile / border handling decide the result:
step heights around every threshold of the filter decision, samples on the rails, lines 1 / 2 of a segment unlike lines 0 / 3, whole-range noise,
QPs where the tables clamp, sizes against the kernels' tiling; for SAO the extreme sums of the packed statistics, band edges, clips, rounding
ties, merge ties.  Both filters read only `depth` and `tr_idx` of a CTU record, so the records are synthesised quadtrees.

deblock_cases() / sao_cases() yield dicts; tests/test_filters_adversarial.py holds the corpus to coverage conditions counted by oracle/filter_spec.py.
"""
import numpy as np

import filter_spec as fs

SEED = 20250911
DEBLOCK_GROUPS = ("steps", "ramps", "rails", "lines", "noise", "qp", "sizes")
SAO_GROUPS = ("packed-max", "bands", "clip", "rounding", "merge", "noise", "sizes")
QPS = (0, 15, 16, 17, 18, 19, 26, 37, 50, 51)
LF_OFFSETS = ((0, 0), (6, 6), (-6, -6), (6, -6), (-6, 6))
REC_DTYPE = np.dtype([("depth", "u1", 256), ("part_size", "u1", 256), ("luma_dir", "u1", 256), ("chroma_dir", "u1", 256), ("tr_idx", "u1", 256),
                      ("cbf", "u1", (3, 256)), ("tskip", "u1", (3, 256)), ("bits", "<u4"), ("dist", "<u4"), ("cost", "<f8"),
                      ("coeff_y", "<i2", 4096), ("coeff_cb", "<i2", 1024), ("coeff_cr", "<i2", 1024)])      # hevcdl_ctu_record (include/hevcdl.h)


# ---- records: quadtrees ---------------------------------------------------------------------------------------------------------------------
def _ctu_tree(rng, kind):
    """(depth, tr_idx) [16, 16] per 4x4 block of one CTU.  kind "rand": a random valid quadtree (CU depth 0..3, TUs 32..4; 4x4 TUs put edges off the
    8x8 grid); "tu32": one CU, four 32x32 TUs; "tu4": every CU 8x8 with 4x4 TUs; "tu8": every CU 8x8, one TU."""
    D, T = np.zeros((16, 16), np.uint8), np.zeros((16, 16), np.uint8)
    if kind != "rand":
        D[:], T[:] = {"tu32": (0, 1), "tu4": (3, 1), "tu8": (3, 0)}[kind]
        return D, T

    def tu(x, y, n, d, tr):
        if n * 4 > 32 or (n > 1 and rng.random() < 0.4):
            for k in range(4):
                tu(x + (k & 1) * n // 2, y + (k >> 1) * n // 2, n // 2, d, tr + 1)
        else:
            D[y:y + n, x:x + n], T[y:y + n, x:x + n] = d, tr

    def cu(x, y, n, d):
        if d < 3 and rng.random() < (0.85, 0.6, 0.5)[d]:
            for k in range(4):
                cu(x + (k & 1) * n // 2, y + (k >> 1) * n // 2, n // 2, d + 1)
        else:
            tu(x, y, n, d, 0)
    cu(0, 0, 16, 0)
    return D, T


def make_records(rng, w, h, n_frames, kind):
    """[n_frames, ctus] records with depth / tr_idx in z-scan order; kind as _ctu_tree, or "per-frame": frame f takes ("rand", "tu4", "tu32")[f % 3]."""
    nctu = ((w + 63) // 64) * ((h + 63) // 64)
    recs = np.zeros((n_frames, nctu), REC_DTYPE)
    for f in range(n_frames):
        k = ("rand", "tu4", "tu32")[f % 3] if kind == "per-frame" else kind
        for a in range(nctu):
            D, T = _ctu_tree(rng, k)
            recs[f, a]["depth"][fs.Z_OF] = D
            recs[f, a]["tr_idx"][fs.Z_OF] = T
    return recs


# ---- deblocking content -----------------------------------------------------------------------------------------------------------------------
def _per_tu(rng, tu, draw):
    """A value per transform block, spread over its samples: [h, w]."""
    h4, w4 = tu.shape
    ys, xs = np.mgrid[0:h4, 0:w4] * 4
    key = ((ys - ys % tu) // 4) * w4 + (xs - xs % tu) // 4
    return np.repeat(np.repeat(draw(h4 * w4)[key], 4, axis=0), 4, axis=1)


def _aim(P):
    """Thresholds to aim content at: the case's own, or those of a middling QP where the case's are 0 (nothing is filtered there)."""
    s = P["mx"] // 255
    return (P["tc"] or 4 * s), (P["beta"] or 32 * s)


def _gen_steps(rng, h, w, tu, P):
    tc, beta = _aim(P)
    g, cut = (5 * tc + 1) >> 1, (160 * tc - 8) // 9
    heights = np.array([0, 1, g - 1, g, g + 1, cut - 1, cut, cut + 1, cut + 2, 2 * tc, 3 * tc, P["mx"] // 4, P["mx"]])
    base = np.repeat(np.repeat(rng.integers(0, P["mx"] + 1, ((h + 63) // 64, (w + 63) // 64)), 64, 0), 64, 1)[:h, :w]
    step = _per_tu(rng, tu, lambda n: heights[rng.integers(0, len(heights), n)] * rng.choice([-1, 1], n))
    amps = np.array([0, 0, 0, 1, 2, beta // 16, beta // 8, beta // 4, beta // 2])
    amp = _per_tu(rng, tu, lambda n: amps[rng.integers(0, len(amps), n)])
    noise = np.rint((rng.random((h, w)) * 2 - 1) * amp).astype(np.int64)
    return np.clip(base + step + noise, 0, P["mx"])


def _gen_ramps(rng, h, w, tu, P):
    tc, beta = _aim(P)
    g = (5 * tc + 1) >> 1
    ys, xs = np.mgrid[0:h, 0:w]
    smax = max(1, (beta >> 3) // 6 + 1)                                     # 6 * slope around beta >> 3
    sx = _per_tu(rng, tu, lambda n: rng.integers(-smax, smax + 1, n) * rng.integers(0, 2, n))
    ramp = (sx * xs + rng.integers(0, smax + 1) * ys) // 2
    offs = np.array([0, 0, g - 2, g - 1, g, g + 1, 2 * g])
    off = _per_tu(rng, tu, lambda n: offs[rng.integers(0, len(offs), n)] * rng.choice([-1, 1], n))
    return np.clip(P["mx"] // 2 + ramp + off, 0, P["mx"])


def _inner_lines(rng, h, w, density):
    """Samples on lines 1 / 2 of the segments: rows 1, 2 of every 4 (vertical edges) in one half of the 16x16 blocks, columns 1, 2 of every 4
    (horizontal edges) in the other; a segment is hit with probability `density`."""
    ys, xs = np.mgrid[0:h, 0:w]
    mode = ((ys >> 4) + (xs >> 4)) & 1
    hit = np.repeat(np.repeat(rng.random(((h + 3) // 4, (w + 3) // 4)) < density, 4, 0), 4, 1)[:h, :w]
    return np.where(mode == 0, (ys % 4 == 1) | (ys % 4 == 2), (xs % 4 == 1) | (xs % 4 == 2)) & hit


def _normal_base(rng, h, w, tu, P):
    """Piecewise constant per TU with steps that take the normal filter (gap >= (5 * tc + 1) >> 1, delta below 10 * tc)."""
    tc, beta = _aim(P)
    g, cut = (5 * tc + 1) >> 1, (160 * tc - 8) // 9
    lvl = _per_tu(rng, tu, lambda n: rng.integers(0, 2, n))
    ys, xs = np.mgrid[0:h, 0:w]
    lvl = (lvl + (ys >> 3) + (xs >> 3)) & 1                                  # neighbouring 8x8 blocks differ whatever the TU grid
    return lvl * rng.integers(g, max(g + 1, cut), (1, 1))


def _gen_lines(rng, h, w, tu, P):
    tc, beta = _aim(P)
    base = P["mx"] // 3 + _normal_base(rng, h, w, tu, P)
    spread = rng.integers(-40 * tc, 40 * tc + 1, (h, w))
    return np.clip(np.where(_inner_lines(rng, h, w, 0.7), base + spread, base), 0, P["mx"])


def _gen_rails(rng, h, w, tu, P):
    """Lines 0 / 3: near a rail, steps that take the normal filter.  Lines 1 / 2: rail values, and the pattern of the hand-derived 16-bit bound of the
    packed luma filter: p1 p0 | q0 q1 = max 0 | max 0 and its mirror (9 * max + 3 * max + 8)."""
    tc, beta = _aim(P)
    mx = P["mx"]
    ys, xs = np.mgrid[0:h, 0:w]
    low = np.repeat(np.repeat(rng.integers(0, 2, ((h + 31) // 32, (w + 31) // 32)), 32, 0), 32, 1)[:h, :w] == 1
    step = _normal_base(rng, h, w, tu, P)
    wob = rng.integers(0, max(1, beta // 8), (h, w)) * (rng.random((h, w)) < 0.3)
    base = np.where(low, step + wob, mx - step - wob)
    inner = _inner_lines(rng, h, w, 0.8)
    palette = np.array([0, 0, mx, mx, 1, mx - 1, tc, mx - tc])
    rnd = palette[rng.integers(0, len(palette), (h, w))]
    # bound pattern along the filtered direction: positions -2 -1 | 0 1 relative to an 8-grid edge = max 0 max 0 (or mirrored per 8x8 block)
    mode = ((ys >> 4) + (xs >> 4)) & 1
    t = np.where(mode == 0, xs, ys) % 8                                      # position across the edge
    flip = (((ys >> 3) * 5 + (xs >> 3) * 3) >> 1) & 1
    bound = np.where((t == 6) | (t == 0), mx, 0)
    bound = np.where(flip == 1, mx - bound, bound)
    near = (t >= 6) | (t <= 1)
    use_bound = np.repeat(np.repeat(rng.random(((h + 7) // 8, (w + 7) // 8)) < 0.5, 8, 0), 8, 1)[:h, :w]
    val = np.where(use_bound & near, bound, np.where(use_bound, base, rnd))
    return np.clip(np.where(inner, val, base), 0, mx)


def _gen_noise(rng, h, w, tu, P):
    return rng.integers(0, P["mx"] + 1, (h, w))


_GEN = {"steps": _gen_steps, "ramps": _gen_ramps, "rails": _gen_rails, "lines": _gen_lines, "noise": _gen_noise}


def _deblock_case(seed_key, name, group, content, w, h, qp, bd, grid="rand", tiles=(1, 1), lf=True, off=(0, 0), n_frames=1):
    rng = np.random.default_rng([SEED, 1] + list(seed_key))
    recs = make_records(rng, w, h, n_frames, grid)
    beta, tc, tc_c = fs.thresholds(qp, bd, off)
    P = {"mx": (1 << bd) - 1, "beta": beta, "tc": tc}
    frames = []
    for f in range(n_frames):
        tu = fs.tu_size_map(recs[f]["depth"], recs[f]["tr_idx"], w, h)
        planes = [_GEN[content](rng, h, w, tu, P)]
        for c in range(2):                                                    # chroma: the same recipe at luma size, every second sample
            planes.append(_GEN[content](rng, h, w, tu, dict(P, tc=tc_c))[::2, ::2])
        frames.append(np.concatenate([p.ravel() for p in planes]))
    return {"name": name, "group": group, "w": w, "h": h, "qp": qp, "bit_depth": bd, "tiles": tiles, "lf_across_tiles": lf, "lf_offsets": off,
            "n_frames": n_frames, "records": recs, "planes": np.stack(frames).astype(np.uint8 if bd == 8 else np.uint16)}


def deblock_cases():
    """Yields the deblocking cases: dict(name, group, w, h, qp, bit_depth, tiles, lf_across_tiles, lf_offsets, n_frames, records [n, ctus], planes [n, w * h * 3 / 2])."""
    k = 0
    for bd in (8, 10):
        def case(group, content, w, h, qp, **kw):
            nonlocal k
            k += 1
            tag = "%s/%s-%dx%d-q%d-b%d" % (group, content, w, h, qp, bd)
            for key in ("grid", "off", "tiles", "lf", "n_frames"):
                if key in kw:
                    tag += "-%s%s" % (key[0], str(kw[key]).replace(" ", ""))
            return _deblock_case([k], tag, group, content, w, h, qp, bd, **kw)
        yield case("steps", "steps", 248, 24, 37)
        yield case("steps", "steps", 504, 72, 26, off=(6, -6))
        yield case("steps", "steps", 200, 136, 45, grid="tu4")
        yield case("ramps", "ramps", 256, 32, 37)
        yield case("ramps", "ramps", 264, 40, 51, off=(-6, 6))
        yield case("ramps", "ramps", 200, 136, 32, grid="tu8")
        yield case("ramps", "ramps", 200, 136, 44, grid="tu8", off=(0, -3))
        yield case("rails", "rails", 264, 40, 51, grid="tu8")
        yield case("rails", "rails", 200, 136, 37, grid="tu4", off=(6, 6))
        yield case("rails", "rails", 504, 72, 50)
        yield case("rails", "rails", 264, 40, 30, grid="tu8")
        yield case("lines", "lines", 504, 72, 37)
        yield case("lines", "lines", 264, 40, 50, grid="tu8")
        yield case("lines", "lines", 200, 136, 28, grid="tu4")
        yield case("noise", "noise", 264, 40, 37)
        yield case("noise", "noise", 72, 72, 51, off=(6, 6))
        for i, qp in enumerate(QPS):                                          # every QP and every offset pair at both bit depths
            yield case("qp", "steps" if i % 2 == 0 else "lines", 264, 40, qp, off=LF_OFFSETS[(i + (bd == 10)) % 5])
        for w, h in ((8, 8), (16, 8), (248, 24), (256, 32), (264, 40), (504, 72)):
            yield case("sizes", "steps", w, h, 34)
        yield case("sizes", "steps", 520, 200, 37, tiles=(2, 2), lf=False)
        yield case("sizes", "lines", 520, 200, 37, tiles=(2, 2), lf=True)
        yield case("sizes", "steps", 1032, 136, 32, tiles=([5, 4, 8], [1, 2]), lf=False)
        yield case("sizes", "steps", 264, 40, 37, grid="per-frame", n_frames=3)      # the batch; the GPU test also runs it with in == out


# ---- SAO content --------------------------------------------------------------------------------------------------------------------------------
def _frame(planes, bd):
    return np.concatenate([np.asarray(p).ravel() for p in planes]).astype(np.uint8 if bd == 8 else np.uint16)


def _sao_case(name, group, w, h, qp, bd, org, dbk, tiles=(1, 1), lf=True):
    org, dbk = np.atleast_2d(org), np.atleast_2d(dbk)
    return {"name": name, "group": group, "w": w, "h": h, "qp": qp, "bit_depth": bd, "tiles": tiles, "lf_across_tiles": lf, "n_frames": org.shape[0], "org": org, "dbk": dbk}


def _shapes(w, h):
    return ((h, w), (h // 2, w // 2), (h // 2, w // 2))


def _packed_max(pattern, w, h, bd):
    """dbk on the rails in a pattern that makes every sample a valley or a peak (rows4: a lower / upper corner) of one edge type, org on the other rail:
    every valley has org - dbk = +max, every peak -max.  A thread of the 8-bit statistics kernel walks rows 16 apart, so all 16 samples it sees
    fall in one class at the extreme difference."""
    mx = (1 << bd) - 1
    out_o, out_d = [], []
    for hh, ww in _shapes(w, h):
        ys, xs = np.mgrid[0:hh, 0:ww]
        hi = {"rows": ys & 1, "cols": xs & 1, "diag135": ((xs + ys) >> 1) & 1, "diag45": ((xs - ys) >> 1) & 1, "rows4": (ys >> 1) & 1, "cols4": (xs >> 1) & 1}[pattern]
        out_d.append(hi * mx); out_o.append((1 - hi) * mx)
    return _frame(out_o, bd), _frame(out_d, bd)


def _bands(rng, w, h, bd, bands, diffs):
    """dbk uniform inside the given bands (a band per 4-column stripe... per sample at random), org = dbk + the band's difference."""
    bw = 1 << (bd - 5)
    out_o, out_d = [], []
    for hh, ww in _shapes(w, h):
        pick = rng.integers(0, len(bands), (hh, ww))
        d = np.asarray(bands)[pick] * bw + rng.integers(0, bw, (hh, ww))
        o = np.clip(d + np.asarray(diffs)[pick] * (bw // 8) + rng.integers(-1, 2, (hh, ww)), 0, (1 << bd) - 1)
        out_d.append(d); out_o.append(o)
    return _frame(out_o, bd), _frame(out_d, bd)


def _eo_target(rng, w, h, bd, types, strength=3, amp=24):
    """dbk: noise of amplitude `amp` around mid grey; org = dbk + strength on the valleys, - strength on the peaks of the edge type wanted in each CTU
    (types[ctu % len]; 4 = band offset: a difference per band), so that each CTU prefers another SAO type."""
    s = 1 << (bd - 8)
    out_o, out_d = [], []
    for comp, (hh, ww) in enumerate(_shapes(w, h)):
        ctb = 64 if comp == 0 else 32
        d = (1 << (bd - 1)) + rng.integers(-amp * s, amp * s + 1, (hh, ww))
        ys, xs = np.mgrid[0:hh, 0:ww]
        want = np.asarray(types)[((ys // ctb) * ((w + 63) // 64) + xs // ctb + (2 if comp else 0)) % len(types)]
        o = d.copy()
        for t in range(4):
            cls = fs._edge_class(d, t)
            o = np.where(want == t, d + strength * s * ((cls == 0) * 1 + (cls == 1) * 1 - (cls == 3) * 1 - (cls == 4) * 1), o)
        band = d >> (bd - 5)
        o = np.where(want == 4, d + strength * s * np.where(band % 2 == 0, 2, -2), o)
        out_d.append(d); out_o.append(np.clip(o, 0, (1 << bd) - 1))
    return _frame(out_o, bd), _frame(out_d, bd)


def sao_cases():
    """Yields the SAO cases: dict(name, group, w, h, qp, bit_depth, tiles, lf_across_tiles, n_frames, org [n, w * h * 3 / 2], dbk)."""
    k = 0
    for bd in (8, 10):
        mx, s = (1 << bd) - 1, 1 << (bd - 8)

        def rng_of():
            nonlocal k
            k += 1
            return np.random.default_rng([SEED, 2, k])
        for pattern in ("rows", "cols", "diag135", "diag45", "rows4", "cols4"):
            rng_of()
            o, d = _packed_max(pattern, 136, 72, bd)
            yield _sao_case("packed-max/%s-b%d" % (pattern, bd), "packed-max", 136, 72, 51 if pattern == "rows" else 37, bd, o, d)
        for name, bands, diffs in (("one", [12], [20]), ("four", [10, 11, 12, 13], [40, -40, 6, -100]), ("top", [28, 29, 30, 31], [-40, 40, -100, 100]),
                                   ("bottom", [0, 1, 2, 3], [100, -3, 40, -40]), ("wrap", [30, 31, 0, 1], [-60, 60, 60, -2]), ("five", [3, 4, 5, 6, 7], [9, 9, -9, 9, 30])):
            o, d = _bands(rng_of(), 136, 72, bd, bands, diffs)
            yield _sao_case("bands/%s-b%d" % (name, bd), "bands", 136, 72, 22 if name != "top" else 37, bd, o, d)
        # clip: dbk within the offset range of a rail, the original beyond it
        rng = rng_of()
        m = fs.max_offset(bd)
        o_pl, d_pl = [], []
        for hh, ww in _shapes(200, 136):
            low = (np.mgrid[0:hh, 0:ww][1] // 16) % 2 == 0
            d = np.where(low, rng.integers(0, m + 1, (hh, ww)), mx - rng.integers(0, m + 1, (hh, ww)))
            o = np.where(low, np.maximum(d - rng.integers(m // 2, 2 * m, (hh, ww)), 0), np.minimum(d + rng.integers(m // 2, 2 * m, (hh, ww)), mx))
            d_pl.append(d); o_pl.append(o)
        yield _sao_case("clip/rails-b%d" % bd, "clip", 200, 136, 22, bd, _frame(o_pl, bd), _frame(d_pl, bd))
        o_pl, d_pl = [], []
        for hh, ww in _shapes(136, 72):                                       # valleys at 0 .. m that want a negative... peaks near 0 pushed below it
            ys, xs = np.mgrid[0:hh, 0:ww]
            pk = ((xs + ys) & 1) == 1
            d = np.where(pk, rng.integers(2, m + 1, (hh, ww)), 0)
            d = np.where(ys >= hh // 2, mx - d, d)
            o = np.where(ys >= hh // 2, mx, 0) + 0 * d
            d_pl.append(d); o_pl.append(o)
        yield _sao_case("clip/peaks-b%d" % bd, "clip", 136, 72, 22, bd, _frame(o_pl, bd), _frame(d_pl, bd))
        # rounding: a flat picture (one band, edge class 2 only), diff / count = j + 0.5 with either sign, another j per CTU; and a picture whose
        # margins (not counted by the statistics) pull the other way
        rng = rng_of()
        o_pl, d_pl = [], []
        for comp, (hh, ww) in enumerate(_shapes(264, 136)):
            ctb = 64 if comp == 0 else 32
            ys, xs = np.mgrid[0:hh, 0:ww]
            j = ((ys // ctb) * 5 + xs // ctb) % 10 - 5                        # -5 .. 4  ->  means -4.5 .. 4.5
            d = np.full((hh, ww), 100 * s)
            o = d + j + ((xs + ys) & 1)
            d_pl.append(d); o_pl.append(o)
        yield _sao_case("rounding/half-b%d" % bd, "rounding", 264, 136, 0, bd, _frame(o_pl, bd), _frame(d_pl, bd))
        o_pl, d_pl = [], []
        for comp, (hh, ww) in enumerate(_shapes(200, 136)):
            ctb, mr, mb = (64, 5, 4) if comp == 0 else (32, 3, 2)
            ys, xs = np.mgrid[0:hh, 0:ww]
            margin = (xs % ctb >= ctb - mr) | (ys % ctb >= ctb - mb)
            d = 128 * s + rng.integers(-6 * s, 6 * s + 1, (hh, ww))
            o = np.where(margin, 0, d + 3)
            d_pl.append(d); o_pl.append(o)
        yield _sao_case("rounding/margins-b%d" % bd, "rounding", 200, 136, 0, bd, _frame(o_pl, bd), _frame(d_pl, bd))
        # merge: identical CTUs, CTUs with org == dbk, a checkerboard of the two; with and without tiles
        rng = rng_of()
        o1, d1 = _eo_target(rng, 64, 64, bd, [0], strength=4)
        for name, w, h, tiles, lf in (("same", 200, 136, (1, 1), True), ("checker", 264, 136, (1, 1), True), ("tiles-lf0", 520, 200, (2, 2), False), ("tiles-lf1", 520, 200, (2, 2), True)):
            o_pl, d_pl = [], []
            for comp, (hh, ww) in enumerate(_shapes(w, h)):
                ctb = 64 if comp == 0 else 32
                src_o, src_d = fs.split_planes(o1, 64, 64)[comp], fs.split_planes(d1, 64, 64)[comp]
                reps = ((hh + ctb - 1) // ctb, (ww + ctb - 1) // ctb)
                d = np.tile(src_d, reps)[:hh, :ww]; o = np.tile(src_o, reps)[:hh, :ww]
                if name != "same":
                    ys, xs = np.mgrid[0:hh, 0:ww]
                    same = ((ys // ctb + xs // ctb) % (2 if name == "checker" else 3)) == 1
                    o = np.where(same, d, o)
                d_pl.append(d); o_pl.append(o)
            yield _sao_case("merge/%s-b%d" % (name, bd), "merge", w, h, 32, bd, _frame(o_pl, bd), _frame(d_pl, bd), tiles=tiles, lf=lf)
        rng = rng_of()
        n = 200 * 136 * 3 // 2
        yield _sao_case("noise/uniform-b%d" % bd, "noise", 200, 136, 22, bd, rng.integers(0, mx + 1, n).astype(np.uint16), rng.integers(0, mx + 1, n).astype(np.uint16))
        for i, (w, h, tiles, lf) in enumerate(((8, 8, (1, 1), True), (72, 8, (1, 1), True), (8, 136, (1, 1), True), (200, 136, (1, 1), True), (520, 200, (2, 2), False),
                                               (520, 200, (2, 2), True), (1032, 136, ([5, 4, 8], [1, 2]), False))):
            qp = (0, 22, 37, 51)[i % 4]
            o, d = _eo_target(rng_of(), w, h, bd, [0, 1, 2, 3, 4], strength=3 + 3 * (qp >= 37) + 20 * (qp == 51))
            yield _sao_case("sizes/%dx%d-q%d-lf%d-b%d" % (w, h, qp, lf, bd), "sizes", w, h, qp, bd, o, d, tiles=tiles, lf=lf)
        rng = rng_of()
        pairs = [_eo_target(rng, 200, 72, bd, t, strength=4) for t in ([4, 0, 1], [2, 3, 4], [1, 4, 2])]
        yield _sao_case("sizes/batch3-b%d" % bd, "sizes", 200, 72, 27, bd, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
