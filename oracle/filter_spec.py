"""oracle/filter_spec.py -- TEST INFRASTRUCTURE, not product code.

An independent numpy restatement of the two in-loop filters, written from the text of H.265 clauses 8.7.2 (deblocking) and 8.7.3 (SAO) for the
configuration the product supports: intra pictures (bS 2 on every transform-block edge of the 8x8 luma grid), one slice, constant QP,
slice_beta_offset_div2 / slice_tc_offset_div2, no PCM / bypass, 4:2:0, 8 and 10 bits, loop_filter_across_tiles_enabled_flag 0 or 1.

It is deliberately a THIRD implementation next to csrc/deblock_kernel.hip / csrc/sao_kernel.hip and oracle/hm_deblock.c / oracle/hm_sao.c: plain
int64 arithmetic on whole planes, no packing, every edge of a pass gathered into one (segments, 4 lines, 8 samples) array.  Besides the pictures it
returns a TALLY of what happened, so that a corpus can be held to "this branch was taken at least N times" (tests/test_filters_adversarial.py).

The keyword switches named in DEFECTS plant one deliberate defect each; they exist so that the tests can show that the corpus tells the
restatement from a wrong one.  They default to off.  The rate-distortion choice of the SAO parameters is NOT restated here.
Nothing here is imported by the product package.
"""
import numpy as np

DEFECTS = ("le_10tc", "own_decision_lines12", "no_clipbd", "filter_picture_edge", "filter_4x4_grid")        # deblock(...)
SAO_DEFECTS = ("no_margins", "swap_diagonals")                                                             # sao_stats(...), sao_apply(...)

# Table 8-12: beta' (Q 0..51) and tC' (Q 0..53)
BETA_PRIME = [0] * 16 + list(range(6, 19)) + list(range(20, 66, 2))
TC_PRIME = [0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24]
assert len(BETA_PRIME) == 52 and len(TC_PRIME) == 54
# Table 8-10 (ChromaArrayType 1): QpC as a function of qPi
QPC_30_43 = [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37]

LUMA_BINS = ("not_edge", "d_ge_beta", "strong", "normal_00", "normal_01", "normal_10", "normal_11", "mixed_lines", "clip_tc", "clip_2tc", "clip_tc_half")
BIN_NAMES = ("off-grid", "not_edge", "d_ge_beta", "strong", "normal_00", "normal_01", "normal_10", "normal_11")         # codes of the per-segment maps


def qpc_of(qpi):
    return qpi if qpi < 30 else (QPC_30_43[qpi - 30] if qpi <= 43 else qpi - 6)


def thresholds(qp, bit_depth, lf_offsets):
    """(beta, tC of luma, tC of chroma) for bS 2, QpY = qp on both sides, cQpPicOffset 0 (8.7.2.5.3, 8.7.2.5.5)."""
    scale = 1 << (bit_depth - 8)
    beta = BETA_PRIME[min(51, max(0, qp + 2 * lf_offsets[0]))] * scale
    tc = TC_PRIME[min(53, max(0, qp + 2 + 2 * lf_offsets[1]))] * scale
    tc_c = TC_PRIME[min(53, max(0, qpc_of(qp) + 2 + 2 * lf_offsets[1]))] * scale
    return beta, tc, tc_c


def tile_starts(tiles, w, h):
    """(first CTU column of every tile column, first CTU row of every tile row) for tiles = (columns, rows) uniformly spaced (6.5.1) or
    ([widths], [heights]) in CTUs."""
    cx, cy = (w + 63) // 64, (h + 63) // 64
    if isinstance(tiles[0], (int, np.integer)):
        return [(i * cx) // int(tiles[0]) for i in range(int(tiles[0]))], [(i * cy) // int(tiles[1]) for i in range(int(tiles[1]))]
    return [int(sum(tiles[0][:i])) for i in range(len(tiles[0]))], [int(sum(tiles[1][:i])) for i in range(len(tiles[1]))]


def split_planes(frame, w, h):
    f = np.asarray(frame).astype(np.int64)
    return [f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)]


def join_planes(planes):
    return np.concatenate([p.ravel() for p in planes])


# ---- transform-block grid -----------------------------------------------------------------------------------------------------------------
_Y4, _X4 = np.mgrid[0:16, 0:16]
Z_OF = sum((((_X4 >> b) & 1) << (2 * b)) | (((_Y4 >> b) & 1) << (2 * b + 1)) for b in range(4))          # 6.5.2: z-scan order of the 4x4 blocks of a CTB


def tu_size_map(depth, tr_idx, w, h):
    """Transform-block size at every 4x4 luma block of the picture, [h / 4, w / 4], from the z-ordered depth / tr_idx of every CTU."""
    cx, cy = (w + 63) // 64, (h + 63) // 64
    size = 64 >> (np.asarray(depth).astype(np.int64) + np.asarray(tr_idx).astype(np.int64)).reshape(cy * cx, 256)
    full = size[:, Z_OF].reshape(cy, cx, 16, 16).transpose(0, 2, 1, 3).reshape(cy * 16, cx * 16)
    return full[:h // 4, :w // 4]


def edge_maps(tu, w, h, tiles, lf_across_tiles, picture_edge=False):
    """filterEdgeFlag of the left / top edge of every 4x4 luma block (8.7.2.3 transform-block edges; 8.7.2.2: not at the picture border, not at
    a tile border when the filter may not cross tiles)."""
    ys, xs = np.mgrid[0:h // 4, 0:w // 4] * 4
    ver, hor = (xs % tu) == 0, (ys % tu) == 0
    if not picture_edge:
        ver &= xs > 0
        hor &= ys > 0
    if not lf_across_tiles:
        cs, rs = tile_starts(tiles, w, h)
        ver &= ~np.isin(xs, [64 * c for c in cs if c > 0])
        hor &= ~np.isin(ys, [64 * r for r in rs if r > 0])
    return ver, hor


# ---- deblocking (8.7.2) ---------------------------------------------------------------------------------------------------------------------
def _clip3(lo, hi, v):
    return np.minimum(np.maximum(v, lo), hi)


def _luma_edges(P, flags, xs, beta, tc, mx, T, bins, sw):
    """Filter the vertical edges at columns xs of P [H, W] in place (8.7.2.5.3, 8.7.2.5.4, 8.7.2.5.6, 8.7.2.5.7).  flags [H / 4, W / 4]."""
    if len(xs) == 0:
        return
    H = P.shape[0]
    idx = np.asarray(xs)[:, None] + np.arange(-4, 4)[None, :]
    S = P[:, idx].reshape(H // 4, 4, len(xs), 8).transpose(0, 2, 1, 3)                   # [segment row, edge, line k, p3 p2 p1 p0 q0 q1 q2 q3]
    p = [S[..., 3 - i] for i in range(4)]
    q = [S[..., 4 + i] for i in range(4)]
    edge = flags[:, np.asarray(xs) // 4]                                                  # [segment row, edge]
    dp, dq = np.abs(p[2] - 2 * p[1] + p[0]), np.abs(q[2] - 2 * q[1] + q[0])               # per line
    # decisions from lines 0 and 3, then spread over the four lines ("k = 0..3")
    def decide(k0, k3):
        d = dp[..., k0] + dq[..., k0] + dp[..., k3] + dq[..., k3]
        def dsam(k):
            return (2 * (dp[..., k] + dq[..., k]) < (beta >> 2)) & (np.abs(p[3][..., k] - p[0][..., k]) + np.abs(q[0][..., k] - q[3][..., k]) < (beta >> 3)) & \
                   (np.abs(p[0][..., k] - q[0][..., k]) < ((5 * tc + 1) >> 1))
        de = np.where(d < beta, np.where(dsam(k0) & dsam(k3), 2, 1), 0)
        side = (beta + (beta >> 1)) >> 3
        return de, (dp[..., k0] + dp[..., k3]) < side, (dq[..., k0] + dq[..., k3]) < side
    de, dep, deq = decide(0, 3)
    de = np.where(edge, de, -1)
    DE, DEP, DEQ = [np.repeat(a[..., None], 4, axis=-1) for a in (de, dep, deq)]
    if sw.get("own_decision_lines12"):
        for k in (1, 2):
            a, b, c = decide(k, k)
            DE[..., k], DEP[..., k], DEQ[..., k] = np.where(edge, a, -1), b, c
    strong, normal = DE == 2, DE == 1
    new = S.copy()
    # strong filter
    cand = {2: (p[2] + 2 * p[1] + 2 * p[0] + 2 * q[0] + q[1] + 4) >> 3, 1: (p[2] + p[1] + p[0] + q[0] + 2) >> 2, 0: (2 * p[3] + 3 * p[2] + p[1] + p[0] + q[0] + 4) >> 3,
            3: (p[1] + 2 * p[0] + 2 * q[0] + 2 * q[1] + q[2] + 4) >> 3, 4: (p[0] + q[0] + q[1] + q[2] + 2) >> 2, 5: (p[0] + q[0] + q[1] + 3 * q[2] + 2 * q[3] + 4) >> 3}
    pos = {2: 3, 1: 2, 0: 1, 3: 4, 4: 5, 5: 6}                                            # candidate -> position in the line (p0' p1' p2' q0' q1' q2')
    clipped_2tc = np.zeros(S.shape[:3], bool)
    for k, v in cand.items():
        old = S[..., pos[k]]
        c = _clip3(old - 2 * tc, old + 2 * tc, v)
        clipped_2tc |= c != v
        new[..., pos[k]] = np.where(strong, c, new[..., pos[k]])
    # normal filter
    inter = 9 * (q[0] - p[0]) - 3 * (q[1] - p[1]) + 8
    delta0 = inter >> 4
    on = (np.abs(delta0) <= 10 * tc) if sw.get("le_10tc") else (np.abs(delta0) < 10 * tc)
    delta = _clip3(-tc, tc, delta0)
    dpr = (((p[2] + p[0] + 1) >> 1) - p[1] + delta) >> 1
    dqr = (((q[2] + q[0] + 1) >> 1) - q[1] - delta) >> 1
    dpc, dqc = _clip3(-(tc >> 1), tc >> 1, dpr), _clip3(-(tc >> 1), tc >> 1, dqr)
    use = normal & on
    raw = {3: (p[0] + delta, use), 4: (q[0] - delta, use), 2: (p[1] + dpc, use & DEP), 5: (q[1] + dqc, use & DEQ)}
    at0 = atmax = 0
    for k, (v, m) in raw.items():
        at0 += int((m & (v < 0)).sum())
        atmax += int((m & (v > mx)).sum())
        new[..., k] = np.where(m, v if sw.get("no_clipbd") else _clip3(0, mx, v), new[..., k])
    P[:, idx] = new.transpose(0, 2, 1, 3).reshape(H, len(xs), 8)
    # tally, per 4-line segment
    seg_n = de == 1
    T["not_edge"] += int((de == -1).sum()); T["d_ge_beta"] += int((de == 0).sum()); T["strong"] += int((de == 2).sum())
    for a in (0, 1):
        for b in (0, 1):
            T["normal_%d%d" % (a, b)] += int((seg_n & (dep == bool(a)) & (deq == bool(b))).sum())
    T["mixed_lines"] += int((seg_n & (on.any(-1) != on.all(-1))).sum())
    T["clip_tc"] += int((seg_n & (on & (delta != delta0)).any(-1)).sum())
    T["clip_2tc"] += int(((de == 2) & clipped_2tc.any(-1)).sum())
    T["clip_tc_half"] += int((seg_n & ((on & DEP & (dpc != dpr)) | (on & DEQ & (dqc != dqr))).any(-1)).sum())
    T["clipbd_0"] += at0; T["clipbd_max"] += atmax
    if seg_n.any():
        T["max_intermediate"] = max(T["max_intermediate"], int(np.abs(inter[seg_n]).max()))
    code = np.where(de == -1, 1, np.where(de == 0, 2, np.where(de == 2, 3, 4 + 2 * dep.astype(np.int64) + deq.astype(np.int64))))
    bins[:, np.asarray(xs) // 4] = code


def _chroma_edges(C, flags, tc, mx, T, sw):
    """Vertical edges of one chroma plane [H / 2, W / 2] in place (8.7.2.5.5, 8.7.2.5.8): edges on the 8-sample chroma grid, bS 2."""
    ch, cw = C.shape
    xs = np.arange(8, cw, 8)
    if len(xs) == 0:
        return
    idx = xs[:, None] + np.arange(-2, 2)[None, :]
    S = C[:, idx]                                                                        # [row, edge, p1 p0 q0 q1]
    p1, p0, q0, q1 = [S[..., i] for i in range(4)]
    edge = flags[np.arange(ch) // 2][:, xs // 2]                                        # chroma row r = luma row 2r = 4x4 block row r // 2; chroma x = luma 2x = block x // 2
    raw = (((q0 - p0) << 2) + p1 - q1 + 4) >> 3
    delta = _clip3(-tc, tc, raw)
    a, b = p0 + delta, q0 - delta
    T["c_clipbd_0"] += int((edge & (a < 0)).sum() + (edge & (b < 0)).sum()); T["c_clipbd_max"] += int((edge & (a > mx)).sum() + (edge & (b > mx)).sum())
    if not sw.get("no_clipbd"):
        a, b = _clip3(0, mx, a), _clip3(0, mx, b)
    S = S.copy()
    S[..., 1] = np.where(edge, a, p0); S[..., 2] = np.where(edge, b, q0)
    C[:, idx] = S
    unit = edge.reshape(ch // 2, 2, len(xs))[:, 0]                                       # a unit: the two chroma lines of one 4x4 luma block
    T["chroma_filtered"] += int(unit.sum())
    T["chroma_clipped"] += int((unit & (edge & (delta != raw)).reshape(ch // 2, 2, len(xs)).any(1)).sum())


def new_tally():
    t = {d: dict.fromkeys(LUMA_BINS + ("clipbd_0", "clipbd_max", "max_intermediate"), 0) for d in ("ver", "hor")}
    t["chroma"] = dict.fromkeys(("chroma_filtered", "chroma_clipped", "c_clipbd_0", "c_clipbd_max"), 0)
    return t


def add_tally(total, t):
    for d in total:
        for k in total[d]:
            total[d][k] = max(total[d][k], t[d][k]) if k == "max_intermediate" else total[d][k] + t[d][k]


def deblock(planes, w, h, qp, depth, tr_idx, bit_depth=8, lf_offsets=(0, 0), tiles=(1, 1), lf_across_tiles=True, **defects):
    """One picture [w * h * 3 / 2] (Y, Cb, Cr) -> (filtered picture int64 [w * h * 3 / 2], tally).  depth / tr_idx: [ctus, 256] in z-scan order.
    tally: {"ver" / "hor": {bin: segments, "clipbd_0" / "clipbd_max": samples, "max_intermediate": largest abs(9 * (q0 - p0) - 3 * (q1 - p1) + 8) of a
    segment that takes the normal filter}, "chroma": {...}, "bins": {"ver" / "hor": [h / 4, w / 4] codes into BIN_NAMES of the segment at the left /
    top edge of every 4x4 block}}.  All vertical edges of the picture first, then all horizontal edges on the result (8.7.2)."""
    assert set(defects) <= set(DEFECTS), defects
    beta, tc, tc_c = thresholds(qp, bit_depth, lf_offsets)
    mx = (1 << bit_depth) - 1
    Y, U, V = split_planes(planes, w, h)
    pe = bool(defects.get("filter_picture_edge"))
    tu = tu_size_map(depth, tr_idx, w, h)
    ver, hor = edge_maps(tu, w, h, tiles, lf_across_tiles, picture_edge=pe)
    ver_c, hor_c = edge_maps(tu, w, h, tiles, lf_across_tiles)
    T = new_tally()
    T["bins"] = {}
    for name, flags, flags_c in (("ver", ver, ver_c), ("hor", hor, hor_c)):
        tr = name == "hor"                                                               # horizontal edges: the same code on the transposed plane
        P = np.ascontiguousarray(Y.T if tr else Y)
        F = np.ascontiguousarray(flags.T if tr else flags)
        B = np.zeros(F.shape, np.int8)
        if pe:                                                                           # defect: the edge at the picture border filtered against a replicated column
            P, F, B = np.pad(P, ((0, 0), (8, 0)), mode="edge"), np.pad(F, ((0, 0), (2, 0))), np.pad(B, ((0, 0), (2, 0)))
            F[:, 2] = np.ascontiguousarray(flags.T if tr else flags)[:, 0]
        for phase in ((0, 4) if defects.get("filter_4x4_grid") else (0,)):                # defect: transform edges off the 8x8 grid filtered too
            xs = [x for x in range(4 if phase else 8, P.shape[1], 8) if x + 4 <= P.shape[1]]
            _luma_edges(P, F, xs, beta, tc, mx, T[name], B, defects)
        if pe:
            P, B = P[:, 8:], B[:, 2:]
        Y = np.ascontiguousarray(P.T if tr else P)
        T["bins"][name] = np.ascontiguousarray(B.T if tr else B)
        planes_c = []
        for C in (U, V):
            Cp = np.ascontiguousarray(C.T if tr else C)
            _chroma_edges(Cp, np.ascontiguousarray(flags_c.T if tr else flags_c), tc_c, mx, T["chroma"], defects)
            planes_c.append(np.ascontiguousarray(Cp.T if tr else Cp))
        U, V = planes_c
    return join_planes([Y, U, V]), T


def describe_sample(tally, plane, y, x):
    """Which segments can have written sample (y, x) of plane 0 / 1 / 2: the bins of the nearest vertical and horizontal edge of the 8x8 grid (for a
    chroma plane: of the luma block the sample's edge belongs to)."""
    s = 1 if plane == 0 else 2
    ly, lx = y * s, x * s
    g = 8 * s
    ex, ey = ((lx + g // 2) // g) * g, ((ly + g // 2) // g) * g
    out = []
    for name, (by, bx) in (("ver", (ly // 4, ex // 4)), ("hor", (ey // 4, lx // 4))):
        B = tally["bins"][name]
        if by < B.shape[0] and bx < B.shape[1]:
            out.append("%s edge at luma (%d, %d): %s" % (name, by * 4, bx * 4, BIN_NAMES[int(B[by, bx])]))
    return "; ".join(out)


# ---- SAO (8.7.3) ----------------------------------------------------------------------------------------------------------------------------
EO_0, EO_90, EO_135, EO_45, BO = range(5)
MODE_OFF, MODE_NEW, MODE_MERGE = range(3)
# SaoEoClass -> (hPos, vPos) of the two neighbours (Table 8-13)
EO_NEIGHBOURS = {EO_0: ((-1, 0), (1, 0)), EO_90: ((0, -1), (0, 1)), EO_135: ((-1, -1), (1, 1)), EO_45: ((1, -1), (-1, 1))}


def max_offset(bit_depth):
    return (1 << (min(bit_depth, 10) - 5)) - 1


def _neighbours(t, swap_diagonals):
    if swap_diagonals and t in (EO_135, EO_45):
        t = EO_135 + EO_45 - t
    return EO_NEIGHBOURS[t]


def _shifted(P, dx, dy):
    """P[y + dy, x + dx] with the border replicated (the caller masks samples whose neighbour does not exist)."""
    h, w = P.shape
    ys, xs = np.clip(np.arange(h) + dy, 0, h - 1), np.clip(np.arange(w) + dx, 0, w - 1)
    return P[ys][:, xs]


def _edge_class(P, t, swap_diagonals=False):
    """2 + Sign(rec - a) + Sign(rec - b) for every sample: 0 valley, 1 / 3 corners, 4 peak, 2 none."""
    (ax, ay), (bx, by) = _neighbours(t, swap_diagonals)
    return 2 + np.sign(P - _shifted(P, ax, ay)) + np.sign(P - _shifted(P, bx, by))


def _tile_ids(n, starts, ctb):
    ctu = np.arange(n) // ctb
    return np.searchsorted(np.asarray(starts), ctu, side="right") - 1


def _exists(shape, ctb, dx, dy, tiles_xy, lf_across_tiles, tiles_on_far_side):
    """Does the neighbour (x + dx, y + dy) of every sample exist: inside the picture and, when the filter may not cross tiles, in the same tile.
    tiles_on_far_side False: the tile rule is applied to left / upper neighbours only (the encoder's statistics)."""
    h, w = shape
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    ok = (xs + dx >= 0) & (xs + dx < w) & (ys + dy >= 0) & (ys + dy < h)
    if not lf_across_tiles:
        tx, ty = _tile_ids(w, tiles_xy[0], ctb), _tile_ids(h, tiles_xy[1], ctb)
        if dx < 0 or (dx > 0 and tiles_on_far_side):
            ok &= (tx[np.clip(np.arange(w) + dx, 0, w - 1)] == tx)[None, :]
        if dy < 0 or (dy > 0 and tiles_on_far_side):
            ok &= (ty[np.clip(np.arange(h) + dy, 0, h - 1)] == ty)[:, None]
    return ok


def sao_stats(org, dbk, w, h, bit_depth=8, tiles=(1, 1), lf_across_tiles=True, no_margins=False, swap_diagonals=False):
    """The encoder's statistics: (sum of org - dbk, count) per (CTU, component, type, class), int64 [ctus, 3, 5, 32].  A sample counts when the
    neighbours its class needs exist (picture border; tile border towards the left / top when the filter may not cross tiles; right / below only
    the picture counts) and it lies outside the margin the deblocking of the next CTU can still change: the last 5 columns / 4 rows (luma),
    3 columns / 2 rows (chroma) of a CTU that has a CTU to its right / below it in the picture."""
    cx, cy = (w + 63) // 64, (h + 63) // 64
    diff, count = np.zeros((cx * cy, 3, 5, 32), np.int64), np.zeros((cx * cy, 3, 5, 32), np.int64)
    starts = tile_starts(tiles, w, h)
    for comp, (O, D) in enumerate(zip(split_planes(org, w, h), split_planes(dbk, w, h))):
        ctb = 64 if comp == 0 else 32
        ph, pw = D.shape
        ys, xs = np.arange(ph)[:, None], np.arange(pw)[None, :]
        keep = np.ones(D.shape, bool)
        if not no_margins:
            mr, mb = (5, 4) if comp == 0 else (3, 2)
            has_right, has_below = (xs // ctb + 1) * ctb < pw, (ys // ctb + 1) * ctb < ph
            keep = ~(has_right & (xs % ctb >= ctb - mr)) & ~(has_below & (ys % ctb >= ctb - mb))
        ctu = (ys // ctb) * cx + xs // ctb
        e = O - D
        for t in range(5):
            if t == BO:
                cls, ok = D >> (bit_depth - 5), keep
            else:
                cls, ok = _edge_class(D, t, swap_diagonals), keep.copy()
                for dx, dy in _neighbours(t, swap_diagonals):
                    ok &= _exists(D.shape, ctb, dx, dy, starts, lf_across_tiles, False)
            key = (ctu * 32 + cls)[ok]
            count[:, comp, t, :] = np.bincount(key, minlength=cx * cy * 32).reshape(-1, 32)
            pos = np.bincount(key, weights=np.maximum(e[ok], 0).astype(np.float64), minlength=cx * cy * 32)      # exact: sums stay far below 2^53
            neg = np.bincount(key, weights=np.maximum(-e[ok], 0).astype(np.float64), minlength=cx * cy * 32)
            diff[:, comp, t, :] = (pos.astype(np.int64) - neg.astype(np.int64)).reshape(-1, 32)
    return diff, count


def resolve_params(params, w, h):
    """Merge candidates replaced by what they copy: [ctus, 3] records whose mode is off or new."""
    cx = (w + 63) // 64
    out = np.array(params, copy=True).reshape(-1, 3)
    for a in range(out.shape[0]):
        for c in range(3):
            if out[a, c]["mode"] == MODE_MERGE:
                out[a, c] = out[a - 1, c] if out[a, c]["type"] == 0 else out[a - cx, c]
    return out


def sao_apply(dbk, params, w, h, bit_depth=8, tiles=(1, 1), lf_across_tiles=True, swap_diagonals=False):
    """Clause 8.7.3 on decided parameters [ctus, 3] (mode, type, aux = band position, offset[32]: edge classes 0, 1, 3, 4 = the four coded offsets in
    order; band offsets at their band) -> (picture int64, tally {"clip_0", "clip_max", "changed": [5 types, 32 classes]})."""
    P = resolve_params(params, w, h)
    cx = (w + 63) // 64
    mx = (1 << bit_depth) - 1
    starts = tile_starts(tiles, w, h)
    tally = {"clip_0": 0, "clip_max": 0, "changed": np.zeros((5, 32), np.int64)}
    out = []
    for comp, D in enumerate(split_planes(dbk, w, h)):
        ctb = 64 if comp == 0 else 32
        R = D.copy()
        cls_of, ok_of = {}, {}
        for a in range(P.shape[0]):
            prm = P[a, comp]
            if prm["mode"] == MODE_OFF:
                continue
            t = int(prm["type"])
            y0, x0 = (a // cx) * ctb, (a % cx) * ctb
            win = (slice(y0, min(y0 + ctb, D.shape[0])), slice(x0, min(x0 + ctb, D.shape[1])))
            if t == BO:
                # bandTable[(k + sao_band_position) & 31] = k + 1; SaoOffsetVal[k + 1] = offset of that band
                table = np.zeros(32, np.int64)
                val = np.zeros(5, np.int64)
                for k in range(4):
                    band = (k + int(prm["aux"])) & 31
                    table[band] = k + 1
                    val[k + 1] = int(prm["offset"][band])
                cls = D[win] >> (bit_depth - 5)
                add, ok = val[table[cls]], np.ones(cls.shape, bool)
            else:
                if t not in cls_of:
                    cls_of[t] = _edge_class(D, t, swap_diagonals)
                    ok = np.ones(D.shape, bool)
                    for dx, dy in _neighbours(t, swap_diagonals):
                        ok &= _exists(D.shape, ctb, dx, dy, starts, lf_across_tiles, True)
                    ok_of[t] = ok
                # edgeIdx = 2 + Sign + Sign; edgeIdx 0, 1, 2 -> (edgeIdx == 2) ? 0 : edgeIdx + 1; SaoOffsetVal[1..4] = the four coded offsets
                cls, ok = cls_of[t][win], ok_of[t][win]
                idx = np.where(cls == 2, 0, np.where(cls < 2, cls + 1, cls))
                val = np.array([0, prm["offset"][0], prm["offset"][1], prm["offset"][3], prm["offset"][4]], np.int64)
                add = val[idx]
            v = D[win] + np.where(ok, add, 0)
            tally["clip_0"] += int((v < 0).sum()); tally["clip_max"] += int((v > mx).sum())
            v = _clip3(0, mx, v)
            np.add.at(tally["changed"][t], cls[v != D[win]], 1)
            R[win] = v
        out.append(R)
    return join_planes(out), tally


def round_offset(diff, count, bit_depth):
    """The encoder's first guess of an offset: diff / count rounded half away from zero (at 10 bits through a truncation of 4 * diff / count, the
    way the reference scales its statistics first), clipped to the range of sao_offset_abs."""
    if count == 0:
        return 0
    s = 1 if diff >= 0 else -1
    if bit_depth == 8:
        q = s * ((2 * abs(diff) + count) // (2 * count))
    else:
        r = 1 << (bit_depth - 8)
        x = (abs(diff) * r) // count                       # truncation towards zero of the scaled mean
        q = s * ((x + (r >> 1)) // r)
    m = max_offset(bit_depth)
    return max(-m, min(m, q))


def offset_violations(params, diff, count, bit_depth):
    """Where decided parameters [ctus, 3] contradict statistics [ctus, 3, 5, 32]: for every component decided "new", edge classes 0 / 1 >= 0 and 3 / 4 <= 0,
    class 2 and bands outside the four signalled ones 0, abs(offset) <= max, band position <= 28, and every offset equal to the rounded, clipped
    diff / count of its class or between it and 0 (the encoder's rate-distortion step only walks an offset towards 0).  -> list of strings."""
    bad = []
    m = max_offset(bit_depth)
    params = np.asarray(params).reshape(-1, 3)
    for a in range(params.shape[0]):
        for c in range(3):
            prm = params[a, c]
            if prm["mode"] != MODE_NEW:
                continue
            t, aux = int(prm["type"]), int(prm["aux"])
            if t == BO and not 0 <= aux <= 28:
                bad.append("ctu %d comp %d: band position %d" % (a, c, aux))
            for k in range(32):
                o = int(prm["offset"][k])
                live = (k in (0, 1, 3, 4)) if t != BO else (aux <= k < aux + 4)
                r = round_offset(int(diff[a, c, t, k]), int(count[a, c, t, k]), bit_depth) if live else 0
                if t != BO and ((k in (0, 1) and r < 0) or (k in (3, 4) and r > 0)):
                    r = 0
                if abs(o) > m or not (min(0, r) <= o <= max(0, r)):
                    bad.append("ctu %d comp %d type %d class %d: offset %d, statistics give %d (diff %d / count %d)" % (a, c, t, k, o, r, diff[a, c, t, k], count[a, c, t, k]))
    return bad
