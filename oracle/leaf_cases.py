"""oracle/leaf_cases.py -- TEST INFRASTRUCTURE: the shared case lists of tests/test_rd_leaf.py (CPU) and tests/test_rd_leaf_gpu.py (device).

Deterministic and seeded: both test files, and the child process that runs the device leaves (oracle/leaf_device.py), build the same lists from here.

The residual-range contract.  Residual blocks stay in [-M, M] with M = 2^BD - 1: a residual is original minus prediction, both samples of BD bits.  That range is the
decision kernel's CONTRACT, not an accident of the corpus: fwd_transform_n (csrc/rd_kernel.hip) stores its first-stage intermediate and the coefficients as int16
without a clip, which is exact because the largest L1 norm of a row of the transform matrices is 64 N (the DC row), so that a first-stage value is at most
(64 N M + a1) >> (log2 N + BD - 9) = 2^15 - 2^(15 - BD) (tests/test_rd_leaf.py asserts the bound and the corpus).  A block outside the range is outside what the kernel
promises; the corpus reaches the range's corners (all +M, all -M, the sign pattern of every basis function) and never leaves it.

A CALL is one parameter set (entry, component, size, QP, mode, transform skip, cbf context, tools) with a batch of blocks and, per block, the context bytes the coder
starts from; hm_oracle_tu_leaf and hevcdl_leaf_tu_run both work on a call.  Parameter sets are not the full product of every list (that would be hundreds of
thousands of codings) but a rotation in which every QP meets every mode, both transform-skip values, every cbf context and every context set.
"""
import math
import os
from collections import namedtuple

import numpy as np

QPS = (0, 1, 5, 6, 22, 32, 37, 51)
DIR_MODES = (0, 1, 10, 26, 34)             # planar, DC, horizontal (vertical scan), vertical (horizontal scan), 34 (diagonal): the three scan types at 4x4 and 8x8
TOOLS_REFERENCE = 0x7f
TOOL_RDOQ, TOOL_RDOQTS, TOOL_SIGN_HIDE, TOOL_STRONG_INTRA = 0x01, 0x02, 0x10, 0x20
# the tool sets beyond the reference's that the builds reading the switches at run time (_tools, _bd10) are run with
TOOL_SETS_RT = (TOOLS_REFERENCE & ~TOOL_RDOQ, TOOLS_REFERENCE & ~TOOL_RDOQTS, TOOLS_REFERENCE & ~TOOL_SIGN_HIDE, TOOLS_REFERENCE & ~(TOOL_RDOQ | TOOL_SIGN_HIDE))
BUILDS = {"": (8, False), "_bd10": (10, True), "_wide": (8, False), "_tools": (8, True)}          # symbol suffix -> (bit depth, reads the tool switches at run time)
GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
STAGE_FIXTURES = ("stage_a64_q32", "stage_b128_q27")
SEEDED = (4, 4, 8)                         # seeded residual blocks per list: uniform, sparse, small.  The only counts to thin when a test runs long; the structured cases stay

# ---- the standard's tables (Rec. ITU-T H.265: 8.6.4.2 transform matrices, 9.3.2.2 context initialisation for I slices, 8.6.1 chroma QP mapping) ----
DCT_MAG = (64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0)
DST4 = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], np.int64)
QUANT_SCALES = (26214, 23302, 20560, 18396, 16384, 14564)
INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)
NUM_CTX = 159
CTX_INIT = (
    139, 141, 157, 184, 184, 63,
    111, 141, 154, 154, 154, 94, 138, 182, 154, 154,
    153, 138, 138, 91, 171, 134, 141,
    111, 111, 125, 110, 110, 94, 124, 108, 124, 107, 125, 141, 179, 153, 125, 107, 125, 141, 179, 153, 125, 107, 125, 141, 179, 153, 125, 141,
    140, 139, 182, 182, 152, 136, 152, 136, 153, 136, 139, 111, 136, 139, 111, 111,
    110, 110, 124, 125, 140, 153, 125, 127, 140, 109, 111, 143, 127, 111, 79, 108, 123, 63, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154,
    110, 110, 124, 125, 140, 153, 125, 127, 140, 109, 111, 143, 127, 111, 79, 108, 123, 63, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154, 154,
    140, 92, 137, 138, 140, 152, 138, 139, 153, 74, 149, 92, 139, 107, 122, 152, 140, 179, 166, 182, 140, 227, 122, 197,
    138, 153, 136, 167, 152, 152, 139, 139)
assert len(CTX_INIT) == NUM_CTX


def transform_matrix(n, dst=False):
    """T_N[k][i] (int64): the DCT of size n as the sub-sampled 32-point matrix, or the 4x4 DST of intra luma."""
    if dst:
        assert n == 4
        return DST4.copy()
    t = np.zeros((n, n), np.int64)
    for k in range(n):
        for i in range(n):
            m = ((2 * i + 1) * k * (32 // n)) & 127           # the angle in units of pi / 64
            if m > 64:
                m = 128 - m
            t[k, i] = DCT_MAG[m] if m <= 32 else -DCT_MAG[64 - m]
    return t


def chroma_qp(qp):
    """4:2:0 chroma QP of a luma QP (offsets 0)."""
    if qp < 30:
        return qp
    if qp >= 44:
        return qp - 6
    return (29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37)[qp - 30]


def rd_consts(qp, bd):
    """The lambda family of hevcdl_config_default_bd (csrc/hevcdl_api.hip) for the device leaves: (consts[12], sbh[2], chroma QP)."""
    lam = 0.57 * 1.0 * math.pow(2.0, (qp - 12) / 3.0)
    qpc = chroma_qp(qp)
    cw = math.pow(2.0, (qp - qpc) / 3.0)
    lam_c = lam / cw
    err, sbh = [], []
    for ch in range(2):
        q = (qpc if ch else qp) + 6 * (bd - 8)
        rem, per, dadj = q % 6, q // 6, 2 * (bd - 8)
        for l in range(4):
            s = float(1 << 15) * math.pow(2.0, -2.0 * (15 - bd - (l + 2)))
            err.append(s / QUANT_SCALES[rem] / QUANT_SCALES[rem] / (1 << dadj))
        inv = float(INV_QUANT_SCALES[rem])
        sbh.append(int(inv * inv * (1 << (2 * per)) / (lam_c if ch else lam) / 16 / (1 << dadj) + 0.5))
    return np.array([lam, math.sqrt(lam), cw, lam_c] + err, np.float64), np.array(sbh, np.int64), qpc


def quant_params(qp, comp, n, bd):
    """(qbits, quantiser scale) of a TU: TComTrQuant's iQBits and the scale of QP % 6."""
    q = (chroma_qp(qp) if comp else qp) + 6 * (bd - 8)
    return 14 + q // 6 + (15 - bd - int(math.log2(n))), QUANT_SCALES[q % 6]


def slice_start_contexts(qp):
    """The 160 context bytes ([159] = 0) an I slice of this QP starts from."""
    out = np.zeros(160, np.uint8)
    for i, v in enumerate(CTX_INIT):
        slope, offset = (v >> 4) * 5 - 45, ((v & 15) << 3) - 16
        st = min(max(((slope * qp) >> 4) + offset, 1), 126)
        mps = st >= 64
        out[i] = (((st - 64) if mps else (63 - st)) << 1) + mps
    return out


def context_sets(qp):
    """[4][160]: the slice-start states of the QP, then 3 seeded sets with every byte uniform in 0..125 (any state a context can be in)."""
    rng = np.random.default_rng(9001)
    sets = np.zeros((4, 160), np.uint8)
    sets[0] = slice_start_contexts(qp)
    sets[1:, :NUM_CTX] = rng.integers(0, 126, (3, NUM_CTX))
    return sets


def _scan_next(kind, bw, bh, line, col):
    if kind == 0:
        if col == bw - 1 or line == 0:
            line += col + 1
            col = 0
            if line >= bh:
                col += line - (bh - 1)
                line = bh - 1
        else:
            col += 1
            line -= 1
    elif kind == 1:
        if col == bw - 1:
            line, col = line + 1, 0
        else:
            col += 1
    else:
        if line == bh - 1:
            col, line = col + 1, 0
        else:
            line += 1
    return line, col


def scan_order(n, kind):
    """Raster position of every scan position of an n x n block: 4x4 groups in the order `kind` (0 diagonal, 1 horizontal, 2 vertical), the same order inside a group."""
    wg, out = n // 4, []
    gl = gc = 0
    for _ in range(wg * wg):
        l2 = c2 = 0
        for _ in range(16):
            out.append((l2 + gl * 4) * n + c2 + gc * 4)
            l2, c2 = _scan_next(kind, 4, 4, l2, c2)
        gl, gc = _scan_next(kind, wg, wg, gl, gc)
    return np.array(out, np.int64)


def scan_kind(comp, n, mode):
    if n > (4 if comp else 8):
        return 0
    if abs(mode - 26) <= 4:
        return 1
    if abs(mode - 10) <= 4:
        return 2
    return 0


# ---- residual blocks -----------------------------------------------------------------------------------------------------------------------------
def residual_blocks(n, luma, bd, seeded=SEEDED):
    """(names, int32 [count][n * n]) of residual blocks in [-M, M], M = 2^bd - 1."""
    M = (1 << bd) - 1
    names, blocks = [], []

    def add(name, b):
        b = np.asarray(b, np.int64).reshape(n, n)
        assert np.abs(b).max() <= M
        names.append(name)
        blocks.append(b.astype(np.int32).ravel())

    yy, xx = np.mgrid[0:n, 0:n]
    add("zero", np.zeros((n, n)))
    add("all+M", np.full((n, n), M))
    add("all-M", np.full((n, n), -M))
    for cname, (cy, cx) in (("tl", (0, 0)), ("tr", (0, n - 1)), ("bl", (n - 1, 0)), ("br", (n - 1, n - 1))):
        for v in (1, -1, M, -M):
            b = np.zeros((n, n), np.int64)
            b[cy, cx] = v
            add("corner-%s%+d" % (cname, v), b)
    for s in (1, -1):
        add("checker%+d" % s, s * M * (1 - 2 * ((yy + xx) & 1)))
        add("rows%+d" % s, s * M * (1 - 2 * (yy & 1)))
        add("cols%+d" % s, s * M * (1 - 2 * (xx & 1)))
    mats = [("dct", transform_matrix(n))] + ([("dst", DST4)] if luma and n == 4 else [])
    some = sorted({0, 1, n // 2, n - 1})
    for mname, t in mats:
        sg = np.sign(t)
        for u in range(n):
            for v in range(n):
                if n <= 8 or (u in some and v in some):
                    add("%s-basis(%d,%d)" % (mname, u, v), M * np.outer(sg[u], sg[v]))
                if u in some and v in some:
                    add("%s-basis(%d,%d)neg" % (mname, u, v), -M * np.outer(sg[u], sg[v]))
    rng = np.random.default_rng(1000 * n + 10 * bd + luma)
    for i in range(seeded[0]):
        add("uniform#%d" % i, rng.integers(-M, M + 1, (n, n)))
    for i in range(seeded[1]):
        b = np.zeros((n, n), np.int64)
        cnt = int(rng.integers(1, max(2, n * n // 8) + 1))
        idx = rng.choice(n * n, cnt, replace=False)
        b.ravel()[idx] = rng.integers(-M, M + 1, cnt)
        add("sparse#%d" % i, b)
    for i in range(seeded[2]):
        add("small#%d" % i, rng.integers(-3, 4, (n, n)))
    return names, np.stack(blocks)


# ---- coefficient blocks (entry 1) ------------------------------------------------------------------------------------------------------------------
def _target_tc(level, qbits, scale, just):
    """A coefficient magnitude whose rounded level (|c| * scale + 2^(qbits - 1)) >> qbits is exactly `level`: the smallest one (just above level - 1/2,
    where RDOQ weighs level against level - 1) or the first at or above `level` itself."""
    lo = ((2 * level - 1) << (qbits - 1)) if just else (level << qbits)
    tc = -(-lo // scale)
    assert tc <= 32767 and (tc * scale + (1 << (qbits - 1))) >> qbits == level, (level, qbits, scale, tc)
    return tc


def coefficient_blocks(n, comp, bd, qp, mode, seeded=4):
    """(names, int32 [count][n * n]) of coefficient blocks for one parameter set (the target-level and Laplacian blocks follow the quantiser step of the QP)."""
    qbits, scale = quant_params(qp, comp, n, bd)
    scan = scan_order(n, scan_kind(comp, n, mode))
    names, blocks = [], []

    def add(name, b):
        b = np.asarray(b, np.int64).ravel()
        assert b.min() >= -32768 and b.max() <= 32767
        names.append(name)
        blocks.append(b.astype(np.int32))

    add("all+32767", np.full(n * n, 32767))
    add("all-32768", np.full(n * n, -32768))
    t1 = _target_tc(1, qbits, scale, False)
    for pname, sp in (("first", 0), ("second", 1), ("last-1", n * n - 2), ("last", n * n - 1)):
        for v in (t1, -t1, 32767, -32768):
            b = np.zeros(n * n, np.int64)
            b[scan[sp]] = v
            add("single-%s%+d" % (pname, v), b)
    wg = n // 4
    gy, gx = (np.arange(n * n) // n) // 4, (np.arange(n * n) % n) // 4
    groups = [("whole", np.ones(n * n, bool))]
    if wg > 1:
        groups += [("alternate", ((gy + gx) & 1) == 0), ("antidiagonal", (gy + gx) == wg - 1)]
    sign = 1 - 2 * ((np.arange(n * n) // n + np.arange(n * n) % n) & 1)
    for level in (1, 2, 3):
        for just in (False, True):
            tc = _target_tc(level, qbits, scale, just)
            for gname, mask in groups:
                add("level%d%s-%s" % (level, "just" if just else "", gname), np.where(mask, tc, 0))
                add("level%d%s-%s-signs" % (level, "just" if just else "", gname), np.where(mask, tc * sign, 0))
    rng = np.random.default_rng(7 * n + 100 * comp + 1000 * qp + bd + 31 * mode)
    step = (1 << qbits) / scale
    fy, fx = np.arange(n * n) // n, np.arange(n * n) % n
    for i in range(seeded):
        spread = step * (0.6 + 2.5 * i) * np.exp(-(fy + fx) * (4.0 / n) * (0.3 + 0.3 * i))
        mag = np.minimum(np.rint(rng.laplace(0, 1, n * n) * spread), 32767)
        add("laplace#%d" % i, np.clip(mag, -32768, 32767))
    return names, np.stack(blocks)


# ---- level blocks (entry 2) and the reference's own events -----------------------------------------------------------------------------------------
_stage_cache = {}


def stage_events(name):
    """The TU events of tests/golden/<name>.npz: {kind: [(n, comp, int32 [3][n * n])]}, kind 2 = (residual, coefficients, levels) through transformNxN,
    kind 3 = (levels, dequantised, residual) through invTransformNxN; and the fixture's QP."""
    if name not in _stage_cache:
        f = np.load(os.path.join(GOLD, name + ".npz"))
        kind, a, b, off, blk = (f[k] for k in ("kind", "a", "b", "blk_off", "blk"))
        ev = {2: [], 3: []}
        for i in np.nonzero(kind >= 2)[0]:
            n = int(a[i])
            ev[int(kind[i])].append((n, int(b[i]), blk[off[i]:off[i + 1]].astype(np.int32).reshape(3, n * n)))
        _stage_cache[name] = (ev, int(f["qp"]))
    return _stage_cache[name]


def level_blocks(n, comp):
    """(names, int32 [count][n * n]): the distinct level blocks of the fixtures' kind-3 events of this size and component, then +-32767 blocks."""
    names, blocks, seen = [], [], set()
    for fx in STAGE_FIXTURES:
        for i, (en, ec, b) in enumerate(stage_events(fx)[0][3]):
            if en == n and ec == comp and b[0].tobytes() not in seen:
                seen.add(b[0].tobytes())
                names.append("%s-ev%d" % (fx, i))
                blocks.append(b[0])
    idx = np.arange(n * n)
    sign = 1 - 2 * ((idx // n + idx % n) & 1)
    for name, b in (("all+32767", np.full(n * n, 32767)), ("all-32767", np.full(n * n, -32767)), ("checker32767", 32767 * sign), ("dc+32767", np.where(idx == 0, 32767, 0)),
                    ("last-32767", np.where(idx == n * n - 1, -32767, 0))):
        names.append(name)
        blocks.append(b.astype(np.int32))
    return names, np.stack(blocks)


# ---- calls ----------------------------------------------------------------------------------------------------------------------------------------
Call = namedtuple("Call", "entry bd tools comp n qp mode tskip cbf_ctx names blocks ctx")


def describe(c, b=None):
    s = "entry %d n %d comp %d qp %d mode %d tskip %d cbf_ctx %d tools 0x%02x bd %d" % (c.entry, c.n, c.comp, c.qp, c.mode, c.tskip, c.cbf_ctx, c.tools, c.bd)
    return s if b is None else s + " case %s (block %d)" % (c.names[b], b)


def _param_sets(n, luma, qps, full):
    """(comp, qp, mode, tskip, cbf_ctx) sets of one block size and channel type.  full: every QP with every mode where the mode chooses the scan, with both cbf contexts
    elsewhere, and transform skip at 4x4; otherwise (the extra tool sets) one rotation through the lists."""
    cbfs = (0, 1) if luma else (0, 1, 2, 3)              # luma: trDepth == 0 ? 1 : 0; chroma: the transform depth
    scans = n <= (8 if luma else 4)
    out = []
    for qi, qp in enumerate(qps):
        if full and scans:
            for mi, mode in enumerate(DIR_MODES):
                out.append((0 if luma else 1 + ((qi + mi) & 1), qp, mode, 0, cbfs[(qi + mi) % len(cbfs)]))
        elif full:
            for ci in range(2):
                out.append((0 if luma else 1 + ((qi + ci) & 1), qp, DIR_MODES[(qi + ci) % 5], 0, cbfs[(qi + 2 * ci) % len(cbfs)]))
        else:
            out.append((0 if luma else 1 + (qi & 1), qp, DIR_MODES[qi % 5], 0, cbfs[qi % len(cbfs)]))
        if n == 4:
            for j in range(2 if full else 1):
                out.append((0 if luma else 1 + ((qi + j) & 1), qp, DIR_MODES[(qi + 2 * j + 1) % 5], 1, cbfs[(qi + j + 1) % len(cbfs)]))
    return out


def _with_ctx(entry, bd, tools, ps, n, names, blocks, index):
    comp, qp, mode, tskip, cbf = ps
    sets = context_sets(qp)
    ctx = sets[(np.arange(len(blocks)) + index) % 4]
    return Call(entry, bd, tools, comp, n, qp, mode, tskip, cbf, names, np.ascontiguousarray(blocks, np.int32), np.ascontiguousarray(ctx, np.uint8))


def tu_calls(bd, tools_rt, seeded=SEEDED):
    """Every call of the TU-chain corpus for a build of bit depth `bd`; tools_rt: the build reads the tool switches at run time (the extra tool sets are added)."""
    calls = []
    shapes = [(n, True) for n in (4, 8, 16, 32)] + [(n, False) for n in (4, 8, 16)]
    for n, luma in shapes:
        rnames, rblocks = residual_blocks(n, luma, bd, seeded)
        tool_sets = [(TOOLS_REFERENCE, True, QPS)] + ([(t, False, QPS[i % 2::2]) for i, t in enumerate(TOOL_SETS_RT)] if tools_rt else [])      # (the extra sets: every second QP, alternating)
        for tools, full, qps in tool_sets:
            for ps in _param_sets(n, luma, qps, full):
                calls.append(_with_ctx(0, bd, tools, ps, n, rnames, rblocks, len(calls)))
                cnames, cblocks = coefficient_blocks(n, ps[0], bd, ps[1], ps[2])
                calls.append(_with_ctx(1, bd, tools, ps, n, cnames, cblocks, len(calls)))
        for comp in ((0,) if luma else (1, 2)):
            lnames, lblocks = level_blocks(n, comp)
            nfix = len(lblocks) - 5                           # the fixtures' blocks are dealt over the QPs, the +-32767 blocks meet every QP
            for qi, qp in enumerate(QPS):
                sel = [i for i in range(nfix) if i % len(QPS) == qi] + list(range(nfix, len(lblocks)))
                for tskip in ((0, 1) if n == 4 else (0,)):
                    calls.append(_with_ctx(2, bd, TOOLS_REFERENCE, (comp, qp, 1, tskip, 0), n, [lnames[i] for i in sel], lblocks[sel], len(calls)))
    return calls


def replay_calls(kind):
    """The fixtures' events as calls (8-bit, the fixture's QP, reference tools): kind 2 -> entry 0 (residual in, the coefficients are the reference's), kind 3 ->
    entry 2 (levels in, dequantised coefficients and residual are the reference's).  Returns [(call, expected int32 [count][3][n * n])].  Whether a 4x4 event was
    transform-skipped is not in the trace; it is read off the event itself: its coefficients are the residual << 5 (kind 2) / its residual is (dequantised + 16) >> 5
    (kind 3).  An event that fits neither way still fails the comparison, under tskip 0."""
    out = []
    for fx in STAGE_FIXTURES:
        ev, qp = stage_events(fx)
        groups = {}
        for i, (n, comp, b) in enumerate(ev[kind]):
            ts = 0
            if n == 4:
                ts = int(np.array_equal(b[1], b[0] << 5) and b[0].any()) if kind == 2 else int(np.array_equal(b[2], (b[1] + 16) >> 5) and b[1].any())
            groups.setdefault((n, comp, ts), []).append((i, b))
        for (n, comp, ts), lst in sorted(groups.items()):
            names = ["%s-ev%d" % (fx, i) for i, _ in lst]
            exp = np.stack([b for _, b in lst])
            c = _with_ctx(0 if kind == 2 else 2, 8, TOOLS_REFERENCE, (comp, qp, 1, ts, 0), n, names, exp[:, 0], 0)
            out.append((c, exp))
    return out


# ---- prediction cases -----------------------------------------------------------------------------------------------------------------------------
PredCall = namedtuple("PredCall", "bd tools comp n names lines org")


def describe_pred(c, i=None):
    s = "n %d comp %d tools 0x%02x bd %d" % (c.n, c.comp, c.tools, c.bd)
    return s if i is None else s + " case %s (case %d)" % (c.names[i], i)


def reference_lines(n, bd, seeded=4):
    """(names, int16 [count][4 n + 1]) of reference lines: bottom-left ... left ... corner (2n) ... top ... top-right."""
    mx, ln, thr = (1 << bd) - 1, 4 * n + 1, 1 << (bd - 5)
    names, lines = [], []

    def add(name, v):
        v = np.asarray(v, np.int64)
        assert v.shape == (ln,) and v.min() >= 0 and v.max() <= mx, name
        names.append(name)
        lines.append(v.astype(np.int16))

    i = np.arange(ln)
    add("zeros", np.zeros(ln))
    add("max", np.full(ln, mx))
    add("alternate0", mx * (i & 1))
    add("alternate1", mx * (1 - (i & 1)))
    for pname, pos in (("corner", 2 * n), ("mid-top", 3 * n + 1), ("mid-left", n)):
        add("step-up@%s" % pname, np.where(i >= pos, mx, 0))
        add("step-down@%s" % pname, np.where(i >= pos, 0, mx))
    # ramps around the strong-smoothing test |bl + tl - 2 mid-left| < thr and |tl + tr - 2 mid-top| < thr (thr = 2^(bd - 5); n = 32 luma; at other sizes plain ramps)
    lo, span = mx // 8, min(8 * n, mx - mx // 8 - 8) & ~7
    base = np.rint(np.linspace(lo, lo + span, ln)).astype(np.int64)
    base[[0, 2 * n, 4 * n]] = [lo, lo + span // 2, lo + span]                          # bl, tl, tr a multiple of 4 apart: bl + tl and tl + tr have the parity of 2 lo, even
    for side, mid, (p, q) in (("left", n, (0, 2 * n)), ("top", 3 * n, (2 * n, 4 * n))):
        for d in (0, thr - 2, thr, -(thr - 2), -thr):                                    # even sums: the deviation is even -- thr - 2 trips, thr just misses
            v = base.copy()
            v[mid] = (v[p] + v[q] - d) // 2
            add("ramp-%s-dev%+d" % (side, d), v)
        v = base.copy()
        v[q] += 1                                                                        # odd sum: deviations thr - 1 (trips) and thr + 1 (misses)
        for d in (thr - 1, thr + 1):
            w = v.copy()
            w[mid] = (w[p] + w[q] - d) // 2
            add("ramp-%s-odd-dev%+d" % (side, d), w)
    rng = np.random.default_rng(50 * n + bd)
    for j in range(seeded):
        add("uniform#%d" % j, rng.integers(0, mx + 1, ln))
        add("walk#%d" % j, np.clip(mx // 2 + np.cumsum(rng.integers(-(3 + 4 * j), 4 + 4 * j + 1, ln)), 0, mx))
    return names, np.stack(lines)


def pred_calls(bd, tools_rt, seeded=4):
    """Prediction cases per (component, size): luma 4..64 (64: filtered line and SATD only -- predict_block stops at 32), chroma 4..16 (lines only: no SATD)."""
    mx = (1 << bd) - 1
    calls = []
    for comp, sizes in ((0, (4, 8, 16, 32, 64)), (1, (4, 8, 16)), (2, (4, 8, 16))):
        for n in sizes:
            lnames, lines = reference_lines(n, bd, seeded)
            if comp:
                calls.append(PredCall(bd, TOOLS_REFERENCE, comp, n, lnames, lines, None))
                continue
            rng = np.random.default_rng(77 * n + bd)
            names, ls, orgs = [], [], []
            for li, (lname, line) in enumerate(zip(lnames, lines)):
                dc = (int(line[2 * n + 1:3 * n + 1].sum()) + int(line[n:2 * n].sum()) + n) // (2 * n)
                kinds = (("org0", np.zeros(n * n)), ("orgmax", np.full(n * n, mx)), ("org~dc", np.full(n * n, mx - dc)), ("orgrand", rng.integers(0, mx + 1, n * n)))
                # every line meets two kinds of original (rotating), the seeded lines all four
                pick = range(4) if "#" in lname else (li % 4, (li + 1 + li // 4) % 4)
                for kname, o in (kinds[p] for p in dict.fromkeys(pick)):
                    names.append(lname + "/" + kname)
                    ls.append(line)
                    orgs.append(np.asarray(o, np.uint16))
            for tools in [TOOLS_REFERENCE] + ([TOOLS_REFERENCE & ~TOOL_STRONG_INTRA] if tools_rt and n >= 32 else []):
                calls.append(PredCall(bd, tools, comp, n, names, np.stack(ls), np.stack(orgs)))
    return calls
