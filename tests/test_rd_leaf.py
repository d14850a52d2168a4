"""The leaf entries of the oracle (hm_oracle_tu_leaf / hm_oracle_pred_leaf, oracle/hm_oracle.c) on their own: the oracle's transforms against the defining
matrix products, the range premise behind the decision kernel's 16-bit transform storage, and the reference's own stage traces replayed through the entries.
tests/test_rd_leaf_gpu.py compares the device leaves with these entries on the same corpus (oracle/leaf_cases.py)."""
import numpy as np
import pytest

import leaf_cases
import ref_tools


def _log2(n):
    return {4: 2, 8: 3, 16: 4, 32: 5}[n]


def _clip16(v):
    return np.clip(v, -32768, 32767)


def fwd_numpy(x, n, bd, dst):
    """The forward transform by its definition, int64: first stage over the rows (X T^t + a1) >> s1, second over the columns (T A + a2) >> s2."""
    t = leaf_cases.transform_matrix(n, dst)
    s1, s2 = _log2(n) + bd - 9, _log2(n) + 6
    a1 = (1 << (s1 - 1)) if s1 > 0 else 0
    a = (x.astype(np.int64) @ t.T + a1) >> s1
    return a, (t @ a + (1 << (s2 - 1))) >> s2


def inv_numpy(c, n, bd, dst):
    """The inverse transform by its definition: columns first, shift 7, then rows, shift 20 - bit depth, each stage clipped to 16 bits."""
    t = leaf_cases.transform_matrix(n, dst)
    e = _clip16((t.T @ c.astype(np.int64) + 64) >> 7)
    return _clip16((e @ t + (1 << (19 - bd))) >> (20 - bd))


def test_transform_matrices_are_the_standards():
    """The matrices the numpy restatement uses are the scaled cosines / sines the standard rounds by hand: within 2 of 64 sqrt(2) cos((2i + 1) k pi / 2N), within 1 of (256 / 3) sin((2k + 1)(i + 1) pi / 9)."""
    for n in (4, 8, 16, 32):
        t = leaf_cases.transform_matrix(n)
        k, i = np.mgrid[0:n, 0:n]
        ideal = 64 * np.sqrt(2.0) * np.cos((2 * i + 1) * k * np.pi / (2 * n))
        ideal[0] = 64
        assert np.abs(t - ideal).max() < 2.0, n
    k, i = np.mgrid[0:4, 0:4]
    assert np.abs(leaf_cases.DST4 - 128 * 2 / 3.0 * np.sin((2 * k + 1) * (i + 1) * np.pi / 9)).max() < 1.0


SHAPES = [(n, luma) for n in (4, 8, 16, 32) for luma in (True, False) if luma or n <= 16]


@pytest.mark.parametrize("bd", [8, 10])
def test_oracle_transforms_equal_the_matrix_products_and_fit_16_bits(oracle_built, bd):
    """Over the whole residual corpus: hm_oracle_tu_leaf's first-stage intermediate and coefficients == the int64 matrix products, its inverse transform of the
    dequantised coefficients == the clipped inverse products -- and every intermediate and coefficient lies within int16, the premise of the kernel's storage."""
    for n, luma in SHAPES:
        names, blocks = leaf_cases.residual_blocks(n, luma, bd)
        comp, dst = 0 if luma else 1, luma and n == 4
        ctx = np.tile(leaf_cases.slice_start_contexts(32), (len(blocks), 1))
        o = ref_tools.oracle_tu_leaf(32, bd, leaf_cases.TOOLS_REFERENCE, comp, n, 1, 0, 0, 0, blocks, ctx, want_stage1=True)
        for b, name in enumerate(names):
            a, c = fwd_numpy(blocks[b].reshape(n, n), n, bd, dst)
            what = "bd %d n %d comp %d case %s" % (bd, n, comp, name)
            assert np.array_equal(o["stage1"][b].reshape(n, n), a.T), what + ": first stage"          # (the oracle keeps it [frequency][row])
            assert np.array_equal(o["coef"][b].reshape(n, n), c), what + ": coefficients"
        for k in ("stage1", "coef"):
            assert o[k].min() >= -32768 and o[k].max() <= 32767, "bd %d n %d comp %d: %s leaves int16: [%d, %d]" % (bd, n, comp, k, o[k].min(), o[k].max())
        # the inverse: the corpus's own coefficients as levels, through the dequantiser (small and large steps: QP 51 drives the 16-bit clips), against its output
        for qp in (4, 51):
            o2 = ref_tools.oracle_tu_leaf(qp, bd, leaf_cases.TOOLS_REFERENCE, comp, n, 1, 0, 0, 2, o["coef"], ctx)
            for b, name in enumerate(names):
                r = inv_numpy(o2["deq"][b].reshape(n, n), n, bd, dst)
                assert np.array_equal(o2["resi"][b].reshape(n, n), r), "bd %d n %d comp %d qp %d case %s: inverse transform" % (bd, n, comp, qp, name)


@pytest.mark.parametrize("bd", [8, 10])
def test_residual_range_bounds_the_forward_transform(bd):
    """The analytic form of the premise: a row of a transform matrix has L1 norm at most 64 N (2048 at 32x32), so with |residual| <= M = 2^bd - 1 the first stage is
    at most (64 N M + a1) >> s1 = 2^15 - 2^(15 - bd), and the second stage cannot grow it: int16 holds both.  One sample more (M + 1) would not fit."""
    m = (1 << bd) - 1
    for n, dst in ((4, False), (4, True), (8, False), (16, False), (32, False)):
        t = leaf_cases.transform_matrix(n, dst)
        l1 = int(np.abs(t).sum(axis=1).max())
        assert l1 <= 64 * n and (dst or l1 == 64 * n), (n, dst, l1)
        s1, s2 = _log2(n) + bd - 9, _log2(n) + 6
        a1 = (1 << (s1 - 1)) if s1 > 0 else 0
        stage1 = (64 * n * m + a1) >> s1
        assert stage1 == (1 << 15) - (1 << (15 - bd)) and (-64 * n * m + a1) >> s1 >= -32768, (n, stage1)
        assert (64 * n * stage1 + (1 << (s2 - 1))) >> s2 <= 32767 and (-64 * n * stage1 + (1 << (s2 - 1))) >> s2 >= -32768
        assert (64 * n * (m + 1) + a1) >> s1 > 32767                      # the contract is tight: the range cannot be one wider


def test_corpus_is_deterministic_and_of_bounded_size():
    """Both test files and the device child build the lists independently: they must be the same lists; and the whole TU corpus stays at a few tens of thousands of codings."""
    for bd, rt in ((8, False), (10, True)):
        a, b = leaf_cases.tu_calls(bd, rt), leaf_cases.tu_calls(bd, rt)
        assert len(a) == len(b) and all(x[:9] == y[:9] and x.names == y.names and np.array_equal(x.blocks, y.blocks) and np.array_equal(x.ctx, y.ctx) for x, y in zip(a, b))
        total = sum(len(c.blocks) for c in a)
        assert 20000 < total < 60000, total
        m = (1 << bd) - 1
        assert all(np.abs(c.blocks).max() <= m for c in a if c.entry == 0)                   # the residual-range contract
        assert {c.qp for c in a} == set(leaf_cases.QPS) and {c.mode for c in a} == set(leaf_cases.DIR_MODES)
        assert {c.tools for c in a} == ({leaf_cases.TOOLS_REFERENCE} | (set(leaf_cases.TOOL_SETS_RT) if rt else set()))
        assert {(c.n, c.tskip) for c in a if c.tskip} == {(4, 1)} and all(c.ctx.max() <= 125 for c in a)


@pytest.mark.parametrize("kind", [2, 3])
def test_oracle_leaf_reproduces_the_reference_traces(oracle_built, kind):
    """Every TU event of the reference's stage traces (tests/golden/stage_*.npz) through the oracle's leaf entry: kind 2 residual -> coefficients (entry 0), kind 3
    levels -> dequantised coefficients -> residual (entry 2).  This pins the entries the device leaves are compared with to the reference itself."""
    replays = leaf_cases.replay_calls(kind)
    assert sum(len(c.blocks) for c, _ in replays) == sum(len(leaf_cases.stage_events(fx)[0][kind]) for fx in leaf_cases.STAGE_FIXTURES) > 3000
    for c, exp in replays:
        o = ref_tools.oracle_tu_leaf(c.qp, c.bd, c.tools, c.comp, c.n, c.mode, c.tskip, c.cbf_ctx, c.entry, c.blocks, c.ctx)
        for key, col in ((("coef", 1),) if kind == 2 else (("deq", 1), ("resi", 2))):
            if not np.array_equal(o[key], exp[:, col]):
                b, pos = np.argwhere(o[key] != exp[:, col])[0]
                raise AssertionError("oracle leaf output %s: %s: first difference at %d: oracle %d, reference %d" % (key, leaf_cases.describe(c, int(b)), pos, o[key][b, pos], exp[b, col, pos]))


def test_oracle_pred_leaf_agrees_with_the_prediction_formulas(oracle_built):
    """A plain check of the prediction entry's plumbing (lines, modes, the SATD's original block): DC, vertical and horizontal prediction of chroma blocks are what
    their definitions say, the luma SATD of a block predicted exactly is 0, and strong smoothing follows tool bit 0x20."""
    for c in leaf_cases.pred_calls(8, True):
        o = ref_tools.oracle_pred_leaf(c.bd, c.tools, c.comp, c.n, c.lines, c.org)
        n = c.n
        if c.comp:
            top, left = c.lines[:, 2 * n + 1:3 * n + 1].astype(np.int64), c.lines[:, n:2 * n][:, ::-1].astype(np.int64)
            p = o["pred"].reshape(len(c.lines), 35, n, n)
            assert np.array_equal(p[:, 26], np.repeat(top[:, None, :], n, axis=1)) and np.array_equal(p[:, 10], np.repeat(left[:, :, None], n, axis=2))
            assert np.array_equal(p[:, 1, 0, 0], (top.sum(1) + left.sum(1) + n) // (2 * n))
        elif n == 32:
            i = [j for j, nm in enumerate(c.names) if nm.startswith("ramp-left-dev+0/")][0]           # an exact ramp: both second differences are 0 < threshold
            ln, j = c.lines[i].astype(np.int64), np.arange(1, 64)
            plain = (ln[:-2] + 2 * ln[1:-1] + ln[2:] + 2) >> 2
            strong = np.concatenate([((64 - j) * ln[0] + j * ln[64] + 32) >> 6, ln[64:65], ((64 - j) * ln[64] + j * ln[128] + 32) >> 6])
            assert not np.array_equal(plain, strong)
            assert np.array_equal(o["fline"][i, 1:-1], strong if c.tools & leaf_cases.TOOL_STRONG_INTRA else plain), leaf_cases.describe_pred(c, i)
            k = [j for j, nm in enumerate(c.names) if nm.startswith("ramp-left-dev+8/")][0]           # deviation == threshold: just misses
            lk = c.lines[k].astype(np.int64)
            assert np.array_equal(o["fline"][k, 1:-1], (lk[:-2] + 2 * lk[1:-1] + lk[2:] + 2) >> 2), leaf_cases.describe_pred(c, k)
    # SATD 0: the original block is the DC prediction of a flat line
    lines = np.full((1, 4 * 8 + 1), 77, np.int16)
    o = ref_tools.oracle_pred_leaf(8, leaf_cases.TOOLS_REFERENCE, 0, 8, lines, np.full((1, 64), 77, np.uint16))
    assert o["satd"][0, 1] == 0 and (o["pred"][0] == 77).all()
    o = ref_tools.oracle_pred_leaf(8, leaf_cases.TOOLS_REFERENCE, 0, 8, lines, np.full((1, 64), 78, np.uint16))
    assert o["satd"][0, 1] == (64 * 1 + 2) >> 2                          # an 8x8 Hadamard of a constant difference: only the DC term, (64 + 2) >> 2


def test_leaf_entries_refuse_what_the_frame_path_cannot_reach(oracle_built):
    ctx = leaf_cases.slice_start_contexts(30)[None]
    for kw in (dict(n=5), dict(n=32, comp=1), dict(tskip=1, n=8), dict(mode=35), dict(entry=3), dict(qp=52), dict(bd=9)):
        a = dict(qp=30, bd=8, comp=0, n=4, mode=1, tskip=0, entry=0)
        a.update(kw)
        with pytest.raises(RuntimeError):
            ref_tools.oracle_tu_leaf(a["qp"], a["bd"], 0x7f, a["comp"], a["n"], a["mode"], a["tskip"], 0, a["entry"], np.zeros((1, a["n"] ** 2), np.int32), ctx)
    with pytest.raises(RuntimeError):
        ref_tools.oracle_pred_leaf(8, 0x7f, 1, 32, np.zeros((1, 129), np.int16))
