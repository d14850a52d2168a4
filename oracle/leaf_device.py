"""oracle/leaf_device.py -- TEST INFRASTRUCTURE: the device side of the leaf tests.

lib/libhevcdl_hip_leaf.so (the decision kernel's four builds with -DHEVCDL_LEAF_TEST) defines the same kernel names as the product library, so it is loaded in a process
of its own: tests/test_rd_leaf_gpu.py starts this file as a child, once per build, and reads what it saved.

    python oracle/leaf_device.py LIB SUFFIX OUT.npz        run the whole corpus of oracle/leaf_cases.py on build SUFFIX ("", _bd10, _wide, _tools), twice; save the outputs
    python oracle/leaf_device.py LIB SUFFIX --compare [entry=E] [n=N] [comp=C] [qp=Q] [mode=M] [tskip=T] [tools=0x..] [case=SUBSTRING] [pred]
        run the calls of the corpus that match, next to the oracle, and print every difference (build, leaf, parameters, case, first differing position):
        the tool for finding which leaf a kernel rewrite broke, and on which block
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import leaf_cases  # noqa: E402

TU_KEYS = ("coef", "lvl", "deq", "resi", "abs_sum", "frac", "ctx")          # the outputs of a TU call, device and oracle alike
PRED_KEYS = ("fline", "pred", "satd")


class Device:
    """The host runners of one build of the leaf library."""

    def __init__(self, lib_path, suffix):
        self.lib, self.suffix = ctypes.CDLL(lib_path), suffix
        vp, ci = ctypes.c_void_p, ctypes.c_int
        self._tu = getattr(self.lib, "hevcdl_leaf_tu_run" + suffix)
        self._tu.restype, self._tu.argtypes = ci, [vp, vp] + [ci] * 10 + [vp] * 9
        self._pred = getattr(self.lib, "hevcdl_leaf_pred_run" + suffix)
        self._pred.restype, self._pred.argtypes = ci, [ci] * 4 + [vp] * 5
        info = getattr(self.lib, "hevcdl_leaf_info" + suffix)
        info.restype = None
        bd, nw, rt = ci(), ci(), ci()
        info(ctypes.byref(bd), ctypes.byref(nw), ctypes.byref(rt))
        self.bit_depth, self.waves, self.tools_rt = bd.value, nw.value, bool(rt.value)

    def tu(self, c):
        """hevcdl_leaf_tu_run on a leaf_cases.Call -> dict of TU_KEYS (16-bit block outputs widened to int32, as the oracle's)."""
        consts, sbh, qpc = leaf_cases.rd_consts(c.qp, c.bd)
        blocks = np.ascontiguousarray(c.blocks, np.int32)
        assert not blocks.size or (blocks.min() >= -32768 and blocks.max() <= 32767)
        inp, ctx = blocks.astype(np.int16), np.ascontiguousarray(c.ctx, np.uint8)
        nb, nn = inp.shape
        o = {k: np.zeros((nb, nn), np.int16) for k in ("coef", "lvl", "deq", "resi")}
        o.update(abs_sum=np.zeros(nb, np.uint32), frac=np.zeros(nb, np.uint64), ctx=np.zeros((nb, 160), np.uint8))
        rc = self._tu(consts.ctypes.data, sbh.ctypes.data, c.qp, qpc, c.tools, c.comp, c.n, c.mode, c.tskip, c.cbf_ctx, c.entry, nb, inp.ctypes.data, ctx.ctypes.data,
                      o["coef"].ctypes.data, o["lvl"].ctypes.data, o["abs_sum"].ctypes.data, o["frac"].ctypes.data, o["ctx"].ctypes.data, o["deq"].ctypes.data, o["resi"].ctypes.data)
        if rc != 0:
            raise RuntimeError("hevcdl_leaf_tu_run%s failed rc=%d: %s" % (self.suffix, rc, leaf_cases.describe(c)))
        for k in ("coef", "lvl", "deq", "resi"):
            o[k] = o[k].astype(np.int32)
        return o

    def pred(self, c):
        """hevcdl_leaf_pred_run on a leaf_cases.PredCall -> dict of PRED_KEYS (those the call has)."""
        lines = np.ascontiguousarray(c.lines, np.int16)
        nc, n = lines.shape[0], c.n
        o = {}
        org = None
        if not c.comp:
            org = np.ascontiguousarray(c.org, np.uint16)
            o["fline"], o["satd"] = np.zeros((nc, 4 * n + 1), np.int16), np.zeros((nc, 35), np.uint32)
        if n <= 32:
            o["pred"] = np.zeros((nc, 35, n * n), np.uint16)
        rc = self._pred(c.tools, c.comp, n, nc, lines.ctypes.data, None if org is None else org.ctypes.data, o["fline"].ctypes.data if "fline" in o else None,
                        o["pred"].ctypes.data if "pred" in o else None, o["satd"].ctypes.data if "satd" in o else None)
        if rc != 0:
            raise RuntimeError("hevcdl_leaf_pred_run%s failed rc=%d: %s" % (self.suffix, rc, leaf_cases.describe_pred(c)))
        if "pred" in o:
            o["pred"] = o["pred"].astype(np.int16)
        return o


def first_difference(build, what, dev, ref, keys):
    """None when every word of every output agrees, else a message naming the build, the leaf output, the call, the case and the first differing position."""
    for k in keys:
        if k not in ref:
            continue
        d, r = np.asarray(dev[k]), np.asarray(ref[k])
        if d.shape != r.shape:
            return "build %r %s: output %s has shape %s, expected %s" % (build, what(None), k, d.shape, r.shape)
        if not np.array_equal(d, r):
            idx = np.argwhere(d != r)[0]
            pos = idx[1:].tolist()
            return "build %r leaf output %s: %s: first difference at %s: device %s, expected %s (%d of %d words differ)" % (
                build, k, what(int(idx[0])), pos if pos else "-", d[tuple(idx)], r[tuple(idx)], int((d != r).sum()), d.size)
    return None


def corpus(suffix):
    """Everything a build is run on: (TU calls, [(replay call, expected)] of kind 2, of kind 3, prediction calls); the replays on the 8-bit builds only."""
    bd, rt = leaf_cases.BUILDS[suffix]
    r2, r3 = (leaf_cases.replay_calls(2), leaf_cases.replay_calls(3)) if bd == 8 else ([], [])
    return leaf_cases.tu_calls(bd, rt), r2, r3, leaf_cases.pred_calls(bd, rt)


def pack(outs, keys):
    """A list of output dicts as one flat array per key (the reader knows the shapes from the calls)."""
    return {k: np.concatenate([np.asarray(o[k]).ravel() for o in outs if k in o] or [np.zeros(0, np.int32)]) for k in keys}


def unpack(flat, like, keys):
    """Inverse of pack: `like` = the matching list of reference dicts (shapes and dtypes)."""
    outs, at = [], {k: 0 for k in keys}
    for r in like:
        o = {}
        for k in keys:
            if k in r:
                o[k] = flat[k][at[k]:at[k] + r[k].size].reshape(r[k].shape)
                at[k] += r[k].size
        outs.append(o)
    assert all(at[k] == flat[k].size for k in keys), "the saved outputs do not match the corpus"
    return outs


def _digest(o):
    h = hashlib.sha256()
    for k in sorted(o):
        h.update(np.ascontiguousarray(o[k]).tobytes())
    return np.frombuffer(h.digest()[:8], np.uint64)[0]


def refusals(dev):
    """(refused, tried): arguments outside what the kernels index with -- the host runners must turn every one of them down (status -1) without launching."""
    bd = dev.bit_depth
    ctx = leaf_cases.slice_start_contexts(30)[None]
    ok = leaf_cases.Call(0, bd, leaf_cases.TOOLS_REFERENCE, 0, 4, 30, 1, 0, 0, ["zero"], np.zeros((1, 16), np.int32), ctx)
    dev.tu(ok)                                       # (the base call itself is accepted)
    bad_ctx = ctx.copy()
    bad_ctx[0, 40] = 126
    bad = [ok._replace(n=5, blocks=np.zeros((1, 25), np.int32)), ok._replace(n=64, blocks=np.zeros((1, 4096), np.int32)), ok._replace(comp=3), ok._replace(comp=-1),
           ok._replace(comp=1, n=32, blocks=np.zeros((1, 1024), np.int32)), ok._replace(mode=35), ok._replace(mode=-1), ok._replace(tskip=2),
           ok._replace(tskip=1, n=8, blocks=np.zeros((1, 64), np.int32)), ok._replace(entry=3), ok._replace(entry=-1), ok._replace(cbf_ctx=5), ok._replace(qp=52),
           ok._replace(cbf_ctx=-1), ok._replace(ctx=bad_ctx), ok._replace(blocks=np.zeros((0, 16), np.int32), ctx=ctx[:0])]
    line = np.full((1, 17), 100, np.int16)
    okp = leaf_cases.PredCall(bd, leaf_cases.TOOLS_REFERENCE, 0, 4, ["flat"], line, np.zeros((1, 16), np.uint16))
    dev.pred(okp)
    badp = [okp._replace(n=3), okp._replace(n=128), okp._replace(comp=3), okp._replace(comp=1, n=32, lines=np.zeros((1, 129), np.int16)), okp._replace(comp=1, n=64, lines=np.zeros((1, 257), np.int16)),
            okp._replace(lines=np.full((1, 17), 1 << bd, np.int16)), okp._replace(lines=np.full((1, 17), -1, np.int16)), okp._replace(org=np.full((1, 16), 1 << bd, np.uint16))]
    refused = 0
    for c, fn in [(c, dev.tu) for c in bad] + [(c, dev.pred) for c in badp]:
        try:
            fn(c)
        except RuntimeError as e:
            refused += "rc=-1" in str(e)
    return refused, len(bad) + len(badp)


def run_all(lib_path, suffix, out_path):
    import time
    t0 = time.time()
    dev = Device(lib_path, suffix)
    assert (dev.bit_depth, dev.tools_rt) == leaf_cases.BUILDS[suffix], "the library's build %r is not what the test expects" % suffix
    tu, r2, r3, pr = corpus(suffix)
    tu_all = tu + [c for c, _ in r2] + [c for c, _ in r3]
    save, times = {}, [time.time() - t0]
    for run in range(2):                         # the second run only for its digests: two launches of the same input must give the same bytes
        tu_out = [dev.tu(c) for c in tu_all]
        pr_out = [dev.pred(c) for c in pr]
        save["digest%d" % run] = np.array([_digest(o) for o in tu_out + pr_out], np.uint64)
        if run == 0:
            save.update({"tu_" + k: v for k, v in pack(tu_out, TU_KEYS).items()})
            save.update({"pred_" + k: v for k, v in pack(pr_out, PRED_KEYS).items()})
        times.append(time.time() - t0)
    save["refusals"] = np.array(refusals(dev))
    save["seconds"] = np.array(times)                     # since the start: corpus built, first run done, second run done
    np.savez(out_path, **save)


def oracle_tu(c):
    import ref_tools
    return ref_tools.oracle_tu_leaf(c.qp, c.bd, c.tools, c.comp, c.n, c.mode, c.tskip, c.cbf_ctx, c.entry, c.blocks, c.ctx)


def oracle_pred(c):
    import ref_tools
    return ref_tools.oracle_pred_leaf(c.bd, c.tools, c.comp, c.n, c.lines, c.org)


def compare_cli(lib_path, suffix, args):
    dev = Device(lib_path, suffix)
    want = dict(a.split("=", 1) for a in args if "=" in a)
    case = want.pop("case", None)
    tu, r2, r3, pr = corpus(suffix)
    bad = ran = 0
    if "pred" in args:
        for c in pr:
            if any(int(v, 0) != getattr(c, k) for k, v in want.items() if k in c._fields):
                continue
            ran += 1
            msg = first_difference(suffix, lambda i, c=c: leaf_cases.describe_pred(c, i), dev.pred(c), oracle_pred(c), PRED_KEYS)
            if msg:
                bad += 1
                print(msg)
    else:
        for c in tu + [c for c, _ in r2] + [c for c, _ in r3]:
            if any(int(v, 0) != getattr(c, k) for k, v in want.items()):
                continue
            if case is not None:
                sel = [i for i, nm in enumerate(c.names) if case in nm]
                if not sel:
                    continue
                c = c._replace(names=[c.names[i] for i in sel], blocks=c.blocks[sel], ctx=c.ctx[sel])
            ran += 1
            msg = first_difference(suffix, lambda i, c=c: leaf_cases.describe(c, i), dev.tu(c), oracle_tu(c), TU_KEYS)
            if msg:
                bad += 1
                print(msg)
    print("%d calls run, %d differ from the oracle" % (ran, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[3] == "--compare":
        sys.exit(compare_cli(sys.argv[1], sys.argv[2], sys.argv[4:]))
    run_all(sys.argv[1], sys.argv[2], sys.argv[3])
