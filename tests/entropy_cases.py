"""Inputs of the entropy-coder tests (tests/test_entropy.py on the CPU, tests/test_entropy_gpu.py on the device): the golden fixtures as coder inputs, a seeded corpus of
synthetic records that no encode produces, garbage records, and the helpers that turn coded slice data into access units."""
import ctypes
import functools
import glob
import os

import numpy as np

from conftest import GOLD, fixture_tiles, fixture_lf, fixture_lf_offsets, fixture_wavefront

CASES = sorted(glob.glob(os.path.join(GOLD, "rd_*.npz")))
SAO_CASES = ["c192_q32_r2", "t576_q27_2x3", "w200_q27_r2"]
FUZZ_SIZES = [(8, 8), (64, 8), (8, 72), (72, 72), (136, 200), (200, 136)]
LEVELS = np.array([0, 0, 0, 1, -1, 2, -2, 3, -3, 5, -7, 12, -40, 300, 32767, -32767, -32768], np.int16)


def fixture_case(path):
    """-> (stream config, records [frames, ctus], expected stream) of a golden fixture, configured as tests/test_bitstream.py::stream_of does."""
    import hevcdl_amd
    f = np.load(path)
    w, h, qp = int(f["width"]), int(f["height"]), int(f["qp"])
    recs = np.frombuffer(f["records"].tobytes(), dtype=hevcdl_amd.REC_DTYPE).reshape(f["records"].shape[0], -1)
    bd = int(f["bit_depth"]) if "bit_depth" in f.files else 8
    tools = int(f["tools"]) if "tools" in f.files else hevcdl_amd.TOOLS_REFERENCE
    cfg = hevcdl_amd.stream_config(w, h, qp, tiles=fixture_tiles(f), bit_depth=bd, lf_across_tiles=fixture_lf(f), tools=tools, lf_offsets=fixture_lf_offsets(f), wavefront=fixture_wavefront(f))
    return cfg, recs, f["bitstream_nosao"].tobytes()


def sao_case(name):
    """-> (stream config with SAO, records, SAO parameters [frames, ctus, 3]) of a fixture, the parameters from the oracle's SAO as tests/test_sao.py takes them."""
    import hevcdl_amd
    import ref_tools
    __import__("__graft_entry__").build_oracle()
    f = np.load(os.path.join(GOLD, "rd_%s.npz" % name))
    w, h, qp, nf = int(f["width"]), int(f["height"]), int(f["qp"]), f["records"].shape[0]
    fb = w * h * 3 // 2
    recs = np.frombuffer(f["records"].tobytes(), dtype=hevcdl_amd.REC_DTYPE).reshape(nf, -1)
    params, _ = ref_tools.run_sao(f["yuv"].reshape(nf, fb), f["recon_deblocked"].reshape(nf, fb), w, h, qp, tiles=fixture_tiles(f))
    cfg = hevcdl_amd.stream_config(w, h, qp, sao=True, tiles=fixture_tiles(f), wavefront=fixture_wavefront(f))
    return cfg, recs, np.ascontiguousarray(params).view(hevcdl_amd.SAO_DTYPE).reshape(nf, -1, 3)


def host_writer_stream(cfg, recs, sao=None):
    """The existing host writer (hevcdl_write_access_unit) with a buffer that also holds pictures of maximal levels -> the frames' access units, joined."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    cap = cfg.width * cfg.height * 12 + (1 << 16)
    buf = np.zeros(cap, np.uint8)
    out = []
    for poc in range(recs.shape[0]):
        n = ctypes.c_size_t(0)
        r = np.ascontiguousarray(recs[poc])
        s = None if sao is None else np.ascontiguousarray(sao[poc])
        st = lib.hevcdl_write_access_unit(ctypes.byref(cfg), poc, r.ctypes.data, None if s is None else s.ctypes.data, buf.ctypes.data, cap, ctypes.byref(n))
        assert st == 0, st
        out.append(buf[:n.value].tobytes())
    return b"".join(out)


def assemble(cfg, coded):
    """code_slice_data's result -> the frames' access units, joined; no sub-stream may have overflowed."""
    import hevcdl_amd
    buf, sizes, ovf, off, cap = coded
    assert not ovf.any() and (sizes <= cap[None, :]).all()
    return b"".join(hevcdl_amd.write_access_unit_from_slice_data(cfg, poc, hevcdl_amd.pack_slice_data(buf[poc], sizes[poc], off), sizes[poc]) for poc in range(buf.shape[0]))


def check_guard(coded):
    """What every run must leave: nothing written outside the sub-stream regions (the gaps still hold the canary), and a length within the capacity or the overflow word."""
    import hevcdl_amd
    buf, sizes, ovf, off, cap = coded
    mask = np.ones(buf.shape[1], bool)
    for o, c in zip(off, cap):
        mask[int(o):int(o) + int(c)] = False
    assert mask.sum() == 64 * len(off)
    assert (buf[:, mask] == hevcdl_amd.CANARY).all(), "a byte outside the sub-stream regions was written"
    assert ((sizes <= cap[None, :]) | (ovf != 0)).all() and ((sizes > cap[None, :]) == (ovf != 0)).all()


# ---- synthetic records ----------------------------------------------------------------------------------------------------------------
def _z_of(x4, y4):
    z = 0
    for b in range(4):
        z |= ((x4 >> b) & 1) << (2 * b) | ((y4 >> b) & 1) << (2 * b + 1)
    return z


def _fill_block(rng, plane, base, n, style):
    blk = np.zeros(n * n, np.int16)
    if style == 0:      # entirely +-32767: escape codes at maximal length, long 0xff runs in the coder
        blk[:] = np.where(rng.integers(0, 2, n * n) == 1, 32767, -32767)
    elif style == 1:    # one coefficient, at the last scan position
        blk[n * n - 1] = LEVELS[rng.integers(3, len(LEVELS))]
    else:
        k = rng.integers(1, n * n + 1) if rng.integers(0, 3) else rng.integers(1, 4)
        idx = rng.choice(n * n, size=int(k), replace=False)
        blk[idx] = LEVELS[rng.integers(0, len(LEVELS), int(k))]
        if not blk.any():
            blk[idx[0]] = 1
    plane[base:base + n * n] = blk


def synth_records(rng, w, h, style=None):
    """Valid records of a w x h picture: random depth maps under the boundary rule, NxN at depth 3, transform trees within the allowed depth, every cbf pattern,
    transform-skip flags on 4x4 blocks, levels from LEVELS.  style 0: every block entirely +-32767; 1: single last-position coefficients; None: mixed."""
    import hevcdl_amd
    cx, cy = (w + 63) // 64, (h + 63) // 64
    recs = np.zeros(cx * cy, hevcdl_amd.REC_DTYPE)
    for a in range(cx * cy):
        r = recs[a]
        x0, y0 = (a % cx) * 64, (a // cx) * 64

        def tu(zb, cu_np, cu_log2, part, zrel, log2, trd, leaves):
            split = part == 3
            min_log2 = 2 if cu_log2 < 4 + split else min(5, cu_log2 - (2 + split))
            sub = log2 > 5 or (split and trd == 0) or (log2 > min_log2 and log2 > 2 and rng.integers(0, 2) == 1)
            if sub:
                for i in range(4):
                    tu(zb, cu_np, cu_log2, part, zrel + i * ((cu_np >> (2 * trd)) >> 2), log2 - 1, trd + 1, leaves)
            else:
                leaves.append((zrel, log2, trd))

        def cu(x, y, d, z):
            size = 64 >> d
            inside = x + size <= w and y + size <= h
            if d < 3 and (not inside or rng.integers(0, 3) != 0 if d < 2 else (not inside or rng.integers(0, 2) == 1)):
                for i in range(4):
                    sx, sy = x + (i & 1) * (size >> 1), y + (i >> 1) * (size >> 1)
                    if sx < w and sy < h:
                        cu(sx, sy, d + 1, z + i * (256 >> (2 * d + 2)))
                return
            n_p = 256 >> (2 * d)
            part = 3 if d == 3 and rng.integers(0, 2) else 0
            r["depth"][z:z + n_p] = d
            r["part_size"][z:z + n_p] = part
            if part == 3:
                for j in range(4):
                    r["luma_dir"][z + j] = rng.integers(0, 35)
            else:
                r["luma_dir"][z:z + n_p] = rng.integers(0, 35)
            allowed = [0, 26, 10, 1]
            luma0 = int(r["luma_dir"][z])
            allowed = [34 if m == luma0 else m for m in allowed] + [36]
            r["chroma_dir"][z:z + n_p] = allowed[rng.integers(0, 5)]
            leaves = []
            tu(z, n_p, 6 - d, part, 0, 6 - d, 0, leaves)
            group_nz = {}
            for zrel, log2, trd in leaves:
                np_t = n_p >> (2 * trd)
                r["tr_idx"][z + zrel:z + zrel + np_t] = trd
                st = style if style is not None else int(rng.integers(1, 6))
                nz = [style == 0 or rng.integers(0, 2) == 1 for _ in range(3)]
                if log2 == 2:      # the chroma of four 4x4 luma blocks is one 4x4 block each, coded with the last of the four
                    nz[1], nz[2] = group_nz.setdefault(zrel & ~3, (nz[1], nz[2]))
                for comp in range(3):
                    if not nz[comp]:
                        continue
                    for dd in range(trd + 1):
                        npd = n_p >> (2 * dd)
                        org = zrel & ~(npd - 1)
                        r["cbf"][comp][z + org:z + org + npd] |= 1 << dd
                    if comp == 0:
                        _fill_block(rng, r["coeff_y"], (z + zrel) * 16, 1 << log2, st)
                    elif log2 > 2:
                        _fill_block(rng, r["coeff_cb" if comp == 1 else "coeff_cr"], (z + zrel) * 4, 1 << (log2 - 1), st)
                    elif (zrel & 3) == 3:
                        _fill_block(rng, r["coeff_cb" if comp == 1 else "coeff_cr"], (z + (zrel & ~3)) * 4, 4, st)
                if log2 <= 3:
                    r["tskip"][:, z + zrel:z + zrel + np_t] = rng.integers(0, 2, (3, np_t))
        cu(x0, y0, 0, 0)
    return recs


def synth_sao(rng, ctus, bit_depth):
    import hevcdl_amd
    mx = (1 << (min(bit_depth, 10) - 5)) - 1
    p = np.zeros((ctus, 3), hevcdl_amd.SAO_DTYPE)
    for a in range(ctus):
        kind = rng.integers(0, 5)
        if kind < 2:      # both merges (the writer codes a merge only where its candidate exists)
            p[a]["mode"] = 2
            p[a]["type"] = kind
            continue
        for c in range(3):
            if c == 2:
                p[a, c]["mode"], p[a, c]["type"] = p[a, 1]["mode"], p[a, 1]["type"]
            else:
                p[a, c]["mode"] = rng.integers(0, 2)
                p[a, c]["type"] = rng.integers(0, 5)
            if p[a, c]["mode"] == 1:
                p[a, c]["aux"] = rng.integers(0, 32)
                p[a, c]["offset"][:] = rng.integers(-mx, mx + 1, 32)
    return p


@functools.lru_cache(maxsize=None)
def fuzz_corpus():
    """At least 200 seeded pictures of 1 to 12 CTUs: [(name, cfg, records [1, ctus], SAO parameters [1, ctus, 3] or None)] -- with and without tiles and wavefront, 8 and 10
    bits, each tool bit off once, with and without SAO; every size has its all-+-32767 picture and its last-position picture."""
    import hevcdl_amd
    rng = np.random.default_rng(20240611)
    out = []
    i = 0
    while len(out) < 204:
        w, h = FUZZ_SIZES[i % 6]
        style = 0 if i < 6 else (1 if i < 12 else None)
        bd = 10 if (i // 6) % 3 == 1 else 8
        tools = 0x7f if (i // 6) % 4 else 0x7f & ~(1 << ((i // 24) % 7))
        rows = (h + 63) // 64
        layout = (i // 6) % 5
        tiles, wpp = (1, 1), False
        if layout == 1:
            wpp = True
        elif layout == 2 and rows >= 2:
            tiles = (1, 2)
        elif layout == 3 and rows >= 3:
            tiles = ([(w + 63) // 64], [1, rows - 1])
        with_sao = (i // 6) % 2 == 1
        cfg = hevcdl_amd.stream_config(w, h, int(rng.integers(0, 52)), sao=with_sao, tiles=tiles, bit_depth=bd, tools=tools, wavefront=wpp)
        recs = synth_records(rng, w, h, style)[None]
        sao = synth_sao(rng, recs.shape[1], bd)[None] if with_sao else None
        out.append(("f%03d_%dx%d" % (i, w, h), cfg, recs, sao))
        i += 1
    return out


def garbage_records(seed, ctus):
    import hevcdl_amd
    rng = np.random.default_rng(seed)
    return np.frombuffer(rng.integers(0, 256, ctus * hevcdl_amd.REC_DTYPE.itemsize, dtype=np.uint8).tobytes(), hevcdl_amd.REC_DTYPE).copy()


def garbage_sao(seed, ctus):
    import hevcdl_amd
    rng = np.random.default_rng(seed)
    return np.frombuffer(rng.integers(0, 256, ctus * 3 * hevcdl_amd.SAO_DTYPE.itemsize, dtype=np.uint8).tobytes(), hevcdl_amd.SAO_DTYPE).reshape(ctus, 3).copy()
