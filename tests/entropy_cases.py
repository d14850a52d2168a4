"""Inputs of the entropy-coder tests (tests/test_entropy.py on the CPU, tests/test_entropy_gpu.py on the device): the golden fixtures as coder inputs, a seeded corpus of
synthetic records that no encode produces, garbage records, the helpers that turn coded slice data into access units, and (last section) the layout corpus: the
same kinds of pictures under every slice and segment layout the writer accepts (tests/test_entropy_slices_roundtrip.py, tests/test_entropy_slices_gpu.py)."""
import ctypes
import functools
import glob
import hashlib
import json
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
    """hevcdl_write_access_unit (the host's entry from records to an access unit) with a buffer that also holds pictures of maximal levels -> the frames' access units,
    joined."""
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


def input_digest(cfg, recs, sao):
    """SHA-256 of what a coder is given: stream configuration, records, SAO parameters."""
    h = hashlib.sha256(bytes(cfg))
    h.update(recs.tobytes())
    if sao is not None:
        h.update(sao.tobytes())
    return h.hexdigest()


def recorded_pictures():
    """The pictures of tests/golden/entropy_host_writer_digests.json (tools/record_entropy_host_writer_digests.py): [(name, cfg, records, SAO parameters or None)]."""
    return fuzz_corpus() + directed_pictures() + [("sao_" + name,) + sao_case(name) for name in SAO_CASES]


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(os.path.join(GOLD, "entropy_host_writer_digests.json")) as f:
        return json.load(f)["pictures"]


def assert_recorded_stream(name, cfg, recs, sao, stream):
    """`stream` (the frames' access units, joined) is what the host writer of the recorded commit -- the second coder this project had until then -- produced for
    the picture.  A picture that is no longer the recorded one fails as that, not as a coder difference."""
    entry = _recorded()[name]
    assert entry["input"] == input_digest(cfg, recs, sao), "%s is not the picture that was recorded: the corpus drifted (record again at a commit whose coder is trusted)" % name
    assert (len(stream), hashlib.sha256(stream).hexdigest()) == (entry["bytes"], entry["stream"]), "%s: the stream differs from the recorded one" % name


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


# ---- what a decoder can give back -----------------------------------------------------------------------------------------------------------------------
def _walk_blocks(r, x0, y0, w, h):
    """The transform blocks of one CTU record, by its depth map and tr_idx alone: (component, first coefficient, log2 of the block, prediction mode that picks its
    scan) for every block whose cbf bit is set.  Recursive over both trees, in any order: only the set of blocks matters here."""
    out = []

    def tu(z, zrel, log2, trd, np_cu, luma0):
        zz = z + zrel
        if log2 > 5 or (log2 > 2 and r["tr_idx"][zz] > trd):
            for i in range(4):
                tu(z, zrel + i * ((np_cu >> (2 * trd)) >> 2), log2 - 1, trd + 1, np_cu, luma0)
            return
        cd = int(r["chroma_dir"][z])
        mode_c = luma0 if cd == 36 else cd
        if (r["cbf"][0][zz] >> trd) & 1:
            out.append((0, zz * 16, log2, int(r["luma_dir"][zz])))
        for c in (1, 2):
            if log2 > 2 and (r["cbf"][c][zz] >> trd) & 1:
                out.append((c, zz * 4, log2 - 1, mode_c))
            elif log2 == 2 and (zrel & 3) == 3 and (r["cbf"][c][zz] >> trd) & 1:
                out.append((c, (z + (zrel & ~3)) * 4, 2, mode_c))

    def cu(x, y, d, z):
        if x >= w or y >= h:
            return
        size = 64 >> d
        if d < 3 and (r["depth"][z] > d or x + size > w or y + size > h):
            for i in range(4):
                cu(x + (i & 1) * (size >> 1), y + (i >> 1) * (size >> 1), d + 1, z + i * (256 >> (2 * d + 2)))
            return
        tu(z, 0, 6 - d, 0, 256 >> (2 * d), int(r["luma_dir"][z]))
    cu(x0, y0, 0, 0)
    return out


def canonical(cfg, recs, sao, mask, counts=None):
    """What a decoder of the slice data can give back of records [ctus] and SAO parameters [ctus, 3] (or None): -> (records, SAO parameters).  mask: the decoder's
    [ctus, 3, 256] mask of the tskip entries whose flag was in the stream.  counts: an optional dict that receives how many hidden signs differed from the input's.
    Dropped or changed, each because the bitstream does not carry it:
      * bits, dist, cost: statistics of the decision, never coded;
      * tskip outside the mask: transform_skip_flag exists only for 4x4 blocks with a coded coefficient and transform_skip_enabled_flag; the records of a larger
        block's partitions, of a block without coefficients and of the three further partitions of a 4x4 chroma block hold values no syntax element says;
      * the sign of the coefficient at the lowest scan position of a coefficient group whose first and last significant scan positions are at least 4 apart, with
        HEVCDL_TOOL_SIGN_HIDE: 7.3.8.11 sends no coeff_sign_flag for it, a decoder takes the parity of the group's absolute sum (odd: negative).  A level of -32768
        there that the parity turns positive does not fit 16 bits; as an int16 it reads -32768 again (the decoder counts such levels in level_out_of_range);
      * SAO: a merge candidate that does not exist cannot be named by the syntax -- the coder writes such a CTU as SAO off (mode 0) for all three components;
        of a merged CTU only mode 2 and left / above (in component 0) are coded; of a component that is off nothing but mode 0; of an edge offset only the
        magnitude (classes 0, 1 positive, 3, 4 negative by 7.4.9.3.2, class 2 none); of the 32 band offsets only the four from the band position on (modulo 32);
        Cr shares mode and edge class with Cb (sao_type_idx_chroma, sao_eo_class_chroma are coded once)."""
    import slice_spec as ss
    out = recs.copy()
    out["bits"], out["dist"], out["cost"] = 0, 0, 0
    out["tskip"] = np.where(mask, recs["tskip"], 0)
    w, h = cfg.width, cfg.height
    cx = (w + 63) // 64
    differed = 0
    if cfg.tools & 0x10:
        for a in range(len(out)):
            r = out[a]
            for comp, base, log2, mode in _walk_blocks(recs[a], (a % cx) * 64, (a // cx) * 64, w, h):
                plane = r[("coeff_y", "coeff_cb", "coeff_cr")[comp]]
                n = 1 << log2
                for sub in ss.block_scan(log2, ss.scan_idx_of(log2, comp, mode)):
                    vals = [int(plane[base + y * n + x]) for x, y in sub]
                    nz = [k for k, v in enumerate(vals) if v]
                    if nz and nz[-1] - nz[0] >= 4:
                        x, y = sub[nz[0]]
                        mag = abs(vals[nz[0]])
                        new = -mag if sum(abs(v) for v in vals) & 1 else mag
                        differed += (new < 0) != (vals[nz[0]] < 0)
                        plane[base + y * n + x] = np.int64(new).astype(np.int16)
    if counts is not None:
        counts["hidden_sign_differed"] = counts.get("hidden_sign_differed", 0) + differed
    if sao is None:
        return out, None
    import hevcdl_amd
    n_sub, _, _, _ = hevcdl_amd.slice_data_layout(cfg)
    _, _, _, cb, rb = hevcdl_amd.tile_layout(tiles_of_cfg(cfg), w, h)
    s = np.zeros_like(sao)
    for a in range(sao.shape[0]):
        p = sao[a]
        if p[0]["mode"] == 2:
            rx, ry = a % cx, a // cx
            have = (rx > 0 and rx not in cb) if p[0]["type"] == 0 else (ry > 0 and ry not in rb)
            if have and p[0]["type"] in (0, 1):
                s[a, 0]["mode"], s[a, 0]["type"] = 2, p[0]["type"]
            continue
        for c in range(3):
            src = p[c]
            if (p[1] if c == 2 else src)["mode"] != 1 if c == 2 else src["mode"] != 1:
                continue
            s[a, c]["mode"] = 1
            ty = int(p[1]["type"]) if c == 2 else int(src["type"])
            if ty == 4:
                s[a, c]["type"], s[a, c]["aux"] = 4, src["aux"] & 31
                for i in range(4):
                    k = (int(src["aux"]) + i) & 31
                    s[a, c]["offset"][k] = src["offset"][k]
            else:
                s[a, c]["type"] = ty
                for i, cls in enumerate((0, 1, 3, 4)):
                    s[a, c]["offset"][cls] = abs(int(src["offset"][cls])) * (1 if i < 2 else -1)
    return out, s


def tiles_of_cfg(cfg):
    """The tiles argument of stream_config back from a configuration: explicit sizes in CTUs of every tile column / row."""
    cx, cy = (cfg.width + 63) // 64, (cfg.height + 63) // 64
    if cfg.tile_uniform_spacing:
        return (cfg.tile_columns, cfg.tile_rows)
    cw = [cfg.tile_column_width[i] for i in range(cfg.tile_columns - 1)]
    rh = [cfg.tile_row_height[i] for i in range(cfg.tile_rows - 1)]
    return (cw + [cx - sum(cw)], rh + [cy - sum(rh)])


@functools.lru_cache(maxsize=None)
def directed_pictures():
    """Seeded pictures for what fuzz_corpus cannot reach: tile COLUMNS (a tile column is at least four CTUs wide, so the picture is eight: the left neighbour of a
    CTU, a CU and a prediction block lies in another tile; the reference decoder takes it too), a 3x3-CTU
    wavefront picture with SAO and a 10-bit picture with two tile rows and SAO (both also decoded from the device coder's output)."""
    import hevcdl_amd
    rng = np.random.default_rng(20240907)
    out = []
    for name, w, h, bd, kw in (("d0_456x64_t2x1", 456, 64, 8, {"tiles": (2, 1)}), ("d1_136x136_wpp", 136, 136, 8, {"wavefront": True}), ("d2_136x200_t1x2", 136, 200, 10, {"tiles": (1, 2)})):
        cfg = hevcdl_amd.stream_config(w, h, int(rng.integers(20, 40)), sao=True, bit_depth=bd, **kw)
        recs = synth_records(rng, w, h)[None]
        out.append((name, cfg, recs, synth_sao(rng, recs.shape[1], bd)[None]))
    return out


# One-CTU pictures (64x64, QP 30, one sub-stream) whose slice data ends on, one byte behind and one byte before a boundary of the device coder's 256-byte output stage,
# and with 1, 2 and 3 bytes in the last dword: (seed of synth_records, length in bytes).  Found by a search over the seeds 1, 2, 3, ...; the tests assert the residues.
STAGE_SEEDS = {"on_boundary": (104, 1792), "one_past": (217, 1793), "one_before": (97, 1535), "tail_1": (3, 1041), "tail_2": (2, 898), "tail_3": (7, 1311)}


def stage_picture(kind):
    import hevcdl_amd
    seed, length = STAGE_SEEDS[kind]
    return hevcdl_amd.stream_config(64, 64, 30), synth_records(np.random.default_rng(seed), 64, 64)[None], length


def flat_picture():
    """8x8, every cbf zero, DC prediction: the whole slice data is two or three bytes."""
    import hevcdl_amd
    recs = np.zeros((1, 1), hevcdl_amd.REC_DTYPE)
    recs["depth"][..., 0:4] = 3
    recs["luma_dir"][..., 0:4] = 1
    recs["chroma_dir"][..., 0:4] = 36
    return hevcdl_amd.stream_config(8, 8, 30), recs


def substreams_of(coded, poc=0):
    """code_slice_data's result -> the sub-streams of picture poc as byte strings (none may have overflowed)."""
    buf, sizes, ovf, off, cap = coded
    assert not ovf[poc].any()
    return [buf[poc, int(o):int(o) + int(n)].tobytes() for o, n in zip(off, sizes[poc])]


_DECODED = {}


def cached_decode_picture(subs, width, height, qp, tools, bit_depth, col_bd, row_bd, wavefront, sao, strict_levels=False, **sps):
    """slice_spec.decode_picture behind a table of its results: the decoder is deterministic and slow, so the same bytes with the same parameters -- the same picture
    coming from another writer or through the access-unit entry -- are decoded once.  Callers do not change what they get."""
    import slice_spec
    key = (tuple(subs), width, height, qp, tools & 0x14, bit_depth, tuple(col_bd), tuple(row_bd), bool(wavefront), bool(sao), bool(strict_levels), tuple(sorted(sps.items())))
    if key not in _DECODED:
        try:
            _DECODED[key] = slice_spec.decode_picture(subs, width, height, qp, tools, bit_depth, col_bd, row_bd, wavefront, sao, strict_levels=strict_levels, **sps)
        except slice_spec.SliceError as e:
            _DECODED[key] = e
    if isinstance(_DECODED[key], Exception):
        raise _DECODED[key]
    return _DECODED[key]


SPS_OF_THE_PRODUCT = {"min_cb_log2": 3, "ctb_log2": 6, "min_tb_log2": 2, "max_tb_log2": 5, "max_th_depth_intra": 2}      # what the access-unit entry reads from the SPS


def decode_substreams(cfg, subs, strict_levels=False):
    """The decoder's picture entry for sub-streams coded under cfg -> (records, SAO parameters, tskip mask, tally)."""
    import hevcdl_amd
    _, _, _, cb, rb = hevcdl_amd.tile_layout(tiles_of_cfg(cfg), cfg.width, cfg.height)
    return cached_decode_picture(subs, cfg.width, cfg.height, cfg.qp, cfg.tools, cfg.bit_depth, cb, rb, bool(cfg.wavefront), bool(cfg.sao_enabled), strict_levels=strict_levels, **SPS_OF_THE_PRODUCT)


RT_FIELDS = ("depth", "part_size", "luma_dir", "chroma_dir", "tr_idx", "cbf", "tskip", "coeff_y", "coeff_cb", "coeff_cr")


def assert_round_trip(name, cfg, recs, sao, decoded, counts=None):
    """The decoder's result == the canonical form of the coder's input, field by field."""
    got, gsao, mask, _ = decoded
    want, wsao = canonical(cfg, recs, sao, mask, counts)
    for k in RT_FIELDS:
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %s" % (name, k, np.argwhere(got[k] != want[k])[:4].tolist())
    assert (gsao is None) == (wsao is None)
    if wsao is not None:
        assert np.array_equal(gsao, wsao), "%s: SAO parameters differ at CTU %s" % (name, [a for a in range(len(wsao)) if not np.array_equal(gsao[a], wsao[a])][:4])


# ---- pictures of several slices and slice segments ----------------------------------------------------------------------------------------------------------------
def _lay(tiles=(1, 1), wavefront=False, slices=None, lf_across_slices=True, segments=None, choice=None, lf_offsets=(0, 0)):
    """A layout: what hevcdl_write_access_unit_segments is told besides the picture.  slices (SliceMode, SliceArgument), segments (SliceSegmentMode, SliceSegmentArgument),
    choice: a hevcdl_dbk_choice 5-tuple (LoopFilterOffsetInPPS 0: every independent header repeats the deblocking fields behind an override flag)."""
    return {"tiles": tiles, "wavefront": wavefront, "slices": slices, "lf_across_slices": lf_across_slices, "segments": segments, "choice": choice, "lf_offsets": lf_offsets}


def layout_keys(lay):
    """-> (layout=, segments=) of code_slice_data / write_access_unit_from_slice_data."""
    import hevcdl_amd
    return hevcdl_amd.slice_layout(lay["slices"], lay["lf_across_slices"]), lay["segments"]


def segment_borders(cfg, lay):
    """What the layout says about the picture's NAL units, from the keys' definitions (not from the coder's grid): -> ([(slice_segment_address, dependent flag, first
    sub-stream, sub-streams)] in decoding order, (col_bd, row_bd) of the tiles the PPS declares, wavefront).  A sub-stream is a tile, a wavefront row or -- SliceMode 1,
    whose PPS has no tiles -- a whole slice of CTU rows."""
    import hevcdl_amd
    cx, cy = (cfg.width + 63) // 64, (cfg.height + 63) // 64
    _, _, _, cb, rb = hevcdl_amd.tile_layout(lay["tiles"], cfg.width, cfg.height)
    slices, segs = lay["slices"], lay["segments"]
    if slices and slices[0] == 1:
        rows = slices[1] // cx
        return [(r * cx, 0, i, 1) for i, r in enumerate(range(0, cy, rows))], ([0, cx], [0, cy]), False
    if lay["wavefront"]:
        addr = [r * cx for r in range(cy)]
    else:
        addr = [rb[ty] * cx + cb[tx] for ty in range(len(rb) - 1) for tx in range(len(cb) - 1)]
    per = slices[1] if slices else len(addr)
    seg = (segs[1] // cx if segs[0] == 1 else segs[1]) if segs else per
    out = []
    for k0 in range(0, len(addr), per):
        k1 = min(k0 + per, len(addr))
        for s0 in range(k0, k1, seg):
            out.append((addr[s0], int(s0 > k0), s0, min(s0 + seg, k1) - s0))
    return out, (cb, rb), bool(lay["wavefront"])


def code_layout(cfg, recs, sao, lay, **kw):
    import hevcdl_amd
    layout, segments = layout_keys(lay)
    return hevcdl_amd.code_slice_data(cfg, recs, sao, layout=layout, segments=segments, **kw)


_DECODED_SEGMENTS = {}


def cached_decode_picture_segments(segments, width, height, qp, tools, bit_depth, col_bd, row_bd, wavefront, sao, strict_levels=False, **kw):
    """slice_spec.decode_picture_segments behind a table of its results, as cached_decode_picture is for the one-segment entry."""
    import slice_spec
    segments = tuple((int(a), int(d), tuple(bytes(b) for b in subs)) for a, d, subs in segments)
    key = (segments, width, height, qp, tools & 0x14, bit_depth, tuple(col_bd), tuple(row_bd), bool(wavefront), bool(sao), bool(strict_levels), tuple(sorted(kw.items())))
    if key not in _DECODED_SEGMENTS:
        try:
            _DECODED_SEGMENTS[key] = slice_spec.decode_picture_segments(segments, width, height, qp, tools, bit_depth, col_bd, row_bd, wavefront, sao, strict_levels=strict_levels, **kw)
        except slice_spec.SliceError as e:
            _DECODED_SEGMENTS[key] = e
    if isinstance(_DECODED_SEGMENTS[key], Exception):
        raise _DECODED_SEGMENTS[key]
    return _DECODED_SEGMENTS[key]


def decode_layout_substreams(cfg, lay, subs, strict_levels=False, **mutants):
    """The decoder's segment entry on sub-streams coded under cfg and the layout (straight from code_slice_data's buffer) -> (records, SAO parameters, tskip mask, tally)."""
    borders, (cb, rb), wpp = segment_borders(cfg, lay)
    assert sum(n for _, _, _, n in borders) == len(subs)
    segments = [(a, d, subs[k:k + n]) for a, d, k, n in borders]
    kw = dict(SPS_OF_THE_PRODUCT)
    kw.update(mutants)
    return cached_decode_picture_segments(segments, cfg.width, cfg.height, cfg.qp, cfg.tools, cfg.bit_depth, cb, rb, wpp, bool(cfg.sao_enabled), strict_levels=strict_levels, **kw)


def write_layout_access_units(cfg, recs, sao, lay, coded=None):
    """-> (hevcdl_write_access_unit_segments from the records, hevcdl_write_access_unit_from_slice_data_segments around the shared coder's sub-streams) of picture 0."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    wcfg = hevcdl_amd.stream_config(cfg.width, cfg.height, cfg.qp, sao=sao is not None, tiles=lay["tiles"], bit_depth=cfg.bit_depth, tools=cfg.tools, lf_offsets=lay["lf_offsets"],
                                    wavefront=lay["wavefront"])
    assert bytes(wcfg) == bytes(cfg)
    layout, segments = layout_keys(lay)
    segments = hevcdl_amd.segment_layout(segments)
    cap = cfg.width * cfg.height * 12 + (1 << 16)                         # as host_writer_stream: room for pictures of maximal levels, which hevcdl_access_unit_bound does not give
    buf, n = np.zeros(cap, np.uint8), ctypes.c_size_t(0)
    cp, _keep = hevcdl_amd._choice_ptr(lay["choice"])
    r, p = np.ascontiguousarray(recs[0]), None if sao is None else np.ascontiguousarray(sao[0])
    st = lib.hevcdl_write_access_unit_segments(ctypes.byref(cfg), hevcdl_amd._layout_ptr(layout), hevcdl_amd._layout_ptr(segments), 0, r.ctypes.data, None if p is None else p.ctypes.data, cp,
                                               buf.ctypes.data, cap, ctypes.byref(n))
    assert st == 0, st
    a = buf[:n.value].tobytes()
    coded = coded or code_layout(cfg, recs, sao, lay)
    buf, sizes, ovf, off, cap = coded
    assert not ovf.any()
    b = hevcdl_amd.write_access_unit_from_slice_data(cfg, 0, hevcdl_amd.pack_slice_data(buf[0], sizes[0], off), sizes[0], choice=lay["choice"], layout=layout, segments=segments)
    return a, b


def layouts_of(cx, cy):
    """The layouts hevcdl_write_access_unit_segments accepts on a picture of cx x cy CTUs (cy >= 2), by what each is there for."""
    rows_t = (1, cy)                                                      # a tile per CTU row (a tile column needs four CTUs: rows are what small pictures have)
    out = [("rs1", _lay(slices=(1, cx))),                                                           # row slices of one row
           ("rs1lf0", _lay(slices=(1, cx), lf_across_slices=False)),
           ("ts1", _lay(tiles=rows_t, slices=(3, 1))),                                             # slices of one tile
           ("ws1", _lay(wavefront=True, segments=(1, cx))),                                        # wavefront segments of one row
           ("tg1", _lay(tiles=rows_t, segments=(3, 1))),                                           # tile segments alone
           ("rs1dbk", _lay(slices=(1, cx), choice=(1, 1, 0, 2, -1), lf_offsets=(2, -1))),          # LoopFilterOffsetInPPS 0: deblocking fields in every independent header
           ("ws1dbk", _lay(wavefront=True, segments=(1, cx), choice=(1, 1, 1, 0, 0)))]             # ... with the filter disabled by the slice
    if cy >= 3:
        out += [("rs2", _lay(slices=(1, 2 * cx), lf_across_slices=cy == 3)),                        # several rows; 3 rows: a shorter last slice
                ("ts2", _lay(tiles=rows_t, slices=(3, 2))),                                        # 2 or more tiles a slice; the last takes what is left
                ("ws2", _lay(wavefront=True, segments=(1, 2 * cx))),                               # several rows a segment (3 rows: a shorter last segment)
                ("tg2", _lay(tiles=rows_t, segments=(3, 2))),
                ("ts2g1", _lay(tiles=rows_t, slices=(3, 2), segments=(3, 1))),                     # tile segments inside tile slices
                ("ts3g2", _lay(tiles=rows_t, slices=(3, 3), segments=(3, 2), choice=(1, 1, 0, -3, 4), lf_offsets=(-3, 4)))]      # a segment cut short at its slice's end
    return out


LAYOUT_SIZES = [s for s in FUZZ_SIZES if s[1] > 64]                       # two CTU rows or more: (8, 72), (72, 72), (136, 200), (200, 136)
# directed: twelve tiles in slices of five in segments of two (5 + 5 + 2 tiles -> 3 + 3 + 1 segments), tile COLUMNS in slices in segments (a slice border to the LEFT of a
# CTU), a one-CTU-wide wavefront picture of three rows
LAYOUT_DIRECTED = [("t12s5g2", 64, 768, _lay(tiles=(1, 12), slices=(3, 5), segments=(3, 2))),
                   ("c2s1", 456, 64, _lay(tiles=(2, 1), slices=(3, 1), lf_across_slices=False)),
                   ("c2g1", 520, 64, _lay(tiles=(2, 1), segments=(3, 1))),
                   ("w1x3", 64, 192, _lay(wavefront=True, segments=(1, 1)))]


@functools.lru_cache(maxsize=None)
def layout_corpus():
    """Seeded pictures of at most 12 CTUs under every layout of layouts_of and LAYOUT_DIRECTED: [(name, cfg, records [1, ctus], SAO parameters [1, ctus, 3] or None,
    layout)].  Styles as in fuzz_corpus (all +-32767, last position, mixed), 8 and 10 bits, SAO on and off; the attributes cycle with periods that share no factor with
    the number of layouts of a size, so that each layout meets each of them."""
    import hevcdl_amd
    rng = np.random.default_rng(20241105)
    out = []
    i = 0
    for rnd in range(3):
        for w, h in LAYOUT_SIZES:
            for lname, lay in layouts_of((w + 63) // 64, (h + 63) // 64):
                if rnd >= 1 and lname in ("rs1lf0", "rs1dbk", "ws1dbk"):
                    continue
                style = (0 if i % 11 == 3 else (1 if i % 11 == 7 else (2 if i % 4 == 1 or (rnd >= 1 and lname in ("ws2", "tg2")) else None)))      # (flat rows under a dependent header's entry points)
                if style == 0 and w * h > 136 * 136:                      # an all-+-32767 picture of 12 CTUs is 100 KB of slice data: 4 CTUs carry the same paths
                    style = None
                bd = 10 if i % 3 == 1 else 8
                with_sao = i % 2 == 0
                tools = 0x7f if i % 5 else 0x7f & ~(0x04 if i % 10 else 0x10)
                out.append(_layout_picture(rng, "%s%02d_%dx%d_%s" % ("M" if style == 0 else "L", i, w, h, lname), w, h, lay, style, bd, with_sao, tools))
                i += 1
    for k, (lname, w, h, lay) in enumerate(LAYOUT_DIRECTED):
        out.append(_layout_picture(rng, "%s%d_%dx%d_%s" % ("M" if lname == "w1x3" else "D", k, w, h, lname), w, h, lay, 0 if lname == "w1x3" else (2 if k == 0 else None), 10 if k == 1 else 8, k != 2, 0x7f))
    return out


def flatten_ctu(r, x0, y0, w, h):
    """One CTU record made flat: 8x8 CUs, planar prediction (the first candidate wherever the neighbours are flat or missing), chroma from luma, no coefficient.  Every bin
    of such a CTU is soon the more probable one and every bypass bin 0, so the arithmetic coder's low stays 0 and it writes zero bytes: the slice data then needs
    emulation prevention bytes, which natural content of a few KB almost never does."""
    for k in ("part_size", "luma_dir", "tr_idx", "cbf", "tskip", "coeff_y", "coeff_cb", "coeff_cr", "depth", "chroma_dir"):
        r[k][...] = 0
    for y4 in range(min(16, (h - y0) // 4)):
        for x4 in range(min(16, (w - x0) // 4)):
            z = _z_of(x4, y4)
            r["depth"][z], r["chroma_dir"][z] = 3, 36


def _layout_picture(rng, name, w, h, lay, style, bd, with_sao, tools):
    """style 2: mixed records with every even CTU row flat (flatten_ctu)."""
    import hevcdl_amd
    cfg = hevcdl_amd.stream_config(w, h, int(rng.integers(0, 52)), sao=with_sao, tiles=lay["tiles"], bit_depth=bd, tools=tools, wavefront=lay["wavefront"], lf_offsets=lay["lf_offsets"])
    recs = synth_records(rng, w, h, None if style == 2 else style)[None]
    if style == 2:
        cx = (w + 63) // 64
        for a in range(recs.shape[1]):
            if (a // cx) % 2 == 0:
                flatten_ctu(recs[0, a], (a % cx) * 64, (a // cx) * 64, w, h)
    sao = synth_sao(rng, recs.shape[1], bd)[None] if with_sao else None
    return name, cfg, recs, sao, lay


def canonical_layout(cfg, recs, sao, mask, lay):
    """canonical() for a picture of slices: a SAO merge candidate in another slice does not exist either.  canonical() knows tile borders from the cfg; the borders of
    slices are added here from segment_borders (the first CTU row / column of every independent segment's rectangle)."""
    out, s = canonical(cfg, recs, sao, mask)
    if sao is None:
        return out, s
    borders, (cb, rb), _ = segment_borders(cfg, lay)
    cx = (cfg.width + 63) // 64
    starts = sorted(a for a, d, _, _ in borders if not d)
    for a in range(sao.shape[0]):
        if sao[a][0]["mode"] != 2 or s[a, 0]["mode"] != 2:
            continue
        nb = a - 1 if sao[a][0]["type"] == 0 else a - cx
        if _slice_of(cfg, lay, starts, a) != _slice_of(cfg, lay, starts, nb):
            s[a] = np.zeros(3, s.dtype)
    return out, s


def _slice_of(cfg, lay, starts, rs):
    """SliceAddrRs of a CTU: the independent segment whose tiles / rows hold it.  Row slices and wavefront: the last start at or below rs; tiles: the start of the slice
    that the CTU's tile belongs to."""
    import hevcdl_amd
    cx = (cfg.width + 63) // 64
    _, _, _, cb, rb = hevcdl_amd.tile_layout(lay["tiles"], cfg.width, cfg.height)
    if len(cb) == 2 and len(rb) == 2:
        return max(a for a in starts if a <= rs)
    rx, ry = rs % cx, rs // cx
    tx, ty = max(i for i in range(len(cb) - 1) if rx >= cb[i]), max(j for j in range(len(rb) - 1) if ry >= rb[j])
    tile = ty * (len(cb) - 1) + tx
    per = lay["slices"][1] if lay["slices"] else (len(cb) - 1) * (len(rb) - 1)
    first = (tile // per) * per
    return rb[first // (len(cb) - 1)] * cx + cb[first % (len(cb) - 1)]


def assert_layout_round_trip(name, cfg, recs, sao, lay, decoded):
    got, gsao, mask, _ = decoded
    want, wsao = canonical_layout(cfg, recs, sao, mask, lay)
    for k in RT_FIELDS:
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %s" % (name, k, np.argwhere(got[k] != want[k])[:4].tolist())
    assert (gsao is None) == (wsao is None)
    if wsao is not None:
        assert np.array_equal(gsao, wsao), "%s: SAO parameters differ at CTU %s" % (name, [a for a in range(len(wsao)) if not np.array_equal(gsao[a], wsao[a])][:4])


# 64x128 pictures (two CTUs, QP 30) whose sub-stream 0 ends a dependent slice segment in mid-slice -- end_of_slice_segment_flag 1 and rbsp_slice_segment_trailing_bits()
# where the same sub-stream without the segment keys writes flag 0, end_of_subset_one_bit and byte_alignment() -- on the edges of the device coder's output stage, in the
# wavefront variant (segments (1, 1): the two-launch path) and the tile-rows variant (tiles (1, 2), segments (3, 1)): (seed of synth_records, length of sub-stream 0).
# Found by a search over the seeds 1, 2, 3, ... with the host coder; the tests assert the residues.
STAGE_VARIANTS = {"wavefront": {"wavefront": True, "segments": (1, 1)}, "tiles": {"tiles": (1, 2), "segments": (3, 1)}}
STAGE_SEEDS_SEGMENT = {(v, k): s for v in STAGE_VARIANTS for k, s in
                       {"on_boundary": (104, 1792), "one_past": (217, 1793), "one_before": (97, 1535), "tail_1": (3, 1041), "tail_2": (2, 898), "tail_3": (1, 1543)}.items()}


def stage_segment_picture(variant, kind):
    """-> (cfg, records [1, 2], layout, the same layout without the segment keys, length of sub-stream 0)."""
    import hevcdl_amd
    seed, length = STAGE_SEEDS_SEGMENT[(variant, kind)]
    lay = _lay(**STAGE_VARIANTS[variant])
    cfg = hevcdl_amd.stream_config(64, 128, 30, tiles=lay["tiles"], wavefront=lay["wavefront"])
    plain = dict(lay)
    plain["segments"] = None
    return cfg, synth_records(np.random.default_rng(seed), 64, 128)[None], lay, plain, length
