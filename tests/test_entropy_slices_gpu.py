"""The device entropy coder (csrc/entropy_kernel.hip) under slice and segment layouts on the MI355X: the layout corpus of tests/entropy_cases.py in batched launches
against the host instantiation and through the decoder (oracle/slice_spec.py) straight from the device's buffer; the output stage's edges and the capacity guard on a
sub-stream that ends a dependent slice segment in mid-picture; the host fallback of such a picture.  Every picture is a few CTUs."""
import numpy as np
import pytest

import entropy_cases as ec
from test_entropy_gpu import same_coded

pytestmark = pytest.mark.gpu

SMALL = 6                                                                 # CTUs


def _decode_device(name, cfg, recs, sao, lay, dev, frame=0):
    """The decoder's segment entry on the device coder's own bytes (no host coder in between) -> the canonical records of frame `frame`."""
    decoded = ec.decode_layout_substreams(cfg, lay, ec.substreams_of(dev, frame))
    ec.assert_layout_round_trip(name, cfg, recs[frame], None if sao is None else sao[frame], lay, decoded)


@pytest.mark.parametrize("size", ["8x72", "72x72", "64x192"])
def test_small_layout_pictures_in_batched_launches(size):
    """The corpus pictures of at most 6 CTUs.  One launch per (size, layout): its first corpus picture gives configuration and layout, and the launch's frames are that
    picture and every other corpus picture of the size with its bit depth and SAO switch (records are valid under any QP and tool set; SAO offsets need the bit depth).
    Sizes and bytes are the host instantiation's, the canaries intact, no overflow word; and the decoder reads the canonical records of EVERY frame out of the device's
    buffer."""
    picks = [c for c in ec.layout_corpus() if c[0].split("_")[1] == size]
    assert picks and all(c[2].shape[1] <= SMALL for c in picks)
    launches = frames = 0
    seen = set()
    for name, cfg, recs, sao, lay in picks:
        lname = name.split("_")[-1]
        if lname in seen:
            continue
        seen.add(lname)
        group = [c for c in picks if c[1].bit_depth == cfg.bit_depth and (c[3] is None) == (sao is None)]
        group = [c for c in group if c[0] == name] + [c for c in group if c[0] != name]
        brecs = np.concatenate([c[2] for c in group])
        bsao = None if sao is None else np.concatenate([c[3] for c in group])
        dev = ec.code_layout(cfg, brecs, bsao, lay, device=0)
        ec.check_guard(dev)
        assert not dev[2].any() and same_coded(dev, ec.code_layout(cfg, brecs, bsao, lay)), name
        for f, c in enumerate(group):
            _decode_device("%s frame %d (%s)" % (name, f, c[0]), cfg, brecs, bsao, lay, dev, f)
        launches += 1
        frames += len(group)
    print("%s: %d launches, %d frames" % (size, launches, frames))
    assert launches < len(picks) or len(picks) == 1


def test_the_small_pictures_are_all_of_the_corpus_up_to_six_ctus():
    small = {c[0] for c in ec.layout_corpus() if c[2].shape[1] <= SMALL}
    assert small == {c[0] for c in ec.layout_corpus() if c[0].split("_")[1] in ("8x72", "72x72", "64x192")}


def _directed(which):
    import hevcdl_amd
    if which == "wavefront_3x3_sao_rows":                                 # the two-launch path, every row ending a segment
        name, cfg, recs, sao = ec.directed_pictures()[1]
        assert cfg.wavefront == 1 and recs.shape[1] == 9 and sao is not None
        return name, cfg, recs, sao, ec._lay(wavefront=True, segments=(1, 3))
    rng = np.random.default_rng(20241106)                                 # 10 bit, four tile rows in slices of two tiles in segments of one: 12 CTUs
    lay = ec._lay(tiles=(1, 4), slices=(3, 2), segments=(3, 1))
    cfg = hevcdl_amd.stream_config(136, 200, 33, sao=True, tiles=lay["tiles"], bit_depth=10)
    recs = ec.synth_records(rng, 136, 200)[None]
    return "tiles_in_slices_in_segments_10bit", cfg, recs, ec.synth_sao(rng, 12, 10)[None], lay


@pytest.mark.parametrize("which", ["wavefront_3x3_sao_rows", "tiles_in_slices_in_segments_10bit"])
def test_directed_pictures(which):
    name, cfg, recs, sao, lay = _directed(which)
    assert 9 <= recs.shape[1] <= 12
    borders = ec.segment_borders(cfg, lay)[0]
    assert [d for _, d, _, _ in borders] == ([0, 1, 1] if which.startswith("wavefront") else [0, 1, 0, 1])
    dev = ec.code_layout(cfg, recs, sao, lay, device=0)
    ec.check_guard(dev)
    assert not dev[2].any() and same_coded(dev, ec.code_layout(cfg, recs, sao, lay))
    _decode_device(name, cfg, recs, sao, lay, dev)


@pytest.mark.parametrize("variant,kind", sorted(ec.STAGE_SEEDS_SEGMENT))
def test_stage_edges_of_a_segment_ending_substream(variant, kind):
    """Sub-stream 0 of a 64x128 picture ends a dependent slice segment on, one byte behind and one byte before a 256-byte stage boundary, and with 1, 2, 3 bytes in its
    last dword.  First the host instantiation confirms the residue the committed seed is there for; then the device gives the same bytes inside intact canaries; and the
    same records WITHOUT the segment keys end sub-stream 0 differently (another length or other last bytes), so the seed sits on the new ending."""
    cfg, recs, lay, plain, length = ec.stage_segment_picture(variant, kind)
    borders = ec.segment_borders(cfg, lay)[0]
    assert [(a, d, n) for a, d, _, n in borders] == [(0, 0, 1), (1, 1, 1)]
    host = ec.code_layout(cfg, recs, None, lay)
    assert host[1].shape == (1, 2) and int(host[1][0, 0]) == length > 256
    want = {"on_boundary": length % 256 == 0, "one_past": length % 256 == 1, "one_before": length % 256 == 255, "tail_1": length % 4 == 1, "tail_2": length % 4 == 2, "tail_3": length % 4 == 3}
    assert want[kind]
    dev = ec.code_layout(cfg, recs, None, lay, device=0)
    ec.check_guard(dev)
    assert int(dev[1][0, 0]) == length and not dev[2].any() and ec.substreams_of(dev) == ec.substreams_of(host)
    old = ec.substreams_of(ec.code_layout(cfg, recs, None, plain))[0]
    new = ec.substreams_of(host)[0]
    assert len(old) != len(new) or old[-4:] != new[-4:]


@pytest.mark.parametrize("variant,kind", [("wavefront", "tail_3"), ("tiles", "one_past"), ("wavefront", "on_boundary")])
def test_capacity_edges_of_a_segment_ending_substream(variant, kind):
    """The capacity c of sub-stream 0's region on and beside its length L rounded down to a dword and the last stage boundary below L: the reported size is L, the
    overflow word is set exactly when L > c, the stored bytes are the head of the full sub-stream, the canaries are intact and the device result is the host's."""
    import hevcdl_amd
    cfg, recs, lay, _, length = ec.stage_segment_picture(variant, kind)
    layout, segments = ec.layout_keys(lay)
    full = ec.substreams_of(ec.code_layout(cfg, recs, None, lay))[0]
    assert len(full) == length
    l4, b = length & ~3, ((length - 1) // 256) * 256
    seen = set()
    for c in sorted({l4 - 4, l4, l4 + 4, b - 4, b, b + 4}):
        cpc = c - 64                                                      # sub-stream 0 is one CTU: its region holds capacity_per_ctu + 64 bytes
        assert cpc > 0 and cpc % 4 == 0 and int(hevcdl_amd.slice_data_layout(cfg, cpc, layout, segments)[3][0]) == c
        host, dev = ec.code_layout(cfg, recs, None, lay, capacity_per_ctu=cpc), ec.code_layout(cfg, recs, None, lay, capacity_per_ctu=cpc, device=0)
        for coded in (host, dev):
            ec.check_guard(coded)
            buf, sizes, ovf, off, cap = coded
            assert int(cap[0]) == c and int(sizes[0, 0]) == length and bool(ovf[0, 0]) == (length > c)
            n = min(length, c)
            assert buf[0, int(off[0]):int(off[0]) + n].tobytes() == full[:n]
        assert same_coded(dev, host)
        seen.add(length > c)
    assert seen == {False, True}


@pytest.mark.parametrize("variant", sorted(ec.STAGE_VARIANTS))
def test_host_fallback_of_a_segment_picture_decodes_to_its_records(variant):
    """encode_pictures_stream with a capacity of 8 bytes per CTU (hevcdl_set_entropy_capacity): the sub-streams overflow, the host codes the pictures under the context's
    segment layout, and the access units around that slice data decode, through decode_access_unit, to the records the call returned."""
    import hevcdl_amd
    import ref_tools
    import slice_spec as ss
    kw = ec.STAGE_VARIANTS[variant]
    lay = ec._lay(**kw)
    w, h, n = 64, 128, 2
    yuv = ref_tools.synth_yuv(w, h, n, seed=23)
    enc = hevcdl_amd.Encoder(w, h, 30, max_frames=n, **kw)
    try:
        enc.set_entropy_capacity(8)
        enc.enable_device_entropy(True)
        chunks = enc.encode_pictures_stream(yuv, sao=False, want_records=True)
        fallbacks = enc.entropy_info()[0]
        layout, segments = enc.slice_layout, enc.segment_layout
    finally:
        enc.close()
    assert fallbacks >= 1 and (segments.mode, segments.argument) == kw["segments"] and layout is None
    cfg = hevcdl_amd.stream_config(w, h, 30, tiles=lay["tiles"], wavefront=lay["wavefront"])
    seen = 0
    for first, data, sizes, _, _, recs in chunks:
        for i in range(len(data)):
            au = hevcdl_amd.write_access_unit_from_slice_data(cfg, first + i, data[i], sizes[i], None, layout=layout, segments=segments)
            out = ss.decode_access_unit(au)
            assert [(g["first_slice"], g["address"], g["dependent"]) for g in out[4]["segments"]] == [(1, 0, 0), (0, 1, 1)]
            ec.assert_layout_round_trip("%s picture %d" % (variant, first + i), cfg, recs[i], None, lay, out[:4])
            seen += 1
    assert seen == n
