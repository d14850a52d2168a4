"""The launches whose form tests/golden/rd_launch_forms.json records (tools/record_rd_launch_forms.py writes it, tests/test_rd_plan.py replays it through
csrc/rd_launch_plan.h on the CPU, tests/test_rd_gpu.py makes the launches again): tiny pictures, one real launch of the decision kernel each, and the string
hevcdl_last_rd_launch reports afterwards.  The frame counts are chosen for 256 CUs: each pair named in PAIRS sits either side of a threshold of the launch plan."""
import numpy as np

NO_HANDOVER, WIDE, NARROW = 1, 2, 4      # HEVCDL_EXEC_*
TOOLS_OTHER = 0x7f & ~0x04                # the reference's tools without transform skip: the context runs the tools build

FORMS = ["independent", "unit-handover", "few-units(passes)", "few-units(passes+chroma)", "few-units(passes while takers idle)", "wavefront-rows",
         "wavefront-rows+few-units", "wavefront(one wave per frame)"]
BUILDS = ["hevcdl_rd_frame_kernel", "hevcdl_rd_frame_kernel_wide", "hevcdl_rd_frame_kernel_tools", "hevcdl_rd_frame_kernel_bd10"]


def _ctx(width=64, height=64, max_frames=1, tiles=(1, 1), wavefront=0, bit_depth=8, tools=0x7f, exec_flags=0):
    return dict(width=width, height=height, max_frames=max_frames, tiles=list(tiles), wavefront=wavefront, bit_depth=bit_depth, tools=tools, exec_flags=exec_flags)


def cases():
    """-> list of dicts: a name, the context's configuration, the call ("frames", "tiles" with tile_begin / tile_count, or "ctu") and n_frames."""
    out = []

    def add(group, ctx, counts, call="frames", **kw):
        for n in counts:
            out.append(dict(name="%s-%d" % (group, n), call=call, n_frames=n, **ctx, **kw))
    add("plain", _ctx(max_frames=1100), [1, 11, 12, 128, 129, 170, 171, 256, 300, 512, 600, 767, 768, 900, 1024, 1100])
    add("tiles", _ctx(256, 128, 384, tiles=(1, 2)), [5, 6, 85, 86, 150, 384])
    add("wavefront", _ctx(128, 192, 400, wavefront=1), [1, 50, 100, 400])
    add("wavefront-no-handover", _ctx(128, 192, 400, wavefront=1, exec_flags=NO_HANDOVER), [4])
    add("ten-bit", _ctx(max_frames=300, bit_depth=10), [1, 300])
    add("tools", _ctx(max_frames=900, tools=TOOLS_OTHER), [1, 900])
    add("forced-wide", _ctx(max_frames=300, exec_flags=WIDE), [1, 300])
    add("forced-narrow", _ctx(max_frames=900, exec_flags=NARROW), [900])
    add("no-handover", _ctx(max_frames=300, exec_flags=NO_HANDOVER), [1, 300])
    add("large-context", _ctx(max_frames=2048), [1])
    add("tile-range", _ctx(256, 128, 384, tiles=(1, 2)), [6], call="tiles", tile_begin=1, tile_count=1)
    add("session-wavefront", _ctx(128, 192, 1, wavefront=1), [1], call="ctu")
    add("session", _ctx(128, 192, 1), [1], call="ctu")
    return out


# pairs of frame counts either side of a threshold: their recorded strings must differ in form or build
PAIRS = [("plain-11", "plain-12"), ("plain-128", "plain-129"), ("plain-170", "plain-171"), ("plain-767", "plain-768"),
         ("tiles-5", "tiles-6"), ("tiles-85", "tiles-86")]

CONTEXT_KEYS = ("width", "height", "max_frames", "tiles", "wavefront", "bit_depth", "tools", "exec_flags")


def context_key(case):
    return tuple(tuple(case[k]) if isinstance(case[k], list) else case[k] for k in CONTEXT_KEYS)


def form_of(launch):
    return launch.split(" form=")[1].split(" workgroups=")[0]


def build_of(launch):
    return launch.split(" ")[0]


def check_coverage(by_name):
    """The conditions on a recorded file: every form and every build at least once, every pair differs in form or build.  by_name: {case name: string}."""
    forms, builds = {form_of(s) for s in by_name.values()}, {build_of(s) for s in by_name.values()}
    assert forms == set(FORMS), "forms not reached: %s" % sorted(set(FORMS) - forms)
    assert builds == set(BUILDS), "builds not reached: %s" % sorted(set(BUILDS) - builds)
    for a, b in PAIRS:
        assert (form_of(by_name[a]), build_of(by_name[a])) != (form_of(by_name[b]), build_of(by_name[b])), "%s and %s do not straddle a threshold: %s" % (a, b, by_name[a])


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def build_waves():
    """{build name: wavefronts per workgroup} of the loaded library's four builds (host functions of the kernels' translation units: no GPU needed)."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    return {b: int(getattr(lib, b.replace("hevcdl_rd_frame_kernel", "hevcdl_rd_waves_per_group"))()) for b in BUILDS}


def run_cases(case_list):
    """Make the launches (GPU) -> {case name: hevcdl_last_rd_launch string}.  One context per configuration, flat grey pictures and depth-0 labels:
    the form of a launch does not depend on the content."""
    import torch
    import hevcdl_amd
    torch.cuda.init()      # torch's HIP runtime before the library's first use of the GPU (tests/conftest.py)
    encs, out = {}, {}
    for c in case_list:
        key = context_key(c)
        if key not in encs:
            cfg = hevcdl_amd.default_config(c["width"], c["height"], 32, max_frames=c["max_frames"], tiles=tuple(c["tiles"]), bit_depth=c["bit_depth"],
                                            tools=c["tools"], wavefront=bool(c["wavefront"]))
            cfg.exec_flags = c["exec_flags"]
            encs[key] = hevcdl_amd.Encoder(c["width"], c["height"], 32, cfg=cfg)
        enc, n = encs[key], c["n_frames"]
        yuv = np.full((n, enc.frame_samples), 128 << (enc.bit_depth - 8), enc.sample_dtype)
        labels = np.zeros((n, enc.ctus, 16), np.uint8)
        if c["call"] == "frames":
            enc.compress_frames(yuv, labels)
        elif c["call"] == "ctu":
            enc.begin_frames(yuv, labels)
            enc.compress_ctu(0, 0)
        else:
            dev = torch.device("cuda:0")
            d_yuv, d_lab = torch.from_numpy(yuv.view(np.uint8).reshape(n, -1)).to(dev), torch.from_numpy(labels).to(dev)
            d_recs = torch.zeros((n, enc.ctus * hevcdl_amd.REC_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            d_recon, d_stats = torch.zeros_like(d_yuv), torch.zeros((n, hevcdl_amd.STATS_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            enc.compress_tiles_dev(d_yuv.data_ptr(), n, d_lab.data_ptr(), d_recs.data_ptr(), d_recon.data_ptr(), d_stats.data_ptr(), c["tile_begin"], c["tile_count"])
            torch.cuda.synchronize()
        out[c["name"]] = enc.last_rd_launch()
    for enc in encs.values():
        enc.close()
    return out
