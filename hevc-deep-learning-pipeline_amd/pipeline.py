"""Whole-sequence encode over one or more GPUs (one process per GPU): the host loop of the reference's TAppEncTop::encode /
TEncGOP::compressGOP for the all-intra configuration, on top of the C ABI.

Per batch of pictures: CNN labels (or label files) -> CTU decisions -> deblocking -> SAO -> access units (+ MD5 SEI) and the
reference's log line.  Across ranks the pictures shard by contiguous frame ranges (`sharding.shard_frames`): every rank writes
the access units of its own pictures; rank 0 concatenates the parts in POC order (all-intra pictures are independent: IDR at POC 0,
CRA afterwards, parameter sets re-sent with every picture, so the shards ARE the single-process stream) and prints the summary from
the gathered per-frame rows (`sharding.gather_frame_summaries`) -- the only collective, 40 bytes per picture.
"""
import os
import time

import numpy as np

from . import Encoder, write_access_unit, picture_hash_sei, stream_config, write_access_unit_from_slice_data, hash_sei as digest_sei, report_digest
from . import load_source_host, store_output_host, source_format as make_source_format
from . import metrics, sharding


_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=min(32, os.cpu_count() or 1))
    return _POOL


def read_frames(path, width, height, first, count, bit_depth=8, frame_samples=None):
    """Planar 4:2:0 frames [count, w*h*3/2] (uint8, or uint16 little endian for bit_depth 10) starting at frame `first`.  frame_samples: the samples of a frame of
    another file format (SourceFormat.source_samples)."""
    dt = np.uint8 if bit_depth == 8 else np.dtype("<u2")
    n = frame_samples or width * height * 3 // 2
    with open(path, "rb") as f:
        f.seek(first * n * (1 if bit_depth == 8 else 2))
        a = np.fromfile(f, dt, n * count)
    if a.size != n * count:
        raise ValueError("short read of %s: wanted %d frames from frame %d" % (path, count, first))
    return a.reshape(count, n)


def encode_sequence(input_path, width, height, qp, n_frames, bitstream_path=None, recon_path=None, frame_skip=0, batch=256, tiles=(1, 1),
                    lf_across_tiles=True, bit_depth=8, level_idc=186, frame_rate=30.0, hash_sei=False, labels_fn=None, device=None, log=print, tools=0x7f, wavefront=False, device_entropy=False, device_report=False, source_format=None,
                    deblocking_metric=0, lf_offset_in_pps=True, slices=None, lf_across_slices=True, segments=None, delta_qp_rd=0, frame_qps=None, lambda_modifier=1.0):
    """Encode frames [frame_skip, frame_skip + n_frames) of a planar YUV file.  Works stand-alone and under torch.distributed
    (initialised by the caller): rank r takes a contiguous share of the frames.  Returns, on rank 0, the summary (metrics.Summary)
    and the list of per-picture rows [poc, bits, sseY, sseU, sseV]; other ranks return (None, None).
    labels_fn(first_poc, count) -> uint8 [count, ctus, 16] replaces the on-device CNN (the reference's label files).
    device_entropy: the slice data is coded on the device (Encoder.enable_device_entropy) and the host only writes what surrounds it; the stream is the same bytes.
    This takes the arithmetic coder off the host threads; alone it saves no copies, since this function then still needs the pictures (hash, SSE) and fetches records and
    SAO parameters with them through encode_pictures.
    device_report: the squared errors and the hash SEI's digests come from the device too (Encoder.enable_picture_report), computed where the output picture is.  Together
    with device_entropy and without a recon_path nothing but slice data, statistics and the 80-byte reports leaves HBM: the batch goes through
    Encoder.encode_pictures_stream(want_pictures=False).  Stream, reconstruction file and rows are the same either way.
    source_format (hevcdl_amd.source_format(...)): the file holds frames of that size and input depth, not of the codec's format; width / height / bit_depth stay the
    CODED size (hevcdl_amd.padded_size) and the internal depth.  The frames go to the device as they are (Encoder.set_source_format), the SPS carries the window, the
    rows' squared errors are the window's and the reconstruction file holds window-sized frames at the format's output depth.  The format also carries the file's layout:
    a 4:0:0 / 4:2:2 / 4:4:4 file, Cr stored before Cb, an explicit window (its offsets go into the SPS; the squared errors then stay those of the whole picture).
    deblocking_metric / lf_offset_in_pps: the cfg keys DeblockingFilterMetric and LoopFilterOffsetInPPS.  Metric 1 (one deblocking offset per picture from the blockiness
    of its reconstruction, signalled in the slice header) keeps no state between pictures, so it shards like everything else; it needs lf_offset_in_pps False, as in the
    reference.  Metric 2 (a search over up to 49 filter trials a picture) searches round the choice of the picture before, so the pictures form one chain: it is refused
    with more than one rank.
    slices = (SliceMode, SliceArgument), lf_across_slices = LFCrossSliceBoundaryFlag: mode 1 cuts a picture into slices of whole CTU rows (SliceArgument a multiple of the
    width in CTUs; independent units of the decision launch, like tiles), mode 3 a picture of tiles into slices of SliceArgument tiles.  Every slice is a NAL unit of its own;
    what the library refuses (hevcdl.h, hevcdl_config.slice_mode) is raised with its reason.
    segments = (SliceSegmentMode, SliceSegmentArgument): dependent slice segments -- mode 1 makes every SliceSegmentArgument / width-in-CTUs rows of a wavefront picture a NAL
    unit of its own, mode 3 every SliceSegmentArgument tiles.  Nothing but the stream changes (hevcdl.h, hevcdl_config.slice_segment_mode).
    delta_qp_rd = N (the cfg key DeltaQpRD): every picture is decided at 2N+1 QPs round `qp` and coded with the cheapest (hevcdl.h, hevcdl_config.delta_qp_rd).  Pictures are
    independent, so it shards like everything else; the rows then carry a sixth column, the QP the picture was coded with, and the log lines print it.
    frame_qps: the QP of every picture of the sequence ([n_frames], POC order; hevcdl_amd.frame_qp_offsets / frame_qp_list make it from the cfg keys dQPFile, QPIncrementFrame
    and IntraQPOffset) -- every batch sets its slice (Encoder.set_frame_qps), pictures of one QP are decided in one launch; lambda_modifier: LambdaModifierI, else
    LambdaModifier0.  Rows and log lines carry the QP as with delta_qp_rd, which excludes both (hevcdl.h, "A QP per picture")."""
    if frame_qps is not None:
        frame_qps = [int(q) for q in frame_qps]
        if len(frame_qps) != n_frames:
            raise ValueError("frame_qps holds %d QPs for %d pictures" % (len(frame_qps), n_frames))
    own_qp = bool(delta_qp_rd) or frame_qps is not None      # the rows carry the QP every picture was coded with
    if deblocking_metric not in (0, 1, 2):
        raise ValueError("DeblockingFilterMetric %r is not a value of the key (0, 1 or 2)" % (deblocking_metric,))
    if deblocking_metric and lf_offset_in_pps:
        raise ValueError("If DeblockingFilterMetric is non-zero then both LoopFilterDisable and LoopFilterOffsetInPPS must be 0")
    dbk = dict(deblocking_metric=deblocking_metric, lf_offset_in_pps=lf_offset_in_pps)
    import torch
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if multi else (0, 1)
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    if deblocking_metric == 2 and world > 1:
        raise ValueError("DeblockingFilterMetric 2 on %d ranks: every picture's search window lies round the choice of the picture before it, so the pictures of a sequence are one "
                         "chain and cannot be dealt to ranks; run it on one rank" % world)
    mine = sharding.shard_frames(n_frames, world, rank)
    per_rank = sharding.max_shard(n_frames, world)
    rows = np.full((per_rank + 1, 6 if own_qp else 5), -1, np.int64)
    part_bits = (bitstream_path + ".part%d" % rank) if bitstream_path else None
    part_rec = (recon_path + ".part%d" % rank) if recon_path else None
    fb, fr = open(part_bits, "wb") if part_bits else None, open(part_rec, "wb") if part_rec else None
    if len(mine):
        enc = Encoder(width, height, qp, max_frames=min(batch, len(mine)), device=device, tiles=tiles, bit_depth=bit_depth, lf_across_tiles=lf_across_tiles, tools=tools, wavefront=wavefront, slices=slices, lf_across_slices=lf_across_slices, segments=segments, delta_qp_rd=delta_qp_rd, **dbk)      # tools: HEVCDL_TOOL_*; wavefront: WaveFrontSynchro mask (the cfg's tool switches)
        if lambda_modifier != 1.0:
            enc.set_lambda_modifier(lambda_modifier)
        sf = source_format
        sw, sh = (sf.source_width, sf.source_height) if sf is not None else (width, height)
        conf_win = (width - sw, height - sh)
        file_order = False
        if sf is not None:
            enc.set_source_format(sf)
            if sf.conf_win_left or sf.conf_win_right or sf.conf_win_top or sf.conf_win_bottom:      # an explicit window: no padding, all four offsets in the SPS
                conf_win = (sf.conf_win_left, sf.conf_win_right, sf.conf_win_top, sf.conf_win_bottom)
            # what the squared errors are taken over, at the internal depth: the coded picture minus the padding, in the coded plane order
            lf = make_source_format(sw, sh, sf.input_bit_depth, bit_depth, chroma_format=sf.chroma_format, colour_space=sf.colour_space)
            wf = make_source_format(sw, sh, bit_depth, bit_depth)
            file_order = bool(sf.colour_space and not sf.snr_internal_colour_space)      # the U and V columns in the file's order
        ysz = sw * sh
        scfg = None
        if device_entropy:
            enc.enable_device_entropy(True)
            scfg = stream_config(width, height, qp, level_idc, True, tiles, bit_depth, lf_across_tiles, tools, wavefront=wavefront, conf_win=conf_win)
        if device_report:
            enc.enable_picture_report(True, 1 if hash_sei else 0)
        stream_only = device_report and device_entropy and not recon_path      # no picture, record or SAO parameter is copied to the host
        for b0 in range(mine.start, mine.stop, batch):
            nb = min(batch, mine.stop - b0)
            yuv = read_frames(input_path, sw, sh, frame_skip + b0, nb, sf.input_bit_depth if sf is not None else bit_depth, sf.source_samples if sf is not None else None)
            t0 = time.time()
            labels = labels_fn(b0, nb) if labels_fn else None
            if frame_qps is not None:
                enc.set_frame_qps(frame_qps[b0:b0 + nb])
            if stream_only:
                recs = final = sao = None
                enc.encode_pictures_stream(yuv, labels, want_pictures=False, want_records=False)
            else:
                recs, final, sao, _ = enc.encode_pictures(yuv, labels)          # CNN -> decisions -> deblocking -> SAO, pictures stay in HBM
            et = (time.time() - t0) / nb
            slice_data, slice_sizes = enc.get_slice_data(0, nb) if device_entropy else (None, None)
            reports = enc.get_picture_report(0, nb) if device_report else None
            choices = enc.get_dbk_choice(0, nb)      # what every picture's slice header says about its deblocking filter
            pic_qp = [int(v) for v in enc.get_qp_rd(0, nb)[1]] if delta_qp_rd else [int(v) for v in enc.get_frame_qps(0, nb)]      # the QP every picture was coded with: its slice_qp_delta
            def one_picture(i):          # host work of a picture (arithmetic coder, hash, SSE): independent -> thread pool (ctypes drops the GIL)
                if device_entropy:
                    pcfg = scfg
                    if pic_qp[i] != qp:          # the access unit's own copy of the stream configuration
                        pcfg = type(scfg).from_buffer_copy(scfg)
                        pcfg.qp = pic_qp[i]
                    au = write_access_unit_from_slice_data(pcfg, b0 + i, slice_data[i], slice_sizes[i], choices[i], layout=enc.slice_layout, segments=enc.segment_layout)
                else:
                    au = write_access_unit(width, height, pic_qp[i], b0 + i, recs[i], level_idc=level_idc, sao=sao[i], tiles=tiles, bit_depth=bit_depth, lf_across_tiles=lf_across_tiles, tools=tools, wavefront=wavefront, conf_win=conf_win, choice=choices[i], slices=slices, lf_across_slices=lf_across_slices, segments=enc.segment_layout)
                if device_report:
                    return au, digest_sei(1, report_digest(reports[i])) if hash_sei else b"", [int(v) for v in reports[i]["sse"]]
                sei = picture_hash_sei(width, height, final[i], bit_depth) if hash_sei else b""
                if sf is not None:
                    d = (load_source_host(lf, sw, sh, bit_depth, yuv[i:i + 1])[0].astype(np.int64) - store_output_host(wf, width, height, bit_depth, final[i:i + 1])[0].astype(np.int64)) ** 2
                else:
                    d = (yuv[i].astype(np.int64) - final[i].astype(np.int64)) ** 2
                sse = [int(d[:ysz].sum()), int(d[ysz:ysz + ysz // 4].sum()), int(d[ysz + ysz // 4:].sum())]
                return au, sei, [sse[0], sse[2], sse[1]] if file_order else sse
            for i, (au, sei, sse) in enumerate(_pool().map(one_picture, range(nb))):
                poc = b0 + i
                if fb:
                    fb.write(au + sei)
                rows[poc - mine.start] = [poc, len(au) * 8] + sse + ([pic_qp[i]] if own_qp else [])
            if fr:
                (final if sf is None else store_output_host(sf, width, height, bit_depth, final)).tofile(fr)
            log("rank %d: pictures %d..%d encoded (%.2f s per picture)" % (rank, b0, b0 + nb - 1, et))
        enc.close()
    for f in (fb, fr):
        if f:
            f.close()
    if multi:
        t = torch.from_numpy(rows)
        allrows = sharding.gather_frame_summaries(t.to(torch.device("cuda", device)) if dist.get_backend() == "nccl" else t)     # the rank's own device, not torch's current one
        dist.barrier()
    else:
        allrows = rows[rows[:, 0] >= 0]
    if rank != 0:
        return None, None
    for path in (bitstream_path, recon_path):                      # parts in rank order = POC order (contiguous shards)
        if path:
            with open(path, "wb") as out:
                for r in range(world):
                    with open(path + ".part%d" % r, "rb") as part:
                        while True:
                            chunk = part.read(1 << 24)
                            if not chunk:
                                break
                            out.write(chunk)
                    os.remove(path + ".part%d" % r)
    summ = metrics.Summary(*((source_format.source_width, source_format.source_height) if source_format is not None else (width, height)), frame_rate, bit_depth)
    for row in allrows:
        poc, bits, sy, su, sv = (int(v) for v in row[:5])
        p = summ.add(bits, (sy, su, sv))
        log(metrics.frame_line(poc, int(row[5]) if own_qp else qp, bits, p))
    log("\n\nSUMMARY --------------------------------------------------------")
    log(summ.text())
    return summ, allrows


def encode_sequence_tile_sharded(input_path, width, height, qp, n_frames, tiles, bitstream_path=None, recon_path=None, frame_skip=0, batch=None, lf_across_tiles=True,
                                 bit_depth=8, level_idc=186, frame_rate=30.0, hash_sei=False, device=None, log=print, tools=0x7f, slices=None, segments=None, delta_qp_rd=0, frame_qps=None, lambda_modifier=1.0):
    """The within-picture partition: every rank decides its share of the TILES of every picture of a batch
    (`hevcdl_compress_tiles_dev`), one all-to-all moves the tile payloads to the picture's owner (`sharding.exchange_tiles_to_owners`:
    picture i of the batch -> rank i mod world), the owner runs the in-loop filters on the assembled picture and writes its access unit.
    Needs torch.distributed initialised; batch (default: world size) is a multiple of the world size.  Output == encode_sequence().  Slices and dependent slice segments
    are refused: the owner writes one slice NAL unit a picture."""
    if slices is not None and int(slices[0]) != 0:
        raise ValueError("the tile-sharded path does not code slices (SliceMode %d): use encode_sequence" % int(slices[0]))
    if segments is not None and int(segments[0]) != 0:
        raise ValueError("the tile-sharded path does not code slice segments (SliceSegmentMode %d): use encode_sequence" % int(segments[0]))
    if delta_qp_rd:      # a picture's QP is picked from the sums of ALL its tiles, which no rank has
        raise ValueError("the tile-sharded path does not search the slice QP (DeltaQpRD %d): use encode_sequence" % int(delta_qp_rd))
    if frame_qps is not None or lambda_modifier != 1.0:      # hevcdl_compress_tiles_dev refuses it: every rank would have to group the same pictures
        raise ValueError("the tile-sharded path does not code a QP per picture (frame_qps, lambda_modifier): use encode_sequence")
    import torch
    import torch.distributed as dist
    from . import REC_DTYPE, SAO_DTYPE
    rank, world = dist.get_rank(), dist.get_world_size()
    via_host = dist.get_backend() != "nccl"                         # gloo moves host tensors
    batch = batch or world
    if batch % world:
        raise ValueError("batch must be a multiple of the world size")
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    dev = torch.device("cuda", device)
    from . import tile_layout
    tl = tile_layout(tiles, width, height)                          # (columns, rows) or explicit CTU sizes
    n_tiles = tl[0] * tl[1]
    t_begin, t_count = sharding.shard_tiles(n_tiles, world, rank)
    enc = Encoder(width, height, qp, max_frames=batch, device=device, tiles=tiles, bit_depth=bit_depth, lf_across_tiles=lf_across_tiles, tools=tools)
    ctus, fsamp, ysz = enc.ctus, width * height * 3 // 2, width * height
    bps = 1 if bit_depth == 8 else 2
    part_bits = (bitstream_path + ".part%d" % rank) if bitstream_path else None
    part_rec = (recon_path + ".part%d" % rank) if recon_path else None
    fb, fr = open(part_bits, "wb") if part_bits else None, open(part_rec, "wb") if part_rec else None
    rows = []
    for b0 in range(0, n_frames, batch):
        nb = min(batch, n_frames - b0)
        yuv = read_frames(input_path, width, height, frame_skip + b0, nb, bit_depth)
        if nb < batch:                                              # last batch: repeat the last picture, the copies are dropped below
            yuv = np.concatenate([yuv, np.repeat(yuv[-1:], batch - nb, axis=0)])
        d_yuv = torch.from_numpy(yuv.view(np.uint8).reshape(batch, fsamp * bps)).to(dev)
        d_lab = torch.zeros((batch, ctus, 16), dtype=torch.uint8, device=dev)
        d_recs = torch.zeros((batch, ctus * REC_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        d_recon = torch.zeros_like(d_yuv)
        enc._check(enc.lib.hevcdl_predict_depth_dev(enc._h, d_yuv.data_ptr(), batch, d_lab.data_ptr(), None, None))
        enc.compress_tiles_dev(d_yuv.data_ptr(), batch, d_lab.data_ptr(), d_recs.data_ptr(), d_recon.data_ptr(), None, t_begin, t_count)
        torch.cuda.synchronize(dev)
        if via_host:
            owned, o_recon, o_recs = sharding.exchange_tiles_to_owners(d_recon.cpu(), d_recs.cpu(), width, height, tiles, bps=bps)
            o_recon, o_recs = o_recon.to(dev), o_recs.to(dev)
        else:
            owned, o_recon, o_recs = sharding.exchange_tiles_to_owners(d_recon, d_recs, width, height, tiles, bps=bps)
        no = len(owned)
        o_org = d_yuv[torch.tensor(owned, device=dev)].contiguous()
        o_dbk = torch.zeros_like(o_recon)
        o_fin = torch.zeros_like(o_recon)
        o_sao = torch.zeros((no, ctus * 3 * SAO_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        enc.deblock_frames_dev(o_recon.data_ptr(), no, o_recs.data_ptr(), o_dbk.data_ptr())
        enc.sao_frames_dev(o_org.data_ptr(), o_dbk.data_ptr(), no, o_sao.data_ptr(), o_fin.data_ptr())
        torch.cuda.synchronize(dev)
        recs = np.frombuffer(o_recs.cpu().numpy().tobytes(), REC_DTYPE).reshape(no, ctus)
        sao = np.frombuffer(o_sao.cpu().numpy().tobytes(), SAO_DTYPE).reshape(no, ctus, 3)
        final = np.frombuffer(o_fin.cpu().numpy().tobytes(), np.uint8 if bit_depth == 8 else "<u2").reshape(no, fsamp)
        for j, i in enumerate(owned):
            poc = b0 + i
            if i >= nb:
                continue
            au = write_access_unit(width, height, qp, poc, recs[j], level_idc=level_idc, sao=sao[j], tiles=tiles, bit_depth=bit_depth, lf_across_tiles=lf_across_tiles, tools=tools)
            blob = au + (picture_hash_sei(width, height, final[j], bit_depth) if hash_sei else b"")
            if fb:
                fb.write(blob)
            if fr:
                final[j].tofile(fr)
            d = (yuv[i].astype(np.int64) - final[j].astype(np.int64)) ** 2
            rows.append([poc, len(au) * 8, int(d[:ysz].sum()), int(d[ysz:ysz + ysz // 4].sum()), int(d[ysz + ysz // 4:].sum()), len(blob)])
        log("pictures %d..%d: tiles [%d, %d) of %d decided on rank %d" % (b0, b0 + nb - 1, t_begin, t_begin + t_count, n_tiles, rank))
    enc.close()
    for f in (fb, fr):
        if f:
            f.close()
    cap = (n_frames + world - 1) // world + batch
    t = torch.full((cap, 6), -1, dtype=torch.int64)
    if rows:
        t[:len(rows)] = torch.tensor(rows, dtype=torch.int64)
    allrows = sharding.gather_frame_summaries(t.to(dev) if not via_host else t)
    dist.barrier()
    if rank != 0:
        return None, None
    # merge the per-rank parts in POC order: every part holds its pictures in increasing POC
    owner_of = {int(r[0]): ((int(r[0]) % batch) % world) for r in allrows}
    size_of = {int(r[0]): int(r[5]) for r in allrows}
    for path, sizes in ((bitstream_path, size_of), (recon_path, None)):
        if not path:
            continue
        parts = [open(path + ".part%d" % r, "rb") for r in range(world)]
        with open(path, "wb") as out:
            for poc in range(n_frames):
                out.write(parts[owner_of[poc]].read(sizes[poc] if sizes else fsamp * bps))
        for r, fpart in enumerate(parts):
            fpart.close(); os.remove(path + ".part%d" % r)
    summ = metrics.Summary(width, height, frame_rate, bit_depth)
    for poc, bits, sy, su, sv, _ in allrows:
        p = summ.add(int(bits), (int(sy), int(su), int(sv)))
        log(metrics.frame_line(int(poc), qp, int(bits), p))
    log("\n\nSUMMARY --------------------------------------------------------")
    log(summ.text())
    return summ, allrows


def parse_sequence(bitstream_path, headers_only=False):
    """A stream file of this pipeline (or of the reference encoder in the same configuration) read back on the host, no GPU: -> a ParsedStream -- the stream's
    configuration and slice / segment layouts, per picture POC, QP, deblocking choice and the hash SEI's digests, and (unless headers_only) the CTU records and SAO
    parameters of every picture, as encode_sequence's writers took them.  HevcdlError says what a stream outside the parser's surface, or a damaged one, was refused for."""
    from . import parse_stream
    with open(bitstream_path, "rb") as f:
        return parse_stream(f.read(), headers_only=headers_only)


def decode_stream_by_stages(stream, device=0, batch=64):
    """TEST AND DIAGNOSTIC: decode_stream with the stages called one by one through host buffers and the digests computed on the host.  A stream of this pipeline (or of the reference encoder in the same configuration) decoded on the device, stage by stage: hevcdl_parse_stream on the host ->
    hevcdl_recon_kernel (the unfiltered reconstruction from the parsed records) -> deblocking with every picture's own QP and slice-header parameters -> SAO with the
    stream's parameters -> the decoded picture hash of every picture against its SEI.  -> (pictures [n, w * h * 3 / 2] in coded format -- the conformance window is NOT
    cut --, the ParsedStream, verdicts [n]: True / False where the stream carries a hash, None where it does not).  Pictures go through the device `batch` at a time."""
    from . import parse_stream, reconstruct_frames, picture_hash, DBK_CHOICE_DTYPE
    p = parse_stream(stream)
    cfg, n = p.cfg, len(p.pictures)
    tiles = (cfg.tile_columns, cfg.tile_rows)
    if not cfg.tile_uniform_spacing:
        cx, cy = (cfg.width + 63) // 64, (cfg.height + 63) // 64
        cw, rh = [cfg.tile_column_width[i] for i in range(cfg.tile_columns - 1)], [cfg.tile_row_height[i] for i in range(cfg.tile_rows - 1)]
        tiles = (cw + [cx - sum(cw)], rh + [cy - sum(rh)])
    slices = (p.slices.mode, p.slices.argument) if p.slices else None
    batch = max(1, min(batch, n))
    enc = Encoder(cfg.width, cfg.height, p.qps[0], max_frames=batch, device=device, tiles=tiles, bit_depth=cfg.bit_depth, lf_across_tiles=bool(cfg.lf_across_tiles),
                  lf_offsets=(cfg.lf_beta_offset_div2, cfg.lf_tc_offset_div2), slices=slices, lf_across_slices=bool(p.slices.lf_across_slices) if p.slices else True)
    out, verdicts = [], []
    try:
        for first in range(0, n, batch):
            pics = p.pictures[first:first + batch]
            recs, qps = p.records[first:first + len(pics)], p.qps[first:first + len(pics)]
            cur = reconstruct_frames(cfg, recs, slices=p.slices, qps=qps, device=device)
            enc.set_frame_qps(qps if any(q != p.qps[0] for q in qps) else None)
            # a picture whose filter is off (in the PPS or in its slice headers) is copied by the stage: the choice says so
            choices = np.zeros(len(pics), DBK_CHOICE_DTYPE)
            for i, pic in enumerate(pics):
                choices[i] = (pic.dbk.override_enabled, pic.dbk.override_flag, pic.dbk.disabled, pic.dbk.beta_offset_div2, pic.dbk.tc_offset_div2)
            cur = enc.deblock_frames_choice(cur, recs, choices)
            if any(pic.sao for pic in pics):
                cur = enc.sao_apply_frames(cur, p.sao[first:first + len(pics)])      # (a picture without SAO holds mode 0 everywhere: copied)
            out.append(cur)
            for i, pic in enumerate(pics):
                method, digest = p.digest(first + i)
                verdicts.append(None if not method else bytes(picture_hash(cfg.width, cfg.height, cur[i], cfg.bit_depth, method)) == digest)
    finally:
        enc.close()
    return np.concatenate(out), p, verdicts


def decode_stream(stream, device=0, batch=64, device_parse=False, cu_qp=False, scaling_lists=False):
    """A stream of this pipeline (or of the reference encoder in the same configuration) decoded by hevcdl_decode_stream: parsed on the host -- with device_parse only its
    headers, the slice data by hevcdl_slice_decode_kernel into the records in HBM (hevcdl_enable_device_parse) --; reconstruction from the
    records, deblocking, SAO with the stream's parameters and the digests of the decoded picture hash on the device, `batch` pictures at a time in HBM.
    -> (pictures [n, w * h * 3 / 2] in coded format -- the conformance window is NOT cut --, the ParsedStream of the headers, verdicts [n]: True / False where the stream
    carries a hash, None where it does not).  cu_qp: accept streams with cu_qp_delta_enabled_flag or PPS chroma QP offsets (hevcdl_enable_cu_qp); off, they are refused.
    scaling_lists: accept streams whose SPS enables scaling lists (hevcdl_enable_scaling_lists); off, they are refused."""
    from . import decode_stream as decode, parse_stream
    pictures, _, _, verdicts = decode(stream, device=device, batch=batch, device_parse=device_parse, cu_qp=cu_qp, scaling_lists=scaling_lists)
    return pictures, parse_stream(stream, headers_only=True, cu_qp=cu_qp, scaling_lists=scaling_lists), verdicts


def decode_sequence(bitstream_path, recon_path=None, device=0, batch=64, log=None, device_parse=False, cu_qp=False, scaling_lists=False):
    """decode_stream over a stream file; with recon_path the output pictures are written as the reference decoder writes them: the conformance window, at the coded bit
    depth.  One line per picture (POC, QP, hash verdict) goes to `log` (a callable, e.g. print).  -> (pictures, ParsedStream, verdicts); a hash mismatch raises
    ValueError behind the file."""
    with open(bitstream_path, "rb") as f:
        pictures, p, verdicts = decode_stream(f.read(), device=device, batch=batch, device_parse=device_parse, cu_qp=cu_qp, scaling_lists=scaling_lists)
    cfg = p.cfg
    w, h = cfg.width, cfg.height
    if recon_path is not None:
        l, r, t, b = cfg.conf_win_left, cfg.conf_win_right, cfg.conf_win_top, cfg.conf_win_bottom
        with open(recon_path, "wb") as f:
            for pic in pictures:
                y, u, v = pic[:w * h].reshape(h, w), pic[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), pic[w * h * 5 // 4:].reshape(h // 2, w // 2)
                for plane, s in ((y, 1), (u, 2), (v, 2)):
                    f.write(np.ascontiguousarray(plane[t // s:(h - b) // s, l // s:(w - r) // s]).tobytes())
    for i, pic in enumerate(p.pictures):
        if log:
            log("POC %4d  QP %2d  [%s]" % (pic.poc if pic.nal_type == 21 else 0, pic.qp, {None: "no hash", True: "hash OK", False: "hash MISMATCH"}[verdicts[i]]))
    if any(v is False for v in verdicts):
        raise ValueError("decoded picture hash mismatch in picture(s) %s" % [i for i, v in enumerate(verdicts) if v is False])
    return pictures, p, verdicts
