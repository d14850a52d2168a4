"""oracle/cnn_torch.py -- TEST INFRASTRUCTURE (checker), not product code.

Plain PyTorch restatement, fp32 or fp64, of oracle/cnn_oracle.py (which restates /root/reference/use_model.py:16-58, 80-119) for sizes the numpy oracle cannot finish in a
bench run (0.3 s per CTU): the same graph -- conv / BatchNorm in TRAINING mode (per-sample statistics, biased variance, eps 1e-5) or with the running statistics / ReLU /
max-pool blocks, cat, three linear layers -- in torch.nn.functional, in the dtype of the weights throughout (fp32 unless asked otherwise), on whatever device the tensors live.
The fp32 form is pinned against cnn_oracle.forward by tests/test_oracle_golden.py (CPU, a handful of CTUs); bench.py's `cnn_label_check` leg runs it on the GPU as the fp32
reference the split-f16 MFMA kernel's labels are counted against.  The fp64 form, with per-layer taps and both BatchNorm modes, is the yardstick of tests/test_cnn_numerics*.py:
pinned to the reference model's own logits there, and the fp32 graph stays within 2e-5 of it, so what a kernel differs beyond that is the kernel's own.
Only tests/ and bench.py's checker legs may import this module.
"""
import numpy as np

import cnn_oracle


def _block(F, x, w, name, pad, pool, bn_eval=False):
    """conv / BatchNorm / ReLU / max-pool in x's dtype.  The statistics and 1 / sqrt are formed in f64 and rounded to the graph's dtype once (as oracle/cnn_oracle.py
    does); in an f64 graph that is no rounding at all."""
    y = F.conv2d(x, w[name + ".0.weight"], w[name + ".0.bias"], padding=pad)
    if bn_eval:      # model.eval(): the checkpoint's running statistics (cnn_oracle._bn_eval)
        mean = w[name + ".1.running_mean"].view(1, -1, 1, 1)
        inv = (1.0 / (w[name + ".1.running_var"].double() + 1e-5).sqrt()).to(y.dtype).view(1, -1, 1, 1)
    else:
        mean = y.double().mean(dim=(2, 3), keepdim=True)
        var = ((y.double() - mean) ** 2).mean(dim=(2, 3), keepdim=True)
        inv = (1.0 / (var + 1e-5).sqrt()).to(y.dtype)
        mean = mean.to(y.dtype)
    y = (y - mean) * inv * w[name + ".1.weight"].view(1, -1, 1, 1) + w[name + ".1.bias"].view(1, -1, 1, 1)
    return F.max_pool2d(F.relu(y), pool)


def forward(torch, w, x32, x64, bn_eval=False, taps=False):
    """cnn_oracle.forward on torch tensors: x32 [N,3,32,32], x64 [N,3,64,64] in [0,1], in the dtype of the weights (f32 | f64) -> logits [N,16].
    taps: -> (logits, {"cat": pooled conv1 ++ conv64 [N,32,16,16], "conv2": [N,64,8,8], "conv3": [N,128,4,4], "fc1": [N,256], "fc2": [N,64]})."""
    F = torch.nn.functional
    a = _block(F, x32, w, "conv1", 2, 2, bn_eval)
    b = _block(F, x64, w, "conv64", 2, 4, bn_eval)
    cat = torch.cat([a, b], dim=1)
    c2 = _block(F, cat, w, "conv2", 1, 2, bn_eval)
    c3 = _block(F, c2, w, "conv3", 1, 2, bn_eval)
    f1 = F.relu(F.linear(c3.reshape(c3.shape[0], -1), w["fc1.0.weight"], w["fc1.0.bias"]))
    f2 = F.relu(F.linear(f1, w["fc2.0.weight"], w["fc2.0.bias"]))
    out = F.linear(f2, w["fc3.weight"], w["fc3.bias"])
    return (out, {"cat": cat, "conv2": c2, "conv3": c3, "fc1": f1, "fc2": f2}) if taps else out


def ctu_logits(torch, w, ctu_rgb, batch=2048, bn_eval=False, taps=False):
    """ctu_rgb [N,64,64,3] uint8 (numpy or tensor) -> logits [N,4,16] on w's device and in w's dtype (quadrant order of use_model.py:89-100).  The input is u8 / 255 formed
    in f32, as ToTensor forms it, and only then widened.  taps: -> (logits, {name: [N,4,...]}), the taps of `forward` per quadrant."""
    dev, dtype = w["fc3.weight"].device, w["fc3.weight"].dtype
    x_all = torch.as_tensor(ctu_rgb)
    outs, tapped = [], {}
    with torch.no_grad():
        for i in range(0, x_all.shape[0], batch):
            x = (x_all[i:i + batch].to(dev).float() / 255.0).permute(0, 3, 1, 2).contiguous().to(dtype)
            qs, ts = [], []
            for q in range(4):
                ox, oy = (q % 2) * 32, (q // 2) * 32
                r = forward(torch, w, x[:, :, oy:oy + 32, ox:ox + 32].contiguous(), x, bn_eval, taps)
                qs.append(r[0] if taps else r)
                if taps:
                    ts.append(r[1])
            outs.append(torch.stack(qs, dim=1))
            if taps:
                for k in ts[0]:
                    tapped.setdefault(k, []).append(torch.stack([t[k] for t in ts], dim=1))
    logits = torch.cat(outs)
    return (logits, {k: torch.cat(v) for k, v in tapped.items()}) if taps else logits


def logits_np(torch, w_np, ctu_rgb, dtype="f64", bn_eval=False):
    """numpy in, numpy out, on the CPU: the logits [N,4,16] of the graph in `dtype` ("f32" | "f64") for a dict of numpy weights."""
    w = weights_to(torch, w_np, "cpu", {"f32": torch.float32, "f64": torch.float64}[dtype])
    return ctu_logits(torch, w, ctu_rgb, bn_eval=bn_eval).numpy()


def weights_to(torch, w_np, dev, dtype=None):
    """dtype: torch.float32 (default) or torch.float64 -- the dtype of the weights is the dtype of the whole graph."""
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=dtype or torch.float32, device=dev) for k, v in w_np.items()}


def label_check(torch, w_np, yuv_frames, width, height, dev, gpu_labels, gap=1e-2):
    """Labels of the fp32 graph for whole frames (numpy [F, w*h*3/2] uint8) against `gpu_labels` [F, ctus, 16]:
    -> {ctus, in_gap_band, labels_differing_from_fp32_oracle, ...}.  A CTU is `in the gap band` when, in any of its 16 argmax decisions, the two largest logits of the
    fp32 graph are closer than `gap` (there a rounding difference of the kernel's split-f16 operands may legitimately pick the other class)."""
    w = weights_to(torch, w_np, dev)
    ctus = band = differ = differ_outside = cells = 0
    for f in range(yuv_frames.shape[0]):
        rgb = cnn_oracle.yuv_to_rgb_ctus(yuv_frames[f], width, height)
        lg = ctu_logits(torch, w, rgb).cpu().numpy()
        lab = cnn_oracle.clamp_labels(cnn_oracle.labels_from_logits(lg)[None], width, height)[0]
        top2 = np.sort(lg.reshape(lg.shape[0], 4, 4, 4), axis=3)
        near = ((top2[..., 3] - top2[..., 2]) < gap).reshape(lg.shape[0], -1).any(axis=1)
        d = (lab != gpu_labels[f]).any(axis=1)
        ctus += lab.shape[0]; band += int(near.sum()); differ += int(d.sum()); differ_outside += int((d & ~near).sum()); cells += int((lab != gpu_labels[f]).sum())
    return {"ctus": ctus, "in_gap_band": band, "labels_differing_from_fp32_oracle": differ, "differing_outside_the_band": differ_outside, "differing_cells": cells,
            "gap": gap, "frames": int(yuv_frames.shape[0]),
            "reference": "oracle/cnn_torch.py: the graph of oracle/cnn_oracle.py (use_model.py:16-58, BatchNorm in training mode) in fp32 torch.nn.functional on the same GPU"}


def reference_pair(torch, w_np, ctu_rgb, bn_eval=False):
    """-> (f64 logits [N,4,16], E_ref = max |f32 graph - f64 graph| over these CTUs), on the CPU: the yardstick and its own resolution (tests/test_cnn_numerics_gpu.py)."""
    l64 = logits_np(torch, w_np, ctu_rgb, "f64", bn_eval)
    return l64, float(np.abs(logits_np(torch, w_np, ctu_rgb, "f32", bn_eval) - l64).max())


def decided(logits, band):
    """logits [N,4,16] -> bool [N]: every one of the CTU's 16 argmax decisions has its two largest logits further apart than `band`."""
    srt = np.sort(np.asarray(logits).reshape(-1, 4, 4, 4), axis=-1)
    return ((srt[..., -1] - srt[..., -2]) > band).all(axis=(1, 2))
