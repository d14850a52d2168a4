"""Largest difference of the on-device CNN's logits from the reference model's (tests/golden/cnn_f1.npz, cnn_f3.npz), and per group of the adversarial corpus
(oracle/cnn_cases.py) from the f64 graph (oracle/cnn_torch.py) next to the f32 graph's own: python tools/cnn_err.py [table file, e.g. profiles/cnn_numerics.txt]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch
import hevcdl_amd, cnn_oracle, cnn_cases, cnn_torch
G = os.path.join(ROOT, "tests", "golden")
e = hevcdl_amd.Encoder(128, 128, 32, max_frames=1)
f = np.load(os.path.join(G, "cnn_f1.npz"))
lab, lg = e.predict_depth_rgb(f["ctu_rgb"])
print("cnn_f1: max |logit - reference model| %.3e   labels differing %d of %d CTUs" % (np.abs(lg - f["logits"]).max(), int((lab != f["labels"]).any(axis=1).sum()), len(lab)))
g = np.load(os.path.join(G, "cnn_f3.npz"))
for n in range(int(g["n_pictures"])):
    lab, lg = e.predict_depth_rgb(cnn_oracle.rgb_picture_to_ctus(g["rgb%d" % n]))
    print("cnn_f3 picture %d: max |logit - reference loop| %.3e   label files differing %d of %d" % (n, np.abs(lg - g["logits%d" % n]).max(), int((lab != g["labels%d" % n]).any(axis=1).sum()), len(lab)))
e.close()
# against the f64 graph: E_ref = max |f32 graph - f64 graph| over the corpus and cnn_f1 (the tests' bound is 16 * E_ref, tests/test_cnn_numerics_gpu.py); a record, never the source of a bound
w = cnn_oracle.load_weights(hevcdl_amd.WEIGHTS_PATH)
ctus, spans = cnn_cases.stacked()
spans = dict(spans, cnn_f1=slice(len(ctus), len(ctus) + len(f["ctu_rgb"])))
ctus = np.concatenate([ctus, f["ctu_rgb"]])
lines = ["%-10s %-8s %5s %11s %11s %13s %6s" % ("BatchNorm", "group", "CTUs", "E_ref", "E_ref group", "kernel error", "ratio")]
for bn_mode in (0, 1):
    l64 = cnn_torch.logits_np(torch, w, ctus, "f64", bool(bn_mode))
    d32 = np.abs(cnn_torch.logits_np(torch, w, ctus, "f32", bool(bn_mode)) - l64)
    e = hevcdl_amd.Encoder(128, 128, 32, max_frames=1, bn_mode=bn_mode)
    err = np.abs(e.predict_depth_rgb(ctus)[1] - l64)
    e.close()
    for name, sl in spans.items():
        lines.append("%-10s %-8s %5d %11.3e %11.3e %13.3e %6.2f" % (("train", "eval")[bn_mode], name, sl.stop - sl.start, d32.max(), d32[sl].max(), err[sl].max(), err[sl].max() / d32.max()))
print("\n".join(lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
