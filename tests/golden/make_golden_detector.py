#!/usr/bin/env python
"""Generate tests/golden/detector.npz and tests/golden/detector_small.cfg by IMPORTING the reference's person detector
(object_detector/YOLOv3; build container only).

Run from the repo root:  ``python tests/golden/make_golden_detector.py``

The reference is imported with the empty ``cv2`` stub of make_golden.py (detector_utils.py imports it; nothing recorded
here calls it).  ``detector_yolov3.py`` parses ``sys.argv`` and loads a weights file while it is imported.  Two patches, both
made before that import: ``sys.argv`` is cut down to the program name, so its argparse sees its own defaults, and
``models.Darknet.load_darknet_weights`` is replaced by a function that does nothing, so the module-level ``Darknet`` of
yolov3.cfg keeps its fresh weights (it is never run).  For the rescale cases the module's ``model`` and
``preprocess_img_for_yolo`` are then replaced by functions that return the crafted predictions, and its own
``inference_yolov3_from_img`` runs the NMS and lines 79-98 on them unmodified.

``detector_small.cfg`` is this project's: 16 blocks at 64 x 64 with every supported block kind (see SMALL_CFG).  Recorded:

- the reference's parse of the small cfg and of its own yolov3.cfg, and the ``state_dict`` key -> shape manifests of its
  ``Darknet`` over both (JSON strings);
- ``Darknet(detector_small.cfg)`` in eval mode on a seeded 2-image batch with the seeded weights of
  tests/detector_ref.py:build_weights (the tests rebuild input and weights from the seeds);
- ``non_max_suppression`` on crafted predictions (the inputs are stored): two 64-row images with overlapping clusters, one of
  them with the same place in two classes; an image without a candidate, one with a single candidate and a one-row image;
  one image of 700 rows.  The margins that make the discrete decisions well defined are ASSERTED here: every conf at least
  0.01 from conf_thres, every tested IoU at least 0.02 from nms_thres, scores pairwise distinct by at least 1e-4;
- ``inference_yolov3_from_img`` (NMS + rescale) for wide, tall and square frames with odd and even ``dim_diff``;
- what ``np.pad`` stores for the pad value 127.5 in a uint8 image (asserted to be 127).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, ROOT, import_reference, save     # noqa: E402
from tests import detector_ref as R                           # noqa: E402

CONF_THRES, NMS_THRES, IMG = 0.4, 0.4, 416
SMALL_IMG, SMALL_SEED, SMALL_INPUT_SEED = 64, 20, 21
RESCALE_FRAMES = ((100, 180), (101, 180), (181, 96), (180, 96), (256, 256))

_BN = "batch_normalize=1\n"
_ANCHORS = "anchors = 4,5,  8,10,  12,9,  16,20,  24,18,  30,40\nclasses=3\nnum=6\n"


def _conv(filters, size, stride, bn=_BN, act="leaky"):
    return f"[convolutional]\n{bn}filters={filters}\nsize={size}\nstride={stride}\npad=1\nactivation={act}\n\n"


SMALL_CFG = (
    "# 16 blocks at 64 x 64 with every block kind of the person detector: 3x3 stride 1 and 2, 1x1, a shortcut, a one-layer and\n"
    "# a two-layer route, an upsample, a conv with a bias instead of BatchNorm, two yolo heads (grids 16 and 32, 3 classes)\n"
    "[net]\nbatch=1\nwidth=64\nheight=64\nchannels=3\n\n"
    + _conv(8, 3, 1) + _conv(16, 3, 2) + _conv(8, 1, 1) + _conv(16, 3, 1)
    + "[shortcut]\nfrom=-3\nactivation=linear\n\n"
    + _conv(32, 3, 2) + _conv(16, 1, 1, bn="batch_normalize=0\n") + _conv(24, 1, 1, bn="", act="linear")
    + "[yolo]\nmask = 3,4,5\n" + _ANCHORS + "\n"
    + "[route]\nlayers = -3\n\n" + _conv(8, 1, 1) + "[upsample]\nstride=2\n\n[route]\nlayers = -1, 4\n\n"
    + _conv(16, 3, 1) + _conv(24, 1, 1, bn="", act="linear")
    + "[yolo]\nmask = 0,1,2\n" + _ANCHORS)


def small_input():
    return torch.from_numpy(np.random.RandomState(SMALL_INPUT_SEED).uniform(0, 1, (2, 3, SMALL_IMG, SMALL_IMG)).astype(np.float32))


def crafted(rs, n_rows, n_clusters, classes=3, per_cluster=(2, 8), twin=False, offsets=True):
    """(n_rows, 5 + classes) float32 rows: clusters of jittered boxes around centers on a 100-pixel lattice (one class per
    cluster; ``twin`` puts two clusters of different classes on one center), some clusters with a partner shifted by 30 % or
    55 % of the width, the rest of the rows below the threshold.  The candidate scores are a permutation of an even ladder."""
    rows = []
    slots = [(60 + 100 * i, 60 + 100 * j) for i in range(4) for j in range(4)]
    rs.shuffle(slots)
    for c in range(n_clusters):
        cx, cy = slots[0 if twin and c < 2 else c % len(slots)]
        cls = c if twin and c < 2 else (c + c // len(slots)) % classes     # clusters that share a center differ in class
        w, h = rs.uniform(40, 70, 2)
        shift = 0.0
        for k in range(rs.randint(per_cluster[0], per_cluster[1] + 1)):
            if offsets and k and k % 3 == 0:
                shift = (0.30, 0.55)[(k // 3) % 2] * w
            j = rs.uniform(-2.0, 2.0, 4)
            rows.append((cx + shift + j[0], cy + j[1], w + j[2], h + j[3], cls))
    rows = rows[:n_rows]
    n_cand = len(rows)
    ladder = np.linspace(0.42, 0.93, n_cand)[rs.permutation(n_cand)]
    out = np.zeros((n_rows, 5 + classes), np.float32)
    for r, ((cx, cy, w, h, cls), s) in enumerate(zip(rows, ladder)):
        top = rs.uniform(0.94, 0.99)
        out[r, :4] = (cx, cy, w, h)
        out[r, 4] = s / top
        out[r, 5:] = rs.uniform(0.01, 0.5, classes)
        out[r, 5 + cls] = top
    for r in range(n_cand, n_rows):                                 # below the threshold
        out[r, :4] = (rs.uniform(30, 380), rs.uniform(30, 380), rs.uniform(20, 80), rs.uniform(20, 80))
        out[r, 4] = rs.uniform(0.02, 0.38)
        out[r, 5:] = rs.uniform(0.01, 0.99, classes)
    return out[rs.permutation(n_rows)]


def pack(dets, width):
    """List of (K, 6) tensors / None -> (B, width, 6) float32 padded with zeros, (B,) counts."""
    out = np.zeros((len(dets), width, 6), np.float32)
    cnt = np.zeros(len(dets), np.int32)
    for i, d in enumerate(dets):
        if d is not None:
            cnt[i] = d.shape[0]
            out[i, :cnt[i]] = d.detach().numpy()
    return out, cnt


def main():
    import_reference()
    import object_detector.YOLOv3.models as M
    from object_detector.YOLOv3.parse_config import parse_model_config
    from object_detector.YOLOv3.detector_utils import non_max_suppression

    out = {}
    assert np.all(np.pad(np.zeros((2, 2, 3), np.uint8), ((1, 1), (0, 0), (0, 0)), "constant", constant_values=127.5)[0] == 127)
    out["pad_level"] = np.array([127], np.uint8)

    cfg_path = os.path.join(HERE, "detector_small.cfg")
    with open(cfg_path, "w") as f:
        f.write(SMALL_CFG)
    ref_cfg = os.path.join(REF, "object_detector", "YOLOv3", "config", "yolov3.cfg")
    out["small_parse"] = np.array(json.dumps(parse_model_config(cfg_path)))
    out["yolov3_parse"] = np.array(json.dumps(parse_model_config(ref_cfg)))

    # ---- the small net: manifest + forward -------------------------------------------------------------------------------
    net = M.Darknet(cfg_path, img_size=SMALL_IMG).eval()
    out["small_manifest"] = np.array(json.dumps({k: list(v.shape) for k, v in net.state_dict().items()}))
    blocks = parse_model_config(cfg_path)[1:]
    net.load_state_dict(R.build_weights(blocks, SMALL_SEED))
    with torch.no_grad():
        out["small_pred"] = net(small_input())
    big = M.Darknet(ref_cfg, img_size=IMG)
    out["yolov3_manifest"] = np.array(json.dumps({k: list(v.shape) for k, v in big.state_dict().items()}))
    del big

    # ---- NMS on crafted predictions ------------------------------------------------------------------------------------------
    rs = np.random.RandomState(5)
    pair = np.stack([crafted(rs, 64, 9), crafted(rs, 64, 8, twin=True)])
    none = crafted(rs, 16, 0)
    one = crafted(rs, 16, 1, per_cluster=(1, 1))
    other = crafted(rs, 16, 3, per_cluster=(1, 3))
    cases = {"pair": pair, "edge": np.stack([none, one, other]), "single": crafted(rs, 1, 1, per_cluster=(1, 1))[None],
             "large": crafted(rs, 700, 40, per_cluster=(8, 32))[None]}
    margins = {}
    for name, pred in cases.items():
        t = torch.from_numpy(pred)
        dets = non_max_suppression(t.clone(), CONF_THRES, NMS_THRES)
        mine = R.nms(t, CONF_THRES, NMS_THRES, margins)
        for a, b in zip(dets, mine):                                # the restatement takes the reference's decisions
            assert (a is None) == (b is None) and (a is None or (a.shape == b.shape and torch.equal(a[:, 4:], b[:, 4:])))
        out[f"nms_{name}_pred"] = pred
        out[f"nms_{name}_dets"], out[f"nms_{name}_counts"] = pack(dets, max(1, max(0 if d is None else len(d) for d in dets)))
        print(name, "counts", out[f"nms_{name}_counts"])
    print("margins", margins)
    assert margins["conf"] >= 0.01 and margins["iou"] >= 0.02 and margins["score"] >= 1e-4, margins
    assert out["nms_edge_counts"][0] == 0 and out["nms_edge_counts"][1] == 1 and out["nms_single_counts"][0] == 1
    twin = out["nms_pair_dets"][1][:out["nms_pair_counts"][1]]
    ctr = lambda d: np.array([d[0] + d[2], d[1] + d[3]]) / 2
    assert any(np.abs(ctr(a) - ctr(b)).max() < 25 and a[5] != b[5] for a in twin for b in twin), "the twin clusters are both kept"
    out["nms_thresholds"] = np.array([CONF_THRES, NMS_THRES])

    # ---- the rescale: the reference's own inference function over the crafted predictions -------------------------------------
    sys.argv = sys.argv[:1]
    M.Darknet.load_darknet_weights = lambda self, path: None
    import object_detector.YOLOv3.detector_yolov3 as D
    assert D.opt.img_size == IMG and D.opt.conf_thres == CONF_THRES and D.opt.nms_thres == NMS_THRES
    D.preprocess_img_for_yolo = lambda img: torch.zeros(1)
    D.model = lambda x: torch.from_numpy(pair[:1]).clone()
    out["rescale_frames"] = np.array(RESCALE_FRAMES)
    for i, (h, w) in enumerate(RESCALE_FRAMES):
        cands = D.inference_yolov3_from_img(np.zeros((h, w, 3), np.uint8))
        assert len(cands) > 0
        out[f"rescale_{i}"] = np.array(cands, dtype=np.float64)
    save("detector", **out)


if __name__ == "__main__":
    main()
