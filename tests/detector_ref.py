"""Plain torch-CPU / numpy restatement of the reference's person detector (object_detector/YOLOv3), for the detector
tests.  It does not import the reference and needs no GPU: the eval forward of ``Darknet`` (models.py:245-276), the yolo
decode (models.py:123-165), the merging NMS (detector_utils.py:253-291), the rescale to frame pixels
(detector_yolov3.py:79-98) and a float64 letterbox (exact area mean, round half to even).  ``dtype=torch.float64`` runs
the same statements in double: the yardstick the float32 results are measured against."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def conv_blocks(blocks):
    """(index, in channels, block) of every convolutional block of a block list without ``[net]`` (3 input channels)."""
    chans, out = [], []
    for i, d in enumerate(blocks):
        t = d["type"]
        if t == "convolutional":
            out.append((i, chans[-1] if chans else 3, d))
            chans.append(int(d["filters"]))
        elif t == "route":
            chans.append(sum(chans[i + int(v) if int(v) < 0 else int(v)] for v in d["layers"].split(",")))
        elif t == "shortcut":
            chans.append(chans[int(d["from"]) + i if int(d["from"]) < 0 else int(d["from"])])
        else:
            chans.append(chans[-1])
    return out


def build_weights(blocks, seed):
    """Seeded ``state_dict`` (the reference ``Darknet``'s keys) of a block list: He-scaled conv weights (gain 1.4 before a
    LeakyReLU, 0.5 for the conv a shortcut adds to its input and 0.1 for a linear head conv, so that 23 residual blocks and
    the ``exp`` of the decode stay in range), BatchNorm weight in [0.6, 1.4], bias and running mean in [-0.3, 0.3], running
    variance in [0.5, 1.5] - away from the 0 / 1 of a fresh layer."""
    rs = np.random.RandomState(seed)
    sd = {}
    for i, cin, d in conv_blocks(blocks):
        k, cout = int(d["size"]), int(d["filters"])
        gain = 0.1 if d["activation"] != "leaky" else 0.5 if blocks[i + 1]["type"] == "shortcut" else 1.4
        w = rs.standard_normal((cout, cin, k, k)) * (gain / np.sqrt(cin * k * k))
        sd[f"module_list.{i}.conv_{i}.weight"] = torch.from_numpy(w.astype(np.float32))
        if int(d["batch_normalize"]):
            p = f"module_list.{i}.batch_norm_{i}."
            sd[p + "weight"] = torch.from_numpy(rs.uniform(0.6, 1.4, cout).astype(np.float32))
            sd[p + "bias"] = torch.from_numpy(rs.uniform(-0.3, 0.3, cout).astype(np.float32))
            sd[p + "running_mean"] = torch.from_numpy(rs.uniform(-0.3, 0.3, cout).astype(np.float32))
            sd[p + "running_var"] = torch.from_numpy(rs.uniform(0.5, 1.5, cout).astype(np.float32))
            sd[p + "num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
        else:
            sd[f"module_list.{i}.conv_{i}.bias"] = torch.from_numpy(rs.uniform(-0.3, 0.3, cout).astype(np.float32))
    return sd


def yolo_anchors(d):
    flat = [int(v) for v in d["anchors"].split(",")]
    return [(flat[2 * int(m)], flat[2 * int(m) + 1]) for m in d["mask"].split(",")]


def decode(head, anchors, num_classes, img_size):
    """models.py:123-165 in eval mode, in ``head``'s dtype."""
    nb, ng, na = head.shape[0], head.shape[2], len(anchors)
    stride = img_size / ng
    p = head.view(nb, na, 5 + num_classes, ng, ng).permute(0, 1, 3, 4, 2).contiguous()
    gx = torch.arange(ng).repeat(ng, 1).view(1, 1, ng, ng).to(head.dtype)
    gy = torch.arange(ng).repeat(ng, 1).t().view(1, 1, ng, ng).to(head.dtype)
    sa = torch.tensor([(aw / stride, ah / stride) for aw, ah in anchors], dtype=head.dtype)
    boxes = torch.empty(p[..., :4].shape, dtype=head.dtype)
    boxes[..., 0] = torch.sigmoid(p[..., 0]) + gx
    boxes[..., 1] = torch.sigmoid(p[..., 1]) + gy
    boxes[..., 2] = torch.exp(p[..., 2]) * sa[:, 0:1].view(1, na, 1, 1)
    boxes[..., 3] = torch.exp(p[..., 3]) * sa[:, 1:2].view(1, na, 1, 1)
    return torch.cat((boxes.view(nb, -1, 4) * stride, torch.sigmoid(p[..., 4]).view(nb, -1, 1),
                      torch.sigmoid(p[..., 5:]).view(nb, -1, num_classes)), -1)


def forward(blocks, sd, x, img_size, dtype=torch.float32):
    """``(prediction (B, N, 5 + C), [head maps])`` of the eval forward, every tensor in ``dtype``."""
    x = x.to(dtype)
    outs, preds, heads = [], [], []
    with torch.no_grad():
        for i, d in enumerate(blocks):
            t = d["type"]
            if t == "convolutional":
                k = int(d["size"])
                pad = (k - 1) // 2 if int(d["pad"]) else 0
                bias = sd.get(f"module_list.{i}.conv_{i}.bias")
                x = F.conv2d(x, sd[f"module_list.{i}.conv_{i}.weight"].to(dtype), None if bias is None else bias.to(dtype),
                             int(d["stride"]), pad)
                if int(d["batch_normalize"]):
                    p = f"module_list.{i}.batch_norm_{i}."
                    x = F.batch_norm(x, sd[p + "running_mean"].to(dtype), sd[p + "running_var"].to(dtype),
                                     sd[p + "weight"].to(dtype), sd[p + "bias"].to(dtype), False, 0.1, 1e-5)
                if d["activation"] == "leaky":
                    x = F.leaky_relu(x, 0.1)
            elif t == "upsample":
                x = F.interpolate(x, scale_factor=int(d["stride"]), mode="nearest")
            elif t == "route":
                x = torch.cat([outs[int(v)] if int(v) >= 0 else outs[i + int(v)] for v in d["layers"].split(",")], 1)
            elif t == "shortcut":
                x = outs[-1] + outs[int(d["from"]) if int(d["from"]) >= 0 else i + int(d["from"])]
            elif t == "yolo":
                heads.append(x)
                x = decode(x, yolo_anchors(d), int(d["classes"]), img_size)
                preds.append(x)
            else:
                raise NotImplementedError(t)
            outs.append(x)
    return torch.cat(preds, 1), heads


def bbox_iou(b1, b2):
    """detector_utils.py:190-220 on corner boxes: the + 1 pixel convention."""
    ix1, iy1 = torch.max(b1[:, 0], b2[:, 0]), torch.max(b1[:, 1], b2[:, 1])
    ix2, iy2 = torch.min(b1[:, 2], b2[:, 2]), torch.min(b1[:, 3], b2[:, 3])
    inter = torch.clamp(ix2 - ix1 + 1, min=0) * torch.clamp(iy2 - iy1 + 1, min=0)
    a1 = (b1[:, 2] - b1[:, 0] + 1) * (b1[:, 3] - b1[:, 1] + 1)
    a2 = (b2[:, 2] - b2[:, 0] + 1) * (b2[:, 3] - b2[:, 1] + 1)
    return inter / (a1 + a2 - inter + 1e-16)


def nms(prediction, conf_thres, nms_thres, margins=None):
    """detector_utils.py:253-291 for (B, N, 5 + C) rows ``cx, cy, w, h, conf, cls...`` (not modified; computed in its dtype):
    a list of (K, 6) tensors ``x1, y1, x2, y2, conf, class`` in keep order, ``None`` for an image without a candidate.  Equal
    scores go to the lower row (a stable sort).  ``margins``: a dict that collects the smallest distances of the discrete
    decisions (``conf``, ``iou``, ``score``)."""
    pred = prediction.clone()
    xy, wh = pred[..., :2].clone(), pred[..., 2:4].clone()
    pred[..., 0:2], pred[..., 2:4] = xy - wh / 2, xy + wh / 2
    out = []
    for img in pred:
        if margins is not None and img.shape[0]:
            margins["conf"] = min(margins.get("conf", np.inf), float((img[:, 4] - conf_thres).abs().min()))
        img = img[img[:, 4] >= conf_thres]
        if not img.size(0):
            out.append(None)
            continue
        score = img[:, 4] * img[:, 5:].max(1)[0]
        order = torch.sort(-score, stable=True)[1]
        if margins is not None and score.numel() > 1:
            s = torch.sort(score)[0]
            margins["score"] = min(margins.get("score", np.inf), float((s[1:] - s[:-1]).min()))
        img = img[order]
        det = torch.cat((img[:, :5], img[:, 5:].max(1, keepdim=True)[1].to(img.dtype)), 1)
        keep = []
        while det.size(0):
            iou = bbox_iou(det[0, :4].unsqueeze(0), det[:, :4])
            same = det[0, -1] == det[:, -1]
            if margins is not None and bool(same[1:].any()):
                margins["iou"] = min(margins.get("iou", np.inf), float((iou[1:][same[1:]] - nms_thres).abs().min()))
            invalid = (iou > nms_thres) & same
            w = det[invalid, 4:5]
            first = det[0].clone()
            first[:4] = (w * det[invalid, :4]).sum(0) / w.sum()
            keep.append(first)
            det = det[~invalid]
        out.append(torch.stack(keep))
    return out


def rescale(dets, frame_hw, img_size, person_class=0):
    """detector_yolov3.py:79-98: (K, 6) float32 detections -> (P, 4) float64 ``x, y, w, h`` in frame pixels of the rows of
    ``person_class``, every value taken to float64 first."""
    h, w = int(frame_hw[0]), int(frame_hw[1])
    pad_x = max(h - w, 0) * (img_size / max(h, w))
    pad_y = max(w - h, 0) * (img_size / max(h, w))
    unpad_h, unpad_w = img_size - pad_y, img_size - pad_x
    rows = []
    for x1, y1, x2, y2, _, c in (np.asarray(dets, dtype=np.float64) if dets is not None else ()):
        if int(c) == person_class:
            rows.append([((x1 - pad_x // 2) / unpad_w) * w, ((y1 - pad_y // 2) / unpad_h) * h,
                         ((x2 - x1) / unpad_w) * w, ((y2 - y1) / unpad_h) * h])
    return np.asarray(rows, dtype=np.float64).reshape(-1, 4)


def pad_to_square(img, value=127):
    """detector_utils.py:29-38 for one (H, W, 3) uint8 image with the level ``np.pad`` stores for 127.5."""
    h, w, _ = img.shape
    diff = abs(h - w)
    p1, p2 = diff // 2, diff - diff // 2
    pad = ((p1, p2), (0, 0), (0, 0)) if h <= w else ((0, 0), (p1, p2), (0, 0))
    return np.pad(img, pad, "constant", constant_values=value), pad


def letterbox64(frames, size):
    """``(mean, pad_mask)``: the exact float64 area mean (B, 3, size, size) in uint8 levels of the padded square of every
    (H, W, 3) frame, and the (size, size) mask of the output pixels that see padding only."""
    frames = np.asarray(frames)
    d = max(frames.shape[1:3])

    def cover(n_out):                                               # (n_out, d) integer coverage in units of 1 / n_out
        o = np.arange(n_out)[:, None] * d
        s = np.arange(d)[None, :] * n_out
        return np.clip(np.minimum(s + n_out, o + d) - np.maximum(s, o), 0, None).astype(np.float64)

    cw = cover(size)
    means = []
    for f in frames:
        sq, pad = pad_to_square(f)
        means.append(np.einsum("oy,yxc,px->cop", cw, sq.astype(np.float64), cw) / float(d * d))
    inside = np.zeros((d, d))
    (p1, p2), (q1, q2) = pad[0], pad[1]
    inside[p1:d - p2, q1:d - q2] = 1.0
    return np.stack(means), (cw @ inside @ cw.T) == 0


def levels(mean):
    """Round half to even, as ``cv2.resize`` saturates a float mean to uint8."""
    return np.rint(mean)
