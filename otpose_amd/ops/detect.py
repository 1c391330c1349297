"""The person detector's passes (csrc/detect.hip; the reference's object_detector/YOLOv3)."""
from __future__ import annotations

import ctypes

import torch

from .. import hip
from .base import View, check_f32, require_gpu, _launch, _slice, _vp


def letterbox(frames_u8, size, out=None):
    """uint8 RGB frames (B, H, W, 3) -> the detector's input (B, 3, size, size) float32 (``preprocess_img_for_yolo``,
    detector_utils.py:12-38): pad to a square with 127, area-average to ``size``, round to a uint8 level, / 255 - one kernel.
    Raises ``ValueError`` for ``max(H, W) < size``: there INTER_AREA is no area average any more."""
    require_gpu(frames_u8)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise TypeError("frames_u8 must be a (B, H, W, 3) uint8 tensor")
    b, h, w, _ = frames_u8.shape
    size = int(size)
    if b < 1 or size < 1 or max(h, w) < size:
        raise ValueError(f"letterbox shrinks: a {h} x {w} frame cannot fill a {size} x {size} input")
    frames_u8 = frames_u8.contiguous()
    if out is None:
        out = torch.empty((b, 3, size, size), dtype=torch.float32, device=frames_u8.device)
    elif out.shape != (b, 3, size, size) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 (B, 3, size, size) tensor")
    _launch(hip.lib().otp_letterbox_u8, "otp_letterbox_u8", (hip.ptr(frames_u8), hip.ptr(out), b, h, w, size), frames_u8)
    return out


def leaky_pass_args(inp: View, out: View, shortcut: View = None, leaky=True, up=1):
    n, _, h, w = inp.t.shape
    assert out.C == inp.C and out.t.shape[0] == n and tuple(out.t.shape[2:]) == (h * up, w * up)
    assert shortcut is None or (shortcut.C == inp.C and shortcut.t.shape[0] == n and tuple(shortcut.t.shape[2:]) == (h, w))
    assert out.t.data_ptr() != inp.t.data_ptr()
    return (_vp(inp), _vp(shortcut), _vp(out), n, inp.C, h, w, int(leaky), int(up), inp.ctot, inp.coff, *_slice(shortcut),
            out.ctot, out.coff)


def leaky_pass(inp: View, out: View, shortcut: View = None, leaky=True, up=1, stream=None):
    """out = up( leaky_0.1(inp) + shortcut ) on channel-slice views: the pass behind a Darknet conv (``leaky``), fused with a
    following ``[shortcut]`` and / or nearest 2x ``[upsample]``; with ``leaky=False`` a plain add / upsample / slice copy."""
    _launch(hip.lib().otp_leaky_pass, "otp_leaky_pass", leaky_pass_args(inp, out, shortcut, leaky, up), inp.t, stream)
    return out


def yolo_decode_args(head, pred, anchors, num_classes, img_size, row_off):
    b, ch, g, g2 = head.shape
    a = len(anchors)
    assert g == g2 and ch == a * (5 + num_classes) and pred.shape[0] == b and pred.shape[2] == 5 + num_classes
    flat = (ctypes.c_double * (2 * a))(*[float(v) for wh in anchors for v in wh])
    return (hip.ptr(head), hip.ptr(pred), flat, b, a, num_classes, g, int(img_size), pred.shape[1], int(row_off)), flat


def yolo_decode(head, anchors, num_classes, img_size, pred=None, row_off=0):
    """Eval output of one ``[yolo]`` layer (models.py:123-165): ``head`` (B, A (5 + C), G, G) -> rows ``row_off ..`` of ``pred``
    (B, N, 5 + C) in the order (anchor, gy, gx), each ``(cx, cy, w, h, conf, cls...)`` in input pixels.  ``anchors``: A pairs
    (w, h) in input pixels.  A fresh (B, A G G, 5 + C) tensor when ``pred`` is None."""
    require_gpu(head, pred)
    check_f32(head, pred)
    if head.dim() != 4 or head.shape[2] != head.shape[3] or head.shape[1] != len(anchors) * (5 + num_classes):
        raise ValueError(f"head must be (B, {len(anchors)} * (5 + {num_classes}), G, G), got {tuple(head.shape)}")
    head = head.contiguous()
    rows = len(anchors) * head.shape[2] * head.shape[3]
    if pred is None:
        pred = torch.empty((head.shape[0], rows, 5 + num_classes), dtype=torch.float32, device=head.device)
    if (pred.dim() != 3 or pred.shape[0] != head.shape[0] or pred.shape[2] != 5 + num_classes or not pred.is_contiguous()
            or row_off < 0 or row_off + rows > pred.shape[1]):
        raise ValueError("pred must be a contiguous (B, N, 5 + C) tensor with room for the layer's rows at row_off")
    args, _keep = yolo_decode_args(head, pred, anchors, num_classes, img_size, row_off)
    _launch(hip.lib().otp_yolo_decode, "otp_yolo_decode", args, head)
    return pred


def frame_rescale(frame_hw, img_size):
    """``(pad_x // 2, pad_y // 2, unpad_w, unpad_h, w, h)`` of a frame, as detector_yolov3.py:79-83 evaluates them (Python
    floats); ``frame_hw=None`` gives the identity (boxes stay in input pixels)."""
    if frame_hw is None:
        return 0.0, 0.0, 1.0, 1.0, 1.0, 1.0
    h, w = int(frame_hw[0]), int(frame_hw[1])
    pad_x = max(h - w, 0) * (img_size / max(h, w))
    pad_y = max(w - h, 0) * (img_size / max(h, w))
    unpad_h = img_size - pad_y
    unpad_w = img_size - pad_x
    return float(pad_x // 2), float(pad_y // 2), float(unpad_w), float(unpad_h), float(w), float(h)


def box_nms_merge(pred, conf_thres=0.4, nms_thres=0.4, frame_hw=None, img_size=416, person_class=0, workspace=None):
    """Confidence filter, the reference's merging NMS (detector_utils.py:253-291) and its rescale to frame pixels
    (detector_yolov3.py:79-98) for every image of ``pred`` (B, N, 5 + C) float32 rows ``(cx, cy, w, h, conf, cls...)``; one
    launch, one workgroup per image, no limit on the number of candidates.  ``pred`` is not modified.  Returns device
    tensors ``(counts (B,) int32, dets (B, N, 6) float32, person_counts (B,) int32, person_boxes (B, N, 4) float64,
    person_scores (B, N) float32)``: ``dets`` rows ``(x1, y1, x2, y2, conf, class)`` in keep order, the ``person_*`` outputs the
    kept rows of ``person_class`` as ``x, y, w, h`` in pixels of a ``frame_hw`` = (H, W) frame.  Rows past a count are zero."""
    require_gpu(pred)
    check_f32(pred)
    if pred.dim() != 3 or pred.shape[2] < 6 or pred.shape[0] < 1 or pred.shape[1] < 1:
        raise ValueError(f"pred must be (B, N, 5 + C) with C >= 1, got {tuple(pred.shape)}")
    pred = pred.contiguous()
    b, n, k = pred.shape
    dev = pred.device
    need = hip.lib().otp_box_nms_merge_workspace(b, n)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(b, dtype=torch.int32, device=dev)
    dets = torch.empty((b, n, 6), dtype=torch.float32, device=dev)
    pcounts = torch.empty(b, dtype=torch.int32, device=dev)
    pboxes = torch.empty((b, n, 4), dtype=torch.float64, device=dev)
    pscores = torch.empty((b, n), dtype=torch.float32, device=dev)
    _launch(hip.lib().otp_box_nms_merge, "otp_box_nms_merge",
            (hip.ptr(pred), b, n, k - 5, float(conf_thres), float(nms_thres), int(person_class),
             *frame_rescale(frame_hw, img_size), n, hip.ptr(workspace), workspace.numel() * workspace.element_size(),
             hip.ptr(counts), hip.ptr(dets), hip.ptr(pcounts), hip.ptr(pboxes), hip.ptr(pscores)), pred)
    return counts, dets, pcounts, pboxes, pscores
